"""GPU probe: batched effect sizes (estimate_betas_many) against the per-SNP path (estimate_betas) in one process.

Config 3 (100 donors x 200 cells, 50 contexts, hK -> Hadamard halves, W = 1): P phenotypes x V lead variants (default
64 x 16 = 1 024 pairs) through the batched route, then estimate_betas on the first few of those pairs.  Prints one JSON
line: pairs/s of both, the speed-up, and the wall split of the batched call (the L-only background, which is built once
and cached, and the warm call; the per-kernel split comes from a rocprofv3 --kernel-trace --stats run of this script).

    python tools/bench_effects_many.py [--phenotypes 64] [--variants 16] [--single 4] [--reps 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cellregmap_amd import estimate_betas, estimate_betas_many  # noqa: E402
from cellregmap_amd.synth import make_config  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phenotypes", type=int, default=64)
    ap.add_argument("--variants", type=int, default=16)
    ap.add_argument("--single", type=int, default=4)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()

    c = make_config("cfg3", n_variants=args.variants)
    n = c.y.size
    rng = np.random.default_rng(0)
    Y = np.stack([c.y] + [0.7 * c.y + rng.normal(size=n) for _ in range(args.phenotypes - 1)], axis=1)
    maf = np.clip(np.minimum(c.G.mean(0) / 2, 1 - c.G.mean(0) / 2), 0.05, 0.5)
    pairs = np.stack(np.meshgrid(np.arange(args.phenotypes), np.arange(args.variants), indexing="ij"),
                     axis=-1).reshape(-1, 2)

    t = time.time()
    bg, bgxe, info = estimate_betas_many(Y, c.W, c.E, c.G, maf=maf, hK=c.hK, pairs=pairs, return_info=True)
    first = time.time() - t
    warm = []
    for _ in range(args.reps):
        t = time.time()
        estimate_betas_many(Y, c.W, c.E, c.G, maf=maf, hK=c.hK, pairs=pairs)
        warm.append(time.time() - t)
    routed = int(np.sum(info["route"] == "woodbury"))

    single = []
    gap = 0.0
    for t_, (i, v) in enumerate(pairs[:args.single]):
        t = time.time()
        sbg, sgxe = estimate_betas(Y[:, i], c.W, c.E, c.G[:, [v]], maf=maf[[v]], hK=c.hK)
        single.append(time.time() - t)
        gap = max(gap, abs(sbg[0] - bg[t_]) / max(abs(sbg[0]), 1e-300),
                  np.max(np.abs(sgxe[0, :, 0] - bgxe[0, :, t_])) / max(np.max(np.abs(sgxe)), 1e-300))
    many_rate = len(pairs) / min(warm)
    single_rate = len(single) / sum(single)
    print(json.dumps({
        "config": "cfg3", "cells": n, "k0": c.E.shape[1], "pairs": len(pairs), "routed": routed,
        "many_first_call_s": round(first, 3), "many_warm_s": [round(w, 3) for w in warm],
        "many_pairs_per_s": round(many_rate, 2),
        "single_s_per_pair": [round(s, 3) for s in single], "single_pairs_per_s": round(single_rate, 3),
        "speedup": round(many_rate / single_rate, 1),
        "max_rel_gap_vs_estimate_betas": float(gap),
    }))


if __name__ == "__main__":
    main()
