"""GPU probe: what pvalue="exact" (csrc/tail_pvalue.hip) adds to an interaction scan.

Scan leg (default): one warm CellRegMap.scan_interaction of a --variants panel of a BASELINE config, pvalue="reference"
and "exact" alternated --reps times on the same panel, on two panels: the cohort's own (null) variants, and "hits" --
every column the planted GxC variant plus a little noise, against a phenotype that carries its effect, so that every
variant's p-value is far below Davies' reach.  Prints one JSON line per panel: the median and minimum wall time of
either method, the added share, and how many p-values the reference left to modified Liu.

Kernel leg (--kernel-only K): the tail kernel alone through crm_test_tail_pvalue on --variants (Q, lambda) pairs of K
weights each, deep in the tail; run it under rocprofv3 --kernel-trace --stats for the kernel's own time.

    python tools/bench_tail_pvalue.py [--config cfg3] [--mode C|B] [--variants 4096] [--reps 5]
    python tools/bench_tail_pvalue.py --kernel-only 20 [--variants 4096]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (one HIP runtime: torch's, as bench.py loads it)

from cellregmap_amd import CellRegMap, GenotypePanel, _engine, _lib, get_L_values  # noqa: E402
from cellregmap_amd.synth import make_config  # noqa: E402


def kernel_only(k, count, reps):
    lib = _lib.load()
    rng = np.random.default_rng(1)
    lam = np.sort(np.exp(rng.uniform(0, np.log(50.0), size=(count, k))), axis=1)
    Q = lam.sum(1) * rng.uniform(3.0, 40.0, size=count)
    p, lp, st = np.empty(count), np.empty(count), np.empty(count, np.int32)
    ctx = _engine._context(0)
    times = []
    for _ in range(reps):
        t = time.time()
        _lib.check(lib.crm_test_tail_pvalue(ctx, count, k, _lib.ptr(Q), _lib.ptr(lam), _lib.ptr(p), _lib.ptr(lp), _lib.ptr(st)))
        times.append(time.time() - t)
    print(json.dumps({"leg": "kernel", "k": k, "variants": count, "hook_wall_s_min": round(min(times), 5),
                      "converged": int(np.sum(st == 0)), "log10_p_range": [round(float(lp.min() / np.log(10)), 1),
                                                                          round(float(lp.max() / np.log(10)), 1)]}))


def timed(crm, panel, pvalue, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.time()
        pv, info = crm.scan_interaction(panel, pvalue=pvalue, progress=False)
        out.append(time.time() - t)
    return out, pv, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--mode", default="C", choices=["C", "B"])
    ap.add_argument("--variants", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-only", type=int, default=0)
    args = ap.parse_args()
    if args.kernel_only:
        kernel_only(args.kernel_only, args.variants, args.reps)
        return

    c = make_config(args.config, n_variants=args.variants)
    kw = {"Ls": get_L_values(c.hK, c.E)} if args.mode == "C" else {"hK": c.hK}
    rng = np.random.default_rng(2)
    g0 = c.G[:, 0] - c.G[:, 0].mean()
    beta = rng.normal(size=c.E.shape[1])
    y_hit = c.y + 0.5 * g0 * (c.E @ beta) / np.std(g0 * (c.E @ beta))
    G_hit = g0[:, None] + 0.05 * rng.normal(size=c.G.shape)
    for name, y, G in (("null", c.y, c.G), ("hits", y_hit, G_hit)):
        crm = CellRegMap(y, c.E, W=c.W, **kw)
        panel = GenotypePanel(G, groups=None)      # dense, as bench.py's headline steps
        crm.scan_interaction(panel, pvalue="exact", progress=False)      # warm-up of every shape and of the tail kernel
        crm.scan_interaction(panel, progress=False)
        ref, exa = [], []
        for _ in range(args.reps):       # alternated, so that drifts of the machine fall on both
            t, pv_ref, _ = timed(crm, panel, "reference", 1)
            ref += t
            t, pv_exact, info = timed(crm, panel, "exact", 1)
            exa += t
        _, rinfo = crm.scan_interaction_info(panel) if name == "hits" else (None, None)
        liu = int(np.sum((rinfo["ifault"] != 0) | (pv_ref == rinfo["liu_pval"]))) if rinfo is not None else None
        mr, me = float(np.median(ref)), float(np.median(exa))
        print(json.dumps({
            "leg": "scan", "config": args.config, "mode": args.mode, "panel": name, "variants": G.shape[1],
            "cells": int(c.y.size), "k0": int(c.E.shape[1]), "groups": panel.n_groups,
            "reference_s": [round(x, 4) for x in ref], "exact_s": [round(x, 4) for x in exa],
            "reference_median_s": round(mr, 4), "exact_median_s": round(me, 4),
            "added_median_pct": round(100 * (me / mr - 1), 2), "added_min_pct": round(100 * (min(exa) / min(ref) - 1), 2),
            "status_converged": int(np.sum(info["pvalue_status"] == 0)),
            "log10_p_exact_min": round(float(np.min(info["log_pvalue"]) / np.log(10)), 1),
            "reference_liu_fallbacks": liu,
        }), flush=True)


if __name__ == "__main__":
    main()
