"""GPU probe: multi-phenotype association scans (scan_association_many) against a loop of single-phenotype scans.

Cohort of tools/bench_association.py: 100 donors x 200 cells, 50 contexts bound to the fixed effects by
run_association's positional swap, W = 1 as the background's contexts, hK (mode B).  Cases:
  (a) G phenotypes x 4 096 variants of one panel
  (b) G phenotypes x 1 024-variant overlapping cis windows of a 16 384-variant panel
  (c) the same work as a loop of scan_association(_fast) calls in this process (the baseline)
for the fast path (G = 64) and the full refit (G = 16, a quarter of the variants: its per-variant fits dominate).
Prints one JSON line per (path, case) with variant-tests/s.

    python tools/bench_association_many.py [--only fast|full] [--case a|b|ab] [--reps R]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cellregmap_amd import CellRegMap, GenotypePanel, scan_association_many  # noqa: E402
from cellregmap_amd.synth import make_cohort  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("fast", "full"), default=None)
    ap.add_argument("--case", default="ab")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()

    c = make_cohort(100, 200, 50, 16, seed=20)
    n = c.y.size
    rng = np.random.default_rng(0)
    Ymax = np.stack([c.y] + [0.7 * c.y + rng.normal(size=n) for _ in range(63)], axis=1)
    t = time.time()
    first = CellRegMap(Ymax[:, 0], c.W, c.E, hK=c.hK)   # the wrapper's positional binding: E <- W, W <- E
    crms_all = [first] + [CellRegMap(Ymax[:, i], c.W, c.E, hK=c.hK, background=first._bg) for i in range(1, 64)]
    ctor = time.time() - t
    big = make_cohort(100, 200, 50, 16384, seed=1001, with_phenotype=False).G
    big = big + 0.05 * np.random.default_rng(1).normal(size=big.shape)   # general genotypes: dense panels
    panel_big = GenotypePanel(big, groups=None)
    print(json.dumps({"setup": "cohort", "cells": n, "covariates": 50, "ctor_s": round(ctor, 2)}), flush=True)

    for path in ("fast", "full"):
        if args.only and path != args.only:
            continue
        fast = path == "fast"
        ng = 64 if fast else 16
        nv = 4096 if fast else 1024
        win = 1024 if fast else 256
        crms = crms_all[:ng]
        panel_a = GenotypePanel(big[:, :nv], groups=None)
        p_b = 16 * nv // 4 if not fast else 16384
        panel_b = panel_big if fast else GenotypePanel(big[:, :p_b], groups=None)
        starts = np.linspace(0, p_b - win, ng).astype(int)
        cis = [(int(s), int(s) + win) for s in starts]
        single = (lambda crm: crm.scan_association_fast) if fast else (lambda crm: crm.scan_association)
        # warm-up: bind every gene, build every kernel
        scan_association_many(crms, GenotypePanel(big[:, :256], groups=None), fast=fast)
        single(crms[0])(GenotypePanel(big[:, :256], groups=None), progress=False)
        if "a" in args.case:
            best = best_loop = np.inf
            for _ in range(args.reps):
                t = time.time()
                scan_association_many(crms, panel_a, fast=fast)
                best = min(best, time.time() - t)
                t = time.time()
                for crm in crms:
                    single(crm)(panel_a, progress=False)
                best_loop = min(best_loop, time.time() - t)
            tests = ng * nv
            print(json.dumps({"path": path, "case": "a", "genes": ng, "variants": nv, "tests": tests,
                              "many_s": round(best, 4), "loop_s": round(best_loop, 4),
                              "many_tests_per_s": round(tests / best), "loop_tests_per_s": round(tests / best_loop),
                              "ratio": round(best_loop / best, 2)}), flush=True)
        if "b" in args.case:
            windows = [GenotypePanel(big[:, a:b], groups=None) for a, b in cis]   # (the loop's uploads are not timed)
            best = best_loop = np.inf
            for _ in range(args.reps):
                t = time.time()
                scan_association_many(crms, panel_b, cis_index=cis, fast=fast)
                best = min(best, time.time() - t)
                t = time.time()
                for crm, w in zip(crms, windows):
                    single(crm)(w, progress=False)
                best_loop = min(best_loop, time.time() - t)
            tests = ng * win
            print(json.dumps({"path": path, "case": "b", "genes": ng, "panel_variants": p_b, "window": win, "tests": tests,
                              "many_s": round(best, 4), "loop_s": round(best_loop, 4),
                              "many_tests_per_s": round(tests / best), "loop_tests_per_s": round(tests / best_loop),
                              "ratio": round(best_loop / best, 2)}), flush=True)
            del windows


if __name__ == "__main__":
    main()
