"""GPU probe: the per-context fixed-effect GxC tests of many phenotypes in one pass (scan_interaction_contexts_many,
DESIGN.md section 14) at config 3, the shape of tools/bench_contexts.py -- 20 000 cells, 100 donors, 50 contexts, general
genotypes, the model of run_interaction (mode C) -- with 64 phenotypes of one cohort, fast=True, one step of 4 096 variants
after a warm-up.  In one process, on one build:

    (a) the many call over all phenotypes
    (b) one call of CellRegMap.scan_interaction_contexts per phenotype (the existing entry, which this feature leaves as it
        is: the yardstick)

    python tools/bench_contexts_many.py
        --phenotypes 64  --variants 4096
        --joint          scan_interaction_contexts_joint_many against scan_interaction_contexts_joint
        --singles N      time only the first N single calls and scale (0: skip (b), e.g. under a profiler)
        --out profiles/context_many_cfg3.json     where the result goes (also printed as one JSON line)

The phenotypes are drawn with the three drives of tests/context_lrt_cases.py (contexts, kinship, both), so their nulls
fall on several grid points; the number of distinct rho* and the timed Khatri-Rao contractions of (a) and (b) -- counts,
time, flops from the context's kernel timer -- are part of the record.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cellregmap_amd as pkg  # noqa: E402
from cellregmap_amd import CellRegMap, GenotypePanel, _engine, _lib, get_L_values  # noqa: E402
from cellregmap_amd.synth import make_cohort  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--phenotypes", type=int, default=64)
ap.add_argument("--variants", type=int, default=4096)
ap.add_argument("--joint", action="store_true")
ap.add_argument("--singles", type=int, default=-1)
ap.add_argument("--out", default=os.path.join("profiles", "context_many_cfg3.json"))
args = ap.parse_args()
P = args.phenotypes
singles = P if args.singles < 0 else min(args.singles, P)

c = make_cohort(100, 200, 50, 16, seed=20)
G = make_cohort(100, 200, 50, args.variants, seed=1000, with_phenotype=False).G
G = G + 0.05 * np.random.default_rng(0).normal(size=G.shape)      # general genotypes
n, k = c.E.shape
DRIVE = ((4.0, 0.0), (0.0, 3.0), (2.0, 1.0))                      # contexts, kinship, both
Y = np.empty((n, P))
for i in range(P):
    rng = np.random.default_rng(100 + i)
    a, b = DRIVE[i % 3]
    Y[:, i] = a * (c.E @ rng.normal(size=k)) / np.sqrt(k) + rng.normal(size=n) + b * (c.hK @ rng.normal(size=c.hK.shape[1]))
t = time.time()
Ls = get_L_values(c.hK, c.E)
first = CellRegMap(y=Y[:, 0], E=c.E, W=c.W, E1=c.E, Ls=Ls)
crms = [first] + [CellRegMap(y=Y[:, i], E=c.E, W=c.W, E1=c.E, Ls=Ls, background=first._bg) for i in range(1, P)]
ctor = time.time() - t
panel = GenotypePanel(G, groups=None)
lib, ctx = _lib.load(), _engine._context(0)
many = pkg.scan_interaction_contexts_joint_many if args.joint else pkg.scan_interaction_contexts_many


def single(obj):
    return (obj.scan_interaction_contexts_joint if args.joint else obj.scan_interaction_contexts)(panel, fast=True)


def timed(run):
    _lib.check(lib.crm_kernel_timer_reset(ctx))
    t0 = time.time()
    result = run()
    wall = time.time() - t0
    ms, launches, flops = ctypes.c_double(), ctypes.c_long(), ctypes.c_double()
    _lib.check(lib.crm_kernel_timer_read(ctx, ctypes.byref(ms), ctypes.byref(launches), ctypes.byref(flops), None))
    _lib.check(lib.crm_kernel_timer_stop(ctx))
    return result, {"wall_s": round(wall, 4), "contraction_ms": round(ms.value, 2), "contraction_launches": launches.value,
                    "contraction_tflops": round(flops.value / (ms.value * 1e-3) / 1e12, 2) if ms.value > 0 else None}


many(crms, panel, fast=True)                                       # warm-up: binds the context genes, every shape of (a)
if singles:
    single(crms[0])                                                # ... and of (b)
(pv, info), rec_many = timed(lambda: many(crms, panel, fast=True))
rho = [float(r) for r in info["rho1"]]
rec_single = None
if singles:
    _, rec_single = timed(lambda: [single(obj) for obj in crms[:singles]])
    rec_single["calls_timed"] = singles
    rec_single["wall_s_all_phenotypes"] = round(rec_single["wall_s"] * P / singles, 4)
out = {
    "shape": {"cells": int(n), "contexts": int(k), "variants": args.variants, "phenotypes": P,
              "ranks": [first._bg.rank(i) for i in range(11)],
              "covariate_basis_columns": int(np.linalg.matrix_rank(np.column_stack([c.W, c.E])))},
    "call": "joint" if args.joint else "per-context", "fast": True, "constructors_s": round(ctor, 3),
    "distinct_rho": len(set(rho)), "phenotypes_per_rho": {"%.1f" % r: rho.count(r) for r in sorted(set(rho))},
    "many": rec_many, "singles": rec_single,
    "speedup": round(rec_single["wall_s_all_phenotypes"] / rec_many["wall_s"], 2) if rec_single else None,
    "tests_per_s_many": round(P * args.variants * (1 if args.joint else k) / rec_many["wall_s"], 1),
    "status_ok": int(np.sum(info["status"] == 0)), "tests": int(info["status"].size), "min_p": float(np.min(pv)),
}
line = json.dumps(out, sort_keys=True)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
