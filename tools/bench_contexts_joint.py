"""GPU probe: the joint fixed-effect GxC test (CellRegMap.scan_interaction_contexts_joint) at config 3
-- tools/bench_contexts.py's workload and protocol with the joint call: 20 000 cells, 100 donors, 50 contexts, general
genotypes, the model of run_interaction (mode C: E1 = E, L_i from hK and E).

    python tools/bench_contexts_joint.py               fast=True: 3 steps of 4096 variants after a warm-up
        --refit             fast=False (delta refitted per variant) instead
        --variants 4096     variants per step;  --steps 3
        --out profiles/context_joint_cfg3.json   where the result goes (also printed as one JSON line)

Per step: wall time around the call (it ends in a device synchronise).  From the context's kernel timer over the timed
steps: the time, launches and FP64 rate of the Khatri-Rao contraction Q0(rho*)'(g o C) alone -- what is left of a step is
the joint kernel, the plain-table launches (the pair table's among them), the rotations and the null fits.  Compare with
tools/bench_contexts.py run in the same session.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cellregmap_amd import CellRegMap, GenotypePanel, _engine, _lib, get_L_values  # noqa: E402
from cellregmap_amd.synth import make_cohort  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--refit", action="store_true")
ap.add_argument("--variants", type=int, default=4096)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=os.path.join("profiles", "context_joint_cfg3.json"))
args = ap.parse_args()

c = make_cohort(100, 200, 50, 16, seed=20)
G = make_cohort(100, 200, 50, args.variants, seed=1000, with_phenotype=False).G
G = G + 0.05 * np.random.default_rng(0).normal(size=G.shape)      # general genotypes
t = time.time()
crm = CellRegMap(y=c.y, E=c.E, W=c.W, E1=c.E, Ls=get_L_values(c.hK, c.E))
ctor = time.time() - t
ranks = [crm._bg.rank(i) for i in range(11)]
panel = GenotypePanel(G, groups=None)
lib, ctx = _lib.load(), _engine._context(0)
fast = not args.refit
for _ in range(args.warmup):
    crm.scan_interaction_contexts_joint(panel, fast=fast)          # (every shape of the timed window)
_lib.check(lib.crm_kernel_timer_reset(ctx))
walls = []
for _ in range(args.steps):
    t = time.time()
    pv, info = crm.scan_interaction_contexts_joint(panel, fast=fast, return_stats=True)
    walls.append(time.time() - t)
kr_ms, launches, flops = ctypes.c_double(), ctypes.c_long(), ctypes.c_double()
_lib.check(lib.crm_kernel_timer_read(ctx, ctypes.byref(kr_ms), ctypes.byref(launches), ctypes.byref(flops), None))
_lib.check(lib.crm_kernel_timer_stop(ctx))
k = c.E.shape[1]
best = min(walls)
out = {
    "shape": {"cells": int(c.y.size), "contexts": k, "variants_per_step": args.variants, "ranks": ranks,
              "covariate_basis_columns": int(np.linalg.matrix_rank(np.column_stack([c.W, c.E])))},
    "fast": fast, "steps": args.steps, "constructor_s": round(ctor, 3),
    "step_wall_s": [round(w, 4) for w in walls],
    "variants_per_s": round(args.variants / best, 1),
    "contraction": {"ms_per_step": round(kr_ms.value / args.steps, 2), "launches_per_step": launches.value / args.steps,
                    "tflops": round(flops.value / (kr_ms.value * 1e-3) / 1e12, 2) if kr_ms.value > 0 else None,
                    "share_of_step": round(kr_ms.value * 1e-3 / sum(walls), 3)},
    "rest_ms_per_step": round(1e3 * sum(walls) / args.steps - kr_ms.value / args.steps, 2),
    "rho1": float(info["rho1"][0]), "gene_null_delta": float(info["gene_null_delta"]),
    "status_ok": int(np.sum(info["status"] == 0)), "tests": int(info["status"].size), "min_p": float(pv.min()),
    "dof": sorted(int(d) for d in np.unique(info["dof"])), "dropped": int(info["dropped"].sum()),
}
line = json.dumps(out, sort_keys=True)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
