"""GPU probe: association LRT throughput at config 3 (run_association binds the 50 contexts to the
fixed effects and W to the background, mode B with hK).

    python tools/bench_association.py                       the scans of one phenotype, then the host-matrix runs
    python tools/bench_association.py --effects             ... each scan timed again with effects=True
        --cov 1            one covariate column (the contexts stay contexts) instead of the wrapper's 50
        --phenotypes 64    scan_association_many over that many phenotypes instead of one
        --skip-host        leave out the end-to-end runs from a host matrix of 32 768 SNPs
        --repeats 2        best of that many timed calls after the warm-up (default: one timed call)
"""
import argparse
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cellregmap_amd import CellRegMap, GenotypePanel, scan_association_many
from cellregmap_amd.synth import make_cohort

ap = argparse.ArgumentParser()
ap.add_argument("--effects", action="store_true")
ap.add_argument("--cov", type=int, default=50, choices=(1, 50))
ap.add_argument("--phenotypes", type=int, default=1)
ap.add_argument("--skip-host", action="store_true")
ap.add_argument("--repeats", type=int, default=1)
args = ap.parse_args()

c = make_cohort(100, 200, 50, 16, seed=20)
s = make_cohort(100, 200, 50, 4096, seed=1000, with_phenotype=False)
t = time.time()
if args.cov == 50:
    make = lambda y, **kw: CellRegMap(y, c.W, c.E, hK=c.hK, **kw)   # the wrapper's positional binding: E <- W, W <- E
else:
    make = lambda y, **kw: CellRegMap(y, c.E, W=c.W, hK=c.hK, **kw)
crm = make(c.y)
crm._bind_gene()
print("ctor", round(time.time() - t, 2), "s; ranks", [crm._bg.rank(i) for i in range(11)])
crms = [crm]
if args.phenotypes > 1:
    rng = np.random.default_rng(5)
    crms += [make(c.y + 0.5 * rng.normal(size=c.y.size), background=crm._bg) for _ in range(args.phenotypes - 1)]
panel = GenotypePanel(s.G, groups=None)


def timed(fn, fast, pan, **kw):
    """Best of ``--repeats`` wall times of one scan (after the caller's warm-up)."""
    best, out = None, None
    if len(crms) > 1 and kw.pop("effects", False):
        kw["return_stats"] = "effects"      # (scan_association_many takes the request there)
    for _ in range(args.repeats):
        t = time.time()
        out = fn(pan, **kw) if len(crms) == 1 else scan_association_many(crms, pan, fast=fast, **kw)
        dt = time.time() - t
        best = dt if best is None else min(best, dt)
    return best, out


nv_full = 1024 if len(crms) == 1 else 256      # (a full refit of many phenotypes runs its fits phenotype by phenotype)
for name, fn, fast, nv in (("fast", crm.scan_association_fast, True, 4096), ("full", crm.scan_association, False, nv_full)):
    pan = GenotypePanel(s.G[:, :nv], groups=None) if nv < 4096 else panel
    warm = GenotypePanel(s.G[:, :256], groups=None)
    timed(fn, fast, warm, progress=False)
    dt, out = timed(fn, fast, pan, progress=False)
    pv, info = out[0], out[1]
    tests = nv * len(crms)
    if len(crms) == 1:
        print(f"scan_association_{name} (c = {args.cov}): {nv} SNPs in {dt:.4f} s -> {nv/dt:.0f} SNPs/s; rho {info['rho1']}, "
              f"min p {pv.min():.3g}")
    else:
        print(f"scan_association_{name} (c = {args.cov}, {len(crms)} phenotypes): {nv} SNPs in {dt:.4f} s -> {tests/dt:.0f} tests/s; "
              f"rho {np.unique(info['rho1'])}, min p {np.min(pv):.3g}")
    if args.effects:
        timed(fn, fast, warm, progress=False, effects=True)
        de, out = timed(fn, fast, pan, progress=False, effects=True)
        st = out[2] if len(crms) == 1 else out[1]
        ok = int(np.sum(np.asarray(st["effect_status"]) == 0))
        print(f"scan_association_{name} with effects=True: {de:.4f} s -> {tests/de:.0f} tests/s; added {de - dt:+.4f} s "
              f"({100 * (de - dt) / dt:+.1f} %); {ok} of {tests} tests with status OK, "
              f"same p-values: {bool(np.array_equal(out[0], pv))}")

if not args.skip_host and len(crms) == 1:
    # end to end from a host matrix of 32 768 SNPs (5.2 GB): uploaded whole, then scanned -- against streamed in column chunks
    # beside the scan (the host's default, CELLREGMAP_AMD_STREAM_CHUNK)
    big = make_cohort(100, 200, 50, 32768, seed=1001, with_phenotype=False).G
    big = big + 0.05 * np.random.default_rng(0).normal(size=big.shape)      # general genotypes: every chunk stays dense
    for name, fn in (("fast", crm.scan_association_fast), ("full", crm.scan_association)):
        for chunk in ("0", "8192"):
            os.environ["CELLREGMAP_AMD_STREAM_CHUNK"] = chunk
            t = time.time(); pv, _ = fn(big, progress=False); dt = time.time() - t
            print(f"scan_association_{name} from the host matrix, {'streamed' if chunk != '0' else 'one panel'}: "
                  f"{big.shape[1]} SNPs in {dt:.3f} s -> {big.shape[1] / dt:.0f} SNPs/s end to end")
