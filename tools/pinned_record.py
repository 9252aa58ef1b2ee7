#!/usr/bin/env python3
"""Assemble profiles/pinned_effects_association_errors.json.

    CRM_PINNED_JSON=<dir>/pinned.json pytest tests/test_gpu_pinned_effects.py tests/test_gpu_pinned_association.py -m gpu
    python tools/pinned_record.py <dir>/pinned_effects.json <dir>/pinned_association.json \
        > profiles/pinned_effects_association_errors.json

The two GPU test files write their per-case errors beside the file $CRM_PINNED_JSON names; this merges them under
``device_cases``, adds a ``summary`` (per quantity the worst device error, its limit and its share of it; the refitting
scan's largest shortfall and overshoot) and computes the ``cpu`` section, which needs no GPU: the float64 oracle against
the reference at its own optimum on every cohort of tests/pinned_cases.py, the oracle's Brent result against the refit
bound, and the injected slips of tests/test_pinned_reference_cpu.py.  The layout is that of
profiles/pinned_reference_errors.json.
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import pinned_cases as pc  # noqa: E402
import pinned_reference as pr  # noqa: E402
import test_pinned_reference_cpu as cpu  # noqa: E402


def _floats(d):
    return {k: float(v) for k, v in d.items()}


def cpu_section():
    own, brent = {}, {}
    for name in pc.EFFECTS:
        _, rows = cpu._effects_rows(name)
        own["effects, " + name] = _floats(pr.worst([pr.effects_errors(o, r) for _, (r, o) in rows]))
    for name in pc.ASSOCIATION:
        cs, (rho, delta, _, _), _, _, variants = cpu._assoc_rows(name)
        err = cpu._assoc_oracle_errors(name)
        own["association, " + name] = dict(_floats(err), rho=float(rho), delta=float(delta))
        lim = pr.limits(err, cs.n)["lml"]
        brent["association, " + name] = [
            {"variant": int(v["j"]), "delta_at_the_maximum": float(pr._logistic(v["x"])), "curvature": float(v["curvature"]),
             "short_of_L*": float(v["top"] - pr.LD(v["brent"])), "limit": lim * abs(float(v["top"])),
             "allowance": pr.refit_allowance(v["x"], v["curvature"])} for v in variants]
    slips = [{"slip": s, "times_the_limit": float("%.4g" % f), "passes_the_bound_the_suite_had_before": bool(b)}
             for s, f, b in cpu.slip_report_effects_association()]
    return {"float64_oracle_against_the_reference_at_its_own_optimum": own,
            "the_oracles_brent_result_against_the_refit_bound": brent, "injected_slips": slips}


def summary(cases):
    worst = {}
    for case, rec in cases.items():
        family = case.split(",")[0].split()[0]
        for k, v in rec["device"].items():
            share = v / rec["limit"][k]
            cur = worst.setdefault(family, {}).get(k)
            if cur is None or share > cur["share_of_the_limit"]:
                at = {"share_of_the_limit": share, "error": v, "limit": rec["limit"][k], "case": case}
            else:
                at = cur
            at["largest_error"] = max(v, cur["largest_error"] if cur else 0.0)
            worst[family][k] = at
    short = [(s, rec["refit"]["allowance"][j], rec["limit"]["lml"], case) for case, rec in cases.items() if "refit" in rec
             for j, s in rec["refit"]["short of L*"].items()]
    if short:
        s, a, l, case = max(short)
        worst["refit"] = {"variants": len(short), "largest_shortfall": s, "its_allowance": a, "case": case,
                          "smallest_shortfall": min(short)[0]}
    return worst


def main(paths):
    cases = {}
    for p in paths:
        with open(p) as fh:
            cases.update(json.load(fh))
    out = {"cpu": cpu_section(), "device_cases": cases, "summary": summary(cases),
           "what": "tests/test_gpu_pinned_effects.py and tests/test_gpu_pinned_association.py on an MI355X, merged by "
                   "tools/pinned_record.py: per case the largest error of the device and of the float64 oracle against the "
                   "longdouble reference at the device's own point ((rho1, v0, v1) for the effect sizes, (rho1, null delta) "
                   "for the association scans), and the limit asserted (32 x oracle, floor cells x 2.2e-16, ceiling 1e-11); "
                   "beta, u, beta_gxe and x relative to the largest magnitude of the reference vector, lml and scale "
                   "relative, lrs = 2 (alt - null) absolute over |null lml|; refit: alt_lml short of the reference's maximum "
                   "L* per variant and the allowance of the search's tolerance.  summary: per family and quantity the case "
                   "with the largest share of its limit.  cpu: tests/test_pinned_reference_cpu.py (no GPU)."}
    json.dump(out, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
