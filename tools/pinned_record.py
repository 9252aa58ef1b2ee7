#!/usr/bin/env python3
"""Assemble profiles/pinned_effects_association_errors.json.

    CRM_PINNED_JSON=<dir>/pinned.json pytest tests/test_gpu_pinned_effects.py tests/test_gpu_pinned_association.py -m gpu
    python tools/pinned_record.py <dir>/pinned_effects.json <dir>/pinned_association.json \
        > profiles/pinned_effects_association_errors.json

    CRM_PINNED_JSON=<dir>/pinned.json pytest tests/test_gpu_pinned_null_model.py -m gpu
    python tools/pinned_record.py --null-model <dir>/pinned_null_model.json > profiles/pinned_null_model_errors.json

The GPU test files write their per-case errors beside the file $CRM_PINNED_JSON names; this merges them under
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


def null_model_cpu_section():
    """No GPU: every cohort of pinned_cases.NULL_MODEL with the float64 oracle's own Brent search in the device's place,
    and the injected slips."""
    own = {}
    for name in pc.NULL_MODEL:
        cs, sel, _, lim, shares, worst = cpu.null_model_oracle_shares(name)
        own[name] = {"cells": cs.n, "variants": [int(j) for j in sel], "trials": len(shares), "limit": _floats(lim),
                     "largest_shares": _floats(worst)}
    slips = [{"slip": s, "times_the_bound": None if f == float("inf") else float("%.4g" % f),
              "rejected_outright": f == float("inf")} for s, f in cpu.slip_report_null_model()]
    return {"the_oracles_own_search_through_the_same_checks": own, "injected_slips": slips}


def null_model_summary(cases):
    """Per bound the case with the largest share of it; the numbers of trials, of trials at a clamp and of ties."""
    worst = {}
    for case, rec in cases.items():
        for k, v in rec["shares"].items():
            if k not in worst or v["share"] > worst[k]["share"]:
                worst[k] = dict(v, case=case)
    return {"largest_share_per_bound": worst, "cases": len(cases), "trials": sum(r["trials"] for r in cases.values()),
            "trials_at_a_clamp": sum(r["at_a_clamp"] for r in cases.values()),
            "held_variants_with_a_tie": sum(r["ties"] for r in cases.values()),
            "nfev": [min(r["nfev"][0] for r in cases.values()), max(r["nfev"][1] for r in cases.values())]}


def main(paths):
    null_model = paths[:1] == ["--null-model"]
    cases = {}
    for p in paths[1:] if null_model else paths:
        with open(p) as fh:
            cases.update(json.load(fh))
    if null_model:
        out = {"cpu": null_model_cpu_section(), "device_cases": cases, "summary": null_model_summary(cases),
               "what": "tests/test_gpu_pinned_null_model.py on an MI355X, merged by tools/pinned_record.py --null-model: per case "
                       "the trial records of a real scan (crm_test_null_fit_probe, on = 2) of the held variants at every grid "
                       "point against the longdouble reference -- shares: the largest share of each bound and where (lml, "
                       "scale: |device - reference at the trial's delta| over the limit, 32 x oracle, floor cells x 2.2e-16, "
                       "ceiling 1e-11; short of L* / above L*: the trial's lml against the reference's own maximum, over "
                       "refit_allowance + limit |L*| and over limit |L*|; stop: |logit(delta) - x*| over stop_allowance; clamp "
                       "value / clamp delta: trials whose maximum sits at delta = 1 - 2^-52).  A share above 1 fails the test.  "
                       "cpu: the float64 oracle's own Brent search through the same checks on every cohort, and the injected "
                       "slips of tests/test_pinned_reference_cpu.py (no GPU)."}
        json.dump(out, sys.stdout, indent=1, sort_keys=True)
        sys.stdout.write("\n")
        return
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
