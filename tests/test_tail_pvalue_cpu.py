"""tools/tail_pvalue_prototype.py (the numpy statement of the exact tail p-value) against
independent truths recorded in tests/golden/tail_pvalue_truth.json (chi-square closed form, Ruben's series, Imhof's
integral, all in mpmath: tests/golden/make_tail_pvalue_golden.py), and the library's declarations of the method."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import tail_pvalue_prototype as tp  # noqa: E402

CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "tail_pvalue_truth.json")))["cases"]


def _rel_err(case, p, logp):
    if case["p"] < 1e-300:
        return abs(logp - case["logp"]) / abs(case["logp"])
    return abs(p / case["p"] - 1.0)


def test_fixture_covers_the_contract():
    ks = {len(c["lam"]) for c in CASES}
    assert {1, 2, 256} <= ks
    assert min(c["logp"] for c in CASES) < np.log(1e-300) and max(c["p"] for c in CASES) > 0.5
    assert {c["source"] for c in CASES} == {"chi2", "ruben", "imhof"}
    spread = max(max(c["lam"]) / min(c["lam"]) for c in CASES if c["source"] == "imhof")
    assert spread > 9e4
    # q just either side of E[Q] (the saddle point changes side of the pole there)
    near = [c["q"] / sum(c["lam"]) for c in CASES]
    assert any(0.99 < r < 1.0 for r in near) and any(1.0 < r < 1.01 for r in near)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_prototype_matches_truth(i):
    case = CASES[i]
    p, logp, status = tp.tail_pvalue(case["q"], case["lam"])
    assert status == tp.CONVERGED
    err = _rel_err(case, p, logp)
    assert err <= 1e-10, (case["source"], len(case["lam"]), case["q"], case["p"], p, err)
    if case["p"] >= 1e-300:
        assert abs(logp - case["logp"]) <= 1e-10 * max(1.0, abs(case["logp"]))


def test_filter_and_status_codes():
    # SKAT's filter: weights at or below mean(lam >= 0) / 1e5 are dropped -- the same distribution Davies integrates
    lam = np.array([-1e-3, 1e-9, 0.5, 2.0])
    assert np.array_equal(tp.kept_weights(lam), [0.5, 2.0])
    assert tp.tail_pvalue(3.0, lam)[:2] == tp.tail_pvalue(3.0, [0.5, 2.0])[:2]
    assert tp.tail_pvalue(np.nan, [1.0, 2.0])[2] == tp.NON_FINITE
    assert tp.tail_pvalue(1.0, [1.0, np.inf])[2] == tp.NON_FINITE
    assert tp.tail_pvalue(1.0, [-1.0, 0.0])[2] == tp.NO_WEIGHTS
    p, logp, status = tp.tail_pvalue(0.0, [1.0, 2.0])
    assert (p, logp, status) == (1.0, 0.0, tp.CONVERGED)
    # far beyond the double range of p: log p stays finite and is the one-term limit's to first order
    p, logp, status = tp.tail_pvalue(5000.0, [1.0, 2.0, 3.0])
    assert status == tp.CONVERGED and p == 0.0 and -5000.0 / 6 - 20 < logp < -5000.0 / 6


def test_library_declares_the_method():
    """The C-ABI carries the exact method (include/crm_hip.h) and its unit-test hook (include/crm_hip_test.h)."""
    from cellregmap_amd import _lib

    for name in ("crm_scan_interaction_tail", "crm_scan_interaction_multi_tail", "crm_scan_interaction_permuted_tail",
                 "crm_test_tail_pvalue"):
        assert name in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "crm_hip.h")).read()
    for i, name in enumerate(("CONVERGED", "NOT_BRACKETED", "NON_FINITE", "NO_WEIGHTS")):
        assert f"#define CRM_TAIL_{name} {i}" in header
        assert getattr(tp, name) == i


def test_bad_pvalue_keyword_raises_before_any_device_work():
    import cellregmap_amd as pkg
    from cellregmap_amd import _engine

    assert _engine._exact_pvalues("reference") is False and _engine._exact_pvalues("exact") is True
    for bad in ("Exact", "davies", None, 1):
        with pytest.raises(ValueError):
            _engine._exact_pvalues(bad)
    with pytest.raises(ValueError):
        pkg.run_interaction(np.zeros(4), np.ones((4, 1)), np.zeros((4, 1)), pvalue="liu")
