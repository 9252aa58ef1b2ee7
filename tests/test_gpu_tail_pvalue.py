"""The exact tail p-value on the device (csrc/tail_pvalue.hip): the kernel against the recorded
truths, the scans with pvalue="exact" against the reference method, the prototype and each other."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import tail_pvalue_prototype as tp  # noqa: E402


def _hook(Q, lam):
    from cellregmap_amd import _engine, _lib

    lib = _lib.load()
    Q = _lib.f64(Q)
    lam = _lib.f64(lam)
    count, k = lam.shape
    p, logp, status = np.empty(count), np.empty(count), np.empty(count, np.int32)
    _lib.check(lib.crm_test_tail_pvalue(_engine._context(0), count, k, _lib.ptr(Q), _lib.ptr(lam), _lib.ptr(p),
                                        _lib.ptr(logp), _lib.ptr(status)))
    return p, logp, status


def _cohort(mode, seed_shift=0):
    from cellregmap_amd import get_L_values
    from cellregmap_amd.synth import make_cohort

    if mode == "C":
        c = make_cohort(6, 40, 4, 24, seed=4 + seed_shift)
    else:
        c = make_cohort(10, 20, 5, 24, seed=5 + seed_shift)
    kw = {}
    if mode == "B":
        kw["hK"] = c.hK
    elif mode == "C":
        kw["Ls"] = get_L_values(c.hK, c.E)
    return c, kw


def test_hook_matches_recorded_truths():
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "tail_pvalue_truth.json")))["cases"]
    for k in sorted({len(c["lam"]) for c in cases}):
        sel = [c for c in cases if len(c["lam"]) == k]
        lam = np.array([sorted(c["lam"]) for c in sel])
        p, logp, status = _hook([c["q"] for c in sel], lam)
        assert np.all(status == 0), (k, status)
        for c, pi, li in zip(sel, p, logp):
            if c["p"] < 1e-300:
                assert abs(li - c["logp"]) <= 1e-10 * abs(c["logp"]), (c, li)
            else:
                assert abs(pi / c["p"] - 1) <= 1e-10, (c, pi)


def test_hook_status_codes_and_filter():
    lam = np.array([[0.5, 1.0, 2.0], [0.5, 1.0, 2.0], [0.5, np.nan, 2.0], [-1.0, 0.0, 0.0], [1e-9, 0.5, 2.0],
                    [0.5, 1.0, 2.0]])
    Q = np.array([np.nan, 3.0, 3.0, 1.0, 3.0, 0.0])
    p, logp, status = _hook(Q, lam)
    assert list(status) == [2, 0, 2, 3, 0, 0]
    assert np.isnan(p[0]) and np.isnan(logp[0]) and np.isnan(p[2]) and np.isnan(p[3])
    pp, _, _ = _hook([3.0], [[0.0, 0.5, 2.0]])
    assert p[4] == pp[0]                  # the filter drops 1e-9 and 0 (<= mean / 1e5)
    assert p[5] == 1.0 and logp[5] == 0.0
    # the device stays usable after the bad inputs; far below the double range log p stays finite
    p2, lp2, s2 = _hook([3.0, 5000.0], [[0.5, 1.0, 2.0], [1.0, 2.0, 3.0]])
    assert list(s2) == [0, 0] and p2[0] == p[1] and p2[1] == 0.0
    ref = tp.tail_pvalue(5000.0, [1.0, 2.0, 3.0])[1]
    assert abs(lp2[1] - ref) <= 1e-10 * abs(ref)


@pytest.mark.parametrize("mode", ["A", "B", "C"])
def test_reference_keyword_is_the_default_bit_for_bit(mode):
    from cellregmap_amd import CellRegMap

    c, kw = _cohort(mode)
    crm = CellRegMap(c.y, c.E, W=c.W, **kw)
    pv0, info0 = crm.scan_interaction(c.G)
    pv1, info1 = crm.scan_interaction(c.G, pvalue="reference")
    assert np.array_equal(pv0, pv1) and set(info1) == {"rho1", "e2", "g2", "eps2"}
    for key in info0:
        assert np.array_equal(info0[key], info1[key])


@pytest.mark.parametrize("mode", ["A", "B", "C"])
def test_exact_agrees_with_converged_davies(mode):
    from cellregmap_amd import CellRegMap

    c, kw = _cohort(mode)
    crm = CellRegMap(c.y, c.E, W=c.W, **kw)
    ref, rinfo = crm.scan_interaction_info(c.G)
    pv, info, stats = crm.scan_interaction(c.G, pvalue="exact", return_stats=True)
    pv0, info0, stats0 = crm.scan_interaction(c.G, return_stats=True)
    for key in ("Q", "lambda", "F", "lml", "delta", "scale"):
        assert np.array_equal(stats[key], stats0[key])
    for key in ("rho1", "e2", "g2", "eps2"):
        assert np.array_equal(info[key], info0[key])
    assert np.all(info["pvalue_status"] == 0)
    assert np.array_equal(ref, pv0)
    ok = (rinfo["ifault"] == 0) & (ref != rinfo["liu_pval"])
    assert ok.sum() >= pv.size // 2
    assert np.all(np.abs(pv[ok] - ref[ok]) <= 2e-6), np.c_[pv, ref][ok]
    assert np.allclose(np.log(pv), info["log_pvalue"], rtol=1e-12, atol=1e-15)
    # the device's exact p is the prototype's on the same (Q, lambda)
    p_proto, lp_proto, st_proto = tp.tail_pvalues(stats["Q"], stats["lambda"])
    assert np.all(st_proto == 0)
    assert np.all(np.abs(pv / p_proto - 1) <= 1e-10)


def _planted(mode, strength):
    """A cohort whose first variants carry a strong GxC effect: y += strength * g o (E beta).  The planted variants vary
    within donors: a donor-constant g o E beta lies in the span of mode C's background K o EE', which absorbs it."""
    c, kw = _cohort(mode, seed_shift=100)
    rng = np.random.default_rng(7)
    G = c.G.copy()
    G[:, :8] += rng.normal(size=(G.shape[0], 8))
    beta = rng.normal(size=c.E.shape[1])
    y = c.y.copy()
    for j in range(8):
        y = y + strength * (G[:, j] - G[:, j].mean()) * (c.E @ beta) / (j + 1)
    return c, kw, y, G


@pytest.mark.parametrize("mode", ["A", "B", "C"])
def test_planted_signals_beyond_davies(mode):
    from cellregmap_amd import CellRegMap

    c, kw, y, G = _planted(mode, 3.0)
    crm = CellRegMap(y, c.E, W=c.W, **kw)
    ref, rinfo = crm.scan_interaction_info(G)
    pv, info, stats = crm.scan_interaction(G, pvalue="exact", return_stats=True)
    liu = (ref == rinfo["liu_pval"]) | (rinfo["ifault"] != 0)
    assert liu.sum() >= 1, (ref, rinfo["ifault"])
    assert np.all(info["pvalue_status"] == 0)
    p_proto, lp_proto, st_proto = tp.tail_pvalues(stats["Q"], stats["lambda"])
    assert np.all(st_proto == 0)
    deep = lp_proto < np.log(1e-300)
    assert np.all(np.abs(info["log_pvalue"] - lp_proto) <= 1e-10 * np.abs(lp_proto))
    assert np.all(deep | (np.abs(pv / p_proto - 1) <= 1e-10))
    assert np.all(np.isfinite(info["log_pvalue"]))


@pytest.mark.parametrize("cis", [False, True])
def test_many_phenotypes_and_permutations_equal_single_scans(cis):
    from cellregmap_amd import CellRegMap, scan_interaction_many

    c, kw, y, G = _planted("B", 1.0)
    ys = [y, c.y, y[::-1].copy()]
    first = CellRegMap(ys[0], c.E, W=c.W, **kw)
    crms = [first] + [CellRegMap(v, c.E, W=c.W, background=first._bg, **kw) for v in ys[1:]]
    windows = [(0, 10), (5, 20), np.array([3, 1, 22, 7])] if cis else None
    pv, info = scan_interaction_many(crms, G, cis_index=windows, pvalue="exact")
    rpv, rinfo = scan_interaction_many(crms, G, cis_index=windows)
    for i, crm in enumerate(crms):
        assert np.array_equal(np.asarray(info["rho1"][i]), np.asarray(rinfo["rho1"][i]))
        if not cis:
            spv, sinfo = crm.scan_interaction(G, pvalue="exact")
            assert np.array_equal(pv[i], spv)
            for key in ("log_pvalue", "pvalue_status", "rho1"):
                assert np.array_equal(info[key][i], sinfo[key]), key
            continue
        # a window is scanned as a sub-range of the panel, with other launch shapes than a panel of its own: the null
        # fits agree to the reference's optimiser tolerance (tests/test_gpu_interaction.py), Q to ~1e-6 of its value
        Gi = G[:, windows[i][0]:windows[i][1]] if isinstance(windows[i], tuple) else G[:, windows[i]]
        spv, sinfo = crm.scan_interaction(Gi, pvalue="exact")
        lp, slp = info["log_pvalue"][i], sinfo["log_pvalue"]
        assert np.all(np.abs(lp - slp) <= 1e-5 * np.maximum(1.0, np.abs(slp))), np.c_[lp, slp]
        assert np.array_equal(info["pvalue_status"][i], sinfo["pvalue_status"])
    if cis:
        return
    rng = np.random.default_rng(3)
    perms = [rng.permutation(y.size) for _ in range(3)]
    ppv, pinfo = first.scan_interaction_permutations(G, idx_E_list=perms, pvalue="exact")
    for b, perm in enumerate(perms):
        spv, sinfo = first.scan_interaction(G, idx_E=perm, pvalue="exact")
        assert np.array_equal(ppv[b], spv)
        assert np.array_equal(pinfo["log_pvalue"][b], sinfo["log_pvalue"])
        assert np.array_equal(pinfo["pvalue_status"][b], sinfo["pvalue_status"])
    rpv, _ = first.scan_interaction_permutations(G, idx_E_list=perms)
    assert not np.array_equal(rpv, ppv)


def test_streamed_chunks_and_run_interaction(monkeypatch):
    import cellregmap_amd as pkg
    from cellregmap_amd import CellRegMap

    c, kw, y, G = _planted("A", 1.0)
    crm = CellRegMap(y, c.E, W=c.W, **kw)
    pv, info = crm.scan_interaction(G, pvalue="exact")
    monkeypatch.setenv("CELLREGMAP_AMD_STREAM_CHUNK", "8")
    spv, sinfo = crm.scan_interaction(G, pvalue="exact")
    assert np.allclose(spv, pv, rtol=1e-9, atol=0) and np.array_equal(sinfo["pvalue_status"], info["pvalue_status"])
    assert sinfo["log_pvalue"].shape == pv.shape
    # (a CellRegMap of their own: the same numbers to rounding, as tests/test_gpu_interaction.py holds run_interaction_many)
    rpv, rinfo = pkg.run_interaction(y, c.E, G, W=c.W, pvalue="exact")
    assert np.allclose(rpv, pv, rtol=1e-10, atol=0)
    assert np.allclose(rinfo["log_pvalue"], info["log_pvalue"], rtol=1e-10, atol=1e-14)
    Y = np.column_stack([y, c.y])
    mpv, minfo = pkg.run_interaction_many(Y, c.E, G, W=c.W, pvalue="exact")
    assert np.allclose(mpv[0], pv, rtol=1e-10, atol=0) and minfo["log_pvalue"].shape == (2, G.shape[1])
    assert np.all(minfo["pvalue_status"] == 0)
    with pytest.raises(ValueError):
        crm.scan_interaction(G, pvalue="liu")
    with pytest.raises(ValueError):
        crm.scan_interaction_permutations(G, idx_E_list=[None], pvalue="Exact")
    with pytest.raises(ValueError):
        pkg.scan_interaction_many([crm], G, pvalue=None)


def test_nan_statistic_reports_a_status_without_faulting():
    """A NaN Q through the scan's own kernels is not reachable from valid inputs: the hook takes it, then a scan runs."""
    from cellregmap_amd import CellRegMap

    p, logp, status = _hook([np.nan, np.inf, 1.0], [[1.0, 2.0]] * 3)
    assert list(status) == [2, 2, 0] and np.isnan(p[:2]).all()
    c, kw = _cohort("A")
    pv, info = CellRegMap(c.y, c.E, W=c.W, **kw).scan_interaction(c.G, pvalue="exact")
    assert np.all(info["pvalue_status"] == 0) and np.all(np.isfinite(pv))
