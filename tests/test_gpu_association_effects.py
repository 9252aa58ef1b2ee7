"""``effects=True`` of the association scans (``return_stats="effects"`` of ``scan_association_many``, whose parameter list
tests/test_association_many_cpu.py pins; cellregmap_amd/csrc/assoc_effects.hip) against the dense
longdouble generalised least squares of tests/assoc_effects_reference.py, evaluated at the delta the device returns -- a
pinned-point comparison, as tests/test_gpu_pinned.py holds Q and F.

Tolerance for beta, beta_se and alt_scale: max(8 e64, 1e-12) = 8 x 1.6e-12 = 1.28e-11 relative, with e64 the float64 oracle's
own worst gap to the same truth over these cases (measured on the CPU by tests/test_assoc_effects_prototype_cpu.py, which
also holds the kernel's algebra in numpy to this bound).  Every compared test has delta inside [1e-4, 1 - 1e-4]
(asserted), so the looser floor 1e-8 for planted tests outside that range is never used.  delta itself: fast, the returned
null_delta bit for bit; full refit, the oracle's ``LMM(y, [W, g], QS, restricted=False).fit()`` to rtol 1e-5, what
tests/test_gpu_association.py asks of the fitted components.  log_pvalue: mpmath at 40 digits at the lrs of the returned
alt_lml and null_lml, 1e-12 relative.

Cohorts, covariate widths and planted columns: tests/assoc_effects_reference.py.  Exactly the planted SPAN and BOUNDARY
columns may carry a status other than CRM_EFFECT_OK; every other test is compared, none is skipped on a tolerance.

Blocks: ``crm_set_block_variants`` rounds up to 128 variants, so the 41-variant panels are one block whatever is set and
a three-block scan needs at least 257 variants; ``test_three_blocks_and_a_ragged_tail`` scans 297 at 128 per block.

Worst gaps measured on an MI355X (relative; beta / beta_se / alt_scale over all cases): see DESIGN.md section 11.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import assoc_effects_reference as ar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, IN_SPAN = 0, 1
TINY = 2.2250738585072014e-308
EPS = 2.220446049250313e-16
KEYS = ("beta", "beta_se", "alt_delta", "alt_scale", "log_pvalue", "effect_status")


def _device(cs, y=None):
    from cellregmap_amd import CellRegMap

    return CellRegMap(cs.y if y is None else y, cs.E, W=cs.W, **cs.device_kw())


def _scan(obj, fast):
    return obj.scan_association_fast if fast else obj.scan_association


def _hold_log_pvalue(case, st, null_lml, sel):
    for j in sel:
        want = ar.mp_log_pvalue(st["alt_lml"][j], null_lml)
        got = float(st["log_pvalue"][j])
        assert abs(got - want) <= 1e-12 * abs(want), (case, j, got, float(want))


def _hold(case, cs, y, G, rho, null_delta, null_lml, st, fast, comp, oracle_delta=True):
    """beta, beta_se, alt_scale of the columns ``comp`` of ``G`` against the truth at the returned delta; delta itself."""
    delta = np.asarray(st["alt_delta"], float)
    assert np.all(st["effect_status"][comp] == OK), (case, st["effect_status"])
    if fast:
        assert np.all(delta == null_delta), (case, delta, null_delta)
    elif oracle_delta:
        want = np.array([ar.oracle_alt_delta(cs, rho, G[:, j], y) for j in comp])
        print("[effects] %s: delta against the oracle's fit, worst %.2e" % (case, np.abs(delta[comp] / want - 1).max()))
        assert np.all(np.abs(delta[comp] - want) <= ar.DELTA_RTOL * want), (case, delta[comp], want)
    assert np.all((delta[comp] >= ar.DELTA_RANGE[0]) & (delta[comp] <= ar.DELTA_RANGE[1])), (case, delta[comp])
    truth = ar.dense_truth(y, cs.W, G[:, comp], cs.gram(rho), delta[comp])
    got = np.array([st["beta"][comp], st["beta_se"][comp], st["alt_scale"][comp]])
    gap = ar.gaps(got, truth)
    print("[effects] %s: beta %.2e  beta_se %.2e  alt_scale %.2e  (tolerance %.2e; delta %.3g .. %.3g)"
          % (case, gap[0].max(), gap[1].max(), gap[2].max(), ar.TOLERANCE, delta[comp].min(), delta[comp].max()))
    assert np.all(gap <= ar.TOLERANCE), (case, gap.max(axis=1))
    _hold_log_pvalue(case, st, null_lml, comp)
    return gap


# ---- one phenotype: every cohort, mode and width, fast and full refit ----------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("name", list(ar.CASES))
def test_effects_against_the_dense_truth(name, fast):
    cs = ar.case(name)
    obj = _device(cs)
    ppv, pinfo, pst = _scan(obj, fast)(cs.G, return_stats=True, progress=False)
    pv, info, st = _scan(obj, fast)(cs.G, effects=True, progress=False)
    case = "%s, %s" % (name, "fast" if fast else "full refit")
    # the plain call's p-values and likelihoods, bit for bit
    assert np.array_equal(pv, ppv) and np.array_equal(st["alt_lml"], pst["alt_lml"])
    assert st["null_lml"] == pst["null_lml"] and st["null_delta"] == pst["null_delta"]
    for k in pinfo:
        assert np.array_equal(info[k], pinfo[k])
    p = cs.G.shape[1]
    for k in KEYS:
        assert st[k].shape == (p,) and st[k].dtype == (np.int32 if k == "effect_status" else np.float64), k
    rho, null_delta, null_lml = float(info["rho1"][0]), float(st["null_delta"]), float(st["null_lml"])
    comp = cs.compared()
    _hold(case, cs, cs.y, cs.G, rho, null_delta, null_lml, st, fast, comp)
    # statuses: exactly the planted columns may differ from OK
    others = [j for j in range(p) if j not in comp]
    if others:
        assert others == [cs.span, cs.boundary]
        assert st["effect_status"][cs.span] == IN_SPAN and st["effect_status"][cs.boundary] in (OK, IN_SPAN)
        print("[effects] %s: boundary column: status %d" % (case, st["effect_status"][cs.boundary]))
        for j in others:
            dropped = st["effect_status"][j] == IN_SPAN
            assert np.isnan(st["beta"][j]) == dropped and np.isnan(st["beta_se"][j]) == dropped
            assert np.isfinite(st["alt_scale"][j]) and np.isfinite(st["alt_delta"][j]) and np.isfinite(pv[j])
        _hold_log_pvalue(case, st, null_lml, others)
    if fast:
        # exact algebra of ML with delta frozen: 2 (alt - null) = n log(1 + z^2 / n), z = beta / beta_se.  z^2 carries four
        # times the tolerance (beta and beta_se each, squared) and moves the right side by at most min(z^2, n) times that;
        # the left side carries the absolute rounding of the two likelihoods, 8 eps |null_lml|.
        z2 = (st["beta"][comp] / st["beta_se"][comp]) ** 2
        lhs = 2 * (st["alt_lml"][comp] - null_lml)
        rhs = cs.n * np.log1p(z2 / cs.n)
        bound = 4 * ar.TOLERANCE * np.minimum(z2, cs.n) + 8 * EPS * abs(null_lml)
        print("[effects] %s: LRT identity, worst share of its bound %.2e" % (case, (np.abs(lhs - rhs) / bound).max()))
        assert np.all(np.abs(lhs - rhs) <= bound), (case, np.abs(lhs - rhs).max())
    # the deep tail
    lrs = 2 * (st["alt_lml"][cs.causal] - null_lml)
    if name.startswith("B"):
        assert lrs > 1500 and pv[cs.causal] == TINY
        assert np.isfinite(st["log_pvalue"][cs.causal]) and st["log_pvalue"][cs.causal] < math.log(1e-300)
    else:
        assert lrs > 100 and st["log_pvalue"][cs.causal] < -50


# ---- identities that need no truth ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
def test_sign_and_scale_of_the_variant(fast):
    """g -> -g flips beta; g -> -2 g halves it and beta_se.  Both maps are exact in floating point (a sign, a power of two),
    so the alt fits see the same numbers and the relations hold to rounding: twice the tolerance is asked."""
    cs = ar.case("A, mode C, c 3")
    sel = [0, 5, 7, 20, ar.CAUSAL]
    g = cs.G[:, sel]
    pv, info, st = _scan(_device(cs), fast)(np.column_stack([g, -g, -2.0 * g]), effects=True, progress=False)
    assert np.all(st["effect_status"] == OK)
    k = len(sel)
    b, s = st["beta"], st["beta_se"]
    print("[effects] sign and scale, %s: delta spread %.2e" % ("fast" if fast else "full refit",
          max(np.abs(st["alt_delta"][k:2 * k] / st["alt_delta"][:k] - 1).max(), np.abs(st["alt_delta"][2 * k:] / st["alt_delta"][:k] - 1).max())))
    tol = 2 * ar.TOLERANCE
    assert np.all(np.abs(b[k:2 * k] + b[:k]) <= tol * np.abs(b[:k])) and np.all(np.abs(s[k:2 * k] - s[:k]) <= tol * s[:k])
    assert np.all(np.abs(b[2 * k:] + b[:k] / 2) <= tol * np.abs(b[:k])) and np.all(np.abs(s[2 * k:] - s[:k] / 2) <= tol * s[:k])
    assert np.all(np.abs(st["alt_scale"][k:2 * k] - st["alt_scale"][:k]) <= tol * st["alt_scale"][:k])


def test_log_pvalue_kernel():
    """The statement of the effects kernels through its test hook: lrs = 0 gives 0 exactly, 1e-300 and 1e-8 sit where
    erfc rounds to 1 - O(eps), 1400 and 1500 straddle the switch to log(erfcx(x)) - x^2 at p = 1e-300."""
    from cellregmap_amd import _engine, _lib

    lrs = np.array([0.0, 1e-300, 1e-8, 1.0, 30.0, 1400.0, 1500.0, 5000.0, -3.0])
    out = np.empty_like(lrs)
    _lib.check(_lib.load().crm_test_lrt_logp(_engine._context(0), lrs.size, _lib.ptr(lrs), _lib.ptr(out)))
    assert out[0] == 0.0 and out[-1] == 0.0                    # (a negative statistic counts as 0)
    for x, got in zip(lrs[1:-1], out[1:-1]):
        want = ar.mp_log_sf(x)
        print("[effects] log p at lrs %g: %.17g, off by %.2e" % (x, got, abs(got - want) / abs(want)))
        assert abs(got - want) <= 1e-12 * abs(want), (x, got, float(want))


# ---- blocks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
def test_three_blocks_and_a_ragged_tail(fast):
    """297 variants at 128 per block (the smallest block the library takes; the last block holds 41).  Fast: every variant
    against the truth (they share one delta, so one longdouble factorisation serves all).  Full refit, where each variant
    needs its own factorisation: both sides of both block borders, the first, the last and every eleventh variant, which
    reaches the interior of every block; the others are held finite with status OK."""
    from cellregmap_amd import _engine, _lib

    cs = ar.case("A, mode C, c 1")
    rng = np.random.default_rng(8)
    G = np.concatenate([cs.G[:, [j for j in range(41) if j not in (ar.SPAN, ar.BOUNDARY)]]] * 8, axis=1)[:, :297]
    G = G + 0.05 * rng.normal(size=G.shape)
    lib, ctx = _lib.load(), _engine._context(0)
    _lib.check(lib.crm_set_block_variants(ctx, 128))
    try:
        obj = _device(cs)
        ppv, _ = _scan(obj, fast)(G, progress=False)
        pv, info, st = _scan(obj, fast)(G, effects=True, progress=False)
    finally:
        _lib.check(lib.crm_set_block_variants(ctx, 0))
    assert np.array_equal(pv, ppv) and np.all(st["effect_status"] == OK)
    for k in KEYS:
        assert st[k].shape == (297,) and np.all(np.isfinite(st[k]))
    _hold("three blocks, %s" % ("fast" if fast else "full refit"), cs, cs.y, G, float(info["rho1"][0]), float(st["null_delta"]),
          float(st["null_lml"]), st, fast,
          list(range(297)) if fast else sorted(set(range(0, 297, 11)) | {127, 128, 255, 256, 296}), oracle_delta=False)


# ---- several phenotypes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
def test_three_phenotypes_with_cis_windows(fast):
    """Overlapping windows, one repeated column and one empty window; every row against the truth at its own delta, and
    equal to the one-phenotype call's arrays: fast, within twice the tolerance (the two calls form g'W and g'y in another
    order; delta is the null model's in both, bit for bit); full refit, delta to twice the alt fit's tolerance (two
    searches) and the numbers through the truth at each call's own delta."""
    from cellregmap_amd import CellRegMap, scan_association_many

    cs = ar.case("A, mode C, c 3")
    Y = ar.phenotypes(cs, 4)
    first = CellRegMap(Y[:, 0], cs.E, W=cs.W, **cs.device_kw())
    crms = [first] + [CellRegMap(Y[:, i], cs.E, W=cs.W, background=first._bg, **cs.device_kw()) for i in (1, 2, 3)]
    cis = [np.array([5, 1, 1, 20, ar.CAUSAL, ar.SPAN]), slice(0, 24), np.array([], int), (15, 41)]
    cols = [np.array([5, 1, 1, 20, ar.CAUSAL, ar.SPAN]), np.arange(0, 24), np.array([], int), np.arange(15, 41)]
    ppv, pinfo = scan_association_many(crms, cs.G, cis_index=cis, fast=fast, return_stats=True)
    pv, info = scan_association_many(crms, cs.G, cis_index=cis, fast=fast, return_stats="effects")
    kind = "fast" if fast else "full refit"
    for i in range(4):
        assert np.array_equal(pv[i], ppv[i]) and np.array_equal(info["alt_lml"][i], pinfo["alt_lml"][i])   # bit for bit
        for k in KEYS:
            assert info[k][i].shape == (cols[i].size,), (k, i)
        if not cols[i].size:
            continue
        G = cs.G[:, cols[i]]
        st = {k: info[k][i] for k in KEYS + ("alt_lml",)}
        comp = [q for q, j in enumerate(cols[i]) if j not in (ar.SPAN, ar.BOUNDARY)]
        rho, nd, nl = float(info["rho1"][i]), float(info["null_delta"][i]), float(info["null_lml"][i])
        _hold("three phenotypes (%s), phenotype %d" % (kind, i), cs, Y[:, i], G, rho, nd, nl, st, fast, comp)
        # the one-phenotype call
        opv, oinfo, ost = _scan(crms[i], fast)(G, effects=True, progress=False)
        assert np.array_equal(ost["effect_status"], st["effect_status"]) and oinfo["rho1"][0] == rho
        if fast:
            assert np.array_equal(ost["alt_delta"], st["alt_delta"])
            for k in ("beta", "beta_se", "alt_scale"):
                assert np.all(np.abs(ost[k][comp] - st[k][comp]) <= 2 * ar.TOLERANCE * np.abs(st[k][comp])), (k, i)
        else:
            assert np.all(np.abs(ost["alt_delta"][comp] - st["alt_delta"][comp]) <= 2 * ar.DELTA_RTOL * st["alt_delta"][comp])
            _hold("one phenotype of the three (%s), phenotype %d" % (kind, i), cs, Y[:, i], G, rho, nd, nl, ost, fast, comp,
                  oracle_delta=False)
    assert info["beta"][0][1] == info["beta"][0][2] and info["log_pvalue"][0][1] == info["log_pvalue"][0][2]
    assert info["effect_status"][0][5] == IN_SPAN and np.isnan(info["beta"][0][5])
    assert np.unique(info["rho1"]).size >= 2, info["rho1"]      # (more than one rho group in the pass)


# ---- the wrappers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
def test_run_association_keeps_the_positional_swap(fast):
    """run_association(y, W, E, G, hK) binds W to the contexts slot and E to the fixed effects (_cellregmap.py:498, :529):
    beta is the coefficient of g beside the contexts, under the background of [W, hK]."""
    import pinned_reference as pr
    from cellregmap_amd import run_association, run_association_fast

    cs = ar.case("A, mode B, c 1")
    G = cs.G[:, [0, 5, 7, 20, ar.CAUSAL]]
    f = run_association_fast if fast else run_association
    ppv, pinfo = f(cs.y, cs.W, cs.E, G, hK=cs.hK_full)
    pv, info, st = f(cs.y, cs.W, cs.E, G, hK=cs.hK_full, effects=True)
    assert np.array_equal(pv, ppv) and np.all(st["effect_status"] == OK)
    rho = float(info["rho1"][0])
    hS = np.asarray(pr.half_factor(rho, cs.W, hK=cs.hK_full), ar.LD)
    delta = st["alt_delta"]
    assert np.all((delta >= ar.DELTA_RANGE[0]) & (delta <= ar.DELTA_RANGE[1])), delta
    if fast:
        assert np.all(delta == st["null_delta"])
    truth = ar.dense_truth(cs.y, cs.E, G, hS @ hS.T, delta)
    gap = ar.gaps(np.array([st["beta"], st["beta_se"], st["alt_scale"]]), truth)
    print("[effects] run_association%s: %s" % ("_fast" if fast else "", gap.max(axis=1)))
    assert np.all(gap <= ar.TOLERANCE), gap.max(axis=1)


@pytest.mark.parametrize("fast", [True, False])
def test_run_association_many_carries_effects(fast):
    import pinned_reference as pr
    from cellregmap_amd import run_association, run_association_fast, run_association_many

    cs = ar.case("A, mode B, c 1")
    Y = ar.phenotypes(cs, 2)
    G = cs.G[:, [0, 5, 7, 20]]
    pv, info = run_association_many(Y, cs.W, cs.E, G, hK=cs.hK_full, fast=fast, effects=True)
    for i in range(2):
        opv, oinfo, ost = (run_association_fast if fast else run_association)(Y[:, i], cs.W, cs.E, G, hK=cs.hK_full, effects=True)
        assert np.array_equal(info["effect_status"][i], ost["effect_status"]) and info["rho1"][i] == oinfo["rho1"][0]
        # each call against the truth at its own delta (the two full-refit searches stop where they stop)
        hS = np.asarray(pr.half_factor(float(info["rho1"][i]), cs.W, hK=cs.hK_full), ar.LD)
        for st in ({k: info[k][i] for k in KEYS}, ost):
            assert np.all((st["alt_delta"] >= ar.DELTA_RANGE[0]) & (st["alt_delta"] <= ar.DELTA_RANGE[1]))
            gap = ar.gaps(np.array([st["beta"], st["beta_se"], st["alt_scale"]]),
                          ar.dense_truth(Y[:, i], cs.E, G, hS @ hS.T, st["alt_delta"]))
            assert np.all(gap <= ar.TOLERANCE), (i, gap.max(axis=1))
        if fast:
            assert np.array_equal(info["alt_delta"][i], ost["alt_delta"])


# ---- the streamed path and the empty panel ----------------------------------------------------------------------------------
_STREAM = """
import json, os, sys
import numpy as np
sys.path.insert(0, %(tests)r)
import assoc_effects_reference as ar
from cellregmap_amd import CellRegMap
cs = ar.case("A, mode B, c 1")
obj = CellRegMap(cs.y, cs.E, W=cs.W, **cs.device_kw())
out = {}
for fast in (True, False):
    scan = obj.scan_association_fast if fast else obj.scan_association
    os.environ["CELLREGMAP_AMD_STREAM_CHUNK"] = "0"
    pv, info, st = scan(cs.G, effects=True, progress=False)
    os.environ["CELLREGMAP_AMD_STREAM_CHUNK"] = "16"
    seen = []
    spv, sinfo, sst = scan(cs.G, effects=True, progress=lambda done, total: seen.append((done, total)))
    out[str(fast)] = {"pv": [pv.tolist(), spv.tolist()], "seen": seen[-1],
                      "stats": {k: [np.asarray(st[k]).tolist(), np.asarray(sst[k]).tolist()] for k in st}}
print("RESULT " + json.dumps(out))
"""


def test_streamed_scan_carries_effects():
    """A host matrix past twice CELLREGMAP_AMD_STREAM_CHUNK goes to the device in column chunks (here 16 of 41 variants), in
    a fresh process: the same arrays as the one-panel scan."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _STREAM % {"tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True,
                       env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for fast in ("True", "False"):
        rec = out[fast]
        assert rec["seen"] == [41, 41]
        a, b = (np.array(v, float) for v in rec["pv"])
        assert np.allclose(a, b, rtol=1e-12, atol=0)
        for k, (one, streamed) in rec["stats"].items():
            one, streamed = np.asarray(one, float), np.asarray(streamed, float)
            assert one.shape == streamed.shape
            if k == "effect_status":
                assert np.array_equal(one, streamed)
            else:
                # (a variant's numbers do not depend on the chunk it travels in)
                assert np.allclose(one, streamed, rtol=1e-12, atol=0, equal_nan=True), (fast, k)
        assert np.isnan(rec["stats"]["beta"][1][ar.SPAN]) and np.isfinite(rec["stats"]["beta"][1][0])


@pytest.mark.parametrize("fast", [True, False])
def test_a_panel_without_variants(fast):
    cs = ar.case("A, mode B, c 1")
    pv, info, st = _scan(_device(cs), fast)(np.zeros((cs.n, 0)), effects=True, progress=False)
    assert pv.shape == (0,) and np.isfinite(st["null_lml"]) and info["rho1"].shape == (1,)
    for k in KEYS:
        assert st[k].shape == (0,) and st[k].dtype == (np.int32 if k == "effect_status" else np.float64)


# ---- misuse -----------------------------------------------------------------------------------------------------------------
def test_misuse_returns_the_argument_error():
    from cellregmap_amd import _lib

    cs = ar.case("A, mode B, c 1")
    obj = _device(cs)
    lib = _lib.load()
    panel, gene = obj._panel(cs.G), obj._bind_gene()
    out = np.empty(41)
    none = [None] * 9
    assert lib.crm_scan_association_effects(None, panel.handle, 0, 41, 1, *none) == -2
    assert lib.crm_scan_association_effects(gene, panel.handle, 0, -1, 1, *none) == -2
    assert lib.crm_scan_association_effects(gene, panel.handle, 40, 2, 1, *none) == -2
    assert lib.crm_scan_association_multi_effects(None, 1, panel.handle, 0, 41, 1, *none) == -2
    # every added output may be NULL: beta alone
    null = np.empty(6)
    _lib.check(lib.crm_scan_association_effects(gene, panel.handle, 0, 41, 1, None, None, _lib.ptr(null), _lib.ptr(out),
                                                None, None, None, None, None))
    assert np.isfinite(out[0]) and np.isnan(out[ar.SPAN])
