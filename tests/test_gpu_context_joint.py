"""The joint fixed-effect GxC test (``CellRegMap.scan_interaction_contexts_joint``, crm_scan_interaction_contexts_joint;
cellregmap_amd/csrc/context_joint.hip) against the extended-precision reference at the point the
device itself reports (tests/context_joint_reference.py: ``pinned_reference.pinned_ml`` of [W, C, g] and of
[W, C, g, kept candidates] with a shared factorisation, beta and beta_se by the same whitening).

Per cohort of tests/context_joint_cases.py and held variant, at (rho1, null_delta_i) of the device:
  * null lml, alt lml, the statistic 2 (alt - null) relative to |null lml|, beta (the largest gap relative to the largest
    |beta|) and beta_se within ``pinned_reference.limits``: 32 x the float64 oracle's own error at the same points (its
    ``LMM`` pinned at delta on both design matrices), floor n x 2.2e-16, ceiling 1e-11, asserted never to bind;
  * the null (null_lml, null_delta, rho1, e2, g2, eps2) is ``scan_interaction_contexts``'s bit for bit; at k = 1 the two
    calls agree on p, alt lml, beta and beta_se within the limits; everywhere the joint statistic is at least the largest
    per-context one (nested models);
  * p and log p against mpmath at the device's own statistic and dof: (dof + 16) x 2.2e-16 x max(1, |log p|).
Shapes: k = 1, 3, 5, 17, 33, 48, 50, 64; c = 2 .. 128; spectrum ranks 13 .. 260; both ``fast`` values.  Then dependent
candidates, the ends of the p-value, panels, sub-ranges and the ABI's refusals.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import context_joint_cases as jc
import context_joint_reference as jr
import pinned_reference as pr
from context_joint_hold import COLLINEAR, LD, OK, ONE_LESS, RECORD, TINY, _abi_scan, _At, _device, _hold, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    """The per-case errors go beside the file $CRM_PINNED_JSON names, as <name>_contexts_joint.json."""
    yield
    dest = os.environ.get("CRM_PINNED_JSON")
    if dest and RECORD:
        with open(os.path.splitext(dest)[0] + "_contexts_joint.json", "w") as fh:
            json.dump(RECORD, fh, indent=1, sort_keys=True)


# ---- every shape, both fast values; the per-context call beside it -----------------------------------------------------
SEEN_DOF = set()
SEEN_RHO = {}


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("name", list(jc.CASES))
def test_against_the_reference(name, fast):
    cs = jc.case(name)
    obj = _device(cs)
    pv, info = obj.scan_interaction_contexts_joint(cs.G, fast=fast, return_stats=True)
    case = "joint %s, %s" % ("fast" if fast else "refit", name)
    at, lim = _hold(case, cs, cs.y, cs.G, pv, info, fast)
    SEEN_DOF.update(int(d) for d in info["dof"])
    SEEN_RHO[name] = at.rho

    # the null is the per-context call's, bit for bit
    pv1, each = obj.scan_interaction_contexts(cs.G, fast=fast, return_stats=True)
    for key in ("null_lml", "null_delta", "rho1", "e2", "g2", "eps2"):
        assert np.array_equal(info[key], each[key]), (name, key)
    assert info["gene_null_lml"] == each["gene_null_lml"] and info["gene_null_delta"] == each["gene_null_delta"]
    # nested models: the joint statistic is at least every per-context one
    lrs = 2 * (info["alt_lml"] - info["null_lml"])
    top = 2 * (each["alt_lml"].max(axis=1) - each["null_lml"])
    assert np.all(lrs >= top - cs.n * 2.2e-16 * np.abs(info["null_lml"])), (name, lrs, top)
    if cs.k == 1:
        # one candidate: the per-context test itself, within the limits of either call
        for j in pr.pick(cs.G.shape[1]):
            assert pr.relative(info["alt_lml"][j], LD(each["alt_lml"][j, 0])) <= 2 * lim["lml"]
            assert abs(lrs[j] - top[j]) <= 2 * lim["lrs"] * abs(info["null_lml"][j])
            assert pr.relative(info["beta"][j, 0], LD(each["beta"][j, 0])) <= 2 * lim["beta"]
            assert pr.relative(info["beta_se"][j, 0], LD(each["beta_se"][j, 0])) <= 2 * lim["beta_se"]
            # p is the same function of the statistic in both calls: apart by no more than the statistics are, times the
            # density exp(-lrs / 2) / sqrt(2 pi lrs) at the smaller one
            gap, low = 2 * lim["lrs"] * abs(info["null_lml"][j]), min(lrs[j], top[j])
            assert low > 0 and abs(pv[j] - pv1[j, 0]) <= gap * math.exp(-low / 2) / math.sqrt(2 * math.pi * low) + 1e-14 * pv1[j, 0]


def test_odd_and_even_dof_and_two_grid_points():
    for name in jc.CASES:
        if name not in SEEN_RHO:
            cs = jc.case(name)
            _, info = _device(cs).scan_interaction_contexts_joint(cs.G[:, :1])
            SEEN_DOF.update(int(d) for d in info["dof"])
            SEEN_RHO[name] = float(info["rho1"][0])
    assert {d % 2 for d in SEEN_DOF} == {0, 1}, SEEN_DOF
    assert SEEN_DOF >= {1, 3, 5, 17, 33, 48, 50, 64}, SEEN_DOF
    rhos = {name: SEEN_RHO[name] for name in jc.CASES if jc.CASES[name][4] == "B"}
    assert len(set(rhos.values())) >= 2, rhos
    assert any(0.0 < SEEN_RHO[name] < 1.0 for name in jc.WIDE), SEEN_RHO


# ---- the ends of the p-value ---------------------------------------------------------------------------------------------
def test_a_planted_effect_underflows_the_pvalue():
    """y carries 40 000 x (g_2 o C_2): the statistic passes 1500, where the tail underflows and ``lrt_pvalues`` clips to
    the smallest normal double; the log is finite, below the log of that, and within its tolerance."""
    cs = jc.case("k 3, c 9, mode B")
    y = cs.y + 4e4 * cs.G[:, 2] * cs.C[:, 2]
    pv, info = _device(cs, y).scan_interaction_contexts_joint(cs.G, return_stats=True)
    lrs = 2 * (info["alt_lml"][2] - info["null_lml"][2])
    assert lrs > 1500 and info["dof"][2] == 3, (lrs, info["dof"])
    assert pv[2] == TINY, pv[2]
    lp = info["log_pvalue"][2]
    assert np.isfinite(lp) and lp < math.log(TINY), lp
    want = jr.mp_log_pvalue(3, lrs)
    assert abs(lp - want) <= jr.tail_tolerance(3, want), (lp, want)
    assert info["status"][2] == OK and np.all(np.isfinite(info["beta"][2]))
    # and an even dof in the far tail: five contexts less one constant column
    cs = jc.case("k 5, c 62, mode B")
    y = cs.y + 4e4 * cs.G[:, 0] * cs.C[:, 0]
    C = cs.C.copy()
    C[:, 3] = 1.0
    pv, info = _device(cs, y, C=C).scan_interaction_contexts_joint(cs.G, return_stats=True)
    lrs = 2 * (info["alt_lml"][0] - info["null_lml"][0])
    assert lrs > 1500 and info["dof"][0] == 4, (lrs, info["dof"])
    assert pv[0] == TINY
    want = jr.mp_log_pvalue(4, lrs)
    assert abs(info["log_pvalue"][0] - want) <= jr.tail_tolerance(4, want), (info["log_pvalue"][0], want)


# ---- dependent candidates ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
def test_a_constant_context_column(fast):
    """Contexts [C_0, 1, C_2] beside a W that holds the intercept: the candidate g o 1 = g lies in the span of [W, C, g]
    and leaves: dof 2, exactly that column flagged, statistic and betas the reference's with the column removed."""
    cs = jc.case("k 3, c 9, mode B")
    C = np.column_stack([cs.C[:, 0], np.ones(cs.n), cs.C[:, 2]])
    pv, info = _device(cs, C=C).scan_interaction_contexts_joint(cs.G, fast=fast, return_stats=True)
    assert np.all(info["dof"] == 2) and np.all(info["status"] == OK)
    assert np.array_equal(info["dropped"], np.tile([False, True, False], (cs.G.shape[1], 1)))
    at = _At(cs, cs.y, float(info["rho1"][0]), C=C, XC=C[:, [0, 2]])
    _hold("joint %s, constant column" % ("fast" if fast else "refit"), cs, cs.y, cs.G, pv, info, fast, at=at, keep=[0, 2])


@pytest.mark.parametrize("fast", [True, False])
def test_one_hot_contexts_drop_the_last(fast):
    """Four one-hot contexts sum to one: beside the intercept [W, C] has rank 9, and of the dependent candidates
    g o C_0 .. g o C_3 (their sum is g) the last in order leaves."""
    cs = jc.case("k 3, c 9, mode B")
    hot = np.eye(4)[np.random.default_rng(5).integers(0, 4, size=cs.n)]
    pv, info = _device(cs, C=hot).scan_interaction_contexts_joint(cs.G, fast=fast, return_stats=True)
    assert np.all(info["dof"] == 3) and np.all(info["status"] == OK), (info["dof"], info["status"])
    assert np.array_equal(info["dropped"], np.tile([False, False, False, True], (cs.G.shape[1], 1)))
    at = _At(cs, cs.y, float(info["rho1"][0]), C=hot, XC=hot[:, :3])
    _hold("joint %s, one-hot contexts" % ("fast" if fast else "refit"), cs, cs.y, cs.G, pv, info, fast, at=at, keep=[0, 1, 2])


@pytest.mark.parametrize("fast", [True, False])
def test_a_variant_in_the_span_of_w(fast):
    cs = jc.case("k 3, c 9, mode B")
    G = cs.G.copy()
    G[:, 1] = cs.W @ np.linspace(-1.0, 2.0, cs.W.shape[1])
    pv, info = _device(cs).scan_interaction_contexts_joint(G, fast=fast, return_stats=True)
    assert info["status"][1] == COLLINEAR and np.all(info["status"][[0, 2]] == OK), info["status"]
    assert info["dof"][1] == 0 and pv[1] == ONE_LESS and info["log_pvalue"][1] == 0.0
    assert np.all(np.isnan(info["beta"][1])) and np.all(np.isnan(info["beta_se"][1])) and np.all(info["dropped"][1])
    assert info["alt_lml"][1] == info["null_lml"][1]
    _hold("joint %s, variant in the span of W" % ("fast" if fast else "refit"), cs, cs.y, G, pv, info, fast, sel=[0, 2])


# ---- panels, sub-ranges, windows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
def test_a_donor_level_panel_equals_the_expanded_matrix(fast):
    from cellregmap_amd import GenotypePanel

    cs = jc.case("k 3, c 9, mode B")
    Gd = np.random.default_rng(11).normal(size=(cs.donors, 5))
    obj = _device(cs)
    grouped = obj.scan_interaction_contexts_joint(GenotypePanel.from_donors(Gd, cs.donor_of_cell), fast=fast, return_stats=True)
    dense = obj.scan_interaction_contexts_joint(GenotypePanel(Gd[cs.donor_of_cell], groups=None), fast=fast, return_stats=True)
    _same(grouped, dense)
    assert np.all(grouped[1]["status"] == OK) and np.all(np.isfinite(grouped[0]))


@pytest.mark.parametrize("fast", [True, False])
def test_a_ragged_last_sub_range(fast):
    """Five variants with room for the rotated candidates of two: sub-ranges of 2, 2 and 1.  Bit for bit the one-range call."""
    from cellregmap_amd import _engine, _lib

    cs = jc.JointCase("k 3, c 9, mode B", variants=5)
    obj = _device(cs)
    whole = obj.scan_interaction_contexts_joint(cs.G, fast=fast, return_stats=True)
    lib, ctx = _lib.load(), _engine._context(0)
    ldq = -(-max(obj._bg.rank(i) for i in range(len(cs.grid))) // 128) * 128    # the spectra's common leading dimension
    per_variant = 8 * cs.k * ldq
    _lib.check(lib.crm_test_set_context_budget(ctx, 2 * per_variant + 8))
    try:
        cut = obj.scan_interaction_contexts_joint(cs.G, fast=fast, return_stats=True)
        _lib.check(lib.crm_test_set_context_budget(ctx, 1))          # (below one variant: one per sub-range)
        one = obj.scan_interaction_contexts_joint(cs.G, fast=fast, return_stats=True)
    finally:
        _lib.check(lib.crm_test_set_context_budget(ctx, 0))
    _same(whole, cut)
    _same(whole, one)


def test_a_ragged_sub_range_with_v_in_global_scratch():
    """The same at k = 48, c = 128, where V lives in the variant's global scratch row: rows of the scratch are per sub-range."""
    from cellregmap_amd import _engine, _lib

    cs = jc.case("k 48, c 128, mode B")
    obj = _device(cs)
    whole = obj.scan_interaction_contexts_joint(cs.G, return_stats=True)
    lib, ctx = _lib.load(), _engine._context(0)
    ldq = -(-max(obj._bg.rank(i) for i in range(len(cs.grid))) // 128) * 128
    _lib.check(lib.crm_test_set_context_budget(ctx, 2 * 8 * cs.k * ldq + 8))
    try:
        cut = obj.scan_interaction_contexts_joint(cs.G, return_stats=True)
    finally:
        _lib.check(lib.crm_test_set_context_budget(ctx, 0))
    _same(whole, cut)


@pytest.mark.parametrize("fast", [True, False])
def test_a_window_of_a_resident_panel_equals_the_sliced_matrix(fast):
    from cellregmap_amd import GenotypePanel

    cs = jc.JointCase("k 3, c 9, mode B", variants=5)
    rc, out = _abi_scan(cs, GenotypePanel(cs.G, groups=None), 1, 3, fast)
    assert rc == 0
    pv, info = _device(cs).scan_interaction_contexts_joint(cs.G[:, 1:4], fast=fast, return_stats=True)
    want = (pv, info["log_pvalue"], info["alt_lml"], info["dof"], info["beta"], info["beta_se"], info["dropped"].astype(np.int32),
            info["status"], info["null_lml"], info["null_delta"])
    for got, ref in zip(out[:10], want):
        assert np.array_equal(got, ref, equal_nan=got.dtype != np.int32)
    assert out[10][4] == info["gene_null_lml"] and out[10][0] == info["rho1"][0]


@pytest.mark.parametrize("fast", [True, False])
def test_run_interaction_contexts_joint_equals_the_class_call(fast):
    from cellregmap_amd import CellRegMap, get_L_values, run_interaction_contexts_joint

    cs = jc.case("k 3, c 9, mode B")
    pv, info = run_interaction_contexts_joint(cs.y, cs.C, cs.G, W=cs.W, hK=cs.hK, fast=fast)
    obj = CellRegMap(y=cs.y, E=cs.C, W=cs.W, E1=cs.C, Ls=get_L_values(cs.hK, cs.C))
    pv2, info2 = obj.scan_interaction_contexts_joint(cs.G, fast=fast)
    assert np.array_equal(pv, pv2) and sorted(info) == sorted(info2)
    assert sorted(info) == ["beta", "beta_se", "dof", "dropped", "e2", "eps2", "g2", "log_pvalue", "rho1", "status"]
    for key in info:
        assert np.array_equal(info[key], info2[key], equal_nan=info[key].dtype == np.float64), key
    # contexts given explicitly: the same tests
    pv3, _ = obj.scan_interaction_contexts_joint(cs.G, contexts=cs.C.copy(), fast=fast)
    assert np.array_equal(pv, pv3)


@pytest.mark.parametrize("fast", [True, False])
def test_a_streamed_host_matrix_equals_the_one_panel_scan(fast, monkeypatch):
    """A host matrix past twice CELLREGMAP_AMD_STREAM_CHUNK goes to the device in column chunks (here 2, 2 and 1 of five
    variants): the same arrays, and the progress callback ends on the whole count."""
    cs = jc.JointCase("k 3, c 9, mode B", variants=5)
    obj = _device(cs)
    monkeypatch.setenv("CELLREGMAP_AMD_STREAM_CHUNK", "0")
    whole = obj.scan_interaction_contexts_joint(cs.G, fast=fast, return_stats=True)
    monkeypatch.setenv("CELLREGMAP_AMD_STREAM_CHUNK", "2")
    seen = []
    streamed = obj.scan_interaction_contexts_joint(cs.G, fast=fast, return_stats=True,
                                                   progress=lambda done, total: seen.append((done, total)))
    _same(whole, streamed)
    assert seen and seen[-1] == (5, 5), seen


def test_a_panel_without_variants():
    cs = jc.case("k 3, c 9, mode B")
    pv, info = _device(cs).scan_interaction_contexts_joint(np.zeros((cs.n, 0)), return_stats=True)
    assert pv.shape == (0,) and info["beta"].shape == (0, 3) and info["dropped"].shape == (0, 3) and info["dof"].shape == (0,)
    assert np.isfinite(info["gene_null_lml"]) and info["rho1"].shape == (1,)


# ---- misuse ----------------------------------------------------------------------------------------------------------------
def test_misuse_returns_the_error_codes():
    from cellregmap_amd import GenotypePanel, _lib

    cs = jc.JointCase("k 3, c 9, mode B", variants=5)
    lib = _lib.load()
    panel = GenotypePanel(cs.G, groups=None)
    none = [None] * 11
    assert lib.crm_scan_interaction_contexts_joint(None, panel.handle, 0, 5, 1, *none) == -2
    assert _abi_scan(cs, panel, 0, -1, True)[0] == -2
    assert _abi_scan(cs, panel, 4, 2, True)[0] == -2
    other = GenotypePanel(cs.G[:-1], groups=None)          # another cell count
    assert _abi_scan(cs, other, 0, 5, True)[0] == -2
    assert b"cell count" in lib.crm_last_error()
    # one past the supported k: refused before anything is launched -- not even the gene-level null is reported
    rng = np.random.default_rng(3)
    wide = rng.normal(size=(cs.n, 65))
    rc, out = _abi_scan(cs, panel, 0, 5, True, C=wide, X0=np.column_stack([cs.W, cs.C]))
    assert rc == -3 and b"65 contexts" in lib.crm_last_error(), (rc, lib.crm_last_error())
    assert np.all(np.isnan(out[10]))


def test_one_past_the_supported_widths():
    from cellregmap_amd import GenotypePanel, _lib

    cs = jc.JointCase("k 3, c 9, mode B", variants=5)
    lib = _lib.load()
    obj = _device(cs)
    rng = np.random.default_rng(4)
    with pytest.raises(_lib.CrmError):
        obj.scan_interaction_contexts_joint(cs.G, contexts=rng.normal(size=(cs.n, 65)))
    assert b"65 contexts" in lib.crm_last_error()
    # a basis of 129 columns: crm_gene_create refuses such a gene already
    y = _lib.f64(cs.y)
    gene = ctypes.c_void_p()
    X129 = _lib.f64(rng.normal(size=(cs.n, 129)))
    C = _lib.f64(cs.C)
    assert lib.crm_gene_create(obj._bg.handle, _lib.ptr(y), _lib.ptr(X129), 129, _lib.ptr(C), cs.k, ctypes.byref(gene)) == -3
    assert not gene.value
    # 64 contexts and every output NULL are served
    pv, info = obj.scan_interaction_contexts_joint(cs.G[:, :1], contexts=rng.normal(size=(cs.n, 64)))
    assert info["dof"][0] == 64 and info["status"][0] == OK
    assert _abi_scan(cs, GenotypePanel(cs.G, groups=None), 0, 5, True, outputs=False)[0] == 0
