"""Per-context fixed-effect GxC tests (``CellRegMap.scan_interaction_contexts``, crm_scan_interaction_contexts;
cellregmap_amd/csrc/context_lrt.hip) against the extended-precision reference at the point the device
itself reports (tests/context_lrt_reference.py: ``pinned_reference.pinned_ml`` of [W, C, g] and [W, C, g, g o C_j] with a
shared factorisation, beta and beta_se by the same whitening).

Per case and held variant (``pinned_reference.pick``: at most three), at (rho1, null_delta_i) of the device:
  * ``null_lml_i``, every ``alt_lml``, the statistic 2 (alt - null) relative to |null lml|, ``beta`` (the largest gap
    over the variant's contexts relative to its largest |beta|) and ``beta_se`` within ``pinned_reference.limits``: 32 x
    the float64 oracle's own error at the same points (its ``LMM`` pinned at delta and its ``FastScanner`` over g o C),
    floor n x 2.2e-16, ceiling 1e-11, asserted never to bind;
  * ``fast=True``: null_delta_i is the gene-level delta bit for bit; ``fast=False``: null_lml_i between the two bounds
    around the reference's own maximum over delta (``pinned_ml_max``), as tests/test_gpu_pinned_association.py holds a
    refit; the optima have delta in (1e-3, 1 - 1e-3) (asserted; tests/test_context_lrt_reference_cpu.py checks it on the CPU);
  * p = erfc(sqrt(lrs / 2)) of the device's own lrs = -2 null + 2 alt in mpmath with the clips of ``lrt_pvalues``, and
    log_pvalue = log erfc(sqrt(max(lrs, 0) / 2)), both to 1e-14 relative;
  * rho1 is the reference's argmax over the grid unless its two best values tie within the lml limit.
Shapes: k = 1, 3, 5, 17; c = rank([W, C]) = 2, 9, 62, 70, 128; spectrum ranks 13 .. 27 and 260; modes A and B; both
``fast`` values.  Then the degenerate candidates, the ends of the p-value, panels, sub-ranges and the ABI's refusals.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import context_lrt_cases as cc
import pinned_reference as pr
from context_lrt_hold import COLLINEAR, OK, ONE_LESS, RECORD, TINY, _abi_scan, _At, _device, _hold, _mp_log_pvalue, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    """The per-case errors go beside the file $CRM_PINNED_JSON names, as <name>_contexts.json."""
    yield
    dest = os.environ.get("CRM_PINNED_JSON")
    if dest and RECORD:
        with open(os.path.splitext(dest)[0] + "_contexts.json", "w") as fh:
            json.dump(RECORD, fh, indent=1, sort_keys=True)


# ---- every shape, both modes ---------------------------------------------------------------------------------------------
SEEN_RHO = {}


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("name", list(cc.CASES))
def test_against_the_reference(name, fast):
    cs = cc.case(name)
    pv, info = _device(cs).scan_interaction_contexts(cs.G, fast=fast, return_stats=True)
    case = "contexts %s, %s" % ("fast" if fast else "refit", name)
    at, lim = _hold(case, cs, cs.y, cs.G, pv, info, fast)
    SEEN_RHO[name] = at.rho
    if fast:
        # the gene-level null: the reference's lml at (rho1, delta0), and its argmax over the grid
        rl, rs = pr.pinned_ml(cs.y, cs.X0(), None, float(info["gene_null_delta"]), gram=at.gram)
        gap = pr.relative(info["gene_null_lml"], rl)
        lmls = pr.grid_lmls(cs.y, cs.X0(), cs.half, cs.grid, restricted=False)
        best, tie = pr.argmax_or_tie(lmls, lim["lml"])
        print("[pinned]   gene-level null lml %.2e; rho1 %.1f, the reference's argmax %.1f%s"
              % (gap, at.rho, cs.grid[best], ", tied" if tie else ""))
        assert gap <= lim["lml"], (name, gap, lim["lml"])
        assert tie or at.rho == cs.grid[best], (name, at.rho, cs.grid[best], [float(v) for v in lmls])
        total = float(info["e2"][0] + info["g2"][0] + info["eps2"][0])
        assert abs(total - float(rs)) <= 32 * lim["lml"] * float(rs) + 1e-12 * float(rs)


def test_gene_level_nulls_on_two_grid_points():
    rhos = {}
    for name in cc.CASES:
        if cc.CASES[name][4] == "B":
            cs = cc.case(name)
            rhos[name] = SEEN_RHO[name] if name in SEEN_RHO else _device(cs).scan_interaction_contexts(cs.G[:, :1])[1]["rho1"][0]
    assert len(set(rhos.values())) >= 2, rhos


# ---- degenerate candidates ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
def test_a_constant_context_column(fast):
    """Contexts [C_0, 1, C_2] beside a W that holds the intercept: [W, C] has rank 8, and the candidate g o 1 = g lies in
    the span of [W, C, g]: flagged, p = 1 - eps, beta NaN; its neighbours are the tests of [W, C_0, C_2, g] at the same
    point (the reference is given the full-rank columns)."""
    cs = cc.case("k 3, c 9, mode B")
    C = np.column_stack([cs.C[:, 0], np.ones(cs.n), cs.C[:, 2]])
    pv, info = _device(cs, C=C).scan_interaction_contexts(cs.G, fast=fast, return_stats=True)
    assert np.all(info["status"][:, 1] == COLLINEAR) and np.all(info["status"][:, [0, 2]] == OK)
    assert np.all(pv[:, 1] == ONE_LESS) and np.all(np.isnan(info["beta"][:, 1])) and np.all(np.isnan(info["beta_se"][:, 1]))
    assert np.array_equal(info["alt_lml"][:, 1], info["null_lml"]) and np.all(info["log_pvalue"][:, 1] == 0.0)
    rho = float(info["rho1"][0])
    keep = C[:, [0, 2]]
    at = _At(cs, cs.y, rho, C=keep)
    sub = dict(info)
    for key in ("alt_lml", "beta", "beta_se", "log_pvalue", "status"):
        sub[key] = info[key][:, [0, 2]]
    _hold("contexts %s, constant column" % ("fast" if fast else "refit"), cs, cs.y, cs.G, pv[:, [0, 2]], sub, fast, at=at)


@pytest.mark.parametrize("fast", [True, False])
def test_a_variant_in_the_span_of_w(fast):
    cs = cc.case("k 3, c 9, mode B")
    G = cs.G.copy()
    G[:, 1] = cs.W @ np.linspace(-1.0, 2.0, cs.W.shape[1])
    pv, info = _device(cs).scan_interaction_contexts(G, fast=fast, return_stats=True)
    assert np.all(info["status"][1] == COLLINEAR) and np.all(info["status"][[0, 2]] == OK), info["status"]
    assert np.all(pv[1] == ONE_LESS) and np.all(np.isnan(info["beta"][1])) and np.all(np.isnan(info["beta_se"][1]))
    assert np.all(info["alt_lml"][1] == info["null_lml"][1])
    # its null is the gene-level null's model: the same likelihood at the same delta
    if fast:
        assert abs(info["null_lml"][1] - info["gene_null_lml"]) <= 1e-12 * abs(info["gene_null_lml"])
    _hold("contexts %s, variant in the span of W" % ("fast" if fast else "refit"), cs, cs.y, G, pv, info, fast, sel=[0, 2])


def test_a_planted_effect_underflows_the_pvalue():
    """y carries 40 000 x (g_2 o C_2): the statistic of that candidate passes 1500, where erfc underflows and
    ``lrt_pvalues`` clips to the smallest normal double; the log is finite and below the log of that."""
    cs = cc.case("k 3, c 9, mode B")
    y = cs.y + 4e4 * cs.G[:, 2] * cs.C[:, 2]
    pv, info = _device(cs, y).scan_interaction_contexts(cs.G, return_stats=True)
    lrs = 2 * (info["alt_lml"][2, 2] - info["null_lml"][2])
    assert lrs > 1500, lrs
    assert pv[2, 2] == TINY, pv[2, 2]
    lp = info["log_pvalue"][2, 2]
    assert np.isfinite(lp) and lp < math.log(TINY), lp
    want = _mp_log_pvalue(float(info["null_lml"][2]), float(info["alt_lml"][2, 2]))
    assert abs(lp - want) <= 1e-14 * abs(want), (lp, want)
    assert info["status"][2, 2] == OK and np.isfinite(info["beta"][2, 2])


# ---- panels, sub-ranges, windows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
def test_a_donor_level_panel_equals_the_expanded_matrix(fast):
    from cellregmap_amd import GenotypePanel

    cs = cc.case("k 3, c 9, mode B")
    Gd = np.random.default_rng(11).normal(size=(cs.donors, 5))
    obj = _device(cs)
    grouped = obj.scan_interaction_contexts(GenotypePanel.from_donors(Gd, cs.donor_of_cell), fast=fast, return_stats=True)
    dense = obj.scan_interaction_contexts(GenotypePanel(Gd[cs.donor_of_cell], groups=None), fast=fast, return_stats=True)
    _same(grouped, dense)
    assert np.all(grouped[1]["status"] == OK) and np.all(np.isfinite(grouped[0]))


@pytest.mark.parametrize("fast", [True, False])
def test_a_ragged_last_sub_range(fast):
    """Five variants with room for the rotated candidates of two: sub-ranges of 2, 2 and 1.  Bit for bit the one-range call."""
    from cellregmap_amd import _engine, _lib

    cs = cc.ContextCase("k 3, c 9, mode B", variants=5)
    obj = _device(cs)
    whole = obj.scan_interaction_contexts(cs.G, fast=fast, return_stats=True)
    lib, ctx = _lib.load(), _engine._context(0)
    ldq = -(-max(obj._bg.rank(i) for i in range(len(cs.grid))) // 128) * 128    # the spectra's common leading dimension
    per_variant = 8 * cs.k * ldq
    _lib.check(lib.crm_test_set_context_budget(ctx, 2 * per_variant + 8))
    try:
        cut = obj.scan_interaction_contexts(cs.G, fast=fast, return_stats=True)
        _lib.check(lib.crm_test_set_context_budget(ctx, 1))          # (below one variant: one per sub-range)
        one = obj.scan_interaction_contexts(cs.G, fast=fast, return_stats=True)
    finally:
        _lib.check(lib.crm_test_set_context_budget(ctx, 0))
    _same(whole, cut)
    _same(whole, one)
    assert lib.crm_test_set_context_budget(ctx, -1) == -2


@pytest.mark.parametrize("fast", [True, False])
def test_a_window_of_a_resident_panel_equals_the_sliced_matrix(fast):
    from cellregmap_amd import GenotypePanel

    cs = cc.ContextCase("k 3, c 9, mode B", variants=5)
    rc, out = _abi_scan(cs, GenotypePanel(cs.G, groups=None), 1, 3, fast)
    assert rc == 0
    pv, info = _device(cs).scan_interaction_contexts(cs.G[:, 1:4], fast=fast, return_stats=True)
    for got, want in zip(out[:8], (pv, info["alt_lml"], info["beta"], info["beta_se"], info["log_pvalue"], info["status"],
                                   info["null_lml"], info["null_delta"])):
        assert np.array_equal(got, want, equal_nan=got.dtype != np.int32)
    assert out[8][4] == info["gene_null_lml"] and out[8][0] == info["rho1"][0]


@pytest.mark.parametrize("fast", [True, False])
def test_run_interaction_contexts_equals_the_class_call(fast):
    from cellregmap_amd import CellRegMap, get_L_values, run_interaction_contexts

    cs = cc.case("k 3, c 9, mode B")
    pv, info = run_interaction_contexts(cs.y, cs.C, cs.G, W=cs.W, hK=cs.hK, fast=fast)
    obj = CellRegMap(y=cs.y, E=cs.C, W=cs.W, E1=cs.C, Ls=get_L_values(cs.hK, cs.C))
    pv2, info2 = obj.scan_interaction_contexts(cs.G, fast=fast)
    assert np.array_equal(pv, pv2) and sorted(info) == sorted(info2)
    assert sorted(info) == ["beta", "beta_se", "e2", "eps2", "g2", "log_pvalue", "rho1", "status"]
    for key in info:
        assert np.array_equal(info[key], info2[key], equal_nan=True), key
    # contexts given explicitly: the same tests
    pv3, _ = obj.scan_interaction_contexts(cs.G, contexts=cs.C.copy(), fast=fast)
    assert np.array_equal(pv, pv3)


@pytest.mark.parametrize("fast", [True, False])
def test_a_streamed_host_matrix_equals_the_one_panel_scan(fast, monkeypatch):
    """A host matrix past twice CELLREGMAP_AMD_STREAM_CHUNK goes to the device in column chunks (here 2, 2 and 1 of five
    variants): the same arrays, and the progress callback ends on the whole count."""
    cs = cc.ContextCase("k 3, c 9, mode B", variants=5)
    obj = _device(cs)
    monkeypatch.setenv("CELLREGMAP_AMD_STREAM_CHUNK", "0")
    whole = obj.scan_interaction_contexts(cs.G, fast=fast, return_stats=True)
    monkeypatch.setenv("CELLREGMAP_AMD_STREAM_CHUNK", "2")
    seen = []
    streamed = obj.scan_interaction_contexts(cs.G, fast=fast, return_stats=True, progress=lambda done, total: seen.append((done, total)))
    _same(whole, streamed)
    assert seen and seen[-1] == (5, 5), seen


def test_a_panel_without_variants():
    cs = cc.case("k 3, c 9, mode B")
    pv, info = _device(cs).scan_interaction_contexts(np.zeros((cs.n, 0)), return_stats=True)
    assert pv.shape == (0, 3) and info["status"].shape == (0, 3) and info["null_lml"].shape == (0,)
    assert np.isfinite(info["gene_null_lml"]) and info["rho1"].shape == (1,)


# ---- misuse ------------------------------------------------------------------------------------------------------------------
def test_misuse_returns_the_error_codes():
    from cellregmap_amd import GenotypePanel, _lib

    cs = cc.ContextCase("k 3, c 9, mode B", variants=5)
    lib = _lib.load()
    panel = GenotypePanel(cs.G, groups=None)
    none = [None] * 9
    assert lib.crm_scan_interaction_contexts(None, panel.handle, 0, 5, 1, *none) == -2
    assert _abi_scan(cs, panel, 0, -1, True)[0] == -2
    assert _abi_scan(cs, panel, 4, 2, True)[0] == -2
    # another cell count
    other = GenotypePanel(cs.G[:-1], groups=None)
    assert _abi_scan(cs, other, 0, 5, True)[0] == -2
    assert b"cell count" in lib.crm_last_error()
    # more than 256 contexts, a basis of more than 128 columns: refused where the gene is bound, before anything is uploaded
    obj = _device(cs)
    y = _lib.f64(cs.y)
    rng = np.random.default_rng(3)
    gene = ctypes.c_void_p()
    wide = _lib.f64(rng.normal(size=(cs.n, 257)))
    X0 = _lib.f64(np.column_stack([cs.W, cs.C]))
    assert lib.crm_gene_create(obj._bg.handle, _lib.ptr(y), _lib.ptr(X0), X0.shape[1], _lib.ptr(wide), 257, ctypes.byref(gene)) == -3
    assert not gene.value
    X129 = _lib.f64(rng.normal(size=(cs.n, 129)))
    C = _lib.f64(cs.C)
    assert lib.crm_gene_create(obj._bg.handle, _lib.ptr(y), _lib.ptr(X129), 129, _lib.ptr(C), cs.k, ctypes.byref(gene)) == -3
    assert not gene.value
    with pytest.raises(_lib.CrmError):
        obj.scan_interaction_contexts(cs.G, contexts=rng.normal(size=(cs.n, 130)))
    # every output may be NULL
    assert _abi_scan(cs, panel, 0, 5, True, outputs=False)[0] == 0
