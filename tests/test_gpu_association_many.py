"""Multi-phenotype association scans (scan_association_many / run_association_many) against the single-phenotype path
and the CPU oracle (cellregmap/_cellregmap.py:246-314, 443-531).

Tolerances of test_gpu_association.py: p within 1e-5 p + 1e-300, info rtol 1e-5; alt lml within 1e-10 |null lml| of the
single-phenotype path; the null models bit for bit those of the single-phenotype path."""
import ctypes

import numpy as np
import pytest
from numpy.testing import assert_allclose

pytestmark = pytest.mark.gpu

ERR_ARG = -2


def _cohort(donors, cells, k, p, seed):
    from cellregmap_amd.synth import make_cohort

    return make_cohort(donors, cells, k, p, seed=seed)


def _phenotypes(c, count, seed):
    """count phenotypes on the cohort of c: mixtures of the context-driven, kinship-driven and noise parts."""
    rng = np.random.default_rng(seed)
    n = c.y.size
    Y = [c.y]
    for i in range(1, count):
        a, b = rng.uniform(0, 1, size=2)
        y = a * (c.E @ rng.normal(size=c.E.shape[1])) + b * (c.hK @ rng.normal(size=c.hK.shape[1])) + rng.normal(size=n)
        Y.append(y + 0.3 * c.G[:, i % c.G.shape[1]])
    return np.stack(Y, axis=1)


def _genotypes(c, seed):
    """the cohort's donor-level variants and as many cell-level ones (dense panel path)"""
    rng = np.random.default_rng(seed)
    return np.concatenate([c.G, rng.normal(size=c.G.shape)], axis=1)


def _close_p(pv, ref):
    assert pv.shape == ref.shape
    assert np.all(np.abs(pv - ref) <= 1e-5 * ref + 1e-300), np.c_[pv.ravel(), ref.ravel()]


def _check_against_single(crms, G, pv, info, fast, cols=None):
    """row i against crms[i].scan_association(_fast)(G[:, cols[i]]) -- null quantities bit for bit"""
    for i, crm in enumerate(crms):
        Gi = G if cols is None else G[:, cols[i]]
        f = crm.scan_association_fast if fast else crm.scan_association
        spv, sinfo, sst = f(Gi, return_stats=True, progress=False)
        for k in ("rho1", "e2", "g2", "eps2"):
            assert info[k][i] == sinfo[k][0], (k, i, info[k][i], sinfo[k][0])
        assert info["null_lml"][i] == sst["null_lml"] and info["null_delta"][i] == sst["null_delta"]
        _close_p(np.asarray(pv[i]), spv)
        alt = np.asarray(info["alt_lml"][i])
        assert np.all(np.abs(alt - sst["alt_lml"]) <= 1e-10 * abs(sst["null_lml"])), np.c_[alt, sst["alt_lml"]]


def _crms(c, Y, W, mode):
    from cellregmap_amd import CellRegMap

    kw = {"hK": c.hK} if mode == "B" else {}
    first = CellRegMap(Y[:, 0], c.E, W=W, **kw)
    return [first] + [CellRegMap(Y[:, i], c.E, W=W, background=first._bg, **kw) for i in range(1, Y.shape[1])]


@pytest.mark.parametrize("ngenes", [1, 3, 17])
@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("mode", ["A", "B"])
def test_many_matches_single_and_oracle(mode, fast, ngenes):
    from cellregmap_amd import scan_association_many
    from oracle.crm import OracleCellRegMap

    c = _cohort(10, 20, 3, 12, seed=31)
    rng = np.random.default_rng(2)
    W = np.concatenate([c.W, rng.normal(size=(c.y.size, 2))], axis=1)
    Y = _phenotypes(c, ngenes, seed=5)
    G = _genotypes(c, seed=6)
    crms = _crms(c, Y, W, mode)
    pv, info = scan_association_many(crms, G, fast=fast, return_stats=True)
    assert pv.shape == (ngenes, G.shape[1]) and info["rho1"].shape == (ngenes,)
    assert info["alt_lml"].shape == pv.shape
    _check_against_single(crms, G, pv, info, fast)
    kw = {"hK": c.hK} if mode == "B" else {}
    for i in sorted({0, ngenes - 1}):
        o = OracleCellRegMap(Y[:, i], c.E, W=W, **kw)
        opv, oinfo = (o.scan_association_fast if fast else o.scan_association)(G)
        _close_p(pv[i], opv)
        for k in ("rho1", "e2", "g2", "eps2"):
            assert_allclose(info[k][i], oinfo[k][0], rtol=1e-5, atol=1e-12)


@pytest.mark.parametrize("fast", [False, True])
def test_genes_on_several_grid_points_in_one_pass(fast):
    from cellregmap_amd import scan_association_many

    c = _cohort(12, 15, 3, 10, seed=32)
    rng = np.random.default_rng(3)
    n = c.y.size
    Y = []
    for wgt in np.linspace(0, 1, 9):   # from kinship-driven (rho* near 0) to context-driven (rho* near 1)
        y = wgt * (c.E @ rng.normal(size=3)) * 3 + (1 - wgt) * (c.hK @ rng.normal(size=c.hK.shape[1])) * 3
        Y.append(y + rng.normal(size=n))
    Y = np.stack(Y, axis=1)
    G = _genotypes(c, seed=7)
    crms = _crms(c, Y, c.W, "B")
    pv, info = scan_association_many(crms, G, fast=fast, return_stats=True)
    assert np.unique(info["rho1"]).size >= 2, info["rho1"]
    _check_against_single(crms, G, pv, info, fast)


@pytest.mark.parametrize("fast", [False, True])
def test_cis_windows(fast):
    from cellregmap_amd import _engine, _lib, scan_association_many

    c = _cohort(10, 20, 3, 40, seed=33)
    G = _genotypes(c, seed=8)[:, :75]   # p = 75: not a multiple of the block
    p = G.shape[1]
    Y = _phenotypes(c, 7, seed=9)
    crms = _crms(c, Y, c.W, "B")
    mask = np.zeros(p, bool)
    mask[[3, 17, 18, 40, 74]] = True
    cis = [(0, 30),                          # range across block boundaries
           slice(20, 60),                    # overlapping slice
           (10, 10),                         # empty window
           mask,                             # boolean mask
           np.array([70, 5, 5, 33, 12, 70]),  # unsorted, repeated
           slice(None, None, 7),             # strided slice
           np.array([-1, 0, 64])]            # negative index
    lib = _lib.load()
    _lib.check(lib.crm_set_block_variants(_engine._context(0), 16))
    try:
        pv, info = scan_association_many(crms, G, cis_index=cis, fast=fast, return_stats=True)
    finally:
        _lib.check(lib.crm_set_block_variants(_engine._context(0), 0))
    cols = [np.arange(p)[s] if isinstance(s, slice) else (np.arange(s[0], s[1]) if isinstance(s, tuple) else
                                                          (np.flatnonzero(s) if s.dtype == bool else s % p)) for s in cis]
    assert isinstance(pv, list) and [x.size for x in pv] == [x.size for x in cols]
    assert pv[2].size == 0 and info["alt_lml"][2].size == 0
    nonempty = [i for i in range(len(cis)) if cols[i].size]
    sub = [crms[i] for i in nonempty]
    subinfo = {k: (v[nonempty] if isinstance(v, np.ndarray) else [v[i] for i in nonempty]) for k, v in info.items()}
    _check_against_single(sub, G, [pv[i] for i in nonempty], subinfo, fast, cols=[cols[i] for i in nonempty])


@pytest.mark.parametrize("driver", ["association", "contexts"])
def test_progress_true_is_one_bar_over_the_walk(driver, monkeypatch):
    """``progress=True``: one tqdm bar over all runs of a cis walk, counted in the variants at least one phenotype tests."""
    import sys
    import types

    import cellregmap_amd as crm

    bars = []

    class Bar:
        def __init__(self, total=None):
            self.total, self.n, self.closed = total, 0, False
            bars.append(self)

        def update(self, by):
            self.n += by

        def close(self):
            self.closed = True

    monkeypatch.setitem(sys.modules, "tqdm", types.SimpleNamespace(tqdm=Bar))
    c = _cohort(10, 20, 3, 40, seed=33)
    G = _genotypes(c, seed=8)[:, :40]
    crms = _crms(c, _phenotypes(c, 3, seed=9), c.W, "B")
    cis = [(0, 30), (10, 36), np.array([38, 5])]     # five runs; variants 36, 37 and 39 are nobody's
    call = crm.scan_association_many if driver == "association" else crm.scan_interaction_contexts_many
    silent = call(crms, G, cis_index=cis, fast=True)
    shown = call(crms, G, cis_index=cis, fast=True, progress=True)
    assert len(bars) == 1 and bars[0].total == 37 and bars[0].n == 37 and bars[0].closed
    for a, b in zip(silent[0], shown[0]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("k", [9, 62, 70])
def test_run_association_many_wrapper(k, fast):
    """W goes to the contexts slot, E to the fixed effects (_cellregmap.py:498): k contexts are k covariate columns --
    the LDS (9), the 62-column and the 63..128-column (xwide) null-fit kernels, and both forms of the finishing kernel."""
    from cellregmap_amd import run_association, run_association_fast, run_association_many
    from oracle import crm as ocrm

    c = _cohort(12, 15, k, 10, seed=34)
    Y = _phenotypes(c, 3, seed=10)
    pv, info = run_association_many(Y, c.W, c.E, c.G, hK=c.hK, fast=fast)
    assert pv.shape == (3, c.G.shape[1])
    f, of = (run_association_fast, ocrm.run_association_fast) if fast else (run_association, ocrm.run_association)
    for i in range(3):
        spv, sinfo = f(Y[:, i], c.W, c.E, c.G, hK=c.hK)
        _close_p(pv[i], spv)
        assert_allclose(info["rho1"][i], sinfo["rho1"][0], rtol=1e-5, atol=1e-12)
    opv, oinfo = of(Y[:, 0], c.W, c.E, c.G, hK=c.hK)
    _close_p(pv[0], opv)


@pytest.mark.parametrize("fast", [False, True])
def test_donor_level_panels_equal_the_dense_panel(fast):
    from cellregmap_amd import GenotypePanel, scan_association_many

    c = _cohort(10, 20, 3, 24, seed=35)
    rng = np.random.default_rng(11)
    D = rng.integers(0, 3, size=(10, 24)).astype(np.int8)
    D[0] = 1   # (no monomorphic column)
    D[1] = 0
    D[2] = 2
    Gd = rng.normal(size=(10, 24))
    Y = _phenotypes(c, 4, seed=12)
    crms = _crms(c, Y, c.W, "B")
    dense_d = GenotypePanel(D[c.donor_of_cell].astype(float), groups=None)
    dense_g = GenotypePanel(Gd[c.donor_of_cell], groups=None)
    ref_d = scan_association_many(crms, dense_d, fast=fast, return_stats=True)
    ref_g = scan_association_many(crms, dense_g, fast=fast, return_stats=True)
    got_d = scan_association_many(crms, GenotypePanel.from_dosages(D, c.donor_of_cell, standardize=False), fast=fast,
                                  return_stats=True)
    got_g = scan_association_many(crms, GenotypePanel.from_donors(Gd, c.donor_of_cell), fast=fast, return_stats=True)
    for got, ref in ((got_d, ref_d), (got_g, ref_g)):
        _close_p(got[0], ref[0])
        assert np.all(np.abs(got[1]["alt_lml"] - ref[1]["alt_lml"]) <= 1e-10 * np.abs(ref[1]["null_lml"])[:, None])


def test_misuse_is_refused_with_a_message():
    from cellregmap_amd import CellRegMap, GenotypePanel, _lib, scan_association_many

    lib = _lib.load()
    c = _cohort(8, 10, 2, 6, seed=36)
    a = CellRegMap(c.y, c.E, W=c.W, hK=c.hK)
    b = CellRegMap(c.y + 1.0, 2.0 * c.E, W=c.W, hK=c.hK)   # its own background
    a._bind_gene()
    b._bind_gene()
    panel = GenotypePanel(c.G, groups=None)
    null = np.empty((2, 6))
    two = (ctypes.c_void_p * 2)(a._gene.value, b._gene.value)
    assert lib.crm_association_null_multi(two, 2, _lib.ptr(null)) == ERR_ARG
    assert b"background" in lib.crm_last_error()
    one = (ctypes.c_void_p * 1)(a._gene.value)
    row = np.empty((1, 6))
    assert lib.crm_association_null_multi(one, 1, _lib.ptr(row)) == 0
    pv = np.empty((2, 6))
    assert lib.crm_scan_association_multi(two, 2, panel.handle, 0, 6, 1, _lib.ptr(np.repeat(row, 2, 0)), _lib.ptr(pv),
                                          None) == ERR_ARG
    assert b"background" in lib.crm_last_error()
    off = row.copy()
    off[0, 0] = 0.123456   # not a grid point
    assert lib.crm_scan_association_multi(one, 1, panel.handle, 0, 6, 1, _lib.ptr(off), _lib.ptr(pv), None) == ERR_ARG
    assert b"grid" in lib.crm_last_error()
    bad = row.copy()
    bad[0, 4] = np.nan
    assert lib.crm_scan_association_multi(one, 1, panel.handle, 0, 6, 0, _lib.ptr(bad), _lib.ptr(pv), None) == ERR_ARG
    other = GenotypePanel(np.random.default_rng(0).normal(size=(c.y.size - 10, 6)), groups=None)
    assert lib.crm_scan_association_multi(one, 1, other.handle, 0, 6, 1, _lib.ptr(row), _lib.ptr(pv), None) == ERR_ARG
    assert b"cell count" in lib.crm_last_error()
    assert lib.crm_scan_association_multi(one, 1, panel.handle, 0, 7, 1, _lib.ptr(row), _lib.ptr(pv), None) == ERR_ARG
    # the context stays usable
    assert lib.crm_scan_association_multi(one, 1, panel.handle, 0, 6, 1, _lib.ptr(row), _lib.ptr(pv), None) == 0
    with pytest.raises(ValueError):
        scan_association_many([a, b], c.G)   # two backgrounds
    rng = np.random.default_rng(1)
    d = CellRegMap(c.y + 2.0, c.E, W=np.c_[c.W, rng.normal(size=c.y.size)], hK=c.hK, background=a._bg)
    with pytest.raises(ValueError):
        scan_association_many([a, d], c.G)   # another W
    e = CellRegMap(c.y + 3.0, c.E + 1.0, W=c.W, hK=c.hK, background=a._bg)
    with pytest.raises(ValueError):
        scan_association_many([a, e], c.G)   # another E


def test_config3_sized_fast_pass():
    """100 donors x 200 cells, 64 phenotypes, 4 096 variants (fast): every row against the single-phenotype path."""
    from cellregmap_amd import CellRegMap, scan_association_many

    c = _cohort(100, 200, 10, 64, seed=37)
    rng = np.random.default_rng(13)
    n = c.y.size
    G = np.concatenate([np.repeat(c.G, 32, axis=1)[:, :2048], rng.normal(size=(n, 2048))], axis=1)
    Y = np.stack([c.y] + [c.y * rng.uniform(0, 1) + rng.normal(size=n) for _ in range(63)], axis=1)
    first = CellRegMap(Y[:, 0], c.W, c.E, hK=c.hK)   # run_association's binding: 10 contexts as covariates
    crms = [first] + [CellRegMap(Y[:, i], c.W, c.E, hK=c.hK, background=first._bg) for i in range(1, 64)]
    pv, info = scan_association_many(crms, G, fast=True, return_stats=True)
    for i in range(64):
        spv, sinfo, sst = crms[i].scan_association_fast(G, return_stats=True)
        assert info["null_lml"][i] == sst["null_lml"] and info["rho1"][i] == sinfo["rho1"][0]
        _close_p(pv[i], spv)
        assert np.all(np.abs(info["alt_lml"][i] - sst["alt_lml"]) <= 1e-10 * abs(sst["null_lml"]))
