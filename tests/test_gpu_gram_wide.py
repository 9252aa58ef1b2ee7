"""The score-statistic Gram for 65 to 144 rows through direct-to-LDS loads (gram_ext.hip: gram_ext_dma_wide_kernel, 5 to 9
rows of 16 x 16 tiles dealt to the four wavefronts) against the register-staged kernel (form ``gram_staged`` = 1), at the
tolerances of test_gpu_edges.py::test_gram_kernel_forms_agree: Q within 1e-11 max(|Q|, tr F), F within 1e-11 max|F|, p
within 1e-6 relative + 1e-13.  The null fits do not read the Gram: rho* and the other outputs are the same bits.  Every
case asserts through crm_test_gram_dma_launches that the direct-to-LDS form served the default scan and not the staged
one.

This file holds the two forms against each other only; what both share (the orthogonalisation against W, the mixing
matrices, the finalisation) is held against an independent extended-precision reference, at the same parameter rows and both
forms, by tests/test_gpu_pinned.py::test_gram_forms."""
import ctypes

import numpy as np
import pytest

from test_gpu_unrelated_donors import _blocks, _ragged, _route

pytestmark = pytest.mark.gpu


def _dma_launches():
    from cellregmap_amd import _engine, _lib

    out = ctypes.c_long(-1)
    _lib.check(_lib.load().crm_test_gram_dma_launches(_engine._context(0), ctypes.byref(out)))
    return out.value


def _pair_blocks():
    from cellregmap_amd import _engine, _lib

    return _lib.load().crm_test_donor_pair_blocks(_engine._context(0))


def _without_pair():
    from cellregmap_amd import _engine, _lib

    return _lib.load().crm_test_tests_without_pair(_engine._context(0))


def _covariates(n, c, seed):
    """c covariate columns, the first one the intercept."""
    return np.column_stack([np.ones(n), np.random.default_rng(seed).normal(size=(n, c - 1))])


def _forms_agree(kernel_form, obj, panel, **kw):
    """Default scan, then the staged form: the counter moves only for the first, the statistics agree to rounding.
    Returns the number of tests of the default scan that had no position (crm_test_tests_without_pair)."""
    before, none_before = _dma_launches(), _without_pair()
    pv, info, st = obj.scan_interaction(panel, return_stats=True, **kw)
    served, without_position = _dma_launches(), _without_pair() - none_before
    assert served > before, "the default scan did not go through a direct-to-LDS Gram"
    kernel_form("gram_staged", 1)
    pv2, info2, st2 = obj.scan_interaction(panel, return_stats=True, **kw)
    assert _dma_launches() == served, "the staged form went through a direct-to-LDS Gram"
    kernel_form("gram_staged", 0, reset=True)
    for k in ("rho1", "e2", "g2", "eps2"):
        assert np.array_equal(info[k], info2[k]), k
    for k in ("lml", "delta"):
        assert np.array_equal(st[k], st2[k]), k
    dq = np.abs(st["Q"] - st2["Q"])
    scale = np.maximum(np.abs(st2["Q"]), np.trace(st2["F"], axis1=1, axis2=2))
    fs = np.abs(st2["F"]).max(axis=(1, 2), keepdims=True)
    df = np.abs(st["F"] - st2["F"])
    print("gram forms: max dQ / scale %.3g, max dF / max|F| %.3g, max dp / p %.3g"
          % (np.max(dq / scale), np.max(df / fs), np.max(np.abs(pv - pv2) / np.maximum(pv2, 1e-300))))
    assert np.all(np.isfinite(st["Q"])) and np.all(np.isfinite(st["F"]))
    assert np.all(dq <= 1e-11 * scale)
    assert np.all(df <= 1e-11 * fs)
    assert np.all(np.abs(pv - pv2) <= 1e-6 * pv2 + 1e-13)
    return without_position


# rows = 2 k0 + c + 2 on the unrelated-donor route, over a spectrum of donors x k0 entries (chunks of 32): every tile-row
# count from 5 to 9 at both of its edges.  The pair form serves k0 <= 54; past that the route runs without it.
@pytest.mark.parametrize("rows,donors,cells,k0,c,variants", [
    (65, 5, 70, 31, 1, 13),        # 5 tile rows; 155 spectrum entries: four chunks and 27
    (67, 4, 70, 32, 1, 10),        # 128 entries: whole chunks only
    (80, 4, 80, 38, 2, 9),
    (81, 5, 80, 39, 1, 11),        # 6 tile rows
    (96, 4, 100, 46, 2, 9),
    (97, 4, 100, 47, 1, 10),       # 7 tile rows
    (99, 4, 100, 48, 1, 9),        # 192 entries: whole chunks only
    (103, 5, 120, 50, 1, 18),      # the large configurations: 50 + 3 + 50
    (112, 4, 120, 54, 2, 9),
    (113, 4, 120, 54, 3, 9),       # 8 tile rows
    (128, 4, 150, 62, 2, 7),
    (129, 4, 150, 63, 1, 7),       # 9 tile rows
    (144, 4, 150, 64, 14, 6),      # (the form serves up to 64 contexts in the kinship term)
])
def test_wide_gram_forms_agree_on_the_unrelated_donor_route(rows, donors, cells, k0, c, variants, kernel_form):
    import cellregmap_amd as crm

    assert rows == 2 * k0 + c + 2
    co, keep, G = _ragged(donors, cells, k0, variants, 900 + rows)
    y, E, hK = co.y[keep], co.E[keep], co.hK[keep]
    W = _covariates(y.size, c, rows)
    pairs = k0 <= 54
    with _route(kernel_form, 2):
        kernel_form("donor_pairs", 2 if pairs else 0)
        obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        before, pair_before = _blocks(), _pair_blocks()
        _forms_agree(kernel_form, obj, crm.GenotypePanel(G, groups=None))
        assert _blocks() > before                                # the route under test ran ...
        assert (_pair_blocks() > pair_before) == pairs           # ... in the form the case names


def test_wide_gram_with_a_spectrum_shorter_than_a_chunk(kernel_form):
    """hK without Ls on the unrelated-donor route: one spectrum entry per donor (9 < 32: no whole chunk at all), 83 rows."""
    import cellregmap_amd as crm

    co, keep, G = _ragged(9, 90, 40, 14, 77)
    y, E, W, hK = co.y[keep], co.E[keep], co.W[keep], co.hK[keep]
    with _route(kernel_form, 2):
        obj = crm.CellRegMap(y, E, W=W, hK=hK)
        before = _blocks()
        _forms_agree(kernel_form, obj, crm.GenotypePanel(G, groups=None))
        assert _blocks() > before


def _flat_phenotype(y, seed):
    """The phenotype with its cells permuted: no random effect is left, the null fits end at the upper clamp of delta and
    such a test gets no rotated test direction (scan.hip: no_kinship_term) -- position -1, the Gram reads the row of zeros
    with stride 0 (A_none) for its first k0 rows."""
    return y[np.random.default_rng(seed).permutation(y.size)]


def test_wide_gram_without_a_test_direction_on_the_unrelated_donor_route(kernel_form):
    """103 rows, tests without a position (A_none) beside ordinary ones (whether a fit ends at the clamp is the phenotype's
    affair and nearly the same for every variant: cohort and permutation are ones where both kinds occur, 48 of 64)."""
    import cellregmap_amd as crm

    co, keep, G = _ragged(5, 300, 50, 64, 31)
    y, E, W, hK = co.y[keep], co.E[keep], co.W[keep], co.hK[keep]
    with _route(kernel_form, 2):
        kernel_form("donor_pairs", 2)
        obj = crm.CellRegMap(_flat_phenotype(y, 6), E, W=W, Ls=crm.get_L_values(hK, E))
        before = _blocks()
        skipped = _forms_agree(kernel_form, obj, crm.GenotypePanel(G, groups=None))
        assert _blocks() > before
        print("tests without a position in the default scan: %d of 64" % skipped)
        assert 0 < skipped < 64               # the direct-to-LDS Gram met positions of -1 beside real ones


def test_wide_gram_without_a_test_direction_on_the_plain_route(kernel_form):
    """73 rows (hK=, k0 = 70), tests without a position (A_none) beside ordinary ones (18 of 64 on this cohort)."""
    import cellregmap_amd as crm
    from cellregmap_amd.synth import make_cohort

    co = make_cohort(8, 120, 70, 64, seed=17)
    G = co.G + 0.05 * np.random.default_rng(2).normal(size=co.G.shape)
    obj = crm.CellRegMap(_flat_phenotype(co.y, 6), co.E, W=co.W, hK=co.hK)
    skipped = _forms_agree(kernel_form, obj, crm.GenotypePanel(G, groups=None))
    print("tests without a position in the default scan: %d of 64" % skipped)
    assert 0 < skipped < 64


@pytest.mark.parametrize("k0,c", [(70, 1), (61, 2), (76, 3)])
def test_wide_gram_on_the_plain_route(k0, c, kernel_form):
    """k0 + c + 2 = 73, 65 and 81 rows with the contraction against Q0(rho*) itself (hK=, the route the library chooses)."""
    import cellregmap_amd as crm
    from cellregmap_amd.synth import make_cohort

    co = make_cohort(10, 30, k0, 12, seed=17)
    W = _covariates(co.y.size, c, k0)
    obj = crm.CellRegMap(co.y, co.E, W=W, hK=co.hK)
    _forms_agree(kernel_form, obj, crm.GenotypePanel(co.G, groups=None))


def test_wide_gram_on_the_mixk_route(kernel_form):
    """73 rows on the kinship-structure route without the unrelated-donor form (A~ = MixK(rho*)'S)."""
    import cellregmap_amd as crm

    co, keep, G = _ragged(4, 160, 70, 9, 5)
    y, E, W, hK = co.y[keep], co.E[keep], co.W[keep], co.hK[keep]
    with _route(kernel_form, 0):
        obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        before = _blocks()
        _forms_agree(kernel_form, obj, crm.GenotypePanel(G, groups=None))
        assert _blocks() == before
