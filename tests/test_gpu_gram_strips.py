"""The strip deal of the 65-144-row direct-to-LDS Gram kernels (tile_gram.h: kStripDeal; form ``gram_strips``, the default)
against the round-robin deal they had (``gram_strips`` = 0), in wb_gram_fused_kernel and in gram_ext_dma_wide_kernel.  A
wavefront owns whole columns of the upper triangle of 16 x 16 tiles, reads every operand tile row once per k-step and
weights one fragment per column; every accumulator still receives the same operands in the same k order, so p, Q, F, lml,
delta, the scale and every info array are the same BITS with the form on, with it off, and -- on the unrelated-donor pair
route -- with the two launches that the fused kernel replaces (``wb_gram_fused`` = 0: the rotated S through memory, then
gram_ext_dma_wide_kernel, itself under the strip deal).  ``crm_test_wb_gram_fused_blocks`` moves where it did: with
``wb_gram_fused`` on, whatever the deal.

The shapes are the smallest that reach every tile-row count (5 to 8 in the fused kernel, 5 to 9 in the wide one), every
chunk length of the fused walk (k0 = 0 and 2 mod 4, odd and even donor counts) and every value of k0 mod 16.  The file
also passes under CRM_POISON=1 (fresh device buffers filled with 0xFF, a red zone behind each): no overrun, the same bits."""
import ctypes

import numpy as np
import pytest

from test_gpu_gram_wide import _covariates, _dma_launches
from test_gpu_unrelated_donors import _blocks, _ragged, _route

pytestmark = pytest.mark.gpu

STATS = ("Q", "F", "lml", "delta", "scale")


def _fused():
    from cellregmap_amd import _engine, _lib

    out = ctypes.c_long(-1)
    _lib.check(_lib.load().crm_test_wb_gram_fused_blocks(_engine._context(0), ctypes.byref(out)))
    return out.value


def _same(a, b, what):
    pv, info, st = a
    pv0, info0, st0 = b
    assert np.all(np.isfinite(pv0)) and np.all(np.isfinite(st0["Q"])) and np.all(np.isfinite(st0["F"])), what
    assert np.array_equal(pv, pv0), what
    assert set(info) == set(info0), what
    for k in info0:
        assert np.array_equal(info[k], info0[k]), (what, k)
    for k in STATS:
        assert np.array_equal(st[k], st0[k]), (what, k)


def _three_runs(kernel_form, run):
    """`run()` on the forced unrelated-donor pair route: strips on, strips off, the two launches -- these under either deal
    of gram_ext_dma_wide_kernel; all the same bits, the fused counter moving for the first two only."""
    out = []
    with _route(kernel_form, 2):
        kernel_form("donor_pairs", 2)
        for strips, fused in ((1, 1), (0, 1), (1, 0), (0, 0)):
            kernel_form("gram_strips", strips)
            kernel_form("wb_gram_fused", fused)
            before, blocks = _fused(), _blocks()
            out.append(run())
            assert _blocks() > blocks
            assert (_fused() > before) == (fused == 1), (strips, fused, _fused() - before)
    on, off, two, two_off = out
    _same(two, two_off, "the two launches, strips on against off")
    _same(on, off, "strips on against off")
    _same(on, two, "strips on against the two launches")
    _same(off, two, "strips off against the two launches")


# Gram rows = 2 k0 + c + 2, donors, cells, k0, variants, covariate columns (0: the cohort's own intercept)
@pytest.mark.parametrize("rows,donors,cells,k0,variants,cov", [
    (67, 4, 70, 32, 10, 0),      # 67 rows, 5 tile rows; k0 = 0 mod 16
    (71, 3, 60, 34, 9, 0),       # 71 rows, 5 tile rows; k0 = 2 mod 16 and 2 mod 4, an odd donor count
    (75, 2, 80, 36, 7, 0),       # 75 rows, 5 tile rows; k0 = 4 mod 16 and 0 mod 4, two donors
    (83, 8, 60, 40, 41, 0),      # 83 rows, 6 tile rows; k0 = 8 mod 16
    (85, 5, 80, 40, 11, 3),      # 85 rows, 6 tile rows; three covariate columns
    (99, 4, 100, 48, 10, 0),     # 99 rows, 7 tile rows; k0 = 0 mod 16
    (103, 5, 120, 50, 18, 0),     # 103 rows, 7 tile rows: the large configuration's shape
    (107, 4, 110, 52, 9, 0),      # 107 rows, 7 tile rows; k0 = 4 mod 16
    (111, 4, 120, 54, 9, 0),      # 111 rows, 7 tile rows; k0 = 6 mod 16, the longest chunk (14 k-steps)
    (118, 4, 120, 54, 9, 8),      # 118 rows, 8 tile rows: one workgroup per CU
])
def test_strips_equal_round_robin_and_the_two_launches(rows, donors, cells, k0, variants, cov, kernel_form):
    import cellregmap_amd as crm

    c, keep, G = _ragged(donors, cells, k0, variants, 800 + k0)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    if cov:
        W = _covariates(y.size, cov, k0)
    assert rows == 2 * k0 + W.shape[1] + 2
    _three_runs(kernel_form, lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E)).scan_interaction(
        crm.GenotypePanel(G, groups=None), return_stats=True))


def test_strips_with_a_null_variant_and_exact_p(kernel_form):
    """A constant variant (has_A false: rows of zeros, the donor sums still formed) beside ordinary ones, exact tails."""
    import cellregmap_amd as crm

    c, keep, G = _ragged(4, 70, 32, 10, 31)
    G = G.copy()
    G[:, 4] = 1.0
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    _three_runs(kernel_form, lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E)).scan_interaction(
        crm.GenotypePanel(G, groups=None), return_stats=True, pvalue="exact"))


def test_strips_with_a_donor_of_fewer_cells_than_contexts(kernel_form):
    """One donor cut to 9 cells under 32 contexts: 23 of its positions are zero columns of Psi with a zero spectrum entry."""
    import cellregmap_amd as crm
    from cellregmap_amd.synth import make_cohort

    donors, cells, k0, variants = 5, 70, 32, 12
    c = make_cohort(donors, cells, k0, variants, seed=91)
    donor = np.repeat(np.arange(donors), cells)
    keep = np.ones(donors * cells, bool)
    keep[np.flatnonzero(donor == 2)[9:]] = False
    G = c.G[keep] + 0.05 * np.random.default_rng(91).normal(size=c.G[keep].shape)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    _three_runs(kernel_form, lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E)).scan_interaction(
        crm.GenotypePanel(G, groups=None), return_stats=True))


@pytest.mark.parametrize("k0", [32, 50])
def test_wide_gram_strips_with_three_phenotypes(k0, kernel_form):
    """Three phenotypes run a Gram each over the same rotated S: gram_ext_dma_wide_kernel (the fused form does not serve
    them), 67 and 103 rows."""
    from cellregmap_amd import CellRegMap, GenotypePanel, get_L_values, scan_interaction_many

    c, keep, G = _ragged(4, 70, 32, 10, 41) if k0 == 32 else _ragged(5, 120, 50, 18, 850)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    rng = np.random.default_rng(7)
    Y = np.stack([y, rng.normal(size=y.size), y + rng.normal(size=y.size)], axis=1)

    def run():
        Ls = get_L_values(hK, E)
        first = CellRegMap(Y[:, 0], E, W=W, Ls=Ls)
        crms = [first] + [CellRegMap(Y[:, i], E, W=W, Ls=Ls, background=first._bg) for i in range(1, 3)]
        return scan_interaction_many(crms, GenotypePanel(G, groups=None))

    out = []
    with _route(kernel_form, 2):
        kernel_form("donor_pairs", 2)
        for strips in (1, 0):
            kernel_form("gram_strips", strips)
            fused, dma, blocks = _fused(), _dma_launches(), _blocks()
            out.append(run())
            assert _blocks() > blocks and _dma_launches() > dma and _fused() == fused
    (pv, info), (pv0, info0) = out
    assert np.all(np.isfinite(pv0)) and np.array_equal(pv, pv0)
    for k in info0:
        assert np.array_equal(info[k], info0[k]), k


def test_wide_gram_strips_at_nine_tile_rows(kernel_form):
    """144 rows (k0 = 64, 14 covariate columns; past the pair form's 54 contexts the route runs without it): the only
    tile-row count at which the roles hold different numbers of tiles twice over (12, 11, 11, 11)."""
    import cellregmap_amd as crm

    rows, donors, cells, k0, c, variants = 144, 4, 150, 64, 14, 6
    co, keep, G = _ragged(donors, cells, k0, variants, 900 + rows)
    y, E, hK = co.y[keep], co.E[keep], co.hK[keep]
    W = _covariates(y.size, c, rows)
    out = []
    with _route(kernel_form, 2):
        kernel_form("donor_pairs", 0)
        obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        for strips in (1, 0):
            kernel_form("gram_strips", strips)
            dma, blocks = _dma_launches(), _blocks()
            out.append(obj.scan_interaction(crm.GenotypePanel(G, groups=None), return_stats=True))
            assert _blocks() > blocks and _dma_launches() > dma
    _same(out[0], out[1], "strips on against off, 9 tile rows")
