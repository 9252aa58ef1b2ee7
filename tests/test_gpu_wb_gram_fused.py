"""The unrelated-donor Gram straight from the per-donor pair products (wb_gram_fused.hip: the rotated S stays in LDS)
against the two launches it replaces (form ``wb_gram_fused`` = 0: donor_pairs_rotate_kernel, the rotated S in memory,
gram_ext_dma_wide_kernel).  The fused kernel walks the donors in chunks that end at multiples of four positions, so every
group of four that the Gram's accumulators take is the two launches' group: Q, F and p are the same bits, and rho*, delta, lml
and scale never pass through it.  ``crm_test_wb_gram_fused_blocks`` says where the form served: one phenotype, no model
flags, no permutation replay, an even context count and a Gram of 65 to 128 rows."""
import ctypes

import numpy as np
import pytest

import parity_bounds
from test_gpu_gram_wide import _covariates
from test_gpu_unrelated_donors import _blocks, _ragged, _route

pytestmark = pytest.mark.gpu


def _fused():
    from cellregmap_amd import _engine, _lib

    out = ctypes.c_long(-1)
    _lib.check(_lib.load().crm_test_wb_gram_fused_blocks(_engine._context(0), ctypes.byref(out)))
    return out.value


def _scan_both(kernel_form, run, serves):
    """`run()` on the forced unrelated-donor route with the pair form, fused and with the two launches; the counter moves
    with the form on, and only where it should serve."""
    out = []
    with _route(kernel_form, 2):
        kernel_form("donor_pairs", 2)
        for fused in (1, 0):
            kernel_form("wb_gram_fused", fused)
            before, blocks = _fused(), _blocks()
            out.append(run())
            assert _blocks() > blocks
            assert (_fused() > before) == (serves and fused == 1), (fused, serves, _fused() - before)
    return out


def _equal(a, b):
    pv, info, st = a
    pv0, info0, st0 = b
    for k in info0:
        assert np.array_equal(info[k], info0[k]), k
    for k in ("lml", "delta", "scale"):
        assert np.array_equal(st[k], st0[k]), k
    scale = np.maximum(np.abs(st0["Q"]), np.trace(st0["F"], axis1=1, axis2=2))
    print("fused against the two launches: max |dQ| / scale %.3g, max |dF| / scale %.3g, max |dp| / p %.3g"
          % (np.max(np.abs(st["Q"] - st0["Q"]) / scale), np.max(np.abs(st["F"] - st0["F"]) / scale[:, None, None]),
             np.max(np.abs(pv - pv0) / np.maximum(pv0, 1e-300))))
    assert np.all(np.isfinite(pv)) and np.all(np.isfinite(st["Q"])) and np.all(np.isfinite(st["F"]))
    assert np.array_equal(st["Q"], st0["Q"])
    assert np.array_equal(st["F"], st0["F"])
    assert np.array_equal(pv, pv0)


@pytest.mark.parametrize("donors,cells,k0,variants,cov,serves", [
    (5, 120, 50, 18, 0, True),     # 103 rows; an odd donor count: the last chunk ends in two columns of zeros
    (8, 60, 40, 41, 0, True),      # 83 rows; k0 = 0 mod 4: every chunk is the donor's own positions
    (4, 120, 54, 9, 0, True),      # 111 rows: the largest k0 of the pair rotation, one workgroup per CU
    (5, 80, 40, 11, 3, True),      # three covariate columns: 85 rows, 6 tile rows
    (4, 70, 32, 10, 0, True),      # 67 rows: the smallest Gram it serves; held to the oracle
    (7, 60, 5, 37, 0, False),      # 13 rows: the two launches, counter unchanged
    (4, 100, 47, 10, 0, False),    # an odd context count: the two launches
])
def test_fused_gram_equals_the_two_launches(donors, cells, k0, variants, cov, serves, kernel_form):
    import cellregmap_amd as crm
    from oracle import crm as ocrm

    c, keep, G = _ragged(donors, cells, k0, variants, 800 + k0)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    if cov:
        W = _covariates(y.size, cov, k0)
    obj = [None]

    def run():
        obj[0] = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        return obj[0].scan_interaction(crm.GenotypePanel(G, groups=None), return_stats=True)

    new, old = _scan_both(kernel_form, run, serves)
    _equal(new, old)
    if k0 == 32:
        with _route(kernel_form, 2):
            kernel_form("donor_pairs", 2)
            bp = parity_bounds.bounds(obj[0], crm.GenotypePanel(G, groups=None))[1]
        sel = np.arange(0, variants, max(1, variants // 4))
        opv, _ = ocrm.OracleCellRegMap(y, E, W=W, Ls=ocrm.khatri_rao_halves(hK, E)).scan_interaction(G[:, sel])
        parity_bounds.assert_p_within(new[0][sel], opv, bp[sel])


def test_fused_gram_with_a_donor_of_fewer_cells_than_contexts(kernel_form):
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
    new, old = _scan_both(kernel_form, lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E)).scan_interaction(
        crm.GenotypePanel(G, groups=None), return_stats=True), True)
    _equal(new, old)


def test_fused_gram_with_a_null_variant_and_exact_p(kernel_form):
    """A constant variant (no kinship term to test: rows of zeros, the donor sums still formed) beside ordinary ones."""
    import cellregmap_amd as crm

    c, keep, G = _ragged(4, 70, 32, 10, 31)
    G = G.copy()
    G[:, 4] = 1.0
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    new, old = _scan_both(kernel_form, lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E)).scan_interaction(
        crm.GenotypePanel(G, groups=None), return_stats=True, pvalue="exact"), True)
    _equal(new, old)


def test_info_calls_keep_the_two_launches(kernel_form):
    """scan_interaction_info: the flat-optimum probes assemble twice more from the rotated S, which must exist."""
    import cellregmap_amd as crm

    c, keep, G = _ragged(4, 70, 32, 10, 17)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    (pv, xi), (pv0, xi0) = _scan_both(kernel_form, lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
                                      .scan_interaction_info(crm.GenotypePanel(G, groups=None)), False)
    assert np.array_equal(pv, pv0)
    for k in xi0:
        assert np.array_equal(np.asarray(xi[k]), np.asarray(xi0[k])), k


def test_permutation_replay_keeps_the_two_launches(kernel_form):
    import cellregmap_amd as crm

    c, keep, G = _ragged(4, 70, 32, 10, 53)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    rng = np.random.default_rng(8)
    perms = [rng.permutation(y.size) for _ in range(2)]
    (pv, info, Q), (pv0, info0, Q0) = _scan_both(kernel_form, lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
                                                 .scan_interaction_permutations(crm.GenotypePanel(G, groups=None),
                                                                                return_Q=True, idx_G_list=perms), False)
    assert np.array_equal(pv, pv0) and np.array_equal(Q, Q0)
    for k in info0:
        assert np.array_equal(info[k], info0[k]), k


def test_several_phenotypes_keep_the_two_launches(kernel_form):
    """Three phenotypes run a Gram each over the same rotated S."""
    from cellregmap_amd import CellRegMap, GenotypePanel, get_L_values, scan_interaction_many

    c, keep, G = _ragged(4, 70, 32, 10, 41)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    rng = np.random.default_rng(7)
    Y = np.stack([y, rng.normal(size=y.size), y + rng.normal(size=y.size)], axis=1)

    def run():
        Ls = get_L_values(hK, E)
        first = CellRegMap(Y[:, 0], E, W=W, Ls=Ls)
        crms = [first] + [CellRegMap(Y[:, i], E, W=W, Ls=Ls, background=first._bg) for i in range(1, 3)]
        return scan_interaction_many(crms, GenotypePanel(G, groups=None))

    (pv, info), (pv0, info0) = _scan_both(kernel_form, run, False)
    assert np.array_equal(pv, pv0)
    for k in info0:
        assert np.array_equal(info[k], info0[k]), k
