"""The unrelated-donor form's rotated S straight from the per-donor pair products (blockops.hip: donor_pairs_rotate_kernel)
against the two launches it replaces (form ``donor_pairs_rotate`` = 0: the rows of S, then the per-donor rotation product).
The rotated S is the same bit for bit and so are the donor sums, so every result of the scan is too; the oracle holds the
new form at the north-star tolerances."""
import numpy as np
import pytest

import parity_bounds
from test_gpu_unrelated_donors import _blocks, _ragged, _route

pytestmark = pytest.mark.gpu


def _pair_blocks():
    from cellregmap_amd import _engine, _lib

    return _lib.load().crm_test_donor_pair_blocks(_engine._context(0))


def _scan_both(kernel_form, run):
    """`run()` with the pair form of the unrelated-donor route forced, once with the one-pass rotation and once with the two
    launches; both must have served the form."""
    out = []
    with _route(kernel_form, 2):
        kernel_form("donor_pairs", 2)
        for rotate in (1, 0):
            kernel_form("donor_pairs_rotate", rotate)
            before, pairs = _blocks(), _pair_blocks()
            out.append(run())
            assert _blocks() > before and _pair_blocks() > pairs
    return out


def _equal(a, b):
    pv, info, st = a
    pv0, info0, st0 = b
    assert np.array_equal(pv, pv0)
    for k in info0:
        assert np.array_equal(info[k], info0[k]), k
    assert np.array_equal(st["Q"], st0["Q"])
    assert np.array_equal(st["F"], st0["F"])


@pytest.mark.parametrize("donors,cells,k0,variants", [
    (7, 60, 5, 37),      # k2 = 5: 13 Gram rows; a partial last group of four variants
    (12, 40, 20, 70),
    (8, 60, 40, 41),     # 83 Gram rows
    (5, 120, 50, 18),    # k2 = 50: 103 Gram rows, as the large configurations
    (4, 120, 54, 9),     # k2 = 54: 14 k-steps, the largest k0 the one-pass form serves
])
def test_rotation_from_pairs_equals_the_two_launches(donors, cells, k0, variants, kernel_form):
    import cellregmap_amd as crm
    from oracle import crm as ocrm

    c, keep, G = _ragged(donors, cells, k0, variants, 700 + k0)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    obj = [None]

    def run():
        obj[0] = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        return obj[0].scan_interaction(crm.GenotypePanel(G, groups=None), return_stats=True)

    new, old = _scan_both(kernel_form, run)
    _equal(new, old)
    if k0 <= 20:
        with _route(kernel_form, 2):
            kernel_form("donor_pairs", 2)
            bp = parity_bounds.bounds(obj[0], crm.GenotypePanel(G, groups=None))[1]
        sel = np.arange(0, variants, max(1, variants // 6))
        opv, _ = ocrm.OracleCellRegMap(y, E, W=W, Ls=ocrm.khatri_rao_halves(hK, E)).scan_interaction(G[:, sel])
        parity_bounds.assert_p_within(new[0][sel], opv, bp[sel])


def test_rotation_from_pairs_with_a_null_variant_and_exact_p(kernel_form):
    """A constant variant (its direction drops out: the A_none row) beside ordinary ones; exact tail p-values."""
    import cellregmap_amd as crm

    c, keep, G = _ragged(8, 40, 6, 21, 29)
    G = G.copy()
    G[:, 4] = 1.0
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    new, old = _scan_both(kernel_form, lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E)).scan_interaction(
        crm.GenotypePanel(G, groups=None), return_stats=True, pvalue="exact"))
    _equal(new, old)


def test_rotation_from_pairs_info_calls(kernel_form):
    """scan_interaction_info: the flat-optimum probes assemble twice more from the same rotated S."""
    import cellregmap_amd as crm

    c, keep, G = _ragged(8, 40, 5, 40, 17)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    (pv, xi), (pv0, xi0) = _scan_both(kernel_form, lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
                                      .scan_interaction_info(crm.GenotypePanel(G, groups=None)))
    assert np.array_equal(pv, pv0)
    for k in xi0:
        assert np.array_equal(np.asarray(xi[k]), np.asarray(xi0[k])), k


def test_rotation_from_pairs_permutation_replay(kernel_form):
    """Genotype permutations in one call (the context permutations leave the pair form: E1 is no longer the contexts)."""
    import cellregmap_amd as crm

    c, keep, G = _ragged(10, 24, 4, 29, 53)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    rng = np.random.default_rng(8)
    perms = [rng.permutation(y.size) for _ in range(3)]
    (pv, info, Q), (pv0, info0, Q0) = _scan_both(kernel_form, lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
                                                 .scan_interaction_permutations(crm.GenotypePanel(G, groups=None),
                                                                                return_Q=True, idx_G_list=perms))
    assert np.array_equal(pv, pv0) and np.array_equal(Q, Q0)
    for k in info0:
        assert np.array_equal(info[k], info0[k]), k


def test_rotation_from_pairs_many_phenotypes(kernel_form):
    """Several phenotypes: the columns are block positions (d_posw), not pairs."""
    from cellregmap_amd import CellRegMap, GenotypePanel, get_L_values, scan_interaction_many

    c, keep, G = _ragged(8, 30, 4, 70, 41)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    rng = np.random.default_rng(7)
    Y = np.stack([y, rng.normal(size=y.size), y + rng.normal(size=y.size)], axis=1)

    def run():
        Ls = get_L_values(hK, E)
        first = CellRegMap(Y[:, 0], E, W=W, Ls=Ls)
        crms = [first] + [CellRegMap(Y[:, i], E, W=W, Ls=Ls, background=first._bg) for i in range(1, 3)]
        return scan_interaction_many(crms, GenotypePanel(G, groups=None))

    (pv, info), (pv0, info0) = _scan_both(kernel_form, run)
    assert np.array_equal(pv, pv0)
    for k in info0:
        assert np.array_equal(info[k], info0[k]), k


def test_gene_constants_are_kept_between_scans(kernel_form):
    """Phi'[y, W] and E1'[y, W] are formed on a gene's first scan and reused: a second scan of the same object gives the
    same bits as the first, and a fresh object the same as both."""
    import cellregmap_amd as crm

    c, keep, G = _ragged(9, 40, 6, 33, 11)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    with _route(kernel_form, 2):
        obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        panel = crm.GenotypePanel(G, groups=None)
        before = _blocks()
        runs = [obj.scan_interaction(panel, return_stats=True) for _ in range(2)]
        runs.append(crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E)).scan_interaction(panel, return_stats=True))
        assert _blocks() > before
    _equal(runs[1], runs[0])
    _equal(runs[2], runs[0])
