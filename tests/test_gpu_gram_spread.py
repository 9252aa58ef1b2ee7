"""The fused unrelated-donor Gram with a donor's LDS-DMA instructions issued among the MFMAs (wb_gram_fused.hip; form
``wb_gram_spread``, the default) against the same kernel with every piece in a bunch behind the barrier that frees its
buffer (``wb_gram_spread`` = 0).  Only the place of the load instructions in a wavefront's stream differs: which barrier
frees a piece's buffer, which one waits for it and what every accumulator receives are the same, so p, Q, F, lml, delta,
the scale and every info array are the same BITS with the form on, with it off and with the two launches that the fused
kernel replaces (``wb_gram_fused`` = 0), under the strip deal (``gram_strips`` = 1) and under the round-robin deal
(``gram_strips`` = 0, whose Gram phase keeps its pieces in a bunch whatever ``wb_gram_spread`` says).
``crm_test_wb_gram_fused_blocks`` moves only with ``wb_gram_fused`` on.

The shapes are the smallest that reach every corner of the placement: more pieces than k-steps (k0 = 32: 7 or 8 Gram
k-steps, up to 10 pieces of P and Psi per wavefront) with wavefronts that rotate nothing but still own pieces (JT = 2);
chunks of k0 - 2 and k0 + 2 positions and an odd donor count; two donors (one Gram phase that carries pieces, one that
has nothing to bring in -- a cohort of ONE donor cannot be made: cellregmap_amd.synth.make_cohort resamples donor-level
genotype columns that are constant, with one donor every column is, and the draw never ends; two is the smallest count
that takes the route); the large configuration's 103 rows; the longest chunk (14 k-steps); 8 tile rows (one workgroup per CU); variants without
a kinship term (no rotation at all: every wavefront issues its other rows in a bunch) beside ordinary ones.  The file
also passes under CRM_POISON=1 (fresh device buffers filled with 0xFF, a red zone behind each): no overrun, the same bits."""
import numpy as np
import pytest

from test_gpu_gram_strips import _fused, _same
from test_gpu_gram_wide import _covariates, _flat_phenotype, _without_pair
from test_gpu_unrelated_donors import _blocks, _ragged, _route

pytestmark = pytest.mark.gpu


def _forms_agree(kernel_form, make):
    """``make()`` builds (object, panel, scan keywords) on the forced unrelated-donor pair route; the scan under
    (gram_strips, wb_gram_spread, wb_gram_fused) = (1, 1, 1), (1, 0, 1), (1, ., 0), (0, 1, 1), (0, 0, 1), (0, ., 0): all the
    same bits, the fused counter moving with wb_gram_fused alone.  Returns how many tests of one scan had no kinship term."""
    out = {}
    with _route(kernel_form, 2):
        kernel_form("donor_pairs", 2)
        obj, panel, kw = make()
        for strips in (1, 0):
            kernel_form("gram_strips", strips)
            for spread, fused in ((1, 1), (0, 1), (1, 0)):
                kernel_form("wb_gram_spread", spread)
                kernel_form("wb_gram_fused", fused)
                before, blocks, none = _fused(), _blocks(), _without_pair()
                out[strips, spread, fused] = obj.scan_interaction(panel, return_stats=True, **kw)
                assert _blocks() > blocks
                assert (_fused() > before) == (fused == 1), (strips, spread, fused, _fused() - before)
                without = _without_pair() - none
    for strips in (1, 0):
        _same(out[strips, 1, 1], out[strips, 0, 1], "spread on against off, gram_strips = %d" % strips)
        _same(out[strips, 1, 1], out[strips, 1, 0], "spread on against the two launches, gram_strips = %d" % strips)
        _same(out[strips, 0, 1], out[strips, 1, 0], "spread off against the two launches, gram_strips = %d" % strips)
    _same(out[1, 1, 1], out[0, 1, 1], "spread on, strips on against off")
    return without


# Gram rows = 2 k0 + c + 2, donors, cells, k0, variants, covariate columns (0: the cohort's own intercept)
@pytest.mark.parametrize("rows,donors,cells,k0,variants,cov", [
    (67, 4, 70, 32, 10, 0),       # more pieces than k-steps (7 or 8 steps, up to 10 pieces), JT = 2: two wavefronts rotate nothing
    (71, 3, 60, 34, 9, 0),        # chunks of k0 - 2 and k0 + 2 positions, an odd donor count
    (75, 2, 80, 36, 7, 0),        # two donors, the fewest a cohort can have (the module's text): one piece-carrying Gram phase
    (103, 5, 120, 50, 18, 0),     # the large configuration's 103 rows
    (111, 4, 120, 54, 9, 0),      # 14 k-steps
    (118, 4, 120, 54, 9, 8),      # 8 tile rows: one workgroup per CU
])
def test_spread_equals_bunched_and_the_two_launches(rows, donors, cells, k0, variants, cov, kernel_form):
    import cellregmap_amd as crm

    c, keep, G = _ragged(donors, cells, k0, variants, 800 + k0)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    if cov:
        W = _covariates(y.size, cov, k0)
    assert rows == 2 * k0 + W.shape[1] + 2
    _forms_agree(kernel_form, lambda: (crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E)), crm.GenotypePanel(G, groups=None), {}))


def test_spread_with_variants_without_a_kinship_term(kernel_form):
    """A phenotype with its cells permuted (test_gpu_gram_wide.py: _flat_phenotype, its cohort and permutation): some fits
    end without a kinship term -- has_A false, no wavefront of that workgroup rotates anything -- beside ordinary ones."""
    import cellregmap_amd as crm

    variants = 64
    co, keep, G = _ragged(5, 300, 50, variants, 31)
    y, E, W, hK = co.y[keep], co.E[keep], co.W[keep], co.hK[keep]
    without = _forms_agree(kernel_form, lambda: (crm.CellRegMap(_flat_phenotype(y, 6), E, W=W, Ls=crm.get_L_values(hK, E)),
                                                 crm.GenotypePanel(G, groups=None), {}))
    print("tests without a kinship term in one scan: %d of %d" % (without, variants))
    assert 0 < without < variants     # at least one variant without a kinship term and one with it
