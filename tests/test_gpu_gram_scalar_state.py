"""The per-donor bookkeeping of the fused unrelated-donor Gram (wb_gram_fused.hip): chunk bounds and columns, the pointers
that move from donor to donor, the rotation's passes over one or two column tiles with their stores into the image, the
donor sums and their splits.  Every case is held bit for bit -- p, rho*, Q, F, lml, delta, the scale and every info array;
the donor sums reach Q and F through the assembly -- against the two launches that the fused kernel replaces
(``wb_gram_fused`` = 0), against the round-robin deal (``gram_strips`` = 0) and against the pieces in a bunch
(``wb_gram_spread`` = 0): test_gpu_gram_spread.py's six runs.

Only the cases that the other Gram files do not reach stand here.  They hold already: k0 = 2 mod 4 with three donors
(3, 60, 34), k0 = 0 mod 4 (32, 36, 40, 48, 52), two donors (2, 80, 36), 103 rows (5, 120, 50), 14 k-steps (4, 120, 54), 8 tile
rows (4, 120, 54 with 8 covariate columns), a constant variant and variants without a kinship term beside ordinary ones
(test_gpu_gram_spread.py, test_gpu_gram_strips.py, test_gpu_wb_gram_fused.py).  Added here:
  * k0 = 2 mod 4 with an EVEN donor count (4, 60, 34): the chunks alternate k0 - 2 and k0 + 2 positions to the end, and the last
    one closes on a multiple of four of its own (no zero padding) -- with three donors it is padded;
  * seven donors at k0 = 34 over 300 variants in blocks of 128: the pointers advance across many donors, the column tiles of
    the rotation are three (a pass over two and a pass over one), and there are three blocks, the last one ragged;
  * nine donors: the donor sums go out in 8 splits of ranges of two donors, so five ranges hold donors and three are the
    zero-filled tail -- with a constant variant (no rotation, the sums still formed) beside the ordinary ones.
The file also passes under CRM_POISON=1 (fresh device buffers filled with 0xFF, a red zone behind each)."""
import contextlib

import pytest

from test_gpu_gram_spread import _forms_agree
from test_gpu_unrelated_donors import _ragged

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _blocks_of(variants):
    from cellregmap_amd import _engine, _lib

    lib, ctx = _lib.load(), _engine._context(0)
    _lib.check(lib.crm_set_block_variants(ctx, variants))
    try:
        yield
    finally:
        _lib.check(lib.crm_set_block_variants(ctx, 0))


def _scan_case(kernel_form, donors, cells, k0, variants, constant=None):
    import cellregmap_amd as crm

    c, keep, G = _ragged(donors, cells, k0, variants, 800 + k0 + donors)
    if constant is not None:
        G = G.copy()
        G[:, constant] = 1.0
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    assert 65 <= 2 * k0 + W.shape[1] + 2 <= 128     # the fused Gram's rows
    return _forms_agree(kernel_form, lambda: (crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E)), crm.GenotypePanel(G, groups=None), {}))


def test_even_donor_count_at_k0_2_mod_4(kernel_form):
    _scan_case(kernel_form, 4, 60, 34, 9)


def test_seven_donors_over_three_blocks(kernel_form):
    with _blocks_of(128):
        _scan_case(kernel_form, 7, 60, 34, 300)


def test_more_splits_than_donor_ranges_with_a_constant_variant(kernel_form):
    _scan_case(kernel_form, 9, 60, 32, 10, constant=4)
