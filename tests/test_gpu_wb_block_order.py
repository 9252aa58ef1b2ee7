"""One phenotype on the unrelated-donor route with the pair stage in block order (scan.hip: select_pairs, donor_columns;
form ``wb_block_order`` = 1, the default) against the rho*-sorted copy of the block it no longer forms (= 0).

The sort exists so that H'(g o E0) comes out as the operand of the MixK(rho*) product; this route has no such product,
and the rotated S of a variant depends on that variant alone.  Every per-variant number is computed by the same
instructions on the same inputs, so every output is the same bits -- lambda and F included -- and so are the increments
of ``crm_test_tests_without_pair``.

The cohort is one whose variants select several rho* (the sort is a real permutation of the block, asserted) with tests
without a kinship term among them (position -1, asserted): the phenotype mixed with a permutation of itself, so that
the random effects are weak, the likelihood is flat in rho and some fits end at the upper clamp of delta.  45 variants
in blocks of 32: a full block and a short one."""
import contextlib

import numpy as np
import pytest

from test_gpu_gram_wide import _without_pair
from test_gpu_unrelated_donors import _blocks, _ragged, _route

pytestmark = pytest.mark.gpu

DONORS, CELLS, K0, VARIANTS, SEED, MIX = 9, 40, 6, 45, 123, 0.16


def _cohort():
    co, keep, G = _ragged(DONORS, CELLS, K0, VARIANTS, SEED)
    y = co.y[keep]
    y = MIX * y + (1.0 - MIX) * y[np.random.default_rng(SEED).permutation(y.size)]
    return y, co.E[keep], co.W[keep], co.hK[keep], G


@contextlib.contextmanager
def _blocks_of(variants):
    from cellregmap_amd import _engine, _lib

    lib, ctx = _lib.load(), _engine._context(0)
    _lib.check(lib.crm_set_block_variants(ctx, variants))
    try:
        yield
    finally:
        _lib.check(lib.crm_set_block_variants(ctx, 0))


def _both(kernel_form, call):
    """``call(obj, panel)`` with the sorted copy (form 0) and in block order (form 1): (sorted, block order, tests without
    a pair)."""
    import cellregmap_amd as crm

    y, E, W, hK, G = _cohort()
    res, none = [], []
    with _route(kernel_form, 2), _blocks_of(32):
        obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        panel = crm.GenotypePanel(G, groups=None)
        for form in (0, 1):
            kernel_form("wb_block_order", form)
            before, none_before = _blocks(), _without_pair()
            res.append(call(obj, panel))
            assert _blocks() > before                            # the route served (45 variants: a block of 32 and one of 13)
            none.append(_without_pair() - none_before)
    assert none[0] == none[1]
    return res[0], res[1], none[0]


def _same(new, old, what):
    assert sorted(new) == sorted(old)
    for k in old:
        assert np.array_equal(new[k], old[k], equal_nan=True), (what, k)


def test_block_order_is_bit_for_bit_the_sorted_copy(kernel_form):
    old, new, none = _both(kernel_form, lambda obj, panel: obj.scan_interaction(panel, return_stats=True))
    pv, info, st = old
    with_term = (info["e2"] + info["g2"]) > 1e-6 * info["eps2"]
    chosen = sorted(set(info["rho1"][with_term]))
    print("\n[block order] tests without a pair: %d of %d; rho* of the others: %s" % (none, VARIANTS, chosen))
    assert 0 < none < VARIANTS                                # tests without a kinship term mixed in
    assert len(chosen) >= 3                                      # the sort is a real permutation of the block
    rho = info["rho1"][:32][with_term[:32]]
    assert np.any(np.diff(rho) < 0)                              # ... the first block is not in rho* order as it stands
    assert set(st) == {"Q", "lml", "delta", "scale", "lambda", "F"}
    assert np.array_equal(new[0], pv)
    _same(new[1], info, "info")
    _same(new[2], st, "stats")


def test_block_order_with_the_exact_tail(kernel_form):
    old, new, _ = _both(kernel_form, lambda obj, panel: obj.scan_interaction(panel, return_stats=True, pvalue="exact"))
    assert "log_pvalue" in old[1] and "pvalue_status" in old[1]
    assert np.array_equal(new[0], old[0])
    _same(new[1], old[1], "info")
    _same(new[2], old[2], "stats")


def test_block_order_in_the_info_call(kernel_form):
    old, new, _ = _both(kernel_form, lambda obj, panel: obj.scan_interaction_info(panel))
    assert np.array_equal(new[0], old[0])
    _same(new[1], old[1], "flags")
