"""The side stream of the interaction scan (scan_side.hip; form ``side_stream``): on the unrelated-donor route with one
phenotype, the products of a block that do not depend on its fits leave the pair stage.  Z2, Z3 and Z1 are enqueued on a
second, lowest-priority stream behind the rotation launch and joined before the assembly; the per-donor pair products
are enqueued on the main stream between the copy of the fits and the host's wait for it.  The same launches on the same
inputs, so every output is the same BITS as with the form off (0: everything in the pair stage, in the old order).
Forms 2 and 3 hold the declared dependencies at the two extremes of the interleaving: 2 lets the main stream wait for the
side work right behind the fork, 3 starts it only when the main stream has reached the join.
``crm_test_side_stream_blocks`` says where the form served: one phenotype, no permutation replay.

The file also passes under CRM_POISON=1 (fresh device buffers filled with 0xFF, a red zone behind each): the same bits, and
no launch that moved writes past its buffer."""
import contextlib
import ctypes

import numpy as np
import pytest

from test_gpu_gram_wide import _covariates
from test_gpu_unrelated_donors import _blocks, _ragged, _route

pytestmark = pytest.mark.gpu

FORMS = (0, 1, 2, 3)


def _lib_ctx():
    from cellregmap_amd import _engine, _lib

    return _lib.load(), _engine._context(0)


def _side_blocks():
    from cellregmap_amd import _lib

    lib, ctx = _lib_ctx()
    out = ctypes.c_long(-1)
    _lib.check(lib.crm_test_side_stream_blocks(ctx, ctypes.byref(out)))
    return out.value


def _fused():
    from cellregmap_amd import _lib

    lib, ctx = _lib_ctx()
    out = ctypes.c_long(-1)
    _lib.check(lib.crm_test_wb_gram_fused_blocks(ctx, ctypes.byref(out)))
    return out.value


def _pair_blocks():
    lib, ctx = _lib_ctx()
    return lib.crm_test_donor_pair_blocks(ctx)


def _live_bytes():
    return _lib_ctx()[0].crm_test_live_device_bytes()


@contextlib.contextmanager
def _blocks_of(variants):
    from cellregmap_amd import _lib

    lib, ctx = _lib_ctx()
    _lib.check(lib.crm_set_block_variants(ctx, variants))
    try:
        yield
    finally:
        _lib.check(lib.crm_set_block_variants(ctx, 0))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b, what):
    """(pv, info[, stats]) of two scans: every array the same bit patterns."""
    assert np.all(np.isfinite(b[0])), what
    assert np.array_equal(_bits(a[0]), _bits(b[0])), (what, "pv")
    for part, ref in zip(a[1:], b[1:]):
        assert set(part) == set(ref), what
        for k in ref:
            assert np.array_equal(_bits(part[k]), _bits(ref[k])), (what, k)


def _every_form(kernel_form, run, blocks, what):
    """`run()` under the four forms: the counter rises by `blocks` exactly where the form is non-zero, the outputs of 1, 2
    and 3 are the bits of 0.  Returns the result of form 0."""
    out = {}
    for form in FORMS:
        kernel_form("side_stream", form)
        before, served = _side_blocks(), _blocks()
        out[form] = run()
        assert _blocks() > served, (what, form)
        assert _side_blocks() - before == (blocks if form else 0), (what, form, _side_blocks() - before)
    for form in FORMS[1:]:
        _same(out[form], out[0], (what, "form %d against 0" % form))
    return out[0]


def _cohort(donors, cells, k0, variants, cov, seed):
    co, keep, G = _ragged(donors, cells, k0, variants, seed)
    y, E, W, hK = co.y[keep], co.E[keep], co.W[keep], co.hK[keep]
    if cov:
        W = _covariates(y.size, cov, k0)
    return y, E, W, hK, G


# donors, cells, k0, variants, covariate columns (0: the cohort's own intercept); forms set beside the route; whether the
# fused Gram / the pair products serve
@pytest.mark.parametrize("donors,cells,k0,variants,cov,forms,fused,pairs", [
    (5, 120, 50, 18, 0, {}, True, True),                     # the workload's 103 rows, fused Gram
    (4, 120, 54, 9, 8, {}, True, True),                      # 8 tile rows: one workgroup per CU
    (4, 70, 32, 10, 0, {"wb_gram_fused": 0}, False, True),   # the rotation launch and the Gram launch behind the pair products
    (4, 70, 32, 10, 0, {"donor_pairs": 0}, False, False),    # no pair products: only the Z products move
])
def test_every_form_gives_the_bits_of_the_main_stream(donors, cells, k0, variants, cov, forms, fused, pairs, kernel_form):
    import cellregmap_amd as crm

    y, E, W, hK, G = _cohort(donors, cells, k0, variants, cov, 800 + k0)
    with _route(kernel_form, 2):
        kernel_form("donor_pairs", 2)
        for name, value in forms.items():
            kernel_form(name, value)
        obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        panel = crm.GenotypePanel(G, groups=None)
        fused_before, pairs_before = _fused(), _pair_blocks()
        _every_form(kernel_form, lambda: obj.scan_interaction(panel, return_stats=True, progress=False), 1, (donors, k0, forms))
        assert _fused() - fused_before == (len(FORMS) if fused else 0)
        assert (_pair_blocks() > pairs_before) == pairs


def _window(obj, panel, first, count, k0):
    """crm_scan_interaction over [first, first + count): every output array of the entry point."""
    from cellregmap_amd import _lib

    lib, _ = _lib_ctx()
    out = {k: np.full(count, np.nan) for k in ("pv", "rho1", "e2", "g2", "eps2", "Q", "lml", "delta", "scale")}
    out["lambda"], out["F"] = np.full((count, k0), np.nan), np.full((count, k0, k0), np.nan)
    order = ("pv", "rho1", "e2", "g2", "eps2", "Q", "lml", "delta", "scale", "lambda", "F")
    _lib.check(lib.crm_scan_interaction(obj._bind_gene(), panel.handle, first, count, None, None, *[_lib.ptr(out[k]) for k in order]))
    return out


def _same_arrays(a, b, what):
    for k in b:
        assert np.all(np.isfinite(b[k])), (what, k)
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def test_several_blocks_in_one_call_and_a_window(kernel_form):
    """300 variants in blocks of 128 (two full blocks and one of 44): the join before the assembly also stands between
    the side work of a block and the next block's block_stats, which rewrites G2, GG and the donor-order copies.  Then the
    window [128, 278): `first` > 0, fewer variants than the rest -- a full block and one of 22."""
    import cellregmap_amd as crm

    k0, variants = 32, 300
    y, E, W, hK, G = _cohort(4, 70, k0, variants, 0, 57)
    with _route(kernel_form, 2), _blocks_of(128):
        kernel_form("donor_pairs", 2)
        obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        panel = crm.GenotypePanel(G, groups=None)
        whole, part = {}, {}
        for form in FORMS:
            kernel_form("side_stream", form)
            before = _side_blocks()
            whole[form] = _window(obj, panel, 0, variants, k0)
            assert _side_blocks() - before == (3 if form else 0), form
            before = _side_blocks()
            part[form] = _window(obj, panel, 128, 150, k0)
            assert _side_blocks() - before == (2 if form else 0), form
        for form in FORMS[1:]:
            _same_arrays(whole[form], whole[0], ("three blocks", form))
            _same_arrays(part[form], part[0], ("window", form))
        # (the blocks of one call are the single calls, as tests/test_gpu_block_passes.py holds for the main stream alone)
        for form in FORMS:
            _same_arrays(part[form], {k: v[128:278] for k, v in whole[0].items()}, ("window against the whole call", form))


def test_an_ordinary_scan_after_the_null_fit_probe(kernel_form):
    """The probe hook ends the pass behind the null fits of its block, with that block's side work in flight: the pass
    leaves with the side stream idle, the scan that follows gives the bits of form 0 and no device buffer is left over."""
    import cellregmap_amd as crm
    from cellregmap_amd import _lib

    lib, ctx = _lib_ctx()
    y, E, W, hK, G = _cohort(4, 70, 32, 10, 0, 832)
    with _route(kernel_form, 2):
        kernel_form("donor_pairs", 2)
        obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        panel = crm.GenotypePanel(G, groups=None)
        kernel_form("side_stream", 0)
        ref = obj.scan_interaction(panel, return_stats=True, progress=False)
        live = _live_bytes()
        for form in FORMS[1:]:
            kernel_form("side_stream", form)
            before = _side_blocks()
            _lib.check(lib.crm_test_null_fit_probe(ctx, 2, 0.0))
            try:
                obj.scan_interaction(panel, progress=False)
                buf = np.full(G.shape[1] * (5 * obj._bg.rho.size + 1), np.nan)
                assert lib.crm_test_null_fit_probe_read(ctx, _lib.ptr(buf), buf.size) == buf.size
            finally:
                _lib.check(lib.crm_test_null_fit_probe(ctx, 0, 0.0))
            assert _side_blocks() - before == 1, form            # the probed pass forked
            _same(obj.scan_interaction(panel, return_stats=True, progress=False), ref, ("after the probe", form))
            assert _live_bytes() == live, form


def test_a_constant_variant_with_exact_tails(kernel_form):
    """A constant variant (has_A false: rows of zeros, the donor sums still formed) beside ordinary ones, exact tails."""
    import cellregmap_amd as crm

    y, E, W, hK, G = _cohort(4, 70, 32, 10, 0, 31)
    G = G.copy()
    G[:, 4] = 1.0
    with _route(kernel_form, 2):
        kernel_form("donor_pairs", 2)
        obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        panel = crm.GenotypePanel(G, groups=None)
        ref = _every_form(kernel_form, lambda: obj.scan_interaction(panel, return_stats=True, progress=False, pvalue="exact"), 1,
                          "constant variant")
        assert "log_pvalue" in ref[1] and "pvalue_status" in ref[1]


def test_the_serial_paths_stay_on_the_main_stream(kernel_form):
    """A replayed permutation scan and a call with two phenotypes: the same bits under every form, and the counter does
    not move."""
    import cellregmap_amd as crm
    from cellregmap_amd import scan_interaction_many

    y, E, W, hK, G = _cohort(4, 70, 32, 10, 0, 41)
    rng = np.random.default_rng(5)
    perms = [None, rng.permutation(y.size), rng.permutation(y.size)]
    y2 = y + rng.normal(size=y.size)
    with _route(kernel_form, 2):
        kernel_form("donor_pairs", 2)
        Ls = crm.get_L_values(hK, E)
        obj = crm.CellRegMap(y, E, W=W, Ls=Ls)
        two = [obj, crm.CellRegMap(y2, E, W=W, Ls=Ls, background=obj._bg)]
        panel = crm.GenotypePanel(G, groups=None)
        out = {}
        for form in FORMS:
            kernel_form("side_stream", form)
            before, served = _side_blocks(), _blocks()
            pv, info, Q = obj.scan_interaction_permutations(panel, idx_E_list=perms, return_Q=True)
            info = dict(info, Q=Q)
            many = scan_interaction_many(two, panel)
            assert _blocks() > served
            assert _side_blocks() == before, form
            out[form] = ((pv, info), many)
        for form in FORMS[1:]:
            _same(out[form][0], out[0][0], ("permutations", form))
            _same(out[form][1], out[0][1], ("two phenotypes", form))
