"""The fused form of a block's elementwise passes (scan_block.hip: copy_block; blockops.hip: block_pass_kernel).

A block of a dense panel that starts at a multiple of 128 variants is read in place: its statistics read the panel slab and
one pass writes Gx, G2 = Gt o Gt, GG = Gt o Gx and, on the kinship routes, Gx and Gt in donor order -- instead of the copy,
the projection, two donor-order gathers and the products, one launch after the other over the same slab.  The arithmetic per
element is the same, so every output of every entry point is the same as with form ``block_fused`` = 0 BIT FOR BIT: each case
runs the same calls with the form off and on and compares p, rho*, the variance components, Q, lml, delta, the scale, the
eigenvalues, F and every array of the info call as 64-bit patterns, and ``crm_test_fused_blocks`` says how many blocks the
fused form served.

Cohort: 7 donors of 5 .. 37 cells (203 cells: no multiple of 16, 64 or 256, one donor below the 16-row padding unit of the donor
order), cells shuffled so that the donor order is a real permutation; 3 contexts.  The file also passes under CRM_POISON=1:
fresh device buffers are filled with 0xFF there, so a padding row or a tail row the pass left unwritten would show up as NaN."""
import contextlib
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CELLS = (5, 25, 30, 33, 36, 37, 37)
K0 = 3
PANEL = 128 + 257          # blocks [0, ...) and [128, 128 + 257)
RANGES = ((0, 1, 1), (0, 70, 1), (0, 257, 1), (128, 257, 1), (128, 70, 1), (3, 70, 0))   # (first, count, fused blocks)


def _lib_ctx():
    from cellregmap_amd import _engine, _lib

    return _lib.load(), _engine._context(0)


def _fused():
    from cellregmap_amd import _lib

    lib, ctx = _lib_ctx()
    out = ctypes.c_long(-1)
    _lib.check(lib.crm_test_fused_blocks(ctx, ctypes.byref(out)))
    return out.value


_cohorts = {}


def _cohort(variants=PANEL, seed=5):
    """(y, E, hK, G dense, G donor-constant), cells in shuffled order; built once per shape and left unchanged."""
    key = (variants, seed)
    if key not in _cohorts:
        from cellregmap_amd.synth import make_cohort

        assert sum(CELLS) == 203 and min(CELLS) < 16
        c = make_cohort(len(CELLS), max(CELLS), K0, variants, seed=seed)
        rng = np.random.default_rng(seed)
        keep = np.concatenate([np.flatnonzero(c.donor_of_cell == d)[:m] for d, m in enumerate(CELLS)])
        keep = keep[rng.permutation(keep.size)]
        G = c.G[keep] + 0.05 * rng.normal(size=(keep.size, variants))
        _cohorts[key] = (c.y[keep], c.E[keep], c.hK[keep], G, c.G[keep])
    return _cohorts[key]


def _covariates(n, c):
    return np.column_stack([np.ones(n), np.random.default_rng(c).normal(size=(n, c - 1))]) if c > 1 else np.ones((n, 1))


@contextlib.contextmanager
def _route(kernel_form, name):
    """The routes, forced as tests/test_gpu_rho0_positions.py and tests/test_gpu_edges.py force them; backgrounds made inside."""
    from cellregmap_amd import _engine, _lib

    lib, ctx = _lib_ctx()
    route = 2
    if name == "unrelated":
        kernel_form("kin_fold", 2), kernel_form("kin_diag", 2)
    elif name == "folded":
        kernel_form("kin_fold", 2), kernel_form("kin_diag", 0)
    elif name == "unfolded_pairs":
        kernel_form("kin_fold", 0), kernel_form("kin_diag", 0), kernel_form("donor_pairs", 2)
    elif name == "direct":
        route = 0
    else:
        assert name == "mode_b"
        kernel_form("kin_fold", 2), kernel_form("kin_diag", 2)
    _engine._bg_cache.clear()
    _lib.check(lib.crm_test_set_kinship_route(ctx, route))
    try:
        yield
    finally:
        _lib.check(lib.crm_test_set_kinship_route(ctx, 1))
        _engine._bg_cache.clear()


def _make(name, y, E, W, hK, **kw):
    import cellregmap_amd as crm

    if name == "mode_b":
        return crm.CellRegMap(y, E, W=W, hK=hK, **kw)
    return crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E), **kw)


def _calls(obj, panel, first, count, idx_E=None, idx_G=None):
    """The scan and the info call over variants [first, first + count): every output array, by name."""
    from cellregmap_amd import _lib

    lib, _ = _lib_ctx()
    gene = obj._bind_gene()
    k0 = obj._E0.shape[1]
    iE = None if idx_E is None else np.ascontiguousarray(idx_E, dtype=np.int32)
    iG = None if idx_G is None else np.ascontiguousarray(idx_G, dtype=np.int32)
    out = {k: np.full(count, np.nan) for k in ("pv", "rho1", "e2", "g2", "eps2", "Q", "lml", "delta", "scale")}
    out["lambda"], out["F"] = np.full((count, k0), np.nan), np.full((count, k0, k0), np.nan)
    _lib.check(lib.crm_scan_interaction(gene, panel.handle, first, count, _lib.ptr(iE), _lib.ptr(iG),
                                        *[_lib.ptr(out[k]) for k in ("pv", "rho1", "e2", "g2", "eps2", "Q", "lml", "delta",
                                                                     "scale", "lambda", "F")]))
    info = {"info_pv": np.full(count, np.nan), "ifault": np.full(count, -99, np.int32), "liu": np.full(count, np.nan),
            "flags": np.full(count, -99, np.int32), "bound_Q": np.full(count, np.nan), "bound_p": np.full(count, np.nan)}
    _lib.check(lib.crm_scan_interaction_bounds(gene, panel.handle, first, count, _lib.ptr(iE), _lib.ptr(iG),
                                               *[_lib.ptr(info[k]) for k in ("info_pv", "ifault", "liu", "flags", "bound_Q",
                                                                             "bound_p")]))
    out.update(info)
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(new, old, what):
    assert new.keys() == old.keys()
    for k in old:
        assert np.array_equal(_bits(new[k]), _bits(old[k])), (what, k)
    assert np.all(np.isfinite(old["Q"])) and np.all(np.isfinite(old["F"])) and np.all(old["pv"] >= 0), what


def _off_and_on(kernel_form, run, fused_blocks, what):
    """run() with the form off, then on: the same bits, and the counter moved by `fused_blocks` with the form on alone."""
    kernel_form("block_fused", 0)
    before = _fused()
    old = run()
    assert _fused() == before, what
    kernel_form("block_fused", 1)
    new = run()
    assert _fused() - before == fused_blocks, (what, _fused() - before, fused_blocks)
    _same(new, old, what)
    return new


@pytest.mark.parametrize("c", [1, 3, 9])       # (9: variant_stats_general_kernel)
@pytest.mark.parametrize("route", ["unrelated", "folded", "unfolded_pairs", "direct", "mode_b"])
def test_fused_blocks_are_bit_identical(route, c, kernel_form):
    """1, 70 and 257 variants from `first` = 0 and 128 (fused) and from 3 (unaligned: the copy, the counter stays)."""
    import cellregmap_amd as crm

    y, E, hK, G, _ = _cohort()
    W = _covariates(y.size, c)
    with _route(kernel_form, route):
        obj = _make(route, y, E, W, hK)
        panel = crm.GenotypePanel(G, groups=None)
        for first, count, fused in RANGES:
            # (the scan and the info call: one block each)
            _off_and_on(kernel_form, lambda: _calls(obj, panel, first, count), 2 * fused, (route, c, first, count))


@pytest.mark.parametrize("route", ["unrelated", "folded", "direct"])
def test_a_short_last_block_after_full_ones(route, kernel_form):
    """Blocks of 128 variants over a panel of 385: three full blocks and one of a single variant."""
    import cellregmap_amd as crm
    from cellregmap_amd import _lib

    lib, ctx = _lib_ctx()
    y, E, hK, G, _ = _cohort()
    W = _covariates(y.size, 3)
    _lib.check(lib.crm_set_block_variants(ctx, 128))
    try:
        with _route(kernel_form, route):
            obj = _make(route, y, E, W, hK)
            panel = crm.GenotypePanel(G, groups=None)
            blocks = -(-PANEL // 128)
            new = _off_and_on(kernel_form, lambda: _calls(obj, panel, 0, PANEL), 2 * blocks, route)
            # (and the blocks of one call are the single calls: a block leaves nothing behind that the next one reads)
            part = _calls(obj, panel, 128, 257)
            for k in part:
                assert np.array_equal(_bits(part[k]), _bits(new[k][128:])), k
    finally:
        _lib.check(lib.crm_set_block_variants(ctx, 0))


@pytest.mark.parametrize("route", ["unrelated", "folded", "unfolded_pairs", "direct"])
def test_three_phenotypes_in_one_pass(route, kernel_form):
    from cellregmap_amd import GenotypePanel, _lib

    lib, _ = _lib_ctx()
    y, E, hK, G, _ = _cohort()
    W = _covariates(y.size, 3)
    rng = np.random.default_rng(11)
    Y = np.stack([y, y[rng.permutation(y.size)], y + rng.normal(size=y.size)], axis=1)
    with _route(kernel_form, route):
        first_obj = _make(route, Y[:, 0], E, W, hK)
        crms = [first_obj] + [_make(route, Y[:, i], E, W, hK, background=first_obj._bg) for i in (1, 2)]
        panel = GenotypePanel(G, groups=None)
        handles = (ctypes.c_void_p * 3)(*[o._bind_gene().value for o in crms])

        def run(first=128, count=257):
            out = {k: np.full((3, count), np.nan) for k in ("pv", "rho1", "e2", "g2", "eps2", "Q")}
            _lib.check(lib.crm_scan_interaction_multi(handles, 3, panel.handle, first, count, None, None,
                                                      *[_lib.ptr(out[k]) for k in ("pv", "rho1", "e2", "g2", "eps2", "Q")]))
            return out

        # (the direct route forms H'(g o E0) of several phenotypes by a Khatri-Rao product that fetches up to 128 columns past
        # the block's last tile: [128, 385) has no such columns behind it in the panel's row of 512 and keeps the copy)
        for first, count, fused in ((128, 257, 0 if route == "direct" else 1), (0, 70, 1)):
            kernel_form("block_fused", 0)
            before = _fused()
            old = run(first, count)
            kernel_form("block_fused", 1)
            new = run(first, count)
            assert _fused() - before == fused, (first, count)
            for k in old:
                assert np.array_equal(_bits(new[k]), _bits(old[k])), k
            assert np.all(np.isfinite(old["Q"]))


@pytest.mark.parametrize("route", ["unrelated", "folded", "direct"])
def test_the_permutation_replay(route, kernel_form):
    """Three context permutations in one call: the first pass records, the others replay -- every pass prepares its blocks."""
    from cellregmap_amd import GenotypePanel

    y, E, hK, G, _ = _cohort()
    W = _covariates(y.size, 3)
    rng = np.random.default_rng(12)
    perms = [rng.permutation(y.size) for _ in range(3)]
    with _route(kernel_form, route):
        obj = _make(route, y, E, W, hK)
        panel = GenotypePanel(G[:, :257], groups=None)

        def run():
            pv, info, Q = obj.scan_interaction_permutations(panel, return_Q=True, idx_E_list=perms)
            return dict(info, pv=pv, Q=Q)

        kernel_form("block_fused", 0)
        before = _fused()
        old = run()
        kernel_form("block_fused", 1)
        new = run()
        assert _fused() - before == 3
        for k in old:
            assert np.array_equal(_bits(new[k]), _bits(old[k])), k


@pytest.mark.parametrize("route", ["unrelated", "direct"])
def test_the_genotype_hook_and_grouped_panels_keep_the_copy(route, kernel_form):
    """idx_G permutes the rows of the test direction and a grouped panel holds one row per donor: neither is read in place."""
    import cellregmap_amd as crm

    y, E, hK, G, Gd = _cohort()
    W = _covariates(y.size, 3)
    perm = np.random.default_rng(13).permutation(y.size)
    with _route(kernel_form, route):
        obj = _make(route, y, E, W, hK)
        dense = crm.GenotypePanel(G, groups=None)
        _off_and_on(kernel_form, lambda: _calls(obj, dense, 128, 70, idx_G=perm), 0, (route, "idx_G"))
        grouped = crm.GenotypePanel(Gd, groups="auto")
        assert grouped.n_groups == len(CELLS)
        _off_and_on(kernel_form, lambda: _calls(obj, grouped, 128, 70), 0, (route, "grouped"))


@pytest.mark.parametrize("route", ["unrelated", "folded", "unfolded_pairs"])
def test_one_gene_keeps_its_context_tables_only_as_long_as_they_hold(route, kernel_form):
    """A gene keeps E, y o E, W o E, E (x) E, their donor-order copies and the answers of the probes between calls
    (crm_gene::tab_key).  One gene scans panel 1, panel 2, panel 1 under idx_E and panel 1 again; then the pair-product forms
    are switched off between two calls (other tables, the same probes); then the kinship structure of its background is
    announced again (a new generation: everything is rebuilt); then the phenotype is bound to a second background (mode B's,
    another kinship structure: a gene belongs to one background for life, so this is a second gene of the same y, W and E0)
    and scans again.  Each result is that of a freshly made gene, bit for bit, with the fused form and without."""
    import cellregmap_amd as crm
    from cellregmap_amd import _engine

    y, E, hK, G, _ = _cohort()
    _, _, _, G2, _ = _cohort(seed=6)
    W = _covariates(y.size, 3)
    perm = np.random.default_rng(14).permutation(y.size)
    steps = [(G, None), (G2, None), (G, perm), (G, None)]
    with _route(kernel_form, route):
        kernel_form("block_fused", 1)
        kept = _make(route, y, E, W, hK)
        panels = {id(M): crm.GenotypePanel(M, groups=None) for M in (G, G2)}
        got = [_calls(kept, panels[id(M)], 128, 257, idx_E=iE) for M, iE in steps]
        for form in (1, 0):
            kernel_form("block_fused", form)
            for (M, iE), have in zip(steps, got):
                fresh = _make(route, y, E, W, hK)
                _same(have, _calls(fresh, panels[id(M)], 128, 257, idx_E=iE), (route, form))
        kernel_form("block_fused", 1)
        # the forms decide after the probes, on every call
        kernel_form("donor_pairs", 0)
        have = _calls(kept, panels[id(G)], 128, 257)
        _same(have, _calls(_make(route, y, E, W, hK), panels[id(G)], 128, 257), (route, "donor_pairs off"))
        kernel_form("donor_pairs", 2, reset=route != "unfolded_pairs")     # (as _route left it)
        _same(got[0], _calls(kept, panels[id(G)], 128, 257), (route, "donor_pairs on again"))
        # the same background, its kinship structure announced again
        halves = crm.get_L_values(hK, E)
        assert isinstance(halves, _engine.HadamardHalves)
        _engine._announce_kinship_groups(kept._bg, halves)
        have = _calls(kept, panels[id(G)], 128, 257)
        _same(have, got[0], (route, "announced again"))
        _same(have, _calls(_make(route, y, E, W, hK), panels[id(G)], 128, 257), (route, "announced again, fresh"))
        # a second background
        second = _make("mode_b", y, E, W, hK)
        assert second._bg is not kept._bg
        have = [_calls(second, panels[id(M)], 128, 257) for M in (G, G2, G)]
        _same(have[2], have[0], (route, "second background, again"))
        for M, h in zip((G, G2), have):
            _same(h, _calls(_make("mode_b", y, E, W, hK), panels[id(M)], 128, 257), (route, "second background"))
        _same(got[0], _calls(kept, panels[id(G)], 128, 257), (route, "first background after the second"))
