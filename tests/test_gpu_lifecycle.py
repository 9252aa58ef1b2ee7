"""Device memory comes back: what a round of work allocates for its backgrounds, genes and panels is released when they
are destroyed (include/crm_hip_test.h: crm_test_live_device_bytes, the bytes held by the live device buffers of the
process).  The context's work buffers only ever grow, so a round is run once to bring them to size and then again: the
second round must leave the count where the first one left it."""
import ctypes
import gc

import numpy as np
import pytest

from test_gpu_unrelated_donors import _blocks, _ragged, _route

pytestmark = pytest.mark.gpu

OK = 0


def _live():
    from cellregmap_amd import _lib

    return _lib.load().crm_test_live_device_bytes()


def _drop_everything():
    from cellregmap_amd import _engine

    _engine._bg_cache.clear()
    gc.collect()
    _engine.release_workspaces(0)


def _round(kernel_form):
    """A ragged unrelated-donor cohort, a dense and a donor-constant panel, three more phenotypes bound in one batch; returns
    the live bytes once every object of the round is gone."""
    import cellregmap_amd as crm

    c, keep, G = _ragged(8, 30, 4, 40, 41)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    rng = np.random.default_rng(7)
    Y = np.stack([y[rng.permutation(y.size)], rng.normal(size=y.size), y + rng.normal(size=y.size)], axis=1)
    with _route(kernel_form, 2):
        Ls = crm.get_L_values(hK, E)
        first = crm.CellRegMap(y, E, W=W, Ls=Ls)
        others = [crm.CellRegMap(Y[:, i], E, W=W, Ls=Ls, background=first._bg) for i in range(3)]
        dense = crm.GenotypePanel(G, groups=None)
        grouped = crm.GenotypePanel(c.G[keep])       # donor-constant columns: stored one row per donor
        assert grouped.n_groups
        before = _blocks()
        pv, _ = crm.scan_interaction_many([first] + others, dense)      # (binds `others` through crm_gene_create_batch)
        pv1, _ = first.scan_interaction(dense)
        pv2, _ = first.scan_interaction(grouped)
        assert _blocks() > before          # the unrelated-donor form, whose tables the background holds, really served
        assert np.array_equal(pv[0], pv1) and np.all(np.isfinite(pv)) and np.all(np.isfinite(pv2))
    del first, others, dense, grouped, Ls
    _drop_everything()
    return _live()


def test_a_second_round_leaves_the_live_device_bytes_where_the_first_left_them(kernel_form):
    _drop_everything()
    warm = _round(kernel_form)
    again = _round(kernel_form)
    print(f"live device bytes after the first round {warm}, after the second {again}")
    assert again == warm


def test_objects_made_and_destroyed_through_the_c_abi_return_every_byte():
    """Every constructor once, on a context of its own that goes as well: the count ends where it began."""
    from cellregmap_amd import _lib
    from cellregmap_amd.synth import make_cohort

    lib = _lib.load()
    _drop_everything()
    start = _live()
    vp = ctypes.c_void_p
    ctx = vp()
    assert lib.crm_ctx_create(0, ctypes.byref(ctx)) == OK
    c = make_cohort(6, 20, 3, 24, seed=9)
    n = c.y.size
    rng = np.random.default_rng(5)
    handles = []          # (destroy function, handle), in order of creation

    # a background from given spectra
    ranks = np.array([5, 4, 6], np.int32)
    rho3 = _lib.f64([0.0, 0.5, 1.0])
    Q0 = [_lib.f64(np.linalg.qr(rng.normal(size=(n, r)))[0]) for r in ranks]
    S0 = [_lib.f64(rng.uniform(0.5, 2.0, size=r)) for r in ranks]
    PP = vp * 3
    bg_qs = vp()
    assert lib.crm_background_create_qs(ctx, n, 3, _lib.ptr(rho3), _lib.ptr(ranks), PP(*[q.ctypes.data for q in Q0]),
                                        PP(*[s.ctypes.data for s in S0]), ctypes.byref(bg_qs)) == OK
    assert _live() > start
    lib.crm_background_destroy(bg_qs)

    # a decomposed background, a gene on it, one more phenotype, four more in a batch
    E, hK, rho = _lib.f64(c.E), _lib.f64(c.hK), _lib.f64(np.linspace(0, 1, 11))
    bg = vp()
    assert lib.crm_background_create(ctx, n, _lib.ptr(E), E.shape[1], _lib.ptr(hK), hK.shape[1], 11, _lib.ptr(rho), 0.0,
                                     ctypes.byref(bg)) == OK
    y, W = _lib.f64(c.y), _lib.f64(c.W)
    gene = vp()
    assert lib.crm_gene_create(bg, _lib.ptr(y), _lib.ptr(W), W.shape[1], _lib.ptr(E), E.shape[1], ctypes.byref(gene)) == OK
    handles.append((lib.crm_gene_destroy, gene))
    y2 = _lib.f64(rng.normal(size=n))
    like = vp()
    assert lib.crm_gene_create_like(gene, _lib.ptr(y2), ctypes.byref(like)) == OK
    handles.append((lib.crm_gene_destroy, like))
    Y = _lib.f64(rng.normal(size=(n, 4)))
    batch = (vp * 4)()
    assert lib.crm_gene_create_batch(gene, _lib.ptr(Y), 4, 4, batch) == OK
    handles += [(lib.crm_gene_destroy, vp(h)) for h in batch]

    # panels: donor-level float64, donor-level int8, and the expanded matrix with a hint that holds / does not hold
    group = np.ascontiguousarray(c.donor_of_cell, dtype=np.int32)
    Gd = _lib.f64(rng.normal(size=(6, 24)))
    panel = vp()
    assert lib.crm_panel_create_grouped(ctx, n, _lib.ptr(group), 6, _lib.ptr(Gd), 24, 24, ctypes.byref(panel)) == OK
    handles.append((lib.crm_panel_destroy, panel))
    D = np.ascontiguousarray((np.arange(6)[:, None] + np.arange(24)[None, :]) % 3, dtype=np.int8)   # no constant column
    panel = vp()
    assert lib.crm_panel_create_grouped_i8(ctx, n, _lib.ptr(group), 6, _lib.ptr(D), 24, 24, 1, ctypes.byref(panel)) == OK
    handles.append((lib.crm_panel_destroy, panel))
    reps = np.ascontiguousarray([int(np.flatnonzero(group == d)[0]) for d in range(6)], dtype=np.int64)
    expanded = _lib.f64(Gd[group])
    for G, expect in ((expanded, 1), (_lib.f64(expanded + rng.normal(size=expanded.shape)), 0)):
        panel, grouped = vp(), ctypes.c_int(-1)
        assert lib.crm_panel_create_auto(ctx, n, _lib.ptr(G), 24, 24, _lib.ptr(group), 6, _lib.ptr(reps), ctypes.byref(panel),
                                         ctypes.byref(grouped)) == OK
        assert grouped.value == expect
        handles.append((lib.crm_panel_destroy, panel))

    assert _live() > start
    for destroy, h in handles:
        destroy(h)
    lib.crm_background_destroy(bg)
    lib.crm_ctx_destroy(ctx)
    print(f"live device bytes before {start}, after {_live()}")
    assert _live() == start
