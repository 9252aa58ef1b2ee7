"""Two forms of the unrelated-donor route's steps 3 and 4 (scan.hip: plan_rotations).

``rho0_positions``: the null fits at rho = 0 read the position basis -- Phi'gx, Phi'[y, W] and s_p(0), the operands of the
assembly -- and the rotation MixK(0)'(H'Gx) is not formed.  ``rotation_tails``: the last r mod 128 <= 16 columns of the
other rotations go through the skinny one-pass kernel instead of another column of 128-wide tiles.

By default either is taken only where the batched launch of the rotations then runs fewer rounds, which takes a block of
some hundred variants against a spectrum of a thousand entries (the last test): the others force the forms (value 2).
Both are held against the same scan with ``rho0_positions`` = 0 and ``rotation_tails`` = 0 (the same rho*, Q and F to
1e-9 of their scale, p to 1e-7 relative + 1e-13: ``_close`` of test_gpu_unrelated_donors), against the oracle on a few
variants, and the counters say which form served.  rho* = 0 is rare, so the scans' results alone say little about the
fit at rho = 0: the null-fit probe compares its likelihood and scale themselves, form on against form off."""
import contextlib
import ctypes

import numpy as np
import pytest

import parity_bounds
from test_gpu_unrelated_donors import _blocks, _close, _ragged, _route

pytestmark = pytest.mark.gpu


def _counter(name):
    from cellregmap_amd import _engine, _lib

    out = ctypes.c_long(-1)
    _lib.check(getattr(_lib.load(), name)(_engine._context(0), ctypes.byref(out)))
    return out.value


def _counters():
    return np.array([_blocks(), _counter("crm_test_rho0_position_blocks"), _counter("crm_test_rotation_tail_launches")])


def _scan(kernel_form, make_obj, G, rho0, tails, call=None, **kw):
    """One scan on the unrelated-donor route with the two forms set; returns (result, object, panel, [blocks of the route,
    blocks with rho = 0 from the positions, rotation tail launches])."""
    import cellregmap_amd as crm

    with _route(kernel_form, 2):
        kernel_form("rho0_positions", rho0)
        kernel_form("rotation_tails", tails)
        obj = make_obj()
        panel = crm.GenotypePanel(G, groups=None)
        before = _counters()
        if call is None:
            res = obj.scan_interaction(panel, return_stats=True, **kw)
        else:
            res = call(obj, panel)
        used = _counters() - before
    return res, obj, panel, used


@contextlib.contextmanager
def _forms(kernel_form, rho0, tails):
    with _route(kernel_form, 2):
        kernel_form("rho0_positions", rho0)
        kernel_form("rotation_tails", tails)
        yield


def _objective(obj, panel, x):
    """[variants x grid x (lml, scale)] of the null fits at delta = 1 / (1 + exp(-x)): the probe hook ends the scan after
    the null-fit kernels of its (only) block and keeps their records."""
    from cellregmap_amd import _engine, _lib

    lib, ctx = _lib.load(), _engine._context(0)
    _lib.check(lib.crm_test_null_fit_probe(ctx, 1, x))
    try:
        obj.scan_interaction(panel, progress=False)
        buf = np.full(2 * panel.shape[1] * obj._bg.rho.size, np.nan)
        got = lib.crm_test_null_fit_probe_read(ctx, _lib.ptr(buf), buf.size)
        assert got == buf.size, got
    finally:
        _lib.check(lib.crm_test_null_fit_probe(ctx, 0, 0.0))
    return buf.reshape(-1, obj._bg.rho.size, 2)


def _pair(kernel_form, make_obj, G, new=(2, 1), **kw):
    """(reference scan with both forms off, scan with the forms at `new`, its object, panel and counters)"""
    old, _, _, used0 = _scan(kernel_form, make_obj, G, 0, 0, **kw)
    assert used0[0] > 0 and used0[1] == 0 and used0[2] == 0    # the route served, neither form did
    res, obj, panel, used = _scan(kernel_form, make_obj, G, *new, **kw)
    assert used[0] > 0
    return old, res, obj, panel, used


def _oracle(obj, panel, G, pv, y, E, W, hK, count=6):
    from oracle import crm as ocrm

    with_bounds = parity_bounds.bounds(obj, panel)[1]
    sel = np.arange(0, G.shape[1], max(1, G.shape[1] // count))[:count]
    opv, _ = ocrm.OracleCellRegMap(y, E, W=W, Ls=ocrm.khatri_rao_halves(hK, E)).scan_interaction(G[:, sel])
    parity_bounds.assert_p_within(pv[sel], opv, with_bounds[sel])


@pytest.mark.parametrize("donors,cells,k0,variants", [
    (7, 60, 5, 37),
    (5, 120, 50, 18),          # 50 + 3 + 50 = 103 Gram rows
])
def test_rho0_from_the_positions_matches_the_dense_product(donors, cells, k0, variants, kernel_form):
    import cellregmap_amd as crm

    c, keep, G = _ragged(donors, cells, k0, variants, 500 + k0 + cells)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    make = lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))  # noqa: E731
    old, new, obj, panel, used = _pair(kernel_form, make, G)
    assert used[1] > 0
    _close(new, old)
    if k0 <= 20:
        with _route(kernel_form, 2):
            _oracle(obj, panel, G, new[0], y, E, W, hK)


def test_rho0_from_the_positions_in_the_lds_shared_null_fit(kernel_form):
    """1 100 variants against W = ones: from 1 024 variants on with one covariate column the null fits run in
    nullfit_shared_kernel, which copies the three spectrum vectors of a grid point into LDS -- here the position-basis ones
    at rho = 0, with their own length and leading dimension.  (The form the flagship benchmark runs.)"""
    import cellregmap_amd as crm

    c, keep, G = _ragged(7, 60, 5, 1100, 565)
    y, E, hK = c.y[keep], c.E[keep], c.hK[keep]
    W = np.ones((y.size, 1))
    make = lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))  # noqa: E731
    old, new, obj, panel, used = _pair(kernel_form, make, G)
    assert used[1] > 0
    _close(new, old)
    with _route(kernel_form, 2):
        _oracle(obj, panel, G, new[0], y, E, W, hK)


@pytest.mark.parametrize("cov", [3, 10])   # the register kernels (c <= 8), the wide kernel
def test_rho0_from_the_positions_with_covariates(cov, kernel_form):
    import cellregmap_amd as crm

    c, keep, G = _ragged(7, 60, 5, 37, 565)
    y, E, hK = c.y[keep], c.E[keep], c.hK[keep]
    W = np.column_stack([np.ones(y.size), np.random.default_rng(cov).normal(size=(y.size, cov - 1))])
    make = lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))  # noqa: E731
    old, new, obj, panel, used = _pair(kernel_form, make, G)
    assert used[1] > 0
    _close(new, old)
    with _route(kernel_form, 2):
        _oracle(obj, panel, G, new[0], y, E, W, hK)


def test_a_donor_with_fewer_cells_than_contexts(kernel_form):
    """6 donors of 30 cells, 12 contexts, one donor cut to 8 cells: us_d of that donor has rank 8, so 4 of its 12 positions
    are zero columns of Phi (seal_unrelated_donors drops them), 68 of 72 kept.  The position form serves when the
    background's rank at rho = 0 is 68 as well; otherwise the dense product stays.  Either way the results hold."""
    import cellregmap_amd as crm
    from cellregmap_amd.synth import make_cohort

    donors, cells, k0, variants = 6, 30, 12, 25
    c = make_cohort(donors, cells, k0, variants, seed=77)
    donor = np.repeat(np.arange(donors), cells)
    keep = np.ones(donors * cells, bool)
    keep[np.flatnonzero(donor == 3)[8:]] = False
    rng = np.random.default_rng(77)
    G = c.G[keep] + 0.05 * rng.normal(size=c.G[keep].shape)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    make = lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))  # noqa: E731
    old, new, obj, panel, used = _pair(kernel_form, make, G)
    rank0 = obj._bg.rank(0)
    print("rank at rho = 0: %d of %d positions; blocks from the positions: %d" % (rank0, donors * k0, used[1]))
    assert rank0 == 68
    assert used[1] > 0     # the two rank rules agree (68 = 68): the position form serves, zero positions included
    _close(new, old)
    with _route(kernel_form, 2):
        _oracle(obj, panel, G, new[0], y, E, W, hK)


def test_rho0_from_the_positions_info_and_exact_tail(kernel_form):
    import cellregmap_amd as crm

    c, keep, G = _ragged(8, 40, 5, 40, 17)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    make = lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))  # noqa: E731
    info_call = lambda obj, panel: obj.scan_interaction_info(panel)  # noqa: E731
    (pv0, xi0), _, _, used0 = _scan(kernel_form, make, G, 0, 0, call=info_call)
    (pv, xi), _, _, used = _scan(kernel_form, make, G, 2, 1, call=info_call)
    assert used0[1] == 0 and used[1] > 0
    assert np.all(np.abs(pv - pv0) <= 1e-7 * pv0 + 1e-13)
    for k in ("ifault", "degenerate", "rho_tie"):
        assert np.array_equal(xi[k], xi0[k]), k
    # (rho* itself is not part of this entry point's record: the pair below compares it on the same cohort)
    old, new, _, _, used = _pair(kernel_form, make, G, pvalue="exact")
    assert used[1] > 0
    _close(new, old)
    assert np.array_equal(new[1]["pvalue_status"], old[1]["pvalue_status"])
    assert np.all(np.abs(new[1]["log_pvalue"] - old[1]["log_pvalue"]) <= 1e-7)


def test_rotation_tails_through_the_one_pass_kernel(kernel_form):
    """24 donors with at least 43 cells each against 43 contexts: rank 24 x 43 = 1032 = 8 tiles + 8 columns at the interior
    grid points.  Forced (``rotation_tails`` = 2), the last 8 columns of every rotation
    go through the skinny kernel; with ``rho0_positions`` as well, rho = 0 has no rotation at all."""
    import cellregmap_amd as crm

    donors, k0, variants = 24, 43, 40
    c, keep, G = _ragged(donors, 80, k0, variants, 91)
    assert np.bincount(np.repeat(np.arange(donors), 80)[keep]).min() >= k0
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    make = lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))  # noqa: E731
    old, new, obj, panel, used = _pair(kernel_form, make, G, new=(0, 2))
    assert obj._bg.rank(5) == 1032
    assert used[1] == 0 and used[2] > 0
    _close(new, old)
    both, _, _, used = _scan(kernel_form, make, G, 2, 2)
    assert used[1] > 0 and used[2] > 0
    _close(both, old)
    default, _, _, used = _scan(kernel_form, make, G, 1, 1)
    assert used[1] == 0 and used[2] == 0      # one block of 40 variants is a fraction of a round: nothing to save
    assert np.array_equal(default[0], old[0]) and np.array_equal(default[2]["Q"], old[2]["Q"])


@pytest.mark.parametrize("donors,cells,k0,variants", [
    (7, 60, 5, 37),
    (5, 120, 50, 18),
    (6, 30, 12, 25),           # (not the cut cohort of the test above: all positions kept)
])
def test_the_objective_at_rho0_from_the_positions(donors, cells, k0, variants, kernel_form):
    """The likelihood and the scale of the null fits at fixed delta, every (variant, grid point), form on against form off.
    The results of a scan see the fit at rho = 0 only through the variants with rho* = 0; this sees it on all of them.
    Bound: 1e-12 of |lml| and of the scale.  Both are sums of n <= 600 terms, summed in another order and from operands
    formed by other products of the same length -- n eps = 7e-14 each way, with an allowance of 8 for the stages in
    between (the eigen-solver's basis against the positions, the weights 1 / ((1 - delta) s + delta) at delta >= 0.12).
    A wrong spectrum, stride, length or operand moves them in the first digits.  The other grid points run the same
    kernels on the same operands."""
    import cellregmap_amd as crm

    c, keep, G = _ragged(donors, cells, k0, variants, 500 + k0 + cells)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    rec = {}
    for rho0 in (0, 2):
        with _forms(kernel_form, rho0, 0):
            obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
            panel = crm.GenotypePanel(G, groups=None)
            before = _counters()
            rec[rho0] = [_objective(obj, panel, x) for x in (-2.0, 0.0, 2.0)]
            used = _counters() - before
            assert used[0] == 0                          # (a probe pass ends before the assembly: no block served)
            assert (used[1] > 0) == (rho0 == 2)
            zero = np.flatnonzero(obj._bg.rho == 0.0)
    assert zero.size == 1
    for new, old in zip(rec[2], rec[0]):
        assert new.shape == (variants, obj._bg.rho.size, 2) and np.all(np.isfinite(old))
        rel = np.abs(new - old) / np.abs(old)
        print("largest relative difference at rho = 0: lml %.3g scale %.3g; elsewhere %.3g" %
              (rel[:, zero, 0].max(), rel[:, zero, 1].max(), np.delete(rel, zero, axis=1).max()))
        assert np.all(rel <= 1e-12)


def test_many_phenotypes_in_one_pass_with_rho0_from_the_positions(kernel_form):
    """Only the Phi'y pointer is per gene: with the form forced, several phenotypes in one pass are bit for bit the single
    scans (genes past the first read wb_yW at their own offset)."""
    from cellregmap_amd import CellRegMap, GenotypePanel, get_L_values, scan_interaction_many

    c, keep, G = _ragged(8, 30, 4, 70, 41)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    rng = np.random.default_rng(7)
    Y = np.stack([y, y[rng.permutation(y.size)], rng.normal(size=y.size), y + rng.normal(size=y.size)], axis=1)
    with _forms(kernel_form, 2, 1):
        Ls = get_L_values(hK, E)
        first = CellRegMap(Y[:, 0], E, W=W, Ls=Ls)
        crms = [first] + [CellRegMap(Y[:, i], E, W=W, Ls=Ls, background=first._bg) for i in range(1, 4)]
        panel = GenotypePanel(G, groups=None)
        for kw in ({}, {"idx_G": rng.permutation(y.size)}):
            before = _counters()
            pv, info = scan_interaction_many(crms, panel, **kw)
            assert np.all((_counters() - before)[:2] > 0)
            for i, one in enumerate(crms):
                before = _counters()
                spv, sinfo = one.scan_interaction(panel, **kw)
                assert np.all((_counters() - before)[:2] > 0)
                assert np.array_equal(pv[i], spv)
                for k in sinfo:
                    assert np.array_equal(info[k][i], sinfo[k])
            if not kw:
                pv_plain, rho_plain = pv[2], info["rho1"][2]
    # (and the genes past the first against the dense product: a wrong offset would still be the same in both scans above)
    with _forms(kernel_form, 0, 0):
        Ls = get_L_values(hK, E)
        old = CellRegMap(Y[:, 2], E, W=W, Ls=Ls).scan_interaction(GenotypePanel(G, groups=None))
    assert np.array_equal(rho_plain, old[1]["rho1"])
    assert np.all(np.abs(pv_plain - old[0]) <= 1e-7 * old[0] + 1e-13)


def test_permutations_in_one_call_with_rho0_from_the_positions(kernel_form):
    """The replayed passes form Phi'gx after the recorded fits are put back and record no rows of T: with the form forced,
    the permutations of one call are bit for bit the separate calls."""
    import cellregmap_amd as crm

    c, keep, G = _ragged(10, 24, 4, 29, 53)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    rng = np.random.default_rng(8)
    perms = [rng.permutation(y.size) for _ in range(3)]
    with _forms(kernel_form, 2, 1):
        obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        panel = crm.GenotypePanel(G, groups=None)
        before = _counters()
        pv, info, Q = obj.scan_interaction_permutations(panel, return_Q=True, idx_E_list=perms)
        assert np.all((_counters() - before)[:2] > 0)
        for b in range(3):
            pv1, info1, st1 = obj.scan_interaction(panel, return_stats=True, idx_E=perms[b])
            assert np.array_equal(pv[b], pv1)
            assert np.array_equal(Q[b], st1["Q"])
            for k in info1:
                assert np.array_equal(info[k], info1[k]), k


def test_mode_b_with_rho0_from_the_positions(kernel_form):
    """hK without Ls (k2 = 1, us_d = 1): one position per donor."""
    import cellregmap_amd as crm

    c, keep, G = _ragged(9, 50, 6, 40, 77)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    old, new, obj, panel, used = _pair(kernel_form, lambda: crm.CellRegMap(y, E, W=W, hK=hK), G)
    assert used[1] > 0
    _close(new, old)


def test_the_default_rule_takes_both_forms_where_they_save_a_round(kernel_form):
    """The decision the flagship benchmark runs, at the smallest shape that reaches it.  The cohort of the tails test with
    960 variants in one block: 8 row tiles, and at ten grid points of rank 1032 nine column tiles each, plus 8 tiles at
    rho = 1 -- 728 tiles on 512 slots (256 CUs, two workgroups each), 2 rounds.  Without rho = 0: 656; the tails through
    the one-pass kernel: 648; both: 9 x 64 + 8 = 584, of which cut_rotations takes the 72 over a round out -- 1 round.
    Neither alone saves the round, both do."""
    import torch
    import cellregmap_amd as crm

    assert torch.cuda.get_device_properties(0).multi_processor_count == 256     # (the arithmetic above)
    donors, k0, variants = 24, 43, 960
    c, keep, G = _ragged(donors, 80, k0, variants, 91)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    make = lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))  # noqa: E731
    old, new, obj, panel, used = _pair(kernel_form, make, G, new=(1, 1))
    assert [obj._bg.rank(i) for i in range(obj._bg.rho.size)] == [1032] * 10 + [k0]
    assert used[1] > 0 and used[2] > 0
    print("variants with rho* = 0: %d of %d" % (int(np.sum(old[1]["rho1"] == 0.0)), variants))
    _close(new, old)
