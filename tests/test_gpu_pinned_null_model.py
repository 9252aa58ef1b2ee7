"""Every null fit of the interaction scan -- each (variant, grid point) search, not only the one that wins -- against the
longdouble reference's own maximum, and the choice of rho* from the records themselves.

tests/test_gpu_pinned.py holds Q, F, the restricted lml and the scale at the point (rho*, delta) the device reports: the
search is deliberately not on the path of that comparison, and of the ``variants x grid`` trial records that
``select_rho_kernel`` reads only the winner's numbers are ever seen.  Here the test hook ``crm_test_null_fit_probe`` with
``on = 2`` (include/crm_hip_test.h) returns the trial table of a real scan -- lml, delta, scale, nfev, use_g per (variant,
grid point), then the grid index the selection wrote -- and an ordinary scan of the same panel follows.  Per case:

  a. records are complete, for every trial of the block: nfev > 0, 0 < delta < 1, use_g = 1, lml and scale finite;
  b. lml and scale of every trial of the held variants against ``pinned`` at the trial's own delta, within
     ``pinned_reference.limits`` (32 x the float64 oracle's error at the same points, floor n x 2.2e-16, ceiling 1e-11);
  c. interior trials: L* - refit_allowance(x*, curvature) - lim |L*| <= lml <= L* + lim |L*| and
     |logit(delta) - x*| <= stop_allowance, with (L*, x*, curvature) the reference's own maximum
     (``pinned_reference.null_trial_reference``) -- the search stopped within its tolerance of the likelihood's maximum;
  d. trials whose maximum sits at a clamp of the logistic: the reference at the device's delta is not below the reference at
     the clamp by more than lim |L*|, and the device's delta is the clamp's own double (1 - 2^-52 in nullfit.hip and in
     oracle/lmm.py alike: the two clamps are the same by construction);
  e. selection from the records, exactly: rho_index is the first index of the maximum of the device's own trial lmls, and
     rho1, delta, lml and scale of the ordinary scan are bitwise the record at that index -- the order of the table
     ([variant][grid]) and the tie rule without any tolerance;
  f. selection against the reference: ``argmax_or_tie`` of L* per grid point; without a tie the device's index is the
     reference's, with one it is among the tied.

The held variants are ``pinned_reference.pick``'s and, where a form packs four fits into a wavefront, the last
``variants mod 4``; no trial of a held variant is left out and a reference that cannot be evaluated raises.  Every share
of a bound is printed and kept (profiles/pinned_null_model_errors.json through $CRM_PINNED_JSON).  The cohorts are those of
tests/pinned_cases.py: NULL_MODEL; tests/test_pinned_reference_cpu.py holds each of them to the conditions this file relies
on, with the float64 oracle's own search in the device's place.

Which kernel serves is decided by the covariate count alone (up to 8 columns nullfit.hip's register kernel, up to 62
nullfit_wide.hip, beyond nullfit_xwide.hip), the LDS-shared queue form by one column and at least 1024 variants, its sub-forms
by their knobs; the routes of mode C through their counters.
"""
import json
import os

import numpy as np
import pytest

import pinned_cases as pc
import pinned_reference as pr
from test_gpu_pinned import RHO0, REPEATS, UD, _kinship, _lib_ctx, _used

pytestmark = pytest.mark.gpu

RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    """The per-case shares go beside the file $CRM_PINNED_JSON names, as <name>_null_model.json (tools/pinned_record.py
    merges them into profiles/pinned_null_model_errors.json)."""
    yield
    dest = os.environ.get("CRM_PINNED_JSON")
    if dest and RECORD:
        with open(os.path.splitext(dest)[0] + "_null_model.json", "w") as fh:
            json.dump(RECORD, fh, indent=1, sort_keys=True)


def _trial_records(obj, panel, flags=False):
    """([variants][grid][lml, delta, scale, nfev, use_g], [variants] grid index) of a real scan's null fits: the hook ends
    the pass after the null-fit kernels of its (only) block.  ``flags``: through the call that asks for model flags."""
    from cellregmap_amd import _lib

    lib, ctx = _lib_ctx()
    p, nrho = panel.shape[1], obj._bg.rho.size
    _lib.check(lib.crm_test_null_fit_probe(ctx, 2, 0.0))
    try:
        if flags:
            obj.scan_interaction_info(panel)
        else:
            obj.scan_interaction(panel, progress=False)
        buf = np.full(p * (5 * nrho + 1), np.nan)
        got = lib.crm_test_null_fit_probe_read(ctx, _lib.ptr(buf), buf.size)
        assert got == buf.size, (got, buf.size)
    finally:
        _lib.check(lib.crm_test_null_fit_probe(ctx, 0, 0.0))
    return buf[:5 * p * nrho].reshape(p, nrho, 5), buf[5 * p * nrho:].astype(int)


def _scan(cs, obj, flags=False):
    """(trial records, grid indices, the ordinary scan's result) on the path the cohort names."""
    import cellregmap_amd as crm

    panel = crm.GenotypePanel(cs.G, groups="auto" if cs.path == "collapsed" else None)
    assert (panel.n_groups is not None) == (cs.path == "collapsed")
    assert np.array_equal(obj._bg.rho, np.asarray(cs.grid, float))
    rec, index = _trial_records(obj, panel, flags)
    before = _used()
    res = obj.scan_interaction(panel, return_stats=True, progress=False)
    assert (_used() - before)[REPEATS] == 0          # the path the case names served every variant
    return rec, index, res


def _make(cs):
    import cellregmap_amd as crm

    kw = {"A": {}, "B": {"hK": cs.hK}, "C": {"Ls": crm.get_L_values(cs.hK, cs.E)} if cs.mode == "C" else {}}[cs.mode]
    return crm.CellRegMap(cs.y, cs.E, W=cs.W, **kw)


def _hold(case, cs, rec, index, res, expect_tie=None):
    pv, info, st = res
    p, nrho = rec.shape[:2]
    assert p == cs.G.shape[1] and nrho == len(cs.grid)
    # a. complete records, every trial of the block
    assert np.all(rec[:, :, 3] > 0) and np.all(rec[:, :, 4] == 1), case
    assert np.all((rec[:, :, 1] > 0) & (rec[:, :, 1] < 1)), case
    assert np.all(np.isfinite(rec[:, :, 0])) and np.all(np.isfinite(rec[:, :, 2])), case
    # e. the selection, exactly, from the records: every variant of the block
    assert np.array_equal(index, np.argmax(rec[:, :, 0], axis=1)), (case, index, np.argmax(rec[:, :, 0], axis=1))
    rows = np.arange(p)
    assert np.array_equal(info["rho1"], np.asarray(cs.grid, float)[index]), case
    for key, col in (("lml", 0), ("delta", 1), ("scale", 2)):
        assert np.array_equal(st[key], rec[rows, index, col]), (case, key)
    # b, c, d. the held variants, every grid point
    sel = cs.picks()
    lim, ora, shares = pc.hold_trials(cs, rec, sel)
    worst, clamps = {}, 0
    for key, sh in shares.items():
        clamps += "clamp value" in sh
        for k, v in sh.items():
            if k not in worst or v > worst[k]["share"]:
                worst[k] = {"share": float(v), "variant": int(key[0]), "grid": int(key[1])}
    # f. the selection against the reference's maxima
    ties = 0
    for j in sel:
        tops = [cs.trial(j, i)[1][0] for i in range(nrho)]
        ok, tie = pr.selection_against_reference(tops, index[j], lim["lml"])
        ties += tie
        assert ok, (case, j, int(index[j]), [float(t) for t in tops])
    print("\n[null model] %s: n %d, variants held %s of %d, %d trials (%d at a clamp), %d ties\n[null model]   oracle %s\n"
          "[null model]   limit  %s\n[null model]   nfev %d..%d\n[null model]   largest shares: %s"
          % (case, cs.n, sel, p, len(shares), clamps, ties, " ".join("%s %.2e" % kv for kv in ora.items()),
             " ".join("%s %.2e" % kv for kv in lim.items()), rec[:, :, 3].min(), rec[:, :, 3].max(),
             ", ".join("%s %.3g (variant %d, grid %d)" % (k, v["share"], v["variant"], v["grid"]) for k, v in worst.items())))
    RECORD[case] = {"cohort": cs.name, "cells": cs.n, "covariates": cs.c, "variants": [int(j) for j in sel], "trials": len(shares),
                    "at_a_clamp": clamps, "ties": ties, "oracle": ora, "limit": lim, "shares": worst,
                    "nfev": [int(rec[:, :, 3].min()), int(rec[:, :, 3].max())]}
    assert max(lim.values()) <= pr.CEILING
    for key, sh in shares.items():
        for k, v in sh.items():
            assert v <= 1, (case, key, k, v, lim)
    if expect_tie is not None:
        assert (ties > 0) == expect_tie, (case, ties)
    return clamps, len(shares)


# ---- the register kernel, one fit per wavefront -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,r", [("c 1, r 63, dense", 63), ("c 1, r 63, collapsed", 63), ("c 3, r 64, dense", 64),
                                    ("c 3, r 64, collapsed", 64), ("c 8, r 65, dense", 65), ("c 8, r 65, collapsed", 65),
                                    ("c 2, r 5", 5)])
def test_register_kernel(name, r):
    """The lane loop over a spectrum of 63, 64 and 65 entries (one pass of 64 lanes, exactly one, one and a lane) and of 5
    (fewer than a row of sixteen), at 1, 3 and 8 covariate columns, on the dense and on the donor-collapsed path."""
    cs = pc.null_model_case(name)
    assert cs.c <= 8 and cs.G.shape[1] < 1024                  # nullfit_kernel, one wavefront per (variant, grid point)
    obj = _make(cs)
    assert obj._bg.rank(5) == r and obj._bg.rank(0) == cs.donors and obj._bg.rank(10) == cs.E.shape[1]
    _hold("register kernel, " + name, cs, *_scan(cs, obj))


def test_register_kernel_in_the_references_own_operations(kernel_form):
    """``nullfit_exact``: IEEE division and one log per spectrum entry."""
    cs = pc.null_model_case("c 1, r 63, dense")
    obj = _make(cs)
    plain = _scan(cs, obj)
    kernel_form("nullfit_exact", 1)
    exact = _scan(cs, obj)
    assert not np.array_equal(plain[0][:, :, 0], exact[0][:, :, 0])       # (another arithmetic did run)
    _hold("register kernel, nullfit_exact, c 1, r 63", cs, *exact)


def test_model_flags_leave_the_search_as_it_is():
    """A call that asks for model flags launches the kernels with TRACK = true; brent_search.h promises the same search
    bit for bit.  lml, delta, scale and use_g are the same bits; nfev is larger by two, the evaluations one stopping
    tolerance to either side of the stopping point that a tracked kernel adds after its search (nullfit.hip: f_up, f_dn)."""
    cs = pc.null_model_case("c 3, r 64, dense")
    obj = _make(cs)
    rec, index, res = _scan(cs, obj)
    tracked, tracked_index, _ = _scan(cs, obj, flags=True)
    assert np.array_equal(rec[:, :, [0, 1, 2, 4]], tracked[:, :, [0, 1, 2, 4]]) and np.array_equal(index, tracked_index)
    assert np.array_equal(tracked[:, :, 3], rec[:, :, 3] + 2)
    _hold("register kernel, model flags, c 3, r 64", cs, tracked, tracked_index, res)


# ---- the LDS-shared queue form ------------------------------------------------------------------------------------------------------
def test_queue_form_four_fits_per_wavefront_r_16():
    cs = pc.null_model_case("queue, r 16")
    assert cs.c == 1 and cs.G.shape[1] == 1027                 # from 1024 variants on; the last wavefront holds three fits
    # (all 1027 in one block, as the form needs: _trial_records would read fewer records than it asks for otherwise)
    assert cs.picks() == [0, 513, 1024, 1025, 1026]
    obj = _make(cs)
    assert obj._bg.rank(5) == 16 and obj._bg.rank(0) == 6 and obj._bg.rank(10) == 10      # rho = 0, 1: shorter than sld = 64
    _hold("queue form, four per wavefront, r 16", cs, *_scan(cs, obj))


def test_queue_form_and_its_sub_forms_r_17(kernel_form):
    """Four fits per wavefront (a variant per row of sixteen lanes, 17 entries: two passes of a row), one fit per wavefront
    (the same bits: include/crm_hip_test.h) and one independent wavefront per (variant, grid point) on the same cohort."""
    cs = pc.null_model_case("queue, r 17")
    assert cs.c == 1 and cs.G.shape[1] == 1027                 # (one block of 1027: see the test above)
    obj = _make(cs)
    assert obj._bg.rank(5) == 17 and obj._bg.rank(0) == 6 and obj._bg.rank(10) == 11
    four = _scan(cs, obj)
    kernel_form("nullfit_one_per_wave", 1)
    one = _scan(cs, obj)
    kernel_form("nullfit_one_per_wave", 0, reset=True)
    kernel_form("nullfit_per_wave", 1)
    per_wave = _scan(cs, obj)
    assert np.array_equal(four[0], one[0]) and np.array_equal(four[1], one[1])
    _hold("queue form, four per wavefront, r 17", cs, *four)
    _hold("queue form, one per wavefront, r 17", cs, *one)
    _hold("per-wave form, 1027 variants, r 17", cs, *per_wave)


# ---- the kernels for more covariate columns ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c 9", "c 62", "c 63", "c 128", "mode A, k0 17"])
def test_wide_kernels_and_mode_a(name):
    """nullfit_wide.hip at 9 and 62 columns, nullfit_xwide.hip at 63 and 128; mode A: one grid point, so the selection is
    trivial and the value and the stopping point remain (17 spectrum entries)."""
    cs = pc.null_model_case(name)
    obj = _make(cs)
    if cs.mode == "A":
        assert len(cs.grid) == 1 and obj._bg.rank(0) == 17 and cs.c <= 8
    else:       # the covariate count decides the kernel: 9 .. 62 nullfit_wide.hip, 63 .. 128 nullfit_xwide.hip
        assert cs.c == int(name[2:]) and ((9 <= cs.c <= 62) if name in ("c 9", "c 62") else (63 <= cs.c <= 128))
    _hold(name if cs.mode == "A" else "wide kernels, " + name, cs, *_scan(cs, obj))


# ---- mode C on the unrelated-donor route ----------------------------------------------------------------------------------------------
def _unrelated(cs, kernel_form, rho0):
    with _kinship(kernel_form, route=2, diag=2, pairs=0, rho0=rho0, tails=0):
        obj = _make(cs)
        before = _used()
        out = _scan(cs, obj)
        used = _used() - before
    assert used[UD] > 0 and (used[RHO0] > 0) == (rho0 == 2), used
    return out


def test_rho0_from_either_set_of_operands(kernel_form):
    """``rho0_positions`` 0 and 2: the trial at rho = 0 from the rotation MixK(0)'(H'Gx) and from the position basis; the
    records at rho > 0 are the same bits in both runs."""
    cs = pc.null_model_case("mode C")
    rotated = _unrelated(cs, kernel_form, 0)
    positions = _unrelated(cs, kernel_form, 2)
    assert np.array_equal(rotated[0][:, 1:], positions[0][:, 1:])
    _hold("mode C, unrelated donors, rho = 0 from the rotation", cs, *rotated)
    _hold("mode C, unrelated donors, rho = 0 from the positions", cs, *positions)


def test_extra_wide_kernel_on_the_unrelated_donor_route(kernel_form):
    """127 covariate columns: the route's documented ceiling (k0 + c + 2 + k1 <= 144)."""
    cs = pc.null_model_case("c 127, mode C")
    assert cs.c == 127                                          # nullfit_xwide.hip
    _hold("mode C, unrelated donors, c 127", cs, *_unrelated(cs, kernel_form, 0))


# ---- the ends of delta ------------------------------------------------------------------------------------------------------------------
def test_a_phenotype_without_a_kinship_term():
    """y is noise: every trial sits at the upper clamp and the likelihood is the same over the whole grid -- e decides
    (the first grid point), f reports a tie."""
    cs = pc.null_model_case("no kinship term")
    rec, index, res = _scan(cs, _make(cs))
    clamps, trials = _hold("no kinship term", cs, rec, index, res, expect_tie=True)
    assert clamps == trials
    assert np.all(rec[cs.picks(), :, 1] == 1 - pr.CLAMP)


def test_a_phenotype_with_a_strong_kinship_term():
    """delta is small at rho < 1 and the curvature large."""
    cs = pc.null_model_case("strong kinship term")
    rec, index, res = _scan(cs, _make(cs))
    clamps, _ = _hold("strong kinship term", cs, rec, index, res, expect_tie=False)
    assert clamps == 0 and np.all(rec[cs.picks(), :-1, 1] < 0.2)


def test_a_saturated_cohort():
    """n - r = 0 at the interior grid points: 60 cells against 50 + 10 spectrum entries, so the complement terms of the
    likelihood, (u'v - (Q0'u)'(Q0'v)) / delta and (n - r) log delta, are differences of equal numbers and zero."""
    cs = pc.null_model_case("saturated")
    obj = _make(cs)
    assert obj._bg.rank(5) == cs.n == 60 and obj._bg.rank(0) == 10 and obj._bg.rank(10) == 50
    with pytest.warns(RuntimeWarning, match="saturated model"):          # (the library says so when the phenotype is bound)
        out = _scan(cs, obj)
    _hold("saturated", cs, *out)


def test_the_hook_serves_one_phenotype_per_pass_and_two_modes():
    """The trial table is written again per phenotype, so a pass over several has no records of a real scan to give:
    CRM_ERR_ARG (-2), as is a mode other than 0, 1 and 2."""
    from cellregmap_amd import CellRegMap, GenotypePanel, _lib, scan_interaction_many

    lib, ctx = _lib_ctx()
    cs = pc.null_model_case("c 2, r 5")
    assert lib.crm_test_null_fit_probe(ctx, 3, 0.0) == -2 and lib.crm_test_null_fit_probe(ctx, -1, 0.0) == -2
    first = CellRegMap(cs.y, cs.E, W=cs.W, hK=cs.hK)
    crms = [first, CellRegMap(cs.y[::-1].copy(), cs.E, W=cs.W, hK=cs.hK, background=first._bg)]
    panel = GenotypePanel(cs.G, groups=None)
    _lib.check(lib.crm_test_null_fit_probe(ctx, 2, 0.0))
    try:
        with pytest.raises(_lib.CrmError, match="one phenotype per pass"):
            scan_interaction_many(crms, panel)
    finally:
        _lib.check(lib.crm_test_null_fit_probe(ctx, 0, 0.0))
    pv, _ = scan_interaction_many(crms, panel)                   # (and the context is as it was)
    assert np.all(np.isfinite(pv))
