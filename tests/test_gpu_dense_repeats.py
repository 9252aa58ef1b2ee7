"""The collapsed scan's dense repeats, at every interaction entry point, with the repeats at KNOWN positions.

A donor-level (grouped) panel is scanned on the collapsed path; variants that keep less than COLLINEAR_TAU = 1e-2 of their
squared norm outside span(W) are scanned a second time on the dense path and that result overwrites the first
(csrc/scan.hip: scan_core).  The hand-off is host-side index arithmetic: the list of marked variants, runs of neighbours at
most 32 apart, everything again when more than a quarter is marked, and every output pointer advanced by the run's offset
(csrc/scan_pass.h: ScanOut::advanced).  tests/dense_repeat_cases.py builds cohorts whose marked variants sit where that
arithmetic can go wrong -- a merged run, a separate one, a run across the boundary of two 128-variant blocks, the last
variant, a call that starts inside the panel, a panel marked on more than a quarter, and plain int8 dosages -- on two
backgrounds, so that the repeats run on two dense routes (mode B: hK=; mode C: Ls=, the unrelated-donor route forced).

Checks (the letters are those of DESIGN.md section 2, "Dense repeats"):

  a. positions, bit for bit: for every run (off, len) of a call over (first, count), every output array sliced at
     [off, off + len) -- with the stride of its kind -- equals, as 64-bit patterns, the same entry point called on the same
     grouped panel over (first + off, len) with crm_set_donor_collapse(ctx, 0).  That call IS the repeat pass (same plan,
     same inputs): no tolerance.
  b. flag consistency of crm_scan_interaction_bounds at every position: flags & 8 iff not (bound_p <= 1e-5), flags & 32 iff
     not (bound_Q <= 1e-6) -- the rule of ScanPass::flat_probes, which ties the arrays to one another.
  c. values against the pinned extended-precision reference (tests/pinned_reference.py) at the runs' first and last variants,
     their unmarked neighbours and variant 0; errors recorded in profiles/dense_repeat_errors.json.
  d. every position against the same call on the dense panel of the expanded genotypes, each variant held to the tolerance
     or to its own bound (tests/parity_bounds.py); the replayed permutations equal the single hooked scans bit for bit.
  e. the Python routes: cis windows on a resident grouped panel (first > 0), streamed chunks, the progress callback.

The repeat counter (crm_test_dense_repeats) must move by exactly (marked variants in range) x (passes that mark).  A pass
that marks is one scan_core call (csrc/scan.hip): the collapsed pass of it fills the list, `dense_repeats += near.size()`
once.  So: 1 per plain / _tail / _info / _bounds call; 1 per _multi(_tail) call whatever the number of phenotypes (the list
is per variant: W is shared); 1 per permutation of a _permuted(_tail) call (scan_permuted calls scan_core per permutation,
the replaying passes mark again).  A collapse-off call never moves it."""
import contextlib
import ctypes
import json
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose

import dense_repeat_cases as drc
import parity_bounds

pytestmark = pytest.mark.gpu

NPERM = 3
RECORD = {}
SCALARS = ("pv", "rho1", "e2", "g2", "eps2", "Q", "lml", "delta", "scale")
SHORT = ("pv", "rho1", "e2", "g2", "eps2", "Q")


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    """The per-case errors of (c) go to the file $CRM_DENSE_REPEAT_JSON names (a copy is kept under profiles/)."""
    yield
    dest = os.environ.get("CRM_DENSE_REPEAT_JSON")
    if dest and RECORD:
        with open(dest, "w") as fh:
            json.dump(RECORD, fh, indent=1, sort_keys=True)


def _lib_ctx():
    from cellregmap_amd import _engine, _lib

    return _lib.load(), _engine._context(0)


def _repeats():
    lib, ctx = _lib_ctx()
    return lib.crm_test_dense_repeats(ctx)


@pytest.fixture(autouse=True)
def _blocks_of_128():
    from cellregmap_amd import _lib

    lib, ctx = _lib_ctx()
    _lib.check(lib.crm_set_block_variants(ctx, 128))
    yield
    _lib.check(lib.crm_set_block_variants(ctx, 0))


@contextlib.contextmanager
def _collapse_off():
    from cellregmap_amd import _lib

    lib, ctx = _lib_ctx()
    _lib.check(lib.crm_set_donor_collapse(ctx, 0))
    try:
        yield
    finally:
        _lib.check(lib.crm_set_donor_collapse(ctx, 1))


@contextlib.contextmanager
def _background(kernel_form, mode):
    """Mode C: the unrelated-donor route forced as tests/test_gpu_pinned.py::_kinship(route=2, diag=2) does."""
    from cellregmap_amd import _engine
    from test_gpu_pinned import _kinship

    _engine._bg_cache.clear()
    try:
        if mode == "C":
            with _kinship(kernel_form, route=2, diag=2):
                yield
        else:
            assert mode == "B"
            yield
    finally:
        _engine._bg_cache.clear()


def _objects(mode, lay):
    """Three phenotypes on one background (made inside ``_background``); the first is the layout's own, the others carry
    noise and a context effect of their own on top of it.  (Not the phenotype with its cells permuted: without a kinship
    term its likelihood is flat in rho, rho* is decided by rounding -- ScanPass::no_kinship_term -- and two paths may
    report different grid points.)"""
    import cellregmap_amd as crm

    rng = np.random.default_rng(21)
    n = lay.y.size
    Y = np.stack([lay.y, lay.y + 0.7 * rng.normal(size=n) + lay.E @ rng.normal(size=drc.K0),
                  lay.y + rng.normal(size=n)], axis=1)
    kw = dict(hK=lay.hK) if mode == "B" else dict(Ls=crm.get_L_values(lay.hK, lay.E))
    first = crm.CellRegMap(Y[:, 0], lay.E, W=lay.W, **kw)
    return [first] + [crm.CellRegMap(Y[:, i], lay.E, W=lay.W, background=first._bg, **kw) for i in (1, 2)]


def _oracle_background(mode, lay):
    from oracle import crm as ocrm

    return dict(hK=lay.hK) if mode == "B" else dict(Ls=ocrm.khatri_rao_halves(lay.hK, lay.E))


def _panel(lay, ctor):
    import cellregmap_amd as crm

    if ctor == "from_donors":
        panel = crm.GenotypePanel.from_donors(lay.Gd, lay.donor)
    elif ctor == "auto":
        panel = crm.GenotypePanel(lay.G, groups="auto")
    elif ctor == "dosages":
        panel = crm.GenotypePanel.from_dosages(lay.dosage, lay.donor, standardize=False)
    else:
        assert ctor == "dense"
        panel = crm.GenotypePanel(lay.G, groups=None)
        assert panel.n_groups is None
        return panel
    assert panel.n_groups == len(drc.CELLS)
    return panel


def _perms(n):
    rng = np.random.default_rng(31)
    return np.ascontiguousarray(np.stack([rng.permutation(n) for _ in range(NPERM)]), dtype=np.int32)


# ---- the entry points through the C-ABI: every output array each of them has, by name ------------------------------------
# each returns (arrays, axis): axis[k] = the axis of arrays[k] that runs over the variants
def _f(*shape):
    return np.full(shape, np.nan)


def _i(*shape):
    return np.full(shape, -99, np.int32)


def _ptrs(out, keys):
    from cellregmap_amd import _lib

    return [_lib.ptr(out[k]) for k in keys]


def _plain(objs, panel, first, count, idx_E=None, idx_G=None, tail=False):
    from cellregmap_amd import _lib

    lib, _ = _lib_ctx()
    k0 = drc.K0
    iE = None if idx_E is None else np.ascontiguousarray(idx_E, dtype=np.int32)
    iG = None if idx_G is None else np.ascontiguousarray(idx_G, dtype=np.int32)
    out = {k: _f(count) for k in SCALARS}
    out["lambda"], out["F"] = _f(count, k0), _f(count, k0, k0)
    keys = SCALARS + ("lambda", "F")
    if tail:
        out["logp"], out["status"] = _f(count), _i(count)
        keys += ("logp", "status")
    fn = lib.crm_scan_interaction_tail if tail else lib.crm_scan_interaction
    _lib.check(fn(objs[0]._bind_gene(), panel.handle, first, count, _lib.ptr(iE), _lib.ptr(iG), *_ptrs(out, keys)))
    return out, {k: 0 for k in out}


def _tail(objs, panel, first, count, **hooks):
    return _plain(objs, panel, first, count, tail=True, **hooks)


def _info(objs, panel, first, count, idx_E=None, idx_G=None, bounds=False):
    from cellregmap_amd import _lib

    lib, _ = _lib_ctx()
    iE = None if idx_E is None else np.ascontiguousarray(idx_E, dtype=np.int32)
    iG = None if idx_G is None else np.ascontiguousarray(idx_G, dtype=np.int32)
    out = {"pv": _f(count), "ifault": _i(count), "liu": _f(count), "flags": _i(count)}
    keys = ("pv", "ifault", "liu", "flags")
    if bounds:
        out["bound_Q"], out["bound_p"] = _f(count), _f(count)
        keys += ("bound_Q", "bound_p")
    fn = lib.crm_scan_interaction_bounds if bounds else lib.crm_scan_interaction_info
    _lib.check(fn(objs[0]._bind_gene(), panel.handle, first, count, _lib.ptr(iE), _lib.ptr(iG), *_ptrs(out, keys)))
    return out, {k: 0 for k in out}


def _bounds(objs, panel, first, count, **hooks):
    return _info(objs, panel, first, count, bounds=True, **hooks)


def _multi(objs, panel, first, count, tail=False):
    from cellregmap_amd import _lib

    lib, _ = _lib_ctx()
    ng = len(objs)
    handles = (ctypes.c_void_p * ng)(*[o._bind_gene().value for o in objs])
    out = {k: _f(ng, count) for k in SHORT}
    keys = SHORT
    if tail:
        out["logp"], out["status"] = _f(ng, count), _i(ng, count)
        keys += ("logp", "status")
    fn = lib.crm_scan_interaction_multi_tail if tail else lib.crm_scan_interaction_multi
    _lib.check(fn(handles, ng, panel.handle, first, count, None, None, *_ptrs(out, keys)))
    return out, {k: 1 for k in out}


def _multi_tail(objs, panel, first, count):
    return _multi(objs, panel, first, count, tail=True)


def _permuted(objs, panel, first, count, hook="idx_E", tail=False):
    """Three permutations in one call: p and Q (and log p, status) per permutation, rho* and the components once."""
    from cellregmap_amd import _lib

    lib, _ = _lib_ctx()
    perms = _perms(panel.shape[0])
    out = {"pv": _f(NPERM, count), "Q": _f(NPERM, count)}
    out.update({k: _f(count) for k in ("rho1", "e2", "g2", "eps2")})
    keys = ("pv", "rho1", "e2", "g2", "eps2", "Q")
    if tail:
        out["logp"], out["status"] = _f(NPERM, count), _i(NPERM, count)
        keys += ("logp", "status")
    fn = lib.crm_scan_interaction_permuted_tail if tail else lib.crm_scan_interaction_permuted
    _lib.check(fn(objs[0]._bind_gene(), panel.handle, first, count, NPERM, _lib.ptr(perms if hook == "idx_E" else None),
                  _lib.ptr(perms if hook == "idx_G" else None), *_ptrs(out, keys)))
    return out, {k: (1 if out[k].ndim == 2 else 0) for k in out}


#: name -> (call, passes that mark per call)
ENTRIES = {
    "plain": (_plain, 1),
    "info": (_info, 1),
    "bounds": (_bounds, 1),
    "tail": (_tail, 1),
    "multi": (_multi, 1),
    "multi_tail": (_multi_tail, 1),
    "permuted idx_E": (lambda *a: _permuted(*a, hook="idx_E"), NPERM),
    "permuted idx_G": (lambda *a: _permuted(*a, hook="idx_G"), NPERM),
    "permuted_tail idx_E": (lambda *a: _permuted(*a, hook="idx_E", tail=True), NPERM),
    "permuted_tail idx_G": (lambda *a: _permuted(*a, hook="idx_G", tail=True), NPERM),
}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _cut(a, axis, off, ln):
    return a[off:off + ln] if axis == 0 else a[:, off:off + ln]


def _where(a, b, axis):
    """Positions along the variant axis at which two arrays differ as bit patterns."""
    diff = np.moveaxis(_bits(a) != _bits(b), axis, 0)
    return np.flatnonzero(diff.reshape(diff.shape[0], -1).any(axis=1))


def _written(out, what):
    """No array keeps the fill the caller put there (NaN / -99) -- Q, p and the rest of these cohorts are finite."""
    for k, a in out.items():
        assert not np.any(a == -99) if a.dtype == np.int32 else np.all(np.isfinite(a)), (what, k)


def _flags_follow_bounds(out, what):
    flags, bq, bp = out["flags"], out["bound_Q"], out["bound_p"]
    assert np.array_equal((flags & 8) != 0, ~(bp <= 1e-5)), (what, "flat optimum", np.flatnonzero(((flags & 8) != 0) != ~(bp <= 1e-5)))
    assert np.array_equal((flags & 32) != 0, ~(bq <= 1e-6)), (what, "statistic at tolerance",
                                                               np.flatnonzero(((flags & 32) != 0) != ~(bq <= 1e-6)))


CASES = [(lay, ctor) for lay in ("scattered", "window", "quarter") for ctor in ("from_donors", "auto")] + [("dosages", "dosages")]


# ---- a, b: positions bit for bit, flags against bounds, the counter -------------------------------------------------------
@pytest.mark.parametrize("name,ctor", CASES)
@pytest.mark.parametrize("mode", ["B", "C"])
def test_every_entry_point_repeats_in_place(mode, name, ctor, kernel_form):
    from test_gpu_unrelated_donors import _blocks

    lay = drc.layout(name)
    first, count, runs, marked = lay.first, lay.count, lay.runs, len(lay.in_range)
    assert marked > 0 and runs
    with _background(kernel_form, mode):
        objs = _objects(mode, lay)
        panel = _panel(lay, ctor)
        for entry, (call, passes) in ENTRIES.items():
            what = (mode, name, ctor, entry)
            before, ud = _repeats(), _blocks()
            full, axis = call(objs, panel, first, count)
            # (a permuted call under idx_G stays on the collapsed path -- 9 donors meet the mixed table's m <= 128 -- or
            # the counter would not move at all)
            assert _repeats() - before == passes * marked, (what, _repeats() - before, passes, marked)
            if mode == "C":      # (a collapsed block does not count: the repeats ran on the unrelated-donor route)
                assert _blocks() > ud, what
            _written(full, what)
            with _collapse_off():
                before = _repeats()
                for off, ln in runs:
                    part, _ = call(objs, panel, first + off, ln)
                    assert part.keys() == full.keys()
                    for k in full:
                        got = _cut(full[k], axis[k], off, ln)
                        assert got.shape == part[k].shape, (what, k)
                        assert np.array_equal(_bits(got), _bits(part[k])), (what, k, off, ln, _where(got, part[k], axis[k]))
                assert _repeats() == before, what
            if entry == "plain" and lay.dosage is None:
                # neighbouring variants differ clearly: a result one position off cannot pass a tolerance
                Q = full["Q"]
                for j in lay.in_range:
                    for nb in (j - 1, j + 1):
                        if 0 <= nb < count:
                            assert abs(Q[j] - Q[nb]) > 1e-3 * max(abs(Q[j]), abs(Q[nb])), (what, j, nb, Q[j], Q[nb])


@pytest.mark.parametrize("name,ctor", CASES)
@pytest.mark.parametrize("mode", ["B", "C"])
def test_flags_follow_the_bounds_at_every_position(mode, name, ctor, kernel_form):
    """(b), a test of its own so that it speaks whatever (a) found: flags and bounds of crm_scan_interaction_bounds on the
    grouped panel obey the rule of ScanPass::flat_probes, and the grouped panel's own bounds are informative."""
    lay = drc.layout(name)
    with _background(kernel_form, mode):
        objs = _objects(mode, lay)
        before = _repeats()
        full, _ = _bounds(objs, _panel(lay, ctor), lay.first, lay.count)
        assert _repeats() - before == len(lay.in_range)
    _written(full, (mode, name, ctor))
    _flags_follow_bounds(full, (mode, name, ctor))
    parity_bounds.assert_bounds_are_informative(full["bound_Q"], full["bound_p"], full["pv"])


# ---- d: every position against the dense panel ------------------------------------------------------------------------------
def _agree(got, want, bq, bp, scale, what):
    """``got`` on the grouped panel, ``want`` the same call on the dense one: the bar of tests/parity_bounds.py."""
    if "Q" in got:
        parity_bounds.assert_Q_within(got["Q"], want["Q"], bq, scale, what)
    parity_bounds.assert_p_within(got["pv"], want["pv"], bp, what)
    if "rho1" in got:
        assert_allclose(got["rho1"], want["rho1"], rtol=0, atol=1e-12, err_msg=str(what))
    if "status" in got:
        assert np.array_equal(got["status"], want["status"]), what


def _dense_bar(obj, dense, first, count, **hooks):
    """(bound_Q, bound_p, max(|Q|, tr F)) of one phenotype's call on the dense panel."""
    ref, _ = _plain([obj], dense, first, count, **hooks)
    bnd, _ = _bounds([obj], dense, first, count, **hooks)
    scale = np.maximum(np.abs(ref["Q"]), np.trace(ref["F"], axis1=1, axis2=2))
    return bnd["bound_Q"], bnd["bound_p"], scale


@pytest.mark.parametrize("name,ctor", [("scattered", "from_donors"), ("window", "auto"), ("quarter", "from_donors"),
                                       ("dosages", "dosages")])
@pytest.mark.parametrize("mode", ["B", "C"])
def test_grouped_and_dense_panels_agree_at_every_position(mode, name, ctor, kernel_form):
    lay = drc.layout(name)
    first, count = lay.first, lay.count
    with _background(kernel_form, mode):
        objs = _objects(mode, lay)
        grouped, dense = _panel(lay, ctor), _panel(lay, "dense")
        bars = [_dense_bar(o, dense, first, count) for o in objs]
        bq, bp, scale = bars[0]
        for entry in ("plain", "tail", "info", "bounds"):
            call = ENTRIES[entry][0]
            before = _repeats()
            want = call(objs, dense, first, count)[0]
            assert _repeats() == before                           # (a dense panel has nothing to repeat)
            _agree(call(objs, grouped, first, count)[0], want, bq, bp, scale, (mode, name, entry))
        bq3, bp3, scale3 = (np.stack([b[i] for b in bars]) for i in range(3))
        for entry in ("multi", "multi_tail"):
            call = ENTRIES[entry][0]
            _agree(call(objs, grouped, first, count)[0], call(objs, dense, first, count)[0], bq3, bp3, scale3, (mode, name, entry))
        # the replayed permutations: each row is the single hooked scan, bit for bit (tests/test_gpu_permutations.py), and
        # that scan agrees with the dense panel's
        perms = _perms(lay.y.size)
        for hook in ("idx_E", "idx_G"):
            many = _permuted(objs, grouped, first, count, hook=hook)[0]
            many_tail = _permuted(objs, grouped, first, count, hook=hook, tail=True)[0]
            for b in range(NPERM):
                what = (mode, name, hook, b)
                one = _plain(objs, grouped, first, count, **{hook: perms[b]})[0]
                one_tail = _tail(objs, grouped, first, count, **{hook: perms[b]})[0]
                for k in ("pv", "Q"):
                    assert np.array_equal(_bits(many[k][b]), _bits(one[k])), (what, k)
                for k in ("pv", "Q", "logp", "status"):
                    assert np.array_equal(_bits(many_tail[k][b]), _bits(one_tail[k])), (what, "tail", k)
                for k in ("rho1", "e2", "g2", "eps2"):
                    assert np.array_equal(_bits(many[k]), _bits(one[k])) and np.array_equal(_bits(many_tail[k]), _bits(one[k])), (what, k)
                hbq, hbp, hscale = _dense_bar(objs[0], dense, first, count, **{hook: perms[b]})
                _agree(one, _plain(objs, dense, first, count, **{hook: perms[b]})[0], hbq, hbp, hscale, what)
                _agree(one_tail, _tail(objs, dense, first, count, **{hook: perms[b]})[0], hbq, hbp, hscale, what + ("tail",))


# ---- c: values against the pinned reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["B", "C"])
def test_repeated_variants_against_the_pinned_reference(mode, kernel_form):
    """The plain scan with return_stats=True on "scattered", held by tests/test_gpu_pinned.py::_hold with its unchanged
    limits (32 x the float64 oracle's own error, floored at n x 2.2e-16, capped at 1e-11) at every run's first and last
    variant, the unmarked neighbour on either side of every run, and variant 0; then once more at the marked variants alone
    (the same reference points), so that the record names the errors there."""
    import test_gpu_pinned as tp

    lay = drc.layout("scattered")
    sel = {0}
    for off, ln in lay.runs:
        sel |= {off, off + ln - 1} | {v for v in (off - 1, off + ln) if 0 <= v < lay.count}
    sel = sorted(sel)
    assert set(sel) >= {0, 2, 3, 34, 35, 66, 67, 68, 126, 127, 128, 129, 298, 299}
    edges = [v for v in sel if v in lay.marked]
    with _background(kernel_form, mode):
        obj = _objects(mode, lay)[0]
        results = []
        for ctor in ("from_donors", "auto"):
            before = _repeats()
            results.append((ctor, obj.scan_interaction(_panel(lay, ctor), return_stats=True)))
            assert _repeats() - before == len(lay.marked)
    prob = tp.Problem(lay.y, lay.W, lay.E, lay.G, **_oracle_background(mode, lay))
    try:
        for case, variants in (("dense repeats, scattered, mode %s" % mode, sel),
                               ("dense repeats, scattered, mode %s, marked variants" % mode, edges)):
            tp._hold(case, prob, results, sel=variants)
            RECORD[case] = tp.RECORD[case]
    finally:
        for case in list(tp.RECORD):           # (this module keeps its own record)
            if case.startswith("dense repeats"):
                del tp.RECORD[case]


# ---- e: the Python routes ---------------------------------------------------------------------------------------------------
WINDOWS = ((0, 300), (130, 280), (60, 70))


@pytest.mark.parametrize("mode", ["B", "C"])
def test_cis_windows_on_a_resident_grouped_panel(mode, kernel_form):
    """scan_interaction_many with contiguous windows on a grouped panel scans window by window on the resident panel
    (first > 0); (60, 70) holds one marked variant at offset 7."""
    import cellregmap_amd as crm

    lay = drc.layout("scattered")
    assert [j - 60 for j in lay.marked if 60 <= j < 70] == [7]
    inside = sum(a <= j < b for a, b in WINDOWS for j in lay.marked)
    with _background(kernel_form, mode):
        objs = _objects(mode, lay)
        panel = _panel(lay, "from_donors")
        before = _repeats()
        pv, info = crm.scan_interaction_many(objs, panel, cis_index=list(WINDOWS))
        assert _repeats() - before == inside == 7
        for i, (a, b) in enumerate(WINDOWS):
            alone = crm.GenotypePanel(lay.G[:, a:b], groups=None)
            bq, bp, xi = parity_bounds.bounds(objs[i], alone)
            opv, oinfo = objs[i].scan_interaction(alone)
            assert pv[i].shape == (b - a,)
            parity_bounds.assert_p_within(pv[i], opv, bp, (mode, a, b))
            assert_allclose(info["rho1"][i], oinfo["rho1"], rtol=0, atol=1e-12)
            # ... and bit for bit the C-ABI call over the window (the run inside it written at its offset)
            direct = _plain([objs[i]], panel, a, b - a)[0]
            assert np.array_equal(_bits(pv[i]), _bits(direct["pv"])) and np.array_equal(_bits(info["e2"][i]), _bits(direct["e2"]))


def test_streamed_chunks_take_the_repeats(monkeypatch, kernel_form):
    """A host matrix in chunks of 64 variants, every chunk a grouped panel of its own: the tolerances of
    tests/test_gpu_tail_pvalue.py::test_streamed_chunks_and_run_interaction."""
    lay = drc.layout("scattered")
    with _background(kernel_form, "B"):
        obj = _objects("B", lay)[0]
        monkeypatch.setenv("CELLREGMAP_AMD_STREAM_CHUNK", "0")
        before = _repeats()
        pv, info = obj.scan_interaction(lay.G, pvalue="exact")
        assert _repeats() - before == len(lay.marked)
        monkeypatch.setenv("CELLREGMAP_AMD_STREAM_CHUNK", "64")
        before = _repeats()
        spv, sinfo = obj.scan_interaction(lay.G, pvalue="exact")
        assert _repeats() - before == len(lay.marked)
    assert np.allclose(spv, pv, rtol=1e-9, atol=0) and np.array_equal(sinfo["pvalue_status"], info["pvalue_status"])
    assert sinfo["log_pvalue"].shape == pv.shape and np.all(info["pvalue_status"] == 0)


def test_progress_reports_every_variant_once(kernel_form):
    """The repeats run with the callback muted (crm_ctx::progress_muted): blocks of 128 over 300 variants report 128, 256,
    300 and nothing after."""
    lay = drc.layout("scattered")
    seen = []
    with _background(kernel_form, "B"):
        obj = _objects("B", lay)[0]
        panel = _panel(lay, "from_donors")
        before = _repeats()
        obj.scan_interaction(panel, progress=lambda done, total: seen.append((done, total)))
        assert _repeats() - before == len(lay.marked)
        assert seen == [(128, 300), (256, 300), (300, 300)], seen
        # the flag is put back: the next scan reports again
        seen.clear()
        obj.scan_interaction(panel, progress=lambda done, total: seen.append((done, total)))
        assert seen == [(128, 300), (256, 300), (300, 300)], seen
