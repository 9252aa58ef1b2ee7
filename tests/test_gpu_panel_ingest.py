"""What the four panel builders put on the device, read back (include/crm_hip_test.h: crm_test_panel_layout,
crm_test_panel_read) and held to tests/panel_reference.py: the standardised int8 dosages entry by entry within the
reference's a-priori bound, everything else bit for bit, the padding of every buffer +0.0 by bit pattern (the contraction
tiles over-read into it).  tests/test_panel_reference_cpu.py shows that the bound separates a faithful kernel from a
subtly wrong one on these very cohorts.

Worst |got - ref| / bound of standardise_dosages_kernel on an MI355X, per cohort (a record, not a threshold):
a (9 donors) 0.0253, b (65) 0.0572, c (257) 0.148, d (300) 0.176 -- what a faithful float64 evaluation on the host gives."""
import contextlib
import ctypes

import numpy as np
import pytest

import panel_reference as pr

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_NUMERIC = 0, -2, -4
WHAT_G, WHAT_GD, WHAT_GROUP, WHAT_Z = 0, 1, 2, 3


def _lib_ctx():
    from cellregmap_amd import _engine, _lib

    return _lib.load(), _engine._context(0)


def _live():
    return _lib_ctx()[0].crm_test_live_device_bytes()


def _forget_groupings():
    from cellregmap_amd import _engine

    _engine._last_grouping.clear()


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float64
    return a.view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _all_plus_zero(a):
    return not _bits(a).any()


def _read_buffer(handle, what, shape, dtype):
    from cellregmap_amd import _lib

    lib, _ = _lib_ctx()
    out = np.full(shape, -1 if dtype == np.int32 else np.nan, dtype)      # (whatever the copy leaves out shows)
    _lib.check(lib.crm_test_panel_read(handle, what, _lib.ptr(out), out.nbytes))
    return out


def _refused(handle, what, nbytes):
    """The status of a read that must not succeed, and the library's message."""
    lib, _ = _lib_ctx()
    dst = np.zeros(max(nbytes, 8), np.uint8)
    rc = lib.crm_test_panel_read(handle, what, dst.ctypes.data_as(ctypes.c_void_p), nbytes)
    assert not dst.any()
    return rc, lib.crm_last_error().decode()


def read_panel(handle):
    """Everything a panel holds, as it lies in device memory: the layout and the whole padded buffers."""
    from cellregmap_amd import _lib

    lib, _ = _lib_ctx()
    lay = (ctypes.c_long * 8)()
    _lib.check(lib.crm_test_panel_layout(handle, lay))
    r = dict(zip(("n", "n_pad", "p", "ld", "grouped", "m", "m_pad", "ldz"), (int(v) for v in lay)))
    assert r["n_pad"] >= r["n"] and r["n_pad"] % 128 == 0 and r["ld"] >= r["p"] and r["ld"] % 128 == 0
    if r["grouped"]:
        assert r["m_pad"] >= r["m"] > 0 and r["ldz"] >= r["m"]
        r["Gd"] = _read_buffer(handle, WHAT_GD, (r["m_pad"], r["ld"]), np.float64)
        r["group"] = _read_buffer(handle, WHAT_GROUP, (r["n"],), np.int32)
        r["Z"] = _read_buffer(handle, WHAT_Z, (r["n_pad"], r["ldz"]), np.float64)
        rc, msg = _refused(handle, WHAT_G, r["n_pad"] * r["ld"] * 8)
        assert rc == ERR_ARG and "holds no G" in msg
        rc, msg = _refused(handle, WHAT_GD, r["Gd"].nbytes - 8)             # not the buffer's size
        assert rc == ERR_ARG and "bytes" in msg
    else:
        r["G"] = _read_buffer(handle, WHAT_G, (r["n_pad"], r["ld"]), np.float64)
        rc, msg = _refused(handle, WHAT_GD, 8)
        assert rc == ERR_ARG and "holds no Gd" in msg
        rc, msg = _refused(handle, WHAT_G, r["G"].nbytes + 8)
        assert rc == ERR_ARG and "bytes" in msg
    return r


def check_grouped(r, n, m, p, donor_of_cell):
    """The donor structure of a grouped panel and the padding of its buffers; returns Gd[:m, :p]."""
    assert (r["grouped"], r["n"], r["m"], r["p"]) == (1, n, m, p)
    assert np.array_equal(r["group"], donor_of_cell)
    assert _same_bits(r["Z"][:n, :m], pr.indicator(donor_of_cell, m))
    assert _all_plus_zero(r["Z"][n:]) and _all_plus_zero(r["Z"][:, m:])
    assert _all_plus_zero(r["Gd"][m:]) and _all_plus_zero(r["Gd"][:, p:])
    return r["Gd"][:m, :p]


def check_dense(r, G):
    n, p = G.shape
    assert (r["grouped"], r["n"], r["p"]) == (0, n, p)
    assert _same_bits(r["G"][:n, :p], np.ascontiguousarray(G))
    assert _all_plus_zero(r["G"][n:]) and _all_plus_zero(r["G"][:, p:])


@contextlib.contextmanager
def created(call):
    """A panel made by a direct call of the C-ABI -- ``call(pointer to the handle)`` returns the status --, destroyed on
    the way out; yields ``(status, handle)``."""
    lib, _ = _lib_ctx()
    h = ctypes.c_void_p()
    rc = call(ctypes.byref(h))
    try:
        yield rc, h
    finally:
        if h.value:
            lib.crm_panel_destroy(h)


def _dosage_panel(c, standardize):
    """The cohort's panel: through ``from_dosages`` where the int8 matrix is tight, through the C-ABI with the leading
    dimension of the wider matrix where the cohort is a column window of one (``ldd > p``)."""
    from cellregmap_amd import GenotypePanel

    lib, ctx = _lib_ctx()
    donor = c["donor_of_cell"]
    if c["ldd"] == c["p"]:
        panel = GenotypePanel.from_dosages(c["D"], donor, standardize=standardize)
        assert panel.n_groups == c["m"] and panel.shape == (donor.shape[0], c["p"])
        return contextlib.nullcontext((OK, panel.handle, panel))
    window = ctypes.c_void_p(c["wide"].ctypes.data + c["col0"])

    @contextlib.contextmanager
    def direct():
        with created(lambda out: lib.crm_panel_create_grouped_i8(ctx, donor.shape[0], donor.ctypes.data_as(ctypes.c_void_p),
                                                                 c["m"], window, c["ldd"], c["p"], int(standardize), out)) as (rc, h):
            yield rc, h, None
    return direct()


# ---- int8 dosages ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pr.COHORTS))
def test_standardised_dosages_are_within_the_bound_of_the_reference(name):
    from cellregmap_amd import GenotypePanel

    c = pr.cohort(name)
    donor, m, p = c["donor_of_cell"], c["m"], c["p"]
    ref, bound = pr.standardised(c["D"], donor)
    with _dosage_panel(c, True) as (rc, handle, _):
        assert rc == OK
        got = check_grouped(read_panel(handle), donor.shape[0], m, p, donor)
    ratio = pr.worst_ratio(got, ref, bound)
    print("[panel-ingest] cohort %s (m = %d, p = %d, ldd = %d): worst |got - ref| / bound = %.3g" % (name, m, p, c["ldd"], ratio))
    assert np.all(np.abs(got.astype(pr.LD) - ref) <= bound)
    if c["ldd"] > p:        # the same window as a tight copy through the Python constructor: the same bits
        tight = GenotypePanel.from_dosages(np.ascontiguousarray(c["D"]), donor)
        assert _same_bits(check_grouped(read_panel(tight.handle), donor.shape[0], m, p, donor), got)


@pytest.mark.parametrize("name", sorted(pr.COHORTS))
def test_unstandardised_dosages_are_the_integers(name):
    c = pr.cohort(name)
    donor = c["donor_of_cell"]
    with _dosage_panel(c, False) as (rc, handle, _):
        assert rc == OK
        got = check_grouped(read_panel(handle), donor.shape[0], c["m"], c["p"], donor)
    assert _same_bits(got, c["D"].astype(np.float64))


def _monomorphic_cases():
    b, d = pr.cohort("b"), pr.cohort("d")
    first, last = b["D"].copy(), b["D"].copy()
    first[:, 0] = 1
    last[:, -1] = -128
    only = np.full((b["m"], 1), 2, np.int8)
    absent = d["D"].copy()                       # varies over the donors, not over the cells: the one carrier has no cell
    absent[:, 40] = 0
    absent[d["empty_donor"], 40] = 1
    return {"first": (first, b), "last": (last, b), "only": (only, b), "carrier_without_cells": (absent, d)}


@pytest.mark.parametrize("case", ["first", "last", "only", "carrier_without_cells"])
def test_a_monomorphic_variant_is_refused_and_leaves_nothing_behind(case):
    from cellregmap_amd import GenotypePanel

    D, c = _monomorphic_cases()[case]
    donor = c["donor_of_cell"]
    assert pr.monomorphic(D, donor).sum() == 1
    if case == "carrier_without_cells":
        assert not (D == D[0]).all(0).any()                   # no column is constant over the donors
    GenotypePanel.from_dosages(c["D"], donor)                 # (the context and its buffers exist from here on)
    before = _live()
    with pytest.raises(ValueError, match="monomorphic"):
        GenotypePanel.from_dosages(D, donor)
    assert _live() == before
    raw = GenotypePanel.from_dosages(D, donor, standardize=False)         # raw counts have nothing to divide by
    assert _same_bits(check_grouped(read_panel(raw.handle), donor.shape[0], c["m"], D.shape[1], donor), D.astype(np.float64))
    panel = GenotypePanel.from_dosages(c["D"], donor)
    got = check_grouped(read_panel(panel.handle), donor.shape[0], c["m"], c["p"], donor)
    ref, bound = pr.standardised(c["D"], donor)
    assert np.all(np.abs(got.astype(pr.LD) - ref) <= bound)
    del raw, panel
    assert _live() == before


# ---- float64 builders ------------------------------------------------------------------------------------------------
def _sprinkle(A):
    """Put into A (in place) the values a copy could lose: subnormals, -0.0, the extremes of the format."""
    rows, cols = A.shape
    A[0, 0], A[-1, -1], A[rows // 2, cols // 2] = -0.0, 5e-324, -2.2250738585072009e-308
    A[0, -1], A[-1, 0] = np.finfo(float).max, -np.finfo(float).tiny
    A[1, 1:4] = (-0.0, 0.0, -5e-324)
    return A


def test_float64_builders_take_a_column_window_by_its_leading_dimension():
    lib, ctx = _lib_ctx()
    rng = np.random.default_rng(1)
    n, p, ldg, col0 = 70, 129, 150, 11
    wide = rng.normal(size=(n, ldg))
    want = np.ascontiguousarray(_sprinkle(wide[:, col0:col0 + p]))
    window = ctypes.c_void_p(wide.ctypes.data + 8 * col0)
    with created(lambda out: lib.crm_panel_create(ctx, n, window, ldg, p, out)) as (rc, h):
        assert rc == OK
        check_dense(read_panel(h), want)
    c = pr.cohort("b")
    donor, m = c["donor_of_cell"], c["m"]
    wide = rng.normal(size=(m, ldg))
    want = np.ascontiguousarray(_sprinkle(wide[:, col0:col0 + p]))
    window = ctypes.c_void_p(wide.ctypes.data + 8 * col0)
    with created(lambda out: lib.crm_panel_create_grouped(ctx, donor.shape[0], donor.ctypes.data_as(ctypes.c_void_p), m,
                                                          window, ldg, p, out)) as (rc, h):
        assert rc == OK
        assert _same_bits(check_grouped(read_panel(h), donor.shape[0], m, p, donor), want)


def _layouts():
    rng = np.random.default_rng(3)
    f32 = rng.normal(size=(70, 131)).astype(np.float32)
    f32[2, 2:5] = (1e-45, -1e-45, -0.0)                                # float32 subnormals widen to normal doubles
    return {
        "column_window": _sprinkle(rng.normal(size=(70, 150))[:, 7:138]),   # rows a fixed number of doubles apart: goes as it lies
        "row_step": _sprinkle(rng.normal(size=(140, 131))[::2]),            # ... and so does every second row
        "column_step": _sprinkle(rng.normal(size=(70, 393))[:, ::3]),
        "fortran": np.asfortranarray(_sprinkle(rng.normal(size=(70, 131)))),
        "float32": f32,
        "integer": rng.integers(-5, 6, size=(70, 131)),
        "bool": rng.random((70, 131)) < 0.3,
    }


@pytest.mark.parametrize("layout", ["column_window", "row_step", "column_step", "fortran", "float32", "integer", "bool"])
def test_genotype_panel_keeps_every_input_layout_bit_for_bit(layout):
    from cellregmap_amd import GenotypePanel

    G = _layouts()[layout]
    want = np.ascontiguousarray(np.asarray(G, float))
    assert want.shape == (70, 131)
    if layout in ("column_window", "row_step", "column_step", "fortran"):
        assert not G.flags.c_contiguous and np.signbit(want[want == 0]).any() and (np.abs(want[want != 0]) < 1e-310).any()
    for groups in (None, "auto"):          # (rows of a general matrix do not collapse: dense either way)
        _forget_groupings()
        panel = GenotypePanel(G, groups=groups)
        assert panel.n_groups is None and panel.shape == (70, 131)
        check_dense(read_panel(panel.handle), want)


# ---- crm_panel_create_auto -------------------------------------------------------------------------------------------
AUTO_N_DONORS, AUTO_P = 40, 257            # the last column alone in the second 256-column chunk of the verification
_auto = {}


def _auto_cohort():
    """About 600 cells of 40 donors in shuffled order, general doubles; the entries the deviations go to are 0.0."""
    if not _auto:
        rng = np.random.default_rng(11)
        donor = rng.permutation(np.repeat(np.arange(AUTO_N_DONORS), rng.integers(5, 26, size=AUTO_N_DONORS)))
        n = donor.shape[0]
        positions = {"first": (0, 0), "last": (n - 1, AUTO_P - 1), "interior": (n // 2 + 1, 123)}
        Gd = rng.normal(size=(AUTO_N_DONORS, AUTO_P))
        for i, j in positions.values():
            Gd[donor[i], j] = 0.0
        # the labels a search gives: donors in order of first appearance; representatives: every donor's LAST cell
        _, first = np.unique(donor, return_index=True)
        relabel = np.empty(AUTO_N_DONORS, np.int32)
        relabel[np.argsort(first)] = np.arange(AUTO_N_DONORS, dtype=np.int32)
        group = relabel[donor].astype(np.int32)
        reps = np.array([np.flatnonzero(group == d)[-1] for d in range(AUTO_N_DONORS)], np.int64)
        G = np.ascontiguousarray(Gd[donor])
        assert 500 <= n <= 700 and np.array_equal(G[reps][group], G)
        for a in (G, group, reps):
            a.setflags(write=False)
        _auto.update(G=G, group=group, reps=reps, n=n, positions=positions)
    return _auto


def _create_auto(G, hint):
    lib, ctx = _lib_ctx()
    grouped = ctypes.c_int(-1)
    n, p = G.shape
    vp = ctypes.c_void_p
    if hint is None:
        call = lambda out: lib.crm_panel_create_auto(ctx, n, G.ctypes.data_as(vp), p, p, None, 0, None, out, ctypes.byref(grouped))
    else:
        group, reps = hint
        call = lambda out: lib.crm_panel_create_auto(ctx, n, G.ctypes.data_as(vp), p, p, group.ctypes.data_as(vp),
                                                     reps.shape[0], reps.ctypes.data_as(vp), out, ctypes.byref(grouped))
    return created(call), grouped


def check_auto_grouped(r, a):
    got = check_grouped(r, a["n"], AUTO_N_DONORS, AUTO_P, a["group"])
    assert _same_bits(got, np.ascontiguousarray(a["G"][a["reps"]]))


def test_auto_with_a_hint_that_holds_stores_the_representative_rows():
    from cellregmap_amd import GenotypePanel

    a = _auto_cohort()
    panel_cm, grouped = _create_auto(a["G"], (a["group"], a["reps"]))
    with panel_cm as (rc, h):
        assert rc == OK and grouped.value == 1
        check_auto_grouped(read_panel(h), a)            # (read_panel: the dense copy has been released, CRM_ERR_ARG)
    panel_cm, grouped = _create_auto(a["G"], None)     # no hint: verified for non-finite entries only, kept dense
    with panel_cm as (rc, h):
        assert rc == OK and grouped.value == 0
        check_dense(read_panel(h), a["G"])
    _forget_groupings()
    for _ in range(2):                                  # the search, then the cached grouping: the same panel
        panel = GenotypePanel(a["G"])
        assert panel.n_groups == AUTO_N_DONORS
        check_auto_grouped(read_panel(panel.handle), a)


@pytest.mark.parametrize("where", ["first", "last", "interior"])
def test_auto_keeps_a_panel_dense_for_one_deviating_entry(where):
    a = _auto_cohort()
    i, j = a["positions"][where]
    assert a["G"][i, j] == 0.0 and not np.signbit(a["G"][i, j])
    for value in (5e-324, 1.0, -0.0):                   # the last bit, a dosage, and only the sign of zero
        G = a["G"].copy()
        G[i, j] = value
        panel_cm, grouped = _create_auto(G, (a["group"], a["reps"]))
        with panel_cm as (rc, h):
            assert rc == OK and grouped.value == 0, value
            check_dense(read_panel(h), G)


@pytest.mark.parametrize("where", ["first", "last", "interior"])
def test_auto_refuses_non_finite_entries_with_and_without_a_hint(where):
    from cellregmap_amd import GenotypePanel, _engine

    a = _auto_cohort()
    i, j = a["positions"][where]
    _forget_groupings()
    GenotypePanel(a["G"])                               # (context up; the grouping is now the cached hint)
    assert a["n"] in _engine._last_grouping
    before = _live()
    for value in (np.nan, np.inf, -np.inf):
        G = a["G"].copy()
        G[i, j] = value
        for hint in (None, (a["group"], a["reps"])):
            panel_cm, _ = _create_auto(G, hint)
            with panel_cm as (rc, h):
                assert rc == ERR_NUMERIC and not h.value, (value, hint is None)
            assert _live() == before
        with pytest.raises(ValueError, match="non-finite"):
            GenotypePanel(G, groups=None)
        with pytest.raises(ValueError, match="non-finite"):
            GenotypePanel(G)                            # tries the cached grouping first
        assert _live() == before
        panel = GenotypePanel(a["G"])                   # ... and the next panel builds
        assert panel.n_groups == AUTO_N_DONORS
        check_auto_grouped(read_panel(panel.handle), a)
        del panel


def test_the_grouping_of_the_previous_panel_is_only_ever_a_hint():
    """Four panels with the same number of cells in a row: each is stored by its own structure, whatever the cache held."""
    from cellregmap_amd import GenotypePanel

    rng = np.random.default_rng(5)
    n, p = 240, 70
    s1, s2 = (np.arange(n) // 20).astype(np.int32), (np.arange(n) % 15).astype(np.int32)   # neither refines the other
    Gd1, Gd2 = rng.normal(size=(12, p)), rng.normal(size=(15, p))
    general = rng.normal(size=(n, p))
    _forget_groupings()
    for group, Gd in ((s1, Gd1), (s2, Gd2), (None, None), (s1, Gd1), (s1, Gd1)):
        if group is None:
            panel = GenotypePanel(general)
            assert panel.n_groups is None
            check_dense(read_panel(panel.handle), general)
            continue
        panel = GenotypePanel(np.ascontiguousarray(Gd[group]))
        assert panel.n_groups == Gd.shape[0]
        assert _same_bits(check_grouped(read_panel(panel.handle), n, Gd.shape[0], p, group), Gd)


# ---- what the scans read ---------------------------------------------------------------------------------------------
def test_scans_read_the_buffer_that_was_held_to_the_reference():
    """The scale-sensitive outputs (beta, beta_se) and every other returned array of a scan on ``from_dosages`` are, bit for
    bit, those of the same scan on ``from_donors`` of the standardised matrix read back from the device."""
    from cellregmap_amd import CellRegMap, GenotypePanel

    c = pr.cohort("b")
    donor, m, p = c["donor_of_cell"], c["m"], c["p"]
    n = donor.shape[0]
    rng = np.random.default_rng(6)
    E = rng.normal(size=(n, 3))
    W = np.column_stack([np.ones(n), rng.normal(size=n)])
    ref, _ = pr.standardised(c["D"], donor)
    g = ref.astype(float)[donor]
    y = 0.4 * g[:, 0] + 0.5 * g[:, 1] * E[:, 0] + 0.3 * E @ rng.normal(size=3) + rng.normal(size=n)
    crm = CellRegMap(y, E, W=W, hK=pr.indicator(donor, m))
    dosages = GenotypePanel.from_dosages(c["D"], donor)
    held = check_grouped(read_panel(dosages.handle), n, m, p, donor)
    donors = GenotypePanel.from_donors(held, donor)
    assert _same_bits(check_grouped(read_panel(donors.handle), n, m, p, donor), held)

    def flat(result):
        out = {"pv": result[0]}
        for part in result[1:]:
            out.update(part)
        return {k: np.atleast_1d(np.asarray(v)) for k, v in out.items()}

    for scan in (lambda panel: crm.scan_interaction(panel, return_stats=True),
                 lambda panel: crm.scan_association_fast(panel, effects=True)):
        one, other = flat(scan(dosages)), flat(scan(donors))
        assert sorted(one) == sorted(other) and "pv" in one
        for key in one:
            assert one[key].dtype == other[key].dtype and one[key].tobytes() == other[key].tobytes(), key
        assert np.all(np.isfinite(one["pv"]))
        if "beta" in one:
            assert np.all(np.isfinite(one["beta"])) and np.all(one["beta_se"] > 0)
