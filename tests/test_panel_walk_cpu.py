"""The host side of the scans without a GPU: the walk of the single-phenotype scans over a panel (resident, streamed in
column chunks, empty), ``scan_interaction_many`` whole and along cis windows, and the cohort binding, with the library
stubbed.  Every stubbed entry point writes, for every output, a function of (output name, phenotype, true panel column),
so a misplaced slice, a wrong offset or a swapped output fails on equality."""
import ctypes
import sys
import threading
import types
import warnings

import numpy as np
import pytest

from cellregmap_amd import _engine, _lib

N, K0, CHUNK = 6, 2, 4
NULL = [0.5, 1.0, 2.0, 3.0, -100.0, 0.25]
INFO = ("rho1", "e2", "g2", "eps2")
STATS = (("Q", ()), ("lml", ()), ("delta", ()), ("scale", ()), ("lambda", (K0,)), ("F", (K0, K0)))
EFFECTS = ("beta", "beta_se", "alt_delta", "alt_scale", "log_pvalue", "effect_status")
INTS = ("pvalue_status", "effect_status", "status", "dof", "dropped")
NAMES = ("pv",) + INFO + tuple(k for k, _ in STATS) + EFFECTS + ("pvalue_status", "alt_lml", "status", "null_lml",
                                                                   "null_delta", "dof", "dropped")
# the outputs of the context entry points in the order of the C-ABI: (name, per context?)
CONTEXTS = (("pv", True), ("alt_lml", True), ("beta", True), ("beta_se", True), ("log_pvalue", True), ("status", True),
            ("null_lml", False), ("null_delta", False))
JOINT = (("pv", False), ("log_pvalue", False), ("alt_lml", False), ("dof", False), ("beta", True), ("beta_se", True),
         ("dropped", True), ("status", False), ("null_lml", False), ("null_delta", False))


def _value(name, gene, cols, trailing=()):
    """What the stubs write for (output, phenotype, true panel columns): (len(cols), *trailing), float64 or int32."""
    cols = np.asarray(cols, np.int64)
    inner = np.zeros(trailing, np.int64)
    for axis, size in enumerate(trailing):
        inner = inner + np.arange(size).reshape([-1 if a == axis else 1 for a in range(len(trailing))]) * 10 ** axis
    grid = cols.reshape((-1,) + (1,) * len(trailing))
    if name in INTS:
        return ((grid + inner) % 2 if name == "dropped" else 100 * grid + 10 * gene + inner + NAMES.index(name)).astype(np.int32)
    return 1e6 * (1 + NAMES.index(name)) + 1e3 * gene + grid + inner / 64.0


def _write(pointer, name, genes, cols, trailing=(), lead=False):
    """Fill the output behind ``pointer``: (len(cols), *trailing), with a leading phenotype axis when ``lead``."""
    if pointer is None:
        return
    kind = ctypes.c_int if name in INTS else ctypes.c_double
    shape = (len(genes),) * lead + (len(cols),) + tuple(trailing)
    if int(np.prod(shape)) == 0:
        return
    out = np.ctypeslib.as_array(ctypes.cast(pointer, ctypes.POINTER(kind)), shape=shape)
    out[...] = np.stack([_value(name, g, cols, trailing) for g in genes]) if lead else _value(name, genes[0], cols, trailing)


def _gene_id(gene):
    return int(gene.value if hasattr(gene, "value") else gene) - 100


class _StubLib:
    """Stands behind ``_lib.load``: records every call, fills the outputs, reports two variants at a time."""

    def __init__(self):
        self.calls, self.created, self.callbacks, self.fail_on_scan = [], [], [], None
        self._callback = None

    # ---- objects and the progress callback
    def crm_gene_create(self, bg, y, W, ncov, E0, k0, out):
        self.created.append(("single", 1))
        out._obj.value = 100
        return 0

    def crm_gene_create_batch(self, like, Y, n, count, handles):
        self.created.append(("batch", count))
        for i in range(count):
            handles[i] = like.value + 1 + i
        return 0

    def crm_gene_destroy(self, handle):
        return 0

    def crm_last_error(self):
        return b"stub failure"

    def crm_set_progress_callback(self, ctx, callback, user):
        self.callbacks.append(callback)
        self._callback = None if callback is None else ctypes.cast(callback, _engine._PROGRESS_CB)
        return 0

    def _scan(self, entry, genes, panel, first, count):
        """Record the call; the true columns it covers, or None when it is the call that fails."""
        self.calls.append((entry, genes, panel, int(first), int(count)))
        if self.fail_on_scan == len(self.calls):
            return None
        assert 0 <= first and first + count <= panel.shape[1]
        return panel.cols[first:first + count]

    def _report(self, count):
        if self._callback is not None:
            for done in list(range(2, count, 2)) + [count]:
                self._callback(done, count, None)

    # ---- the interaction scan, one phenotype and many
    def _interaction(self, entry, genes, panel, first, count, iE, iG, five, stats, tail, lead):
        cols = self._scan(entry, genes, panel, first, count)
        if cols is None:
            return -1
        for name, pointer in zip(("pv",) + INFO, five):
            _write(pointer, name, genes, cols, lead=lead)
        for (name, trailing), pointer in zip(STATS, stats):
            _write(pointer, name, genes, cols, trailing, lead=lead)
        for name, pointer in zip(("log_pvalue", "pvalue_status"), tail):
            _write(pointer, name, genes, cols, lead=lead)
        self._report(count)
        return 0

    def crm_scan_interaction(self, gene, panel, first, count, iE, iG, *out):
        assert len(out) == 11
        return self._interaction("single", [_gene_id(gene)], panel, first, count, iE, iG, out[:5], out[5:], (), False)

    def crm_scan_interaction_tail(self, gene, panel, first, count, iE, iG, *out):
        assert len(out) == 13 and out[11] is not None and out[12] is not None
        return self._interaction("single_tail", [_gene_id(gene)], panel, first, count, iE, iG, out[:5], out[5:11], out[11:], False)

    def crm_scan_interaction_multi(self, hs, ng, panel, first, count, iE, iG, *out):
        assert len(out) == 6 and out[5] is None                                   # (the Q slot stays empty)
        return self._interaction("multi", [_gene_id(hs[i]) for i in range(ng)], panel, first, count, iE, iG, out[:5], (), (), True)

    def crm_scan_interaction_multi_tail(self, hs, ng, panel, first, count, iE, iG, *out):
        assert len(out) == 8 and out[5] is None and out[6] is not None and out[7] is not None
        return self._interaction("multi_tail", [_gene_id(hs[i]) for i in range(ng)], panel, first, count, iE, iG, out[:5], (),
                                 out[6:], True)

    # ---- the association scans
    def _association(self, entry, gene, panel, first, count, fast, pv, alt, null, effects=()):
        cols = self._scan((entry, int(fast)), [_gene_id(gene)], panel, first, count)
        if cols is None:
            return -1
        np.ctypeslib.as_array(ctypes.cast(null, ctypes.POINTER(ctypes.c_double)), shape=(6,))[:] = NULL
        for name, pointer in zip(("pv", "alt_lml") + EFFECTS, (pv, alt) + tuple(effects)):
            _write(pointer, name, [0], cols)
        self._report(count)
        return 0

    def crm_scan_association(self, gene, panel, first, count, fast, pv, alt, null):
        return self._association("association", gene, panel, first, count, fast, pv, alt, null)

    def crm_scan_association_effects(self, gene, panel, first, count, fast, pv, alt, null, *effects):
        assert len(effects) == 6 and all(e is not None for e in effects)
        return self._association("association_effects", gene, panel, first, count, fast, pv, alt, null, effects)

    # ---- the context scans
    def _contexts(self, entry, order, gene, panel, first, count, fast, out):
        assert len(out) == len(order) + 1
        cols = self._scan((entry, int(fast)), [_gene_id(gene)], panel, first, count)
        if cols is None:
            return -1
        np.ctypeslib.as_array(ctypes.cast(out[-1], ctypes.POINTER(ctypes.c_double)), shape=(6,))[:] = NULL
        for (name, each), pointer in zip(order, out):
            _write(pointer, name, [0], cols, (K0,) if each else ())
        self._report(count)
        return 0

    def crm_scan_interaction_contexts(self, gene, panel, first, count, fast, *out):
        return self._contexts("contexts", CONTEXTS, gene, panel, first, count, fast, out)

    def crm_scan_interaction_contexts_joint(self, gene, panel, first, count, fast, *out):
        return self._contexts("joint", JOINT, gene, panel, first, count, fast, out)


class _Panel:
    """Stands in for ``GenotypePanel``: every entry of a test matrix holds its true column number, which is what the
    panel remembers of the columns it was built from, beside the ``groups`` it was built with."""
    made = []

    def __init__(self, G, device=0, groups="auto"):
        G = np.asarray(G, float)
        if not np.all(np.isfinite(G)):
            raise ValueError("There are non-finite values in the covariates matrix.")
        self.shape, self.groups, self.n_groups = G.shape, groups, None
        self.cols = G[0].astype(np.int64)
        self.handle = self
        _Panel.made.append(self)


class _Background:
    handle = ctypes.c_void_p(7)

    def __init__(self, rank=2):
        self._rank = rank

    def rank(self, i):
        return self._rank


class _Bar:
    made = []

    def __init__(self, total=None):
        self.total, self.n, self.closed = total, 0, False
        _Bar.made.append(self)

    def update(self, by):
        self.n += by

    def close(self):
        self.closed = True


@pytest.fixture
def stub(monkeypatch):
    lib = _StubLib()
    _Panel.made, _Bar.made = [], []
    monkeypatch.setenv("CELLREGMAP_AMD_STREAM_CHUNK", str(CHUNK))
    monkeypatch.setattr(_engine._lib, "load", lambda: lib)
    monkeypatch.setattr(_engine, "GenotypePanel", _Panel)
    monkeypatch.setattr(_engine, "_context", lambda device=0: "context")
    monkeypatch.setitem(sys.modules, "tqdm", types.SimpleNamespace(tqdm=_Bar))
    return lib


def _matrix(p, rows=N):
    return np.tile(np.arange(p, dtype=float), (rows, 1))


def _crm(y=None, rank=2, background=None):
    rng = np.random.default_rng(5)
    E = rng.standard_normal((N, K0))
    return _engine.CellRegMap(np.arange(N, dtype=float) if y is None else y, E,
                              background=_Background(rank) if background is None else background)


def _uploads_alive():
    return [t for t in threading.enumerate() if t.name == "cellregmap-amd-upload" and t.is_alive()]


# ---- the drivers: how each is called, and its per-variant outputs as {name: (array, trailing shape)} ---------------------
def _interaction(crm, G, progress=False, **kw):
    res = crm.scan_interaction(G, progress=progress, **kw)
    out = {"pv": (res[0], ())}
    out.update({k: (v, ()) for k, v in res[1].items()})
    if kw.get("return_stats"):
        out.update({k: (res[2][k], trailing) for k, trailing in STATS})
        assert list(res[2]) == [k for k, _ in STATS]
    assert list(res[1]) == list(INFO) + (["log_pvalue", "pvalue_status"] if kw.get("pvalue") == "exact" else [])
    return out, None


def _association(fast, effects):
    def run(crm, G, progress=False):
        res = (crm.scan_association_fast if fast else crm.scan_association)(G, progress=progress, effects=effects)
        assert len(res) == (3 if effects else 2) and list(res[1]) == list(INFO)
        out = {"pv": (res[0], ())}
        null = [res[1][k] for k in INFO]
        if effects:
            assert list(res[2]) == ["alt_lml", "null_lml", "null_delta"] + list(EFFECTS)
            out.update({k: (res[2][k], ()) for k in ("alt_lml",) + EFFECTS})
            null += [res[2]["null_lml"], res[2]["null_delta"]]
        return out, null
    return run


def _contexts(joint):
    def run(crm, G, progress=False):
        scan = crm.scan_interaction_contexts_joint if joint else crm.scan_interaction_contexts
        pv, info = scan(G, return_stats=True, progress=progress)
        order = JOINT if joint else CONTEXTS
        keys = (["dof", "log_pvalue", "beta", "beta_se", "dropped", "status"] if joint else
                ["beta", "beta_se", "log_pvalue", "status"])
        assert list(info) == list(INFO) + keys + ["null_lml", "null_delta", "alt_lml", "gene_null_lml", "gene_null_delta"]
        out = {name: (pv if name == "pv" else info[name], (K0,) if each else ()) for name, each in order}
        return out, [info[k] for k in INFO] + [info["gene_null_lml"], info["gene_null_delta"]]
    return run


DRIVERS = {
    "interaction": (_interaction, "single"),
    "interaction_stats": (lambda crm, G, **kw: _interaction(crm, G, return_stats=True, **kw), "single"),
    "interaction_exact": (lambda crm, G, **kw: _interaction(crm, G, pvalue="exact", **kw), "single_tail"),
    "association": (_association(False, False), ("association", 0)),
    "association_effects": (_association(False, True), ("association_effects", 0)),
    "association_fast": (_association(True, False), ("association", 1)),
    "association_fast_effects": (_association(True, True), ("association_effects", 1)),
    "contexts": (_contexts(False), ("contexts", 1)),
    "contexts_joint": (_contexts(True), ("joint", 1)),
}
FAMILIES = ("interaction_exact", "association_effects", "contexts_joint")       # one of each walk, for the progress tests


def _check_outputs(out, p):
    for name, (got, trailing) in out.items():
        want = _value(name, 0, np.arange(p), trailing)
        if name == "dropped":
            want = want.astype(bool)
        assert got.shape == (p,) + tuple(trailing) and got.dtype == want.dtype, (name, got.shape, got.dtype)
        assert np.array_equal(got, want), name


def _check_null(null):
    if null is not None:
        assert all(np.asarray(v).shape == (1,) and np.asarray(v).dtype == np.float64 for v in null[:4])
        assert [float(np.asarray(v).reshape(-1)[0]) for v in null] == NULL[:len(null)]
        assert all(np.ndim(v) == 0 for v in null[4:])


@pytest.mark.parametrize("driver", sorted(DRIVERS))
@pytest.mark.parametrize("p, chunks", [(7, None), (8, [(0, 4), (4, 8)]), (11, [(0, 4), (4, 8), (8, 11)])])
def test_a_host_matrix_is_scanned_resident_or_in_chunks(stub, driver, p, chunks):
    run, entry = DRIVERS[driver]
    out, null = run(_crm(), _matrix(p))
    bounds = chunks or [(0, p)]                    # below twice the chunk: one panel, one call; from there on: streamed
    assert [list(panel.cols) for panel in _Panel.made] == [list(range(a, b)) for a, b in bounds]
    assert all(panel.groups == "auto" for panel in _Panel.made)
    assert [(c[0], c[1], c[3], c[4]) for c in stub.calls] == [(entry, [0], 0, b - a) for a, b in bounds]
    assert [c[2] for c in stub.calls] == _Panel.made                # every chunk's call on that chunk's panel, in order
    assert stub.created == [("single", 1)] and not stub.callbacks and not _Bar.made and not _uploads_alive()
    _check_outputs(out, p)
    _check_null(null)


@pytest.mark.parametrize("driver", sorted(DRIVERS))
def test_a_genotype_panel_is_never_streamed(stub, driver):
    run, entry = DRIVERS[driver]
    panel = _Panel(_matrix(11))
    out, null = run(_crm(), panel)
    assert _Panel.made == [panel] and [(c[0], c[2], c[3], c[4]) for c in stub.calls] == [(entry, panel, 0, 11)]
    _check_outputs(out, 11)
    _check_null(null)


@pytest.mark.parametrize("driver", ["interaction", "interaction_stats", "interaction_exact"])
def test_no_variants_interaction_scan_calls_nothing(stub, driver):
    out, _ = DRIVERS[driver][0](_crm(), np.empty((N, 0)))
    assert not stub.calls and not stub.created and not stub.callbacks and not _Panel.made
    _check_outputs(out, 0)                                          # the keys, (0, ...) shapes and dtypes of any other scan
    assert ("pvalue_status" in out) == (driver == "interaction_exact") and ("F" in out) == (driver == "interaction_stats")


@pytest.mark.parametrize("driver", [d for d in sorted(DRIVERS) if not d.startswith("interaction")])
def test_no_variants_association_and_context_scans_report_the_null(stub, driver):
    run, entry = DRIVERS[driver]
    out, null = run(_crm(), np.empty((N, 0)))
    assert [(c[0], c[3], c[4]) for c in stub.calls] == [(entry, 0, 0)]       # one call, count = 0 ...
    assert len(_Panel.made) == 1 and _Panel.made[0].shape == (N, 1)              # ... on a one-column panel
    _check_outputs(out, 0)
    _check_null(null)


@pytest.mark.parametrize("driver", sorted(DRIVERS))
@pytest.mark.parametrize("p", [0, 3])
def test_a_matrix_with_the_wrong_row_count_is_refused(stub, driver, p):
    with pytest.raises(ValueError):
        DRIVERS[driver][0](_crm(), _matrix(p, rows=N - 1))
    assert not stub.calls


@pytest.mark.parametrize("p", [7, 11])
def test_groups_reach_every_panel_of_the_interaction_scan(stub, p):
    _crm().scan_interaction(_matrix(p), progress=False, groups=None)
    assert len(_Panel.made) == (1 if p == 7 else 3) and all(panel.groups is None for panel in _Panel.made)


@pytest.mark.parametrize("driver", FAMILIES)
@pytest.mark.parametrize("p", [7, 11])
def test_progress_true_is_one_bar(stub, driver, p):
    DRIVERS[driver][0](_crm(), _matrix(p), progress=True)
    assert len(_Bar.made) == 1 and _Bar.made[0].total == p and _Bar.made[0].n == p and _Bar.made[0].closed
    assert stub.callbacks and stub.callbacks[-1] is None               # (the callback is taken off the context again)


@pytest.mark.parametrize("driver", FAMILIES)
@pytest.mark.parametrize("p", [7, 11])
def test_a_callable_progress_counts_the_whole_panel(stub, driver, p):
    seen = []
    DRIVERS[driver][0](_crm(), _matrix(p), progress=lambda done, total: seen.append((done, total)))
    assert not _Bar.made and seen[-1] == (p, p) and all(total == p for _, total in seen)
    assert [d for d, _ in seen] == sorted(d for d, _ in seen) and len(seen) >= (p + 1) // 2


@pytest.mark.parametrize("driver", FAMILIES)
def test_a_failing_call_closes_the_bar_and_stops_the_upload(stub, driver):
    stub.fail_on_scan = 2
    with pytest.raises(_lib.CrmError):
        DRIVERS[driver][0](_crm(), _matrix(11), progress=True)
    assert len(stub.calls) == 2 and len(_Bar.made) == 1 and _Bar.made[0].closed and _Bar.made[0].n == CHUNK
    assert stub.callbacks[-1] is None and not _uploads_alive()


@pytest.mark.parametrize("driver", FAMILIES)
def test_a_non_finite_entry_in_a_later_chunk_reaches_the_caller(stub, driver):
    G = _matrix(11)
    G[2, 9] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        DRIVERS[driver][0](_crm(), G, progress=True)
    assert len(stub.calls) == 2 and _Bar.made[0].closed and not _uploads_alive()


# ---- scan_interaction_many ----------------------------------------------------------------------------------------------
class _ManyPanel:
    shape, cols = (30, 12), np.arange(12)

    def __init__(self, n_groups=None):
        self.n_groups, self.handle = n_groups, self


class _Crm:
    """A bound phenotype of a cohort of three (as in test_assoc_effects_abi_cpu.py)."""
    _W, _E0, _device = np.ones((30, 1)), np.ones((30, 2)), 0

    def __init__(self, i, bg, panel):
        self._gene, self._bg, self._the_panel = ctypes.c_void_p(100 + i), bg, panel

    def _panel(self, G):
        return self._the_panel

    def _bind_gene(self, like=None):
        return self._gene


def _cohort(n_groups=None):
    bg, panel = object(), _ManyPanel(n_groups)
    return [_Crm(i, bg, panel) for i in range(3)], panel


def _many_keys(exact):
    return ("pv",) + INFO + (("log_pvalue", "pvalue_status") if exact else ())


def _check_windows(pv, info, columns, exact):
    assert list(info) == list(_many_keys(exact)[1:])
    for name in _many_keys(exact):
        got = pv if name == "pv" else info[name]
        assert isinstance(got, list) and len(got) == len(columns)
        for i, cols in enumerate(columns):
            want = _value(name, i, cols)
            assert got[i].shape == (len(cols),) and got[i].dtype == want.dtype, (name, i, got[i].dtype)
            assert np.array_equal(got[i], want), (name, i)


@pytest.mark.parametrize("exact", [False, True])
def test_many_whole_panel_is_one_call(stub, exact):
    crms, panel = _cohort()
    pv, info = _engine.scan_interaction_many(crms, None, pvalue="exact" if exact else "reference")
    assert stub.calls == [("multi_tail" if exact else "multi", [0, 1, 2], panel, 0, 12)] and not stub.callbacks
    assert list(info) == list(_many_keys(exact)[1:])
    for name in _many_keys(exact):
        got, want = pv if name == "pv" else info[name], np.stack([_value(name, i, np.arange(12)) for i in range(3)])
        assert got.shape == (3, 12) and got.dtype == want.dtype and np.array_equal(got, want), name


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("n_groups", [None, 5])
def test_many_cis_windows_go_by_runs(stub, exact, n_groups):
    """Index arrays with a repeat, a slice and an empty window: on a general panel, and -- the first window is not a
    stretch of neighbours -- on a donor-level panel too."""
    crms, panel = _cohort(n_groups)
    cis = [np.array([7, 2, 2, 9]), slice(1, 8), np.array([], int)]
    columns = [np.array([7, 2, 2, 9]), np.arange(1, 8), np.array([], int)]
    seen = []
    pv, info = _engine.scan_interaction_many(crms, None, cis_index=cis, pvalue="exact" if exact else "reference",
                                             progress=lambda done, total: seen.append((done, total)))
    assert all(c[0] == ("multi_tail" if exact else "multi") and c[2] is panel for c in stub.calls)
    tested = sorted((first, count, tuple(genes)) for _, genes, _, first, count in stub.calls)
    assert tested == [(1, 1, (1,)), (2, 1, (0, 1)), (3, 4, (1,)), (7, 1, (0, 1)), (9, 1, (0,))], tested
    _check_windows(pv, info, columns, exact)
    assert pv[0][1] == pv[0][2]                                                    # the repeated column
    assert seen[-1] == (8, 8) and [d for d, _ in seen] == sorted(d for d, _ in seen) and all(t == 8 for _, t in seen)
    if exact:
        assert all(np.all(s >= 0) for s in info["pvalue_status"])                  # the fill of untested positions is never seen


@pytest.mark.parametrize("exact", [False, True])
def test_many_contiguous_windows_on_a_donor_level_panel_go_phenotype_by_phenotype(stub, exact):
    crms, panel = _cohort(n_groups=5)
    seen = []
    pv, info = _engine.scan_interaction_many(crms, None, cis_index=[(2, 6), slice(0, 3), (4, 4)],
                                             pvalue="exact" if exact else "reference",
                                             progress=lambda done, total: seen.append((done, total)))
    entry = "single_tail" if exact else "single"
    assert stub.calls == [(entry, [0], panel, 2, 4), (entry, [1], panel, 0, 3)]   # first = cols[0]; nothing for the empty window
    _check_windows(pv, info, [np.arange(2, 6), np.arange(0, 3), np.arange(0)], exact)
    assert seen == [(4, 7), (7, 7), (7, 7)] and not stub.callbacks                 # (seen, tested) after every window


def test_many_progress_true_is_one_bar(stub):
    for n_groups, cis in ((None, None), (None, [(0, 5), (3, 9), (4, 4)]), (5, [(0, 5), (3, 9), (4, 4)])):
        _Bar.made.clear()
        _engine.scan_interaction_many(_cohort(n_groups)[0], None, cis_index=cis, progress=True)
        total = 12 if cis is None else (11 if n_groups else 9)     # donor-level windows count every test, runs every variant
        assert len(_Bar.made) == 1 and _Bar.made[0].total == total and _Bar.made[0].n == total and _Bar.made[0].closed


# ---- the cohort binding ------------------------------------------------------------------------------------------------
def _saturated_message(n, rank, ncov):
    return (f"saturated model: the background covariance has rank {rank} and with the {ncov} covariate "
            f"column(s) and the variant it spans all {n} cells; the reference's likelihood then divides "
            "rounding noise by delta and its results (and these) are not reproducible to the usual "
            "tolerances (scan_interaction_info flags such variants)")


def test_the_saturated_model_warning_points_at_the_call(stub):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _crm(rank=N - 2).scan_interaction(_matrix(3), progress=False)                  # bound by _bind_gene
    assert [(str(w.message), w.category, w.filename) for w in caught] == [(_saturated_message(N, N - 2, 1), RuntimeWarning, __file__)]
    assert stub.created == [("single", 1)]

    bg = _Background(rank=N - 2)
    crms = [_crm(y=np.arange(N, dtype=float) + i, background=bg) for i in range(3)]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        pv, info = _engine.scan_interaction_many(crms, _matrix(5))                     # the first by itself, the others in a batch
    assert stub.created == [("single", 1), ("single", 1), ("batch", 2)]
    assert [(str(w.message), w.category, w.filename) for w in caught] == [(_saturated_message(N, N - 2, 1), RuntimeWarning, __file__)] * 2
    assert stub.calls[-1][:2] == ("multi", [0, 1, 2]) and pv.shape == (3, 5)

    crms[2]._y = crms[2]._y.copy()
    crms[2]._y[1] = np.inf
    crms[1]._gene = crms[2]._gene = None
    with pytest.raises(ValueError, match="non-finite values in the outcome"):
        _engine.scan_interaction_many(crms, _matrix(5))
