"""The host body of the two context scans (``scan_contexts``, cellregmap_amd/csrc/context_host.hip) past one block of
variants: ``CellRegMap.scan_interaction_contexts`` ("each") and ``scan_interaction_contexts_joint`` ("joint") on the cohorts
of tests/context_block_cases.py -- 130 .. 300 variants -- with ``crm_set_block_variants(ctx, 128)`` and room for the rotated
candidates of 50 variants (``crm_test_set_context_budget``), so that a scan of 300 variants runs blocks of 128, 128 and 44
in sub-ranges of 50, 50, 28 and 44.  tests/test_gpu_context_lrt.py and tests/test_gpu_context_joint.py hold the kernels at
every shape on three to five variants, which is one block and, but for their ragged sub-range tests, one sub-range.

  1. the held variants of every cohort (both sides of every block and sub-range boundary) against the extended-precision
     reference, by ``_hold`` of tests/context_lrt_hold.py and tests/context_joint_hold.py: the limits are
     ``pinned_reference.limits`` (32 x the float64 oracle's own error at the same points, floor n x 2.2e-16, ceiling 1e-11,
     asserted never to bind), the tails against mpmath; tests/test_context_blocks_cpu.py holds the cohorts' conditions;
  2. the cut scan is the one-block scan bit for bit;
  3. a window (first, count) of a resident panel is the scan of the sliced matrix bit for bit, dense and donor-level;
  4. int8 dosages (``GenotypePanel.from_dosages(.., standardize=False)``) are the dense matrix bit for bit;
  5. a variant in the span of W in the second and in the third block, a constant context column on every row;
  6. the progress callback ends every block;
  7. the work buffers carved for one shape serve the next and the first again.
The per-case errors go beside the file $CRM_PINNED_JSON names, as <name>_contexts_blocks.json.
"""
import contextlib
import json
import os

import numpy as np
import pytest

import context_block_cases as bc
import context_joint_hold as jh
import context_lrt_hold as lh

pytestmark = pytest.mark.gpu

RECORD = {}
OK, COLLINEAR, ONE_LESS = lh.OK, lh.COLLINEAR, lh.ONE_LESS
CALLS = ["each", "joint"]
K3 = "k 3, c 9, mode B"
K17 = "k 17, c 70, mode B"
K48 = "k 48, c 128, mode B"


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    yield
    dest = os.environ.get("CRM_PINNED_JSON")
    if dest and RECORD:
        with open(os.path.splitext(dest)[0] + "_contexts_blocks.json", "w") as fh:
            json.dump(RECORD, fh, indent=1, sort_keys=True)


def _kit(call):
    return jh if call == "joint" else lh


def _cohorts(call):
    return [name for name in bc.CASES if call == "joint" or bc.CASES[name][2] == "both"]


def _scan(obj, call, G, fast, **kw):
    method = obj.scan_interaction_contexts_joint if call == "joint" else obj.scan_interaction_contexts
    return method(G, fast=fast, return_stats=True, **kw)


@contextlib.contextmanager
def _cut(obj, cs, block=bc.BLOCK, sub=bc.SUB):
    """Blocks of ``block`` variants and room for the rotated candidates of ``sub`` of them (0: the defaults)."""
    from cellregmap_amd import _engine, _lib

    lib, ctx = _lib.load(), _engine._context(0)
    ldq = -(-max(obj._bg.rank(i) for i in range(len(cs.grid))) // 128) * 128    # the spectra's common leading dimension
    _lib.check(lib.crm_set_block_variants(ctx, block))
    _lib.check(lib.crm_test_set_context_budget(ctx, sub * 8 * cs.k * ldq + 8 if sub else 0))
    try:
        yield
    finally:
        _lib.check(lib.crm_test_set_context_budget(ctx, 0))
        _lib.check(lib.crm_set_block_variants(ctx, 0))


def _panel(cs):
    """What the scans of a cohort are given: the host matrix kept dense; the dosage cohort's int8 panel."""
    from cellregmap_amd import GenotypePanel

    if cs.name == bc.DOSAGES:
        return GenotypePanel.from_dosages(cs.D, cs.donor_of_cell, standardize=False)
    return GenotypePanel(cs.G, groups=None)


_scans = {}


def _scanned(call, name, fast, cut):
    """(pv, info) of a cohort: in blocks of 128 and sub-ranges of 50 (``cut``) or as one block.  One scan per process."""
    key = (call, name, fast, cut)
    if key not in _scans:
        cs = bc.case(name)
        obj = _kit(call)._device(cs)
        with _cut(obj, cs) if cut else _cut(obj, cs, block=0, sub=0):
            _scans[key] = _scan(obj, call, _panel(cs), fast)
    return _scans[key]


class _EachAt(lh._At):
    """``context_lrt_hold._At`` that computes every record once: they depend on the cohort, the variant and delta alone."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self._memo = {}

    def at(self, g, delta):
        key = ("at", g.tobytes(), delta)
        if key not in self._memo:
            self._memo[key] = super().at(g, delta)
        return self._memo[key]

    def refit(self, g):
        key = ("refit", g.tobytes())
        if key not in self._memo:
            self._memo[key] = super().refit(g)
        return self._memo[key]


class _JointAt(jh._At):
    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self._memo = {}

    def at(self, g, delta, keep=None):
        key = (g.tobytes(), delta, None if keep is None else tuple(keep))
        if key not in self._memo:
            self._memo[key] = super().at(g, delta, keep=keep)
        return self._memo[key]


_ats = {}


def _at(call, cs, rho, tag="", **kw):
    key = (call, cs.name, float(rho), tag)
    if key not in _ats:
        _ats[key] = (_JointAt if call == "joint" else _EachAt)(cs, cs.y, rho, **kw)
    return _ats[key]


def _hold(call, case, cs, G, result, fast, sel):
    pv, info = result
    at = _at(call, cs, info["rho1"][0])
    return _kit(call)._hold(case, cs, cs.y, G, pv, info, fast, sel=sel, at=at, record=RECORD)


def _label(call, fast, name):
    return "blocks %s %s, %s" % (call, "fast" if fast else "refit", name)


# ---- 1: the reference across blocks and sub-ranges ---------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("call,name", [(call, name) for call in CALLS for name in _cohorts(call)])
def test_the_held_variants_against_the_reference(call, name, fast):
    cs = bc.case(name)
    pv, info = _scanned(call, name, fast, True)
    _hold(call, _label(call, fast, name), cs, cs.G, (pv, info), fast, bc.held(name))
    if fast:
        assert np.all(info["null_delta"] == info["gene_null_delta"]), name      # every variant, not the held ones alone
    assert np.all(info["status"] == OK), name


# ---- 2: blocks do not change the answer ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("call,name", [(call, name) for call in CALLS for name in _cohorts(call)])
def test_the_cut_scan_equals_the_one_block_scan(call, name, fast):
    _kit(call)._same(_scanned(call, name, fast, False), _scanned(call, name, fast, True))


# ---- 3: a window equals the slice ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("first,count", [(128, 128), (256, 44), (37, 230)])
@pytest.mark.parametrize("call", CALLS)
def test_a_window_equals_the_sliced_panel(call, first, count, fast):
    from cellregmap_amd import GenotypePanel

    cs = bc.case(K3)
    p = cs.G.shape[1]
    Gd = np.random.default_rng(11).normal(size=(cs.donors, p))
    G = Gd[cs.donor_of_cell]
    kit = _kit(call)
    runs = {}
    with _cut(kit._device(cs), cs):
        for kind, whole, part in (("dense", GenotypePanel(G, groups=None), GenotypePanel(G[:, first:first + count], groups=None)),
                                  ("donors", GenotypePanel.from_donors(Gd, cs.donor_of_cell),
                                   GenotypePanel.from_donors(Gd[:, first:first + count], cs.donor_of_cell))):
            for what, panel, j0 in (("window", whole, first), ("slice", part, 0)):
                rc, out = kit._abi_scan(cs, panel, j0, count, fast)
                assert rc == 0, (kind, what, rc)
                runs[kind, what] = out
    want = runs["dense", "slice"]
    status = want[7 if call == "joint" else 5]
    assert np.all(status == OK) and np.all(np.isfinite(want[0])), status
    for key, out in runs.items():
        for i, (got, ref) in enumerate(zip(out, want)):
            assert got.shape == ref.shape and np.array_equal(got, ref, equal_nan=got.dtype != np.int32), (key, i)


# ---- 4: int8 dosages -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("call", CALLS)
def test_int8_dosages_equal_the_dense_matrix(call, fast):
    """The panel of test 1's dosage cohort (held there to the reference at 0, 127, 128 and 139) against the expanded
    float64 matrix kept dense, blocks of 128."""
    from cellregmap_amd import GenotypePanel

    cs = bc.case(bc.DOSAGES)
    assert cs.D.dtype == np.int8 and set(np.unique(cs.D)) == {0, 1, 2} and np.all(cs.D.min(axis=0) < cs.D.max(axis=0))
    kit = _kit(call)
    obj = kit._device(cs)
    with _cut(obj, cs):
        dense = _scan(obj, call, GenotypePanel(cs.D[cs.donor_of_cell].astype(float), groups=None), fast)
    kit._same(dense, _scanned(call, bc.DOSAGES, fast, True))
    assert np.all(dense[1]["status"] == OK)


# ---- 5: special statuses away from the start -------------------------------------------------------------------------------
SPAN = [130, 299]


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("call", CALLS)
def test_variants_in_the_span_of_w_in_later_blocks(call, fast):
    """Columns 130 (second block, first sub-range) and 299 (third block, the last variant) are W times coefficients."""
    from cellregmap_amd import GenotypePanel

    cs = bc.case(K3)
    G = cs.G.copy()
    G[:, 130] = cs.W @ np.linspace(-1.0, 2.0, cs.W.shape[1])
    G[:, 299] = cs.W @ np.linspace(1.5, -0.5, cs.W.shape[1])
    kit = _kit(call)
    obj = kit._device(cs)
    with _cut(obj, cs):
        pv, info = _scan(obj, call, GenotypePanel(G, groups=None), fast)
    status = info["status"]
    if call == "joint":
        assert np.array_equal(np.flatnonzero(status != OK), SPAN) and np.all(status[SPAN] == COLLINEAR), status
        assert np.all(info["dof"][SPAN] == 0) and np.all(info["dropped"][SPAN])
        assert np.array_equal(info["alt_lml"][SPAN], info["null_lml"][SPAN])
        assert np.all(pv[SPAN] == ONE_LESS) and np.all(info["log_pvalue"][SPAN] == 0.0)
    else:
        assert np.array_equal(np.flatnonzero((status != OK).any(axis=1)), SPAN) and np.all(status[SPAN] == COLLINEAR), status
        assert np.all(pv[SPAN] == ONE_LESS) and np.all(info["log_pvalue"][SPAN] == 0.0)
        assert np.array_equal(info["alt_lml"][SPAN], np.repeat(info["null_lml"][SPAN, None], cs.k, axis=1))
    assert np.all(np.isnan(info["beta"][SPAN])) and np.all(np.isnan(info["beta_se"][SPAN]))
    rest = np.setdiff1d(np.arange(G.shape[1]), SPAN)
    assert np.all(np.isfinite(info["beta"][rest])) and np.all(np.isfinite(pv[rest]))
    _hold(call, _label(call, fast, "variants in the span of W"), cs, G, (pv, info), fast, [129, 131, 177, 178, 298])


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("call", CALLS)
def test_a_constant_context_column_on_every_row(call, fast):
    """Contexts [C_0, 1, C_2] beside a W that holds the intercept: the candidate g o 1 = g leaves on all 300 rows, and the
    held variants are the reference's with the column removed."""
    cs = bc.case(K3)
    p = cs.G.shape[1]
    C = np.column_stack([cs.C[:, 0], np.ones(cs.n), cs.C[:, 2]])
    kit = _kit(call)
    obj = kit._device(cs, C=C)
    with _cut(obj, cs):
        pv, info = _scan(obj, call, _panel(cs), fast)
    case = _label(call, fast, "constant column")
    if call == "joint":
        assert np.all(info["dof"] == 2) and np.all(info["status"] == OK)
        assert np.array_equal(info["dropped"], np.tile([False, True, False], (p, 1)))
        at = _at(call, cs, info["rho1"][0], "constant column", C=C, XC=C[:, [0, 2]])
        jh._hold(case, cs, cs.y, cs.G, pv, info, fast, sel=bc.held(K3), at=at, keep=[0, 2], record=RECORD)
    else:
        assert np.all(info["status"][:, 1] == COLLINEAR) and np.all(info["status"][:, [0, 2]] == OK)
        assert np.all(pv[:, 1] == ONE_LESS) and np.all(np.isnan(info["beta"][:, 1])) and np.all(np.isnan(info["beta_se"][:, 1]))
        assert np.array_equal(info["alt_lml"][:, 1], info["null_lml"]) and np.all(info["log_pvalue"][:, 1] == 0.0)
        at = _at(call, cs, info["rho1"][0], "constant column", C=C[:, [0, 2]])
        sub = dict(info)
        for key in ("alt_lml", "beta", "beta_se", "log_pvalue", "status"):
            sub[key] = info[key][:, [0, 2]]
        lh._hold(case, cs, cs.y, cs.G, pv[:, [0, 2]], sub, fast, sel=bc.held(K3), at=at, record=RECORD)


# ---- 6: progress -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("call", CALLS)
def test_the_progress_callback_ends_every_block(call, fast):
    cs = bc.case(K3)
    kit = _kit(call)
    obj = kit._device(cs)
    seen = []
    with _cut(obj, cs):
        told = _scan(obj, call, _panel(cs), fast, progress=lambda done, total: seen.append((done, total)))
    assert seen == [(128, 300), (256, 300), (300, 300)], seen
    kit._same(_scanned(call, K3, fast, True), told)


# ---- 7: reused work buffers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change", [False, True])
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("call", CALLS)
def test_the_work_buffers_serve_another_shape_and_the_first_again(call, fast, change):
    """k = 17, c = 70, then k = 3, c = 9 (and k = 48, c = 128 for the joint call), then k = 17 again on the one context:
    every shape carves the context's work buffers its own way.  ``change``: the first scan as one block, the last cut."""
    kit = _kit(call)
    names = [K17, K3] + ([K48] if call == "joint" else [])
    objs = {name: kit._device(bc.case(name)) for name in names}     # (held: the background cache keeps two)

    def run(name, cut):
        cs, obj = bc.case(name), objs[name]
        with _cut(obj, cs) if cut else _cut(obj, cs, block=0, sub=0):
            return _scan(obj, call, _panel(cs), fast)

    first = run(K17, not change)
    between = [run(name, True) for name in names[1:]]
    again = run(K17, True)
    kit._same(first, again)
    for name, got in zip(names[1:], between):       # and the scans between are their cohorts' own
        kit._same(_scanned(call, name, fast, True), got)
