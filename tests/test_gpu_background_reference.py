"""The background constructor (cellregmap_amd/csrc/background.hip: begin / complete / seal) held to the half factor it was
given: Q0, S0, the ranks and the mixing matrices of every grid point against tests/background_reference.py -- longdouble
products straight from (E1, B), LAPACK's spectrum by the reference's own route, the documented rank rule on inputs whose
rank is decided by a factor 10 -- at the shapes where the constructor branches: n against cols, the block of rho = 1,
the two-stage family solver and its padding, both rank rules, the slab arithmetic of the polish, the decision of
``seal``, the Hadamard ingest, kb = 0 and a rank-0 grid point, ownership patterns with an empty batch, and the upload of
given spectra.  tests/test_background_reference_cpu.py shows that LAPACK's own decompositions of the same inputs pass
the same checker.

Every case is built through ``BackgroundBuilder``; the mixing matrices are exported into host memory between ``complete`` and
``seal`` (after ``seal`` the builder's entry points are gone).  What ``seal`` decided is read from the device memory the
sealed background holds: with the mixing matrices kept it is H, H' and Mix, S0 of every grid point; without them Q0, S0 of
every grid point (``crm_test_live_device_bytes``).  Which solver ran, the slab the polish looked at and its own defect
figures come from the constructor's trace (``CRM_TRACE_SETUP``).

The mixing matrices are held to the caps where ``seal`` keeps them (``background_reference.seal_keeps_mix``, from the
reference spectra with a factor 2 to spare).  Where it drops them the sealed background is (Q0, S0) alone, and Q0 is what is
checked.

These cases found the polish of the thin branch working against the rounded Gram matrix: with B = P diag(s) R', R orthogonal,
|Q0'Q0 - I| was 1.8e-7 for a kept eigenvalue of 1e-10 S_max, 1.2e-8 over nine decades, 1.2e-11 and 3.1e-11 at
S_max / S_min = 5e5 and 2e6, while the constructor's own figure said 2e-14 (the correction is now
taken in the cell axis).

With ``CRM_BACKGROUND_JSON`` set the measured maxima per case are written there when the module is done
(profiles/background_reference_errors.json is such a record)."""
import ctypes
import gc
import json
import os
import re

import numpy as np
import pytest

import background_reference as br

pytestmark = pytest.mark.gpu

GRID = br.RHO_GRID
RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    yield
    dest = os.environ.get("CRM_BACKGROUND_JSON")
    if dest and RECORD:
        with open(dest, "w") as fh:
            json.dump({"caps": {"ortho": br.ORTHO_CAP, "mix_defect": br.MIX_CAP, "spectrum_and_reconstruction": "%g * dim" % br.SPECTRUM_TOL,
                                "h_mix_share": 1.0},
                       "cases": RECORD}, fh, indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def _no_cached_backgrounds():
    from cellregmap_amd import _engine

    _engine._bg_cache.clear()
    yield
    _engine._bg_cache.clear()


class HostSlot:
    """A host buffer in the place of the device tensor ``export_slot`` / ``import_slot`` expect."""

    def __init__(self, doubles):
        self.a = np.full(int(doubles), np.nan)

    def data_ptr(self):
        return self.a.ctypes.data


def _layout(builder):
    from cellregmap_amd import _lib

    n_pad, ldq, ldh, mix = ctypes.c_long(), ctypes.c_long(), ctypes.c_long(), ctypes.c_int()
    _lib.check(_lib.load().crm_background_layout(builder._bg.handle, ctypes.byref(n_pad), ctypes.byref(ldq), ctypes.byref(ldh),
                                                 ctypes.byref(mix)))
    return n_pad.value, ldq.value, ldh.value, bool(mix.value)


def _export_mixes(builder, points):
    n_pad, ldq, ldh, mix = _layout(builder)
    assert mix and builder.layout() == {"S0": ldq, "Mix": ldh * ldq}
    out = {}
    for i in points:
        slot = HostSlot(ldh * ldq)
        builder.export_slot(i, "Mix", slot)
        out[i] = slot.a.reshape(ldh, ldq)
    return out


TRACE_SLAB = re.compile(r"rho\[(\d+)\] defect over the last (\d+) columns: (\S+)")
TRACE_PASS = re.compile(r"rho\[(\d+)\] pass (\d+): \|Mix' C Mix - I\| = (\S+)")


def _trace(text):
    slab = {int(i): (int(ns), float(v)) for i, ns, v in TRACE_SLAB.findall(text)}
    passes = {}
    for i, p, v in TRACE_PASS.findall(text):
        passes.setdefault(int(i), []).append(float(v))
    return {"slab": slab, "passes": passes, "two_stage": len(re.findall(r"\] eigen-decompositions \(two-stage\)", text)),
            "one_stage": len(re.findall(r"\] eigen-decompositions\s+\d", text))}


def _construct(E1, B, grid, rel_tol=0.0, capfd=None):
    """begin (every grid point) -> complete -> export Mix to the host -> seal.  Returns
    (background, mixes or None, (n_pad, ldq, ldh, has_mix), trace)."""
    from cellregmap_amd._engine import BackgroundBuilder

    if capfd is not None:
        capfd.readouterr()
    b = BackgroundBuilder(E1, B, grid, rel_tol=rel_tol)
    ranks = [b.rank(i) for i in range(len(grid))]
    assert min(ranks) >= 0
    b.complete(ranks)
    lay = _layout(b)
    mixes = _export_mixes(b, range(len(grid))) if lay[3] else None
    if not lay[3]:
        assert set(b.layout()) == {"Q0", "S0"}
    bg = b.seal()
    trace = _trace(capfd.readouterr().err) if capfd is not None else None
    return bg, mixes, lay, trace


def _reader(bg, n):
    def read(i):
        Q0, S0 = bg.read(i, n)
        return Q0, S0, bg.rank(i)
    return read


def _check(name, E1, B, grid, bg, mixes=None, rel_tol=None, s=None, trace=None, extra=None):
    pres = None if s is None else (lambda rho: br.prescribed_spectrum(s[0], s[1], rho))
    if mixes is not None and not br.seal_keeps_mix(E1, B, grid, rel_tol):
        # seal dropped the mixing matrices and set the columns of every Q0 right in the cell axis: the sealed background is
        # (Q0, S0) alone; Mix was a stage on the way and nothing of the product
        mixes = None
    figs = br.check_grid(E1, B, grid, _reader(bg, E1.shape[0]), rel_tol=rel_tol, prescribed=pres,
                         mixes=None if mixes is None else [mixes[i] for i in range(len(grid))])
    w = br.worst(figs)
    if trace is not None:
        w["polish_slab_estimate"] = max([v for _, v in trace["slab"].values()], default=None)
        w["polish_last_defect"] = max([p[-1] for p in trace["passes"].values()], default=None)
        w["polish_passes"] = max([len(p) for p in trace["passes"].values()], default=0)
    if extra:
        w.update(extra)
    RECORD[name] = w
    print(name, w)
    return w


@pytest.fixture
def traced(monkeypatch, capfd):
    monkeypatch.setenv("CRM_TRACE_SETUP", "1")
    return capfd


# ---- thin, well conditioned ------------------------------------------------------------------------------------------
def test_thin_well_conditioned_nothing_a_multiple_of_the_padding(traced):
    E1, B = br.random_family(97, 3, 20, seed=1)
    _warm_up(E1, B, GRID)
    bg, mixes, (n_pad, ldq, ldh, has_mix), tr = _construct(E1, B, GRID, capfd=traced)
    assert (n_pad, ldq, ldh, has_mix) == (128, 128, 128, True)
    assert br.seal_keeps_mix(E1, B, GRID)
    assert _held_by(bg) == _mix_kept_bytes(n_pad, ldh, ldq, 11)        # the mixing matrices survive seal
    assert len(tr["slab"]) == 11 and max(v for _, v in tr["slab"].values()) < 2e-13 and not tr["passes"]    # no polish
    _check("thin_well_97_3_20", E1, B, GRID, bg, mixes, trace=tr)


# ---- n against cols ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 64, 63])
def test_branch_boundary(n):
    E1, B = br.random_family(n, 5, 59, seed=2)
    bg, mixes, (n_pad, ldq, ldh, has_mix), _ = _construct(E1, B, GRID)
    assert has_mix == (n == 65) and (mixes is not None) == (n == 65)
    assert ldh == (128 if n == 65 else 0)
    _check("boundary_n%d_cols64" % n, E1, B, GRID, bg, mixes)


# ---- the thin rank rule --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rel_tol", [None, 1e-6], ids=["default", "1e-6"])
def test_thin_rank_rule(rel_tol, traced):
    """Eigenvalues at 100 x and 1 / 100 x the cut: the ranks are exact at all eleven grid points, and the kept ones at
    100 x the cut are the columns whose orthonormality the polish has to restore."""
    E1, B, s1, s2 = br.rank_rule_family(rel_tol)
    bg, mixes, lay, tr = _construct(E1, B, GRID, rel_tol=rel_tol or 0.0, capfd=traced)
    assert [bg.rank(i) for i in range(11)] == [55] + [61] * 9 + [6]
    _check("rank_rule_%s" % (rel_tol or "default"), E1, B, GRID, bg, mixes, rel_tol=rel_tol, s=(s1, s2), trace=tr)


# ---- slab arithmetic of the polish -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [257, 384, 385])
def test_polish_slab_arithmetic(cols, traced):
    """r > 256: the first look covers the last ns = r - (r - 256) / 128 * 128 columns only (ns == r at 257, ns < r from
    384 on), the full passes follow.  Nine decades: the polish runs, and seal drops the mixing matrices."""
    E1, B, s1, s2 = br.geometric_family(cols)
    _warm_up(E1, B, GRID)
    bg, mixes, (n_pad, ldq, ldh, has_mix), tr = _construct(E1, B, GRID, capfd=traced)
    assert has_mix and not br.seal_keeps_mix(E1, B, GRID)
    assert _held_by(bg) == _mix_dropped_bytes(n_pad, ldq, 11)      # no Mix, every Q0 present
    ns = {257: 257, 384: 256, 385: 257}[cols]
    assert tr["slab"][5][0] == ns and tr["passes"].get(5)          # rho = 0.5: r = cols; the polish ran
    w = _check("polish_cols%d" % cols, E1, B, GRID, bg, mixes, s=(s1, s2), trace=tr)
    assert w["ranks"] == [cols - 5] + [cols] * 9 + [5]


# ---- what seal decides -----------------------------------------------------------------------------------------------
def _live():
    from cellregmap_amd import _engine, _lib

    gc.collect()
    _engine.release_workspaces(0)
    return _lib.load().crm_test_live_device_bytes()


_BASE = {}


def _held_by(bg):
    """Device bytes the process holds beyond what it held before the first background of the test -- call it while
    ``bg`` is the only background alive and before anything reads a lazily formed Q0."""
    return _live() - _BASE["bytes"]


@pytest.fixture(autouse=True)
def _baseline(_no_cached_backgrounds):
    """Live device bytes with no background alive.  The context's own buffers (problem records, split-k partials) grow to a
    shape's needs once and stay: a test that compares byte counts builds its shape once before it measures."""
    _BASE["bytes"] = _live()
    yield


def _warm_up(E1, B, grid):
    """Build, read and drop the same shape once, then take the baseline: the context's buffers have their sizes."""
    bg = _construct(E1, B, grid)[0]
    for i in range(len(grid)):
        bg.read(i, E1.shape[0])
    del bg
    _BASE["bytes"] = _live()


def _mix_kept_bytes(n_pad, ldh, ldq, nrho):
    return 8 * (2 * n_pad * ldh + nrho * (ldh * ldq + ldq))       # H, H'; Mix, S0 per grid point


def _mix_dropped_bytes(n_pad, ldq, nrho):
    return 8 * nrho * (n_pad * ldq + ldq)                          # Q0, S0 per grid point


@pytest.mark.parametrize("cond", [5e5, 2e6])
def test_seal_keeps_the_mixing_matrices_up_to_a_condition_number_of_1e6(cond):
    """S_max / S_min = 5e5 at the worst grid point: kept.  2e6: dropped, every Q0 formed.  A factor 2 on either side."""
    E1, B, s1, s2 = br.conditioned_family(cond)
    _warm_up(E1, B, GRID)
    bg, mixes, (n_pad, ldq, ldh, has_mix), _ = _construct(E1, B, GRID)
    held = _held_by(bg)
    kept, dropped = _mix_kept_bytes(n_pad, ldh, ldq, 11), _mix_dropped_bytes(n_pad, ldq, 11)
    assert kept != dropped and has_mix and br.seal_keeps_mix(E1, B, GRID) == (cond < 1e6)
    assert held == (kept if cond < 1e6 else dropped), (held, kept, dropped)
    _check("seal_cond%g" % cond, E1, B, GRID, bg, mixes, s=(s1, s2), extra={"mix_kept": bool(cond < 1e6)})


# ---- the two-stage family solver and its padding -------------------------------------------------------------------------
@pytest.mark.parametrize("k1,kb,n,served", [(10, 960, 990, True), (10, 959, 989, False), (64, 960, 1050, True), (65, 960, 1050, False)],
                         ids=["order1024", "order1023", "pad0", "k1_65"])
def test_two_stage_family_solver(k1, kb, n, served, traced):
    """sub + 64 - k1 >= 1024 and k1 <= 64 choose the two-stage form; 20 duplicated columns of B put genuine null directions
    beside the 64 - k1 of the padding: both kinds are dropped, the rank is cols - 20 inside the grid."""
    grid = np.array([0.0, 0.5, 1.0])
    E1, B = br.duplicated_family(n, k1, kb, dup=20, seed=31)
    bg, mixes, lay, tr = _construct(E1, B, grid, capfd=traced)
    assert [bg.rank(i) for i in range(3)] == [kb - 20, k1 + kb - 20, k1]
    assert tr["two_stage"] == (1 if served else 0) and tr["one_stage"] == (1 if served else 2)
    _check("two_stage_k1_%d_kb%d_n%d" % (k1, kb, n), E1, B, grid, bg, mixes, trace=tr, extra={"two_stage": served})


# ---- n <= cols -----------------------------------------------------------------------------------------------------------
def test_eigh_branch_random():
    E1, B = br.random_family(60, 10, 100, seed=3)
    bg, mixes, lay, _ = _construct(E1, B, GRID)
    assert mixes is None
    _check("eigh_random_60_10_100", E1, B, GRID, bg)


def test_eigh_branch_rank_rule():
    """lam_max ~ 1, eigenvalues at 1.5e-6 and 1.5e-10 on either side of sqrt(eps) (absolute)."""
    E1, B, s1, s2 = br.eigh_prescribed_family()
    bg, mixes, lay, _ = _construct(E1, B, GRID)
    assert [bg.rank(i) for i in range(11)] == [47] + [56] * 9 + [9]
    _check("eigh_prescribed", E1, B, GRID, bg, s=(s1, s2))


# ---- kb = 0, a grid point of rank 0 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [[1.0], list(GRID)], ids=["rho1", "grid"])
def test_no_second_factor(grid):
    grid = np.asarray(grid, float)
    E1, _ = br.random_family(80, 7, 0, seed=4)
    bg, mixes, lay, _ = _construct(E1, None, grid)
    if len(grid) > 1:
        assert bg.rank(0) == 0
        Q0, S0 = bg.read(0, 80)
        assert Q0.shape == (80, 0) and S0.shape == (0,)
    _check("kb0_%d_points" % len(grid), E1, None, grid, bg, mixes)


# ---- Hadamard ingest ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k2,m", [(4, 9), (10, 15)], ids=["thin", "eigh"])
def test_hadamard_halves_against_the_same_B_written_out(k2, m):
    from cellregmap_amd._engine import HadamardHalves

    n, k1 = 120, 5
    E1, us, hK, B = br.hadamard_family(n, k1, k2, m, seed=6 if k2 == 4 else 7)
    assert br.is_thin(E1, B) == (k2 == 4)
    bg_h, mix_h, _, _ = _construct(E1, HadamardHalves(us, hK), GRID)
    bg_b, mix_b, _, _ = _construct(E1, B, GRID)
    name = "hadamard_%s" % ("thin" if k2 == 4 else "eigh")
    _check(name + "_explicit", E1, B, GRID, bg_b, mix_b)
    _check(name, E1, B, GRID, bg_h, mix_h)
    for i, rho in enumerate(GRID):
        assert bg_h.rank(i) == bg_b.rank(i)
        lam, dim = br.reference_spectrum(E1, B, rho)
        assert np.abs(bg_h.read(i, n)[1] - bg_b.read(i, n)[1]).max() <= br.SPECTRUM_TOL * dim * lam.max()


# ---- ownership patterns with an empty batch -------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["only_rho1", "all_but_rho1", "none"])
def test_ownership_patterns(pattern):
    """Two builders; the first owns only rho = 1 (no full-size batch), all but rho = 1 (no leading-block batch) or nothing
    (every rank and slot comes from the other); slots travel through host buffers.  Both sealed backgrounds pass the checker
    at every grid point and hold the same bits."""
    from cellregmap_amd._engine import BackgroundBuilder

    E1, B, s1, s2 = br.rank_rule_family(None)
    n = E1.shape[0]
    mine = {"only_rho1": np.arange(11) == 10, "all_but_rho1": np.arange(11) != 10, "none": np.zeros(11, bool)}[pattern]
    a = BackgroundBuilder(E1, B, GRID, mine=mine)
    b = BackgroundBuilder(E1, B, GRID, mine=~mine)
    assert [a.rank(i) >= 0 for i in range(11)] == list(mine) and [b.rank(i) >= 0 for i in range(11)] == list(~mine)
    ranks = [a.rank(i) if mine[i] else b.rank(i) for i in range(11)]
    assert ranks == [55] + [61] * 9 + [6]
    a.complete(ranks)
    b.complete(ranks)
    layout = a.layout()
    assert layout == b.layout() and set(layout) == {"S0", "Mix"}
    n_pad, ldq, ldh, _ = _layout(a)
    mixes = {}
    for what, size in layout.items():
        for i in range(11):
            src, dst = (a, b) if mine[i] else (b, a)
            slot = HostSlot(size)
            src.export_slot(i, what, slot)
            dst.import_slot(i, what, slot)
            if what == "Mix":
                mixes[i] = slot.a.reshape(ldh, ldq)
    bga, bgb = a.seal(), b.seal()
    for who, bg in (("a", bga), ("b", bgb)):
        _check("ownership_%s_%s" % (pattern, who), E1, B, GRID, bg, mixes, s=(s1, s2))
    for i in range(11):
        qa, sa = bga.read(i, n)
        qb, sb = bgb.read(i, n)
        assert np.array_equal(qa, qb) and np.array_equal(sa, sb)


# ---- given spectra -----------------------------------------------------------------------------------------------------
def test_given_spectra_come_back_bit_for_bit():
    from cellregmap_amd._engine import background_from_qs

    n, ranks = 70, [0, 1, 129]
    rng = np.random.default_rng(8)
    qs = [((rng.normal(size=(n, r)),), rng.uniform(0.5, 2.0, size=r)) for r in ranks]
    bg = background_from_qs(qs, [0.0, 0.5, 1.0])
    for i, r in enumerate(ranks):
        assert bg.rank(i) == r
        Q0, S0 = bg.read(i, n)
        assert Q0.shape == (n, r) and S0.shape == (r,)
        assert np.array_equal(Q0, qs[i][0][0]) and np.array_equal(S0, qs[i][1])
