"""Q, F, the restricted log-likelihood and the scale of the interaction scan against an extended-precision reference at
the point where the device itself stopped (tests/pinned_reference.py).

Every other parity test either compares two searches -- and then 1e-6 is all it may ask, because where a Brent search
stops within its tolerance is rounding noise -- or two forms of the library, where an error both share passes.  Here the
search is not on the path of the comparison: ``return_stats=True`` reports (rho*, delta) per variant, and at that fixed
point the four quantities are closed-form functions of the inputs, evaluated in longdouble from the dense definitions
(no spectral decomposition, no Q0).  That works for every covariate count, route and kernel form, so this file walks
through them: the three null-fit kernels on both paths, the routes of mode C, the background modes, the Gram forms at the
edges of their tile rows, tests without a rotated test direction, both permutation hooks, several phenotypes in one
pass, and a slice of the fuzz stream.

Per case, at most three variants by fixed index (first, p // 2, last):

  * Q (relative to max(|Q|, tr F)), F (to max|F|), lml and the scale (relative) against the reference;
  * e2 / g2 / eps2 against rho s (1 - delta), (1 - rho) s (1 - delta) and s delta of the reference's s;
  * ``lambda`` against ``eigvalsh`` of the reference's F rounded to double, atol 1e-12 max|lambda|;
  * p against the oracle's Davies on the reference's (Q, F): parity_bounds.DAVIES relative + 1e-13;
  * the counters say which form served.

Tolerance: not a constant.  Per case and quantity, 32 x the float64 ORACLE's own error against the reference at the same
points (``pinned_reference.oracle_at``; the largest over the case's variants), never below n x 2.2e-16 and never above
1e-11 (``pinned_reference.limits``).  Both errors are printed for every case and kept in
profiles/pinned_reference_errors.json.  No variant is left out: a reference that cannot be evaluated raises.

The null-fit kernels have no counter of their own: which one serves is decided by the covariate count alone
(crm_internal.h: up to CRM_MAX_COV = 8 columns the register kernel, up to 62 nullfit_wide.hip, beyond nullfit_xwide.hip), the
queue-drawn form of the register kernel by one covariate column and at least 1024 variants, the per-wave one by its knob.
"""
import contextlib
import ctypes
import json
import os

import numpy as np
import pytest

import parity_bounds
import pinned_reference as pr
from fuzz_cases import build_case, fuzz_cases
from test_gpu_gram_wide import _covariates, _dma_launches, _flat_phenotype, _pair_blocks, _without_pair
from test_gpu_rho0_positions import _counter
from test_gpu_unrelated_donors import _blocks, _ragged

pytestmark = pytest.mark.gpu

RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    """The per-case errors go to the file $CRM_PINNED_JSON names (a copy is kept under profiles/)."""
    yield
    dest = os.environ.get("CRM_PINNED_JSON")
    if dest and RECORD:
        with open(dest, "w") as fh:
            json.dump(RECORD, fh, indent=1, sort_keys=True)


def _lib_ctx():
    from cellregmap_amd import _engine, _lib

    return _lib.load(), _engine._context(0)


@contextlib.contextmanager
def _kinship(kernel_form, route, fold=2, diag=0, pairs=None, rho0=None, tails=None):
    """Backgrounds made and scans run inside the block: contraction route (crm_test_set_kinship_route), folded / unfolded
    structure, unrelated-donor form and its sub-forms."""
    from cellregmap_amd import _engine, _lib

    lib, ctx = _lib_ctx()
    kernel_form("kin_fold", fold)
    kernel_form("kin_diag", diag)
    for name, value in (("donor_pairs", pairs), ("rho0_positions", rho0), ("rotation_tails", tails)):
        if value is not None:
            kernel_form(name, value)
    _engine._bg_cache.clear()
    _lib.check(lib.crm_test_set_kinship_route(ctx, route))
    try:
        yield
    finally:
        _lib.check(lib.crm_test_set_kinship_route(ctx, 1))


def _used():
    """[unrelated-donor blocks, pair blocks, rho = 0 from the positions, rotation tails, direct-to-LDS Grams, tests without
    a test direction, variants repeated on the dense path]"""
    lib, ctx = _lib_ctx()
    return np.array([_blocks(), _pair_blocks(), _counter("crm_test_rho0_position_blocks"),
                     _counter("crm_test_rotation_tail_launches"), _dma_launches(), _without_pair(),
                     lib.crm_test_dense_repeats(ctx)])


UD, PAIRS, RHO0, TAILS, DMA, NONE, REPEATS = range(7)


class Problem:
    """Inputs of one case as the reference reads them: ``background`` holds hK= or Ls= (a list of half factors) or nothing."""

    def __init__(self, y, W, E0, G, E1=None, idx_E=None, idx_G=None, gram=None, **background):
        self.y, self.W, self.E0, self.G = np.asarray(y, float), np.asarray(W, float), np.asarray(E0, float), np.asarray(G, float)
        self.E1 = self.E0 if E1 is None else np.asarray(E1, float)
        self.idx_E, self.idx_G, self.background = idx_E, idx_G, background
        self._qs, self._ref, self.gram = {}, {}, gram        # gram(rho): hS hS' in longdouble by a shorter way

    def at(self, j, rho, delta):
        """(reference, the oracle's own evaluation) of variant j at (rho, delta): computed once per point."""
        from oracle.sugar import economic_qs_linear

        key = (int(j), float(rho), float(delta))
        if key not in self._ref:
            hS = pr.half_factor(float(rho), self.E1, **self.background)
            if float(rho) not in self._qs:
                (Q0,), S0 = economic_qs_linear(hS, return_q1=False)
                self._qs[float(rho)] = (Q0, S0)
            g = self.G[:, j]
            X = np.column_stack([self.W, g])
            gt = g if self.idx_G is None else g[self.idx_G]
            E0 = self.E0 if self.idx_E is None else self.E0[self.idx_E]
            D = gt[:, None] * E0
            ref = pr.pinned(self.y, X, hS, D, delta, gram=None if self.gram is None else self.gram(float(rho)))
            self._ref[key] = (ref, pr.oracle_at(self.y, X, *self._qs[float(rho)], D, delta))
        return self._ref[key]


def _hold(case, prob, results, sel=None):
    """``results``: [(label, (pv, info, stats))] of device scans of the same problem (forms that stop at the same points
    share the reference).  Asserts everything the module's docstring lists and records the errors."""
    from oracle.davies import davies_pvalue

    n, p = prob.y.size, prob.G.shape[1]
    sel = pr.pick(p) if sel is None else list(sel)
    dev, ora, rows = {}, [], []
    for label, (pv, info, st) in results:
        errs = []
        for j in sel:
            rho, delta = info["rho1"][j], st["delta"][j]
            assert 0.0 <= rho <= 1.0 and 0.0 < delta < 1.0, (case, label, j, rho, delta)
            ref, own = prob.at(j, rho, delta)
            ora.append(pr.errors(own, ref))
            errs.append(pr.errors((st["Q"][j], st["F"][j], st["lml"][j], st["scale"][j]), ref))
            rows.append((label, j, pv[j], info, st, ref))
        dev[label] = pr.worst(errs)
    ora = pr.worst(ora)
    lim = pr.limits(ora, n)
    fmt = lambda e: " ".join("%s %.2e" % (k, e[k]) for k in ("Q", "F", "lml", "scale"))  # noqa: E731
    print("\n[pinned] %s: n %d, variants %s\n[pinned]   oracle  %s\n[pinned]   limit   %s" % (case, n, sel, fmt(ora), fmt(lim)))
    for label, e in dev.items():
        print("[pinned]   device  %s   (%s)" % (fmt(e), label))
    RECORD[case] = {"cells": n, "variants": [int(j) for j in sel], "oracle": ora, "limit": lim, "device": dev}
    assert max(lim.values()) <= pr.CEILING
    for label, e in dev.items():
        for k in lim:
            assert e[k] <= lim[k], (case, label, k, e[k], lim[k])
    for label, j, pj, info, st, (Q, F, lml, s) in rows:
        rho, delta = pr.LD(info["rho1"][j]), pr.LD(st["delta"][j])
        tol = float(lim["scale"] * s)
        for key, want in (("e2", rho * s * (1 - delta)), ("g2", (1 - rho) * s * (1 - delta)), ("eps2", s * delta)):
            assert abs(float(pr.LD(info[key][j]) - want)) <= tol, (case, label, j, key, info[key][j], float(want))
        F64 = np.asarray(F, float)
        lam = np.linalg.eigvalsh(F64)
        assert np.all(np.abs(st["lambda"][j] - lam) <= 1e-12 * np.abs(lam).max()), (case, label, j)
        pref = davies_pvalue(float(Q), F64, True)[0]
        assert abs(pj - pref) <= parity_bounds.DAVIES * pref + parity_bounds.P_ATOL, (case, label, j, pj, pref)


# ---- the three null-fit kernels, dense and donor-collapsed ---------------------------------------------------------------------
@pytest.mark.parametrize("path", ["dense", "collapsed"])
@pytest.mark.parametrize("c,form,variants", [
    (1, "queue", 1100),            # register kernel: LDS-sharing workgroups that draw from a queue (from 1024 variants on)
    (1, "per_wave", 12),           # ... one independent wavefront per (variant, grid point)
    (8, "default", 12),            # ... at its last covariate count
    (8, "per_wave", 12),
    (9, "wide", 12),               # nullfit_wide.hip at its first count,
    (14, "wide", 12),
    (62, "wide", 12),              # ... and at its last
    (63, "xwide", 12),             # nullfit_xwide.hip at its first count
    (70, "xwide", 12),
])
def test_null_fit_kernels(c, form, variants, path, kernel_form):
    import cellregmap_amd as crm
    from cellregmap_amd.synth import make_cohort

    co = make_cohort(10, 40 if c > 62 else 30, 4, variants, seed=38 + c)
    n = co.y.size
    W = _covariates(n, c, c)
    G = co.G if path == "collapsed" else co.G + 0.05 * np.random.default_rng(c).normal(size=co.G.shape)
    if form == "per_wave":
        kernel_form("nullfit_per_wave", 1)
    obj = crm.CellRegMap(co.y, co.E, W=W, hK=co.hK)
    panel = crm.GenotypePanel(G, groups="auto" if path == "collapsed" else None)
    assert (panel.n_groups is not None) == (path == "collapsed")
    before = _used()
    res = obj.scan_interaction(panel, return_stats=True)
    used = _used() - before
    assert used[REPEATS] == 0 and used[NONE] == 0          # the path the case names served every variant
    _hold("null fit c=%d %s %s" % (c, form, path), Problem(co.y, W, co.E, G, hK=co.hK), [(form, res)])


# ---- the routes of mode C, ragged donors -----------------------------------------------------------------------------------------
ROUTES = {
    "direct": dict(route=0, pairs=0),
    "unfolded": dict(route=2, fold=0, pairs=0),
    "folded": dict(route=2, pairs=0),
    "folded-pairs": dict(route=2, pairs=2),
    "unrelated": dict(route=2, diag=2, pairs=0, rho0=0, tails=0),
    "unrelated-pairs": dict(route=2, diag=2, pairs=2, rho0=0, tails=0),
    "unrelated-rho0": dict(route=2, diag=2, pairs=0, rho0=2, tails=0),
    "unrelated-pairs-rho0": dict(route=2, diag=2, pairs=2, rho0=2, tails=0),
}


def _assert_route(name, obj, used, donors):
    lib, _ = _lib_ctx()
    forms = ROUTES[name]
    if forms["route"] == 2:
        assert lib.crm_background_kinship_groups(obj._bg.handle) == donors
        assert (lib.crm_background_kinship_folded(obj._bg.handle) > 0) == (forms.get("fold", 2) == 2)
    assert (used[UD] > 0) == (forms.get("diag", 0) == 2), (name, used)
    assert (used[PAIRS] > 0) == (forms["pairs"] == 2 and forms["route"] == 2), (name, used)
    assert (used[RHO0] > 0) == (forms.get("rho0", 0) == 2), (name, used)
    assert used[TAILS] == 0, (name, used)


@pytest.mark.parametrize("name", list(ROUTES))
def test_routes_of_mode_c(name, kernel_form):
    import cellregmap_amd as crm
    from oracle import crm as ocrm

    donors = 7
    co, keep, G = _ragged(donors, 60, 5, 37, 565)
    y, E, W, hK = co.y[keep], co.E[keep], co.W[keep], co.hK[keep]
    with _kinship(kernel_form, **ROUTES[name]):
        obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        before = _used()
        res = obj.scan_interaction(crm.GenotypePanel(G, groups=None), return_stats=True)
        used = _used() - before
        _assert_route(name, obj, used, donors)
    _hold("mode C route " + name, Problem(y, W, E, G, Ls=ocrm.khatri_rao_halves(hK, E)), [(name, res)])


def test_rotation_tails_on_the_unrelated_donor_route(kernel_form):
    """The skinny one-pass kernel takes the last r mod 128 <= 16 columns of a rotation only from 1024 spectrum entries on
    (scan.hip: plan_rotations), so this is the one case past 640 cells: 24 donors of 46 cells against 43 contexts, rank
    24 x 43 = 1032 = 8 tiles + 8 columns at the interior grid points, 1104 cells (43 + 1032 columns: not saturated).  One
    variant is held, and Sigma is formed as (hK hK') o (us us') instead of the product of the 1104 x 1075 factor
    (``pinned_reference.kronecker_gram``: the same doubles), which keeps the case at a few seconds."""
    import cellregmap_amd as crm
    from cellregmap_amd.synth import make_cohort
    from oracle import crm as ocrm
    from oracle.sugar import economic_svd

    donors, k0, variants = 24, 43, 9
    co = make_cohort(donors, 46, k0, variants, seed=91)
    G = co.G + 0.05 * np.random.default_rng(91).normal(size=co.G.shape)
    y, E, W, hK = co.y, co.E, co.W, co.hK
    with _kinship(kernel_form, route=2, diag=2, rho0=0, tails=2):
        obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        assert obj._bg.rank(5) == 1032
        before = _used()
        res = obj.scan_interaction(crm.GenotypePanel(G, groups=None), return_stats=True)
        used = _used() - before
        assert used[UD] > 0 and used[TAILS] > 0 and used[RHO0] == 0, used
    U, S, _ = economic_svd(E)
    us = U * S                                                   # (oracle/crm.py: khatri_rao_halves)
    prob = Problem(y, W, E, G, Ls=ocrm.khatri_rao_halves(hK, E), gram=lambda rho: pr.kronecker_gram(rho, E, hK, us))
    _hold("mode C route unrelated, rotation tails", prob, [("tails", res)], sel=[variants // 2])


def test_three_context_sets_on_the_unrelated_donor_route(kernel_form):
    """E1 != E2 != E0 (k1 = 7, k2 = 5, k0 = 6)."""
    import cellregmap_amd as crm
    from oracle import crm as ocrm

    co, keep, G = _ragged(9, 40, 6, 45, 123)
    rng = np.random.default_rng(4)
    n = int(keep.sum())
    y, E0, W, hK = co.y[keep], co.E[keep], co.W[keep], co.hK[keep]
    E1, E2 = rng.normal(size=(n, 7)), rng.normal(size=(n, 5))
    with _kinship(kernel_form, route=2, diag=2):
        obj = crm.CellRegMap(y, E0, W=W, E1=E1, Ls=crm.get_L_values(hK, E2))
        before = _used()
        res = obj.scan_interaction(crm.GenotypePanel(G, groups=None), return_stats=True)
        assert (_used() - before)[UD] > 0
    _hold("mode C three context sets, unrelated", Problem(y, W, E0, G, E1=E1, Ls=ocrm.khatri_rao_halves(hK, E2)),
          [("unrelated", res)])


@pytest.mark.parametrize("hook", ["idx_E", "idx_G"])
def test_permutation_hooks(hook, kernel_form):
    import cellregmap_amd as crm
    from oracle import crm as ocrm

    co, keep, G = _ragged(8, 40, 5, 33, 61)
    y, E, W, hK = co.y[keep], co.E[keep], co.W[keep], co.hK[keep]
    hooks = {hook: np.random.default_rng(3).permutation(y.size)}
    with _kinship(kernel_form, route=2, diag=2):
        obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        before = _used()
        res = obj.scan_interaction(crm.GenotypePanel(G, groups=None), return_stats=True, **hooks)
        assert (_used() - before)[UD] > 0
    _hold("mode C unrelated, hook " + hook, Problem(y, W, E, G, Ls=ocrm.khatri_rao_halves(hK, E), **hooks), [(hook, res)])


# ---- background modes on both paths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["dense", "collapsed"])
@pytest.mark.parametrize("mode", ["A", "B", "C"])
def test_background_modes(mode, path):
    import cellregmap_amd as crm
    from cellregmap_amd.synth import make_cohort
    from oracle import crm as ocrm

    co = make_cohort(9, 28, 6, 23, seed=70 + "ABC".index(mode))
    W = _covariates(co.y.size, 3, 5)
    G = co.G if path == "collapsed" else co.G + 0.05 * np.random.default_rng(6).normal(size=co.G.shape)
    kw = {"A": {}, "B": {"hK": co.hK}, "C": {"Ls": crm.get_L_values(co.hK, co.E)}}[mode]
    okw = {"A": {}, "B": {"hK": co.hK}, "C": {"Ls": ocrm.khatri_rao_halves(co.hK, co.E)}}[mode]
    obj = crm.CellRegMap(co.y, co.E, W=W, **kw)
    panel = crm.GenotypePanel(G, groups="auto" if path == "collapsed" else None)
    assert (panel.n_groups is not None) == (path == "collapsed")
    before = _used()
    res = obj.scan_interaction(panel, return_stats=True)
    assert (_used() - before)[REPEATS] == 0
    if mode == "A":
        assert np.all(res[1]["rho1"] == 1.0)
    _hold("mode %s %s" % (mode, path), Problem(co.y, W, co.E, G, **okw), [(path, res)])


# ---- Gram forms ----------------------------------------------------------------------------------------------------------------------
# rows = 2 k0 + c + 2 on the unrelated-donor route (the parameter rows of test_gpu_gram_wide.py, and 13 and 64 rows below them)
@pytest.mark.parametrize("rows,donors,cells,k0,c,variants", [
    (13, 7, 60, 5, 1, 37),         # one tile row
    (64, 4, 70, 30, 2, 10),        # four tile rows: the last count of the narrow direct-to-LDS kernel
    (65, 5, 70, 31, 1, 13),        # 5 tile rows
    (80, 4, 80, 38, 2, 9),
    (81, 5, 80, 39, 1, 11),        # 6
    (96, 4, 100, 46, 2, 9),
    (97, 4, 100, 47, 1, 10),       # 7
    (112, 4, 120, 54, 2, 9),
    (113, 4, 120, 54, 3, 9),       # 8
    (128, 4, 150, 62, 2, 7),
    (129, 4, 150, 63, 1, 7),       # 9
    (144, 4, 150, 64, 14, 6),
])
def test_gram_forms(rows, donors, cells, k0, c, variants, kernel_form):
    """Direct-to-LDS and register-staged Gram on the same scan: the null fits do not read the Gram, so both forms stop at
    the same points and share the reference."""
    import cellregmap_amd as crm
    from oracle import crm as ocrm

    assert rows == 2 * k0 + c + 2
    co, keep, G = _ragged(donors, cells, k0, variants, 900 + rows)
    y, E, hK = co.y[keep], co.E[keep], co.hK[keep]
    assert y.size <= 640
    W = _covariates(y.size, c, rows)
    pairs = k0 <= 54
    with _kinship(kernel_form, route=2, diag=2, pairs=2 if pairs else 0):
        obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        panel = crm.GenotypePanel(G, groups=None)
        before = _used()
        dma = obj.scan_interaction(panel, return_stats=True)
        used = _used() - before
        assert used[DMA] > 0 and used[UD] > 0 and (used[PAIRS] > 0) == pairs, used
        kernel_form("gram_staged", 1)
        before = _used()
        staged = obj.scan_interaction(panel, return_stats=True)
        used = _used() - before
        kernel_form("gram_staged", 0, reset=True)
        assert used[DMA] == 0 and used[UD] > 0, used
    assert np.array_equal(dma[2]["delta"], staged[2]["delta"]) and np.array_equal(dma[1]["rho1"], staged[1]["rho1"])
    _hold("gram %d rows" % rows, Problem(y, W, E, G, Ls=ocrm.khatri_rao_halves(hK, E)),
          [("direct-to-LDS", dma), ("staged", staged)], sel=pr.pick(variants)[::2])


@pytest.mark.parametrize("k0,c,mode,what", [
    (160, 70, "A", "232 rows"),             # past 144 rows: the Gram over several workgroups per variant
    (150, 3, "B", "150 contexts"),          # past 128 contexts
])
def test_gram_past_the_fast_forms(k0, c, mode, what, kernel_form):
    import cellregmap_amd as crm
    from cellregmap_amd.synth import make_cohort

    co = make_cohort(8, 80, k0, 5, seed=41 + k0)                 # 640 cells
    W = _covariates(co.y.size, c, k0 + c)
    kw = {"hK": co.hK} if mode == "B" else {}
    obj = crm.CellRegMap(co.y, co.E, W=W, **kw)
    before = _used()
    res = obj.scan_interaction(crm.GenotypePanel(co.G, groups=None), return_stats=True)
    used = _used() - before
    assert used[DMA] == 0 and used[UD] == 0, used                # neither the direct-to-LDS Gram nor the Woodbury form
    _hold("mode %s %s" % (mode, what), Problem(co.y, W, co.E, co.G, **kw), [(what, res)], sel=[0, 4])


# ---- tests without a rotated test direction -----------------------------------------------------------------------------------------------
def _hold_both_kinds(case, prob, res, used, label):
    p = prob.G.shape[1]
    assert 0 < used[NONE] < p, used                              # both kinds in one scan
    at_clamp = res[2]["delta"][pr.pick(p)] > 1 - 1e-9
    assert at_clamp.any() and not at_clamp.all(), res[2]["delta"][pr.pick(p)]     # ... and among the variants held
    _hold(case, prob, [(label, res)])


def test_without_a_test_direction_on_the_unrelated_donor_route(kernel_form):
    """The phenotype with its cells permuted (``_flat_phenotype``): where a fit ends at the upper clamp of delta the test
    gets no rotated direction and the Gram reads the row of zeros (A_none).  Cohort and permutation are ones where both
    kinds occur -- 19 of 24 variants at the clamp, the one at p // 2 not."""
    import cellregmap_amd as crm
    from oracle import crm as ocrm

    co, keep, G = _ragged(6, 70, 12, 24, 31)
    y, E, W, hK = _flat_phenotype(co.y[keep], 9), co.E[keep], co.W[keep], co.hK[keep]
    with _kinship(kernel_form, route=2, diag=2, pairs=2):
        obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        before = _used()
        res = obj.scan_interaction(crm.GenotypePanel(G, groups=None), return_stats=True)
        used = _used() - before
        assert used[UD] > 0 and used[PAIRS] > 0 and used[DMA] > 0, used
    _hold_both_kinds("no test direction, unrelated route", Problem(y, W, E, G, Ls=ocrm.khatri_rao_halves(hK, E)), res, used,
                     "A_none")


def test_without_a_test_direction_on_the_plain_route():
    """Mode B (hK=), the contraction against Q0(rho*) itself: 4 of 24 variants at the clamp; the columns are rotated by one so
    that the variant at p // 2 is one of them."""
    import cellregmap_amd as crm
    from cellregmap_amd.synth import make_cohort

    co = make_cohort(8, 50, 20, 24, seed=17)
    G = np.roll(co.G + 0.05 * np.random.default_rng(2).normal(size=co.G.shape), -1, axis=1)
    y = _flat_phenotype(co.y, 5)
    obj = crm.CellRegMap(y, co.E, W=co.W, hK=co.hK)
    before = _used()
    res = obj.scan_interaction(crm.GenotypePanel(G, groups=None), return_stats=True)
    used = _used() - before
    assert used[UD] == 0, used
    _hold_both_kinds("no test direction, plain route", Problem(y, co.W, co.E, G, hK=co.hK), res, used, "A_none")


# ---- several phenotypes in one pass ----------------------------------------------------------------------------------------------------
def test_two_phenotypes_in_one_pass(kernel_form):
    """crm_scan_interaction_multi reports p, rho*, the variance components and Q: delta and the scale are read off the
    components (delta = eps2 / (e2 + g2 + eps2)), Q, the components and p are held; F, lambda and lml are not reported."""
    from cellregmap_amd import CellRegMap, GenotypePanel, _lib, get_L_values, scan_interaction_many
    from oracle import crm as ocrm
    from oracle.davies import davies_pvalue

    co, keep, G = _ragged(8, 30, 4, 70, 41)
    y, E, W, hK = co.y[keep], co.E[keep], co.W[keep], co.hK[keep]
    n, p = G.shape
    rng = np.random.default_rng(7)
    Y = np.stack([y, y + rng.normal(size=n)], axis=1)
    lib, ctx = _lib_ctx()
    with _kinship(kernel_form, route=2, diag=2):
        Ls = get_L_values(hK, E)
        first = CellRegMap(Y[:, 0], E, W=W, Ls=Ls)
        crms = [first, CellRegMap(Y[:, 1], E, W=W, Ls=Ls, background=first._bg)]
        panel = GenotypePanel(G, groups=None)
        before = _used()
        pv, info = scan_interaction_many(crms, panel)             # (binds the genes)
        assert (_used() - before)[UD] > 0
        handles = (ctypes.c_void_p * 2)(*[c._gene.value for c in crms])
        out = {k: np.empty((2, p)) for k in ("pv", "rho1", "e2", "g2", "eps2", "Q")}
        _lib.check(lib.crm_scan_interaction_multi(handles, 2, panel.handle, 0, p, None, None,
                                                  *[_lib.ptr(out[k]) for k in ("pv", "rho1", "e2", "g2", "eps2", "Q")]))
    assert np.array_equal(out["pv"], pv) and np.array_equal(out["rho1"], info["rho1"])
    sel = pr.pick(p, block=64)
    Lo = ocrm.khatri_rao_halves(hK, E)
    for i in range(2):
        prob = Problem(Y[:, i], W, E, G, Ls=Lo)
        dev, ora = [], []
        for j in sel:
            rho = out["rho1"][i, j]
            total = out["e2"][i, j] + out["g2"][i, j] + out["eps2"][i, j]
            delta = out["eps2"][i, j] / total
            (Q, F, lml, s), own = prob.at(j, rho, delta)
            ora.append(pr.errors(own, (Q, F, lml, s)))
            dev.append({"Q": float(abs(out["Q"][i, j] - Q) / max(abs(Q), np.trace(F))), "scale": float(abs(total - s) / s)})
            pref = davies_pvalue(float(Q), np.asarray(F, float), True)[0]
            assert abs(pv[i, j] - pref) <= parity_bounds.DAVIES * pref + parity_bounds.P_ATOL, (i, j, pv[i, j], pref)
        ora, dev = pr.worst(ora), pr.worst(dev)
        lim = pr.limits(ora, n)
        case = "two phenotypes in one pass, phenotype %d" % i
        print("\n[pinned] %s: n %d, variants %s\n[pinned]   oracle %s\n[pinned]   limit  %s\n[pinned]   device %s"
              % (case, n, sel, ora, lim, dev))
        RECORD[case] = {"cells": n, "variants": sel, "oracle": ora, "limit": lim, "device": {"multi": dev}}
        # (delta = eps2 / total is the device's delta rounded once more: half an ulp of delta, within the floor)
        assert dev["Q"] <= lim["Q"] and dev["scale"] <= lim["scale"], (case, dev, lim)


# ---- a slice of the fuzz stream ------------------------------------------------------------------------------------------------------------
FUZZ = fuzz_cases(24, max_cells=300, wide_covariates=True, extra_covariates=(70,))


@pytest.mark.parametrize("first", range(0, 24, 4))
def test_fuzz_slice(first):
    """Four problems of the stream per case (modes A / B / C, 1 .. 14 covariate columns, the hooks; 70 columns are among the
    stream's choices but none of its first 24 problems draws them: test_null_fit_kernels has that count), the first and
    the last variant of each, on the dense and on the donor-collapsed path."""
    from cellregmap_amd import CellRegMap, GenotypePanel

    for case in FUZZ[first:first + 4]:
        y, E, W, G, kw, hooks = build_case(case)
        obj = CellRegMap(y, E, W=W, **kw)
        res = [(path, obj.scan_interaction(GenotypePanel(G, groups=groups), return_stats=True, **hooks))
               for path, groups in (("dense", None), ("collapsed", "auto"))]
        _hold("fuzz problem %d: mode %s n %d k0 %d c %d hook %s" % (case[0], case[6], case[1], case[2], case[3], case[7]),
              Problem(y, W, E, G, **hooks, **kw), res, sel=sorted({0, G.shape[1] - 1}))
