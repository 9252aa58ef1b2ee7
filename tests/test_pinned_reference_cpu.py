"""The pinned-point reference (tests/pinned_reference.py) checked on the CPU, in three ways.

  * against something else: mpmath at 40 digits on one tiny problem per background mode (1e-17 relative), and the float64
    oracle's implicit forms at the oracle's own stopping points on the three shapes at which the reference was prototyped
    (the oracle's error there, times 4);
  * teeth: ``oracle_at`` fed operands that imitate kernel slips -- every one must fall outside the limit that
    tests/test_gpu_pinned.py applies (32 x the oracle's own error, floor n x 2.2e-16, ceiling 1e-11); printed per slip: by
    how much, and whether the tolerances the suite had before (1e-6 against the oracle, 1e-9 between two forms) would
    have let it through;
  * nothing is left out silently: a reference that cannot be evaluated raises.

The same three for the effect sizes and the association likelihood-ratio tests (``pinned_effects``, ``pinned_ml``,
``pinned_ml_max`` and their yardsticks), and two conditions the GPU tests of those rely on, for every cohort they name
(tests/pinned_cases.py): at the oracle's own optimum 32 x the oracle's error stays below the 1e-11 ceiling, so the ceiling
never sets a limit; and the oracle's own Brent result meets the two-sided bound the refitting association scan is held to.
"""
import numpy as np
import pytest

import pinned_cases as pc
import pinned_reference as pr
from oracle import crm as ocrm
from oracle.scoretest import Projection, cov_solve, lstsq_solve

LD = np.longdouble


def _problem(mode, donors, cells, k0, variants, c, seed=17):
    """(y, W, E, G, keywords of the background) of a synthetic cohort with general (not donor-constant) genotypes and c
    covariate columns."""
    from cellregmap_amd.synth import make_cohort

    co = make_cohort(donors, cells, k0, variants, seed=seed)
    rng = np.random.default_rng(1)
    G = co.G + 0.05 * rng.normal(size=co.G.shape)
    W = np.column_stack([np.ones(co.y.size), rng.normal(size=(co.y.size, c - 1))])
    kw = {"A": {}, "B": {"hK": co.hK}, "C": {"Ls": ocrm.khatri_rao_halves(co.hK, co.E)}}[mode]
    return co.y, W, co.E, G, kw


# ---- against mpmath ---------------------------------------------------------------------------------------------------
def _mp_exact(x):
    """A longdouble (64-bit mantissa) as the exact sum of two doubles."""
    import mpmath as mp

    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(LD(x) - LD(hi)))


def _mp_reference(y, X, hS, D, delta):
    """The same definitions with explicit inverses and determinants at 40 digits (doubles enter exactly)."""
    import mpmath as mp

    mp.mp.dps = 40
    M = lambda a: mp.matrix(np.asarray(a, float).tolist())  # noqa: E731
    y, X, hS, D = M(np.asarray(y, float).reshape(-1, 1)), M(X), M(hS), M(D)
    n, c = X.rows, X.cols
    delta = mp.mpf(float(delta))
    Sigma = (1 - delta) * (hS * hS.T) + delta * mp.eye(n)
    Si = mp.inverse(Sigma)
    SiX = Si * X
    A = X.T * SiX
    P = Si - SiX * mp.inverse(A) * SiX.T
    Py = P * y
    df = n - c
    s = (y.T * Py)[0] / df
    u = D.T * Py
    Q = sum(v * v for v in u) / (2 * s * s)
    F = (D.T * P * D) / (2 * s)
    lml = -(df * mp.log(2 * mp.pi) + df + df * mp.log(s) + mp.log(mp.det(Sigma)) + mp.log(mp.det(A))
            - mp.log(mp.det(X.T * X))) / 2
    return Q, F, lml, s


@pytest.mark.parametrize("mode", ["A", "B", "C"])
def test_the_reference_agrees_with_mpmath_at_forty_digits(mode):
    y, W, E, G, kw = _problem(mode, 3, 12, 2, 4, 2, seed=5)          # 36 cells
    n = y.size
    rho, delta = (1.0, 0.37) if mode == "A" else (0.3, 0.37)
    hS = pr.half_factor(rho, E, **kw)
    X = np.column_stack([W, G[:, 1]])
    D = G[:, [1]] * E
    Q, F, lml, s = pr.pinned(y, X, hS, D, delta)
    mQ, mF, mlml, ms = _mp_reference(y, X, hS, D, delta)
    rel = {"Q": abs(_mp_exact(Q) - mQ) / abs(mQ), "lml": abs(_mp_exact(lml) - mlml) / abs(mlml),
           "scale": abs(_mp_exact(s) - ms) / ms,
           "F": max(abs(_mp_exact(F[i, j]) - mF[i, j]) for i in range(2) for j in range(2)) / max(abs(v) for v in mF)}
    print("mode %s, %d cells: longdouble reference against mpmath (40 digits): %s"
          % (mode, n, ", ".join("%s %.2e" % (k, float(v)) for k, v in rel.items())))
    for k, v in rel.items():
        assert v <= 1e-17, (k, float(v))


# ---- against the float64 oracle at its own stopping points -----------------------------------------------------------------
# (donors, cells per donor, k0, c), and the oracle's float64 error measured when the reference was prototyped: Q, F, lml / scale
SHAPES = {
    "300 cells, k0 = 20": ((5, 60, 20, 1), (7.7e-16, 3.5e-15, 2e-15)),
    "600 cells, k0 = 50, c = 3": ((5, 120, 50, 3), (1.6e-15, 2.3e-15, 4e-16)),
    "144 cells, k0 = 6, c = 12": ((6, 24, 6, 12), (7.4e-15, 1.1e-15, 4e-16)),
}
_cache = {}


def _at_the_oracles_points(name):
    """Per variant 0, 1, 2 of a shape: (operands, the reference, the oracle's own evaluation there); computed once."""
    if name not in _cache:
        (donors, cells, k0, c), _ = SHAPES[name]
        y, W, E, G, kw = _problem("C", donors, cells, k0, 6, c)
        o = ocrm.OracleCellRegMap(y, E, W=W, **kw)
        pv, info, st = o.scan_interaction(G[:, :3], return_stats=True)
        rows = []
        for j in range(3):
            rho, delta = info["rho1"][j], st["delta"][j]
            X, D = np.column_stack([W, G[:, j]]), G[:, [j]] * E
            Q0, S0 = o._qs[rho][0][0], o._qs[rho][1]
            ops = dict(y=y, X=X, Q0=Q0, S0=S0, half_dK=D, delta=delta)
            ref = pr.pinned(y, X, o._half[rho], D, delta)          # raises if it cannot be evaluated: nothing is dropped
            got = pr.oracle_at(**ops)
            # (oracle_at at the stopping point is the scan's own record)
            assert abs(got[0] - st["Q"][j]) <= 1e-9 * abs(st["Q"][j]) and abs(got[2] - st["lml"][j]) <= 1e-9 * abs(got[2])
            rows.append((ops, ref, got))
        _cache[name] = rows
    return _cache[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_float64_oracle_is_within_its_measured_error_of_the_reference(name):
    rows = _at_the_oracles_points(name)
    err = pr.worst([pr.errors(got, ref) for _, ref, got in rows])
    n = rows[0][0]["y"].size
    print("mode C, %s: float64 oracle against the reference: %s; the device's limit there: %s"
          % (name, ", ".join("%s %.2e" % kv for kv in err.items()),
             ", ".join("%s %.2e" % kv for kv in pr.limits(err, n).items())))
    q, f, ls = SHAPES[name][1]
    assert err["Q"] <= 4 * q and err["F"] <= 4 * f and err["lml"] <= 4 * ls and err["scale"] <= 4 * ls, err


# ---- teeth --------------------------------------------------------------------------------------------------------------
class _GNotOrthogonalised(Projection):
    """P with the row of g taken as orthogonal to W's in X' K^-1 X although nobody made it so."""

    def apply(self, v):
        A = self.X.T @ self.KiX
        A[-1, :-1] = 0.0
        A[:-1, -1] = 0.0
        return cov_solve(self.K, v) - self.KiX @ lstsq_solve(A, self.KiX.T @ v)


def _slips(rows):
    """name -> (Q, F, lml, scale) of variant 0 from wrong operands."""
    ops, _, good = rows[0]
    y, X, Q0, S0, D, delta = (ops[k] for k in ("y", "X", "Q0", "S0", "half_dK", "delta"))
    S_off = S0.copy()
    S_off[0] *= 1 + 1e-10
    r = int(np.sum(S0 > 1e-8 * S0.max()))       # (E1 = E lies in the span of the Ls: the entries past the rank are zeros,
    F_mixed = good[1].copy()                    # and leaving a zero out is no slip)
    neighbour = rows[1][2][1]
    F_mixed[-1, :], F_mixed[:, -1] = neighbour[-1, :], neighbour[:, -1]
    return {
        "the last spectrum entry (of the rank) dropped": pr.oracle_at(y, X, Q0[:, :r - 1], S0[:r - 1], D, delta),
        "the last cell left out of the n-length sums": pr.oracle_at(y[:-1], X[:-1], Q0[:-1], S0, D[:-1], delta),
        "one S0 entry off by 1e-10 relative": pr.oracle_at(y, X, Q0, S_off, D, delta),
        "one row of [W, g] not orthogonalised": pr.oracle_at(y, X, Q0, S0, D, delta, projection=_GNotOrthogonalised),
        "F's last row and column from the neighbouring variant": (good[0], F_mixed, good[2], good[3]),
        "delta (1 + 1e-9)": pr.oracle_at(y, X, Q0, S0, D, delta * (1 + 1e-9)),
    }


def slip_report(name):
    """[(slip, factor over the limit, passes 1e-6, passes 1e-9)] on a shape (the record under profiles/ keeps the
    same figures)."""
    rows = _at_the_oracles_points(name)
    n = rows[0][0]["y"].size
    lim = pr.limits(pr.worst([pr.errors(got, ref) for _, ref, got in rows]), n)
    out = []
    for slip, got in _slips(rows).items():
        err = pr.errors(got, rows[0][1])
        out.append((slip, max(err[k] / lim[k] for k in lim), max(err.values()) <= 1e-6, max(err.values()) <= 1e-9))
    return out


@pytest.mark.parametrize("name", ["300 cells, k0 = 20", "144 cells, k0 = 6, c = 12"])
def test_every_injected_slip_is_rejected(name):
    report = slip_report(name)
    for slip, factor, at_1e6, at_1e9 in report:
        print("%s / %-55s %9.3g x the limit; 1e-6 against the oracle would %s it, 1e-9 between forms would %s it"
              % (name, slip + ":", factor, "pass" if at_1e6 else "reject", "pass" if at_1e9 else "reject"))
    assert len(report) == 6
    for slip, factor, _, _ in report:
        assert factor > 1, (slip, factor)


# ---- nothing is left out silently ---------------------------------------------------------------------------------------------
def test_a_reference_that_cannot_be_evaluated_raises():
    y, W, E, G, kw = _problem("B", 3, 12, 2, 4, 2, seed=5)
    X, D = np.column_stack([W, G[:, 0]]), G[:, [0]] * E
    hS = pr.half_factor(0.3, E, **kw)                               # 5 columns for 36 cells: hS hS' is singular
    with pytest.raises(np.linalg.LinAlgError):
        pr.pinned(y, X, hS, D, 0.0)
    with pytest.raises(ValueError):
        pr.pinned(y, np.column_stack([X, X[:, 1] - 2 * X[:, 2]]), hS, D, 0.4)
    assert np.all(np.isfinite(np.asarray(pr.pinned(y, X, hS, D, 0.4)[1], float)))


def test_limits_keep_their_floor_and_their_ceiling():
    lim = pr.limits({"Q": 1e-16, "F": 3e-15, "lml": 1e-3, "scale": 0.0}, 300)
    assert lim == {"Q": 300 * 2.2e-16, "F": 32 * 3e-15, "lml": 1e-11, "scale": 300 * 2.2e-16}
    assert pr.pick(40) == [0, 20, 39] and pr.pick(1) == [0] and pr.pick(2) == [0, 1] and pr.pick(70, block=64) == [0, 64, 69]


# =========================================================================================================================
# effect sizes and association likelihood-ratio tests
# =========================================================================================================================
def _mp_matrix(a):
    import mpmath as mp

    return mp.matrix(np.asarray(a, float).tolist())


def _mp_gap(x, ref):
    return float(abs(_mp_exact(x) - ref) / abs(ref))


@pytest.mark.parametrize("mode", ["A", "C"])
def test_the_effects_reference_agrees_with_mpmath_at_forty_digits(mode):
    import mpmath as mp

    mp.mp.dps = 40
    y, W, E, G, kw = _problem(mode, 3, 12, 2, 4, 2, seed=5)          # 36 cells
    g = G[:, [1]]
    M, U = np.column_stack([W, g, E]), g * E
    half_L = None if mode == "A" else np.concatenate(kw["Ls"], axis=1)
    rho, v0, v1 = (1.0, 0.8, 0.5) if mode == "A" else (0.3, 0.8, 0.5)
    beta, u = pr.pinned_effects(y, M, U, half_L, rho, v0, v1)
    mU, mM, my = _mp_matrix(U), _mp_matrix(M), _mp_matrix(y.reshape(-1, 1))
    K = mp.mpf(v0) * mp.mpf(rho) * (mU * mU.T) + mp.mpf(v1) * mp.eye(y.size)
    if half_L is not None:
        mL = _mp_matrix(half_L)
        K += mp.mpf(v0) * (1 - mp.mpf(rho)) * (mL * mL.T)
    Ki = mp.inverse(K)
    mbeta = mp.inverse(mM.T * Ki * mM) * (mM.T * Ki * my)
    mu = mU.T * Ki * (my - mM * mbeta)
    gaps = {"beta": max(abs(_mp_exact(beta[i]) - mbeta[i]) for i in range(M.shape[1])) / max(abs(v) for v in mbeta),
            "u": max(abs(_mp_exact(u[i]) - mu[i]) for i in range(U.shape[1])) / max(abs(v) for v in mu)}
    print("mode %s, %d cells: pinned_effects against mpmath (40 digits): %s"
          % (mode, y.size, ", ".join("%s %.2e" % (k, float(v)) for k, v in gaps.items())))
    for k, v in gaps.items():
        assert v <= 1e-18, (k, float(v))


def _mp_ml(y, X, hS, delta):
    """ML lml and scale at 40 digits; ``delta`` an mpf."""
    import mpmath as mp

    my, mX, mS = _mp_matrix(np.asarray(y, float).reshape(-1, 1)), _mp_matrix(X), _mp_matrix(hS)
    n = my.rows
    Sigma = (1 - delta) * (mS * mS.T) + delta * mp.eye(n)
    Si = mp.inverse(Sigma)
    SiX = Si * mX
    P = Si - SiX * mp.inverse(mX.T * SiX) * SiX.T
    s = (my.T * P * my)[0] / n
    return -(n * mp.log(2 * mp.pi) + n + n * mp.log(s) + mp.log(mp.det(Sigma))) / 2, s


@pytest.mark.parametrize("mode", ["A", "B"])
def test_the_ml_reference_and_its_maximum_agree_with_mpmath_at_forty_digits(mode):
    import mpmath as mp

    mp.mp.dps = 40
    y, W, E, G, kw = _problem(mode, 3, 12, 2, 4, 2, seed=5)
    hS = pr.half_factor(1.0 if mode == "A" else 0.3, E, **kw)
    X = np.column_stack([W, G[:, 1]])
    lml, s = pr.pinned_ml(y, X, hS, 0.37)
    mlml, ms = _mp_ml(y, X, hS, mp.mpf(0.37))
    gaps = {"lml": _mp_gap(lml, mlml), "scale": _mp_gap(s, ms)}
    # the maximum: the value at x* is the reference's there, and mpmath's likelihood falls off on both sides of x*
    o = ocrm.LMM(y, X, ocrm.economic_qs_linear(hS, return_q1=False), restricted=False)
    o.fit(verbose=False)
    top, x, curvature = pr.pinned_ml_max(y, X, hS, o._x)
    mx = _mp_exact(x)
    at = lambda t: _mp_ml(y, X, hS, 1 / (1 + mp.exp(-t)))[0]  # noqa: E731
    mtop = at(mx)
    gaps["maximum"] = _mp_gap(top, mtop)
    h = mp.mpf("1e-5")
    lo, hi = at(mx - h), at(mx + h)
    assert lo < mtop and hi < mtop
    gaps["curvature"] = float(abs(-(hi - 2 * mtop + lo) / (h * h) - _mp_exact(curvature)) / _mp_exact(curvature))
    # (the vertex of mpmath's own parabola through the three points: where x* should be)
    gaps["x*"] = float(abs(-h * (hi - lo) / (2 * (hi - 2 * mtop + lo))))
    print("mode %s: pinned_ml / pinned_ml_max against mpmath: %s" % (mode, ", ".join("%s %.2e" % kv for kv in gaps.items())))
    assert gaps["lml"] <= 1e-18 and gaps["scale"] <= 1e-18 and gaps["maximum"] <= 1e-18, gaps
    assert gaps["curvature"] <= 1e-6 and gaps["x*"] <= 1e-9, gaps
    assert abs(float(x) - o._x) <= 3 * (1e-6 * abs(o._x) + 1e-6)          # (Brent stopped within its tolerance of it)


# ---- the yardsticks at the oracle's own points, every cohort the GPU tests name ---------------------------------------------------
_effects_cache, _assoc_cache = {}, {}


def _effects_rows(name):
    """Per pair of a cohort that the GPU tests hold (pinned_cases.EFFECTS_HELD): (operands and the oracle's point,
    (reference record, oracle record))."""
    if name not in _effects_cache:
        cs = pc.EffectsCase(name)
        rows = []
        for i, v in pc.EFFECTS_HELD[name]:
            y, M, U = cs.operands(i, v)
            rho, v0, v1, _ = pc.oracle_effects_point(y, M, U, cs.half_L, cs.grid)
            rows.append(((y, M, U, cs.half_L, rho, v0, v1), pc.effects_records(cs, y, M, U, rho, v0, v1)))
        _effects_cache[name] = (cs, rows)
    return _effects_cache[name]


def _assoc_rows(name):
    """Of a cohort, at the oracle's own null model: the case, (rho, delta, Q0, S0), the reference's and the oracle's null
    (lml, scale), and per variant the fast scanner's alternative, the refit's maximum and the oracle's Brent result."""
    if name not in _assoc_cache:
        cs = pc.AssociationCase(name)
        rho, null, (Q0, S0) = pc.oracle_null(cs.y, cs.W, cs.half, cs.grid)
        delta, hS = null.delta, cs.half(rho)
        ref_null = pr.pinned_ml(cs.y, cs.W, hS, delta)
        own_null = pr.oracle_ml_at(cs.y, cs.W, Q0, S0, delta, cs.G)
        hS_ld = np.asarray(hS, pr.LD)
        gram = hS_ld @ hS_ld.T
        variants = []
        for j in pr.pick(cs.G.shape[1]):
            X = np.column_stack([cs.W, cs.G[:, j]])
            fast = pr.pinned_ml(cs.y, X, None, delta, gram=gram)[0]
            o = ocrm.LMM(cs.y, X, ((Q0,), S0), restricted=False)
            o.fit(verbose=False)
            top, x, curvature = pr.pinned_ml_max(cs.y, X, None, o._x, gram=gram)
            at = float(pr._logistic(x))
            variants.append({"j": j, "fast": fast, "top": top, "x": x, "curvature": curvature, "brent": o.lml(),
                             "own_top": pr.oracle_ml_at(cs.y, X, Q0, S0, at)[0],
                             "ref_at": pr.pinned_ml(cs.y, X, None, at, gram=gram)[0]})
        _assoc_cache[name] = (cs, (rho, delta, Q0, S0), ref_null, own_null, variants)
    return _assoc_cache[name]


def _assoc_oracle_errors(name):
    cs, _, (rl, rs), (ol, osc, oalt), variants = _assoc_rows(name)
    rows = [pr.ml_errors({"lml": ol, "scale": osc}, {"lml": rl, "scale": rs})]
    for v in variants:
        rows.append(pr.ml_errors({"lml": oalt[v["j"]], "lrs": (oalt[v["j"]], ol)}, {"lml": v["fast"], "lrs": (v["fast"], rl)}))
        rows.append(pr.ml_errors({"lml": v["own_top"]}, {"lml": v["ref_at"]}))
    return {k: max(r[k] for r in rows if k in r) for k in ("lml", "scale", "lrs")}


# the oracle's float64 error measured when these references were prototyped (the largest over the three phenotypes)
EFFECTS_MEASURED = {
    "width 10, r_L 24": {"beta": 3.0e-14, "u": 1.4e-13, "beta_gxe": 1.1e-13, "lml": 1.5e-15, "scale": 5.0e-15},
    "width 66, r_L 40": {"beta": 8.3e-15, "u": 1.8e-14, "beta_gxe": 2.5e-14, "lml": 2.3e-15, "scale": 9.3e-15},
    "width 130, r_L 10": {"beta": 6.4e-15, "u": 1.8e-14, "beta_gxe": 2.1e-14, "lml": 4.5e-16, "scale": 2.7e-15},
}
ASSOCIATION_MEASURED = {
    "c 1, mode B": {"lml": 4.9e-15, "scale": 1.4e-14, "lrs": 4.8e-16},
    "c 70, mode B": {"lml": 7.1e-16, "scale": 7.8e-16, "lrs": 9.3e-16},
    "rank 260, mode B": {"lml": 3.9e-16, "scale": 6.3e-16, "lrs": 4.5e-16},
}


@pytest.mark.parametrize("name", list(EFFECTS_MEASURED))
def test_the_effects_yardstick_is_within_its_measured_error(name):
    _, rows = _effects_rows(name)
    err = pr.worst([pr.effects_errors(own, ref) for _, (ref, own) in rows[:3]])
    print("%s: float64 oracle against pinned_effects: %s" % (name, ", ".join("%s %.2e" % kv for kv in err.items())))
    for k, v in EFFECTS_MEASURED[name].items():
        assert err[k] <= 4 * v, (k, err[k], v)


@pytest.mark.parametrize("name", list(ASSOCIATION_MEASURED))
def test_the_ml_yardstick_is_within_its_measured_error(name):
    err = _assoc_oracle_errors(name)
    print("%s: float64 oracle against pinned_ml: %s" % (name, ", ".join("%s %.2e" % kv for kv in err.items())))
    for k, v in ASSOCIATION_MEASURED[name].items():
        assert err[k] <= 4 * v, (k, err[k], v)


@pytest.mark.parametrize("name", list(pc.EFFECTS))
def test_the_ceiling_never_sets_a_limit_on_the_effects_cohorts(name):
    cs, rows = _effects_rows(name)
    err = pr.worst([pr.effects_errors(own, ref) for _, (ref, own) in rows])
    print("%s (%d cells): 32 x the oracle's error: %s" % (name, cs.n, ", ".join("%s %.2e" % (k, 32 * v) for k, v in err.items())))
    for k, v in err.items():
        assert pr.PATHS * v <= pr.CEILING, (name, k, v)
    if name == "width 10, r_L 24":          # the three ends the GPU test asks of this cohort
        rhos = [row[0][4] for row in rows[:3]]
        assert rhos[0] == 0.0 and 0.0 < rhos[1] < 1.0 and rhos[2] == 1.0, rhos


@pytest.mark.parametrize("name", list(pc.ASSOCIATION))
def test_the_ceiling_never_sets_a_limit_on_the_association_cohorts(name):
    cs, (rho, delta, _, _), _, _, variants = _assoc_rows(name)
    err = _assoc_oracle_errors(name)
    print("%s (%d cells, rho %.1f, delta %.4g): 32 x the oracle's error: %s"
          % (name, cs.n, rho, delta, ", ".join("%s %.2e" % (k, 32 * v) for k, v in err.items())))
    for k, v in err.items():
        assert pr.PATHS * v <= pr.CEILING, (name, k, v)
    for v in variants:                      # the refit bound is stated for optima away from the clamps
        assert 1e-3 < float(pr._logistic(v["x"])) < 1 - 1e-3, (name, v["j"], float(v["x"]))


def test_the_association_cohorts_land_on_both_ends_and_the_interior_of_the_grid():
    rhos = {name: _assoc_rows(name)[1][0] for name in pc.ASSOCIATION if pc.ASSOCIATION[name][4] == "B"}
    assert 0.0 in rhos.values() and 1.0 in rhos.values() and any(0.0 < r < 1.0 for r in rhos.values()), rhos


@pytest.mark.parametrize("name", list(pc.ASSOCIATION))
def test_the_oracles_brent_result_meets_the_refit_bound(name):
    cs, _, _, _, variants = _assoc_rows(name)
    lim = pr.limits(_assoc_oracle_errors(name), cs.n)["lml"]
    for v in variants:
        top, short = float(v["top"]), float(v["top"] - pr.LD(v["brent"]))
        allowed = lim * abs(top) + pr.refit_allowance(v["x"], v["curvature"])
        print("%s variant %d: L* %.6f, the oracle's Brent result short of it by %.3e (limit %.3e, allowance %.3e)"
              % (name, v["j"], top, short, lim * abs(top), allowed - lim * abs(top)))
        assert -short <= lim * abs(top), (name, v["j"], short)
        assert short <= allowed, (name, v["j"], short, allowed)


# ---- teeth ------------------------------------------------------------------------------------------------------------------
def _woodbury(cs, y, M, U, rho, v0, v1, slip=None):
    """(beta, u, lml, scale) through the rank-k0 form effects_multi.hip evaluates (its header's formulas) in float64;
    ``slip``: one of the imitated mistakes."""
    from oracle.sugar import economic_svd

    n, P, k0 = y.size, M.shape[1], U.shape[1]
    s, delta = v0 + v1, v1 / (v0 + v1)
    if cs.half_L is None:
        QL, SL = np.zeros((n, 0)), np.zeros(0)
    else:
        QL, sv, _ = economic_svd(cs.half_L)
        SL = sv ** 2
    if slip == "S_L rounded to float32":
        SL = SL.astype(np.float32).astype(float)
    Z = np.column_stack([M, y, U])
    T = QL.T @ Z
    Cp = Z.T @ Z - T.T @ T
    Cd = Cp / delta
    if slip == "one complement numerator without its / delta":
        Cd[cs.cW, P] = Cd[P, cs.cW] = Cp[cs.cW, P]                # c(g, y)
    w = 1 / (delta + (1 - delta) * (1 - rho) * SL)
    N = (T.T * w) @ T + Cd
    H, B, C = N[:P + 1, :P + 1], N[P + 1:, :P + 1], N[P + 1:, P + 1:]
    logdet = np.log(delta + (1 - delta) * (1 - rho) * SL).sum() + (n - SL.size) * np.log(delta)
    cdiag = 1.0
    if rho > 0:
        cdiag = 1 / ((1 - delta) * rho) * (1 + 1e-8 if slip == "the core's I / ((1 - delta) rho) off by 1e-8" else 1)
        C = C + cdiag * np.eye(k0)
        H = H - B.T @ np.linalg.solve(C, B)
        logdet += np.linalg.slogdet(C)[1] + k0 * np.log((1 - delta) * rho)
    beta = np.linalg.solve(H[:P, :P], H[:P, P])
    t = B[:, P] - B[:, :P] @ beta
    if rho > 0:
        t = np.linalg.solve(C, t) * cdiag
    scale = (H[P, P] - H[:P, P] @ beta) / (n - P)
    lml = -0.5 * ((n - P) * np.log(2 * np.pi) + (n - P) + (n - P) * np.log(scale) + logdet
                  + np.linalg.slogdet(H[:P, :P])[1] - np.linalg.slogdet(M.T @ M)[1])
    return beta, t / s, lml, scale


def _fast_scan(lmm, g, delta, reduced=True):
    """The fast scanner's alternative lml of one variant by the Schur reduction assoc.hip uses: the null model's residual
    sum less num^2 / schur; ``reduced=False``: with the unreduced g'K^-1 g in place of the Schur complement."""
    yKy, XKy, XKX, logdet = lmm._terms(delta)
    w = 1.0 / ((1.0 - delta) * lmm._S0 + delta)
    tg = lmm._Q0.T @ g
    gKg = (tg * w) @ tg + (g @ g - tg @ tg) / delta
    gKy = (tg * w) @ lmm._ty + (g @ lmm._y - tg @ lmm._ty) / delta
    gKX = lmm._tXr.T @ (w * tg) + (lmm._tX.T @ g - lmm._tXr.T @ tg) / delta
    beta0 = np.linalg.solve(XKX, XKy)
    num = gKy - gKX @ beta0
    schur = gKg - gKX @ np.linalg.solve(XKX, gKX) if reduced else gKg
    n = lmm._n
    s = (yKy - XKy @ beta0 - num * num / schur) / n
    return -0.5 * (n * np.log(2 * np.pi) + n + n * np.log(s) + logdet)


def slip_report_effects_association():
    """[(slip, factor over the limit, whether the bound the suite had before passes it)]: five slips of the effect-size
    kernels on the pair of the smallest cohort whose rho* is interior, three of the association kernels on the c = 9 cohort.
    The bounds before: 1e-7 of the largest magnitude for beta, u and beta_gxe (test_gpu_effects.py, polished fits);
    1e-10 |null lml| for an alternative lml (test_gpu_association*.py)."""
    out = []
    cs, rows = _effects_rows("width 10, r_L 24")
    (y, M, U, half_L, rho, v0, v1), (ref, own) = rows[1]
    lim = pr.limits(pr.worst([pr.effects_errors(o, r) for _, (r, o) in rows[:3]]), cs.n)
    clean = pr.effects_errors(pc.effects_records(cs, y, M, U, rho, v0, v1, got=_woodbury(cs, y, M, U, rho, v0, v1))[1], ref)
    assert all(clean[k] <= lim[k] for k in lim), (clean, lim)          # the imitation itself is within the limit

    def ols_residual(lmm, Q0, S0):
        from oracle.scoretest import LowRankCov

        r = y - M @ np.linalg.lstsq(M, y, rcond=None)[0]
        return lmm.beta, U.T @ cov_solve(LowRankCov(Q0, S0, v0, v1), r)

    slipped = {s: _woodbury(cs, y, M, U, rho, v0, v1, slip=s)
               for s in ("the core's I / ((1 - delta) rho) off by 1e-8", "one complement numerator without its / delta",
                         "S_L rounded to float32")}
    slipped["u from the OLS residual"] = pr.oracle_effects_at(y, M, U, half_L, rho, v0, v1, fit=ols_residual)
    records = {s: pc.effects_records(cs, y, M, U, rho, v0, v1, got=got)[1] for s, got in slipped.items()}
    records["beta_gxe scaled by v0 instead of v0 rho"] = dict(own, beta_gxe=v0 * (cs.E0 @ own["u"]))
    for slip, rec in records.items():
        err = pr.effects_errors(rec, ref)
        out.append((slip, max(err[k] / lim[k] for k in lim), max(err[k] for k in ("beta", "u", "beta_gxe")) <= 1e-7))

    name = "c 9, mode B"
    cs, (rho, delta, Q0, S0), (rl, rs), (ol, osc, oalt), variants = _assoc_rows(name)
    lim = pr.limits(_assoc_oracle_errors(name), cs.n)
    n, c, r = cs.n, cs.W.shape[1], S0.size
    j, fast = variants[0]["j"], variants[0]["fast"]
    lmm = pr._LMMAt(cs.y, cs.W, ((Q0,), S0), restricted=False)
    lmm._at = delta
    clean = pr.ml_errors({"lml": _fast_scan(lmm, cs.G[:, j], delta)}, {"lml": fast})
    assert clean["lml"] <= lim["lml"], (clean, lim)
    for slip, got, ref in (
            ("ML scale with n - c for n", {"lml": ol - n / 2 * np.log(n / (n - c)), "scale": osc * n / (n - c)},
             {"lml": rl, "scale": rs}),
            ("log|K| with r for n in the (n - r) log delta term", {"lml": ol + (n - r) / 2 * np.log(delta)}, {"lml": rl}),
            ("num^2 / schur with the unreduced g'K^-1 g", {"lml": _fast_scan(lmm, cs.G[:, j], delta, reduced=False)},
             {"lml": fast})):
        err = pr.ml_errors(got, ref)
        out.append((slip, max(err[k] / lim[k] for k in err), abs(float(got["lml"] - ref["lml"])) <= 1e-10 * abs(float(rl))))
    return out


def test_every_injected_slip_of_the_effects_and_association_kernels_is_rejected():
    report = slip_report_effects_association()
    for slip, factor, before in report:
        print("%-55s %9.3g x the limit; the bound the suite had before would %s it" % (slip + ":", factor, "pass" if before else "reject"))
    assert len(report) == 8
    for slip, factor, _ in report:
        assert factor > 1, (slip, factor)


def test_an_effects_reference_that_cannot_be_evaluated_raises():
    cs, rows = _effects_rows("width 10, r_L 24")
    y, M, U, half_L, rho, v0, v1 = rows[1][0]
    with pytest.raises(ValueError):
        pr.pinned_effects(y, np.column_stack([M, M[:, 1] - 2 * M[:, 3]]), U, half_L, rho, v0, v1)
    with pytest.raises(np.linalg.LinAlgError):
        pr.pinned_effects(y, M, U, half_L, rho, v0, 0.0)             # K singular: 3 + 24 columns for 120 cells


# =========================================================================================================================
# the null fits of the interaction scan at every grid point (tests/test_gpu_pinned_null_model.py)
# =========================================================================================================================
def _mp_restricted(y, X, hS, delta):
    """The restricted lml at 40 digits; ``delta`` an mpf."""
    import mpmath as mp

    my, mX, mS = _mp_matrix(np.asarray(y, float).reshape(-1, 1)), _mp_matrix(X), _mp_matrix(hS)
    n, c = mX.rows, mX.cols
    Sigma = (1 - delta) * (mS * mS.T) + delta * mp.eye(n)
    Si = mp.inverse(Sigma)
    SiX = Si * mX
    A = mX.T * SiX
    P = Si - SiX * mp.inverse(A) * SiX.T
    df = n - c
    s = (my.T * P * my)[0] / df
    return -(df * mp.log(2 * mp.pi) + df + df * mp.log(s) + mp.log(mp.det(Sigma)) + mp.log(mp.det(A))
             - mp.log(mp.det(mX.T * mX))) / 2


def test_the_restricted_maximum_agrees_with_mpmath_at_forty_digits():
    import mpmath as mp

    mp.mp.dps = 40
    y, W, E, G, kw = _problem("B", 3, 12, 2, 4, 2, seed=5)
    hS = pr.half_factor(0.3, E, **kw)
    X = np.column_stack([W, G[:, 1]])
    o = ocrm.LMM(y, X, ocrm.economic_qs_linear(hS, return_q1=False), restricted=True)
    o.fit(verbose=False, polish=True)
    top, x, curvature, clamp = pr.null_trial_reference(y, X, hS, o._x)
    assert clamp is None
    mx = _mp_exact(x)
    at = lambda t: _mp_restricted(y, X, hS, 1 / (1 + mp.exp(-t)))  # noqa: E731
    mtop = at(mx)
    h = mp.mpf("1e-5")
    lo, hi = at(mx - h), at(mx + h)
    assert lo < mtop and hi < mtop
    gaps = {"maximum": _mp_gap(top, mtop),
            "curvature": float(abs(-(hi - 2 * mtop + lo) / (h * h) - _mp_exact(curvature)) / _mp_exact(curvature)),
            "x*": float(abs(-h * (hi - lo) / (2 * (hi - 2 * mtop + lo))))}
    print("pinned_max(restricted=True) against mpmath: %s" % ", ".join("%s %.2e" % kv for kv in gaps.items()))
    assert gaps["maximum"] <= 1e-18 and gaps["curvature"] <= 1e-6 and gaps["x*"] <= 1e-9, gaps


def test_a_trial_at_the_clamp_is_marked_not_raised():
    """No random effect at all: the oracle's polished fit sits at delta = 1 - 2^-52, where no stencil has a vertex."""
    cs = pc.null_model_case("no kinship term")
    top, x, curvature, clamp = cs.trial(0, 3)[1]
    assert clamp == 1 - pr.CLAMP and curvature is None and abs(float(x) - 36.04365338911715) < 1e-9
    assert float(top) == float(pr.pinned(cs.y, cs.X(0), cs.half(3), np.zeros((cs.n, 0)), clamp)[2])
    with pytest.raises(ValueError):                    # (started anywhere else on that likelihood it has no maximum nearby)
        pr.pinned_max(cs.y, cs.X(0), cs.half(3), 5.0, restricted=True)


LADDER = (-12, -8, -4, -2, -1, 0, 1, 2, 4, 8, 12)


def _oracle_records(cs, variants):
    """[variant][grid] -> (lml, delta, scale) of the float64 oracle's own Brent search: what stands in for the device."""
    return {j: [cs.oracle_fit(j, i)[0] for i in range(len(cs.grid))] for j in variants}


def null_model_oracle_shares(name):
    """(case, held variants, the oracle's Brent records, limits, {(variant, grid): shares}, the largest share per bound) of
    a cohort with the float64 oracle's own unpolished search in the device's place."""
    cs = pc.null_model_case(name)
    sel = cs.picks()
    rec = _oracle_records(cs, sel)
    lim, ora, shares = pc.hold_trials(cs, rec, sel)              # (a reference that cannot be evaluated raises here)
    worst = {}
    for sh in shares.values():
        for k, v in sh.items():
            worst[k] = max(worst.get(k, -np.inf), v)
    return cs, sel, rec, lim, shares, worst


@pytest.mark.parametrize("name", list(pc.NULL_MODEL))
def test_the_null_model_cohorts_meet_their_conditions(name):
    """What tests/test_gpu_pinned_null_model.py relies on, for every cohort it names and every trial it holds, from the
    reference and the float64 oracle alone: ``pinned`` raises nowhere; the oracle's own unpolished Brent stop passes b, c
    and d within the same limits; the maximum found from the oracle's basin is the global one on a ladder of x; and the
    oracle's own choice of rho* passes e and f.  (With the oracle in the device's place its lml and scale shares are 1/32
    at most by construction -- the limit is 32 x its own error; the stopping point and the two sides of L* are what this
    run decides.)"""
    cs, sel, rec, lim, shares, worst = null_model_oracle_shares(name)
    assert max(lim.values()) <= pr.CEILING, (name, lim)
    for key, sh in shares.items():
        for k, v in sh.items():
            assert v <= 1, (name, key, k, v)
    for j in sel:
        tops = []
        for i in range(len(cs.grid)):
            top = cs.trial(j, i)[1][0]
            tops.append(top)
            for x in LADDER:
                assert cs.reference_lml(j, i, x) <= top + lim["lml"] * abs(top), (name, j, i, x)
        index = int(np.argmax([r[0] for r in rec[j]]))
        assert pr.selection_from_records([r[0] for r in rec[j]], index)
        assert pr.selection_against_reference(tops, index, lim["lml"])[0], (name, j, index)
    print("%s (%d cells, variants %s): limits %s; the oracle's own search, largest shares: %s"
          % (name, cs.n, sel, " ".join("%s %.2e" % kv for kv in lim.items()), ", ".join("%s %.3g" % kv for kv in worst.items())))


def test_the_clamped_and_the_tied_cohorts_are_what_they_are_named():
    cs = pc.null_model_case("no kinship term")
    lim = pc.hold_trials(cs, _oracle_records(cs, cs.picks()), cs.picks())[0]
    for j in cs.picks():
        trials = [cs.trial(j, i)[1] for i in range(len(cs.grid))]
        assert all(t[3] == 1 - pr.CLAMP for t in trials)
        assert pr.argmax_or_tie([t[0] for t in trials], lim["lml"])[1]
    cs = pc.null_model_case("strong kinship term")
    for j in cs.picks():
        assert all(cs.trial(j, i)[1][3] is None and cs.oracle_fit(j, i)[0][1] < 0.2 for i in range(len(cs.grid) - 1))


def slip_report_null_model():
    """[(slip, factor over the bound that rejects it)] on the cohort "c 3, r 64, dense": the float64 oracle's own records --
    which pass -- with one imitated mistake each, through the checks of tests/test_gpu_pinned_null_model.py."""
    cs = pc.null_model_case("c 3, r 64, dense")
    p, nrho = cs.G.shape[1], len(cs.grid)
    sel = cs.picks()
    good = _oracle_records(cs, range(p))
    j, i = sel[1], 5                                              # an interior trial of an interior grid point
    (top, x, curvature, clamp), won = cs.trial(j, i)[1], int(np.argmax([r[0] for r in good[j]]))
    assert clamp is None and i != won

    def at_x(xx, delta=None):
        delta = float(pr._logistic(xx)) if delta is None else delta
        lml, scale = pr.oracle_null_at(cs.y, cs.X(j), *cs.qs(i), delta)
        return lml, delta, scale

    def worst_share(rec_ji, keys=None):
        rec = {v: list(good[v]) for v in sel}
        rec[j][i] = rec_ji
        _, _, shares = pc.hold_trials(cs, rec, sel)
        return max(v for k, v in shares[(j, i)].items() if keys is None or k in keys)

    tol = 1e-6 * abs(float(x)) + 1e-6
    lml, delta, scale = good[j][i]
    out = [("a stop ten tolerances from x*", worst_share(at_x(float(x) + 10 * tol), ("stop",))),
           ("a clamp reported for an interior optimum", worst_share(at_x(None, 1 - pr.CLAMP), ("short of L*", "stop"))),
           ("the wrong side of the bracket (x* - 4)", worst_share(at_x(float(x) - 4.0), ("short of L*",))),
           ("a non-winning grid point's lml off by 1e-9 relative", worst_share((lml * (1 + 1e-9), delta, scale), ("lml",))),
           ("the ML scale (/ n) where the restricted one belongs",
            worst_share((lml, delta, scale * (cs.n - cs.c - 1) / cs.n), ("scale",)))]
    # the table read as [grid][variant]
    flat = [good[v][g] for v in range(p) for g in range(nrho)]
    swapped = {v: [flat[g * p + v] for g in range(nrho)] for v in range(p)}
    _, _, shares = pc.hold_trials(cs, swapped, sel)
    out.append(("the trial table read as [grid][variant]", max(max(sh.values()) for sh in shares.values())))
    # selection
    lim = pc.hold_trials(cs, good, sel)[0]
    tops = [cs.trial(j, g)[1][0] for g in range(nrho)]
    lmls = [r[0] for r in good[j]]
    assert pr.selection_from_records(lmls, won) and pr.selection_against_reference(tops, won, lim["lml"]) == (True, False)
    tied = list(lmls)
    tied[nrho - 1] = tied[won]
    assert pr.selection_from_records(tied, won)
    inf = float("inf")
    off = won + 1 if won + 1 < nrho else won - 1
    out.append(("the last instead of the first of equal maxima", 1.0 if pr.selection_from_records(tied, nrho - 1) else inf))
    out.append(("a rho index off by one without a tie (from the records)", 1.0 if pr.selection_from_records(lmls, off) else inf))
    out.append(("a rho index off by one without a tie (against the reference)",
                1.0 if pr.selection_against_reference(tops, off, lim["lml"])[0] else inf))
    return out


def test_every_injected_slip_of_the_null_model_is_rejected():
    report = slip_report_null_model()
    for slip, factor in report:
        print("%-62s %9.3g x the bound" % (slip + ":", factor))
    assert len(report) == 9
    for slip, factor in report:
        assert factor > 1, (slip, factor)
