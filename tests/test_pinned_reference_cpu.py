"""The pinned-point reference (tests/pinned_reference.py) checked on the CPU, in three ways.

  * against something else: mpmath at 40 digits on one tiny problem per background mode (1e-17 relative), and the float64
    oracle's implicit forms at the oracle's own stopping points on the three shapes at which the reference was prototyped
    (the oracle's error there, times 4);
  * teeth: ``oracle_at`` fed operands that imitate kernel slips -- every one must fall outside the limit that
    tests/test_gpu_pinned.py applies (32 x the oracle's own error, floor n x 2.2e-16, ceiling 1e-11); printed per slip: by
    how much, and whether the tolerances the suite had before (1e-6 against the oracle, 1e-9 between two forms) would
    have let it through;
  * nothing is left out silently: a reference that cannot be evaluated raises.
"""
import numpy as np
import pytest

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
