"""Yardsticks for the table of tests/davies_cases.py (plain helper module, not a test): the float64 and long-double
runs of oracle/qfc.c per case, the limit a device p-value is held to, and mpmath statements of the modified-Liu value
and of the exact tail probability.  Computed once per process and shared by every test that asks.
"""
import functools
import math
import os
import sys

import numpy as np

import davies_cases as dc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

EPS = 2.220446049250313e-16
CEILING = 1e-9          # 32 x the float64 oracle's distance from the long-double one stays below this on every case
LIU_FLOOR = 1e-13       # relative; Liu's limit is never below it
LIU_PRESENT = 1e-8      # the relative tolerance tests/test_gpu_kernels.py holds Liu's value to
DENORMAL = 5e-324


def davies_limit(r, terms, p64, p_ld):
    """32 x what the float64 oracle achieves on this problem, and not below the floor of the device's form.

    The floor: the kernel takes sum_j atan(x_j) and sum_j log(1 + x_j^2) at an abscissa u_k from one product of r complex
    factors, about r roundings in its argument and as many in its log-modulus, so the term sin(theta / 2) w_k, with
    w_k = (Delta / pi) e^{sum3} / u_k, moves by at most about 0.75 r eps w_k (0.5 r eps from theta / 2, 0.25 r eps from
    sum3).  With u_k = (k + 1/2) Delta and e^{sum3} <= 1,  sum_k w_k <= (1 / pi) sum_k 1 / (k + 1/2)
    <= (2 + ln(2 terms + 1)) / pi, and 0.75 / pi (2 + ln(2 terms + 1)) <= 1 + ln(1 + terms)."""
    return max(32.0 * abs(p64 - p_ld), r * EPS * (1.0 + math.log(1.0 + terms)))


class Ref:
    """One case under both builds of the oracle."""

    def __init__(self, case):
        from oracle.davies import qfc, qfc_ld

        self.case = case
        self.lam = dc.kept(case.lam)
        self.r = self.lam.size
        cdf, self.ifault, tr = qfc(self.lam, case.q)
        self.p64 = 1.0 - cdf
        self.trace = (int(tr[6]), int(tr[1]), int(tr[2]))      # evaluation counter, terms, integrations
        self.p_ld, ifault_ld, tl = qfc_ld(self.lam, case.q)
        self.same_path = (self.ifault == ifault_ld and self.trace == (int(tl[6]), int(tl[1]), int(tl[2])))
        # what oracle.davies.pvalue_from_weights does with it
        self.liu_returned = self.r == 1 or not (0.0 < self.p64 <= 1.0)
        self.davies_held = self.ifault == 0 and not self.liu_returned
        self.limit = davies_limit(self.r, self.trace[1], self.p64, self.p_ld) if self.davies_held else None
        if self.r == 1:
            self.exit = "single survivor"
        elif self.ifault != 0:
            self.exit = "ifault %d" % self.ifault
        elif self.trace[2] == 0:
            self.exit = "early cdf 1 or 0"
        else:
            self.exit = "converged"


@functools.lru_cache(maxsize=None)
def refs():
    return tuple(Ref(c) for c in dc.CASES)


# ---- modified Liu in mpmath ------------------------------------------------------------------------------------------
def liu_mp(lam, q, digits=40):
    """Lee, Wu & Lin's modification of Liu's approximation for sum lam_j chi2_1, from the doubles lam and q, every step at
    `digits` digits; the non-central chi-square tail is the Poisson mixture of regularised upper incomplete gamma functions
    (non-centrality max(delta, 1e-9), as chiscore calls scipy).  Returns an mpf."""
    import mpmath as mp

    with mp.workdps(digits):
        l = [mp.mpf(float(x)) for x in lam]
        c1, c2, c3, c4 = (mp.fsum(x ** i for x in l) for i in (1, 2, 3, 4))
        s1 = c3 / mp.sqrt(c2) ** 3
        s2 = c4 / c2 ** 2
        if s1 * s1 > s2:
            a = 1 / (s1 - mp.sqrt(s1 * s1 - s2))
            delta = s1 * a ** 3 - a ** 2
            dof = a ** 2 - 2 * delta
        else:
            delta = mp.mpf(0)
            dof = 1 / s2
        t = (mp.mpf(float(q)) - c1) / mp.sqrt(2 * c2) * mp.sqrt(2 * (dof + 2 * delta)) + dof + delta
        if t <= 0:
            return mp.mpf(1)
        nc = max(delta, mp.mpf(1e-9))
        z, h, a0 = t / 2, nc / 2, dof / 2
        total = mp.mpf(0)
        w = mp.exp(-h)
        for i in range(200):
            term = w * mp.gammainc(a0 + i, z, regularized=True)
            total += term
            if i > h and term <= total * mp.mpf(10) ** (-digits):
                break
            w = w * h / (i + 1)
        return +total


def liu_limit_ok(got, want_mp, limit):
    """|got - want| <= limit * want, with one denormal step of slack where want is below the normal range (a denormal
    holds fewer digits than the limit asks for); both 0 where want underflows."""
    want = float(want_mp)
    return abs(got - want) <= limit * want + (DENORMAL if want < 2.3e-308 else 0.0)


def liu_rel_err(got, want_mp):
    want = float(want_mp)
    if want < 2.3e-308:
        return 0.0 if abs(got - want) <= DENORMAL else float("inf")
    import mpmath as mp

    return float(abs(mp.mpf(got) - want_mp) / want_mp)


@functools.lru_cache(maxsize=None)
def liu_refs():
    """{case name: (mpmath value, relative limit, relative error of oracle.davies.liu_sf)} for every case that keeps more
    than one weight.  The limit is 32 x the float64 oracle's (scipy's) own relative error, never below LIU_FLOOR.

    Rows with one weight -- or with equal weights -- are not in the table.  By Cauchy-Schwarz (sum lam^3)^2 <= sum lam^2
    sum lam^4, with equality exactly there: s1^2 = s2, so which branch of the approximation is taken turns on a rounding,
    and the branches differ by far more than a rounding."""
    from oracle.davies import liu_sf

    out = {}
    for ref in refs():
        if ref.r < 2:
            continue
        want = liu_mp(ref.lam, ref.case.q)
        got = float(liu_sf(ref.case.q, ref.lam, np.ones(ref.r), np.zeros(ref.r), True)[0])
        err = liu_rel_err(got, want)
        out[ref.case.name] = (want, max(32.0 * err, LIU_FLOOR), err)
    return out


# ---- the exact tail probability in mpmath ----------------------------------------------------------------------------
def tail_contour_mp(lam, q, digits=30):
    """P(sum lam_j chi2_1 > q) from Imhof's inversion integral, its path moved off the imaginary axis to the parabola
    t(u) = c + i sigma u + mu u^2 through the saddle point c (tools/tail_pvalue_prototype.py states the path): the
    integrand then falls like a Gaussian and the trapezoid rule converges geometrically.  The nodes are doubled until two
    rounds agree to 1e-22 relative.  c > 0 needs q > sum(lam)."""
    import mpmath as mp

    from tail_pvalue_prototype import saddle

    w64 = np.asarray(lam, float)
    c64, ok = saddle(w64, float(q))
    assert ok and c64 > 0
    with mp.workdps(digits + 10):
        w = [mp.mpf(float(x)) for x in w64]
        qq = mp.mpf(float(q))
        c = mp.mpf(c64)       # any abscissa in (0, 1 / (2 lam_max)) gives the same integral; the saddle point only makes it easy
        s = [1 - 2 * x * c for x in w]
        kc = -mp.fsum(mp.log(x) for x in s) / 2
        sigma = 1 / mp.sqrt(mp.fsum(2 * x * x / (y * y) for x, y in zip(w, s)) + 1 / (c * c))
        mu = mp.mpf("0.1") / qq
        wr = [2 * x / y for x, y in zip(w, s)]
        U = mp.mpf(30)

        wr64, sg64, mu64 = np.array([float(x) for x in wr]), float(sigma), float(mu)

        def g(u):
            # sum_j log(1 - wr_j d) on the principal branch (1 - wr d meets the real axis at d = 0 only) as the log of the
            # product, whose argument is put on the right sheet by the float64 sum of the arguments
            d = mp.mpc(mu * u * u, sigma * u)
            prod = mp.mpc(1)
            for x in wr:
                prod *= 1 - x * d
            lg = mp.log(prod)
            uf = float(u)
            arg64 = float(np.sum(np.arctan2(-wr64 * sg64 * uf, 1.0 - wr64 * mu64 * uf * uf)))
            lg = mp.mpc(lg.real, lg.imag + 2 * mp.pi * round((arg64 - float(lg.imag)) / (2 * math.pi)))
            return (mp.exp(-lg / 2 - d * qq) / (c + d) * mp.mpc(sigma, -2 * mu * u)).real

        def rule(m):
            h = U / m
            return h / mp.pi * (sigma / c / 2 + mp.fsum(g(i * h) for i in range(1, m + 1)))

        m, prev = 96, None
        while True:
            cur = rule(m)
            if prev is not None and abs(cur - prev) <= abs(cur) * mp.mpf(10) ** -22:
                break
            prev, m = cur, 2 * m
            assert m <= 6144, "the contour sum did not settle"
        return +(mp.exp(kc - c * qq) * cur)


def imhof_real_axis_mp(lam, q, digits=30):
    """Imhof (1961): P(Q > q) = 1/2 + (1 / pi) int_0^inf sin(theta(u)) / (u rho(u)) du, theta = (sum atan(lam_j u) - q u) / 2,
    rho = prod (1 + lam_j^2 u^2)^(1/4), on the real axis by mpmath's oscillatory quadrature (few weights only: the
    integrand falls like u^(-1 - r/2))."""
    import mpmath as mp

    with mp.workdps(digits):
        l = [mp.mpf(float(x)) for x in lam]
        qq = mp.mpf(float(q))

        def f(u):
            theta = (mp.fsum(mp.atan(x * u) for x in l) - qq * u) / 2
            rho = mp.fprod((1 + (x * u) ** 2) ** mp.mpf("0.25") for x in l)
            return mp.sin(theta) / (u * rho)

        return mp.mpf("0.5") + mp.quadosc(f, [0, mp.inf], omega=qq / 2) / mp.pi
