"""Regenerates tests/golden/tail_pvalue_truth.json: P(sum_j lam_j chi2_1 > q) from three sources independent of the
contour route (tools/tail_pvalue_prototype.py, csrc/tail_pvalue.hip), in mpmath:

  chi2     equal weights: the regularised upper incomplete gamma (scipy.stats.chi2.sf where it is representable)
  ruben    Ruben's (1962) series of central chi-square laws, beta = 2 lam_min lam_max / (lam_min + lam_max), summed until
           two terms in a row are below 1e-40 of the sum (weight ratios <= 50)
  imhof    Imhof's (1961) integral by mpmath.quadosc at 40 + |log10 p| digits (spreads up to SKAT's filter, 1e5)

The weights are given as kept by SKAT's filter (none is at or below mean / 1e5).  q = the quantile of a target p,
plus q at 0.999 and 1.001 of E[Q] (the saddle point crosses from the lower tail to the upper one).

    python tests/golden/make_tail_pvalue_golden.py      (a few minutes; needs mpmath and scipy)
"""
import json
import os
import sys

import mpmath as mp
import numpy as np
from scipy.stats import chi2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tools"))
from tail_pvalue_prototype import tail_pvalue  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tail_pvalue_truth.json")


def sf_equal(k, lam, q):
    mp.mp.dps = 60
    return mp.gammainc(mp.mpf(k) / 2, mp.mpf(q) / (2 * mp.mpf(lam)), mp.inf, regularized=True)


def sf_ruben(lam, q):
    mp.mp.dps = 60
    lam = [mp.mpf(x) for x in lam]
    n = len(lam)
    beta = 2 * min(lam) * max(lam) / (min(lam) + max(lam))
    gam = [1 - beta / x for x in lam]
    a = [mp.sqrt(mp.fprod(beta / x for x in lam))]
    g = []
    x = mp.mpf(q) / (2 * beta)
    # upper regularised gamma of (n/2 + j, x), stepped by Gamma(a + 1, x) = Gamma(a, x) + x^a e^-x / Gamma(a + 1)
    ah = mp.mpf(n) / 2
    sf = mp.gammainc(ah, x, mp.inf, regularized=True)
    lead = mp.exp(ah * mp.log(x) - x - mp.loggamma(ah + 1))     # x^a e^-x / Gamma(a + 1)
    total = a[0] * sf
    prev = total
    j = 0
    while True:
        j += 1
        g.append(sum(gk ** j for gk in gam) / 2)
        a.append(sum(g[j - r - 1] * a[r] for r in range(j)) / j)
        sf += lead
        lead *= x / (ah + 1)
        ah += 1
        term = a[j] * sf
        total += term
        # (two in a row: with two weights every odd coefficient is zero)
        if j > 20 and abs(term) + abs(prev) < mp.mpf(10) ** -40 * abs(total):
            return total
        prev = term
        if j > 20000:
            raise RuntimeError("Ruben series did not converge")


def sf_imhof(lam, q, digits):
    mp.mp.dps = digits
    lam = [mp.mpf(x) for x in lam]
    q = mp.mpf(q)

    def f(u):
        if u == 0:
            return (sum(lam) - q) / 2
        th = sum(mp.atan(x * u) for x in lam) / 2 - q * u / 2
        rho = mp.exp(sum(mp.log1p((x * u) ** 2) for x in lam) / 4)
        return mp.sin(th) / (u * rho)

    return mp.mpf(1) / 2 + mp.quadosc(f, [0, mp.inf], omega=q / 2) / mp.pi


def quantile_equal(k, p):
    lo, hi = 0.0, 10.0 * k + 4000.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if sf_equal(k, 1.0, mid) > p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def quantile_of(lam, p):
    """q whose p is near the target, by bisection on the prototype's log p (only the placement of q comes from it: the
    truth recorded is the series' p of the q recorded)."""
    lo, hi = 0.0, float(sum(lam)) * 2.0 + 2000.0 * max(lam)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if tail_pvalue(mid, lam)[1] > np.log(p):
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def record(cases, source, lam, q, p):
    p = mp.mpf(p)
    cases.append({"source": source, "lam": [float(x) for x in lam], "q": float(q), "p": float(p),
                  "logp": float(mp.log(p))})


def main():
    rng = np.random.default_rng(20261016)
    cases = []
    targets = [0.5, 1e-2, 1e-10, 1e-50, 1e-150, 1e-300]
    for k in (1, 2, 3, 5, 8, 20, 64, 256):
        lam = 0.7
        for p in targets:
            q = quantile_equal(k, p) * lam
            q = float(q)
            record(cases, "chi2", [lam] * k, q, sf_equal(k, lam, q))
        for f in (1e-3, 0.5, 0.999, 1.001, 3.0):
            q = f * k * lam
            record(cases, "chi2", [lam] * k, q, sf_equal(k, lam, q))
    # (the series converges like ((ratio - 1) / (ratio + 1))^j against terms that grow with q / lam_min: deep tails only
    # for narrow spreads)
    for k, ratio, deepest in ((2, 50.0, 1e-6), (3, 50.0, 1e-6), (5, 20.0, 1e-10), (8, 10.0, 1e-30), (20, 10.0, 1e-30),
                              (3, 2.0, 1e-300), (64, 3.0, 1e-50), (256, 2.0, 1e-300)):
        lam = np.sort(np.exp(rng.uniform(0.0, np.log(ratio), k)))
        lam[0], lam[-1] = 1.0, ratio
        lam = lam * 0.3
        mean = float(lam.sum())
        for p in sorted({t for t in targets if t >= deepest} | {deepest}, reverse=True):
            q = quantile_of(lam, p)
            record(cases, "ruben", lam, q, sf_ruben(lam, q))
        for f in (0.999, 1.001):
            record(cases, "ruben", lam, f * mean, sf_ruben(lam, f * mean))
    for k, spread in ((2, 1e5), (3, 1e3), (5, 1e5), (8, 1e4), (20, 1e5)):
        lam = np.sort(np.exp(rng.uniform(0.0, np.log(spread), k)))
        lam[0], lam[-1] = 1.0, spread * 0.999
        mean = float(lam.sum())
        for q in (0.999 * mean, 1.001 * mean, 0.05 * mean, 4.0 * mean, 8.0 * mean, 14.0 * mean):
            p0 = sf_imhof(lam, q, 30)
            digits = 40 + int(abs(mp.log10(p0))) + 5
            record(cases, "imhof", lam, q, sf_imhof(lam, q, digits))
    # consistency of the sources where they overlap
    for c in cases:
        if c["source"] == "chi2" and c["p"] > 1e-290:
            ref = chi2.sf(c["q"] / c["lam"][0], len(c["lam"]))
            assert abs(ref / c["p"] - 1) < 1e-12, (c, ref)
    for c in cases:
        if c["source"] == "ruben" and len(c["lam"]) <= 3 and c["p"] > 1e-15:
            im = sf_imhof(c["lam"], c["q"], 60)
            assert abs(im / mp.mpf(c["p"]) - 1) < 1e-15, (c, im)     # (p is recorded as a double)
    with open(OUT, "w") as fh:
        json.dump({"cases": cases}, fh, indent=0)
    print(f"{len(cases)} cases -> {OUT}")


if __name__ == "__main__":
    main()
