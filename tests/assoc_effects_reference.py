"""Cohorts and the dense reference of the association scans' effect sizes (plain helper module, not a test).

For one test -- phenotype y, covariates W, variant g, the null model's grid point rho* and a variance ratio delta -- the
truth is the textbook generalised least squares at K = (1 - delta) Sigma(rho*) + delta I, formed as an n x n matrix in
``numpy.longdouble`` from the oracle's half factor of the same background (``pinned_reference.half_factor``), factorised by
the Cholesky written out in tests/pinned_reference.py, [y, W, g] whitened, W projected off by Gram-Schmidt run twice
(Frisch-Waugh: the g coefficient of the full regression is the regression of the residual y on the residual g):

    schur = |g_perp|^2 = 1 / [(X'K^-1X)^-1]_gg      beta = g_perp'y_perp / schur
    scale = (|y_perp|^2 - (g_perp'y_perp)^2 / schur) / n          beta_se = sqrt(scale / schur)

Nothing is shared with the device's path (sums over the rotated space) or with the float64 oracle's (``oracle64``: its
``LMM._terms`` at delta, then ``_rsolve``), whose distance to the truth is the yardstick e64 of the tolerance.

Cohorts (the smallest at which the kernels can still go wrong):
  A  16 donors x 12 cells = 192 cells, 4 contexts, indicator kinship factor; modes A / B / C give spectra of 4, 20 and 68
     entries (shorter than a wavefront, and no multiple of 64); 41 variants: donor-constant ones, four cell-level columns
     (GENERAL) and the planted ones below
  B  32 donors x 20 cells = 640 cells, 8 contexts, mode C: 264 spectrum entries (past one 256-thread stride)
Planted columns of cohort A: SPAN = the last column of W (the scan's rank rule drops it), BOUNDARY = that column plus 1e-9
noise (the rule's boundary: either outcome is legitimate, the column's beta is conditioned 1e7 worse than the others' and
is not held), CAUSAL = a cell-level variant that carries most of the phenotype's variance (a donor-constant one would be
absorbed by the kinship term).  At 192 cells a statistic past 1500 -- where p itself underflows -- needs a variant that
explains 99.96 % of the variance, which leaves no null model with delta inside (0, 1); cohort A's causal variant reaches a
statistic of a few hundred, and cohort B's (CAUSAL_B, 640 cells: 90 % of the variance suffice) passes 1500.  Every
phenotype also carries context, donor and donor-by-context random effects strong enough that the null models' delta stays
inside [1e-4, 1 - 1e-4] beside the causal variant's variance and that modes B and C land inside the rho grid (at rho = 1
their spectra would shrink to the contexts').
"""
import numpy as np

import pinned_reference as pr
from cellregmap_amd.synth import make_cohort
from oracle import crm as ocrm
from oracle.lmm import LMM, _rsolve
from oracle.sugar import economic_qs_linear

LD = pr.LD
GENERAL = (7, 20, 33, 40)
SPAN, BOUNDARY, CAUSAL = 3, 18, 33
PLANTED = (SPAN, BOUNDARY, CAUSAL)
CAUSAL_B = 4

# name -> cohort, mode, covariate columns.  Widths 1, 3, 9 and 63 lie on either side of the 8- and 62-column switches of
# the fit kernels; 100 columns take the effects kernel's widest tile and more than 64 KB of LDS (95 columns and more); 63
# and 100 columns go with mode B so that r + c + 1 < n.
CASES = {
    "A, mode A, c 1": ("A", "A", 1),
    "A, mode B, c 1": ("A", "B", 1),
    "A, mode C, c 1": ("A", "C", 1),
    "A, mode C, c 3": ("A", "C", 3),
    "A, mode C, c 9": ("A", "C", 9),
    "A, mode B, c 63": ("A", "B", 63),
    "A, mode B, c 100": ("A", "B", 100, (0, SPAN, 7, BOUNDARY, 20, CAUSAL, 40)),   # (a fit costs 0.13 s at this width)
    "B, mode C, c 1": ("B", "C", 1),
}

# ---- the tolerance ----------------------------------------------------------------------------------------------------
# e64: the worst relative gap of the float64 oracle's own route (LMM._terms at delta, _rsolve) to the longdouble truth for
# beta, beta_se and alt_scale over every compared test of CASES, fast and full refit, at the oracle's own delta
# (tests/test_assoc_effects_prototype_cpu.py measures it, prints it and fails if it grows past this figure): 1.557e-12,
# recorded to two digits rounded up so that another BLAS's order of summation does not fail that check.  The device may be
# off by max(8 x 1.6e-12, 1e-12) = 1.28e-11 relative: 8 for another order of summation over the spectrum (wave and tile sums against
# numpy's pairwise ones) and for the difference (plain - sum) / delta, which loses digits as delta -> 0.
E64 = 1.6e-12
TOLERANCE = max(8 * E64, 1e-12)
LOOSE = 1e-8          # planted tests whose delta leaves [1e-4, 1 - 1e-4]: tests/test_effects_woodbury_prototype_cpu.py's floor
DELTA_RANGE = (1e-4, 1 - 1e-4)
DELTA_RTOL = 1e-5     # the alt fit against the oracle's: what tests/test_gpu_association.py asks of the fitted components


class Case:
    def __init__(self, name):
        cohort, mode, c = CASES[name][:3]
        keep = CASES[name][3] if len(CASES[name]) > 3 else None      # the columns of cohort A's panel a case keeps
        self.name, self.mode, self.c = name, mode, c
        if cohort == "A":
            co = make_cohort(16, 12, 4, 41, seed=71)
        else:
            co = make_cohort(32, 20, 8, 6, seed=72, g_causals=(1,), gxe_causals=(2,))
        rng = np.random.default_rng(900 + len(name) + c)
        n = co.y.size
        self.n, self.E, self.hK_full = n, co.E, co.hK
        self.W = np.column_stack([np.ones(n)] + [rng.normal(size=n) for _ in range(c - 1)])
        G = co.G.copy()
        yk = sum(co.E[:, i] * (co.hK @ rng.normal(size=co.hK.shape[1])) for i in range(co.E.shape[1]))
        y = co.y + co.E @ (1.2 * rng.normal(size=co.E.shape[1])) + 1.5 * yk / yk.std()
        y = y + co.hK @ (1.2 * rng.normal(size=co.hK.shape[1]))
        if cohort == "A":
            for j in GENERAL:
                G[:, j] = rng.normal(size=n)
            G[:, SPAN] = self.W[:, -1]
            G[:, BOUNDARY] = self.W[:, -1] + 1e-9 * rng.normal(size=n)
            y = y + 2.5 * G[:, CAUSAL]
            self.planted, self.span, self.boundary, self.causal = PLANTED, SPAN, BOUNDARY, CAUSAL
            if keep is not None:
                G = G[:, list(keep)]
                self.span, self.boundary, self.causal = (keep.index(j) for j in PLANTED)
                self.planted = (self.span, self.boundary, self.causal)
        else:
            G[:, CAUSAL_B] = rng.normal(size=n)
            y = y + 8.0 * G[:, CAUSAL_B]
            self.planted, self.span, self.boundary, self.causal = (CAUSAL_B,), None, None, CAUSAL_B
        self.G, self.y = np.ascontiguousarray(G), y
        self.grid = [1.0] if mode == "A" else list(ocrm.RHO_GRID)
        self._gram, self._qs = {}, {}

    # the device's and the oracle's constructor arguments
    def device_kw(self):
        from cellregmap_amd import get_L_values

        if self.mode == "A":
            return {}
        return {"hK": self.hK_full} if self.mode == "B" else {"Ls": get_L_values(self.hK_full, self.E)}

    def half(self, rho):
        if self.mode == "A":
            return pr.half_factor(rho, self.E)
        if self.mode == "B":
            return pr.half_factor(rho, self.E, hK=self.hK_full)
        return pr.half_factor(rho, self.E, Ls=ocrm.khatri_rao_halves(self.hK_full, self.E))

    def gram(self, rho):
        """Sigma(rho) = hS hS' in longdouble."""
        if rho not in self._gram:
            hS = np.asarray(self.half(rho), LD)
            self._gram[rho] = hS @ hS.T
        return self._gram[rho]

    def qs(self, rho):
        if rho not in self._qs:
            (Q0,), S0 = economic_qs_linear(self.half(rho), return_q1=False)
            self._qs[rho] = (Q0, S0)
        return self._qs[rho]

    def compared(self):
        """The variants whose status must be CRM_EFFECT_OK and whose numbers are held (all but SPAN and BOUNDARY)."""
        return [j for j in range(self.G.shape[1]) if j not in (self.span, self.boundary)]


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def phenotypes(cs, count=3):
    """``count`` phenotypes on the case's background: the case's own, then ones driven by other variants."""
    rng = np.random.default_rng(33)
    cols = [cs.y]
    for i in range(1, count):
        cols.append(cs.y[rng.permutation(cs.n)] * 0.2 + cs.E @ rng.normal(size=cs.E.shape[1]) + 0.4 * cs.G[:, 10 + i]
                    + rng.normal(size=cs.n))
    return np.column_stack(cols)


def dense_truth(y, W, G, gram, deltas):
    """(beta, beta_se, scale) per column of ``G`` in longdouble at its own ``deltas[j]``; columns that share a delta share
    the factorisation of K."""
    y = np.asarray(y, LD).ravel()
    W, G = np.asarray(W, LD), np.asarray(G, LD)
    n, p = G.shape
    deltas = np.broadcast_to(np.asarray(deltas, float), (p,))
    out = np.full((3, p), np.nan, LD)
    for d in np.unique(deltas):
        sel = np.flatnonzero(deltas == d)
        K = (1 - LD(d)) * gram
        K[np.diag_indices(n)] += LD(d)
        white = pr._forward(pr._cholesky(K), np.column_stack([y, W, G[:, sel]]))
        basis, _ = pr._orthonormal(white[:, 1:1 + W.shape[1]])
        yp = pr._off(basis, white[:, 0])
        for q, j in enumerate(sel):
            gp = pr._off(basis, white[:, 1 + W.shape[1] + q])
            schur, num = gp @ gp, gp @ yp
            scale = (yp @ yp - num * num / schur) / n
            out[:, j] = num / schur, np.sqrt(scale / schur), scale
    return out


def oracle64(y, W, g, Q0, S0, delta):
    """The same three numbers by the float64 oracle's own route: ``LMM._terms`` at delta, then ``_rsolve``."""
    lmm = LMM(y, np.column_stack([W, g]), ((Q0,), S0), restricted=False)
    yKy, XKy, XKX, _ = lmm._terms(float(delta))
    tb = _rsolve(XKX, XKy)
    scale = (yKy - float(XKy @ tb)) / lmm._n
    v = lmm._Vt[:, -1]
    return float((lmm._Vt.T @ tb)[-1]), float(np.sqrt(scale * float(v @ _rsolve(XKX, v)))), float(scale)


def gaps(got, truth):
    """Relative gaps of (beta, beta_se, scale) rows to the truth, per column."""
    truth = np.asarray(truth, LD)
    return np.asarray(np.abs(np.asarray(got, LD) - truth) / np.abs(truth), float)


def oracle_null(cs, y=None):
    """(rho*, delta, Q0, S0) of the oracle's ML null model (oracle/crm.py: first strictly larger lml over the grid)."""
    y = cs.y if y is None else y
    best = None
    for rho in cs.grid:
        Q0, S0 = cs.qs(float(rho))
        lmm = LMM(y, cs.W, ((Q0,), S0), restricted=False)
        lmm.fit(verbose=False)
        if best is None or lmm.lml() > best[0]:
            best = (lmm.lml(), float(rho), lmm.delta)
    return best[1], best[2]


def oracle_alt_delta(cs, rho, g, y=None):
    """delta of ``LMM(y, [W, g], QS(rho), restricted=False).fit()``."""
    Q0, S0 = cs.qs(float(rho))
    lmm = LMM(cs.y if y is None else y, np.column_stack([cs.W, g]), ((Q0,), S0), restricted=False)
    lmm.fit(verbose=False)
    return lmm.delta


def mp_log_pvalue(alt_lml, null_lml):
    """log erfc(sqrt(lrs / 2)) at lrs = max(2 (alt - null), 0) of the given doubles, in mpmath at 40 digits."""
    import mpmath as mp

    mp.mp.dps = 40
    lrs = 2 * (mp.mpf(float(alt_lml)) - mp.mpf(float(null_lml)))
    return mp_log_sf(lrs if lrs > 0 else mp.mpf(0))


def mp_log_sf(lrs):
    import mpmath as mp

    mp.mp.dps = 40
    lrs = mp.mpf(lrs)
    if lrs == 0:
        return mp.mpf(0)
    x = mp.sqrt(lrs / 2)
    if x < 1:      # (40 digits of erfc(x) near 1 would leave none of 1 - erfc(x) at x = 1e-150)
        return mp.log1p(-mp.erf(x))
    return mp.log(mp.erfc(x))
