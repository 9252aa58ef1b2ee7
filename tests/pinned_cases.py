"""The cohorts of tests/test_gpu_pinned_effects.py, tests/test_gpu_pinned_association.py and
tests/test_gpu_pinned_null_model.py (plain helper module, not a test): built here so that
tests/test_pinned_reference_cpu.py can hold every one of them to the condition the GPU tests rely on -- at the float64 oracle's own optimum, 32 x the oracle's error against the longdouble reference stays below the
1e-11 ceiling, so that the ceiling never sets a limit.  A cohort that fails that check is replaced here.  The null-model
cohorts (NULL_MODEL) are held to more: the oracle's own Brent search passes every check the device's is put to.

All cohorts stay at or below 320 cells: one longdouble evaluation of the reference is then well under a second.
"""
import numpy as np

from cellregmap_amd.synth import make_cohort
from oracle import crm as ocrm
from oracle.lmm import LMM
from oracle.sugar import economic_qs_linear

import pinned_reference as pr

# ---- effect sizes ---------------------------------------------------------------------------------------------------------
# name -> (donors, cells per donor, k0, columns of W, columns of E2 or None for mode A, variants, seed)
# packed width = cW + 2 k0 + 2; r_L = donors x columns of E2
EFFECTS = {
    "width 10, r_L 24": (8, 15, 3, 2, 3, 70, 3),              # 120 cells; 70 variants: two variant blocks
    "width 10, mode A": (8, 15, 3, 2, None, 4, 3),
    "width 66, r_L 40": (8, 22, 31, 2, 5, 3, 12),             # 176 cells; r_L above 32 and no multiple of it
    "width 130, r_L 10": (5, 31, 63, 2, 2, 3, 13),            # 155 cells; the last width of the batched form
    "k0 65, mode A": (10, 20, 65, 1, None, 2, 8),             # 200 cells; width 133: the per-SNP path serves it
}

# the (phenotype, variant) pairs the GPU tests name, per cohort -- the three phenotypes on variant 1 first; on the smallest
# cohort every phenotype also on the variants at the edges of the variant block and of the pair chunk.  The CPU suite
# holds the ceiling condition on each of them.  (Phenotype 2 carries the g o E0 effect of variant 1 alone.  With that
# effect at 3 x the noise, as this cohort first had it, the fit on any other variant puts the unexplained variance into
# v0 = 6.3 at rho <= 0.2 and the float64 oracle's own beta is off by up to 1.5e-12 there, 4.8 x what the ceiling leaves
# room for; at 1 x the noise -- rho* = 1 on variant 1 still -- it is 8e-14 at most, so the cohort was replaced.)
EFFECTS_HELD = {
    "width 10, r_L 24": [(0, 1), (1, 1), (2, 1), (1, 0), (1, 63), (1, 64), (1, 69), (2, 0), (2, 63), (2, 64), (2, 69),
                         (0, 0), (1, 2), (2, 2), (0, 2)],
    "width 10, mode A": [(0, 1), (1, 1), (2, 1)],
    "width 66, r_L 40": [(0, 1), (1, 1), (2, 1)],
    "width 130, r_L 10": [(0, 1), (1, 1), (2, 1)],
    "k0 65, mode A": [(1, 0), (2, 1)],
}


class EffectsCase:
    """Y holds three phenotypes: one driven by the L component (rho* = 0 on variant 1), a mixture (interior), one driven
    by g o E0 of variant 1 (rho* = 1)."""

    def __init__(self, name):
        donors, cells, k0, cW, e2, variants, seed = EFFECTS[name]
        co = make_cohort(donors, cells, k0, variants, seed=seed)
        rng = np.random.default_rng(seed + 500)
        n = co.y.size
        self.name, self.n, self.k0, self.cW = name, n, k0, cW
        self.W = np.column_stack([np.ones(n)] + [rng.normal(size=n) for _ in range(cW - 1)])
        self.E0, self.G, self.hK = co.E, co.G, co.hK
        self.maf = np.clip(np.minimum(co.G.mean(0) / 2, 1 - co.G.mean(0) / 2), 0.05, 0.5)
        self.E2 = None if e2 is None else (co.E if e2 == k0 else rng.normal(size=(n, e2)))
        self.half_L = None if e2 is None else np.concatenate(ocrm.khatri_rao_halves(co.hK, self.E2), axis=1)
        self.grid = [1.0] if e2 is None else list(ocrm.RHO_GRID)
        part_l = np.zeros(n) if e2 is None else (self.half_L @ rng.normal(size=self.half_L.shape[1])) / np.sqrt(e2)
        part_gxe = co.G[:, 1] * (co.E @ rng.normal(size=k0)) / np.sqrt(k0)
        noise = rng.normal(size=(n, 3))
        self.Y = np.column_stack([3.0 * part_l + noise[:, 0], 1.5 * part_l + 1.5 * part_gxe + noise[:, 1],
                                  (1.0 if k0 == 3 else 2.0) * part_gxe + noise[:, 2]])

    def operands(self, i, v):
        """(y, M, U) of the pair (phenotype i, variant v)."""
        g = self.G[:, [v]]
        return self.Y[:, i], np.concatenate((self.W, g, self.E0), axis=1), g * self.E0


def effects_records(cs, y, M, U, rho, v0, v1, got=None, norm=1.0):
    """(the reference's record, the float64 oracle's at the same point -- or that of ``got`` = (beta, u, lml, scale)):
    dicts with beta, u, beta_gxe = norm v0 rho E0 u, the restricted lml and the scale at delta = v1 / (v0 + v1)."""
    LD = pr.LD
    beta, u = pr.pinned_effects(y, M, U, cs.half_L, rho, v0, v1)
    _, _, lml, s = pr.pinned(y, M, pr.effects_half(U, cs.half_L, rho), np.zeros((y.size, 0)), LD(v1) / (LD(v0) + LD(v1)))
    ref = {"beta": beta, "u": u, "beta_gxe": (LD(norm) * LD(v0) * LD(rho)) * (np.asarray(cs.E0, LD) @ u), "lml": lml, "scale": s}
    b, uu, l, sc = pr.oracle_effects_at(y, M, U, cs.half_L, rho, v0, v1) if got is None else got
    return ref, {"beta": b, "u": uu, "beta_gxe": (v0 * rho) * (cs.E0 @ uu) * norm, "lml": l, "scale": sc}


def oracle_effects_point(y, M, U, half_L, grid):
    """(rho, v0, v1, lml) of the oracle's own fit: oracle/crm.py: predict_interaction's loop over the grid."""
    best = None
    for rho in grid:
        lmm = LMM(y, M, economic_qs_linear(pr.effects_half(U, half_L, rho), return_q1=False), restricted=True)
        lmm.fit(verbose=False)
        if best is None or lmm.lml() > best[3]:
            best = (float(rho), lmm.v0, lmm.v1, lmm.lml())
    return best


# ---- association ------------------------------------------------------------------------------------------------------------
# name -> (donors, cells per donor, contexts, covariate columns, mode, seed, what drives the phenotype)
# spectrum rank: contexts (mode A), contexts + donors at the interior grid points (mode B); past 256 contexts (the limit
# of E0) the background's contexts go in as E1 and E0 keeps the first three of them
ASSOCIATION = {
    "c 1, mode B": (10, 15, 3, 1, "B", 61, "mix"),                  # 150 cells, register null-fit kernel
    "c 9, mode B": (12, 15, 3, 9, "B", 62, "kinship"),              # 180 cells, LDS kernel at its first count
    "c 62, mode B": (12, 15, 3, 62, "B", 63, "contexts"),           # ... at its last
    "c 70, mode B": (12, 15, 3, 70, "B", 64, "mix"),                # 63..128 columns
    "c 128, mode A": (10, 20, 5, 128, "A", 65, "contexts"),         # 200 cells, CMAX
    "rank 260, mode A": (10, 30, 260, 2, "A", 66, "contexts"),      # 300 cells: past one 256-thread stride, no multiple
    "rank 260, mode B": (30, 10, 230, 3, "B", 67, "mix"),           # 300 cells, 230 + 30 at the interior points
}
DRIVE = {"kinship": (0.0, 3.0), "contexts": (6.0, 0.0), "mix": (2.0, 1.0)}


class AssociationCase:
    def __init__(self, name, variants=3):
        donors, cells, k, c, mode, seed, drive = ASSOCIATION[name]
        co = make_cohort(donors, cells, k, variants, seed=seed)
        rng = np.random.default_rng(seed + 500)
        n = co.y.size
        self.name, self.n, self.mode = name, n, mode
        self.E1, self.hK, self.donor_of_cell, self.donors = co.E, (co.hK if mode == "B" else None), co.donor_of_cell, donors
        self.E = co.E if k <= 256 else co.E[:, :3]
        self.W = np.column_stack([np.ones(n)] + [rng.normal(size=n) for _ in range(c - 1)])
        self.G = co.G + 0.05 * rng.normal(size=co.G.shape)
        self.grid = [1.0] if mode == "A" else list(ocrm.RHO_GRID)
        self.y = self.phenotype(rng, drive) + 0.3 * self.G[:, 0]

    def phenotype(self, rng, drive):
        a, b = DRIVE[drive]
        y = a * (self.E1 @ rng.normal(size=self.E1.shape[1])) / np.sqrt(self.E1.shape[1]) + rng.normal(size=self.n)
        if self.hK is not None:
            y = y + b * (self.hK @ rng.normal(size=self.hK.shape[1]))
        return y

    def half(self, rho):
        return pr.half_factor(rho, self.E1, hK=self.hK)


def oracle_null(y, W, half_of, grid):
    """(rho, the fitted LMM, (Q0, S0)) of the oracle's ML null model (oracle/crm.py: null_fit)."""
    best = None
    for rho in grid:
        (Q0,), S0 = economic_qs_linear(half_of(rho), return_q1=False)
        lmm = LMM(y, W, ((Q0,), S0), restricted=False)
        lmm.fit(verbose=False)
        if best is None or lmm.lml() > best[1].lml():
            best = (float(rho), lmm, (Q0, S0))
    return best


# ---- null fits of the interaction scan, every grid point ------------------------------------------------------------------
# name -> donors, cells per donor, contexts k0, covariate columns c, mode, seed, variants, and optionally
#   path: "dense" (default; the donor-constant genotypes get cell-level noise) or "collapsed" (kept donor-constant),
#   y: "cohort" (default; the simulator's phenotype), "noise" (no random effect at all) or "kinship" (a strong one),
#   ragged: unequal donor sizes (test_gpu_unrelated_donors._ragged; the unrelated-donor route of mode C asks for them),
#   per_wave: fits that the form under test packs into a wavefront (the last `variants mod per_wave` ones are held too)
# Mode B: hS = [sqrt(rho) E, sqrt(1 - rho) hK] with hK cells x donors, so the spectrum has `donors` entries at rho = 0, k0
# at rho = 1 and r = k0 + donors in between.  Mode C: k0 + donors x k0.  60 to 130 cells, except where 127 / 128 covariate
# columns need more cells than columns (160 and about 170).
NULL_MODEL = {
    # the register kernel, one fit per wavefront: the lane loop over a spectrum of 63, 64, 65 and of 5 entries
    "c 1, r 63, dense": dict(donors=10, cells=12, k0=53, c=1, mode="B", seed=101, variants=7),
    "c 1, r 63, collapsed": dict(donors=10, cells=12, k0=53, c=1, mode="B", seed=101, variants=7, path="collapsed"),
    "c 3, r 64, dense": dict(donors=10, cells=12, k0=54, c=3, mode="B", seed=102, variants=7),
    "c 3, r 64, collapsed": dict(donors=10, cells=12, k0=54, c=3, mode="B", seed=102, variants=7, path="collapsed"),
    "c 8, r 65, dense": dict(donors=10, cells=12, k0=55, c=8, mode="B", seed=103, variants=7),
    "c 8, r 65, collapsed": dict(donors=10, cells=12, k0=55, c=8, mode="B", seed=103, variants=7, path="collapsed"),
    "c 2, r 5": dict(donors=3, cells=30, k0=2, c=2, mode="B", seed=104, variants=7),
    # the LDS-shared queue form: one covariate column and 1027 variants (1024 at least; a last wavefront of three fits)
    "queue, r 16": dict(donors=6, cells=15, k0=10, c=1, mode="B", seed=105, variants=1027, per_wave=4),
    "queue, r 17": dict(donors=6, cells=15, k0=11, c=1, mode="B", seed=106, variants=1027, per_wave=4),
    # nullfit_wide.hip at its first and last covariate count, nullfit_xwide.hip at its first and last
    "c 9": dict(donors=10, cells=12, k0=4, c=9, mode="B", seed=107, variants=5),
    # (one longdouble evaluation costs 30 ms at 62 columns and 60 ms at 128, eight of them per trial: two variants, both
    # held, at 62 / 63 columns and one at 127 / 128 keep a case at a few seconds)
    "c 62": dict(donors=10, cells=13, k0=4, c=62, mode="B", seed=108, variants=2),
    "c 63": dict(donors=10, cells=13, k0=4, c=63, mode="B", seed=109, variants=2),
    "c 128": dict(donors=8, cells=20, k0=4, c=128, mode="B", seed=110, variants=1),
    "c 127, mode C": dict(donors=5, cells=40, k0=3, c=127, mode="C", seed=111, variants=1, ragged=True),
    "mode A, k0 17": dict(donors=8, cells=10, k0=17, c=2, mode="A", seed=112, variants=7),
    "mode C": dict(donors=5, cells=24, k0=3, c=1, mode="C", seed=113, variants=12, ragged=True),
    "no kinship term": dict(donors=9, cells=10, k0=4, c=1, mode="B", seed=114, variants=7, y="noise"),
    "strong kinship term": dict(donors=9, cells=10, k0=4, c=1, mode="B", seed=115, variants=7, y="kinship"),
    # as many spectrum entries as cells at the interior grid points (50 + 10 = 60): n - r = 0, the complement terms vanish
    "saturated": dict(donors=10, cells=6, k0=50, c=1, mode="B", seed=120, variants=7),
}


class NullModelCase:
    def __init__(self, name):
        spec = dict(path="dense", y="cohort", ragged=False, per_wave=1)
        spec.update(NULL_MODEL[name])
        donors, cells, k0, c, seed, variants = (spec[k] for k in ("donors", "cells", "k0", "c", "seed", "variants"))
        rng = np.random.default_rng(seed + 500)
        if spec["ragged"]:
            from test_gpu_unrelated_donors import _ragged

            co, keep, G = _ragged(donors, cells, k0, variants, seed)
            y, E, hK = co.y[keep], co.E[keep], co.hK[keep]
        else:
            co = make_cohort(donors, cells, k0, variants, seed=seed)
            y, E, hK = co.y, co.E, co.hK
            G = co.G if spec["path"] == "collapsed" else co.G + 0.05 * rng.normal(size=co.G.shape)
        n = y.size
        if spec["y"] == "noise":
            y = rng.normal(size=n)
        elif spec["y"] == "kinship":
            y = 3.0 * (hK @ rng.normal(size=hK.shape[1])) + 0.5 * rng.normal(size=n)
        self.name, self.n, self.c, self.mode, self.path, self.donors = name, n, c, spec["mode"], spec["path"], donors
        self.per_wave = spec["per_wave"]
        self.y, self.E, self.hK, self.G = y, E, hK, np.ascontiguousarray(G)
        self.W = np.column_stack([np.ones(n)] + [rng.normal(size=n) for _ in range(c - 1)])
        self.grid = [1.0] if self.mode == "A" else list(ocrm.RHO_GRID)
        self.Ls = ocrm.khatri_rao_halves(hK, E) if self.mode == "C" else None
        self._half, self._qs, self._gram, self._trial, self._logdet, self._at, self._fit = {}, {}, {}, {}, {}, {}, {}

    def picks(self):
        """The variants held: ``pinned_reference.pick``'s three, and for a form that packs ``per_wave`` fits into a
        wavefront the last ``variants mod per_wave`` ones."""
        p = self.G.shape[1]
        return sorted(set(pr.pick(p)) | set(range(p - p % self.per_wave, p)))

    def half(self, i):
        if i not in self._half:
            rho = float(self.grid[i])
            kw = {"A": {}, "B": {"hK": self.hK}, "C": {"Ls": self.Ls}}[self.mode]
            self._half[i] = pr.half_factor(rho, self.E, **kw)
        return self._half[i]

    def qs(self, i):
        if i not in self._qs:
            (Q0,), S0 = economic_qs_linear(self.half(i), return_q1=False)
            self._qs[i] = (Q0, S0)
        return self._qs[i]

    def gram(self, i):
        if i not in self._gram:
            hS = np.asarray(self.half(i), pr.LD)
            self._gram[i] = hS @ hS.T
        return self._gram[i]

    def X(self, j):
        return np.column_stack([self.W, self.G[:, j]])

    def logdet_XX(self, j):
        if j not in self._logdet:
            self._logdet[j] = pr.log_gram(self.X(j))
        return self._logdet[j]

    def oracle_fit(self, j, i):
        """Of variant j at grid point i, computed once: the float64 oracle's fit as the reference procedure leaves it (Brent
        alone: lml, delta, scale), and the x of the polished one."""
        if (j, i) not in self._fit:
            Q0, S0 = self.qs(i)
            lmm = LMM(self.y, self.X(j), ((Q0,), S0), restricted=True)
            lmm.fit(verbose=False)
            brent = (lmm.lml(), lmm.delta, lmm.scale)
            self._fit[(j, i)] = (brent, lmm._polish(lmm._x, -brent[0]))   # (what fit(polish=True) does after the same search)
        return self._fit[(j, i)]

    def trial(self, j, i):
        """(the oracle's Brent record, ``pinned_reference.null_trial_reference`` started from its polished fit), once."""
        if (j, i) not in self._trial:
            brent, x0 = self.oracle_fit(j, i)
            self._trial[(j, i)] = (brent, pr.null_trial_reference(self.y, self.X(j), None, x0, gram=self.gram(i)))
        return self._trial[(j, i)]

    def reference_lml(self, j, i, x):
        """The reference's restricted lml of variant j at grid point i and x = logit(delta)."""
        none = np.zeros((self.n, 0))
        return pr.pinned(self.y, self.X(j), None, none, pr._logistic(x), gram=self.gram(i), logdet_XX=self.logdet_XX(j))[2]

    def at(self, j, i, delta):
        """((lml, scale) of the reference, of the float64 oracle) of variant j at grid point i and ``delta``."""
        key = (j, i, float(delta))
        if key not in self._at:
            none = np.zeros((self.n, 0))
            ref = pr.pinned(self.y, self.X(j), None, none, delta, gram=self.gram(i), logdet_XX=self.logdet_XX(j))
            self._at[key] = ((ref[2], ref[3]), pr.oracle_null_at(self.y, self.X(j), *self.qs(i), delta))
        return self._at[key]


_null_model_cases = {}


def null_model_case(name):
    """One object per cohort and process: the references of its trials are computed once and shared."""
    if name not in _null_model_cases:
        _null_model_cases[name] = NullModelCase(name)
    return _null_model_cases[name]


def hold_trials(cs, records, variants):
    """Checks b, c and d of tests/test_gpu_pinned_null_model.py on ``records[j][i] = (lml, delta, scale, ...)`` for the
    variants given: (the limits, the float64 oracle's errors at the same points, {(j, i): shares of every bound}).  The
    limits are ``pinned_reference.limits`` of the oracle's own error at the same points, the largest over the trials held."""
    rows, ora = {}, []
    for j in variants:
        for i in range(len(cs.grid)):
            ref_at, own = cs.at(j, i, records[j][i][1])
            ora.append({"lml": pr.relative(own[0], ref_at[0]), "scale": pr.relative(own[1], ref_at[1])})
            rows[(j, i)] = ref_at
    ora = pr.worst(ora)
    lim = pr.limits(ora, cs.n)
    shares = {key: pr.trial_shares(records[key[0]][key[1]], ref_at, cs.trial(*key)[1], lim) for key, ref_at in rows.items()}
    return lim, ora, shares
