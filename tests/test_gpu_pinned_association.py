"""Association likelihood-ratio tests against the extended-precision reference at the point the device itself reports
(tests/pinned_reference.py: ``pinned_ml``, ``pinned_ml_max``).

tests/test_gpu_association*.py ask for p within 1e-5 p of the oracle's and for alt_lml within 1e-10 |null lml| of another
form of the library: two forms share their common errors -- every Gram entry of the fast scanner is
sw + (plain - s1) / delta, a cancellation both perform alike.  Here:

  * null model: ``null_lml`` and e2 + g2 + eps2 against ``pinned_ml(y, W, hS(rho1), null_delta)``; rho1 must be the
    reference's argmax over the grid unless its two best values are within the lml limit of each other; e2 / g2 / eps2
    against rho s (1 - delta), (1 - rho) s (1 - delta), s delta of the reference's s;
  * fast scanner: ``alt_lml`` against ``pinned_ml(y, [W, g], hS(rho1), null_delta)``, and the statistic
    2 (alt_lml - null_lml) against the reference's difference (absolute, relative to |null lml|);
  * refit scan (fast = 0): the device reports no alternative delta, so alt_lml is bounded from both sides by the
    reference's own maximum L* over x = logit(delta) (``pinned_ml_max``: x*, curvature):
        alt_lml <= L* + limit          L* - alt_lml <= limit + 1/2 curvature (3 (1e-6 |x*| + 1e-6))^2
    -- the allowance is what a search with rtol = atol = 1e-6 on x (brent_search.h) may leave of a likelihood of that
    curvature; tests/test_pinned_reference_cpu.py shows the oracle's own Brent result meets the same bound on these
    cohorts, whose optima have delta in (1e-3, 1 - 1e-3).  The shortfalls are printed and recorded;
  * p: ``erfc(sqrt(lrs / 2))`` of the device's own lrs = -2 null_lml + 2 alt_lml in mpmath, clipped as
    ``lrt_pvalues`` clips, to 1e-14 relative; a variant in the span of W: alt_lml is the reference's NULL value at
    null_delta and p is 1 - 2.220446049250313e-16; a planted effect with a statistic above 1500: p is
    2.2250738585072014e-308 exactly.

At most three variants per case (``pinned_reference.pick``).  Tolerance (``pinned_reference.limits``): per case and
quantity 32 x the float64 oracle's own error against the reference at the same points (``oracle_ml_at``: its LMM and
its FastScanner at the frozen delta), floor n x 2.2e-16, ceiling 1e-11; the ceiling never sets a limit (asserted).
"""
import json
import os

import numpy as np
import pytest

import pinned_cases as pc
import pinned_reference as pr

pytestmark = pytest.mark.gpu

RECORD = {}
LD = pr.LD
TINY, ONE_LESS = 2.2250738585072014e-308, 1 - 2.220446049250313e-16


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    """The per-case errors go beside the file $CRM_PINNED_JSON names, as <name>_association.json (tools/pinned_record.py
    merges them into profiles/pinned_effects_association_errors.json)."""
    yield
    dest = os.environ.get("CRM_PINNED_JSON")
    if dest and RECORD:
        with open(os.path.splitext(dest)[0] + "_association.json", "w") as fh:
            json.dump(RECORD, fh, indent=1, sort_keys=True)


_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = pc.AssociationCase(name)
    return _cases[name]


def _device(cs, y=None):
    import cellregmap_amd as crm

    kw = {} if cs.hK is None else {"hK": cs.hK}
    return crm.CellRegMap(cs.y if y is None else y, cs.E, W=cs.W, E1=cs.E1, **kw)


class _At:
    """The reference and the oracle at the null model a device scan reports: (rho1, null_delta)."""

    def __init__(self, cs, y, rho, delta):
        from oracle.sugar import economic_qs_linear

        self.cs, self.y, self.rho, self.delta = cs, np.asarray(y, float), float(rho), float(delta)
        hS = np.asarray(cs.half(self.rho), LD)
        self.gram = hS @ hS.T
        (self.Q0,), self.S0 = economic_qs_linear(cs.half(self.rho), return_q1=False)
        self.null = pr.pinned_ml(self.y, cs.W, None, self.delta, gram=self.gram)
        self.own_null = pr.oracle_ml_at(self.y, cs.W, self.Q0, self.S0, self.delta)

    def fast(self, g):
        """(reference alt lml, the oracle's) of one variant at the frozen delta."""
        ref = pr.pinned_ml(self.y, np.column_stack([self.cs.W, g]), None, self.delta, gram=self.gram)[0]
        return ref, pr.oracle_ml_at(self.y, self.cs.W, self.Q0, self.S0, self.delta, np.asarray(g, float).reshape(-1, 1))[2][0]

    def refit(self, g):
        """(L*, x*, curvature, the oracle's error at x*) of one variant."""
        from oracle.lmm import LMM

        X = np.column_stack([self.cs.W, g])
        o = LMM(self.y, X, ((self.Q0,), self.S0), restricted=False)
        o.fit(verbose=False)
        top, x, curvature = pr.pinned_ml_max(self.y, X, None, o._x, gram=self.gram)
        at = float(pr._logistic(x))
        own = pr.ml_errors({"lml": pr.oracle_ml_at(self.y, X, self.Q0, self.S0, at)[0]},
                           {"lml": pr.pinned_ml(self.y, X, None, at, gram=self.gram)[0]})
        return top, x, curvature, own


def _mp_pvalue(null_lml, alt_lml):
    """``lrt_pvalues`` of the device's own doubles with the tail in mpmath."""
    import mpmath as mp

    mp.mp.dps = 40
    lrs = max(-2 * null_lml + 2 * alt_lml, TINY)
    return min(max(float(mp.erfc(mp.sqrt(mp.mpf(lrs) / 2))), TINY), ONE_LESS)


def _finish(case, n, ora, dev, extra=None):
    lim = pr.limits(ora, n)
    fmt = lambda e: " ".join("%s %.2e" % kv for kv in sorted(e.items()))  # noqa: E731
    print("\n[pinned] %s: n %d\n[pinned]   oracle  %s\n[pinned]   limit   %s\n[pinned]   device  %s%s"
          % (case, n, fmt(ora), fmt(lim), fmt(dev), "" if extra is None else "\n[pinned]   %s" % extra))
    RECORD[case] = {"cells": n, "oracle": ora, "limit": lim, "device": dev}
    if extra is not None:
        RECORD[case]["refit"] = extra
    for k, v in ora.items():
        assert pr.PATHS * v <= pr.CEILING, (case, k, v)                  # the ceiling sets no limit
    for k, v in dev.items():
        assert v <= lim[k], (case, k, v, lim[k])
    return lim


def _union(rows):
    return {k: max(r[k] for r in rows if k in r) for k in ("lml", "scale", "lrs") if any(k in r for r in rows)}


def _hold_fast(case, cs, y, G, pv, info, st, sel=None, at=None):
    """Null model, alternatives and p of a fast scan of one phenotype; ``G``: the n x p matrix the panel stands for."""
    rho, delta, null_lml = float(info["rho1"][0]), float(st["null_delta"]), float(st["null_lml"])
    assert 0.0 <= rho <= 1.0 and 0.0 < delta < 1.0
    at = _At(cs, y, rho, delta) if at is None else at
    rl, rs = at.null
    total = float(info["e2"][0] + info["g2"][0] + info["eps2"][0])
    dev = [pr.ml_errors({"lml": null_lml, "scale": total}, {"lml": rl, "scale": rs})]
    ora = [pr.ml_errors({"lml": at.own_null[0], "scale": at.own_null[1]}, {"lml": rl, "scale": rs})]
    sel = pr.pick(G.shape[1]) if sel is None else sel
    for j in sel:
        ref, own = at.fast(G[:, j])
        dev.append(pr.ml_errors({"lml": st["alt_lml"][j], "lrs": (st["alt_lml"][j], null_lml)}, {"lml": ref, "lrs": (ref, rl)}))
        ora.append(pr.ml_errors({"lml": own, "lrs": (own, at.own_null[0])}, {"lml": ref, "lrs": (ref, rl)}))
        want = _mp_pvalue(null_lml, float(st["alt_lml"][j]))
        assert abs(pv[j] - want) <= 1e-14 * want, (case, j, pv[j], want)
    lim = _finish(case, cs.n, _union(ora), _union(dev))
    tol = float(lim["scale"] * rs)
    for key, want in (("e2", rho * rs * (1 - LD(delta))), ("g2", (1 - LD(rho)) * rs * (1 - LD(delta))), ("eps2", rs * LD(delta))):
        assert abs(float(LD(info[key][0]) - want)) <= tol, (case, key, info[key][0], float(want))
    return at, lim


def _hold_refit(case, cs, y, G, pv, info, st, sel=None, at=None):
    """alt_lml of a refitting scan between the two bounds around the reference's maximum."""
    rho, delta, null_lml = float(info["rho1"][0]), float(st["null_delta"]), float(st["null_lml"])
    at = _At(cs, y, rho, delta) if at is None else at
    rl, rs = at.null
    ora = [pr.ml_errors({"lml": at.own_null[0]}, {"lml": rl})]
    tops = []
    sel = pr.pick(G.shape[1]) if sel is None else sel
    for j in sel:
        top, x, curvature, own = at.refit(G[:, j])
        assert 1e-3 < float(pr._logistic(x)) < 1 - 1e-3, (case, j, float(x))
        ora.append(own)
        tops.append((j, top, x, curvature))
        want = _mp_pvalue(null_lml, float(st["alt_lml"][j]))
        assert abs(pv[j] - want) <= 1e-14 * want, (case, j, pv[j], want)
    ora = _union(ora)
    short = {int(j): float(top - LD(st["alt_lml"][j])) for j, top, _, _ in tops}
    allow = {int(j): pr.refit_allowance(x, c) for j, _, x, c in tops}
    lim = _finish(case, cs.n, ora, {"lml": pr.relative(null_lml, rl)},
                  extra={"short of L*": short, "allowance": allow})
    for j, top, x, curvature in tops:
        edge = lim["lml"] * abs(float(top))
        assert -short[int(j)] <= edge, (case, j, short[int(j)], edge)
        assert short[int(j)] <= edge + allow[int(j)], (case, j, short[int(j)], edge, allow[int(j)])


# ---- null models -------------------------------------------------------------------------------------------------------------------
SEEN_RHO = {}


@pytest.mark.parametrize("name", list(pc.ASSOCIATION))
def test_null_model_and_fast_scanner(name):
    """Covariate widths 1 (register kernel), 9 and 62 (LDS kernel, first and last), 70 and 128 (63 .. CMAX columns); spectrum
    ranks 13 .. 15 (below one 256-thread stride) and 260 (past one, no multiple); modes A and B; null fits that land on
    rho = 0, inside the grid and on 1 (checked by the last test of this group)."""
    cs = _case(name)
    pv, info, st = _device(cs).scan_association_fast(cs.G, return_stats=True)
    at, lim = _hold_fast("association fast, " + name, cs, cs.y, cs.G, pv, info, st)
    SEEN_RHO[name] = at.rho
    lmls = pr.grid_lmls(cs.y, cs.W, cs.half, cs.grid, restricted=False)
    best, tie = pr.argmax_or_tie(lmls, lim["lml"])
    print("[pinned]   rho1 %.1f, the reference's argmax %.1f%s" % (at.rho, cs.grid[best], ", tied" if tie else ""))
    assert tie or at.rho == cs.grid[best], (name, at.rho, cs.grid[best], [float(v) for v in lmls])


def test_null_models_land_on_both_ends_and_inside_the_grid():
    rhos = {}
    for name in pc.ASSOCIATION:
        cs = _case(name)
        if cs.mode == "B":
            rhos[name] = SEEN_RHO[name] if name in SEEN_RHO else _device(cs).scan_association_fast(cs.G[:, :1])[1]["rho1"][0]
    assert 0.0 in rhos.values() and 1.0 in rhos.values() and any(0.0 < r < 1.0 for r in rhos.values()), rhos


@pytest.mark.parametrize("name", list(pc.ASSOCIATION))
def test_refit_scan(name):
    cs = _case(name)
    pv, info, st = _device(cs).scan_association(cs.G, return_stats=True, progress=False)
    _hold_refit("association refit, " + name, cs, cs.y, cs.G, pv, info, st)


# ---- panels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("kind", ["dosages", "donors"])
def test_donor_level_panels(kind, fast):
    """``from_dosages`` (int8 allele counts, not standardised) and ``from_donors`` (float64 donor rows): the reference reads
    the expanded n x p matrix."""
    from cellregmap_amd import GenotypePanel

    cs = _case("c 9, mode B")
    rng = np.random.default_rng(11)
    if kind == "dosages":
        D = rng.integers(0, 3, size=(cs.donors, 5)).astype(np.int8)
        D[0], D[1], D[2] = 1, 0, 2                                   # (no monomorphic column)
        panel, G = GenotypePanel.from_dosages(D, cs.donor_of_cell, standardize=False), D[cs.donor_of_cell].astype(float)
    else:
        Gd = rng.normal(size=(cs.donors, 5))
        panel, G = GenotypePanel.from_donors(Gd, cs.donor_of_cell), Gd[cs.donor_of_cell]
    obj = _device(cs)
    case = "association %s, %s panel" % ("fast" if fast else "refit", kind)
    if fast:
        _hold_fast(case, cs, cs.y, G, *obj.scan_association_fast(panel, return_stats=True))
    else:
        _hold_refit(case, cs, cs.y, G, *obj.scan_association(panel, return_stats=True, progress=False))


# ---- several phenotypes in one pass ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
def test_three_phenotypes_in_one_pass_with_a_cis_window(fast):
    """``scan_association_many``: genes driven by the kinship, by the contexts and by both (at least two grid points), one of
    them on a cis window with a repeat; every row at the limit of its own null model."""
    from cellregmap_amd import CellRegMap, scan_association_many

    cs = pc.AssociationCase("c 1, mode B", variants=8)
    rng = np.random.default_rng(5)
    Y = np.column_stack([cs.phenotype(rng, d) + 0.3 * cs.G[:, i] for i, d in enumerate(("kinship", "contexts", "mix"))])
    assert cs.E1 is cs.E
    first = CellRegMap(Y[:, 0], cs.E, W=cs.W, hK=cs.hK)
    crms = [first] + [CellRegMap(Y[:, i], cs.E, W=cs.W, hK=cs.hK, background=first._bg) for i in (1, 2)]
    cis = [(0, 8), np.array([5, 1, 1]), slice(2, 7)]
    cols = [np.arange(8), np.array([5, 1, 1]), np.arange(2, 7)]
    pv, info = scan_association_many(crms, cs.G, cis_index=cis, fast=fast, return_stats=True)
    assert np.unique(info["rho1"]).size >= 2, info["rho1"]
    for i in range(3):
        one = {k: info[k][[i]] for k in ("rho1", "e2", "g2", "eps2")}
        st = {"null_lml": info["null_lml"][i], "null_delta": info["null_delta"][i], "alt_lml": info["alt_lml"][i]}
        G = cs.G[:, cols[i]]
        assert pv[i].shape == st["alt_lml"].shape == (cols[i].size,)
        if i == 1:
            assert pv[i][1] == pv[i][2] and st["alt_lml"][1] == st["alt_lml"][2]
        case = "association %s, three phenotypes, phenotype %d" % ("fast" if fast else "refit", i)
        (_hold_fast if fast else _hold_refit)(case, cs, Y[:, i], G, pv[i], one, st)


# ---- the ends of the p-value --------------------------------------------------------------------------------------------------------------
def test_a_variant_in_the_span_of_w_and_a_planted_effect():
    """Variant 1 = W b: the alternative model is the null model, alt_lml is the reference's null value at null_delta and p
    is 1 - eps.  Variant 2 carries 40 000 x its column in y: the statistic passes 1500, where erfc underflows and
    ``lrt_pvalues`` clips to the smallest normal double.  (Its alt_lml is the logarithm of a residual 1e-9 of y'y: the float64
    oracle itself is 1.6e-7 off there, so that one number is held through p and the statistic's size only; the null model of
    this phenotype and variant 0 are held as everywhere.)"""
    cs = _case("c 9, mode B")
    G = cs.G.copy()
    G[:, 1] = cs.W @ np.linspace(-1.0, 2.0, cs.W.shape[1])
    y = cs.y + 4e4 * G[:, 2]
    pv, info, st = _device(cs, y).scan_association_fast(G, return_stats=True)
    at, lim = _hold_fast("association fast, span of W and planted effect", cs, y, G, pv, info, st, sel=[0])
    rl = at.null[0]
    gap = pr.relative(st["alt_lml"][1], rl)
    print("[pinned]   variant in the span of W: alt_lml against the reference's null value %.2e (limit %.2e)" % (gap, lim["lml"]))
    assert gap <= lim["lml"], (gap, lim["lml"])
    assert pv[1] == ONE_LESS, pv[1]
    ref2 = at.fast(G[:, 2])[0]
    assert float(2 * (ref2 - rl)) > 1500 and 2 * (st["alt_lml"][2] - st["null_lml"]) > 1500
    assert pv[2] == TINY, pv[2]
