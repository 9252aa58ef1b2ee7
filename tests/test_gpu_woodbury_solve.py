"""The capacitance solve of the unrelated-donor route in its Y'Y form (assemble.hip: woodbury_yty_kernel, form
``woodbury_ytY`` = 1, the default) against the factor-and-two-substitutions kernel it replaces (``woodbury_ytY`` = 0).

M_uE C^-1 M_Ev = Y'Y with Y = L^-1 M_E., C = L L': the factor and the forward substitution are one right-looking sweep
over the augmented matrix [C ; M_.E], the product a Gram on the matrix pipe, formed over u <= v and mirrored.  Small
unrelated-donor cohorts (``kin_diag`` = 2 forces the route) put the kernel's index arithmetic through an odd k1, the
route's limit k1 = 64, and k1 = 50 with one and with five covariate columns (KT = 53 and 57).  Every shape is scanned
with three phenotypes -- one of donor-specific context effects (rho* = 0: the copy path), one with a planted large E E'
component (rho* > 0: the correction proper), one with its cells permuted (tests without a kinship term:
``sorted_pos`` < 0, the X rows of the correction are zero) -- and the test asserts that rho* = 0 (the copy path),
rho* > 0 and tests without a pair all occur.

Checks, per shape:

  1. form 1 against form 0: rho*, lml and delta bit for bit (the null fits do not pass through this kernel); Q and F
     within 1e-9 of their scale and p within 1e-7 relative -- the project's standing bound between two forms of one
     computation (``_close`` of test_gpu_unrelated_donors);
  2. Q and F at the device's reported (rho*, delta) against the longdouble reference of tests/pinned_reference.py, at
     that file's own limit rule (32 x the float64 oracle's error, floor n x 2.2e-16, ceiling 1e-11): ``_hold`` of
     test_gpu_pinned.py, on variants of the kind each phenotype is there for (asserted);
  3. the returned F is exactly symmetric.
"""
import numpy as np
import pytest

from test_gpu_gram_wide import _covariates, _flat_phenotype, _without_pair
from test_gpu_pinned import Problem, _hold, _kinship
from test_gpu_unrelated_donors import _blocks, _ragged

pytestmark = pytest.mark.gpu


def _phenotypes(co, keep, donors, cells, seed):
    """(name, y): a phenotype of donor-specific context effects E b_d that sum to zero over the donors (no shared E E'
    component: rho* = 0), one dominated by a shared context effect E b (rho* > 0), and the cohort's own with its cells
    permuted (no random effect left: tests without a kinship term)."""
    rng = np.random.default_rng(seed)
    y, E = co.y[keep], co.E[keep]
    donor = np.repeat(np.arange(donors), cells)[keep]
    b = rng.normal(size=(donors, E.shape[1]))
    own = np.einsum("ij,ij->i", E, (b - b.mean(axis=0))[donor])
    shared = E @ rng.normal(size=E.shape[1])
    out = []
    for name, effect in (("donor-specific", own), ("planted", shared)):
        v = 3.0 * effect / effect.std() + rng.normal(size=y.size)
        out.append((name, (v - v.mean()) / v.std()))
    # (whether a permuted phenotype's fits end at the upper clamp of delta is the permutation's affair: the test takes the
    # first of these four that leaves some test without a kinship term)
    return out + [("permuted", [_flat_phenotype(y, seed + i) for i in range(4)])]


SHAPES = [
    (8, 60, 13, 1, 32, 14),        # k1 odd
    (4, 150, 64, 1, 24, 65),       # k1 = 64, the route's limit: 64 + 3 + 64 = 131 Gram rows
    (5, 120, 50, 1, 24, 55),       # the large configurations' k1 = 50, KT = 53
    (5, 120, 50, 5, 24, 55),       # ... KT = 57
]   # (the route needs more cells than k1 + donors x k1 columns: the wide shapes take fewer, larger donors)


@pytest.mark.parametrize("donors,cells,k0,c,variants,seed", SHAPES)
def test_the_ytY_form_of_the_capacitance_solve(donors, cells, k0, c, variants, seed, kernel_form):
    import cellregmap_amd as crm
    from oracle import crm as ocrm

    co, keep, G = _ragged(donors, cells, k0, variants, 300 + seed)
    E, hK = co.E[keep], co.hK[keep]
    W = _covariates(E.shape[0], c, k0 + c)
    seen_zero = seen_positive = seen_none = 0
    for name, ys in _phenotypes(co, keep, donors, cells, 11 + seed):
        res = {}
        with _kinship(kernel_form, route=2, diag=2):
            panel = crm.GenotypePanel(G, groups=None)
            if name == "permuted":
                for y in ys:
                    obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
                    none_before = _without_pair()
                    obj.scan_interaction(panel)
                    if _without_pair() > none_before:
                        break
            else:
                y = ys
                obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
            assert 0.0 in obj._bg.rho                            # the grid contains rho = 0
            for form in (0, 1):
                kernel_form("woodbury_ytY", form)
                before, none_before = _blocks(), _without_pair()
                res[form] = obj.scan_interaction(panel, return_stats=True)
                assert _blocks() > before                        # the unrelated-donor route served
                none = _without_pair() - none_before
        (pv0, info0, st0), (pv, info, st) = res[0], res[1]
        rho = info["rho1"]
        print("\n[woodbury] k1 %d c %d %s: rho* = 0 at %d, > 0 at %d of %d variants, %d tests without a pair"
              % (k0, c, name, int(np.sum(rho == 0.0)), int(np.sum(rho > 0.0)), variants, none))
        seen_none += none
        # (a test without a pair reports a rho* too: only tests with a kinship term count for the two paths of the kernel)
        with_term = (info["e2"] + info["g2"]) > 1e-6 * info["eps2"]
        seen_zero += int(np.sum(with_term & (rho == 0.0)))
        seen_positive += int(np.sum(with_term & (rho > 0.0)))
        # 1. form against form
        for k in ("rho1", "e2", "g2", "eps2"):
            assert np.array_equal(info[k], info0[k]), (name, k)
        for k in ("lml", "delta", "scale"):
            assert np.array_equal(st[k], st0[k]), (name, k)
        scale = np.maximum(np.abs(st0["Q"]), np.trace(st0["F"], axis1=1, axis2=2))
        fs = np.abs(st0["F"]).max(axis=(1, 2), keepdims=True)
        dq, df = np.abs(st["Q"] - st0["Q"]) / scale, np.abs(st["F"] - st0["F"]) / fs
        dp = np.abs(pv - pv0) / pv0
        print("[woodbury]   form 1 against form 0: max dQ / scale %.3g, max dF / max|F| %.3g, max dp / p %.3g"
              % (dq.max(), df.max(), dp.max()))
        assert np.all(np.isfinite(st["Q"])) and np.all(np.isfinite(st["F"]))
        assert np.all(dq <= 1e-9) and np.all(df <= 1e-9) and np.all(dp <= 1e-7), name
        # 2. against the longdouble reference at the device's own (rho*, delta), on variants of the kind the phenotype is
        # there for: the correction proper (the first and the last with rho* > 0), the copy path, a test without a pair
        # (the one with the smallest kinship variance: where any test has none, that one has)
        if name == "planted":
            kind = np.flatnonzero(with_term & (rho > 0.0))
            assert kind.size > 0, name
            sel = sorted({int(kind[0]), int(kind[-1])})
        elif name == "donor-specific":
            kind = np.flatnonzero(with_term & (rho == 0.0))
            sel = [int(kind[kind.size // 2])] if kind.size else [variants // 2]
        else:
            assert none > 0, name
            sel = [int(np.argmin((info["e2"] + info["g2"]) / info["eps2"]))]
            assert not with_term[sel[0]]
        _hold("woodbury k1 %d c %d %s" % (k0, c, name), Problem(y, W, E, G, Ls=ocrm.khatri_rao_halves(hK, E)),
              [("ytY", res[1]), ("substitutions", res[0])], sel=sel)
    assert seen_zero > 0 and seen_positive > 0 and seen_none > 0, (seen_zero, seen_positive, seen_none)


def test_the_returned_F_is_exactly_symmetric(kernel_form):
    """Check 3, on the planted phenotype of every shape.  The correction Y'Y is symmetric by construction and the kernel
    mirrors what it writes; F is not the Gram alone, though: finalize_kernel subtracts D'K^-1X (X'K^-1X)^-1 X'K^-1D as
    dkx(j, .) . sol(j', .), which rounds differently for (j, j') and (j', j) -- 4e-17 to 9e-17 of max|F| with
    ``woodbury_ytY`` = 0, whose results stay what they were.  Behind the Y'Y form it takes both entries from the same
    operands in the same order."""
    import cellregmap_amd as crm

    worst = []
    for donors, cells, k0, c, variants, seed in SHAPES:
        co, keep, G = _ragged(donors, cells, k0, variants, 300 + seed)
        E, hK = co.E[keep], co.hK[keep]
        W = _covariates(E.shape[0], c, k0 + c)
        name, y = _phenotypes(co, keep, donors, cells, 11 + seed)[1]
        assert name == "planted"
        with _kinship(kernel_form, route=2, diag=2):
            obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
            panel = crm.GenotypePanel(G, groups=None)
            F = {}
            for form in (0, 1):
                kernel_form("woodbury_ytY", form)
                F[form] = obj.scan_interaction(panel, return_stats=True)[2]["F"]
        asym = [np.abs(F[f] - F[f].transpose(0, 2, 1)).max() / np.abs(F[f]).max() for f in (0, 1)]
        print("\n[woodbury] k1 %d c %d: max |F - F'| / max|F| %.3g (form 0: %.3g)" % (k0, c, asym[1], asym[0]))
        worst.append(asym[1])
    assert max(worst) == 0.0, worst
