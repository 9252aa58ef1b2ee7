"""Effect sizes against the extended-precision reference at the point the device itself reports
(tests/pinned_reference.py: ``pinned_effects``, ``pinned``).

tests/test_gpu_effects.py and tests/test_gpu_effects_many.py compare two searches (2 x |oracle - oracle polished| + 3e-6 of
the scale; 1e-7 at best): a Woodbury term wrong in the eighth digit passes them.  Here the search is not on the path of
the comparison.  ``predict_interaction_many(..., return_info=True)`` and ``CellRegMap._last_fit`` report (rho1, v0, v1),
and at that point beta, u = U'K^-1 (y - M beta), beta_gxe, the restricted lml and the scale v0 + v1 are closed forms of the
inputs, evaluated in longdouble from the dense K = v0 (rho U U' + (1 - rho) L L') + v1 I.

Held per pair: all of beta (``crm_effects_multi`` called directly as the wrapper calls it -- the wrapper keeps beta_g
only -- and bit for bit what the wrapper delivers), u, the delivered beta_gxe, lml and v0 + v1 (the reference's at
delta = v1 / (v0 + v1)).  The per-SNP path delivers beta_g, beta_gxe and, through ``predict_interaction_many``'s fallback,
u: those are held.  rho1 must be the reference's argmax over the grid unless its two best grid values are within the lml
limit of each other (``pinned_reference.grid_lmls``).

Tolerance (``pinned_reference.limits``): per case and quantity 32 x the float64 oracle's own error against the reference
at the same points (``oracle_effects_at``), floor n x 2.2e-16, ceiling 1e-11 -- and the ceiling never sets a limit: asserted
here at the device's points, and on the CPU at the oracle's (tests/test_pinned_reference_cpu.py) for the cohorts of
tests/pinned_cases.py.  Vectors are relative to the largest magnitude of the reference vector; a beta_gxe whose reference
is zero throughout (rho1 = 0) is met by zeros only.

Left out: a rank-deficient M = [W, g, E0].  The device takes the minimum-norm solution through the SVD basis and the
reference raises; tests/test_gpu_effects.py::test_collinear_contexts_go_through_the_svd_basis keeps that case.
"""
import json
import os

import numpy as np
import pytest

import pinned_cases as pc
import pinned_reference as pr

pytestmark = pytest.mark.gpu

RECORD = {}
KEYS = ("beta", "u", "beta_gxe", "lml", "scale")


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    """The per-case errors go beside the file $CRM_PINNED_JSON names, as <name>_effects.json (tools/pinned_record.py merges
    them into profiles/pinned_effects_association_errors.json)."""
    yield
    dest = os.environ.get("CRM_PINNED_JSON")
    if dest and RECORD:
        with open(os.path.splitext(dest)[0] + "_effects.json", "w") as fh:
            json.dump(RECORD, fh, indent=1, sort_keys=True)


_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = pc.EffectsCase(name)
    return _cases[name]


def _many(cs, pairs):
    """(beta_g, beta_gxe, info) of the wrapper on the pairs, and (fit, beta, u) of crm_effects_multi called with the
    same operands (None where the cohort is past the batched form)."""
    import cellregmap_amd as crm
    from cellregmap_amd import _engine, _lib

    pairs = np.asarray(pairs)
    hK = None if cs.E2 is None else cs.hK
    bg_, bgxe, info = crm.estimate_betas_many(cs.Y, cs.W, cs.E0, cs.G, maf=cs.maf, E2=cs.E2, hK=hK, pairs=pairs,
                                              return_info=True)
    if cs.cW + 2 * cs.k0 + 2 > 130:
        return bg_, bgxe, info, None
    lib, ctx = _lib.load(), _engine._context(0)
    bg = None
    if hK is not None:
        bg = _engine._make_background(np.zeros((cs.n, 1)), crm.get_L_values(hK, cs.E2), [0.0], 0)
    Y, W, E0, G = (_lib.f64(a) for a in (cs.Y, cs.W, cs.E0, cs.G))
    sub = np.ascontiguousarray(pairs, dtype=np.int32)
    grid = _lib.f64(np.asarray(cs.grid, float))
    fit, beta, u = np.empty((len(sub), 6)), np.empty((len(sub), cs.cW + 1 + cs.k0)), np.empty((len(sub), cs.k0))
    _lib.check(lib.crm_effects_multi(ctx, None if bg is None else bg.handle, cs.n, _lib.ptr(W), cs.cW, _lib.ptr(E0), cs.k0,
                                     _lib.ptr(Y), Y.shape[1], _lib.ptr(G), G.shape[1], _lib.ptr(sub), len(sub),
                                     grid.shape[0], _lib.ptr(grid), _lib.ptr(fit), _lib.ptr(beta), _lib.ptr(u)))
    # the wrapper delivers these numbers
    assert np.all(info["route"] == "woodbury")
    assert np.array_equal(fit[:, 0], info["rho1"]) and np.array_equal(fit[:, 1], info["v0"])
    assert np.array_equal(fit[:, 2], info["v1"]) and np.array_equal(fit[:, 3], info["lml"])
    assert np.array_equal(u, info["u"]) and np.array_equal(beta[:, cs.cW], bg_)
    return bg_, bgxe, info, beta


def _hold(case, cs, rows):
    """``rows``: [(label, (y, M, U), (rho, v0, v1), norm, device record)] -- the record holds some of KEYS; a scalar under
    "beta" is beta_g.  Asserts every entry against the reference within the limit and records the errors."""
    dev, ora = [], []
    for label, (y, M, U), (rho, v0, v1), norm, got in rows:
        assert 0.0 <= rho <= 1.0 and v0 >= 0.0 and v1 > 0.0, (case, label, rho, v0, v1)
        ref, own = pc.effects_records(cs, y, M, U, rho, v0, v1, norm=norm)
        if np.ndim(got.get("beta", ())) == 0 and "beta" in got:          # beta_g alone, in the units of all of beta
            top = np.abs(ref["beta"]).max()
            err = pr.effects_errors({k: v for k, v in got.items() if k != "beta"}, ref)
            err["beta"] = float(abs(pr.LD(got["beta"]) - ref["beta"][cs.cW]) / top)
        else:
            err = pr.effects_errors(got, ref)
        dev.append(err)
        ora.append(pr.effects_errors(own, ref))
    ora = pr.worst(ora)
    lim = pr.limits(ora, cs.n)
    worst = {k: max(e[k] for e in dev if k in e) for k in KEYS if any(k in e for e in dev)}
    fmt = lambda e: " ".join("%s %.2e" % (k, e[k]) for k in KEYS if k in e)  # noqa: E731
    print("\n[pinned] %s: n %d, %s\n[pinned]   oracle  %s\n[pinned]   limit   %s\n[pinned]   device  %s"
          % (case, cs.n, [r[0] for r in rows], fmt(ora), fmt(lim), fmt(worst)))
    RECORD[case] = {"cells": cs.n, "pairs": [r[0] for r in rows], "oracle": ora, "limit": lim, "device": worst}
    for k, v in ora.items():
        assert pr.PATHS * v <= pr.CEILING, (case, k, v)                  # the ceiling sets no limit
    for (label, *_), err in zip(rows, dev):
        for k, v in err.items():
            assert v <= lim[k], (case, label, k, v, lim[k])


def _rows_of_many(cs, pairs, sel, out):
    bg_, bgxe, info, beta = out
    rows = []
    for t in sel:
        i, v = (int(x) for x in pairs[t])
        assert (i, v) in pc.EFFECTS_HELD[cs.name]          # (the CPU suite holds the ceiling condition on these)
        got = {"beta": bg_[t] if beta is None else beta[t], "u": info["u"][t], "beta_gxe": bgxe[0, :, t],
               "lml": info["lml"][t], "scale": info["v0"][t] + info["v1"][t]}
        rows.append(("pair %d = (%d, %d)" % (t, i, v), cs.operands(i, v), (info["rho1"][t], info["v0"][t], info["v1"][t]),
                     1 / np.sqrt(2 * cs.maf[v] * (1 - cs.maf[v])), got))
    return rows


# ---- the batched form: widths, modes, the three ends of rho ------------------------------------------------------------------------
THREE = np.array([[0, 1], [1, 1], [2, 1]])


@pytest.mark.parametrize("name", ["width 10, r_L 24", "width 10, mode A", "width 66, r_L 40", "width 130, r_L 10"])
def test_batched_form(name):
    """Packed widths 10 (tiles of 2), 66 (tiles of 6) and exactly 130 (tiles of 9; k0 = 63, cW = 2); r_L of 24 and 10 (below
    one staging step of 32), 40 (past one, no multiple) and none (mode A: no rotations read); 120, 176 and 155 cells (no
    multiples of 32).  On the smallest cohort with kinship the three phenotypes end at rho1 = 0, inside the grid and at 1:
    the degenerate ends of the Woodbury form (no core at rho = 0, a = 0 at rho = 1)."""
    cs = _case(name)
    assert cs.n % 32 and cs.cW + 2 * cs.k0 + 2 == int(name.split(",")[0].split()[1])
    out = _many(cs, THREE)
    rho1 = out[2]["rho1"]
    if name == "width 10, r_L 24":
        assert rho1[0] == 0.0 and 0.0 < rho1[1] < 1.0 and rho1[2] == 1.0, rho1
    if cs.E2 is None:
        assert np.all(rho1 == 1.0)
    _hold("effects, " + name, cs, _rows_of_many(cs, THREE, range(3), out))


@pytest.mark.parametrize("i", [0, 1, 2])
@pytest.mark.parametrize("name", ["width 10, r_L 24", "width 66, r_L 40", "width 130, r_L 10"])
def test_rho1_is_the_references_argmax(name, i):
    cs = _case(name)
    pairs = np.array([[i, 1]])
    info = _many(cs, pairs)[2]
    y, M, U = cs.operands(i, 1)
    rho, v0, v1 = info["rho1"][0], info["v0"][0], info["v1"][0]
    ref, own = pc.effects_records(cs, y, M, U, rho, v0, v1)
    lim = pr.limits(pr.effects_errors(own, ref), cs.n)["lml"]
    lmls = pr.grid_lmls(y, M, lambda r: pr.effects_half(U, cs.half_L, r), cs.grid, restricted=True)
    best, tie = pr.argmax_or_tie(lmls, lim)
    print("\n[pinned] %s phenotype %d: rho1 %.1f, the reference's argmax %.1f%s" % (name, i, rho, cs.grid[best], ", tied" if tie else ""))
    assert tie or rho == cs.grid[best], (name, i, rho, cs.grid[best], [float(v) for v in lmls])


# ---- variant blocks and pair chunks ---------------------------------------------------------------------------------------------------
def test_seventy_variants_cross_the_variant_block():
    """VARIANT_BLOCK = 64 distinct variants per rotation block: pairs on variants 0, 63 (the last of the first block), 64 (the
    first of the second) and 69, of the phenotype with both components and of the one that carries g o E0 of variant 1."""
    cs = _case("width 10, r_L 24")
    assert cs.G.shape[1] == 70
    pairs = np.column_stack([np.repeat([1, 2], 70), np.tile(np.arange(70), 2)])
    out = _many(cs, pairs)
    _hold("effects, 70 variants", cs, _rows_of_many(cs, pairs, [0, 63, 64, 69, 70, 133, 134, 139], out))


def test_two_thousand_and_fifty_pairs_cross_the_pair_chunk():
    """PAIR_CHUNK = 2048 pairs per launch: 2050 pairs on three variants (one variant block; the pairs in variant order, so
    the launches split where the list does), nine distinct ones.  Pairs 0, 2047, 2048 and 2049 against the reference;
    every repeat bit for bit its first occurrence."""
    cs = _case("width 10, r_L 24")
    var = np.repeat([0, 1, 2], [700, 700, 650])
    pairs = np.column_stack([np.arange(2050) % 3, var])
    bg_, bgxe, info, beta = out = _many(cs, pairs)
    first = {}
    for t, key in enumerate(map(tuple, pairs)):
        f = first.setdefault(key, t)
        if f != t:
            assert bg_[t] == bg_[f] and np.array_equal(beta[t], beta[f]) and np.array_equal(info["u"][t], info["u"][f])
            assert np.array_equal(bgxe[0, :, t], bgxe[0, :, f])
            assert all(info[k][t] == info[k][f] for k in ("rho1", "v0", "v1", "lml")), (t, f)
    assert len(first) == 9
    _hold("effects, 2050 pairs", cs, _rows_of_many(cs, pairs, [0, 2047, 2048, 2049], out))


# ---- the per-SNP path -----------------------------------------------------------------------------------------------------------------
def test_per_snp_path_one_column_at_a_time():
    """``CellRegMap.predict_interaction`` (crm_lmm_fit on the per-SNP decompositions, crm_cov_solve): beta_g, the delivered
    beta_gxe, and lml and v0 + v1 of ``_last_fit``; one phenotype per end of rho."""
    import cellregmap_amd as crm

    cs = _case("width 10, r_L 24")
    Ls = crm.get_L_values(cs.hK, cs.E2)
    rows, rhos = [], []
    for i in range(3):
        obj = crm.CellRegMap(cs.Y[:, i], cs.E0, W=cs.W, Ls=Ls)
        bg_, bgxe = obj.predict_interaction(cs.G[:, [1]], cs.maf[[1]])
        rho, v0, v1, lml = obj._last_fit[:4]
        rhos.append(rho)
        rows.append(("phenotype %d, variant 1" % i, cs.operands(i, 1), (rho, v0, v1), 1 / np.sqrt(2 * cs.maf[1] * (1 - cs.maf[1])),
                     {"beta": bg_[0], "beta_gxe": bgxe[0, :, 0], "lml": lml, "scale": v0 + v1}))
    assert rhos[0] == 0.0 and 0.0 < rhos[1] < 1.0 and rhos[2] == 1.0, rhos
    _hold("effects, per-SNP path", cs, rows)


def test_per_snp_fallback_at_sixty_five_contexts():
    """k0 = 65 in mode A: cW + 2 k0 + 2 = 133 > 130, so ``predict_interaction_many`` hands the pairs to the per-SNP path and
    reports its u."""
    cs = _case("k0 65, mode A")
    pairs = np.array([[1, 0], [2, 1]])
    out = _many(cs, pairs)
    assert np.all(out[2]["route"] == "per_snp")
    _hold("effects, per-SNP fallback k0 65", cs, _rows_of_many(cs, pairs, range(2), out))


def test_estimate_aggregate_environment():
    """The fit runs under the object's own background (E1 in place of g o E0; a distinct E1 keeps rho identifiable, and the
    phenotype carries a random effect of E1 so that rho1 > 0 and the result is not zero), the solve under the per-SNP halves
    at the same (rho, v0, v1): beta from the first covariance, u from the second."""
    import cellregmap_amd as crm

    cs = _case("width 10, r_L 24")
    LD = pr.LD
    rng = np.random.default_rng(2)
    E1 = rng.standard_normal((cs.n, 4))
    yy = cs.Y[:, 1] + (E1 @ rng.standard_normal(4)) / 2
    obj = crm.CellRegMap(yy, cs.E0, W=cs.W, Ls=crm.get_L_values(cs.hK, cs.E2), E1=E1)
    dev, ora, rows = [], [], []
    for v in (0, 2):
        got = obj.estimate_aggregate_environment(cs.G[:, v])
        rho, v0, v1, lml = obj._last_fit[:4]
        assert rho > 0.0 and np.abs(got).max() > 0.0, (v, rho)
        _, M, U = cs.operands(1, v)
        y = yy
        beta, _ = pr.pinned_effects(y, M, E1, cs.half_L, rho, v0, v1)
        _, u = pr.pinned_effects(y, M, U, cs.half_L, rho, v0, v1, beta=beta)
        _, _, rlml, s = pr.pinned(y, M, pr.effects_half(E1, cs.half_L, rho), np.zeros((cs.n, 0)), LD(v1) / (LD(v0) + LD(v1)))
        ref = {"beta_gxe": (LD(rho) * LD(v0)) * (np.asarray(cs.E0, LD) @ u), "lml": rlml, "scale": s}
        ob, _, olml, os_ = pr.oracle_effects_at(y, M, E1, cs.half_L, rho, v0, v1)
        _, ou, _, _ = pr.oracle_effects_at(y, M, U, cs.half_L, rho, v0, v1, beta=ob)
        ora.append(pr.effects_errors({"beta_gxe": (rho * v0) * (cs.E0 @ ou), "lml": olml, "scale": os_}, ref))
        dev.append(pr.effects_errors({"beta_gxe": got, "lml": lml, "scale": v0 + v1}, ref))
        rows.append("variant %d" % v)
    ora, dev = pr.worst(ora), pr.worst(dev)
    lim = pr.limits(ora, cs.n)
    print("\n[pinned] aggregate environment: oracle %s\n[pinned]   limit %s\n[pinned]   device %s" % (ora, lim, dev))
    RECORD["effects, aggregate environment"] = {"cells": cs.n, "pairs": rows, "oracle": ora, "limit": lim, "device": dev}
    for k in lim:
        assert pr.PATHS * ora[k] <= pr.CEILING and dev[k] <= lim[k], (k, dev[k], lim[k])


def test_cov_solve_against_the_longdouble_solve():
    """crm_cov_solve: (v0 Q0 S0 Q0' + v1 I) x = rhs at the first grid point (rho = 0: the context part has no weight), an
    interior one and the last, against the Cholesky solve of the dense v0 hS hS' + v1 I in longdouble."""
    import cellregmap_amd as crm
    from oracle.scoretest import LowRankCov, cov_solve
    from oracle.sugar import economic_qs_linear

    cs = _case("width 10, r_L 24")
    obj = crm.CellRegMap(cs.Y[:, 1], cs.E0, W=cs.W, Ls=crm.get_L_values(cs.hK, cs.E2))
    rhs = np.random.default_rng(0).standard_normal((cs.n, 3))
    v0, v1 = 0.7, 0.4
    dev, ora = [], []
    for ri in (0, 5, 10):
        rho = float(cs.grid[ri])
        hS = pr.effects_half(cs.E0, cs.half_L, rho)
        ref = pr.pinned_solve(hS, v0, v1, rhs)
        (Q0,), S0 = economic_qs_linear(hS, return_q1=False)
        ora.append({"x": pr.vector_error(cov_solve(LowRankCov(Q0, S0, v0, v1), rhs), ref)})
        dev.append({"x": pr.vector_error(obj._cov_solve(obj._bg, ri, v0, v1, rhs), ref)})
    ora, dev = pr.worst(ora), pr.worst(dev)
    lim = pr.limits(ora, cs.n)
    print("\n[pinned] cov_solve: oracle %s, limit %s, device %s" % (ora, lim, dev))
    RECORD["effects, cov_solve"] = {"cells": cs.n, "pairs": ["rho index 0", "5", "10"], "oracle": ora, "limit": lim, "device": dev}
    assert pr.PATHS * ora["x"] <= pr.CEILING and dev["x"] <= lim["x"], (dev, lim)
