"""CPU checks behind tests/test_gpu_context_joint.py: the entry point is declared, bound and exported; the longdouble
reference of the joint test (tests/context_joint_reference.py) is ``pinned_reference.pinned_ml`` with a shared
factorisation; every cohort of tests/context_joint_cases.py meets the conditions the GPU tests rely on; a numpy float64
statement of the device's form (the phi metric, the Schur complement, the Cholesky factor in column order with the drop
rule) stays inside the limits; and the closed-form chi^2 tail holds its tolerance against mpmath.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import context_joint_cases as jc
import context_joint_reference as jr
import context_lrt_cases as cc
import pinned_reference as pr
from oracle.lmm import LMM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = pr.LD
_CTYPE = {"int": ctypes.c_int, "long": ctypes.c_long, "double": ctypes.c_double}


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crm_hip.h")).read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "%s is not declared in include/crm_hip.h" % name
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


def test_the_ctypes_signature_follows_the_header():
    import cellregmap_amd as pkg
    from cellregmap_amd import _lib

    res, args = _declaration("crm_scan_interaction_contexts_joint")
    restype, argtypes = _lib.SIGNATURES["crm_scan_interaction_contexts_joint"]
    assert res == "int" and restype is ctypes.c_int
    got = [ctypes.c_void_p if "*" in a else _CTYPE[a.replace("const", "").split()[0]] for a in args]
    assert got == argtypes, args
    # the leading arguments of the per-context call, then the outputs in the order the issue states
    _, plain = _declaration("crm_scan_interaction_contexts")
    assert args[:5] == plain[:5]
    assert [a.split()[-1] for a in args[5:]] == ["out_pvalue", "out_logp", "out_alt_lml", "out_dof", "out_beta", "out_beta_se",
                                                 "out_dropped", "out_status", "out_null_lml", "out_null_delta", "out_null"]
    assert [a.split()[0] for a in args[5:]] == ["double*", "double*", "double*", "int*", "double*", "double*", "int*", "int*",
                                                "double*", "double*", "double*"]
    assert "run_interaction_contexts_joint" in pkg.__all__ and callable(pkg.run_interaction_contexts_joint)
    sig = inspect.signature(pkg.CellRegMap.scan_interaction_contexts_joint)
    assert list(sig.parameters) == ["self", "G", "contexts", "fast", "return_stats", "progress"]
    assert sig.parameters["contexts"].default is None and sig.parameters["fast"].default is True
    sig = inspect.signature(pkg.run_interaction_contexts_joint)
    assert list(sig.parameters) == ["y", "E", "G", "W", "E1", "E2", "hK", "contexts", "fast", "device"]


def test_the_reference_is_pinned_ml_with_a_shared_factorisation():
    cs = jc.case("k 3, c 9, mode B")
    hS = np.asarray(cs.half(0.3), LD)
    gram = hS @ hS.T
    g, X = cs.G[:, 1], cs.X(1)
    for keep in (None, [0, 2]):
        ref = jr.joint_test(cs.y, X, g, cs.C, gram, 0.37, keep=keep)
        lml, s = pr.pinned_ml(cs.y, X, None, 0.37, gram=gram)
        assert pr.relative(ref["null_lml"], lml) <= 1e-17 and pr.relative(ref["null_scale"], s) <= 1e-17
        cand = g[:, None] * (cs.C if keep is None else cs.C[:, keep])
        lml, s = pr.pinned_ml(cs.y, np.column_stack([X, cand]), None, 0.37, gram=gram)
        assert pr.relative(ref["alt_lml"], lml) <= 1e-17
        # the frozen-delta ML identity: rss0 - rss1 = beta' S beta, so 2 (alt - null) = n log(rss0 / rss1)
        assert abs(2 * (ref["alt_lml"] - ref["null_lml"]) - cs.n * np.log(ref["null_scale"] / s)) <= 1e-16 * abs(lml)
    # one candidate: the per-context reference's numbers
    import context_lrt_reference as cr

    one = jr.joint_test(cs.y, X, g, cs.C, gram, 0.37, keep=[1])
    each = cr.context_tests(cs.y, X, g, cs.C, gram, 0.37)
    assert pr.relative(one["alt_lml"], each["alt_lml"][1]) <= 1e-17
    assert pr.relative(one["beta"][0], each["beta"][1]) <= 1e-16 and pr.relative(one["beta_se"][0], each["beta_se"][1]) <= 1e-16


def _oracle_rows(cs, sel=None):
    """(rho, delta0, [(delta_i, the oracle's errors, the device form's errors)]) of a cohort at the oracle's own optimum, per
    held variant (``sel``; default ``pinned_reference.pick``)."""
    rho, null, (Q0, S0) = cc.oracle_gene_null(cs)
    hS = np.asarray(cs.half(rho), LD)
    gram = hS @ hS.T
    rows = []
    for j in pr.pick(cs.G.shape[1]) if sel is None else sel:
        X, g = cs.X(j), cs.G[:, j]
        o = LMM(cs.y, X, ((Q0,), S0), restricted=False)
        o.fit(verbose=False)
        ref = jr.joint_test(cs.y, X, g, cs.C, gram, o.delta)
        own = jr.oracle_joint_at(cs.y, X, Q0, S0, g, cs.C, o.delta)
        form = jr.device_form(cs.y, X, Q0, S0, g, cs.C, o.delta)
        assert form["dof"] == cs.k and not form["dropped"].any(), (cs.name, j, form["dof"])
        rows.append((o.delta, jr.errors(own, ref), jr.errors(form, ref)))
    return rho, null.delta, rows


_rows = {}


def _case_rows(name):
    if name not in _rows:
        _rows[name] = _oracle_rows(jc.case(name))
    return _rows[name]


@pytest.mark.parametrize("name", list(jc.CASES))
def test_the_cohorts_meet_the_conditions_and_the_device_form_the_limits(name):
    cs = jc.case(name)
    rho, delta0, rows = _case_rows(name)
    ora, form = pr.worst([r[1] for r in rows]), pr.worst([r[2] for r in rows])
    lim = pr.limits(ora, cs.n)
    fmt = lambda e: ", ".join("%s %.2e" % kv for kv in sorted(e.items()))  # noqa: E731
    print("%s (%d cells, rho %.1f): oracle %s; limits %s; device form %s" % (name, cs.n, rho, fmt(ora), fmt(lim), fmt(form)))
    for key, v in ora.items():
        assert pr.PATHS * v <= pr.CEILING, (name, key, v)      # the ceiling never sets a limit
    for delta, _, _ in rows:                                   # the refit bound is stated for optima away from the clamps
        assert 1e-3 < delta < 1 - 1e-3, (name, delta)
    assert 1e-3 < delta0 < 1 - 1e-3
    for j in pr.pick(cs.G.shape[1]):                           # no candidate set that is dependent up to the noise
        assert jc.candidate_condition(cs, j) < 100.0, (name, j, jc.candidate_condition(cs, j))
    for key, v in form.items():
        assert v <= lim[key], (name, key, v, lim[key])


def test_the_gene_level_nulls_fall_on_more_than_one_grid_point():
    rhos = {name: _case_rows(name)[0] for name in jc.CASES if jc.CASES[name][4] == "B"}
    assert len(set(rhos.values())) >= 2, rhos
    wide = {name: _case_rows(name)[0] for name in jc.WIDE}
    assert any(0.0 < rho < 1.0 for rho in wide.values()), wide
    shapes = {(jc.CASES[name][2], jc.CASES[name][2] + jc.CASES[name][3]) for name in jc.WIDE}
    assert shapes == {(33, 35), (50, 51), (64, 66), (48, 128)}, shapes


def test_the_device_forms_drop_rule():
    """A constant context beside the intercept leaves in its own place; of one-hot contexts the last one does."""
    cs = jc.case("k 3, c 9, mode B")
    rho, null, (Q0, S0) = cc.oracle_gene_null(cs)
    hS = np.asarray(cs.half(rho), LD)
    gram = hS @ hS.T
    g = cs.G[:, 0]
    C = np.column_stack([cs.C[:, 0], np.ones(cs.n), cs.C[:, 2]])
    X = np.column_stack([cs.W, C[:, [0, 2]], g])            # (the full-rank columns of [W, C, g])
    form = jr.device_form(cs.y, X, Q0, S0, g, C, null.delta)
    assert form["dof"] == 2 and list(form["dropped"]) == [False, True, False]
    ref = jr.joint_test(cs.y, X, g, C, gram, null.delta, keep=[0, 2])
    own = jr.oracle_joint_at(cs.y, X, Q0, S0, g, C, null.delta, keep=[0, 2])
    kept = dict(form, beta=form["beta"][[0, 2]], beta_se=form["beta_se"][[0, 2]])
    lim = pr.limits(jr.errors(own, ref), cs.n)
    for key, v in jr.errors(kept, ref).items():
        assert v <= lim[key], (key, v, lim[key])
    hot = np.eye(4)[np.arange(cs.n) % 4]
    X = np.column_stack([cs.W, hot[:, :3], g])
    form = jr.device_form(cs.y, X, Q0, S0, g, hot, null.delta)
    assert form["dof"] == 3 and list(form["dropped"]) == [False, False, False, True]


@pytest.mark.parametrize("dof", [1, 2, 3, 5, 17, 33, 48, 50, 64])
def test_the_closed_form_tail_against_mpmath(dof):
    worst = 0.0
    for lrs in np.concatenate([np.geomspace(1e-3, 3000.0, 60), [0.5, 1.0, 2.0, float(dof), 2.0 * dof, 1500.0, 2999.0]]):
        got, want = jr.log_chi2_sf(dof, lrs), jr.mp_log_pvalue(dof, lrs)
        tol = jr.tail_tolerance(dof, want)
        worst = max(worst, abs(got - want) / tol)
        assert abs(got - want) <= tol, (dof, lrs, got, want)
    print("dof %d: worst share of the tolerance %.2f" % (dof, worst))
