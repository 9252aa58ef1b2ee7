"""CPU checks behind tests/test_gpu_context_lrt.py: the entry point is declared, bound and exported; the longdouble
reference of the per-context tests (tests/context_lrt_reference.py) is ``pinned_reference.pinned_ml`` with a shared
factorisation; the float64 oracle's own composition -- ``LMM`` with [W, C, g], then
``get_fast_scanner().fast_scan(g[:, None] * C)`` -- agrees with it at the oracle's delta; and every cohort of
tests/context_lrt_cases.py meets the conditions the GPU tests rely on.

Measured when the reference was written, on the association cohorts "c 1", "c 9", "c 62" and "c 70, mode B" with C = E
(the three held variants, all contexts, at the delta of the oracle's own fit of [W, C, g]): the float64 oracle within
3.7e-14 (relative) of the reference on lml and 8.0e-14 on the statistic, both at 62 + 3 columns;
``pinned_reference.limits`` 4e-14 .. 2.6e-12, so the 1e-11 ceiling never sets a limit (asserted).
"""
import inspect
import os
import re

import numpy as np
import pytest

import context_lrt_cases as cc
import context_lrt_reference as cr
import pinned_cases as pc
import pinned_reference as pr
from oracle.lmm import LMM
from oracle.sugar import economic_qs_linear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = pr.LD


def test_the_entry_point_is_declared_bound_and_exported():
    import cellregmap_amd as pkg
    from cellregmap_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crm_hip.h")).read(), flags=re.S)
    proto = re.search(r"int\s+crm_scan_interaction_contexts\s*\(([^)]*)\)", text)
    assert proto, "crm_scan_interaction_contexts is not declared in include/crm_hip.h"
    args = [a.strip() for a in proto.group(1).split(",")]
    assert len(args) == 14 and args[0].startswith("crm_gene*") and args[1].startswith("crm_panel*")
    restype, argtypes = _lib.SIGNATURES["crm_scan_interaction_contexts"]
    assert len(argtypes) == len(args)
    for name in ("CRM_CONTEXT_OK 0", "CRM_CONTEXT_COLLINEAR 1", "CRM_CONTEXT_NO_FIT 2", "CRM_CONTEXT_NON_FINITE 3"):
        assert re.search(r"#define\s+" + name.replace(" ", r"\s+") + r"\b", text), name
    assert "crm_test_set_context_budget" in _lib.SIGNATURES
    assert "run_interaction_contexts" in pkg.__all__ and callable(pkg.run_interaction_contexts)
    sig = inspect.signature(pkg.CellRegMap.scan_interaction_contexts)
    assert list(sig.parameters) == ["self", "G", "contexts", "fast", "return_stats", "progress"]
    assert sig.parameters["contexts"].default is None and sig.parameters["fast"].default is True
    sig = inspect.signature(pkg.run_interaction_contexts)
    assert list(sig.parameters) == ["y", "E", "G", "W", "E1", "E2", "hK", "contexts", "fast", "device"]
    from cellregmap_amd import _engine

    assert (_engine.CONTEXT_OK, _engine.CONTEXT_COLLINEAR, _engine.CONTEXT_NO_FIT, _engine.CONTEXT_NON_FINITE) == (0, 1, 2, 3)


def test_the_reference_is_pinned_ml_with_a_shared_factorisation():
    cs = cc.case("k 3, c 9, mode B")
    hS = np.asarray(cs.half(0.3), LD)
    gram = hS @ hS.T
    g, X = cs.G[:, 1], cs.X(1)
    ref = cr.context_tests(cs.y, X, g, cs.C, gram, 0.37)
    lml, s = pr.pinned_ml(cs.y, X, None, 0.37, gram=gram)
    assert pr.relative(ref["null_lml"], lml) <= 1e-17 and pr.relative(ref["null_scale"], s) <= 1e-17
    for j in range(cs.k):
        lml, s = pr.pinned_ml(cs.y, np.column_stack([X, g * cs.C[:, j]]), None, 0.37, gram=gram)
        assert pr.relative(ref["alt_lml"][j], lml) <= 1e-17, j
        # the frozen-delta ML identity: 2 (alt - null) = n log(1 + z^2 / n), z = beta / beta_se
        z2 = (ref["beta"][j] / ref["beta_se"][j]) ** 2
        assert abs(2 * (ref["alt_lml"][j] - ref["null_lml"]) - cs.n * np.log1p(z2 / cs.n)) <= 1e-16 * abs(lml), j


def _oracle_rows(y, W, C, G, half_of, grid, sel=None):
    """Per held variant (``sel``; default ``pinned_reference.pick``): the oracle's own composition at the oracle's delta
    against the reference there."""
    best = None
    X0 = np.column_stack([W, C])
    for rho in grid:
        (Q0,), S0 = economic_qs_linear(half_of(rho), return_q1=False)
        lmm = LMM(y, X0, ((Q0,), S0), restricted=False)
        lmm.fit(verbose=False)
        if best is None or lmm.lml() > best[1]:
            best = (float(rho), lmm.lml(), Q0, S0)
    rho, _, Q0, S0 = best
    hS = np.asarray(half_of(rho), LD)
    gram = hS @ hS.T
    rows = []
    for j in pr.pick(G.shape[1]) if sel is None else sel:
        X = np.column_stack([X0, G[:, j]])
        o = LMM(y, X, ((Q0,), S0), restricted=False)
        o.fit(verbose=False)
        # the composition of the issue, verbatim: the fitted LMM's lml and its scanner over g * C
        alt = o.get_fast_scanner().fast_scan(G[:, [j]] * C)["lml"]
        ref = cr.context_tests(y, X, G[:, j], C, gram, o.delta)
        own = cr.oracle_context_at(y, X, Q0, S0, G[:, j], C, o.delta)
        assert np.array_equal(own["alt_lml"], alt) and own["null_lml"] == o.lml()
        rows.append((o.delta, cr.errors(own, ref)))
    return rho, rows


@pytest.mark.parametrize("name", ["c 1, mode B", "c 9, mode B", "c 62, mode B", "c 70, mode B"])
def test_the_oracles_composition_agrees_with_the_reference(name):
    cs = pc.AssociationCase(name)
    rho, rows = _oracle_rows(cs.y, cs.W, cs.E, cs.G, cs.half, cs.grid)
    err = pr.worst([e for _, e in rows])
    lim = pr.limits(err, cs.n)
    print("%s (%d cells, rho %.1f): oracle %s; limits %s" % (name, cs.n, rho, ", ".join("%s %.2e" % kv for kv in err.items()),
                                                             ", ".join("%s %.2e" % kv for kv in lim.items())))
    for k, v in err.items():
        assert pr.PATHS * v <= pr.CEILING, (name, k, v)      # the ceiling never sets a limit


_rows = {}


def _case_rows(name):
    if name not in _rows:
        cs = cc.case(name)
        _rows[name] = _oracle_rows(cs.y, cs.W, cs.C, cs.G, cs.half, cs.grid)
    return _rows[name]


@pytest.mark.parametrize("name", list(cc.CASES))
def test_the_ceiling_never_sets_a_limit_on_the_context_cohorts(name):
    cs = cc.case(name)
    rho, rows = _case_rows(name)
    assert rho == cc.oracle_gene_null(cs)[0]
    err = pr.worst([e for _, e in rows])
    print("%s (%d cells, rho %.1f): 32 x the oracle's error: %s" % (name, cs.n, rho, ", ".join("%s %.2e" % (k, 32 * v) for k, v in err.items())))
    for k, v in err.items():
        assert pr.PATHS * v <= pr.CEILING, (name, k, v)
    for delta, _ in rows:                   # the refit bound is stated for optima away from the clamps
        assert 1e-3 < delta < 1 - 1e-3, (name, delta)
    assert 1e-3 < cc.oracle_gene_null(cs)[1].delta < 1 - 1e-3


def test_the_gene_level_nulls_fall_on_more_than_one_grid_point():
    rhos = {name: _case_rows(name)[0] for name in cc.CASES if cc.CASES[name][4] == "B"}
    assert len(set(rhos.values())) >= 2, rhos
    shapes = {(cc.CASES[name][2], cc.CASES[name][2] + cc.CASES[name][3]) for name in cc.CASES}
    assert {k for k, _ in shapes} >= {1, 3, 5, 17} and {c for _, c in shapes} >= {2, 9, 62, 70, 128}, shapes
