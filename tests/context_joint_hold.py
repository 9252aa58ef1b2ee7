"""What tests/test_gpu_context_joint.py and tests/test_gpu_context_blocks.py hold a joint scan
(``CellRegMap.scan_interaction_contexts_joint``) to (plain helper module, not a test): the reference's operands at the
grid point a scan reports (``_At``), the comparison of the held variants of a scan against it (``_hold``, with the tail
``_hold_tail`` and the limits and the record ``_finish``), bit equality of two scans (``_same``) and the C entry point called
directly (``_abi_scan``).

``RECORD`` collects the per-case errors of tests/test_gpu_context_joint.py, which writes them out; a module with a record
file of its own passes its dictionary as ``record=``.
"""
import ctypes
import math

import numpy as np

import context_joint_reference as jr
import pinned_reference as pr

RECORD = {}
LD = pr.LD
TINY, ONE_LESS = jr.TINY, jr.ONE_LESS
OK, COLLINEAR = 0, 1


def _device(cs, y=None, C=None, W=None):
    import cellregmap_amd as crm

    return crm.CellRegMap(cs.y if y is None else y, cs.C if C is None else C, W=cs.W if W is None else W, **cs.device_kw())


class _At:
    """The reference's and the oracle's operands at the grid point a scan reports."""

    def __init__(self, cs, y, rho, W=None, C=None, XC=None):
        from oracle.sugar import economic_qs_linear

        self.cs, self.y, self.rho = cs, np.asarray(y, float), float(rho)
        self.W, self.C = cs.W if W is None else W, cs.C if C is None else C
        self.XC = self.C if XC is None else XC            # the context columns of the design matrix (full rank)
        hS = np.asarray(cs.half(self.rho), LD)
        self.gram = hS @ hS.T
        (self.Q0,), self.S0 = economic_qs_linear(cs.half(self.rho), return_q1=False)

    def at(self, g, delta, keep=None):
        X = np.column_stack([self.W, self.XC, g])
        return (jr.joint_test(self.y, X, g, self.C, self.gram, delta, keep=keep),
                jr.oracle_joint_at(self.y, X, self.Q0, self.S0, g, self.C, delta, keep=keep))


def _hold_tail(case, j, pv, info):
    dof = int(info["dof"][j])
    lrs = -2 * float(info["null_lml"][j]) + 2 * float(info["alt_lml"][j])
    want = jr.mp_log_pvalue(dof, lrs)
    got = float(info["log_pvalue"][j])
    assert abs(got - want) <= jr.tail_tolerance(dof, want), (case, j, dof, lrs, got, want)
    want_p = jr.mp_pvalue(dof, lrs)
    if TINY < want_p < ONE_LESS:
        assert abs(pv[j] - want_p) <= jr.tail_tolerance(dof, math.log(want_p)) * want_p, (case, j, dof, lrs, pv[j], want_p)
    else:
        assert pv[j] == want_p, (case, j, pv[j], want_p)
    return dof


def _finish(case, n, ora, dev, record=None):
    lim = pr.limits(ora, n)
    fmt = lambda e: " ".join("%s %.2e" % kv for kv in sorted(e.items()))  # noqa: E731
    print("\n[pinned] %s: n %d\n[pinned]   oracle  %s\n[pinned]   limit   %s\n[pinned]   device  %s"
          % (case, n, fmt(ora), fmt(lim), fmt(dev)))
    (RECORD if record is None else record)[case] = {"cells": n, "oracle": ora, "limit": lim, "device": dev,
                                                    "share": {k: dev[k] / lim[k] for k in dev}}
    for k, v in ora.items():
        assert pr.PATHS * v <= pr.CEILING, (case, k, v)                  # the ceiling sets no limit
    for k, v in dev.items():
        assert v <= lim[k], (case, k, v, lim[k])
    return lim


def _hold(case, cs, y, G, pv, info, fast, sel=None, at=None, keep=None, record=None):
    """Every number of the variants ``sel`` of a joint scan of ``G`` against the reference at the device's own
    (rho1, null_delta_i).  ``keep``: the candidates the device is to keep (default all)."""
    rho, gene_delta = float(info["rho1"][0]), float(info["gene_null_delta"])
    assert 0.0 <= rho <= 1.0 and 0.0 < gene_delta < 1.0
    at = _At(cs, y, rho) if at is None else at
    k = at.C.shape[1]
    keep = list(range(k)) if keep is None else list(keep)
    p = G.shape[1]
    assert pv.shape == (p,) and info["beta"].shape == (p, k) and info["dropped"].shape == (p, k)
    assert info["status"].dtype == np.int32 and info["dof"].dtype == np.int32 and info["dropped"].dtype == bool
    sel = pr.pick(p) if sel is None else sel
    want_dropped = np.ones(k, bool)
    want_dropped[keep] = False
    ora, dev, dofs = [], [], set()
    for j in sel:
        delta = float(info["null_delta"][j])
        if fast:
            assert delta == gene_delta, (case, j, delta, gene_delta)
        assert 1e-3 < delta < 1 - 1e-3, (case, j, delta)
        assert info["status"][j] == OK and info["dof"][j] == len(keep), (case, j, info["status"][j], info["dof"][j])
        assert np.array_equal(info["dropped"][j], want_dropped), (case, j, info["dropped"][j])
        rest = [q for q in range(k) if q not in keep]
        assert np.all(np.isnan(info["beta"][j, rest])) and np.all(np.isnan(info["beta_se"][j, rest]))
        ref, own = at.at(G[:, j], delta, keep=keep)
        got = {"null_lml": info["null_lml"][j], "alt_lml": info["alt_lml"][j], "beta": info["beta"][j, keep],
               "beta_se": info["beta_se"][j, keep]}
        ora.append(jr.errors(own, ref))
        dev.append(jr.errors(got, ref))
        dofs.add(_hold_tail(case, j, pv, info))
    lim = _finish(case, cs.n, pr.worst(ora), pr.worst(dev), record)
    return at, lim


_KEYS = ("null_lml", "null_delta", "alt_lml", "dof", "beta", "beta_se", "dropped", "log_pvalue", "status")
_INT = ("dof", "dropped", "status")


def _same(a, b):
    (pa, ia), (pb, ib) = a, b
    assert np.array_equal(pa, pb)
    for key in _KEYS:
        assert np.array_equal(ia[key], ib[key], equal_nan=key not in _INT), key
    for key in ("rho1", "e2", "g2", "eps2"):
        assert np.array_equal(ia[key], ib[key]), key
    assert ia["gene_null_lml"] == ib["gene_null_lml"] and ia["gene_null_delta"] == ib["gene_null_delta"]


def _abi_scan(cs, panel, first, count, fast, outputs=True, C=None, X0=None):
    """crm_scan_interaction_contexts_joint called directly on a gene bound as the Python method binds it."""
    from cellregmap_amd import _engine, _lib

    lib = _lib.load()
    obj = _device(cs)
    C = cs.C if C is None else C
    if X0 is None:
        U, s, _ = _engine._economic_svd(np.concatenate([cs.W, C], axis=1))
        X0 = U * s
    X0, y, C = _lib.f64(X0), _lib.f64(cs.y), _lib.f64(C)
    k = C.shape[1]
    gene = ctypes.c_void_p()
    _lib.check(lib.crm_gene_create(obj._bg.handle, _lib.ptr(y), _lib.ptr(X0), X0.shape[1], _lib.ptr(C), k, ctypes.byref(gene)))
    try:
        m = max(count, 0)
        out = [np.empty(m), np.empty(m), np.empty(m), np.empty(m, np.int32), np.empty((m, k)), np.empty((m, k)),
               np.empty((m, k), np.int32), np.empty(m, np.int32), np.empty(m), np.empty(m), np.full(6, np.nan)]
        rc = lib.crm_scan_interaction_contexts_joint(gene, panel.handle, first, count, int(fast),
                                                     *[_lib.ptr(a) if outputs else None for a in out])
    finally:
        lib.crm_gene_destroy(gene)
    return rc, out
