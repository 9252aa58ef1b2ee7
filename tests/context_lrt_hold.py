"""What tests/test_gpu_context_lrt.py and tests/test_gpu_context_blocks.py hold a per-context scan
(``CellRegMap.scan_interaction_contexts``) to (plain helper module, not a test): the reference's operands at the grid point
a scan reports (``_At``), the comparison of the held variants of a scan against it (``_hold``, with the tails
``_hold_tails`` and the limits and the record ``_finish``), bit equality of two scans (``_same``) and the C entry point
called directly (``_abi_scan``).

``RECORD`` collects the per-case errors of tests/test_gpu_context_lrt.py, which writes them out; a module with a record
file of its own passes its dictionary as ``record=``.
"""
import ctypes

import numpy as np

import context_lrt_reference as cr
import pinned_reference as pr

RECORD = {}
LD = pr.LD
TINY, ONE_LESS = 2.2250738585072014e-308, 1 - 2.220446049250313e-16
OK, COLLINEAR = 0, 1


def _device(cs, y=None, C=None):
    import cellregmap_amd as crm

    return crm.CellRegMap(cs.y if y is None else y, cs.C if C is None else C, W=cs.W, **cs.device_kw())


class _At:
    """The reference's and the oracle's operands at the grid point a scan reports."""

    def __init__(self, cs, y, rho, W=None, C=None):
        from oracle.sugar import economic_qs_linear

        self.cs, self.y, self.rho = cs, np.asarray(y, float), float(rho)
        self.W, self.C = cs.W if W is None else W, cs.C if C is None else C
        hS = np.asarray(cs.half(self.rho), LD)
        self.gram = hS @ hS.T
        (self.Q0,), self.S0 = economic_qs_linear(cs.half(self.rho), return_q1=False)

    def X(self, g):
        return np.column_stack([self.W, self.C, g])

    def at(self, g, delta):
        """(the reference's record, the float64 oracle's) of one variant at ``delta``."""
        return (cr.context_tests(self.y, self.X(g), g, self.C, self.gram, delta),
                cr.oracle_context_at(self.y, self.X(g), self.Q0, self.S0, g, self.C, delta))

    def refit(self, g):
        """(L*, x*, curvature) of the variant's null [W, C, g] maximised over delta by the reference."""
        from oracle.lmm import LMM

        o = LMM(self.y, self.X(g), ((self.Q0,), self.S0), restricted=False)
        o.fit(verbose=False)
        return pr.pinned_ml_max(self.y, self.X(g), None, o._x, gram=self.gram)


def _mp():
    import mpmath as mp

    mp.mp.dps = 40
    return mp


def _mp_pvalue(null_lml, alt_lml):
    """``lrt_pvalues`` of the device's own doubles with the tail in mpmath."""
    mp = _mp()
    lrs = max(-2 * null_lml + 2 * alt_lml, TINY)
    return min(max(float(mp.erfc(mp.sqrt(mp.mpf(lrs) / 2))), TINY), ONE_LESS)


def _mp_log_pvalue(null_lml, alt_lml):
    mp = _mp()
    lrs = max(-2 * null_lml + 2 * alt_lml, 0.0)
    return float(mp.log(mp.erfc(mp.sqrt(mp.mpf(lrs) / 2))))


def _hold_tails(case, j, pv, info, cols):
    null_lml = float(info["null_lml"][j])
    for q in cols:
        alt = float(info["alt_lml"][j, q])
        want = _mp_pvalue(null_lml, alt)
        assert abs(pv[j, q] - want) <= 1e-14 * want, (case, j, q, pv[j, q], want)
        want = _mp_log_pvalue(null_lml, alt)
        got = float(info["log_pvalue"][j, q])
        assert abs(got - want) <= 1e-14 * abs(want), (case, j, q, got, want)


def _finish(case, n, ora, dev, extra=None, record=None):
    lim = pr.limits(ora, n)
    fmt = lambda e: " ".join("%s %.2e" % kv for kv in sorted(e.items()))  # noqa: E731
    print("\n[pinned] %s: n %d\n[pinned]   oracle  %s\n[pinned]   limit   %s\n[pinned]   device  %s%s"
          % (case, n, fmt(ora), fmt(lim), fmt(dev), "" if extra is None else "\n[pinned]   %s" % extra))
    record = RECORD if record is None else record
    record[case] = {"cells": n, "oracle": ora, "limit": lim, "device": dev, "share": {k: dev[k] / lim[k] for k in dev}}
    if extra is not None:
        record[case]["refit"] = extra
    for k, v in ora.items():
        assert pr.PATHS * v <= pr.CEILING, (case, k, v)                  # the ceiling sets no limit
    for k, v in dev.items():
        assert v <= lim[k], (case, k, v, lim[k])
    return lim


def _hold(case, cs, y, G, pv, info, fast, sel=None, at=None, cols=None, record=None):
    """Every number of the variants ``sel`` of a scan of ``G`` (the n x p matrix the panel stands for) against the
    reference at the device's own (rho1, null_delta_i).  ``cols``: the contexts compared (default all)."""
    rho, gene_delta = float(info["rho1"][0]), float(info["gene_null_delta"])
    assert 0.0 <= rho <= 1.0 and 0.0 < gene_delta < 1.0
    at = _At(cs, y, rho) if at is None else at
    k = at.C.shape[1]
    cols = list(range(k)) if cols is None else cols
    p = G.shape[1]
    assert pv.shape == (p, k) and info["null_lml"].shape == (p,) and info["status"].dtype == np.int32
    sel = pr.pick(p) if sel is None else sel
    ora, dev, tops = [], [], []
    for j in sel:
        delta = float(info["null_delta"][j])
        if fast:
            assert delta == gene_delta, (case, j, delta, gene_delta)
        else:
            top, x, curvature = at.refit(G[:, j])
            assert 1e-3 < float(pr._logistic(x)) < 1 - 1e-3, (case, j, float(x))
            tops.append((j, top, x, curvature))
        assert 1e-3 < delta < 1 - 1e-3, (case, j, delta)
        ref, own = at.at(G[:, j], delta)
        got = {"null_lml": info["null_lml"][j], "alt_lml": info["alt_lml"][j], "beta": info["beta"][j],
               "beta_se": info["beta_se"][j]}
        assert np.all(info["status"][j, cols] == OK), (case, j, info["status"][j])
        ora.append(cr.errors(own, ref, cols))
        dev.append(cr.errors(got, ref, cols))
        _hold_tails(case, j, pv, info, cols)
    extra = None
    if tops:
        short = {int(j): float(top - LD(info["null_lml"][j])) for j, top, _, _ in tops}
        allow = {int(j): pr.refit_allowance(x, c) for j, _, x, c in tops}
        extra = {"short of L*": short, "allowance": allow}
    lim = _finish(case, cs.n, pr.worst(ora), pr.worst(dev), extra, record)
    for j, top, x, curvature in tops:
        edge = lim["lml"] * abs(float(top))
        assert -short[int(j)] <= edge, (case, j, short[int(j)], edge)
        assert short[int(j)] <= edge + allow[int(j)], (case, j, short[int(j)], edge, allow[int(j)])
    return at, lim


_KEYS = ("null_lml", "null_delta", "alt_lml", "beta", "beta_se", "log_pvalue", "status")


def _same(a, b):
    (pa, ia), (pb, ib) = a, b
    assert np.array_equal(pa, pb)
    for key in _KEYS:
        assert np.array_equal(ia[key], ib[key], equal_nan=(key != "status")), key
    for key in ("rho1", "e2", "g2", "eps2"):
        assert np.array_equal(ia[key], ib[key]), key
    assert ia["gene_null_lml"] == ib["gene_null_lml"] and ia["gene_null_delta"] == ib["gene_null_delta"]


def _abi_scan(cs, panel, first, count, fast, outputs=True):
    """crm_scan_interaction_contexts called directly on a gene bound as the Python method binds it."""
    from cellregmap_amd import _engine, _lib

    lib = _lib.load()
    obj = _device(cs)
    U, s, _ = _engine._economic_svd(np.concatenate([cs.W, cs.C], axis=1))
    X0, y, C = _lib.f64(U * s), _lib.f64(cs.y), _lib.f64(cs.C)
    gene = ctypes.c_void_p()
    _lib.check(lib.crm_gene_create(obj._bg.handle, _lib.ptr(y), _lib.ptr(X0), X0.shape[1], _lib.ptr(C), cs.k, ctypes.byref(gene)))
    try:
        m = max(count, 0)
        out = [np.empty((m, cs.k)) for _ in range(5)] + [np.empty((m, cs.k), np.int32), np.empty(m), np.empty(m), np.empty(6)]
        rc = lib.crm_scan_interaction_contexts(gene, panel.handle, first, count, int(fast),
                                               *[_lib.ptr(a) if outputs else None for a in out])
    finally:
        lib.crm_gene_destroy(gene)
    return rc, out
