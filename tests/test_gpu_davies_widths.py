"""Davies' and Liu's p-values of csrc/davies.hip on a real MI355X, at 2 to 256 weights, against the long-double build of
oracle/qfc.c and an mpmath statement of the modified-Liu value (tests/davies_reference.py; the yardsticks themselves are
proved in tests/test_oracle_davies_widths_cpu.py).  One launch of the trace hook per width; per case

* ifault and the path -- evaluation counter, abscissas summed, integrations -- are the float64 oracle's;
* where ifault is 0 and 0 < p <= 1, |p_device - p_LD| is within the limit of davies_reference.davies_limit;
* where the oracle returns Liu's value, pv is liu bitwise;
* liu is within 32 x scipy's own error (never below 1e-13 relative) of the mpmath value, down to 0 below the double range;
* a row that the filter shortens gives the bits of the same row shortened by the host;
* crm_test_davies and crm_test_davies_trace give the same bits: the trace changes no arithmetic.

CRM_DAVIES_WIDTHS_JSON=<file> records the measured errors (profiles/davies_widths_errors.json).

Measured on the MI355X (profiles/davies_widths_errors.json): the path is the oracle's on all 962 rows, |p - p_LD| <= 7.1e-16
(at most 0.053 of the limit), Liu within 1.9e-13 relative of mpmath (at most 0.89 of its limit).
"""
import ctypes
import json
import os

import numpy as np
import pytest

import davies_cases as dc
import davies_reference as dr

pytestmark = pytest.mark.gpu

SET_ASIDE_CAP = 0.02


@pytest.fixture(scope="module")
def ctx():
    from cellregmap_amd import _lib

    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.crm_ctx_create(0, ctypes.byref(h)))
    record = {}
    yield lib, h, record
    lib.crm_ctx_destroy(h)
    path = os.environ.get("CRM_DAVIES_WIDTHS_JSON")
    if path and record:
        widths = [dict(width=k, **record[k]) for k in sorted(record)]
        out = {"limits": "tests/davies_reference.py: davies_limit (absolute), liu_refs (relative)", "widths": widths,
               "largest_share_of_the_limit": {"davies": max(w["davies_share"] for w in widths),
                                              "liu": max(w["liu_share"] for w in widths)},
               "largest_error": {"davies_absolute": max(w["davies_error"] for w in widths),
                                 "liu_relative": max(w["liu_error"] for w in widths)}}
        with open(path, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


def _launch(ctx, k, Q, lam, trace=True):
    from cellregmap_amd import _lib

    lib, h, _ = ctx
    Q, lam = _lib.f64(Q), _lib.f64(lam)
    n = Q.size
    pv = np.full(n, np.nan); ifault = np.full(n, -99, np.int32); liu = np.full(n, np.nan)
    if not trace:
        _lib.check(lib.crm_test_davies(h, n, k, _lib.ptr(Q), _lib.ptr(lam), _lib.ptr(pv), _lib.ptr(ifault), _lib.ptr(liu)))
        return pv, ifault, liu
    tr = np.full((n, 3), -1, np.int32)
    _lib.check(lib.crm_test_davies_trace(h, n, k, _lib.ptr(Q), _lib.ptr(lam), _lib.ptr(pv), _lib.ptr(ifault), _lib.ptr(liu),
                                         _lib.ptr(tr)))
    return pv, ifault, liu, tr


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def test_the_set_aside_share():
    refs = dr.refs()
    assert sum(not r.same_path for r in refs) <= SET_ASIDE_CAP * len(refs)


@pytest.mark.parametrize("k", sorted(dc.by_width()))
def test_davies_and_liu_at_width(ctx, k):
    refs = [r for r in dr.refs() if r.case.k == k]
    liu_table = dr.liu_refs()
    Q = np.array([r.case.q for r in refs])
    lam = np.stack([r.case.lam for r in refs])
    pv, ifault, liu, tr = _launch(ctx, k, Q, lam)
    pv0, ifault0, liu0 = _launch(ctx, k, Q, lam, trace=False)
    assert np.array_equal(_bits(pv), _bits(pv0)) and np.array_equal(_bits(liu), _bits(liu0))
    assert np.array_equal(ifault, ifault0)

    failures = []
    worst_davies = worst_liu = err_davies = err_liu = 0.0
    exits = {}
    for i, r in enumerate(refs):
        exits[r.exit] = exits.get(r.exit, 0) + 1
        if not r.same_path:
            continue
        name = r.case.name
        if ifault[i] != r.ifault or tuple(tr[i]) != r.trace:
            failures.append((name, "path", int(ifault[i]), tuple(int(x) for x in tr[i]), r.ifault, r.trace))
        if r.davies_held:
            share = abs(pv[i] - r.p_ld) / r.limit
            print("%-28s p %.17g  |p - p_LD| %.3g  limit %.3g  share %.3g" % (name, pv[i], abs(pv[i] - r.p_ld), r.limit, share))
            worst_davies = max(worst_davies, share)
            err_davies = max(err_davies, abs(pv[i] - r.p_ld))
            if not share <= 1.0:
                failures.append((name, "davies", pv[i], r.p_ld, r.limit))
        if r.liu_returned and _bits(pv[i:i + 1])[0] != _bits(liu[i:i + 1])[0]:
            failures.append((name, "pv is not liu", pv[i], liu[i]))
        if name in liu_table:
            want, limit, _ = liu_table[name]
            err = dr.liu_rel_err(liu[i], want)
            worst_liu = max(worst_liu, err / limit)
            err_liu = max(err_liu, err)
            if not dr.liu_limit_ok(liu[i], want, limit):
                failures.append((name, "liu", liu[i], float(want), err, limit))
    print("width %d: largest share of the limit: Davies %.3g, Liu %.3g" % (k, worst_davies, worst_liu))
    ctx[2][k] = {"cases": len(refs), "davies_share": worst_davies, "liu_share": worst_liu,
                 "davies_error": err_davies, "liu_error": err_liu,
                 "exits": {e: n / len(refs) for e, n in sorted(exits.items())}}
    assert not failures, failures


@pytest.mark.parametrize("k", dc.FILTER_WIDTHS)
def test_a_row_the_filter_shortens_gives_the_bits_of_the_shortened_row(ctx, k):
    rows = dc.filter_rows(k)
    Q = np.array([c.q for c in rows])
    pv, ifault, liu, tr = _launch(ctx, k, Q, np.stack([c.lam for c in rows]))
    for i, c in enumerate(rows):
        kept = dc.kept(c.lam)
        assert kept.size < k
        pv1, ifault1, liu1, tr1 = _launch(ctx, kept.size, Q[i:i + 1], kept[None, :])
        assert _bits(pv1)[0] == _bits(pv[i:i + 1])[0] and _bits(liu1)[0] == _bits(liu[i:i + 1])[0], (c.name, pv1, pv[i])
        assert ifault1[0] == ifault[i] and tuple(tr1[0]) == tuple(tr[i]), c.name
        if kept.size == 1:
            assert _bits(pv[i:i + 1])[0] == _bits(liu[i:i + 1])[0]
