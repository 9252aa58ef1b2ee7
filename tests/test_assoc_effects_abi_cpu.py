"""The two effects entry points of the association scans without a GPU: their ctypes signatures against the header's
declarations, their misuse codes' constants, and the Python plumbing of ``cis_index`` (repeats, an empty window, runs with
different sets of phenotypes) with the library call stubbed."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CTYPE = {"int": ctypes.c_int, "long": ctypes.c_long, "double": ctypes.c_double}


def _declaration(name):
    text = open(os.path.join(ROOT, "include", "crm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


def _argtype(decl):
    if "*" in decl:
        return ctypes.c_void_p
    base = decl.replace("const", "").split()[0]
    return _CTYPE[base]


def test_ctypes_signatures_follow_the_header():
    from cellregmap_amd import _lib

    for name, plain in (("crm_scan_association_effects", "crm_scan_association"),
                        ("crm_scan_association_multi_effects", "crm_scan_association_multi")):
        res, args = _declaration(name)
        restype, argtypes = _lib.SIGNATURES[name]
        assert res == "int" and restype is ctypes.c_int
        assert [_argtype(a) for a in args] == argtypes, (name, args)
        # the arguments of the plain call, then beta, se, delta, scale, log p (doubles) and the status (ints)
        _, plain_args = _declaration(plain)
        assert args[:len(plain_args)] == plain_args
        added = args[len(plain_args):]
        assert [a.split()[-1] for a in added] == ["out_beta", "out_se", "out_delta", "out_scale", "out_logp", "out_status"]
        assert all(a.startswith("double*") for a in added[:5]) and added[5].startswith("int*")
        assert _lib.SIGNATURES[plain][1] == argtypes[:len(plain_args)]


def test_status_constants_match_the_header():
    from cellregmap_amd import _engine

    text = open(os.path.join(ROOT, "include", "crm_hip.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define CRM_EFFECT_(\w+) (\d+)", text)}
    assert got == {"OK": _engine.EFFECT_OK, "G_IN_SPAN_W": _engine.EFFECT_G_IN_SPAN_W, "NO_FIT": _engine.EFFECT_NO_FIT,
                   "NON_FINITE": _engine.EFFECT_NON_FINITE} == {"OK": 0, "G_IN_SPAN_W": 1, "NO_FIT": 2, "NON_FINITE": 3}


# ---- the plumbing of cis_index with the library stubbed -----------------------------------------------------------------
_KEYS = ("beta", "beta_se", "alt_delta", "alt_scale", "log_pvalue")


def _value(key, gene, column):
    """What the stub writes for (output, phenotype, panel column)."""
    return 1e6 * (1 + _KEYS.index(key)) + 1e3 * gene + column if key in _KEYS else {"pv": 0.5, "alt": -7.0}[key] + gene + 1e-3 * column


class _StubLib:
    def __init__(self):
        self.calls = []

    def crm_association_null_multi(self, handles, ng, out):
        rows = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_double)), shape=(ng, 6))
        for i in range(ng):
            rows[i] = [0.5, 1.0, 2.0, 3.0, -100.0 - i, 0.25]
        return 0

    def _fill(self, hs, ng, first, count, pv, alt, extra):
        def arr(p, t=ctypes.c_double):
            return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(t)), shape=(ng, count))

        genes = [hs[i] - 100 for i in range(ng)]
        cols = first + np.arange(count)
        for row, g in enumerate(genes):
            arr(pv)[row] = _value("pv", g, cols)
            arr(alt)[row] = _value("alt", g, cols)
            if extra:
                for key, p in zip(_KEYS, extra[:5]):
                    arr(p)[row] = _value(key, g, cols)
                arr(extra[5], ctypes.c_int)[row] = cols % 4
        return genes

    def crm_scan_association_multi(self, hs, ng, panel, first, count, fast, null, pv, alt):
        self.calls.append(("plain", self._fill(hs, ng, first, count, pv, alt, None), first, count))
        return 0

    def crm_scan_association_multi_effects(self, hs, ng, panel, first, count, fast, null, pv, alt, *extra):
        assert len(extra) == 6
        self.calls.append(("effects", self._fill(hs, ng, first, count, pv, alt, extra), first, count))
        return 0


class _Panel:
    shape = (30, 12)
    handle = ctypes.c_void_p(1)


class _Crm:
    _bg, _W, _E0, _device = object(), np.ones((30, 1)), np.ones((30, 2)), 0

    def __init__(self, i):
        self._gene = ctypes.c_void_p(100 + i)

    def _panel(self, G):
        return _Panel

    def _bind_gene(self, like=None):
        return self._gene


def _stubbed(monkeypatch):
    from cellregmap_amd import _engine

    stub = _StubLib()
    monkeypatch.setattr(_engine._lib, "load", lambda: stub)
    crms = [_Crm(i) for i in range(3)]
    for c in crms[1:]:
        c._bg = crms[0]._bg
    return _engine, stub, crms


def test_cis_windows_with_a_repeat_and_an_empty_window(monkeypatch):
    _engine, stub, crms = _stubbed(monkeypatch)
    cis = [np.array([7, 2, 2, 9]), slice(1, 8), np.array([], int)]
    cols = [np.array([7, 2, 2, 9]), np.arange(1, 8), np.array([], int)]
    pv, info = _engine.scan_association_many(crms, None, cis_index=cis, fast=True, return_stats="effects")
    assert all(kind == "effects" for kind, *_ in stub.calls)                       # the plain entry point is not called
    tested = sorted((first, count, tuple(genes)) for _, genes, first, count in stub.calls)
    assert tested == [(1, 1, (1,)), (2, 1, (0, 1)), (3, 4, (1,)), (7, 1, (0, 1)), (9, 1, (0,))], tested
    for i in range(3):
        assert np.array_equal(pv[i], _value("pv", i, cols[i]))
        for key in _KEYS:
            assert info[key][i].dtype == np.float64 and np.array_equal(info[key][i], _value(key, i, cols[i])), (key, i)
        assert info["effect_status"][i].dtype == np.int32 and np.array_equal(info["effect_status"][i], cols[i] % 4)
    assert info["rho1"].shape == (3,) and np.array_equal(info["alt_lml"][1], _value("alt", 1, cols[1]))
    assert info["beta"][0][1] == info["beta"][0][2]                                # the repeated column


def test_no_cis_index_and_the_plain_call(monkeypatch):
    _engine, stub, crms = _stubbed(monkeypatch)
    pv, info = _engine.scan_association_many(crms, None, fast=False, return_stats="effects")
    assert [c[0] for c in stub.calls] == ["effects"]
    cols = np.arange(12)
    for key in _KEYS:
        assert info[key].shape == (3, 12)
        assert np.array_equal(info[key], np.stack([_value(key, i, cols) for i in range(3)]))
    assert info["effect_status"].dtype == np.int32 and np.array_equal(info["effect_status"], np.tile(cols % 4, (3, 1)))
    assert info["alt_lml"].shape == (3, 12)
    stub.calls.clear()
    pv2, info2 = _engine.scan_association_many(crms, None, fast=False)
    assert [c[0] for c in stub.calls] == ["plain"] and np.array_equal(pv2, pv)     # effects=False: the new entry point is not called
    assert not set(info2) & set(_KEYS + ("effect_status",))
    with pytest.raises(ValueError):
        _engine.scan_association_many(crms, None, return_stats="everything")
