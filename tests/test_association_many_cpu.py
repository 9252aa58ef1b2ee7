"""Multi-phenotype association scans: the C-ABI entries and the Python surface, without a GPU."""
import ctypes
import inspect

ERR_ARG = -2


def test_multi_association_symbols_are_exported():
    from cellregmap_amd import _lib

    lib = _lib.load()
    for name in ("crm_association_null_multi", "crm_scan_association_multi"):
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES


def test_null_and_empty_gene_lists_are_refused_before_the_device():
    from cellregmap_amd import _lib

    lib = _lib.load()
    out = (ctypes.c_double * 12)()
    null = (ctypes.c_double * 6)(1.0, 0.0, 0.0, 1.0, -1.0, 0.5)
    pv = (ctypes.c_double * 4)()
    assert lib.crm_association_null_multi(None, 1, out) == ERR_ARG
    assert lib.crm_association_null_multi(None, 0, out) == ERR_ARG
    one = (ctypes.c_void_p * 1)(None)
    assert lib.crm_association_null_multi(one, 1, out) == ERR_ARG
    assert lib.crm_association_null_multi(one, 0, out) == ERR_ARG
    assert lib.crm_association_null_multi(one, -3, out) == ERR_ARG
    assert lib.crm_scan_association_multi(None, 1, None, 0, 4, 1, null, pv, None) == ERR_ARG
    assert lib.crm_scan_association_multi(one, 0, None, 0, 4, 1, null, pv, None) == ERR_ARG
    assert lib.crm_scan_association_multi(one, 1, None, 0, 4, 0, null, pv, None) == ERR_ARG
    assert lib.crm_scan_association_multi(one, -1, None, 0, 4, 0, None, None, None) == ERR_ARG
    assert lib.crm_last_error()


def test_python_entries_are_public():
    import cellregmap_amd as pkg

    for name in ("scan_association_many", "run_association_many"):
        assert name in pkg.__all__
        assert callable(getattr(pkg, name))
    sig = inspect.signature(pkg.run_association_many)
    assert list(sig.parameters)[:5] == ["Y", "W", "E", "G", "hK"]   # run_association's positional order
    assert sig.parameters["cis_index"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["fast"].default is False
    sig = inspect.signature(pkg.scan_association_many)
    assert list(sig.parameters) == ["crms", "G", "cis_index", "fast", "return_stats", "progress"]


def test_scan_association_many_refuses_an_empty_list():
    import pytest

    from cellregmap_amd import scan_association_many

    with pytest.raises(ValueError):
        scan_association_many([], None)
