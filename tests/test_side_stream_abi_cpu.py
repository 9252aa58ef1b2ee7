"""The side stream's test hooks exist without a GPU: the form ``side_stream`` is registered (crm_test_set_form refuses a name
it does not know) and ``crm_test_side_stream_blocks`` is exported with the signature include/crm_hip_test.h declares."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_form_is_registered():
    from cellregmap_amd import _lib

    lib = _lib.load()
    assert lib.crm_test_set_form(b"side_stream_", 1, 0) != 0     # (an unknown name is refused ...)
    try:
        for value in (0, 2, 3, 1):
            assert lib.crm_test_set_form(b"side_stream", value, 0) == 0     # (... this one is taken)
    finally:
        assert lib.crm_test_set_form(b"side_stream", 0, 1) == 0             # back to the default


def test_the_counter_is_exported_with_its_signature():
    from cellregmap_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "crm_test_side_stream_blocks")
    restype, argtypes = _lib.SIGNATURES["crm_test_side_stream_blocks"]
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_long)]
    header = open(os.path.join(ROOT, "include", "crm_hip_test.h")).read()
    assert re.search(r"int\s+crm_test_side_stream_blocks\(const crm_ctx\* ctx, long\* blocks\);", header)
    out = ctypes.c_long(-1)
    assert lib.crm_test_side_stream_blocks(None, ctypes.byref(out)) != 0     # (no context: an argument error, no crash)
    assert out.value == -1
