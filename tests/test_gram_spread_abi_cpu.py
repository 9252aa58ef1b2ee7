"""The form ``wb_gram_spread`` exists without a GPU: crm_test_set_form refuses a name it does not know and takes this one,
and include/crm_hip_test.h lists it beside ``wb_gram_fused``."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_form_is_registered_and_documented():
    from cellregmap_amd import _lib

    lib = _lib.load()
    assert lib.crm_test_set_form(b"wb_gram_spread_", 1, 0) != 0     # (an unknown name is refused ...)
    try:
        for value in (0, 1):
            assert lib.crm_test_set_form(b"wb_gram_spread", value, 0) == 0     # (... this one is taken)
    finally:
        assert lib.crm_test_set_form(b"wb_gram_spread", 0, 1) == 0             # back to the default
    assert '"wb_gram_spread" 0' in open(os.path.join(ROOT, "include", "crm_hip_test.h")).read()
