"""CPU checks of the many-phenotype context entries: declared in include/crm_hip.h beside the single-gene entries, bound in
``cellregmap_amd._lib`` with the header's signatures, exported by the library, and the Python scans and wrappers of the
package with the parameter lists the other many-phenotype calls have."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CTYPE = {"int": ctypes.c_int, "long": ctypes.c_long, "double": ctypes.c_double}
OUTPUTS = {
    "crm_scan_interaction_contexts": ["out_pvalue", "out_alt_lml", "out_beta", "out_beta_se", "out_logp", "out_status",
                                      "out_null_lml", "out_null_delta"],
    "crm_scan_interaction_contexts_joint": ["out_pvalue", "out_logp", "out_alt_lml", "out_dof", "out_beta", "out_beta_se",
                                            "out_dropped", "out_status", "out_null_lml", "out_null_delta"],
}


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crm_hip.h")).read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "%s is not declared in include/crm_hip.h" % name
    return m.group(1), [" ".join(a.split()) for a in m.group(2).split(",")], m.start()


@pytest.mark.parametrize("single", sorted(OUTPUTS))
def test_the_ctypes_signature_follows_the_header(single):
    from cellregmap_amd import _lib

    name = single + "_multi"
    res, args, at = _declaration(name)
    restype, argtypes = _lib.SIGNATURES[name]
    assert res == "int" and restype is ctypes.c_int
    got = [ctypes.c_void_p if "*" in a else _CTYPE[a.replace("const", "").split()[0]] for a in args]
    assert got == argtypes, args
    # the leading arguments of crm_scan_association_multi, then the single-gene entry's outputs without its out_null
    _, assoc, _ = _declaration("crm_scan_association_multi")
    assert args[:7] == assoc[:7] == ["crm_gene* const* genes", "int ngenes", "crm_panel* panel", "long first", "long count",
                                    "int fast", "const double* null"]
    _, plain, before = _declaration(single)
    assert before < at                                              # declared beside (after) the single-gene entry
    assert [a.split()[-1] for a in args[7:]] == OUTPUTS[single]
    assert args[7:] == plain[5:-1] and plain[-1] == "double* out_null"
    # exported by the library
    assert hasattr(_lib.load(), name)


def test_the_python_calls_are_exported_with_the_parameters_of_the_other_many_calls():
    import cellregmap_amd as pkg

    for name in ("scan_interaction_contexts_many", "scan_interaction_contexts_joint_many"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
        sig = inspect.signature(getattr(pkg, name))
        assert list(sig.parameters) == ["crms", "G", "cis_index", "contexts", "fast", "return_stats", "progress"]
        assert [sig.parameters[q].default for q in list(sig.parameters)[2:]] == [None, None, True, False, False]
    for name in ("run_interaction_contexts_many", "run_interaction_contexts_joint_many"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
        sig = inspect.signature(getattr(pkg, name))
        assert list(sig.parameters) == ["Y", "E", "G", "W", "E1", "E2", "hK", "cis_index", "contexts", "fast", "device"]
        kinds = [sig.parameters[q].kind for q in ("cis_index", "contexts", "fast", "device")]
        assert kinds == [inspect.Parameter.KEYWORD_ONLY] * 4
        assert sig.parameters["fast"].default is True and sig.parameters["cis_index"].default is None


def test_the_python_calls_check_their_arguments_before_the_device_is_asked():
    import cellregmap_amd as pkg

    with pytest.raises(ValueError, match="no phenotypes"):
        pkg.scan_interaction_contexts_many([], None)
    with pytest.raises(ValueError, match="no phenotypes"):
        pkg.scan_interaction_contexts_joint_many([], None)
    with pytest.raises(ValueError, match="n x genes"):
        pkg.run_interaction_contexts_many([1.0, 2.0], None, None)
