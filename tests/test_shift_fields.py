"""Where the dynamics given as data and the cost's linear terms live on each plan, and how altro_hip_shift_dynamics / _shift_linear_costs walk
them in place (altro_amd/csrc/shift_fields.h), checked on the CPU by tests/cpp/shift_fields_test.cpp against offsets written out by hand
(plain g++, nothing of the library linked); once more as a stand-alone build with the address and undefined-behaviour sanitizers."""
from tests import cpp_build

ARGS = dict(include_dirs=["altro_amd/csrc"], link_lib=False, timeout=120)


def test_shift_fields():
    rc, out, err = cpp_build.run("shift_fields_test", **ARGS)
    assert rc == 0 and "shift_fields_test ok" in out, out + err


def test_shift_fields_sanitized():
    rc, out, err = cpp_build.run("shift_fields_test", out_name="shift_fields_test_san",
                                 extra_link=["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"], **ARGS)
    assert rc == 0 and "shift_fields_test ok" in out, out + err
