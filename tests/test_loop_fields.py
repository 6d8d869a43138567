"""Where each field of the iLQR loop lives on each plan (altro_amd/csrc/loop_fields.h), checked on the CPU by tests/cpp/loop_fields_test.cpp
against offsets written out by hand (plain g++, nothing of the library linked); once more as a build with the address and undefined-behaviour
sanitizers."""
from tests import cpp_build


def test_loop_fields_offsets():
    rc, out, err = cpp_build.run("loop_fields_test", include_dirs=["altro_amd/csrc"], link_lib=False, timeout=120)
    assert rc == 0 and "loop_fields_test ok" in out, out + err


def test_loop_fields_offsets_sanitized():
    rc, out, err = cpp_build.run("loop_fields_test", include_dirs=["altro_amd/csrc"], link_lib=False, timeout=120, out_name="loop_fields_test_san",
                                 extra_link=["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    assert rc == 0 and "loop_fields_test ok" in out, out + err
