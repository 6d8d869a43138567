"""The units the library compiles at run time around a caller's model source (altro_amd/csrc/rtc_unit.h): their text, name expressions
and compile options, checked on the CPU by tests/cpp/rtc_unit_test.cpp (plain g++, nothing of the library linked)."""
from tests import cpp_build


def test_rtc_unit_text_names_options():
    rc, out, err = cpp_build.run("rtc_unit_test", include_dirs=["altro_amd/csrc"], link_lib=False, timeout=120)
    assert rc == 0 and "rtc_unit_test ok" in out, out + err
