"""The `num_params` argument of the run-time unit makers (altro_amd/csrc/rtc_unit.h; altro_hip_set_model_source_params): P = 0 is the
unit of altro_hip_set_model_source byte for byte, P > 0 adds one define and one piece of the cache key.  Checked on the CPU by
tests/cpp/rtc_unit_params_test.cpp (plain g++, nothing of the library linked)."""
from tests import cpp_build


def test_rtc_unit_num_params():
    rc, out, err = cpp_build.run("rtc_unit_params_test", include_dirs=["altro_amd/csrc"], link_lib=False, timeout=120)
    assert rc == 0 and "rtc_unit_params_test ok" in out, out + err
