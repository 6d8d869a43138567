"""The link table of altro_hip_shift_duals (altro_amd/csrc/al_shift.h: al_shift_build), checked on the CPU by tests/cpp/al_shift_test.cpp against
tables written out by hand for plans LANE, MFMA16 and GENERIC (plain g++, nothing of the library linked); once more as a build with the
address and undefined-behaviour sanitizers."""
import os

from tests import cpp_build

# kernels/al_types.h includes the HIP runtime header for its device helper: the host compiler needs its directory and the platform define
HIP = ["-isystem", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-Wno-attributes"]
ARGS = dict(include_dirs=["altro_amd/csrc"], defines=["__HIP_PLATFORM_AMD__"], link_lib=False, timeout=300)


def test_al_shift():
    rc, out, err = cpp_build.run("al_shift_test", extra_link=HIP, **ARGS)
    assert rc == 0 and "al_shift_test ok" in out, out + err


def test_al_shift_sanitized():
    rc, out, err = cpp_build.run("al_shift_test", out_name="al_shift_test_san",
                                 extra_link=HIP + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"], **ARGS)
    assert rc == 0 and "al_shift_test ok" in out, out + err
