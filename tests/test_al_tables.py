"""What the constraint tables contain (altro_amd/csrc/al_tables.h: al_build, al_slots, al_admit), checked on the CPU by tests/cpp/al_tables_test.cpp
against recordings of the function the builder replaced, against entries written out by hand from kernels/al_types.h, and every capacity at
its limit (plain g++, nothing of the library linked); once more as a build with the address and undefined-behaviour sanitizers."""
import os

from tests import cpp_build

# kernels/al_types.h includes the HIP runtime header for its device helper: the host compiler needs its directory and the platform define
HIP = ["-isystem", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-Wno-attributes"]
ARGS = dict(include_dirs=["altro_amd/csrc"], defines=["__HIP_PLATFORM_AMD__"], link_lib=False, timeout=300)


def test_al_tables():
    rc, out, err = cpp_build.run("al_tables_test", extra_link=HIP, **ARGS)
    assert rc == 0 and "al_tables_test ok" in out, out + err


def test_al_tables_sanitized():
    rc, out, err = cpp_build.run("al_tables_test", out_name="al_tables_test_san",
                                 extra_link=HIP + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"], **ARGS)
    assert rc == 0 and "al_tables_test ok" in out, out + err
