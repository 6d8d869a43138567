"""Which kernels run each operation of the iLQR loop, with which grid, dynamic LDS and mode (altro_amd/csrc/loop_route.h), checked on the CPU by
tests/cpp/loop_route_test.cpp against rows written out by hand (plain g++, nothing of the library linked); once more as a build with the
address and undefined-behaviour sanitizers."""
import os

from tests import cpp_build

# kernels/al_types.h includes the HIP runtime header for its device helper: the host compiler needs its directory and the platform define
HIP = ["-isystem", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-Wno-attributes"]
ARGS = dict(include_dirs=["altro_amd/csrc"], defines=["__HIP_PLATFORM_AMD__"], link_lib=False, timeout=300)


def test_loop_route_rows():
    rc, out, err = cpp_build.run("loop_route_test", extra_link=HIP, **ARGS)
    assert rc == 0 and "loop_route_test ok" in out, out + err


def test_loop_route_rows_sanitized():
    # (-O0: the rows are one long function of initializer lists, which the instrumented optimiser takes minutes over)
    rc, out, err = cpp_build.run("loop_route_test", out_name="loop_route_test_san",
                                 extra_link=HIP + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O0"], **ARGS)
    assert rc == 0 and "loop_route_test ok" in out, out + err
