"""Which instantiation of plan GENERIC's sweep kernels a launch takes (altro_amd/csrc/sweep_route.h: blocks in LDS, late Q, work block in
global memory; forward sweep staged or not), checked on the CPU by tests/cpp/sweep_route_test.cpp against rows written out by hand (plain
g++, nothing of the library linked); once more as a build with the address and undefined-behaviour sanitizers."""
from tests import cpp_build

ARGS = dict(include_dirs=["altro_amd/csrc"], link_lib=False, timeout=300)


def test_sweep_route_rows():
    rc, out, err = cpp_build.run("sweep_route_test", **ARGS)
    assert rc == 0 and "sweep_route_test ok" in out, out + err


def test_sweep_route_rows_sanitized():
    rc, out, err = cpp_build.run("sweep_route_test", out_name="sweep_route_test_san",
                                 extra_link=["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"], **ARGS)
    assert rc == 0 and "sweep_route_test ok" in out, out + err
