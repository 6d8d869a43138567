"""Right-hand sides per knot point in the constraint tables (altro_amd/csrc/al_tables.h: al_build with AlDef::g_per_knot; kernels/al_types.h:
al_g_index), checked on the CPU by tests/cpp/al_rhs_test.cpp against pool offsets and per-knot-point g_off written out by hand on plans LANE,
MFMA16 and GENERIC, AlSummary::uniform under its rule, and the index function against a brute-force walk (plain g++, nothing of the library
linked); once more as a build with the address and undefined-behaviour sanitizers."""
import os

from tests import cpp_build

# kernels/al_types.h includes the HIP runtime header for its device helper: the host compiler needs its directory and the platform define
HIP = ["-isystem", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-Wno-attributes"]
ARGS = dict(include_dirs=["altro_amd/csrc"], defines=["__HIP_PLATFORM_AMD__"], link_lib=False, timeout=300)


def test_al_rhs():
    rc, out, err = cpp_build.run("al_rhs_test", extra_link=HIP, **ARGS)
    assert rc == 0 and "al_rhs_test ok" in out, out + err


def test_al_rhs_sanitized():
    rc, out, err = cpp_build.run("al_rhs_test", out_name="al_rhs_test_san",
                                 extra_link=HIP + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"], **ARGS)
    assert rc == 0 and "al_rhs_test ok" in out, out + err
