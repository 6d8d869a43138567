"""rtc_unit_tile's `user` argument (altro_amd/csrc/rtc_unit.h): the unit a plan MFMA16 handle with a constraint slot from the caller's
source compiles -- text, defines, name expressions, options, key; the unit without the argument is today's byte for byte
(tests/cpp/rtc_unit_tile_user_test.cpp, plain g++, nothing of the library linked).  Also built with the address and undefined-behaviour
sanitizers as the stand-alone program it is."""
import os
import shutil
import subprocess

import pytest

from tests import cpp_build


def test_rtc_unit_tile_user():
    rc, out, err = cpp_build.run("rtc_unit_tile_user_test", include_dirs=["altro_amd/csrc"], link_lib=False, timeout=120)
    assert rc == 0 and "rtc_unit_tile_user_test ok" in out, out + err
    rc, out, err = cpp_build.run("rtc_unit_test", include_dirs=["altro_amd/csrc"], link_lib=False, timeout=120)   # unchanged, and still passes
    assert rc == 0 and "rtc_unit_test ok" in out, out + err


def test_rtc_unit_tile_user_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed")
    exe = str(tmp_path / "rtc_unit_tile_user_test_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(cpp_build.ROOT, "altro_amd", "csrc"),
                           os.path.join(cpp_build.CPP, "rtc_unit_tile_user_test.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "rtc_unit_tile_user_test ok" in p.stdout, p.stdout + p.stderr
