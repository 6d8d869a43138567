"""The ledger of a batch handle's buffers (altro_amd/csrc/device_ledger.h): what altro_hip_batch_device_bytes adds up and what
altro_hip_batch_destroy drains.  Checked on the CPU by tests/cpp/device_ledger_test.cpp (plain g++, malloc / free as the backends,
nothing of the library linked)."""
from tests import cpp_build


def test_device_ledger():
    rc, out, err = cpp_build.run("device_ledger_test", include_dirs=["altro_amd/csrc"], link_lib=False, timeout=120)
    assert rc == 0 and "device_ledger_test ok" in out, out + err
