"""BatchSolver::SetModelSource(source, h, num_params) / SetModelParams / GetModelParams (tests/cpp/batch_model_params_test.cpp): the
bicycle from source with a wheel base per vehicle through the C++ wrapper, its rollout equal to the C ABI's on the same plan.  Needs an MI355X."""
import pytest

from tests import cpp_build

pytestmark = pytest.mark.gpu


def test_batch_solver_model_params():
    rc, out, err = cpp_build.run("batch_model_params_test")
    print(out)
    assert rc == 0 and out.strip().endswith("OK"), out + err
    assert out.count("|rollout difference|") == 1
