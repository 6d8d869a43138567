"""ALTROSolver::SetTimeStep per knot-point range with SetDeviceModel (tests/cpp/altro_time_steps_test.cpp): the goal-constrained pendulum
on a two-step grid through host callbacks and through the device solve, then a uniform grid on the same solvers; the batch wrapper's
SetTimeSteps / GetTimeSteps.  Needs an MI355X."""
import pytest

from tests import cpp_build

pytestmark = pytest.mark.gpu


def test_altro_solver_time_steps_per_range_with_a_device_model():
    rc, out, err = cpp_build.run("altro_time_steps_test")
    print(out)
    assert rc == 0 and out.strip().endswith("OK"), out + err
    assert out.count("|trajectory difference|") == 2
