"""bench.py's plain run on one GPU (no --full): the result line and what --dump-outputs writes, against the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle
from tests import problems

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plain_run_dumps_the_last_timed_step(tmp_path):
    batch, N, steps = 256, 32, 4
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", str(batch), "--horizon", str(N),
                        "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=560)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["n_gpus"] == 1 and out["dtype"] == "f64" and out["higher_is_better"] is True
    assert out["value"] == pytest.approx(batch * steps / (out["ms_per_step"] * steps * 1e-3), rel=1e-9)
    # nothing beyond the timed steps without --full
    assert "cpu_baseline" not in out and "single_problem_seam" not in out
    assert out["config"]["other_configs"] is None and out["config"]["ilqr_full_solve"] is None and out["config"]["repeat"] is None

    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert set(got) == {"K", "d", "P", "p", "x", "u", "y", "delta_V", "status", "problems"}
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert all(a.dtype == np.float64 for a in got.values())
    idx = got["problems"].astype(np.int64)
    assert len(idx) == 64 and (np.diff(idx) > 0).all() and idx[-1] < batch
    assert got["delta_V"].shape == (batch, 2) and (got["status"] == -1).all()

    pr = problems.c1_double_integrator(batch, N=N)
    pr = {k: v[idx] for k, v in pr.items() if isinstance(v, np.ndarray)}
    ref = oracle.backward_batch(pr["A"], pr["B"], pr["f"], pr["Q"], pr["R"], pr["H"], pr["q"], pr["r"])
    fw = oracle.forward_batch(pr["A"], pr["B"], pr["f"], ref["K"], ref["d"], ref["P"], ref["p"], pr["x0"])
    for k, want in (("K", ref["K"]), ("d", ref["d"]), ("P", ref["P"]), ("p", ref["p"]), ("x", fw["x"]), ("u", fw["u"]),
                    ("y", fw["y"])):
        assert got[k].shape == want.shape, k
        assert np.abs(got[k] - want).max() <= 1e-8 * max(1.0, np.abs(want).max()), k
