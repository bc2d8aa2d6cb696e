"""bench.py on the GPU, in its plain form: the line's timed-step fields, and --dump-outputs
writing the state the timed steps left, the same arrays in every run of the same arguments."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(capsys, argv):
    bench.main(argv)
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_plain_run_dumps_the_same_state_every_time(tmp_path, capsys):
    from vaeb_amd.model import initial_params
    argv = ["--gpus", "1", "--steps", "6", "--warmup", "3"]
    lines = [_run(capsys, argv + ["--dump-outputs", str(tmp_path / d)]) for d in ("a", "b")]
    for line in lines:
        assert line["steps"] == 6 and line["warmup"] == 3 and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(100 * 6 / (line["ms_per_step"] * 6e-3), rel=1e-9)
        assert line["graph"] == ["replay"] and "kernels_ms" not in line and "cpu_baseline" not in line
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["adagrad_state.npy", "elbo.npy", "params.npy"]
    a = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n in a:
        assert a[n].dtype in (np.float32, np.float64) and np.isfinite(a[n]).all()
        assert np.array_equal(a[n], np.load(tmp_path / "b" / f"{n}.npy")), n
    theta0 = np.concatenate([p.ravel() for p in initial_params(784, 500, 20, False)])
    assert a["params"].shape == theta0.shape and not np.array_equal(a["params"], theta0)
    assert (a["adagrad_state"] >= 0).all() and a["adagrad_state"].max() > 0
    mean, total, n = a["elbo"]
    assert n == 6 and mean == pytest.approx(total / 6) and mean == pytest.approx(lines[0]["elbo"])
