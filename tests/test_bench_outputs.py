"""bench.py as the driver runs it: a plain run prints the headline line without the --full sections, `ms_per_step` is the
timed region over --steps, and --dump-outputs writes what the last timed step computed (float64, in the order of the harvested
states, so the same arrays whatever --steps is)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(common.PKG)
NAMES = ["gathered_iters.npy", "gathered_status.npy", "iters.npy", "status.npy", "u_nom.npy", "x_nom0.npy", "xu_ss.npy"]


def _bench(out, steps, warmup):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                          "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_plain_run_line_and_dumped_outputs(tmp_path):
    lines = {k: _bench(tmp_path / str(k), k, 2) for k in (12, 7)}
    for k, line in lines.items():
        assert line["steps"] == k and line["warmup"] == 2 and line["ms_per_step"] > 0
        assert abs(line["value"] * line["ms_per_step"] - 4096e3) < 1e-6 * 4096e3          # one step = one solve of the batch
        assert line["dtype"] == "f64" and line["higher_is_better"] is True and line["unit"] == "solves/s"
        assert line["preload"] == "solves" and line["config"]["optimal_fraction"] == 1.0
        assert not {"cpu_baseline", "closed_loop", "closed_loop_small", "config3", "config5", "offline_lp", "pipelined",
                    "single_call"} & set(line)
    assert sorted(os.listdir(tmp_path / "12")) == NAMES
    total = 0
    for n in NAMES:
        a, b = np.load(tmp_path / "12" / n), np.load(tmp_path / "7" / n)
        assert a.dtype == np.float64 and a.shape == b.shape and np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "12" / "u_nom.npy").shape == (4096, 10, 1)
    assert np.all(np.load(tmp_path / "12" / "status.npy") == 0) and np.all(np.isfinite(np.load(tmp_path / "12" / "u_nom.npy")))
