"""examples/reference_schedules.py runs end to end and reports sane numbers."""
import os
import re
import runpy
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_reference_schedules_example_runs(hip_lib, capsys, monkeypatch):
    from LinearMPCOverNetworks import polytope_lite as pl
    old = pl.set_lp_backend("hip")           # the examples use the package defaults
    monkeypatch.setattr(sys, "argv", ["reference_schedules.py", "--trajectories", "4", "--steps", "24"])
    try:
        runpy.run_path(os.path.join(ROOT, "examples", "reference_schedules.py"), run_name="__main__")
    finally:
        pl.set_lp_backend(old)
    out = capsys.readouterr().out
    assert "1. set-point x = (+0.200, +0.020, -0.250): 16 trajectories, 24 steps" in out
    assert "2. 8 manoeuvres x 4 trajectories" in out and "manoeuvre 7 (amplitude 2.00)" in out
    assert "3. stepped session, references filtered on the device: 16 trajectories, 24 steps" in out
    assert len(re.findall(r"solves not optimal 0\b", out)) == 3
    assert "steps outside the tube 0" in out and "outside the tube 0;" in out
