"""The two regulator examples (the reference's Example_of_Regulator_MPC.py and Example_of_Tube_Regulator_MPC.py scenarios
through this package) run and print their expected lines."""
import os
import runpy
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(script, argv, monkeypatch, capsys):
    from LinearMPCOverNetworks import polytope_lite as pl
    old = pl.set_lp_backend("hip")           # the examples use the package defaults
    monkeypatch.setattr(sys, "argv", [script] + argv)
    try:
        runpy.run_path(os.path.join(ROOT, "examples", script), run_name="__main__")
    finally:
        pl.set_lp_backend(old)
    return capsys.readouterr().out


@pytest.mark.gpu
def test_regulator_example(hip_lib, capsys, monkeypatch):
    out = _run("regulator_mpc.py", [], monkeypatch, capsys)
    assert "regulator MPC: 20 steps from x0 = (1, 3): max |u_t| = 1.0000 (U = [-1, 1])" in out
    assert "Input constraints violated" not in out
    assert "input constraint violations 0, infeasible solves 0" in out
    line = [ln for ln in out.splitlines() if "device loop" in ln][0]
    assert float(line.rsplit("=", 1)[1]) < 1e-12


@pytest.mark.gpu
def test_tube_regulator_example(hip_lib, capsys, monkeypatch):
    out = _run("tube_regulator_mpc.py", ["--mc", "1024", "--T", "30"], monkeypatch, capsys)
    assert "x - x_nom in Z at 10 of 10 steps, x in X at 10, u in U at 10" in out
    assert ("tube regulator MPC Monte Carlo: 1024 trajectories x 30 steps: tube violations 0, X violations 0, "
            "U violations 0, infeasible solves 0") in out
