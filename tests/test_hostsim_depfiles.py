"""The host-model binaries of tests/wavesim follow the headers their kernels include: the Makefile takes its prerequisites from the
compiler (-MMD), not from a list kept by hand.  A list once left out csrc/tmpc_law_wave.hpp, and the sanitizer tests of the wave kernel
passed against a binary of the previous source.  CPU only."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "wavesim"))
import hostsim  # noqa: E402
import run_case  # noqa: E402


def _prerequisites(binary):
    with open(binary + ".d") as f:
        text = f.read().replace("\\\n", " ")
    rule = next(ln for ln in text.splitlines() if ln.startswith(f"_build/{os.path.basename(binary)}:"))
    return {os.path.basename(p) for p in rule.split(":", 1)[1].split()}


def test_depfiles_name_the_headers_the_kernels_include(tmp_path_factory):
    wave = hostsim.binaries_or_skip(tmp_path_factory, "wavesim", extra=run_case.EXTRA)
    assert {"wavesim_main.cpp", "tmpc_kernels.hip", "tmpc_law_wave.hpp", "tmpc_law.hpp", "hip_sim.hpp"} <= _prerequisites(wave["wavesim_asan"])
    wgrad = hostsim.binaries_or_skip(tmp_path_factory, "wgradsim")
    assert {"wgradsim_main.cpp", "tmpc_sens.hip", "tmpc_sens.hpp", "hip_sim.hpp"} <= _prerequisites(wgrad["wgradsim_asan"])
