"""Resource notes of the gfx950 code objects inside lib/libtmpc_hip.so (no GPU needed: the notes are read from the
library's .hip_fatbin section, scripts/code_object_notes.py).  The wave-per-QP shapes must not touch scratch: builds of that
kernel with > 120 spilled registers once returned wrong statuses.

And their disassembly: no DPP read of a register inside the wait states that gfx9 hardware leaves to software, in the
product library and in the two harness libraries of tests/wavecheck."""
import importlib.util
import os
import subprocess

import pytest

import common
import dpp_hazard_lint

ROOT = os.path.dirname(common.PKG)
spec = importlib.util.spec_from_file_location("code_object_notes", os.path.join(ROOT, "scripts", "code_object_notes.py"))
notes = importlib.util.module_from_spec(spec)
spec.loader.exec_module(notes)


OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
LIBS = {"product": "libtmpc_hip.so", "harness": "libtmpc_wavecheck.so", "harness, compiler's form": "libtmpc_wavecheck_nofmac.so"}


def _listings(libname, tmp_path):
    """the disassembly of every gfx950 code object inside a library of lib/ (a missing library is an error)"""
    objs = notes.code_objects(os.path.join(common.PKG, "lib", libname))
    assert objs, libname
    for i, (ident, elf) in enumerate(objs):
        assert "gfx950" in ident, ident
        p = tmp_path / f"{libname}.{i}.elf"
        p.write_bytes(elf)
        yield subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", "--symbolize-operands", str(p)], capture_output=True, text=True,
                             check=True).stdout


@pytest.mark.parametrize("which", list(LIBS))
def test_no_dpp_read_hazard_in_the_code_objects(which, tmp_path):
    """Two wait states between a vector-ALU write of a register and a DPP read of it, five after a vector-ALU write of EXEC
    (tests/dpp_hazard_lint.py): csrc/tmpc_wave.hpp keeps them by hand around its inline-assembly v_fmac_f64_dpp / v_mov_b64_dpp, and
    what surrounds each inlined copy decides.  The harness libraries of tests/test_wave_primitives_gpu.py are held to the same rule, so
    that what they measure is not a hazard of their own."""
    tot = {"dpp": 0, "cut": 0, "violations": [], "fused": 0, "without_waits": 0}
    for text in _listings(LIBS[which], tmp_path):
        r = dpp_hazard_lint.lint(text)
        tot["dpp"] += r["dpp"]
        tot["cut"] += r["cut"]
        tot["violations"] += r["violations"]
        tot["fused"] += text.count("\tv_fmac_f64_dpp ")
        if which != "product":
            # the same listing with every s_nop taken out: the lint must object to a real listing too, not only to hand-written ones
            bare = "\n".join(ln for ln in text.split("\n") if "\ts_nop " not in ln)
            tot["without_waits"] += len(dpp_hazard_lint.lint(bare)["violations"])
    print(f"{LIBS[which]}: {tot['dpp']} DPP instructions ({tot['fused']} v_fmac_f64_dpp), {tot['cut']} windows cut at a label or "
          f"a branch, {len(tot['violations'])} violations" + (f"; {tot['without_waits']} with the s_nop deleted" if which != "product" else ""))
    assert not tot["violations"], tot["violations"][:20]
    if which == "product":
        assert tot["dpp"] >= 10000 and tot["fused"] > 0, tot
    else:
        assert tot["dpp"] > 0 and tot["without_waits"] > 0, tot
        assert (tot["fused"] == 0) == (which != "harness"), tot      # the fused form is in the one library and not in the other


def test_dpp_hazard_lint_flags_what_it_should():
    """the lint on hand-written listings: exactly the hazardous ones are flagged"""
    dpp = "\tv_fmac_f64_dpp v[6:7], v[4:5], v[34:35] row_newbcast:0 row_mask:0xf bank_mask:0xf// 000000001000: 00000000 00000000\n"
    far = "\tv_add_f64 v[10:11], v[12:13], v[14:15]\n"
    cases = {
        "clean": ("\tv_mul_f64 v[4:5], v[0:1], v[2:3]\n" + far + far + dpp, 0),
        "write one before": (far + "\tv_mul_f64 v[4:5], v[0:1], v[2:3]\n" + dpp, 1),
        "write two before, s_nop 0": ("\tv_mul_f64 v[4:5], v[0:1], v[2:3]\n\ts_nop 0\n" + dpp, 1),
        "write two before, s_nop 1": ("\tv_mul_f64 v[4:5], v[0:1], v[2:3]\n\ts_nop 1\n" + dpp, 0),
        "pair overlap": ("\tv_fma_f64 v[5:6], v[0:1], v[2:3], v[8:9]\n" + far + dpp, 1),
        "no overlap": ("\tv_fma_f64 v[2:3], v[0:1], v[4:5], v[8:9]\n" + dpp, 0),        # reads v[4:5], writes neither
        "another file": ("\tv_accvgpr_write_b32 a4, v0\n" + dpp, 0),
        "a load is not the vector ALU": ("\tds_read_b64 v[4:5], v20\n\ts_waitcnt lgkmcnt(0)\n" + dpp, 0),
        "the destination alone": ("\tv_mul_f64 v[6:7], v[0:1], v[2:3]\n" + dpp, 0),
        "second source alone": ("\tv_mul_f64 v[34:35], v[0:1], v[2:3]\n" + dpp, 0),
        "v_cmpx three ahead": ("\tv_cmpx_lt_f64_e32 v[0:1], v[2:3]\n" + far + far + dpp, 1),
        "v_cmpx six ahead": ("\tv_cmpx_lt_f64_e32 v[0:1], v[2:3]\n" + far * 5 + dpp, 0),
        "v_cmpx behind s_nop 4": ("\tv_cmpx_lt_f64_e32 v[0:1], v[2:3]\n\ts_nop 4\n" + dpp, 0),
        "32-bit move": ("\tv_mov_b32_e32 v5, v3\n\tv_mov_b32_dpp v5, v5 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n", 1),
        "swap writes both": ("\tv_permlane32_swap_b32_e32 v8, v4\n" + far + dpp, 1),
        "behind a label": ("\tv_mul_f64 v[4:5], v[0:1], v[2:3]\n0000000000001000 <L0>:\n" + dpp, 0),
        "behind a branch": ("\tv_mul_f64 v[4:5], v[0:1], v[2:3]\n\ts_cbranch_execz L8\n" + dpp, 0),
    }
    for name, (text, want) in cases.items():
        r = dpp_hazard_lint.lint(text)
        assert r["dpp"] == 1, name
        assert len(r["violations"]) == want, (name, r)
        assert r["cut"] == (1 if name.startswith("behind a") else 0), (name, r)
    both = dpp_hazard_lint.lint(cases["clean"][0] + cases["write one before"][0] + cases["pair overlap"][0])
    assert both["dpp"] == 3 and [v[0] for v in both["violations"]] == [7, 10]      # (line numbers of the two flagged reads)


def _kernels():
    ks = notes.kernels(os.path.join(common.PKG, "lib", "libtmpc_hip.so"))
    dm = notes.demangle(list(ks))
    return {dm[n]: k for n, k in ks.items()}


def test_wave_shapes_have_no_private_segment():
    ks = _kernels()
    wave = {n: k for n, k in ks.items() if "::solve_kernel<" in n}
    assert len(wave) == 13, sorted(wave)
    for n, k in wave.items():
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"], k[".vgpr_spill_count"])
        # (a spill count without a private segment is the accumulation-register file used as spill space: one wave per SIMD)
        assert k[".vgpr_spill_count"] <= 16, (n, k[".vgpr_spill_count"])
    bench = [k for n, k in wave.items() if "solve_kernel<11, 1, 0, 5, 4, 0, 8>" in n]
    assert len(bench) == 1 and bench[0][".vgpr_count"] <= 256 and bench[0][".vgpr_spill_count"] == 0      # two waves per SIMD


def test_fused_closed_loop_kernels_match_the_solve_kernels():
    """closed_loop_kernel<shape> is solve_kernel<shape>'s body with the trajectory's state machines between two solves (the record of
    the loop read through the constant address space, field by field): the same register budget, no scratch."""
    ks = _kernels()
    fused = {n: k for n, k in ks.items() if "::closed_loop_kernel<" in n}
    wave = {n.split("::solve_kernel")[1]: k for n, k in ks.items() if "::solve_kernel<" in n}
    assert len(fused) == 13, sorted(fused)
    for n, k in fused.items():
        shape = n.split("::closed_loop_kernel")[1].split("(")[0]
        twin = [v for m, v in wave.items() if m.split("(")[0] == shape]
        assert len(twin) == 1, (n, sorted(wave))
        assert k[".vgpr_count"] <= twin[0][".vgpr_count"] + 24, (n, k[".vgpr_count"], twin[0][".vgpr_count"])
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
    bench = [k for n, k in fused.items() if "closed_loop_kernel<11, 1, 0, 5, 4, 0, 8>" in n]
    assert len(bench) == 1 and bench[0][".vgpr_count"] <= 256 and bench[0][".vgpr_spill_count"] == 0
    # the extended controller's form: one problem at one time step, the state machines of its trajectories inside
    step = {n: k for n, k in ks.items() if "::closed_loop_step_kernel<" in n}
    assert len(step) == 13, sorted(step)
    for n, k in step.items():
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])


def test_other_kernels_stay_within_their_known_footprint():
    """The block kernel carries no scratch since round 3 (model record and launch record behind one pointer each, read through
    the constant address space; lane- and record-derived values re-derived per phase: DESIGN.md 5.2).  The LP kernels and the
    closed-loop kernels: the LP shapes up to d = 16 carry none."""
    ks = _kernels()
    block = {n: k for n, k in ks.items() if "::solve_block_kernel<" in n}
    assert len(block) == 4
    for n, k in block.items():
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, (n, k[".vgpr_spill_count"], k[".private_segment_fixed_size"])
        assert k[".vgpr_count"] <= 256, (n, k[".vgpr_count"])        # T = 8: two waves per SIMD
    # the closed loop's state machines: one wave per trajectory, state vectors on the lanes -- no private arrays (round 3: a
    # thread per trajectory with 1168 B of them)
    step = [k for n, k in ks.items() if "mc_step_kernel" in n]
    assert len(step) == 1 and step[0][".private_segment_fixed_size"] == 0 and step[0][".vgpr_spill_count"] == 0
    assert not any("mc_post_kernel" in n or "mc_tube_kernel" in n for n in ks)
    for n, k in ks.items():
        if "::lp_kernel<" in n:
            # d <= 16: no scratch.  D = 32 (one wave per SIMD, all 512 registers: the normal matrix's column blocks) keeps
            # nine dwords of kernel-prologue values in scratch since the round-3 hand-over code (five stores and six loads
            # in the whole kernel, none inside a loop: `scratch_` lines of the -S output sit at the prologue and at two
            # phase boundaries)
            limit = 64 if "lp_kernel<32" in n else 0
            assert k[".private_segment_fixed_size"] <= limit, (n, k[".private_segment_fixed_size"])
