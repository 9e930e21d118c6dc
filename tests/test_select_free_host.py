"""The select-free factorisation and back substitution of csrc/tmpc_wave.hpp (wv::rows16_factor_masked, wv::rows16_backsub_lane_masked:
what depends on a lane's place in the triangle runs under a constant EXEC pattern) against the forms with a select per use, on the host
execution model.  CPU only.  tests/wavesim/selectfree_main.cpp keeps a copy of the select forms as the reference and runs both through
factor (right-hand side carried) + back substitution, then forward + back substitution of a second right-hand side; every output of
all 64 lanes -- factor rows, 1 / d, both solutions, the flag -- must agree BIT FOR BIT, NaNs included.  The program is built plain and,
where the host toolchain has the runtimes, under ASan + UBSan and MSan.

What runs here is the model of the masked instructions (`if (lane in pattern)`), not the instructions: that the device agrees with
this model is tests/test_select_free_gpu.py.

Also here: the opcode classifier of scripts/asm_phase_mix.py on literal lines of compiler output."""
import os
import sys

import numpy as np
import pytest

import select_free_cases as sf

sys.path.insert(0, os.path.join(sf.ROOT, "tests", "wavesim"))
import hostsim  # noqa: E402

SIZES = [1, 2, 8, 11, 12, 16]
KINDS = ("plain", "asan", "msan")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return str(tmp_path_factory.mktemp("selectfree")), hostsim.binaries_or_skip(tmp_path_factory, "selectfree", KINDS, per_variant=True)


def _both(programs, kind, n, rows, b1, b2, tag):
    d, exes = programs
    exe = exes[hostsim.names("selectfree", [kind])[0]]          # (skips where the host toolchain has no runtime of this kind)
    rc, err, forms = sf.run(exe, n, rows, b1, b2, d, f"{kind}_{n}_{tag}", env=hostsim.SAN_ENV)
    hostsim.assert_clean(err)
    assert rc in (0, 1), (rc, err[-2000:])
    for key in sf.KEYS:
        assert np.array_equal(sf.bits(forms["masked"][key]), sf.bits(forms["select"][key])), (kind, n, tag, key)
    assert rc == 0
    return forms["masked"]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", SIZES)
def test_masked_forms_equal_the_select_forms_on_spd_matrices(programs, kind, n):
    rows, b1, b2 = sf.random_problems(n)
    o = _both(programs, kind, n, rows, b1, b2, "spd")
    assert np.all(o["ok"] == 1.0) and np.all(np.isfinite(o["x"])) and np.all(np.isfinite(o["x2"]))
    # the solutions solve: row 0 of the first wave against numpy (the comparison above is the test; this guards the set-up)
    A = rows[0, :n, :]
    assert np.allclose(A @ o["x"][0, :n], b1[0, :n], atol=1e-6 * np.abs(b1[0, :n]).max() * np.linalg.cond(A))
    live = (np.arange(sf.L) % 16) < n
    assert np.all(o["x"][:, ~live] == 0.0) and np.all(o["dinv"][:, ~live] == 1.0)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", SIZES)
def test_a_pivot_that_is_not_positive_gives_the_same_flag_and_outputs(programs, kind, n):
    steps, (rows, b1, b2) = sf.bad_pivot_problems(n)
    o = _both(programs, kind, n, rows, b1, b2, "pivot")
    assert np.all(o["ok"] == 0.0), (steps, o["ok"][:, 0])          # (wave-uniform: 16-lane row 0 decides)
    assert np.all(o["dinv"][:, (np.arange(sf.L) % 16) >= n] == 1.0)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", SIZES)
def test_an_infinity_in_an_excluded_lane_still_meets_its_zero_multiplier(programs, kind, n):
    rows, b1, b2 = sf.infinity_problems(n)
    o = _both(programs, kind, n, rows, b1, b2, "inf")
    if n > 1:
        # the carried right-hand side of wave 0 has its infinity on lane n / 2 of 16-lane row 0: at step n / 2 of the factorisation
        # lane 0 multiplies it by its -0 and carries a NaN into the solve -- a masked UPDATE would have left x_0 finite
        assert np.isnan(o["x"][0, 0])
        # the same for the forward substitution of the second right-hand side (wave 2, 16-lane row 1; its steps broadcast the
        # lanes 0 ... n - 2, so lane n / 2 is among them from n = 3)
        assert n < 3 or np.isnan(o["x2"][2, 16])
        # and the 16-lane rows without an infinity are untouched by it
        assert np.all(np.isfinite(o["x"][0, 16:])) and np.all(np.isfinite(o["x2"][2, 32:]))


# ---------------------------------------------------------------- scripts/asm_phase_mix.py
def _mix():
    sys.path.insert(0, os.path.join(sf.ROOT, "scripts"))
    import asm_phase_mix
    return asm_phase_mix


LINES = [("\tv_fmac_f64_e32 v[124:125], v[24:25], v[124:125]", "fp64"),
         ("\tv_fmac_f64_dpp v[18:19], v[18:19], v[28:29] row_newbcast:0 row_mask:0xf bank_mask:0xf", "fp64"),
         ("\tv_fma_f64 v[24:25], -v[122:123], v[124:125], 1.0", "fp64"),
         ("\tv_mul_f64_e64 v[28:29], -v[16:17], v[124:125]", "fp64"),
         ("\tv_cmp_lt_f64_e32 vcc, 0, v[122:123]", "fp64"),
         ("\tv_rcp_f64_e32 v[124:125], v[122:123]", "fp64"),
         ("\tv_mfma_f64_4x4x4_4b_f64 v[0:1], v[2:3], v[4:5], v[0:1]", "mfma"),
         ("\tv_cndmask_b32_e64 v33, v31, v201, s[10:11]", "v_cndmask"),
         ("\tv_cmp_gt_u32_e32 vcc, 3, v0", "v_cmp"),
         ("\tv_mov_b64_dpp v[122:123], v[16:17] row_newbcast:0 row_mask:0xf bank_mask:0xf", "v_mov_dpp"),
         ("\tv_mov_b64_e32 v[24:25], 1.0", "v_mov"),
         ("\tv_readlane_b32 s4, v250, 17", "readlane"),
         ("\tv_permlane32_swap_b32_e32 v4, v6", "v_swap"),
         ("\tv_lshlrev_b64 v[28:29], 63, 1", "valu_other"),
         ("\ts_mov_b32 exec_lo, 0x10001", "salu"),
         ("\tds_read_b64 v[2:3], v1 offset:8", "ds_read")]


def test_asm_phase_mix_classifies_every_f64_opcode_as_arithmetic():
    m = _mix()
    for line, want in LINES:
        assert m.classify(m.opcode(line)) == want, line
    for line in ("", "\t; MARK 3", ".LBB0_12:", "\t.p2align 6", "\t;;#ASMSTART"):
        assert m.opcode(line) is None, line
    text = ["\t; MARK 2"] + [ln for ln, _ in LINES] + ["\t; MARK 3", "\tv_add_f64 v[0:1], v[0:1], v[2:3]", "\t; MARK 4"]
    rows = m.phase_mix(text)
    assert [(p0, p1) for p0, p1, _, _ in rows] == [(2, 3), (3, 4)]
    vec, ari, rest = m.split(rows[0][2])
    assert (vec, ari, rest) == (14, 7, 7)           # (the two last lines are scalar and LDS: not vector instructions)
    assert rows[0][3] == 2 and m.split(rows[1][2]) == (1, 1, 0)
