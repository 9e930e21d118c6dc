"""v_mfma_f64_4x4x4_4b_f64 and the pass built on it (csrc/tmpc_wave.hpp: mfma_blocks, gdg_blocks -- sweep A's G'DG on 4 x 4 x 4 matrix
blocks) on the device, through the probe library lib/libtmpc_mfmablocks.so (tests/wavecheck/mfmablocks.hip, built by
csrc/Makefile with the product's flags):

  * the lane maps of the three operands, read off one-hot operands and checked with index-coded ones against numpy;
  * the pass's [(D.G)'; t'] G against numpy in float64, per entry within 64 eps sum |terms| (every term is rounded once where D g is
    formed, and a sum of n = 4 nks terms adds at most n roundings of partial sums that sum |terms| bounds: (n + 1) eps, 61 eps at the
    largest count, nks = 15), both triangles bit for bit equal, row NV equal to G't;
  * the same inputs through the host-model emulation (tests/wavesim/mfmablocks_main.cpp, a stand-alone host program): equal to the
    last bit, because the emulation adds in the probed order -- k = 0 .. 3 by fused multiply-adds starting from C -- and everything
    else (the order of the k-steps, the even / odd accumulators) is the source's."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import common

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "wavesim"))
import hostsim  # noqa: E402

L = 64
EPS = np.finfo(np.float64).eps
CSRC = os.path.join(common.PKG, "csrc")
_dp = C.POINTER(C.c_double)
SHAPES = [(nv, nks) for nv in (11, 8) for nks in (1, 2, 3, 15)] + [(12, 3), (12, 8)]      # (12: three instructions per k-step; 8: whole trips of the loop)


def _d(a):
    return a.ctypes.data_as(_dp)


class Probe:
    def __init__(self):
        path = os.path.join(common.PKG, "lib", "libtmpc_mfmablocks.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it with `make -C {CSRC}`")
        self.lib = C.CDLL(path)
        self.lib.mfmablocks_sentinel.restype = C.c_double
        self.sentinel = self.lib.mfmablocks_sentinel()

    def raw(self, a, b, c):
        a, b, c = (np.ascontiguousarray(x, dtype=np.float64) for x in (a, b, c))
        assert a.shape == b.shape == c.shape and a.shape[1] == L
        d = np.empty_like(a)
        rc = self.lib.mfmablocks_raw(C.c_int(a.shape[0]), _d(a), _d(b), _d(c), _d(d))
        assert rc == 0, rc
        return d

    def gdg(self, G, D, t):
        P, rows, nv = G.shape
        G, D, t = (np.ascontiguousarray(x, dtype=np.float64) for x in (G, D, t))
        ldm = self.lib.mfmablocks_ldm(C.c_int(nv))
        assert ldm == ((nv + 1) | 1)
        mf, gdr = np.empty((P, nv, ldm)), np.empty((P, nv))
        rc = self.lib.mfmablocks_gdg(C.c_int(nv), C.c_int(rows // 4), C.c_int(P), _d(G), _d(D), _d(t), _d(mf), _d(gdr))
        assert rc == 0, rc
        return mf, gdr


@pytest.fixture(scope="module")
def probe(hip_lib):
    return Probe()


@pytest.mark.gpu
def test_operand_maps(probe):
    """A: lane 16 k + 4 b + i holds A_b[i][k]; B: lane 16 k + 4 b + j holds B_b[k][j]; C / D: lane 16 i + 4 b + j holds D_b[i][j]."""
    eye, one, zero = np.eye(L), np.ones((L, L)), np.zeros((L, L))
    lanes = np.arange(L)
    blk, minor, major = (lanes >> 2) & 3, lanes & 3, lanes >> 4
    same_blk = blk[:, None] == blk[None, :]
    # where a single A entry / B entry shows in D, and which A and B entries meet (same block, same k)
    assert np.array_equal(probe.raw(eye, one, zero) != 0, same_blk & (minor[:, None] == major[None, :]))
    assert np.array_equal(probe.raw(one, eye, zero) != 0, same_blk & (minor[:, None] == minor[None, :]))
    meets = (probe.raw(np.repeat(eye, L, axis=0), np.tile(eye, (L, 1)), np.zeros((L * L, L))) != 0).reshape(L, L, L).any(axis=2)
    assert np.array_equal(meets, same_blk & (major[:, None] == major[None, :]))
    # C passes through on its own lane
    c = np.arange(1.0, L + 1.0)[None, :]
    assert np.array_equal(probe.raw(np.zeros((1, L)), np.zeros((1, L)), c), c)
    # index-coded operands (small integers: every product and sum is exact) against numpy under these maps
    rng = np.random.default_rng(5)
    a, b, c = (rng.integers(-50, 51, (16, L)).astype(np.float64) for _ in range(3))
    A = a.reshape(16, 4, 4, 4).transpose(0, 2, 3, 1)          # [p][k][b][i] -> [p][b][i][k]
    B = b.reshape(16, 4, 4, 4).transpose(0, 2, 1, 3)          # [p][k][b][j] -> [p][b][k][j]
    Cm = c.reshape(16, 4, 4, 4).transpose(0, 2, 1, 3)         # [p][i][b][j] -> [p][b][i][j]
    want = (A @ B + Cm).transpose(0, 2, 1, 3).reshape(16, L)
    assert np.array_equal(probe.raw(a, b, c), want)


def _inputs(nv, nks):
    """per shape six problems: three with D over ten decades as late in a solve, three with one functional's row all zero as well"""
    rng = np.random.default_rng(100 * nv + nks)
    rows = 4 * nks
    G = rng.standard_normal((6, rows, nv))
    D = 10.0 ** rng.uniform(-5.0, 5.0, (6, rows))
    t = rng.standard_normal((6, rows)) * D
    for p in range(3, 6):
        G[p, rng.integers(rows)] = 0.0
    return G, D, t


@pytest.fixture(scope="module")
def device_runs(probe):
    return {s: (_inputs(*s), probe.gdg(*_inputs(*s))) for s in SHAPES}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=[f"nv{nv}-nks{nks}" for nv, nks in SHAPES])
def test_gdg_against_numpy(probe, device_runs, shape):
    nv, nks = shape
    (G, D, t), (mf, gdr) = device_runs[shape]
    M = np.einsum("pfi,pf,pfj->pij", G, D, G)
    Mabs = np.einsum("pfi,pf,pfj->pij", np.abs(G), np.abs(D), np.abs(G))
    g = np.einsum("pfi,pf->pi", G, t)
    gabs = np.einsum("pfi,pf->pi", np.abs(G), np.abs(t))
    got = mf[:, :, :nv]
    worst = float(np.max(np.abs(got - M) / (EPS * Mabs)))
    worst_g = float(np.max(np.abs(gdr - g) / (EPS * gabs)))
    print(f"nv {nv} nks {nks}: max |M - numpy| / (eps sum|terms|) {worst:.2f}, row NV {worst_g:.2f} (bound 64)")
    assert np.all(np.abs(got - M) <= 64 * EPS * Mabs)
    assert np.all(np.abs(gdr - g) <= 64 * EPS * gabs)
    assert np.array_equal(got.view(np.uint64), got.transpose(0, 2, 1).copy().view(np.uint64))
    assert np.all(mf[:, :, nv:] == probe.sentinel)          # the reciprocal pivots' column and the padding are not the pass's


@pytest.mark.gpu
def test_sizes_that_are_not_compiled_are_refused(probe):
    z = np.zeros(64 * 64)
    assert probe.lib.mfmablocks_gdg(C.c_int(10), C.c_int(1), C.c_int(1), _d(z), _d(z), _d(z), _d(z), _d(z)) == -2
    assert probe.lib.mfmablocks_gdg(C.c_int(11), C.c_int(17), C.c_int(1), _d(z), _d(z), _d(z), _d(z), _d(z)) == -3
    assert probe.lib.mfmablocks_raw(C.c_int(0), _d(z), _d(z), _d(z), _d(z)) == -3


@pytest.mark.gpu
def test_device_equals_the_host_emulation(device_runs, tmp_path):
    exe = hostsim.build("mfmablocks", ["plain"])["mfmablocks"]
    for (nv, nks), ((G, D, t), (mf, gdr)) in device_runs.items():
        inp, outp = str(tmp_path / f"in_{nv}_{nks}.bin"), str(tmp_path / f"out_{nv}_{nks}.bin")
        np.concatenate([np.concatenate([G[p].ravel(), D[p], t[p]]) for p in range(G.shape[0])]).tofile(inp)
        res = subprocess.run([exe, str(nv), str(nks), str(G.shape[0]), inp, outp], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr[-2000:]
        host = np.fromfile(outp, dtype=np.float64).reshape(G.shape[0], -1)
        ldm = (nv + 1) | 1
        assert np.array_equal(host[:, :nv * ldm].view(np.uint64), mf.reshape(G.shape[0], -1).view(np.uint64)), (nv, nks)
        assert np.array_equal(host[:, nv * ldm:].view(np.uint64), gdr.view(np.uint64)), (nv, nks)
