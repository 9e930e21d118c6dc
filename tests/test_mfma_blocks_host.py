"""wv::gdg_blocks (csrc/tmpc_wave.hpp) on the host execution model, no GPU: tests/wavesim/mfmablocks_main.cpp as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer (skipped where the host toolchain lacks their runtime), against numpy in float64 -- the shapes of
tests/test_mfma_blocks_gpu.py and NV = 22 (21 blocks, six instructions per k-step, two of them with row NV), which no kernel shape takes yet."""
import os
import subprocess

import numpy as np
import pytest

import test_mfma_blocks_gpu as dev

import hostsim  # noqa: E402  (tests/wavesim: test_mfma_blocks_gpu puts it on sys.path)

SHAPES = dev.SHAPES + [(22, 2), (22, 5)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = hostsim.binaries_or_skip(tmp_path_factory, "mfmablocks", ["asan"])["mfmablocks_asan"]
    return exe, tmp_path_factory.mktemp("mfmablocks_host")


@pytest.mark.parametrize("shape", SHAPES, ids=[f"nv{nv}-nks{nks}" for nv, nks in SHAPES])
def test_gdg_on_the_host_model(program, shape):
    exe, d = program
    nv, nks = shape
    G, D, t = dev._inputs(nv, nks)
    P, ldm = G.shape[0], (nv + 1) | 1
    inp, outp = str(d / f"in_{nv}_{nks}.bin"), str(d / f"out_{nv}_{nks}.bin")
    np.concatenate([np.concatenate([G[p].ravel(), D[p], t[p]]) for p in range(P)]).tofile(inp)
    res = subprocess.run([exe, str(nv), str(nks), str(P), inp, outp], capture_output=True, text=True, timeout=300, env=dict(os.environ, **hostsim.SAN_ENV))
    assert res.returncode == 0, res.stderr[-4000:]
    hostsim.assert_clean(res.stderr)
    host = np.fromfile(outp, dtype=np.float64).reshape(P, -1)
    mf, gdr = host[:, :nv * ldm].reshape(P, nv, ldm), host[:, nv * ldm:]
    M = np.einsum("pfi,pf,pfj->pij", G, D, G)
    Mabs = np.einsum("pfi,pf,pfj->pij", np.abs(G), np.abs(D), np.abs(G))
    g = np.einsum("pfi,pf->pi", G, t)
    gabs = np.einsum("pfi,pf->pi", np.abs(G), np.abs(t))
    got = mf[:, :, :nv]
    assert np.all(np.abs(got - M) <= 64 * dev.EPS * Mabs)
    assert np.all(np.abs(gdr - g) <= 64 * dev.EPS * gabs)
    assert np.array_equal(got, got.transpose(0, 2, 1))
    assert np.all(mf[:, :, nv:] == -7.0e77)
