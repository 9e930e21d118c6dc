"""Every compiled QP kernel instantiation has a case of tests/shape_cases.py, and every case lands where the table says (no GPU:
host-only handles, device = -1, make the same dispatch decision as a device handle; the compiled names are read from the
library's code objects, scripts/code_object_notes.py).  A shape added to TMPC_SHAPES without a case fails here, and so does a
case that drifts off its edge or is deleted."""
import importlib.util
import os
import re

import pytest

import common
import shape_cases
from LinearMPCOverNetworks import _native

ROOT = os.path.dirname(common.PKG)
spec = importlib.util.spec_from_file_location("code_object_notes", os.path.join(ROOT, "scripts", "code_object_notes.py"))
notes = importlib.util.module_from_spec(spec)
spec.loader.exec_module(notes)

CASES = shape_cases.CASES


def _w(*shape):
    return "tmpc::solve_kernel<" + ",".join(map(str, shape)) + ">"


def _b(t):
    return f"tmpc::solve_block_kernel<{t}>"


# The edges the table must hold, as (kernel, nv, condensed rows): nv == NVP and the smallest nv a problem family brings to a
# shape, single-row slots exactly full (rows == 64 DS) and the first row count past the narrower shape, both ends of every
# block tile.  Every case holds one of these alone; deleting one fails test_every_edge_has_a_case.
EDGES = {
    (_w(8, 0, 2, 0, 0, 0, 8), 6, 90), (_w(8, 0, 2, 0, 0, 0, 8), 8, 102), (_w(8, 0, 2, 0, 0, 0, 8), 8, 128),
    (_w(8, 0, 4, 0, 0, 0, 8), 8, 135), (_w(8, 0, 4, 0, 0, 0, 8), 8, 254), (_w(8, 0, 4, 0, 0, 0, 8), 8, 256),
    (_w(12, 0, 2, 0, 0, 0, 8), 10, 72), (_w(12, 0, 2, 0, 0, 0, 8), 12, 126), (_w(12, 0, 2, 0, 0, 0, 8), 10, 128),
    (_w(12, 0, 4, 0, 0, 0, 4), 12, 145), (_w(12, 0, 4, 0, 0, 0, 4), 12, 255), (_w(12, 0, 4, 0, 0, 0, 4), 12, 256),
    (_w(16, 0, 2, 0, 0, 0, 4), 14, 96), (_w(16, 0, 2, 0, 0, 0, 4), 16, 108), (_w(16, 0, 2, 0, 0, 0, 4), 13, 126),
    (_w(16, 0, 4, 0, 0, 0, 4), 14, 138), (_w(16, 0, 4, 0, 0, 0, 4), 16, 150),
    (_w(11, 1, 0, 5, 4, 0, 8), 8, 474), (_w(11, 1, 0, 5, 4, 0, 8), 11, 504), (_w(12, 1, 0, 5, 4, 0, 8), 12, 514),
    (_w(22, 2, 0, 5, 4, 0, 4), 13, 524), (_w(22, 2, 0, 5, 4, 0, 4), 22, 614),
    (_w(24, 2, 0, 5, 4, 0, 4), 23, 624), (_w(24, 2, 0, 5, 4, 0, 4), 24, 634),
    (_b(1), 4, 434), (_b(1), 16, 150), (_b(2), 17, 156), (_b(2), 32, 246), (_b(2), 25, 644),
    (_b(4), 33, 252), (_b(4), 64, 438), (_b(8), 65, 444), (_b(8), 128, 822),
}
# ... and those of the extended controller (two problems per handle; its closed loop runs closed_loop_step_kernel)
EXT_EDGES = {
    (_w(11, 1, 0, 5, 4, 0, 8), 10, 494), (_w(15, 1, 0, 4, 7, 0, 4), 14, 946), (_w(15, 1, 0, 4, 7, 0, 4), 15, 956),
    (_w(12, 1, 0, 5, 4, 0, 8), 12, 514), (_w(16, 1, 0, 4, 7, 0, 4), 16, 966),
    (_w(26, 2, 0, 4, 7, 0, 4), 17, 976), (_w(26, 2, 0, 4, 7, 0, 4), 26, 1066),
}
ALL_EDGES = {e + (False,) for e in EDGES} | {e + (True,) for e in EXT_EDGES}


def _compiled():
    """Normalised names of the solve_kernel / solve_block_kernel instantiations inside lib/libtmpc_hip.so."""
    ks = notes.kernels(os.path.join(common.PKG, "lib", "libtmpc_hip.so"))
    out = set()
    for n in notes.demangle(list(ks)).values():
        m = re.search(r"::(solve_kernel|solve_block_kernel)<([^>]*)>", n)
        if m:
            out.add("tmpc::" + m.group(1) + "<" + "".join(m.group(2).split()) + ">")
    return out


def _edges_of(c):
    return {(k, nv, rows, c.extended) for k, (nv, rows) in zip(c.kernels, c.dims)}


@pytest.fixture(scope="module")
def landed(hip_lib):
    """case id -> (kernel names, (nv, rows), kernel paths) per variant, on host-only handles."""
    res = {}
    for c in CASES:
        m = c.build(device=-1)
        try:
            h = m._handle
            assert h.nvariants == len(c.kernels), (c.id, h.nvariants)
            res[c.id] = (tuple(_native.kernel_name(h, v) for v in range(h.nvariants)),
                         tuple(_native.get_dims(h, v)[:2] for v in range(h.nvariants)),
                         tuple(_native.get_kernel_path(h, v) for v in range(h.nvariants)))
        finally:
            m._close()
    return res


def test_case_ids_are_unique():
    assert len({c.id for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_lands_on_its_kernel(landed, case):
    names, dims, paths = landed[case.id]
    assert names == case.kernels, (case.id, names)
    assert dims == case.dims, (case.id, dims)
    assert paths == tuple("block" if "block" in k else "wave" for k in case.kernels), (case.id, paths)


def test_the_table_covers_exactly_the_compiled_kernels():
    compiled = _compiled()
    assert len([n for n in compiled if "::solve_kernel<" in n]) == 13 and len([n for n in compiled if "block" in n]) == 4, sorted(compiled)
    covered = {k for c in CASES for k in c.kernels}
    assert covered == compiled, (sorted(compiled - covered), sorted(covered - compiled))


def test_every_edge_has_a_case():
    have = set().union(*(_edges_of(c) for c in CASES))
    assert ALL_EDGES <= have, sorted(ALL_EDGES - have)
    for c in CASES:
        others = set().union(*(_edges_of(o) for o in CASES if o is not c))
        assert (_edges_of(c) & ALL_EDGES) - others, f"{c.id}: holds no edge of its own"


def test_the_edges_are_where_the_shapes_end():
    """What makes them edges, from the kernel names alone: for every wave shape a case with nv == NVP and, for the four
    dense-single shapes the polygon regulator reaches, one with exactly 64 DS rows; for every block tile T a case at
    nv = 16 T and, from T = 2 on, one at the first nv past the narrower tile."""
    have = set().union(*(_edges_of(c) for c in CASES))
    for name in _compiled():
        t = [int(a) for a in name[name.index("<") + 1:-1].split(",")]
        if "::solve_kernel<" in name:
            assert any(k == name and nv == t[0] for k, nv, _, _ in have), name
            if t[1] == 0 and t[3] == 0 and t[0] in (8, 12):
                assert any(k == name and rows == 64 * t[2] for k, _, rows, _ in have), name
        else:
            T = t[0]
            assert any(k == name and nv == 16 * T for k, nv, _, _ in have), name
            if T > 1:
                assert any(k == name and nv == 8 * T + 1 for k, nv, _, _ in have), name
    # the forced block path really moves a wave-shape problem: the same QP has a wave case
    forced = [c for c in CASES if c.path == "block"]
    assert forced and all(any(o.path == "auto" and o.wave and o.dims == c.dims for o in CASES) for c in forced)
