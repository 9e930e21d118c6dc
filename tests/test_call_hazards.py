"""The overlap predicate behind the two launch lanes of a device handle (csrc/tmpc_hazard.hpp, through tmpc_debug_calls_conflict): a
tmpc_solve_batch_device call may run beside an unfinished earlier one only if it reads nothing that call writes (RAW), writes nothing it
writes (WAW) and writes nothing it reads (WAR).  The addresses are made up and never dereferenced.  CPU only."""
import itertools

import pytest

NX, NU, N, B = 4, 1, 10, 8
# bytes per instance of every argument (include/tmpc.h: tmpc_solve_batch)
WIDTH = {"x_k": 8 * NX, "ref": 8 * NX, "variant": 1, "u_nom": 8 * N * NU, "x_nom0": 8 * NX, "xu_ss": 8 * (NX + NU),
         "x_nom": 8 * (N + 1) * NX, "status": 4, "iters": 4}
READS, WRITES = ("x_k", "ref", "variant"), ("u_nom", "x_nom0", "xu_ss", "x_nom", "status", "iters")


def call(base, b=B):
    """every argument in a block of its own, 64 KiB apart, from `base` on: no two of them overlap for b <= 8"""
    return {k: base + 0x10000 * i for i, k in enumerate(WIDTH)}


@pytest.fixture(scope="module")
def conflict(hip_lib):
    assert set(hip_lib.SOLVE_POINTERS) == set(WIDTH)

    def f(a, b, Ba=B, Bb=B):
        ab, ba = hip_lib.calls_conflict(NX, NU, N, Ba, a, Bb, b), hip_lib.calls_conflict(NX, NU, N, Bb, b, Ba, a)
        assert ab == ba, "a hazard does not depend on which call came first"
        return ab
    return f


def test_disjoint_calls_do_not_conflict(conflict):
    assert not conflict(call(0x1000000), call(0x2000000))
    # allocations that interleave (the hulls of the two calls overlap, no two ranges do)
    assert not conflict(call(0x1000000), call(0x1008000))


def test_shared_inputs_are_no_hazard(conflict):
    a, b = call(0x1000000), call(0x2000000)
    for k in READS:
        b[k] = a[k]
    assert not conflict(a, b)


@pytest.mark.parametrize("r,w", list(itertools.product(READS, WRITES)))
def test_raw_and_war(conflict, r, w):
    """a call that reads (RAW) what the other one writes; seen from the other side it is the WAR case"""
    a, b = call(0x1000000), call(0x2000000)
    b[r] = a[w]
    assert conflict(a, b)


@pytest.mark.parametrize("w1,w2", list(itertools.product(WRITES, WRITES)))
def test_waw(conflict, w1, w2):
    a, b = call(0x1000000), call(0x2000000)
    b[w2] = a[w1]
    assert conflict(a, b)


def test_nested_ranges(conflict):
    a, b = call(0x1000000), call(0x2000000)
    b["status"] = a["x_nom"] + 1000               # 32 bytes well inside the 2816 of x_nom
    assert conflict(a, b)
    a, b = call(0x1000000), call(0x2000000)
    b["x_nom"] = a["x_k"] - 1000                  # ... and a range that contains one of the other call's
    assert conflict(a, b)


def test_ranges_that_touch_at_a_boundary(conflict):
    for k in WRITES:
        a, b = call(0x1000000), call(0x2000000)
        b["x_k"] = a[k] + B * WIDTH[k]            # begins where the other call's output ends
        assert not conflict(a, b), k
        b["x_k"] -= 1                             # ... and one byte earlier
        assert conflict(a, b), k
        b["x_k"] = a[k] - B * WIDTH["x_k"]        # ends where it begins
        assert not conflict(a, b), k
        b["x_k"] += 1
        assert conflict(a, b), k


def test_zero_length_ranges(conflict):
    a = call(0x1000000)
    assert conflict(a, dict(a))
    assert not conflict(a, dict(a), Bb=0)         # a call over no instance touches nothing, whatever its pointers
    assert not conflict(a, dict(a), Ba=0, Bb=0)
    b = call(0x2000000)
    b["x_k"] = a["u_nom"] + 8                     # an empty range inside a range is no overlap either
    assert conflict(a, b) and not conflict(a, b, Bb=0)


def test_null_optional_pointers(conflict):
    """x_nom0, xu_ss, x_nom, variant (and ref on a regulator handle) may be NULL: a NULL pointer is no range, not one at address 0"""
    a, b = call(0x1000000), call(0x2000000)
    for k in ("variant", "x_nom0", "xu_ss", "x_nom", "ref"):
        a[k] = b[k] = None
    assert not conflict(a, b)
    del a["x_nom"], b["variant"]                  # (a missing name is NULL as well)
    assert not conflict(a, b)
    # a buffer at a low address against the other call's NULL pointers
    c = call(0x2000000)
    c["u_nom"] = 16
    assert not conflict(a, c)
    # the pointers that are given still count
    b["x_k"] = a["u_nom"]
    assert conflict(a, b)


def test_views_at_an_offset_into_one_allocation(conflict):
    """both calls work on slices of the same arrays: rows [0, B) and rows [first, first + B)"""
    base = call(0x1000000)
    def rows(first):
        return {k: base[k] + first * WIDTH[k] for k in WIDTH}
    assert not conflict(rows(0), rows(B))
    assert not conflict(rows(0), rows(3 * B))
    assert conflict(rows(0), rows(B - 1))         # one shared row
    assert conflict(rows(0), rows(0))
    # the later call's input is the earlier call's x_nom0 seen through an offset view of a larger array
    a, b = call(0x1000000), call(0x2000000)
    b["x_k"] = a["x_nom0"] + 5 * WIDTH["x_nom0"]
    assert conflict(a, b)
    assert not conflict(a, b, Ba=5)               # the earlier call wrote rows [0, 5) only
