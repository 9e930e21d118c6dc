"""TEST INFRASTRUCTURE: drives tests/wavesim/lawhop_* (the explicit-law kernel of csrc/tmpc_law.hip with the hops of its search on the
host execution model; the file format is described in lawhop_main.cpp)."""

import numpy as np

from law_case import pack_table
from hostsim import run_files


def keys_of(table):
    """The keys of a table of explicit_law.region_law dicts (None: a region without a key) and their hash, as csrc/tmpc_law.cpp builds them."""
    from LinearMPCOverNetworks import explicit_law as E
    keys = np.array([E.NO_KEY if t is None else E.signature_key(t["rows"]) for t in table], dtype=np.uint64)
    return keys, E.hash_slots(keys)


def run(binary, table, P, hint=None, order=None, max_tries=0, max_hops=0, nc=None, env=None):
    """One launch; arguments as LinearMPCOverNetworks.explicit_law.locate -> dict(y, region, tries, hits, stats, stderr)."""
    first = next(t for t in table if t is not None)
    (ny, npar), nrow = first["Ky"].shape, first["s"].shape[0]
    P = np.asarray(P, dtype=np.float64).reshape(-1, npar)
    B, R = P.shape[0], len(table)
    order = np.arange(R, dtype=np.int32) if order is None else np.asarray(order, dtype=np.int32).reshape(-1)
    S, K = pack_table(table, npar, ny, nrow)
    keys, slot = keys_of(table)
    payload = [np.array([npar, ny, nrow, R, len(order), B, max_tries, int(hint is not None), max_hops, nrow if nc is None else nc, len(slot), 0], dtype=np.int64),
               S, K, order, P]
    if hint is not None:
        payload.append(np.ascontiguousarray(np.broadcast_to(np.asarray(hint, dtype=np.int32).reshape(-1), (B,))))
    payload += [keys, slot]
    raw, err = run_files(binary, "run", payload, env)
    y = np.frombuffer(raw, dtype=np.float64, count=B * ny).reshape(B, ny).copy()
    off = 8 * B * ny
    region = np.frombuffer(raw, dtype=np.int32, count=B, offset=off).copy()
    tries = np.frombuffer(raw, dtype=np.int32, count=B, offset=off + 4 * B).copy()
    hits = np.frombuffer(raw, dtype=np.uint64, count=R, offset=off + 8 * B).copy()
    stats = np.frombuffer(raw, dtype=np.uint64, count=6, offset=off + 8 * B + 8 * R).astype(np.int64)
    assert off + 8 * B + 8 * R + 48 == len(raw), (off, len(raw))
    return dict(y=y, region=region, tries=tries, hits=hits, stats=stats, stderr=err)
