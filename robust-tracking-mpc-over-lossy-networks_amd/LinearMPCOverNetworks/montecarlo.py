"""Sharding of a Monte-Carlo sweep over ranks (one process per GPU) and the one collective of
the path: gathering per-trajectory statistics.

The reference runs `for i in p_loss: for l_mc in N_MC: for t in T:` in one Python process
(results_linear_system.py:165-209); trajectories never interact (estimator/actuator are
re-created per run, :186-188), so they are sharded with no data-path collective.  What is
exchanged is what the script aggregates afterwards (:291 tracking error, :268-270 failure
counts, :305-315 timing/iteration statistics): a few numbers per trajectory, once per sweep.
"""
from __future__ import annotations

import numpy as np


def trajectory_table(p_loss, n_mc: int):
    """Global trajectory index -> (p_loss index, seed index), p_loss-minor so that every
    contiguous shard sees all loss rates (balanced iteration counts)."""
    p_loss = np.asarray(p_loss, dtype=np.float64)
    n = len(p_loss) * int(n_mc)
    g = np.arange(n)
    return g % len(p_loss), g // len(p_loss)


def shard_bounds(n_items: int, rank: int, world: int):
    """Contiguous shard [lo, hi) of rank; sizes differ by at most one."""
    if not (0 <= rank < world):
        raise ValueError("rank out of range")
    base, rem = divmod(int(n_items), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def gather_statistics(local, n_total: int, rank: int, world: int, group=None, force_collective: bool = False):
    """All-gather of a (n_local, k) tensor of per-trajectory statistics into the global
    (n_total, k) table, identical on every rank.  Backend-agnostic: `nccl` (= RCCL over xGMI) on
    the GPUs, `gloo` in the CPU tests.  Shards of unequal size are padded to the largest.
    force_collective: a one-rank run goes through the collective as well (needs an initialised process group;
    the single-GPU rehearsal of the RCCL path)."""
    import torch
    import torch.distributed as dist
    if world == 1 and not force_collective:
        return local
    sizes = [shard_bounds(n_total, r, world)[1] - shard_bounds(n_total, r, world)[0] for r in range(world)]
    if local.shape[0] != sizes[rank]:
        raise ValueError(f"rank {rank} holds {local.shape[0]} rows, expected {sizes[rank]}")
    m = max(sizes)
    pad = torch.zeros((m,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    pad[:local.shape[0]] = local
    out = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(out, pad, group=group)
    return torch.cat([o[:s] for o, s in zip(out, sizes)], dim=0)


# --------------------------------------------------------------------------- closed loop
def draw_realisations(n_traj: int, T: int, w_bound, seed: int = 20240301, first: int = 0):
    """Per-trajectory random streams (uniforms for theta, gamma and the disturbance), so that a
    trajectory's realisation does not depend on how the sweep is sharded.  Trajectory g uses
    SeedSequence(seed, spawn_key=(g,)).  (The reference draws from three shared generators in loop
    order, results_linear_system.py:21-23,218-233; that order cannot be kept under sharding.)"""
    w_bound = np.asarray(w_bound, dtype=np.float64)
    th = np.empty((n_traj, T))
    ga = np.empty((n_traj, T))
    w = np.empty((n_traj, T, w_bound.size))
    for i in range(n_traj):
        rng = np.random.default_rng(np.random.SeedSequence(seed, spawn_key=(first + i,)))
        th[i] = rng.uniform(size=T)
        ga[i] = rng.uniform(size=T)
        w[i] = rng.uniform(-1.0, 1.0, size=(T, w_bound.size)) * w_bound
    return th, ga, w


# Philox4x64-10 (Salmon et al., SC'11), the numpy twin of the device generator in csrc/tmpc_mc.hip (tmpc_mc_set_device_rng).
_PHILOX_M0, _PHILOX_M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B


def _mulhilo64(a, b: int):
    """(high, low) 64-bit halves of a * b for a uint64 array a and a 64-bit constant b."""
    m32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    a0, a1 = a & m32, a >> s32
    b0, b1 = np.uint64(b & 0xFFFFFFFF), np.uint64(b >> 32)
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    carry = ((p00 >> s32) + (p01 & m32) + (p10 & m32)) >> s32
    return p11 + (p01 >> s32) + (p10 >> s32) + carry, a * np.uint64(b)


def philox4x64(c0, c1, k0, k1):
    """Ten rounds of Philox-4x64 on the counter (c0, c1, 0, 0) with the key (k0, k1), vectorised: arrays that broadcast
    against each other -> (4, ...) uint64.  numpy.random.Philox(key=[k0, k1], counter=[c0 - 1, c1, 0, 0]).random_raw(4) gives
    the same four words (numpy increments the counter before it generates; tests/test_condense.py pins this)."""
    with np.errstate(over="ignore"):
        c0, c1, k0, k1 = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) for v in (c0, c1, k0, k1)))
        c = [c0.copy(), c1.copy(), np.zeros_like(c0), np.zeros_like(c0)]
        k0, k1 = k0.copy(), k1.copy()
        for _ in range(10):
            hi0, lo0 = _mulhilo64(c[0], _PHILOX_M0)
            hi1, lo1 = _mulhilo64(c[2], _PHILOX_M1)
            c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
            k0 = k0 + np.uint64(_PHILOX_W0)
            k1 = k1 + np.uint64(_PHILOX_W1)
    return np.stack(c)


def draw_realisations_philox(n_traj: int, T: int, w_bound, seed: int = 20240301, first: int = 0):
    """The realisations tmpc_mc_run draws on the device with tmpc_mc_set_device_rng(seed, first, w_bound), reproduced on the
    host (include/tmpc.h): trajectory g = first + i, step t: Philox4x64-10 with key (seed, g), counter (t, j, 0, 0);
    block 0 = [theta, gamma, w_0, w_1], block j = w_{4j-2} .. w_{4j+1}; u = (x >> 11) 2^-53; w_i = w_bound_i (2 u - 1).
    Like draw_realisations, a trajectory's stream does not depend on how the sweep is sharded."""
    w_bound = np.asarray(w_bound, dtype=np.float64).reshape(-1)
    nx = w_bound.size
    g = (np.uint64(first) + np.arange(n_traj, dtype=np.uint64))[:, None]
    t = np.arange(T, dtype=np.uint64)[None, :]
    nblk = (nx + 2 + 3) // 4
    words = np.concatenate([philox4x64(t, np.uint64(j), np.uint64(seed), g) for j in range(nblk)], axis=0)     # (4 nblk, n, T)
    u = (words >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    th, ga = u[0], u[1]
    w = np.moveaxis(u[2:2 + nx], 0, -1) * 2.0 - 1.0
    return np.ascontiguousarray(th), np.ascontiguousarray(ga), np.ascontiguousarray(w * w_bound)


def draw_realisations_reference_order(p_loss, n_mc: int, T: int, w_bound, seeds=(679, 347, 124)):
    """The realisations of the reference's own experiment: three shared generators -- disturbance 679, gamma 347,
    theta 124 (results_linear_system.py:21-23) -- consumed in loop order over (loss rate i, run l_mc, step t): one theta
    and one gamma uniform per step t >= 1 (:218-226, the first transmission always succeeds, :211-214) and nx disturbance
    components per step (:229-233).  Only valid for the whole sweep on one rank (the order is the point).

    Returns (p (B,), th (B,T), ga (B,T), w (B,T,nx)), B = len(p_loss) * n_mc in (i, l_mc) order; the t = 0 entries
    of th/ga are 1.0 (never below a loss probability)."""
    p_loss = np.asarray(p_loss, dtype=np.float64)
    w_bound = np.asarray(w_bound, dtype=np.float64)
    rng_w, rng_gamma, rng_theta = (np.random.default_rng(sd) for sd in seeds)
    nb = len(p_loss) * int(n_mc)
    th = np.ones((nb, T))
    ga = np.ones((nb, T))
    th[:, 1:] = rng_theta.uniform(size=(nb, T - 1))
    ga[:, 1:] = rng_gamma.uniform(size=(nb, T - 1))
    w = rng_w.uniform(-w_bound, w_bound, size=(nb, T, w_bound.size))
    return np.repeat(p_loss, int(n_mc)), th, ga, w


# --------------------------------------------------------------------------- bursty losses: the Gilbert-Elliott channel
def channel_parameters(channel, n_traj=None):
    """The `channel` argument of the closed loops -> (p_gb, p_bg, e_g, e_b), four float64 arrays of n_traj entries: a dict with these
    keys (burst_channel returns one) or a sequence in this order; scalars are shared by the batch."""
    if isinstance(channel, dict):
        channel = [channel[k] for k in ("p_gb", "p_bg", "e_g", "e_b")]
    par = [np.asarray(v, dtype=np.float64).reshape(-1) for v in channel]
    if len(par) != 4:
        raise ValueError("channel: (p_gb, p_bg, e_g, e_b)")
    n = max(v.size for v in par) if n_traj is None else int(n_traj)
    if any(v.size not in (1, n) for v in par):
        raise ValueError(f"channel: every parameter is a scalar or holds one entry per trajectory ({n})")
    par = [np.ascontiguousarray(np.broadcast_to(v, (n,))) for v in par]
    if any(not np.all((v >= 0.0) & (v <= 1.0)) for v in par):
        raise ValueError("channel: p_gb, p_bg, e_g, e_b are probabilities")
    return tuple(par)


def gilbert_elliott_thresholds(p_gb, p_bg, e_g, e_b):
    """The thresholds the device compares a link's uniform against (include/tmpc.h: tmpc_mc_set_channel), (n, 2, 3): with
    a = P(B | previous state) = p_gb after G (index 0), 1 - p_bg after B (index 1), thr = [a e_b, a, a + (1 - a) e_g]; every product
    and sum rounded on its own, as the library computes them (tmpc_mc_get_channel returns the same bits)."""
    p_gb, p_bg, e_g, e_b = channel_parameters((p_gb, p_bg, e_g, e_b))
    a = np.stack([p_gb, 1.0 - p_bg], axis=1)                                   # (n, 2)
    return np.ascontiguousarray(np.stack([a * e_b[:, None], a, a + (1.0 - a) * e_g[:, None]], axis=2))


def channel_arrivals(channel, th_u, ga_u):
    """The numpy twin of the device's loss channel: channel (see channel_parameters) and the uniforms th_u, ga_u (B, T) of the two
    links -> dict(theta, gamma: arrival flags (B, T), 1 = arrives; state_up, state_down: the links' states after the draw of step t
    (B, T), 0 = G, 1 = B).  u < thr[0]: (B, lost); else u < thr[1]: (B, arrives); else u < thr[2]: (G, lost); else (G, arrives) --
    strict comparisons; both links start in G; at t = 0 the packet arrives and the state stays."""
    th_u, ga_u = np.asarray(th_u, dtype=np.float64), np.asarray(ga_u, dtype=np.float64)
    nb, T = th_u.shape
    thr = gilbert_elliott_thresholds(*channel_parameters(channel, nb))
    rows = np.arange(nb)
    out = {}
    for name, sname, u in (("theta", "state_up", th_u), ("gamma", "state_down", ga_u)):
        flag = np.ones((nb, T), dtype=np.uint8)
        state = np.zeros((nb, T), dtype=np.uint8)
        if nb < 8:                                # a few long chains: plain Python floats, a trajectory at a time -- the table below, entry for entry
            for b in range(nb):
                tb, ub, s = thr[b].tolist(), u[b].tolist(), 0
                for t in range(1, T):
                    r, v = tb[s], ub[t]
                    lost = 1 if v < r[0] else (0 if v < r[1] else (1 if v < r[2] else 0))
                    s = 1 if (v < r[0] or v < r[1]) else 0
                    flag[b, t], state[b, t] = 1 - lost, s
            out[name], out[sname] = flag, state
            continue
        s = np.zeros(nb, dtype=np.int64)
        for t in range(1, T):
            r = thr[rows, s]                                                   # (B, 3): the thresholds of the previous state
            lost = np.where(u[:, t] < r[:, 0], 1, np.where(u[:, t] < r[:, 1], 0, np.where(u[:, t] < r[:, 2], 1, 0)))
            s = ((u[:, t] < r[:, 0]) | (u[:, t] < r[:, 1])).astype(np.int64)
            flag[:, t], state[:, t] = 1 - lost, s
        out[name], out[sname] = flag, state
    return out


def burst_channel(loss_rate, mean_burst):
    """The simple Gilbert channel (e_g = 0, e_b = 1: every packet in B is lost, none in G) with stationary loss rate
    p_gb / (p_gb + p_bg) = loss_rate and mean burst length 1 / p_bg = mean_burst, as the `channel` dict of the closed loops.
    mean_burst = 1 / (1 - loss_rate) gives independent losses."""
    loss_rate, mean_burst = np.broadcast_arrays(np.asarray(loss_rate, dtype=np.float64), np.asarray(mean_burst, dtype=np.float64))
    if np.any(mean_burst < 1.0) or np.any((loss_rate < 0.0) | (loss_rate >= 1.0)):
        raise ValueError("burst_channel: need mean_burst >= 1 and 0 <= loss_rate < 1")
    p_bg = 1.0 / mean_burst
    p_gb = loss_rate * p_bg / (1.0 - loss_rate)
    if np.any(p_gb > 1.0):
        raise ValueError("burst_channel: this loss rate needs longer bursts (p_gb = loss_rate / ((1 - loss_rate) mean_burst) > 1)")
    return dict(p_gb=p_gb.reshape(-1).copy(), p_bg=p_bg.reshape(-1).copy(), e_g=np.zeros(p_gb.size), e_b=np.ones(p_gb.size))


def _loss_flags(channel, p_loss, th_u, ga_u):
    """Arrival flags (B, T) of the two links as the loops draw them: the channel's, or the Bernoulli model's u >= p_loss; t = 0 arrives."""
    if channel is not None:
        arr = channel_arrivals(channel, th_u, ga_u)
        return arr["theta"].astype(np.int64), arr["gamma"].astype(np.int64)
    theta = np.where(th_u < p_loss[:, None], 0, 1)                             # :211-226, strict <
    gamma = np.where(ga_u < p_loss[:, None], 0, 1)
    theta[:, 0] = gamma[:, 0] = 1
    return theta, gamma


# --------------------------------------------------------------------------- the per-step record and its ensemble statistics
# the word of the per-step record (include/tmpc.h: TMPC_SER_*)
SER_ALIVE, SER_LOST_UP, SER_LOST_DOWN, SER_ADOPTED, SER_TUBE, SER_NOT_OPTIMAL, SER_OVERRUN = (1 << i for i in range(7))
SER_ITERS_SHIFT, SER_AGE_SHIFT, SER_SATURATE, SER_MAX_Q = 8, 20, 4095, 16
SERIES_FLAGS = ("alive", "lost_up", "lost_down", "adopted", "tube", "not_optimal", "overrun")
SERIES_INT_TABLES = ("n_alive", "n_nan", "lost_up", "lost_down", "adopted", "tube", "not_optimal", "overrun", "age_max", "age_sum",
                     "iters_max", "iters_sum")


def pack_series_word(alive, lost_up=0, lost_down=0, adopted=0, tube=0, not_optimal=0, overrun=0, iters=0, age=0):
    """The packed word of the loops' per-step record (include/tmpc.h: TMPC_SER_*): bits 0-6 the flags in the order of the arguments,
    bits 8-19 the iterations and bits 20-31 the age t - s_t, each saturating at 4095.  Arrays broadcast; returns uint32."""
    flags = (alive, lost_up, lost_down, adopted, tube, not_optimal, overrun)
    word = np.zeros(np.broadcast(*flags, iters, age).shape, dtype=np.uint32)
    for i, f in enumerate(flags):
        word |= (np.asarray(f).astype(bool).astype(np.uint32) << np.uint32(i))
    word |= np.clip(np.asarray(iters, dtype=np.int64), 0, SER_SATURATE).astype(np.uint32) << np.uint32(SER_ITERS_SHIFT)
    word |= np.clip(np.asarray(age, dtype=np.int64), 0, SER_SATURATE).astype(np.uint32) << np.uint32(SER_AGE_SHIFT)
    return word


def unpack_series_word(word) -> dict:
    """The fields of pack_series_word: the seven flags as bool arrays, iters and age as int32."""
    word = np.asarray(word, dtype=np.uint32)
    out = {name: ((word >> np.uint32(i)) & np.uint32(1)).astype(bool) for i, name in enumerate(SERIES_FLAGS)}
    out["iters"] = ((word >> np.uint32(SER_ITERS_SHIFT)) & np.uint32(SER_SATURATE)).astype(np.int32)
    out["age"] = (word >> np.uint32(SER_AGE_SHIFT)).astype(np.int32)
    return out


def decode_series(e, word) -> dict:
    """The `series` entry of a loop's result: e and word (T, B) and the word's fields (unpack_series_word)."""
    return dict(e=e, word=word, **unpack_series_word(word))


def series_stats(e, word, group=None, q=(0.5, 0.95), G=None) -> dict:
    """The numpy twin of the device reduction (include/tmpc.h: tmpc_series_stats): per time step t and group g the statistics of the
    entries [t][b] of the members b of g.  e, word (T, B); group (B,) ids in [0, G) or -1 (in no group), None: one group of everybody;
    G: the number of groups (default: the largest id + 1).  An entry takes part iff its ALIVE bit is set; an alive entry with e = NaN
    is counted in n_nan and left out of the e statistics.  Quantile q of the n values that take part is the element of rank
    floor(q (n - 1)) of np.sort (NaN for n = 0, like e_max; e_sum is then 0).  Returns (T, G) tables, e_q (T, G, len(q))."""
    e = np.asarray(e, dtype=np.float64)
    word = np.asarray(word, dtype=np.uint32)
    T, B = word.shape
    group = np.zeros(B, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64).reshape(B)
    G = int(group.max()) + 1 if G is None else int(G)
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    f = unpack_series_word(word)
    out = {k: np.zeros((T, G), dtype=np.int64 if k.endswith("_sum") else np.int32) for k in SERIES_INT_TABLES}
    out["e_sum"], out["e_max"] = np.zeros((T, G)), np.full((T, G), np.nan)
    out["e_q"] = np.full((T, G, q.size), np.nan)
    for g in range(G):
        members = np.flatnonzero(group == g)
        for t in range(T):
            m = members[f["alive"][t, members]]
            out["n_alive"][t, g] = m.size
            for k in ("lost_up", "lost_down", "adopted", "tube", "not_optimal", "overrun"):
                out[k][t, g] = np.count_nonzero(f[k][t, m])
            for k in ("age", "iters"):
                out[k + "_max"][t, g] = f[k][t, m].max(initial=0)
                out[k + "_sum"][t, g] = f[k][t, m].sum(dtype=np.int64)
            v = e[t, m]
            nan = np.isnan(v)
            out["n_nan"][t, g] = np.count_nonzero(nan)
            v = np.sort(v[~nan])
            if v.size:
                out["e_sum"][t, g], out["e_max"][t, g] = v.sum(), v[-1]
                out["e_q"][t, g] = v[np.floor(q * (v.size - 1)).astype(np.int64)]
    return out


class _SeriesRecord:
    """The per-step record of the closed loops (include/tmpc.h: tmpc_mc_set_series), kept by the host twins: e (T, B) the error term
    of the step, word (T, B) the packed flags, iterations and age; entries of trajectories that did not take the step stay 0."""

    def __init__(self, T: int, nb: int, N: int):
        self.N = int(N)
        self.e, self.word = np.zeros((T, nb)), np.zeros((T, nb), dtype=np.uint32)

    def step(self, t: int, alive, a, theta_drawn, gamma_drawn, Theta, tube, status, iters, s):
        age = t - np.asarray(s, dtype=np.int64)
        w = pack_series_word(True, theta_drawn == 0, gamma_drawn == 0, np.asarray(Theta) == 1, tube, np.asarray(status) != 0, age >= self.N,
                             iters, age)
        self.e[t] = np.where(alive, a, 0.0)
        self.word[t] = np.where(alive, w, np.uint32(0))

    def result(self):
        return decode_series(self.e, self.word)


def _packets(res):
    """(U_t, x_nom_0, status, iters) of a packets_fn result: the fourth entry, the iterations of the solves, is optional (0)."""
    return res[0], res[1], res[2], (res[3] if len(res) > 3 else 0)


class _LinkStats:
    """The four link statistics of the closed loops (include/tmpc.h: tmpc_mc_get_link_stats), kept by the host twins."""

    def __init__(self, nb: int, N: int):
        self.N = int(N)
        self.lost_up, self.lost_down, self.max_gap, self.overrun = (np.zeros(nb, dtype=np.int32) for _ in range(4))

    def step(self, t: int, alive, theta_drawn, gamma_drawn, s):
        gap = t - np.asarray(s, dtype=np.int64)
        self.lost_up += (alive & (theta_drawn == 0)).astype(np.int32)
        self.lost_down += (alive & (gamma_drawn == 0)).astype(np.int32)
        self.max_gap = np.where(alive, np.maximum(self.max_gap, gap), self.max_gap).astype(np.int32)
        self.overrun += (alive & (gap >= self.N)).astype(np.int32)

    def result(self):
        return dict(lost_up=self.lost_up, lost_down=self.lost_down, max_gap=self.max_gap, overrun=self.overrun)


class LawPackets:
    """The host twin of the device loops through the explicit law (include/tmpc.h: tmpc_mc_set_law): a `packets_fn` for
    run_remote_tube_mpc that looks every step up in a table of critical regions first -- the trajectory's region of the step before as
    the hint, -1 at t = 0 and after a miss -- and hands only the misses to `packets_fn` (normally TubeTrackingMPC.determine_packets, or
    an oracle's).  It keeps the device's bookkeeping: hits (B,), tries (B,), region (B,) of the last step, the hit counters per region,
    the miss log (the first miss_capacity [x_hat | ref] and variant ids) and n_total.

    lookup(k, P (n, 2 nx), hint (n,), max_tries) -> (region (n,), tries (n,), y (n, ny)) for the instances of problem k, y = [u_nom
    (N nu) | x_nom0 (nx) | x_ss (nx) | u_ss (nu)]: `from_tables` builds one from numpy tables (explicit_law.region_law / locate, no
    GPU), `from_law` from an ExplicitLaw on the device.  K: the steady-state gain of the packet's last column u_ss + K x_ss.

    max_hops > 0 (tmpc_law_set_hops): the lookup is called as lookup(k, P, hint, max_tries, max_hops, stats) and adds the chains' six
    counters to stats = hop_stats[k] (explicit_law.HOP_STATS); tries include the chains' tests."""

    def __init__(self, packets_fn, lookup, K, N: int, max_tries: int = 0, miss_capacity: int = 0, max_hops: int = 0):
        self._fn, self._lookup, self._K, self._N = packets_fn, lookup, np.atleast_2d(np.asarray(K, dtype=np.float64)), int(N)
        self.max_tries, self.miss_capacity, self.max_hops = int(max_tries), int(miss_capacity), int(max_hops)
        self.hop_stats = np.zeros((2, 6), np.int64)
        self.hits = self.tries = self.region = None
        self.region_hits = [{}, {}]
        self.steps = 0               # instances seen: hits + misses
        self.n_total, self.miss_x, self.miss_ref, self.miss_variant = 0, [], [], []

    @classmethod
    def from_tables(cls, packets_fn, tables, K, N, orders=None, ncs=None, **kw):
        """tables: one list of explicit_law.region_law dicts per problem (a single list: problem 0).  ncs: per problem the number of rows
        that belong to a constraint (the rows of G; the parameter-only rows follow them) -- None: all of them; read by the hops only."""
        from .explicit_law import locate
        if len(tables) == 0 or isinstance(tables[0], dict) or tables[0] is None:
            tables = [tables]
        orders = [None] * len(tables) if orders is None else orders
        ncs = [None] * len(tables) if ncs is None else ([ncs] * len(tables) if np.isscalar(ncs) else ncs)

        def lookup(k, P, hint, max_tries, max_hops=0, stats=None):
            return locate(tables[k], P, hint, orders[k], max_tries, max_hops, ncs[k], stats)
        return cls(packets_fn, lookup, K, N, **kw)

    @classmethod
    def from_law(cls, mpc, law=None, **kw):
        """The table of `law` (default mpc.explicit_law()) on the device, the solver of `mpc` behind it.  max_hops: set on the law's
        handle (ExplicitLaw.set_hops), whose own counters (ExplicitLaw.hop_stats) count the chains -- hop_stats here stays zero."""
        law = mpc.explicit_law() if law is None else law
        nx = mpc._nx
        if "max_hops" in kw:
            law.set_hops(kw["max_hops"])

        def lookup(k, P, hint, max_tries, max_hops=0, stats=None):
            out = law.evaluate(P[:, :nx], P[:, nx:], variant=None if mpc._handle.nvariants == 1 else np.full(len(P), k, np.uint8),
                               hint=hint, max_tries=max_tries, want_traj=False)
            y = np.c_[out["u_nom"].reshape(len(P), -1), out["x_nom0"], out["x_ss"], out["u_ss"]]
            return out["region"], out["tries"], y
        return cls(mpc.determine_packets, lookup, mpc.get_steady_state_controller_gain(), mpc._N, **kw)

    def __call__(self, x_hat, ref, gamma=None):
        x_hat, ref = np.asarray(x_hat, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        nb, nx = x_hat.shape
        nu, N = self._K.shape[0], self._N
        if self.hits is None:
            self.hits, self.tries, self.region = np.zeros(nb, np.int32), np.zeros(nb, np.int64), np.full(nb, -1, np.int32)
        var = np.zeros(nb, np.uint8) if gamma is None else np.asarray(gamma, dtype=np.uint8)
        P = np.c_[x_hat, ref]
        region, y = np.full(nb, -1, np.int32), np.full((nb, N * nu + 2 * nx + nu), np.nan)
        for k in np.unique(var):
            sel = np.flatnonzero(var == k)
            if self.max_hops > 0:
                reg, tries, yk = self._lookup(int(k), P[sel], self.region[sel], self.max_tries, self.max_hops, self.hop_stats[int(k)])
            else:
                reg, tries, yk = self._lookup(int(k), P[sel], self.region[sel], self.max_tries)
            region[sel] = reg
            self.tries[sel] += tries
            if yk.shape[1] == y.shape[1]:            # (an empty table has no rows of y)
                y[sel] = yk
            for r in reg[reg >= 0]:
                self.region_hits[int(k)][int(r)] = self.region_hits[int(k)].get(int(r), 0) + 1
        hit = region >= 0
        self.region = region
        self.hits += hit
        self.steps += nb
        U = np.empty((nb, nu, N + 1))
        x_nom0, status, iters = np.empty((nb, nx)), np.zeros(nb, np.int32), np.zeros(nb, np.int32)
        if hit.any():
            yh = y[hit]
            u_nom, x_ss, u_ss = yh[:, :N * nu].reshape(-1, N, nu), yh[:, N * nu + nx:N * nu + 2 * nx], yh[:, N * nu + 2 * nx:]
            U[hit] = np.concatenate([u_nom, (u_ss + x_ss @ self._K.T)[:, None, :]], axis=1).transpose(0, 2, 1)
            x_nom0[hit] = yh[:, N * nu:N * nu + nx]
        miss = np.flatnonzero(~hit)
        if len(miss):
            for b in miss:
                if self.n_total < self.miss_capacity:
                    self.miss_x.append(x_hat[b].copy())
                    self.miss_ref.append(ref[b].copy())
                    self.miss_variant.append(int(var[b]))
                self.n_total += 1
            res = self._fn(x_hat[miss], ref[miss]) if gamma is None else self._fn(x_hat[miss], ref[miss], var[miss])
            Um, xm, sm, im = _packets(res)
            U[miss], x_nom0[miss], status[miss] = Um, xm, sm
            iters[miss] = im
        return U, x_nom0, status, iters

    def result(self) -> dict:
        """law_hits, law_tries, law_region as the device loops return them, and the miss log (dict of n_total, x_k, ref, variant)."""
        nx = self._K.shape[1]
        return dict(law_hits=self.hits, law_tries=self.tries, law_region=self.region, hop_stats=self.hop_stats,
                    misses=dict(n_total=self.n_total, x_k=np.array(self.miss_x, dtype=np.float64).reshape(-1, nx),
                                ref=np.array(self.miss_ref, dtype=np.float64).reshape(-1, nx),
                                variant=np.array(self.miss_variant, np.uint8)))


def run_remote_tube_mpc(packets_fn, A, B, K, K_plant, N, Z, p_loss, ref, th_u, ga_u, w, x0=None, extended: bool = False,
                        plant=None, capture=None, observer=None, channel=None, series: bool = False):
    """Closed loop of the remote tube-based MPC over a lossy network for a batch of trajectories:
    the body of the reference's Monte-Carlo loop (results_linear_system.py:209-259, 291) with the
    per-trajectory objects replaced by the batched state machines and the QP solves of one time
    step done by ONE call of `packets_fn(x_hat (B,nx), ref_t (B,nx)[, gamma (B,)]) -> (U_t (B,nu,N+1),
    x_nom0, status (B,))` -- normally `TubeTrackingMPC.determine_packets`, i.e. one kernel launch.

    extended=True is the loop of results_linear_system_with_extendedMPC.py:247-378: the controller is an
    ExtendedTubeTrackingMPC that is told whether the previous plant packet arrived (gamma_{t-1}, :276), the
    estimator is the RobustEstimator (it also stores x_nom_0, :279) and the actuator adopts x_nom_0 (:133-147).

    p_loss (B,), ref (T,) or (B,T) position reference -- or (B,T,nx) full-state references: the solve of step t gets ref[:, t, :] and
    the tracking error is sum_i (x_i - r_i)^2 (the device loop's tmpc_mc_set_reference_table) --, th_u/ga_u (B,T) uniforms, w (B,T,nx) disturbances.
    plant: None = the linear model x+ = A x + B u + w (:248); or a callable (x (B,nx), u (B,nu)) -> x+ (w is added to it),
    e.g. workloads.cartpole_step for the nonlinear cart-pole of results_nonlinear_system.py.
    capture: index of one trajectory whose x_t, nominal state of the tube check and u_t are recorded (the scripts' sample run,
    :298-301) -> 'x_traj' (T, nx), 'x_nom_traj' (T, nx), 'u_traj' (T, nu).
    observer: optional callable (t, {'s', 'Theta', 'u'}) called after the actuator of step t (copies of its s_t, Theta_t and u_t).
    channel: None = independent losses with probability p_loss; or the Gilbert-Elliott channel (channel_parameters, e.g.
    burst_channel(..)) driven by the same uniforms -- p_loss is then not read and may be None.
    series: also keep the per-step record of the device loops (include/tmpc.h: tmpc_mc_set_series) -> 'series', a dict of (T, B)
    arrays: e, the error term of every step -- summed over t in order it is 'err2' --, word, and the word's fields (unpack_series_word);
    the iterations are those packets_fn returns as an optional fourth entry (0 without one).
    Returns a dict of per-trajectory statistics, the link statistics lost_up, lost_down, max_gap, overrun among them."""
    from .Estimator import BatchedEstimator
    from .SmartActuator import BatchedConsistentActuator
    A = np.asarray(A, dtype=np.float64)
    Bm = np.asarray(B, dtype=np.float64)
    nb, T = th_u.shape
    nx = A.shape[0]
    p_loss = None if channel is not None else np.asarray(p_loss, dtype=np.float64).reshape(nb)
    theta_all, gamma_all = _loss_flags(channel, p_loss, th_u, ga_u)
    link = _LinkStats(nb, N)
    rec = _SeriesRecord(T, nb, N) if series else None
    every = np.ones(nb, dtype=bool)
    ref = np.asarray(ref, dtype=np.float64)          # (T,) shared by the batch, (B, T) per trajectory, or (B, T, nx) full states
    full_ref = ref.ndim == 3                         # the solve gets ref[:, t, :], the error is sum_i (x_i - r_i)^2

    def ref_at(t):
        return ref[t] if ref.ndim == 1 else ref[:, t]
    x = np.zeros((nb, nx)) if x0 is None else np.array(x0, dtype=np.float64).reshape(nb, nx)
    cap = None if capture is None else dict(x_traj=np.zeros((T, nx)), x_nom_traj=np.zeros((T, nx)), u_traj=np.zeros((T, Bm.shape[1])))
    est = BatchedEstimator(A, Bm, K, x, N, K_plant=K_plant if extended else None, robust=extended)
    act = BatchedConsistentActuator(A, Bm, K, K_plant, x, is_extended_MPC_used=extended)
    err2 = np.zeros(nb)
    err2_phys, n_phys = np.zeros(nb), 0
    tube_viol = np.zeros(nb, dtype=np.int32)
    not_optimal = np.zeros(nb, dtype=np.int32)
    consistent_err = 0.0
    U_prev = x0_prev = None
    gamma = np.ones(nb, dtype=np.int64)
    for t in range(T):
        theta = theta_all[:, t]                                                                    # :211-226, strict <
        if full_ref:
            r_t = np.ascontiguousarray(ref[:, t, :])
        else:
            r_t = np.zeros((nb, nx))
            r_t[:, 0] = ref_at(t)
        q_t = est.get_qt()
        if extended:
            U_t, x_nom_0, status, iters = _packets(packets_fn(est.get_estimate(), r_t, gamma.astype(np.uint8)))     # RLX:276, gamma of step t-1
        else:
            U_t, x_nom_0, status, iters = _packets(packets_fn(est.get_estimate(), r_t))            # :240
        bad = status >= 2
        not_optimal += (status != 0)
        if bad.any():
            # the reference's tube branch has no handling for a failed solve (it would raise); here the
            # packet of such a trajectory is treated as lost and its previous sequence stays in use
            U_t = np.where(bad[:, None, None], U_prev if U_prev is not None else 0.0, U_t)
            x_nom_0 = np.where(bad[:, None], x0_prev if x0_prev is not None else 0.0, x_nom_0)
            theta = np.where(bad, 0, theta)
        U_prev, x0_prev = U_t, x_nom_0
        est.store(U_t)                                                                             # :242
        if extended:
            est.store_x_nom_0(x_nom_0)                                                             # RLX:279
        x_nom_now = act.x_nom.copy()       # the nominal state the scripts test against: column t of x_nom_traj, i.e. BEFORE process_packet
        u, pkt = act.process(U_t, q_t, x, theta, x_nom_0 if extended else None)                    # :244
        link.step(t, every, theta_all[:, t], gamma_all[:, t], act.s)      # (what the channel dropped: theta before a failed solve's 0)
        if observer is not None:
            observer(t, dict(s=np.array(act.s).copy(), Theta=np.array(act.Theta).copy(), u=np.array(u).copy()))
        if full_ref:
            a_t = (x[:, 0] - r_t[:, 0]) ** 2 + np.sum((x[:, 1:] - r_t[:, 1:]) ** 2, axis=1)          # (the order of the sum below)
        else:
            a_t = (x[:, 0] - ref_at(t)) ** 2 + np.sum(x[:, 1:] ** 2, axis=1)                          # :291 (x_t, t = 0..T-1)
        err2 += a_t
        # :258 / results_linear_system_with_extendedMPC.py:310-318,331-333 -- x_traj[:, t] - x_nom_traj[:, t]: the nominal state
        # appended after the PREVIOUS step's process_packet, so for the extended controller the state before this step's
        # adoption of x_nom_0 (SmartActuator.py:219-222); for the plain tube MPC the two coincide
        outside = ~np.asarray(Z.contains((x - x_nom_now).T)).reshape(nb)
        tube_viol += outside
        if rec is not None:
            rec.step(t, every, a_t, theta_all[:, t], gamma_all[:, t], act.Theta, outside, status, iters, act.s)
        if cap is not None:
            cap["x_traj"][t], cap["x_nom_traj"][t], cap["u_traj"][t] = x[capture], x_nom_now[capture], u[capture]
        if plant is not None and hasattr(plant, "trace"):
            xs = plant.trace(x, u)                                    # results_nonlinear_system.py:332-361: error over x_traj[:, 0:-1] at 500 Hz
            if full_ref:
                err2_phys += np.sum((xs[:-1, :, 0] - r_t[None, :, 0]) ** 2 + np.sum((xs[:-1, :, 1:] - r_t[None, :, 1:]) ** 2, axis=2), axis=0)
            else:
                err2_phys += np.sum((xs[:-1, :, 0] - ref_at(t)) ** 2 + np.sum(xs[:-1, :, 1:] ** 2, axis=2), axis=0)
            n_phys += xs.shape[0] - 1
            x = xs[-1] + w[:, t]
        else:
            x = (x @ A.T + u @ Bm.T if plant is None else plant(x, u)) + w[:, t]                  # :248
        gamma = gamma_all[:, t]                                                                    # :218-226
        est.update(pkt, gamma)                                                                     # :254
        # Proposition 1 of the paper: whenever the actuator is consistent and the plant packet arrives,
        # the estimate equals the nominal plant state
        ok = (act.Theta == 1) & (gamma == 1)
        if ok.any():
            consistent_err = max(consistent_err, float(np.max(np.abs(est.x_hat[ok] - act.x_nom[ok]))))
    out = dict(tracking_error=np.sqrt(err2) / T, err2=err2, tube_violations=tube_viol, not_optimal=not_optimal,
               consistent_estimate_error=consistent_err, x_final=x, **link.result())
    if rec is not None:
        out["series"] = rec.result()
    if n_phys:
        out["tracking_error_physics"] = np.sqrt(err2_phys) / n_phys
    if cap is not None:
        out.update(cap)
    return out


def run_remote_tracking_mpc(packets_fn, A, B, K, N, p_loss, ref, th_u, ga_u, w, x0=None, channel=None, plant=None, series: bool = False):
    """Closed loop of the non-robust comparator (R-MPC) over the lossy network: TrackingMPC + Estimator + plain
    SmartActuator (results_linear_system.py:198-205, 262-287).  A trajectory whose solve is infeasible stops there
    (track_feasible = False, :268-270) and reports a NaN tracking error (:297), and its link statistics stop at that step.  Same
    conventions as run_remote_tube_mpc otherwise (`channel`, `plant` and `series` included: a stopped trajectory's record is not alive
    from the step of its infeasible solve on; 'err2' keeps the sum up to there, the tracking error is NaN)."""
    from .Estimator import BatchedEstimator
    from .SmartActuator import BatchedConsistentActuator
    A = np.asarray(A, dtype=np.float64)
    Bm = np.asarray(B, dtype=np.float64)
    nb, T = th_u.shape
    nx = A.shape[0]
    p_loss = None if channel is not None else np.asarray(p_loss, dtype=np.float64).reshape(nb)
    theta_all, gamma_all = _loss_flags(channel, p_loss, th_u, ga_u)
    link = _LinkStats(nb, N)
    rec = _SeriesRecord(T, nb, N) if series else None
    ref = np.asarray(ref, dtype=np.float64)          # (T,) shared by the batch, (B, T) per trajectory, or (B, T, nx) full states
    full_ref = ref.ndim == 3                         # the solve gets ref[:, t, :], the error is sum_i (x_i - r_i)^2

    def ref_at(t):
        return ref[t] if ref.ndim == 1 else ref[:, t]
    x = np.zeros((nb, nx)) if x0 is None else np.array(x0, dtype=np.float64).reshape(nb, nx)
    est = BatchedEstimator(A, Bm, K, x, N)
    act = BatchedConsistentActuator(A, Bm, K, np.zeros_like(np.atleast_2d(K)), x)     # no nominal model: x_nom := x each step
    err2 = np.zeros(nb)
    dead = np.zeros(nb, dtype=bool)
    not_optimal = np.zeros(nb, dtype=np.int32)
    U_prev = None
    for t in range(T):
        theta = theta_all[:, t]
        if full_ref:
            r_t = np.ascontiguousarray(ref[:, t, :])
        else:
            r_t = np.zeros((nb, nx))
            r_t[:, 0] = ref_at(t)
        q_t = est.get_qt()
        U_t, _, status, iters = _packets(packets_fn(est.get_estimate(), r_t))
        newly = ~dead & (status >= 2)
        not_optimal += (~dead & (status != 0))
        dead |= newly
        U_t = np.where(np.isfinite(U_t), U_t, 0.0 if U_prev is None else U_prev)       # keeps the frozen trajectories' state machines NaN-free
        U_prev = U_t
        est.store(U_t)
        act.x_nom = x.copy()
        u, pkt = act.process(U_t, q_t, x, theta)
        pkt = {"x_t": x.copy(), "s_t": pkt["s_t"]}
        link.step(t, ~dead, theta_all[:, t], gamma_all[:, t], act.s)
        if full_ref:
            a_t = np.where(dead, 0.0, (x[:, 0] - r_t[:, 0]) ** 2 + np.sum((x[:, 1:] - r_t[:, 1:]) ** 2, axis=1))
        else:
            a_t = np.where(dead, 0.0, (x[:, 0] - ref_at(t)) ** 2 + np.sum(x[:, 1:] ** 2, axis=1))
        err2 += a_t
        if rec is not None:      # (no tube: the comparator has no nominal model)
            rec.step(t, ~dead, a_t, theta_all[:, t], gamma_all[:, t], act.Theta, False, status, iters, act.s)
        x = np.where(dead[:, None], x, (x @ A.T + u @ Bm.T if plant is None else plant(x, u)) + w[:, t])
        gamma = gamma_all[:, t]
        est.update(pkt, gamma)
    te = np.sqrt(err2) / T
    te[dead] = np.nan
    out = dict(tracking_error=te, err2=err2, not_optimal=not_optimal, infeasible=dead, x_final=x, **link.result())
    if rec is not None:
        out["series"] = rec.result()
    return out


CARTPOLE_KEYS = ("M", "m", "b", "I", "g", "l")      # the order of a cart-pole row {M, m, b, I, g, l, Th} (include/tmpc.h)
PLANT_STREAM = 0x706c616e74                          # second counter word of the Philox block sample_cartpole draws from


class PlantFamily:
    """A plant per trajectory for the host loops, the device loops (include/tmpc.h: tmpc_mc_run_plants for the tracking controllers,
    tmpc_mc_set_plant_models for the regulators) and the W estimate (tmpc_estimate_w_models) -- what plant_family returns.
    kind "linear": A (B, nx, nx), B (B, nx, nu), the plant of trajectory b is x+ = A_b x + B_b u; kind "cartpole": par (B, 7) rows
    {M, m, b, I, g, l, Th}, the RK4 cart-pole of workloads.cartpole_trace with `substeps` steps per period.  The controller's model
    stays the nominal one.  models: the C layout; family(x, u) -> x+ for x (B, nx), u (B, nu) (the host loops add w); family[slice]:
    the plants of a shard; len(family): B."""

    def __init__(self, kind, par=None, A=None, B=None, substeps: int = 10):
        self.kind, self.substeps = kind, int(substeps)
        self.par = self.A = self.B = None
        if kind == "cartpole":
            self.par = np.ascontiguousarray(par, dtype=np.float64).reshape(-1, 7)
            self.trace = self._trace          # (the host loops take the physics-rate tracking error from a plant that has one)
        elif kind == "linear":
            self.A = np.ascontiguousarray(A, dtype=np.float64)
            self.B = np.ascontiguousarray(B, dtype=np.float64)
            if self.A.ndim != 3 or self.B.ndim != 3 or self.A.shape[1] != self.A.shape[2] or self.B.shape[:2] != self.A.shape[:2]:
                raise ValueError("plant_family: A is (B, nx, nx) and B is (B, nx, nu)")
        else:
            raise ValueError(f"plant_family: unknown kind {kind!r}")

    def __len__(self):
        return (self.par if self.kind == "cartpole" else self.A).shape[0]

    @property
    def models(self):
        """(B, 7), or (B, nx, nx + nu) rows [A_b[i, :] | B_b[i, :]]: what tmpc_mc_set_plant_models takes."""
        return self.par if self.kind == "cartpole" else np.ascontiguousarray(np.concatenate([self.A, self.B], axis=2))

    def __getitem__(self, idx):
        if not isinstance(idx, slice):
            idx = np.atleast_1d(idx)
        if self.kind == "cartpole":
            return PlantFamily("cartpole", par=self.par[idx], substeps=self.substeps)
        return PlantFamily("linear", A=self.A[idx], B=self.B[idx])

    def _trace(self, x, u):
        from . import workloads
        par = {k: self.par[:, i] for i, k in enumerate(CARTPOLE_KEYS)}
        return workloads.cartpole_trace(x, np.asarray(u, dtype=np.float64).reshape(len(self), -1)[:, 0], self.par[:, 6], self.substeps, par)

    def __call__(self, x, u):
        if self.kind == "cartpole":
            return self._trace(x, u)[-1]
        return np.einsum("bij,bj->bi", self.A, x) + np.einsum("bij,bj->bi", self.B, u)


def plant_family(kind, *, par=None, A=None, B=None, Th=0.02, substeps: int = 10):
    """A plant per trajectory for the closed loops and the W estimate (PlantFamily).  kind "cartpole": par is a dict over
    workloads.CARTPOLE_PARAMS' keys, each a scalar or (B,) -- missing keys take the nominal value, the period is Th --, or a (B, 7)
    array of rows {M, m, b, I, g, l, Th}.  kind "linear": A (B, nx, nx), B (B, nx, nu)."""
    if kind == "cartpole":
        from .workloads import CARTPOLE_PARAMS
        if par is None:
            par = {}
        if isinstance(par, dict):
            unknown = set(par) - set(CARTPOLE_KEYS)
            if unknown:
                raise ValueError(f"plant_family: unknown cart-pole parameters {sorted(unknown)}")
            cols = np.broadcast_arrays(*[np.atleast_1d(np.asarray(par.get(k, CARTPOLE_PARAMS[k]), dtype=np.float64)) for k in CARTPOLE_KEYS],
                                       np.atleast_1d(np.asarray(Th, dtype=np.float64)))
            par = np.stack(cols, axis=1)
        return PlantFamily("cartpole", par=par, substeps=substeps)
    return PlantFamily(kind, A=A, B=B)


def sample_cartpole(n: int, spread: float, seed: int, first: int = 0, Th: float = 0.02, substeps: int = 10):
    """n cart-poles around workloads.CARTPOLE_PARAMS: M, m and l are the nominal value times 1 + spread U(-1, 1), the cart's friction b
    is spread U(0, 1); I and g stay.  Trajectory first + i takes the four words of Philox4x64-10 with key (seed, first + i) and counter
    (0, PLANT_STREAM) as (M, m, l, b), u = (word >> 11) 2^-53: a trajectory's plant does not depend on how a sweep is sharded."""
    from .workloads import CARTPOLE_PARAMS as P
    g = np.uint64(first) + np.arange(n, dtype=np.uint64)
    words = philox4x64(np.uint64(0), np.uint64(PLANT_STREAM), np.uint64(seed), g)                # (4, n)
    u = (words >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    rel = 1.0 + float(spread) * (2.0 * u[:3] - 1.0)
    return plant_family("cartpole", par=dict(M=P["M"] * rel[0], m=P["m"] * rel[1], l=P["l"] * rel[2], b=float(spread) * u[3]), Th=Th,
                        substeps=substeps)


plant_family.sample_cartpole = sample_cartpole


def cartpole_rows(par, n: int, Th: float = 0.02):
    """par= of the W estimates -> (n, 7) rows {M, m, b, I, g, l, Th}: a cart-pole PlantFamily, a dict as plant_family takes it, or rows."""
    fam = par if isinstance(par, PlantFamily) else plant_family("cartpole", par=par, Th=Th)
    if fam.kind != "cartpole":
        raise ValueError("the W estimate runs cart-pole plants")
    rows = fam.par
    if rows.shape[0] == 1 and n != 1:
        rows = np.repeat(rows, n, axis=0)
    if rows.shape[0] != n:
        raise ValueError(f"par holds {rows.shape[0]} plants, the estimate {n} trajectories")
    return np.ascontiguousarray(rows)


def plant_callable(plant):
    """'cartpole' -> the numpy counterpart of the device plant (workloads.cartpole_step); callables -- a PlantFamily among them -- pass
    through."""
    if callable(plant):
        return plant
    if plant == "cartpole":
        from . import workloads

        def step(x, u):
            return workloads.cartpole_step(x, u[:, 0])
        step.trace = lambda x, u: workloads.cartpole_trace(x, u[:, 0])       # physics-rate states (tracking error at 500 Hz)
        return step
    raise ValueError(f"unknown plant {plant!r}")


def mc_sweep(mpc, model: dict, p_loss, n_mc: int, T: int, ref, seed: int = 20240301, rank: int = 0, world: int = 1,
             extended: bool = False, device=None, on_device: bool = False, plant=None, warm_start: bool = False,
             timing: bool = False, device_rng: bool = False, force_collective: bool = False, ref_id=None, mean_burst=None,
             link_stats: bool = False, series=None, law=None):
    """The Monte-Carlo sweep of results_linear_system.py:147-301 (BASELINE config 4): len(p_loss) x n_mc
    trajectories of T steps, sharded over `world` ranks (one process per GPU, contiguous p_loss-balanced
    shards), every time step of a shard solved by one kernel launch, statistics all-gathered at the end.
    Returns (table (n_total, 3) = [tracking error, tube violations, non-optimal solves], p_index (n_total,)),
    identical on every rank.  timing (device loop only): two more columns, the mean and the maximum device time of a
    trajectory's solves in seconds -- the computational times results_linear_system.py:305-315 reports.
    device_rng: Philox streams keyed by (seed, global trajectory index), drawn on the device in the device loop
    (tmpc_mc_set_device_rng) and by draw_realisations_philox, the same numbers, in the host loops.
    ref: a scalar or (T,) position reference; or (T, nx) one full-state schedule for every trajectory; or (K, T, nx) schedules
    with ref_id (n_total,) naming each trajectory's -- sliced with the shard, so the sweep stays shard-invariant.
    plant: None / "cartpole"; or a PlantFamily of n_total plants (plant_family, sample_cartpole), sliced with the shard -- on the device
    the loop of tmpc_mc_run_plants.
    mean_burst: None -- independent losses; else every loss rate p as the stationary rate of burst_channel(p, mean_burst), on the
    same uniforms (a rate above 1 - 1 / mean_burst keeps independent losses, whose bursts last 1 / (1 - p) on average; every rate must be below 1).  link_stats: four more columns at the end of the table: lost_up, lost_down, max_gap, overrun.
    series: None -- nothing more; True or a sequence of quantiles (True: 0.5, 0.95) -- the loops keep their per-step record and a third
    value is returned, the record's ensemble statistics per time step and loss rate (series_stats, (T, len(p_loss)) tables; on the device
    tmpc_mc_series_stats).  One rank only: quantiles of shards do not merge (ValueError with world > 1).
    law: None -- every step is solved; else the loops go through the controller's explicit-law table (run_closed_loop's `law` on the device,
    LawPackets.from_law in the host loop of the tube controller) and solve the misses only."""
    if series is not None and series is not False and world > 1:
        raise ValueError("mc_sweep: series needs world == 1 (order statistics of shards do not merge)")
    want_series = series is not None and series is not False
    series_q = (0.5, 0.95) if series is True else (tuple(series) if want_series else ())
    import torch
    p_loss = np.asarray(p_loss, dtype=np.float64)
    pi, _ = trajectory_table(p_loss, n_mc)
    n_total = len(pi)
    lo, hi = shard_bounds(n_total, rank, world)
    if device_rng and on_device:
        th = ga = w = None
    elif device_rng:
        th, ga, w = draw_realisations_philox(hi - lo, T, model["w_bound"], seed=seed, first=lo)
    else:
        th, ga, w = draw_realisations(hi - lo, T, model["w_bound"], seed=seed, first=lo)
    ref = np.asarray(ref, dtype=np.float64)
    ids = None
    if ref.ndim >= 2:
        ref = ref if ref.ndim == 3 else ref[None]
        ids = np.zeros(n_total, dtype=np.int32) if ref_id is None else np.asarray(ref_id, dtype=np.int32).reshape(n_total)
        ids = ids[lo:hi]
        if not on_device:
            ref = ref[ids, :T]                        # the host twins take one schedule per trajectory
    else:
        ref = np.broadcast_to(ref, (T,))
    channel = None
    if mean_burst is not None:
        if np.any(p_loss >= 1.0):
            raise ValueError("mc_sweep: mean_burst needs every loss rate below 1 (a channel that loses every packet has no bursts)")
        rate = p_loss[pi[lo:hi]]
        channel = burst_channel(rate, np.maximum(float(mean_burst), 1.0 / (1.0 - rate)))
    if isinstance(plant, PlantFamily):                # a plant per trajectory of the whole sweep: the shard's
        if len(plant) != n_total:
            raise ValueError(f"mc_sweep: the plant family holds {len(plant)} plants, the sweep {n_total} trajectories")
        plant = plant[lo:hi]
    if on_device:        # state machines on the GPU as well (tmpc_mc_run); otherwise the host loop around determine_packets
        out = mpc.run_closed_loop(p_loss[pi[lo:hi]], ref, th, ga, w, extended=extended, plant=plant, warm_start=warm_start,
                                  timing=timing, device_rng=(seed, lo, model["w_bound"]) if device_rng else None, ref_id=ids,
                                  T=T if ids is not None else None, channel=channel, **(dict(series=True) if want_series else {}),
                                  **({} if law is None else dict(law=law)))
    elif getattr(mpc, "_smart_actuator", False):       # TrackingMPC: the comparator's loop (results_linear_system.py:262-287)
        out = run_remote_tracking_mpc(mpc.determine_packets, model["A"], model["B"], mpc.get_steady_state_controller_gain(), mpc._N,
                                      p_loss[pi[lo:hi]], ref, th, ga, w, channel=channel, plant=None if plant is None else plant_callable(plant),
                                      series=want_series)
        out["tube_violations"] = np.zeros(hi - lo, dtype=np.int32)
    else:
        fn = mpc.determine_packets
        if law is not None and law is not False:
            from . import _native
            _, max_tries, miss_capacity = _native._law_setting(law)
            fn = LawPackets.from_law(mpc, max_tries=max_tries, miss_capacity=miss_capacity)
        out = run_remote_tube_mpc(fn, model["A"], model["B"], mpc.get_steady_state_controller_gain(),
                                  mpc.get_ancillary_controller_gain(), mpc._N, mpc._Z, p_loss[pi[lo:hi]], ref, th, ga, w,
                                  extended=extended, plant=None if plant is None else plant_callable(plant), channel=channel, series=want_series)
    cols = [out["tracking_error"], out["tube_violations"], out["not_optimal"]]
    if timing and on_device:
        cols += [out["solve_time_mean"], out["solve_time_max"]]
    if link_stats:
        cols += [out[k] for k in ("lost_up", "lost_down", "max_gap", "overrun")]
    local = torch.tensor(np.column_stack(cols), dtype=torch.float64)
    if device is not None:
        local = local.to(device)
    table = gather_statistics(local, n_total, rank, world, force_collective=force_collective)
    if want_series:
        if on_device:
            from . import _native
            stats = _native.mc_series_stats(mpc._handle, group=pi, q=series_q, G=len(p_loss))
        else:
            stats = series_stats(out["series"]["e"], out["series"]["word"], pi, series_q, G=len(p_loss))
        return table.cpu().numpy(), pi, stats
    return table.cpu().numpy(), pi


# --------------------------------------------------------------------------- the disturbance set W of the linear model
W_REFERENCE_X0_BOX = (np.array([-1.0, -0.5, -0.3, -0.5]), np.array([1.0, 0.5, 0.3, 0.5]))      # estimate_W_for_Cartpole.py:66-73


def draw_initial_states_philox(n: int, lo, hi, seed: int, first: int = 0):
    """The initial states tmpc_estimate_w draws on the device (include/tmpc.h), reproduced on the host: trajectory g = first + i takes
    the four words of Philox4x64-10 with key (seed, g), counter (0, 0, 0, 0); u = (word >> 11) 2^-53; x0 = lo + (hi - lo) u.
    A trajectory's start does not depend on how a sweep is split."""
    lo = np.asarray(lo, dtype=np.float64).reshape(-1)
    hi = np.asarray(hi, dtype=np.float64).reshape(-1)
    if lo.size != 4 or hi.size != 4:
        raise ValueError("draw_initial_states_philox: one Philox block per trajectory, four states")
    g = np.uint64(first) + np.arange(n, dtype=np.uint64)
    words = philox4x64(np.uint64(0), np.uint64(0), np.uint64(seed), g)                        # (4, n)
    u = (words >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return lo + (hi - lo) * u.T


def reference_initial_states(n: int = 100, seed: int = 456, box=W_REFERENCE_X0_BOX):
    """The initial states of the reference's run: four scalar uniform draws per trajectory from default_rng(456)
    (estimate_W_for_Cartpole.py:12, 82-85); one (n, 4) draw consumes the generator in the same order."""
    return np.random.default_rng(seed).uniform(box[0], box[1], (n, 4))


def quantile_ranks(n: int, discard: float):
    """The four ranks numpy's default (linear) quantile rule reads for q = discard / 2 and 1 - discard / 2 of n values, and the weight
    of the upper neighbour of each pair: (ranks [lo_floor, lo_ceil, hi_floor, hi_ceil], gamma [lo, hi])."""
    ranks, gam = [], []
    for q in (discard / 2.0, 1.0 - discard / 2.0):
        virt = (n - 1) * q                                 # numpy.lib: the virtual index of method 'linear'
        prev = int(np.floor(virt))
        gam.append(virt - prev)
        ranks += [min(max(prev, 0), n - 1), min(max(prev + 1, 0), n - 1)]
    return np.array(ranks, dtype=np.int64), np.array(gam)


def _lerp(a, b, t):
    """numpy.lib's _lerp for scalars"""
    d = b - a
    return a + d * t if t < 0.5 else b - d * (1.0 - t)


def _box_result(samples, lo, hi, wmin, wmax, n_nonfinite, not_settled, x_final_norm_max, **extra):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    return dict(samples=samples, lo=lo, hi=hi, w_bound=np.maximum(np.abs(lo), np.abs(hi)), min=np.asarray(wmin), max=np.asarray(wmax),
                n_samples=None if samples is None else samples.shape[1] * samples.shape[2], n_nonfinite=np.asarray(n_nonfinite),
                not_settled=int(not_settled), x_final_norm_max=float(x_final_norm_max), **extra)


def estimate_disturbance_box_host(A, B, K, x0, T: int, discard: float = 0.025, plant="cartpole", Th: float = 0.02, substeps: int = 10,
                                  settle_tol: float = 1e-3, par=None):
    """The reference's estimate of the disturbance set (Results/estimate_W_for_Cartpole.py) on the numpy twin of the device plant
    (workloads.cartpole_step: the closed-form cart-pole, RK4 at the physics rate -- NOT the reference's PyBullet model, so the numbers
    are those of this plant and no replication of the reference's): closed loops u = -K x from the initial states x0 (n x 4) over T
    sampling periods, the samples w_k = x_k - (A - B K) x_{k-1} for k = 1 .. T - 1 (:94-107), and per component the
    discard / 2 and 1 - discard / 2 quantiles of all samples (:117-120, numpy's default linear rule).

    The reference starts its sample list with one all-zero column (:77) that takes part in its quantiles; this function does not add
    it (at the reference's size, 39 900 samples, that changes the fourth significant digit of the box).

    par: None -- every trajectory on workloads.CARTPOLE_PARAMS; or a cart-pole per trajectory (a PlantFamily, a dict as plant_family
    takes it, or (n, 7) rows): A, B and K stay the nominal ones, so the samples contain the parametric mismatch of the family.

    Returns dict(samples (4, T - 1, n), lo, hi, w_bound = max(|lo|, |hi|), min, max, n_samples, n_nonfinite, not_settled: the number
    of trajectories with |x_T|_2 > settle_tol (:110), x_final_norm_max).  Non-finite samples are counted per component; a component
    that has any gets lo = hi = NaN (the loop diverged: there is no box)."""
    if plant != "cartpole":
        raise ValueError("estimate_disturbance_box_host: only the cart-pole plant")
    from .workloads import cartpole_step
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64).reshape(1, 4)
    Acl = A - B @ K
    x = np.array(x0, dtype=np.float64).reshape(-1, 4)
    n = x.shape[0]
    step = (lambda xk, uk: cartpole_step(xk, uk, Th, substeps)) if par is None else plant_family("cartpole", par=cartpole_rows(par, n, Th), substeps=substeps)
    samples = np.empty((4, T - 1, n))
    for k in range(T):
        xp = x
        u = np.zeros(n)
        for i in range(4):                                # the sums run in index order, as on the device
            u = u - K[0, i] * xp[:, i]
        x = step(xp, u)
        if k + 1 < T:
            for c in range(4):
                s = Acl[c, 0] * xp[:, 0]
                for i in range(1, 4):
                    s = s + Acl[c, i] * xp[:, i]
                samples[c, k] = x[:, c] - s
    flat = samples.reshape(4, -1)
    fin = np.isfinite(flat)
    nf = (~fin).sum(axis=1)
    q = [discard / 2.0, 1.0 - discard / 2.0]
    lo, hi, wmin, wmax = (np.full(4, np.nan) for _ in range(4))
    for c in range(4):
        if nf[c] == 0:
            lo[c], hi[c] = np.quantile(flat[c], q)
        if fin[c].any():
            wmin[c], wmax[c] = flat[c][fin[c]].min(), flat[c][fin[c]].max()
    nrm = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2] + x[:, 3] * x[:, 3])
    return _box_result(samples, lo, hi, wmin, wmax, nf, np.sum(~(nrm <= settle_tol)), np.nan if np.isnan(nrm).any() else np.max(nrm),
                       x0_used=np.array(x0, dtype=np.float64).reshape(-1, 4))


def estimate_disturbance_box(A, B, K, x0=None, T: int = 400, discard: float = 0.025, plant="cartpole", x0_box=None, n_traj=None,
                             seed: int = 456, first: int = 0, Th: float = 0.02, substeps: int = 10, settle_tol: float = 1e-3,
                             device: int = 0, want_samples: bool = False, par=None):
    """estimate_disturbance_box_host on the device (include/tmpc.h: tmpc_estimate_w; csrc/tmpc_west.hip): one lane per trajectory,
    the samples stay in device memory (8 * 4 * (T - 1) * n_traj bytes), and the four order statistics behind the two quantiles of each
    component -- the neighbours floor and ceil of q (n - 1) -- are selected there exactly; the interpolation between them is numpy's.
    Initial states: x0 (n x 4), or x0_box = (lo, hi) with n_traj and seed: drawn on the device, trajectory first + i from the stream
    of draw_initial_states_philox.  Like the host twin -- and unlike the reference -- no all-zero sample is added in front.
    par: a cart-pole per trajectory, as estimate_disturbance_box_host takes it (tmpc_estimate_w_models).
    Same return values (samples: None unless want_samples), and rollout_ms / selection_ms, the device times of the two stages."""
    from . import _native
    if x0 is not None:
        n_traj = np.asarray(x0).reshape(-1, 4).shape[0]
    if n_traj is None:
        raise ValueError("estimate_disturbance_box: give x0, or x0_box and n_traj")
    n = int(n_traj) * (int(T) - 1)
    ranks, gam = quantile_ranks(max(n, 1), discard)
    out = _native.estimate_w(A, B, K, T, x0=x0, x0_box=x0_box, n_traj=n_traj, seed=seed, first=first, ranks=ranks, settle_tol=settle_tol,
                             plant=plant, Th=Th, substeps=substeps, device=device, want_samples=want_samples,
                             par=None if par is None else cartpole_rows(par, int(n_traj), Th))
    st = out["order_stats"]
    lo, hi = np.full(4, np.nan), np.full(4, np.nan)
    for c in range(4):
        if out["n_nonfinite"][c] == 0:
            lo[c], hi[c] = _lerp(st[c, 0], st[c, 1], gam[0]), _lerp(st[c, 2], st[c, 3], gam[1])
    res = _box_result(out.get("samples"), lo, hi, out["w_min"], out["w_max"], out["n_nonfinite"], out["not_settled"],
                      out["x_final_norm_max"], x0_used=out["x0_used"], rollout_ms=out["rollout_ms"], selection_ms=out["selection_ms"],
                      order_stats=st, ranks=ranks)
    res["n_samples"] = out["n_samples"]
    return res
