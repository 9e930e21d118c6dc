"""The explicit control law on the host: the numpy twin (LinearMPCOverNetworks/explicit_law.py) against closed forms and planted QPs, the
table of a host-only handle (tmpc_law_add / tmpc_law_get_region) against the twin on the golden cart-pole states, the refusals of the C
entry points, the kernel's source on the host execution model, and its resource notes.  The kernel itself runs in
tests/test_explicit_law_gpu.py.

Bounds.  * Clipped family: 1e-12 on z (the issue's; H is diagonal and M with it, so only a division and a product separate the law from
the closed form).  * Planted cases: Ky against the long-double judge to the bound of tests/test_sensitivity.py for the twin of the
sensitivity kernel, 8 n eps cond(H) cond(M) max(1, |J|_max) with n = nv + |A|; z(p) = Kz p + kz sums np + 1 such terms, so
Z is reproduced to that bound with |J|_max replaced by (np + 1) max(1, |Kz|_max, |kz|_max) max(1, |p|_max).  * Golden states: TOL_U0 = 1e-8
of tests/certificates.py on every output, against the oracle's solutions."""
import importlib.util
import os
import sys

import numpy as np
import pytest

import common
import law_cases as lc
import sensitivity_reference as sr
from LinearMPCOverNetworks import explicit_law as E
from LinearMPCOverNetworks import sensitivity as S
from oracle.oracle import Oracle

ROOT = os.path.dirname(common.PKG)
STATES = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))
EPS = np.finfo(np.float64).eps
KEYS = ("u_nom", "x_nom0", "xu_ss", "status")
TOL_U0 = 1e-8                             # tests/certificates.py
E_INVALID, E_UNSUPPORTED, E_DEVICE = -1, -2, -3


# ------------------------------------------------------------------ 1: the clipped family
@pytest.mark.parametrize("nv", [1, 17, 128])
def test_clipped_family_law_and_search(nv):
    c = lc.clipped_case(100 + nv, nv, 2 * nv + 5, 8, 12)
    m, P = c["model"], c["P"]
    own = []
    for s in c["sets"]:
        if s not in own:
            own.append(s)
    others = lc.other_patterns(c, 20, own)
    assert len(others) == 20 or nv == 1
    sets = own + others
    table = [E.region_law(m, s) for s in sets]
    assert all(t is not None for t in table)
    for b in range(c["B"]):
        t = table[sets.index(c["sets"][b])]
        assert np.max(np.abs(t["Kz"] @ P[b] + t["kz"] - c["Z"][b])) <= 1e-12, (nv, b)
        inside = [r for r, tt in enumerate(table) if np.all(tt["S"] @ P[b] + tt["s"] >= 0.0)]
        assert inside == [sets.index(c["sets"][b])], (nv, b, inside)
    want = np.array([sets.index(s) for s in c["sets"]])
    region, tries, y = E.locate(table, P)
    assert np.array_equal(region, want) and np.array_equal(tries, want + 1)
    assert np.max(np.abs(y - c["Z"])) <= 1e-12
    # the region absent: a miss after every candidate
    absent = [t for r, t in enumerate(table) if r != want[0]]
    region, tries, y = E.locate(absent, P[:1])
    assert region[0] == -1 and tries[0] == len(absent) and np.all(np.isnan(y[0]))
    # the hint first, then the order without it; max_tries cuts the walk
    R = len(table)
    rev = np.arange(R)[::-1]
    region, tries, _ = E.locate(table, P, hint=want)
    assert np.array_equal(region, want) and np.all(tries == 1)
    region, tries, _ = E.locate(table, P, order=rev)
    assert np.array_equal(region, want) and np.array_equal(tries, R - want)
    wrong = (want + 1) % R
    region, tries, _ = E.locate(table, P, hint=wrong)
    exp = np.where(wrong < want, want + 1, want + 2)       # the hint, then 0 .. want without the hint
    assert np.array_equal(region, want) and np.array_equal(tries, exp)
    region, tries, _ = E.locate(table, P, hint=np.full(len(P), R))      # an id out of range is no hint
    assert np.array_equal(region, want) and np.array_equal(tries, want + 1)
    for mt in (1, 2):
        region, tries, _ = E.locate(table, P, max_tries=mt)
        assert np.array_equal(region, np.where(want < mt, want, -1)) and np.array_equal(tries, np.minimum(want + 1, mt))
    region, tries, _ = E.locate(table, P, order=rev[:3], hint=want, max_tries=1)
    assert np.array_equal(region, want) and np.all(tries == 1)
    bad = P.copy()
    bad[0, 0] = np.inf
    region, tries, y = E.locate(table, bad)
    assert region[0] == -1 and tries[0] == 0 and np.all(np.isnan(y[0])) and region[1] == want[1]


# ------------------------------------------------------------------ 2: planted cases
def _planted_bound(c, scale):
    A = c["A"]
    M = c["G"][A] @ np.linalg.solve(c["H"], c["G"][A].T) if len(A) else np.eye(1)
    return 8 * (c["nv"] + len(A)) * EPS * np.linalg.cond(c["H"]) * np.linalg.cond(M) * scale


def test_planted_cases():
    for gdef in sr.planted_grid():
        c = sr.planted_case(**gdef)
        J = sr.planted_judge(c)
        t = E.region_law(c, c["A"])
        assert t is not None, gdef
        err = float(np.max(np.abs(t["Ky"].astype(np.longdouble) - J)))
        assert err <= _planted_bound(c, max(1.0, float(np.abs(J).max()))), (gdef, err)
        kmax = max(1.0, float(np.abs(t["Kz"]).max()), float(np.abs(t["kz"]).max(initial=0.0)))
        zerr = float(np.max(np.abs(c["P"] @ t["Kz"].T + t["kz"] - c["Z"])))
        assert zerr <= _planted_bound(c, (c["P"].shape[1] + 1) * kmax * max(1.0, float(np.abs(c["P"]).max()))), (gdef, zerr)
        region, tries, y = E.locate([t], c["P"])
        assert np.all(region == 0) and np.all(tries == 1), gdef
        assert np.max(np.abs(y - (c["Z"] @ c["Y"].T + c["P"] @ c["Yp"].T))) <= c["ny"] * max(1.0, float(np.abs(c["Y"]).max())) * \
            _planted_bound(c, (c["P"].shape[1] + 1) * kmax * max(1.0, float(np.abs(c["P"]).max()))), gdef


# ------------------------------------------------------------------ 3: the golden cart-pole states on host-only handles
@pytest.mark.parametrize("which", ["fixed", "free", "variant1"])
def test_golden_states_on_a_host_only_handle(hip_lib, which):
    X, R = STATES[:, :4], STATES[:, 4:]
    if which == "fixed":
        mpc, _ = common.make_mpc("cartpole", 10, True, create=True, device=-1)
        sol, var, k = dict(np.load(os.path.join(common.GOLDEN, "cartpole_N10_oracle.npz"))), None, 0
    elif which == "free":
        mpc, _ = common.make_mpc("cartpole", 10, False, create=True, device=-1)
        sol, var, k = Oracle(mpc._problem_dict()).solve(X, R), None, 0
    else:
        mpc, _ = common.make_mpc("cartpole", 10, True, extended=True, create=True, device=-1)
        var, k = np.ones(len(X), np.uint8), 1
        sol = Oracle(mpc._problem_dict()).solve(X, R, variant=var)
    try:
        h = mpc._handle
        tw = S.handle_sensitivity(mpc, X, R, {kk: sol[kk] for kk in KEYS}, variant=var)
        ok = (tw["flag"] & (S.SKIPPED | S.NOT_KKT)) == 0
        m = E.law_model(h, k)
        nc = m["G"].shape[0]
        nw = (nc + 31) // 32
        ids = hip_lib.law_add(h, tw["active"][ok][:, :nw], k)
        again = hip_lib.law_add(h, tw["active"][ok][:, :nw], k)
        assert np.array_equal(ids, again)                 # a set already stored keeps its id
        n = int(ids.max()) + 1
        assert n >= 16 and len(hip_lib.law_stats(h, k)) == n
        first = {}
        for i, a in zip(ids, tw["active"][ok]):
            first.setdefault(int(i), a)
        first.pop(-1, None)
        assert sorted(first) == list(range(n))            # ids in insertion order
        table = [E.region_law(m, S.decode_active(first[i][:nw], nc=nc)) for i in range(n)]
        # the C table is the twin's, to rounding: cond(M) of these working sets reaches 1e7
        for i in range(0, n, max(1, n // 25)):
            r = hip_lib.law_get_region(h, i, k)
            assert np.array_equal(r["words"], first[i][:nw])
            for key in ("Ky", "ky", "S", "s"):
                assert np.max(np.abs(r[key] - table[i][key])) <= 1e-7 * max(1.0, float(np.abs(r[key]).max())), (which, i, key)
        region, tries, y = E.locate(table, STATES)
        added = np.flatnonzero(ok)[ids >= 0]
        assert np.all(region[added] >= 0), (which, np.flatnonzero(region[added] < 0))
        assert not np.any(region[sol["status"] >= 2] >= 0)
        hit = region >= 0
        want = np.c_[sol["u_nom"].reshape(len(X), -1), sol["x_nom0"], sol["xu_ss"]]
        assert np.all(sol["status"][hit] == 0)
        err = float(np.max(np.abs(y[hit] - want[hit])))
        print(f"{which}: {n} regions from {int(ok.sum())} admissible signatures, {int(hit.sum())} of {len(X)} located, mean tries {tries[hit].mean():.1f}, "
              f"largest output difference to the oracle {err:.2e}")
        assert err <= TOL_U0, (which, err)
        # without the parameter-only rows an infeasible state may be located: they are part of every region
        npar = len(m["gp0"])
        assert table[0]["S"].shape[0] == nc + npar
        hip_lib.law_clear(h, k)
        assert len(hip_lib.law_stats(h, k)) == 0
        with pytest.raises(ValueError, match="no such region"):
            hip_lib.law_get_region(h, 0, k)
    finally:
        mpc._close()


# ------------------------------------------------------------------ 4: refusals, on host-only handles
@pytest.fixture(scope="module")
def handles(hip_lib):
    import regulator_problems
    plain, _ = common.make_mpc("cartpole", 10, True, create=True, device=-1)
    reg = regulator_problems.plain_double_integrator(device=-1)
    lit, _ = common.make_mpc("cartpole", 10, True, extended=True, device=-1)
    lit._eliminate_auxiliaries = False            # the literal terminal row: variant 1 keeps its auxiliaries
    lit.generate_optimization_problem(True)
    yield dict(plain=plain._handle, reg=reg._handle, literal=lit._handle)
    for m in (plain, reg, lit):
        m._close()


EVAL = ("tmpc_law_eval", "tmpc_law_eval_device", "tmpc_law_solve", "tmpc_law_solve_device")


def _call(hip_lib, h, name, B=2, null=None, variant=False):
    nx, nu, N = h.nx, h.nu, h.N
    Bc, B = B, max(B, 1)
    a = dict(x_k=np.zeros((B, nx)), ref=np.zeros((B, nx)), variant=np.zeros(B, np.uint8) if variant else None, hint=np.zeros(B, np.int32),
             u_nom=np.zeros((B, N, nu)), x_nom0=np.zeros((B, nx)), xu_ss=np.zeros((B, nx + nu)), x_nom=np.zeros((B, N + 1, nx)), status=np.zeros(B, np.int32),
             iters=np.zeros(B, np.int32), region=np.zeros(B, np.int32), tries=np.zeros(B, np.int32), ids=np.zeros(B, np.int32))
    if null:
        a[null] = None
    p = {k: (None if v is None else v.ctypes.data) for k, v in a.items()}
    if name == "tmpc_law_learn":
        rc = hip_lib.lib().tmpc_law_learn(h.ptr, Bc, p["x_k"], p["ref"], p["variant"], p["u_nom"], p["x_nom0"], p["xu_ss"], p["status"], 0.0, p["ids"], None)
    else:
        rc = getattr(hip_lib.lib(), name)(h.ptr, Bc, p["x_k"], p["ref"], p["variant"], p["hint"], 0, p["u_nom"], p["x_nom0"], p["xu_ss"], p["x_nom"], p["status"],
                                          p["iters"], p["region"], p["tries"])
    return rc, h.error()


@pytest.mark.parametrize("name", EVAL + ("tmpc_law_learn",))
def test_null_arguments_and_negative_batch_are_refused(hip_lib, handles, name):
    h = handles["plain"]
    required = ("x_k", "ref", "u_nom", "x_nom0", "xu_ss") + (("status", "region") if name != "tmpc_law_learn" else ()) + (("iters",) if "solve" in name else ())
    for null in required:
        rc, msg = _call(hip_lib, h, name, null=null)
        assert rc == E_INVALID and msg == f"{name}: NULL argument", (null, rc, msg)
    optional = () if name == "tmpc_law_learn" else ("hint", "x_nom", "tries") + (() if "solve" in name else ("iters",))
    for null in optional:                 # may be NULL: the call gets as far as the device check
        assert _call(hip_lib, h, name, null=null)[0] == E_DEVICE, null
    rc, msg = _call(hip_lib, h, name, B=-1)
    assert rc == E_INVALID and msg == f"{name}: B < 0"
    assert _call(hip_lib, h, name, B=0)[0] == 0
    tail = (0.0, None, None) if name == "tmpc_law_learn" else (0, *([None] * 8))
    assert getattr(hip_lib.lib(), name)(None, 1, *([None] * (7 if name == "tmpc_law_learn" else 4)), *tail) == E_INVALID


@pytest.mark.parametrize("name", EVAL + ("tmpc_law_learn",))
def test_a_host_only_handle_is_refused_by_the_evaluating_entries(hip_lib, handles, name):
    rc, msg = _call(hip_lib, handles["plain"], name)
    assert rc == E_DEVICE and msg == "host-only handle (device < 0): nothing can be solved without the GPU"


@pytest.mark.parametrize("name", EVAL + ("tmpc_law_learn", "tmpc_law_add", "tmpc_law_get_stats", "tmpc_law_reorder", "tmpc_law_clear", "tmpc_law_get_region"))
def test_a_regulator_handle_is_refused(hip_lib, handles, name):
    h = handles["reg"]
    L = hip_lib.lib()
    if name in EVAL or name == "tmpc_law_learn":
        rc = _call(hip_lib, h, name)[0]
    elif name == "tmpc_law_add":
        rc = L.tmpc_law_add(h.ptr, 0, 1, np.zeros(64, np.uint32).ctypes.data, None)
    elif name == "tmpc_law_get_stats":
        rc = L.tmpc_law_get_stats(h.ptr, 0, None, None)
    elif name == "tmpc_law_get_region":
        rc = L.tmpc_law_get_region(h.ptr, 0, 0, None, None, None, None, None)
    else:
        rc = getattr(L, name)(h.ptr, 0)
    assert rc == E_UNSUPPORTED and "regulator handle" in h.error(), (name, rc, h.error())


@pytest.mark.parametrize("name", EVAL + ("tmpc_law_learn", "tmpc_law_add"))
def test_a_variant_with_unpriced_auxiliaries_is_refused(hip_lib, handles, name):
    h = handles["literal"]
    if name == "tmpc_law_add":
        rc = hip_lib.lib().tmpc_law_add(h.ptr, 1, 1, np.zeros(64, np.uint32).ctypes.data, None)
        assert rc == E_UNSUPPORTED and "auxiliaries" in h.error()
        assert hip_lib.lib().tmpc_law_add(h.ptr, 0, 1, np.zeros(64, np.uint32).ctypes.data, None) == 0        # (variant 0 alone has none)
        return
    rc, msg = _call(hip_lib, h, name, variant=True)
    assert rc == E_UNSUPPORTED and "auxiliaries" in msg
    assert _call(hip_lib, h, name)[0] == E_DEVICE          # (variant 0 alone has none)


def test_table_entries_check_their_arguments(hip_lib, handles):
    h = handles["plain"]
    L = hip_lib.lib()
    assert L.tmpc_law_add(None, 0, 0, None, None) == E_INVALID
    assert L.tmpc_law_add(h.ptr, 1, 0, None, None) == E_INVALID and "variant out of range" in h.error()
    assert L.tmpc_law_add(h.ptr, 0, 1, None, None) == E_INVALID and h.error() == "tmpc_law_add: NULL argument"
    assert L.tmpc_law_add(h.ptr, 0, -1, None, None) == E_INVALID
    assert L.tmpc_law_add(h.ptr, 0, 0, None, None) == 0
    nc = hip_lib.get_dims(h, 0)[1]
    # the empty set is a region; a bit beyond nc and a set with more rows than variables are refused one by one
    w = np.zeros((3, (nc + 31) // 32), np.uint32)
    w[1, -1] = np.uint32(1 << 31) if nc % 32 else 0
    w[2, :] = 0xFFFFFFFF
    ids = hip_lib.law_add(h, w)
    assert ids[0] == 0 and ids[2] == -1 and (ids[1] == -1 or nc % 32 == 0)
    r = hip_lib.law_get_region(h, 0)
    m = E.law_model(h, 0)
    t = E.region_law(m, [])
    assert np.max(np.abs(r["Ky"] - t["Ky"])) <= 1e-9 * np.abs(t["Ky"]).max() and np.max(np.abs(r["s"] - t["s"])) <= 1e-9 * np.abs(t["s"]).max()
    pr = hip_lib.get_param_rows(h, 0)
    assert pr["Ep"].shape == (hip_lib.get_dims(h, 0)[2], h.nx) and np.array_equal(r["S"][nc:, :h.nx], pr["Ep"]) and not r["S"][nc:, h.nx:].any()
    assert np.array_equal(r["s"][nc:], pr["gp0"] + E.FEAS_TOL)
    assert L.tmpc_get_param_rows(h.ptr, 3, None, None) == E_INVALID
    hip_lib.law_reorder(h)                # host-only: by id, no counters
    hip_lib.law_clear(h)


def test_refusals_of_the_handle_free_entry(hip_lib):
    L = hip_lib.lib()
    c = lc.clipped_case(1, 4, 8, 3, 2)
    m = c["model"]
    arr = {k: np.ascontiguousarray(m[k]) for k in ("H", "F", "G", "g0", "Ebar", "Y", "Yp")}
    arr["P"] = np.ascontiguousarray(c["P"])
    arr["words"] = np.zeros((2, 1), np.uint32)
    arr["order"] = np.arange(2, dtype=np.int32)
    y, region = np.zeros((2, 4)), np.zeros(2, np.int32)

    def call(device=0, nv=4, nc=8, npar=3, ny=4, B=2, n_sets=2, n_order=2, null=None, order=None):
        p = {k: v.ctypes.data for k, v in arr.items()}
        p.update(y=y.ctypes.data, region=region.ctypes.data)
        if order is not None:
            p["order"] = order.ctypes.data
        if null:
            p[null] = None
        rc = L.tmpc_qp_law_eval(device, nv, nc, npar, ny, p["H"], p["F"], p["G"], p["g0"], p["Ebar"], p["Y"], p["Yp"], n_sets, p["words"], n_order, p["order"], B,
                                p["P"], None, 0, p["y"], p["region"], None)
        return rc, L.tmpc_last_error(None).decode()

    for kw, frag in ((dict(nv=0), "nv = 0 is not in [1, 128]"), (dict(nv=129), "nv = 129"), (dict(npar=33), "np = 33 is not in [1, 32]"), (dict(npar=0), "np = 0"),
                     (dict(ny=4097), "ny = 4097"), (dict(ny=0), "ny = 0"), (dict(nc=-1), "nc = -1"), (dict(nc=(1 << 20) + 1), "nc ="), (dict(B=-1), "B < 0"),
                     (dict(n_sets=-1), "n_sets"), (dict(order=np.array([0, 2], np.int32)), "order[1] is not a set")) + tuple(
                         (dict(null=k), "NULL argument") for k in ("H", "F", "G", "g0", "Ebar", "Y", "Yp", "P", "words", "order", "y", "region")):
        rc, msg = call(**kw)
        assert rc == E_INVALID and msg.startswith("tmpc_qp_law_eval: ") and frag in msg, (kw, rc, msg)
    assert call(B=0)[0] == 0
    rc, msg = call(device=-1)
    assert rc == E_DEVICE and "device < 0" in msg


# ------------------------------------------------------------------ 5: the kernel's source on the host execution model
@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    """The host-model programs under the sanitizers (tests/wavesim/hostsim.py: a host without their runtimes skips, a program that does not
    build fails).  Stand-alone programs: nothing is loaded into Python under a sanitizer."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "wavesim"))
    import hostsim
    import law_case
    return law_case, hostsim.binaries_or_skip(tmp_path_factory, "lawsim")


@pytest.mark.parametrize("build", ["lawsim_asan", "lawsim_msan"])
@pytest.mark.parametrize("shape", [(1, 2, 1), (17, 65, 8), (128, 2049, 32)])
def test_kernel_source_on_the_host_model(binaries, build, shape):
    """csrc/tmpc_law.hip compiled for the CPU under ASan + UBSan and under MSan, outputs uninitialised, exact-size blocks: the clipped family
    with B in {1, 65} (one wave and four waves taking turns), hints valid, absent and out of range, max_tries 0, 1 and 2 -- region, tries and
    the hit counters equal the twin's, y the closed form."""
    import hostsim
    law_case, bins = binaries
    nv, nc, npar = shape
    for B in (1, 65):
        c = lc.clipped_case(7 * nv + B, nv, nc, npar, B)
        sets, _ = lc.table_of(c, 9)
        table = [E.region_law(c["model"], s) for s in sets]
        table[4] = None if nv > 1 else table[4]           # a refused set holds no p
        order = np.random.default_rng(B).permutation(9)
        hint = np.array([(-1, 2, 9, 0)[b % 4] for b in range(B)], np.int32)
        for mt, hn in ((0, None), (0, hint), (1, hint), (2, None)):
            out = law_case.run(bins[build], table, c["P"], hint=hn, order=order, max_tries=mt, env=hostsim.SAN_ENV)
            hostsim.assert_clean(out["stderr"])
            region, tries, y = E.locate(table, c["P"], hint=hn, order=order, max_tries=mt)
            assert np.array_equal(out["region"], region) and np.array_equal(out["tries"], tries), (shape, B, mt)
            hit = region >= 0
            assert np.all(np.isnan(out["y"][~hit]))
            assert np.max(np.abs(out["y"][hit] - c["Z"][hit]), initial=0.0) <= 1e-11 * max(1.0, float(np.abs(c["Z"]).max()))
            assert np.array_equal(out["hits"], np.bincount(region[hit], minlength=9).astype(np.uint64))
        assert (E.locate(table, c["P"])[0] >= 0).any()


# ------------------------------------------------------------------ the kernel's code object
def test_law_kernel_has_no_scratch(hip_lib):
    spec = importlib.util.spec_from_file_location("code_object_notes", os.path.join(ROOT, "scripts", "code_object_notes.py"))
    notes = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(notes)
    ks = notes.kernels(os.path.join(common.PKG, "lib", "libtmpc_hip.so"))
    dm = notes.demangle(list(ks))
    law = {dm[n]: k for n, k in ks.items() if "law_kernel" in dm[n]}
    assert len(law) == 1, sorted(law)
    for n, k in law.items():
        assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0, (n, k[".private_segment_fixed_size"], k[".vgpr_spill_count"])
        assert k[".vgpr_count"] <= 128 and k[".agpr_count"] == 0, (n, k[".vgpr_count"], k[".agpr_count"])      # four waves per SIMD, as the sensitivity kernel
        # none of the name filters of tests/test_code_objects.py catches it
        assert not any(f in n for f in ("::solve_kernel<", "::closed_loop", "::solve_block_kernel<", "mc_step_kernel", "::lp_kernel<")), n
