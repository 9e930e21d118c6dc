"""Every answer the closed-loop entry points (include/tmpc.h: tmpc_mc_run, tmpc_mc_replay, tmpc_mc_open, tmpc_reg_run, the steps and
tmpc_mc_close) give before they touch a device, on host-only handles: a table of calls and the (code, message) each one returns.  The
entry points share their argument checks; the table is what callers have seen from each of them, the order of the checks included
(a host-only handle makes it visible: which refusal comes before "host-only handle" differs between tmpc_mc_run and tmpc_mc_open)."""
import numpy as np
import pytest

import common
import regulator_problems
from LinearMPCOverNetworks import _native

OK, E_INVALID, E_DEVICE = 0, -1, -3          # include/tmpc.h
B, T = 2, 3
HOST_ONLY = (E_DEVICE, "host-only handle (device < 0): nothing can be solved without the GPU")

# the arguments of each entry point behind the handle, in order: (name, shape of a float64 array | dtype and shape | a number)
ENTRY = {
    "tmpc_mc_run": [("B", B), ("T", T), ("extended", 0), ("p_loss", "B"), ("ref", "T"), ("th_u", "B T"), ("ga_u", "B T"), ("w", "B T nx"),
                    ("x0", None), ("HZ", None), ("hZ", None), ("rZ", 0)] + [(k, None) for k in ("err2", "tube", "nopt", "xf", "cons", "its")],
    "tmpc_mc_replay": [("B", B), ("T", T), ("extended", 0), ("U", "B T N1 nu"), ("xn0", None), ("theta", "u8 B T"), ("gamma", "u8 B T"),
                       ("w", "B T nx"), ("x0", None), ("trace_f", "B T 3nx+nu"), ("trace_i", "i32 B T 3")],
    "tmpc_mc_open": [("B", B), ("T", T), ("extended", 0), ("p_loss", "B"), ("ref", "T"), ("th_u", "B T"), ("ga_u", "B T"), ("x0", None),
                     ("HZ", None), ("hZ", None), ("rZ", 0), ("HX", None), ("hX", None), ("rX", 0), ("HU", None), ("hU", None), ("rU", 0)],
    "tmpc_reg_run": [("B", B), ("T", T), ("x0", "B nx"), ("w", None), ("HX", None), ("hX", None), ("rX", 0), ("HU", None), ("hU", None),
                     ("rU", 0), ("HZ", None), ("hZ", None), ("rZ", 0)] + [(k, None) for k in ("cost", "xv", "uv", "tv", "nopt", "fail", "xf", "its")]
                    + [("capture", -1), ("cap_x", None), ("cap_xn", None), ("cap_u", None)],
    "tmpc_mc_step": [("x", "B nx"), ("u", "B nu")],
    "tmpc_mc_step_device": [("x", "B nx"), ("u", "B nu"), ("stream", None)],
    "tmpc_mc_step_ref": [("x", "B nx"), ("u", "B nu"), ("ref_next", "B nx")],
    "tmpc_mc_step_device_ref": [("x", "B nx"), ("u", "B nu"), ("ref_next", "B nx"), ("stream", None)],
    "tmpc_mc_close": [(k, None) for k in ("err2", "tube", "xv", "uv", "nopt", "cons", "its", "steps")],
}

# (label, handle, entry point, settings on the handle, arguments that differ from ENTRY's (None: NULL; True: an array of 8 rows), answer)
# settings: "channel B=5", "table B=5" (T_tab = 8), "table T_tab=2" (B = 2), "table" / "channel" (fit), "rng", "models B=5", "models"
CASES = [
    # tmpc_mc_run: the argument checks come first, then "host-only handle" -- before extended / gains / the table's fit
    ("run", "plain", "tmpc_mc_run", "", {}, HOST_ONLY),
    ("run no p_loss", "plain", "tmpc_mc_run", "", dict(p_loss=None), (E_INVALID, "tmpc_mc_run: NULL argument")),
    ("run no ref", "plain", "tmpc_mc_run", "", dict(ref=None), (E_INVALID, "tmpc_mc_run: NULL argument")),
    ("run no th_u", "plain", "tmpc_mc_run", "", dict(th_u=None), (E_INVALID, "tmpc_mc_run: NULL argument")),
    ("run no ga_u", "plain", "tmpc_mc_run", "", dict(ga_u=None), (E_INVALID, "tmpc_mc_run: NULL argument")),
    ("run no w", "plain", "tmpc_mc_run", "", dict(w=None), (E_INVALID, "tmpc_mc_run: NULL argument")),
    ("run rZ without arrays", "plain", "tmpc_mc_run", "", dict(rZ=4), (E_INVALID, "tmpc_mc_run: NULL argument")),
    ("run rZ without hZ", "plain", "tmpc_mc_run", "", dict(rZ=8, HZ=True), (E_INVALID, "tmpc_mc_run: NULL argument")),
    ("run B < 0", "plain", "tmpc_mc_run", "", dict(B=-1), (E_INVALID, "tmpc_mc_run: NULL argument")),
    ("run T < 0", "plain", "tmpc_mc_run", "", dict(T=-1), (E_INVALID, "tmpc_mc_run: NULL argument")),
    ("run B = 0", "plain", "tmpc_mc_run", "", dict(B=0), HOST_ONLY),
    ("run T = 0", "plain", "tmpc_mc_run", "", dict(T=0), HOST_ONLY),
    ("run rng, no draws", "plain", "tmpc_mc_run", "rng", dict(th_u=None, ga_u=None, w=None), HOST_ONLY),
    ("run channel, no p_loss", "plain", "tmpc_mc_run", "channel", dict(p_loss=None), HOST_ONLY),
    ("run table, no ref", "plain", "tmpc_mc_run", "table", dict(ref=None), HOST_ONLY),
    ("run on a regulator", "reg", "tmpc_mc_run", "", {}, (E_INVALID, "tmpc_mc_run: a regulator handle runs its loop with tmpc_reg_run")),
    ("run NULL on a regulator", "reg", "tmpc_mc_run", "", dict(ref=None), (E_INVALID, "tmpc_mc_run: NULL argument")),
    ("run channel of another B", "plain", "tmpc_mc_run", "channel B=5", {},
     (E_INVALID, "tmpc_mc_run: B = 2, but the loss channel was set for B = 5 trajectories")),
    ("run table of another B", "plain", "tmpc_mc_run", "table B=5", {}, HOST_ONLY),
    ("run table too short", "plain", "tmpc_mc_run", "table T_tab=2", {}, HOST_ONLY),
    ("run extended, one problem", "plain", "tmpc_mc_run", "", dict(extended=1), HOST_ONLY),
    ("run extended", "ext", "tmpc_mc_run", "", dict(extended=1), HOST_ONLY),
    ("run without gains", "nogains", "tmpc_mc_run", "", {}, HOST_ONLY),
    # tmpc_mc_replay: its own NULL check, then tmpc_mc_run's checks under tmpc_mc_run's name; the channel and the table are ignored
    ("replay", "plain", "tmpc_mc_replay", "", {}, HOST_ONLY),
    ("replay no U", "plain", "tmpc_mc_replay", "", dict(U=None), (E_INVALID, "tmpc_mc_replay: NULL argument")),
    ("replay no theta", "plain", "tmpc_mc_replay", "", dict(theta=None), (E_INVALID, "tmpc_mc_replay: NULL argument")),
    ("replay no gamma", "plain", "tmpc_mc_replay", "", dict(gamma=None), (E_INVALID, "tmpc_mc_replay: NULL argument")),
    ("replay no w", "plain", "tmpc_mc_replay", "", dict(w=None), (E_INVALID, "tmpc_mc_replay: NULL argument")),
    ("replay no trace_f", "plain", "tmpc_mc_replay", "", dict(trace_f=None), (E_INVALID, "tmpc_mc_replay: NULL argument")),
    ("replay no trace_i", "plain", "tmpc_mc_replay", "", dict(trace_i=None), (E_INVALID, "tmpc_mc_replay: NULL argument")),
    ("replay extended, no xn0", "ext", "tmpc_mc_replay", "", dict(extended=1), (E_INVALID, "tmpc_mc_replay: NULL argument")),
    ("replay B < 0", "plain", "tmpc_mc_replay", "", dict(B=-1), (E_INVALID, "tmpc_mc_replay: NULL argument")),
    ("replay T < 0", "plain", "tmpc_mc_replay", "", dict(T=-1), (E_INVALID, "tmpc_mc_replay: NULL argument")),
    ("replay on a regulator", "reg", "tmpc_mc_replay", "", {}, (E_INVALID, "tmpc_mc_run: a regulator handle runs its loop with tmpc_reg_run")),
    ("replay channel of another B", "plain", "tmpc_mc_replay", "channel B=5", {}, HOST_ONLY),
    ("replay table of another B", "plain", "tmpc_mc_replay", "table B=5", {}, HOST_ONLY),
    ("replay extended, one problem", "plain", "tmpc_mc_replay", "", dict(extended=1, xn0="B T nx"), HOST_ONLY),
    # tmpc_mc_open: regulator, counts, NULL arguments, the channel's fit, extended, gains -- then "host-only handle", before the table's fit
    ("open", "plain", "tmpc_mc_open", "", {}, HOST_ONLY),
    ("open extended", "ext", "tmpc_mc_open", "", dict(extended=1), HOST_ONLY),
    ("open on a regulator", "reg", "tmpc_mc_open", "", {}, (E_INVALID, "tmpc_mc_open: a regulator handle has no stepped loop")),
    ("open NULL on a regulator", "reg", "tmpc_mc_open", "", dict(ref=None), (E_INVALID, "tmpc_mc_open: a regulator handle has no stepped loop")),
    ("open B < 0", "plain", "tmpc_mc_open", "", dict(B=-1), (E_INVALID, "tmpc_mc_open: need B > 0, T > 0 and row counts >= 0")),
    ("open B = 0", "plain", "tmpc_mc_open", "", dict(B=0), (E_INVALID, "tmpc_mc_open: need B > 0, T > 0 and row counts >= 0")),
    ("open T < 0", "plain", "tmpc_mc_open", "", dict(T=-3), (E_INVALID, "tmpc_mc_open: need B > 0, T > 0 and row counts >= 0")),
    ("open T = 0", "plain", "tmpc_mc_open", "", dict(T=0), (E_INVALID, "tmpc_mc_open: need B > 0, T > 0 and row counts >= 0")),
    ("open rZ < 0", "plain", "tmpc_mc_open", "", dict(rZ=-1), (E_INVALID, "tmpc_mc_open: need B > 0, T > 0 and row counts >= 0")),
    ("open rX < 0", "plain", "tmpc_mc_open", "", dict(rX=-1), (E_INVALID, "tmpc_mc_open: need B > 0, T > 0 and row counts >= 0")),
    ("open rU < 0", "plain", "tmpc_mc_open", "", dict(rU=-1), (E_INVALID, "tmpc_mc_open: need B > 0, T > 0 and row counts >= 0")),
    ("open counts before NULL", "plain", "tmpc_mc_open", "", dict(B=0, ref=None), (E_INVALID, "tmpc_mc_open: need B > 0, T > 0 and row counts >= 0")),
    ("open no p_loss", "plain", "tmpc_mc_open", "", dict(p_loss=None), (E_INVALID, "tmpc_mc_open: NULL argument")),
    ("open no ref", "plain", "tmpc_mc_open", "", dict(ref=None), (E_INVALID, "tmpc_mc_open: NULL argument")),
    ("open no th_u", "plain", "tmpc_mc_open", "", dict(th_u=None), (E_INVALID, "tmpc_mc_open: NULL argument")),
    ("open no ga_u", "plain", "tmpc_mc_open", "", dict(ga_u=None), (E_INVALID, "tmpc_mc_open: NULL argument")),
    ("open rZ without arrays", "plain", "tmpc_mc_open", "", dict(rZ=4), (E_INVALID, "tmpc_mc_open: NULL argument")),
    ("open rX without arrays", "plain", "tmpc_mc_open", "", dict(rX=2), (E_INVALID, "tmpc_mc_open: NULL argument")),
    ("open rU without hU", "plain", "tmpc_mc_open", "", dict(rU=8, HU=True), (E_INVALID, "tmpc_mc_open: NULL argument")),
    ("open rng, no draws", "plain", "tmpc_mc_open", "rng", dict(th_u=None, ga_u=None), HOST_ONLY),
    ("open channel, no p_loss", "plain", "tmpc_mc_open", "channel", dict(p_loss=None), HOST_ONLY),
    ("open table, no ref", "plain", "tmpc_mc_open", "table", dict(ref=None), HOST_ONLY),
    ("open channel of another B", "plain", "tmpc_mc_open", "channel B=5", {},
     (E_INVALID, "tmpc_mc_open: B = 2, but the loss channel was set for B = 5 trajectories")),
    ("open table of another B", "plain", "tmpc_mc_open", "table B=5", {}, HOST_ONLY),
    ("open table too short", "plain", "tmpc_mc_open", "table T_tab=2", {}, HOST_ONLY),
    ("open extended, one problem", "plain", "tmpc_mc_open", "", dict(extended=1),
     (E_INVALID, "tmpc_mc_open: extended loop needs a problem created with extended = 1")),
    ("open without gains", "nogains", "tmpc_mc_open", "", {}, (E_INVALID, "tmpc_mc_open: the problem description carries no gains K / K_anc")),
    # tmpc_reg_run
    ("reg", "reg", "tmpc_reg_run", "", {}, HOST_ONLY),
    ("reg with w", "reg", "tmpc_reg_run", "", dict(w="B T nx"), HOST_ONLY),
    ("reg B = 0", "reg", "tmpc_reg_run", "", dict(B=0), HOST_ONLY),
    ("reg on a tracking handle", "plain", "tmpc_reg_run", "", {},
     (E_INVALID, "tmpc_reg_run: needs a regulator handle (tmpc_create_regulator); tracking handles run tmpc_mc_run")),
    ("reg NULL on a tracking handle", "plain", "tmpc_reg_run", "", dict(x0=None),
     (E_INVALID, "tmpc_reg_run: needs a regulator handle (tmpc_create_regulator); tracking handles run tmpc_mc_run")),
    ("reg no x0", "reg", "tmpc_reg_run", "", dict(x0=None), (E_INVALID, "tmpc_reg_run: NULL argument or negative count")),
    ("reg B < 0", "reg", "tmpc_reg_run", "", dict(B=-1), (E_INVALID, "tmpc_reg_run: NULL argument or negative count")),
    ("reg T < 0", "reg", "tmpc_reg_run", "", dict(T=-1), (E_INVALID, "tmpc_reg_run: NULL argument or negative count")),
    ("reg rX < 0", "reg", "tmpc_reg_run", "", dict(rX=-1), (E_INVALID, "tmpc_reg_run: NULL argument or negative count")),
    ("reg rU < 0", "reg", "tmpc_reg_run", "", dict(rU=-1), (E_INVALID, "tmpc_reg_run: NULL argument or negative count")),
    ("reg rZ < 0", "reg", "tmpc_reg_run", "", dict(rZ=-1), (E_INVALID, "tmpc_reg_run: NULL argument or negative count")),
    ("reg rX without arrays", "reg", "tmpc_reg_run", "", dict(rX=2), (E_INVALID, "tmpc_reg_run: NULL argument or negative count")),
    ("reg rU without hU", "reg", "tmpc_reg_run", "", dict(rU=8, HU=True), (E_INVALID, "tmpc_reg_run: NULL argument or negative count")),
    ("reg rZ without HZ", "reg", "tmpc_reg_run", "", dict(rZ=8, hZ=True), (E_INVALID, "tmpc_reg_run: NULL argument or negative count")),
    ("reg models of another B", "reg", "tmpc_reg_run", "models B=5", {},
     (E_INVALID, "tmpc_reg_run: B = 2, but the plant models were set for B = 5 trajectories")),
    ("reg models", "reg", "tmpc_reg_run", "models", {}, HOST_ONLY),
    # the steps and the close of a session that is not open
    ("step", "plain", "tmpc_mc_step", "", {}, (E_INVALID, "tmpc_mc_step: no stepped closed loop is open on this handle (tmpc_mc_open)")),
    ("step NULL", "plain", "tmpc_mc_step", "", dict(x=None), (E_INVALID, "tmpc_mc_step: no stepped closed loop is open on this handle (tmpc_mc_open)")),
    ("step_device", "plain", "tmpc_mc_step_device", "", {},
     (E_INVALID, "tmpc_mc_step_device: no stepped closed loop is open on this handle (tmpc_mc_open)")),
    ("step_ref", "plain", "tmpc_mc_step_ref", "", {}, (E_INVALID, "tmpc_mc_step_ref: no stepped closed loop is open on this handle (tmpc_mc_open)")),
    ("step_ref with a table", "plain", "tmpc_mc_step_ref", "table", {},
     (E_INVALID, "tmpc_mc_step_ref: no stepped closed loop is open on this handle (tmpc_mc_open)")),
    ("step_device_ref", "plain", "tmpc_mc_step_device_ref", "", {},
     (E_INVALID, "tmpc_mc_step_device_ref: no stepped closed loop is open on this handle (tmpc_mc_open)")),
    ("step on a regulator", "reg", "tmpc_mc_step", "", {}, (E_INVALID, "tmpc_mc_step: no stepped closed loop is open on this handle (tmpc_mc_open)")),
    ("close", "plain", "tmpc_mc_close", "", {}, (E_INVALID, "tmpc_mc_close: no stepped closed loop is open on this handle (tmpc_mc_open)")),
    ("close on a regulator", "reg", "tmpc_mc_close", "", {}, (E_INVALID, "tmpc_mc_close: no stepped closed loop is open on this handle (tmpc_mc_open)")),
]


@pytest.fixture(scope="module")
def handles(hip_lib):
    """Host-only handles: the cart-pole at N = 10 (plain, extended, and the plain one created without its gains) and the
    double-integrator regulator."""
    plain, _ = common.make_mpc("cartpole", 10, True, create=True, device=-1)
    ext, _ = common.make_mpc("cartpole", 10, True, extended=True, create=True, device=-1)
    reg = regulator_problems.plain_double_integrator(device=-1)
    bare = dict(plain._problem_dict())
    bare["K"] = bare["K_anc"] = None
    nogains = _native.create(bare, device=-1)
    yield dict(plain=plain._handle, ext=ext._handle, reg=reg._handle, nogains=nogains)
    plain._close()
    ext._close()
    reg._close()
    _native.destroy(nogains)


def apply_settings(h, what):
    """Puts the settings named in `what` on the handle; everything else is cleared, so no case sees another's."""
    L = _native.lib()
    if not h.regulator:
        nb = 5 if what == "channel B=5" else B
        _native.mc_set_channel(h, dict(p_gb=0.1, p_bg=0.5, e_g=0.0, e_b=1.0) if what.startswith("channel") else None, nb)
        tab = None
        if what.startswith("table"):
            tab = np.zeros((1, 2 if what == "table T_tab=2" else 8, h.nx))
        _native.mc_set_reference(h, tab, B=(5 if what == "table B=5" else B) if tab is not None else None)
    else:
        _native.mc_set_plant_models(h, "linear", np.ones((5 if what == "models B=5" else B, h.nx, h.nx + h.nu)) if what.startswith("models") else None)
    wb = np.ones(h.nx)
    assert L.tmpc_mc_set_device_rng(h.ptr, int(what == "rng"), 7, 0, wb.ctypes.data) == OK


def call(h, entry, over):
    """The entry point on the handle with ENTRY's arguments, `over` replacing some -> (code, message)."""
    dims = dict(B=max(over.get("B", B), 1), T=max(over.get("T", T), 1), nx=h.nx, nu=h.nu, N1=h.N + 1)
    dims["3nx+nu"] = 3 * h.nx + h.nu
    keep, args = [], []
    for name, default in ENTRY[entry]:
        v = over.get(name, default)
        if v is True:
            v = "8 8"
        if isinstance(v, str):
            dtype = {"u8": np.uint8, "i32": np.int32}.get(v.split()[0], np.float64)
            a = np.zeros([dims[k] if k in dims else int(k) for k in v.split() if k not in ("u8", "i32")], dtype)
            keep.append(a)
            v = a.ctypes.data
        args.append(v)
    rc = getattr(_native.lib(), entry)(h.ptr, *args)
    return rc, h.error()


@pytest.mark.parametrize("label,handle,entry,settings,over,answer", CASES, ids=[c[0] for c in CASES])
def test_refusal(handles, label, handle, entry, settings, over, answer):
    h = handles[handle]
    apply_settings(h, settings)
    try:
        got = call(h, entry, over)
    finally:
        apply_settings(h, "")
    assert got == answer, label


def test_every_entry_point_refuses_a_null_handle(hip_lib):
    for entry, spec in ENTRY.items():
        args = [d if isinstance(d, int) and not isinstance(d, bool) else None for _, d in spec]
        assert getattr(_native.lib(), entry)(None, *args) == E_INVALID, entry
