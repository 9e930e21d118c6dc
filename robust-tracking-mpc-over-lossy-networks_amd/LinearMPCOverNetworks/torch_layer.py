"""The batched MPC solve as a differentiable torch layer.

    layer = MPCLayer(mpc)                      # a controller with a device handle
    u_nom, x_nom0, xu_ss = layer(x, ref)       # float64 tensors on the handle's device, (B, nx) each
    cost(u_nom).backward()                     # gradients flow to x and ref

forward runs tmpc_solve_batch_device, backward tmpc_sens_vjp_device (csrc/tmpc_sens.hip): one right-hand side through the KKT system of
the solution's working set, the Jacobian is never formed.

Stream rule: the handle's streams are its own and are NOT ordered against torch's current stream.  The layer therefore synchronises
torch's current stream before each call into the library (the producers of its inputs have finished) and calls tmpc_synchronize after it
(its outputs are complete before torch reads them).

Instances the sensitivity kernel skips (flag TMPC_SENS_SKIPPED: an infeasible solve, a non-finite input) get a ZERO gradient; their
forward outputs are NaN as the solve leaves them.  `layer.last_flag` / `layer.last_n_active` are the tensors of the last backward call,
`layer.last_status` that of the last forward call.

    layer = TunableMPCLayer(mpc)               # the same, with the weights Q, R, P, T as parameters
    loss(layer(x, ref)[0]).backward()          # layer.Q.grad ... layer.T.grad: summed over the batch

backward of the tunable layer is one tmpc_sens_vjp_weights_device call: the vector-Jacobian products for x and ref and, from the same
KKT solves, the gradients of the four weight matrices (include/tmpc.h).  K, K_anc and the sets are held fixed; the four weights count
as independent symmetric parameters.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native


class _MPCFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layer, x, ref):
        h = layer.handle
        B = x.shape[0]
        dev = x.device
        x = x.detach().contiguous()
        ref = ref.detach().contiguous()
        u = torch.empty((B, h.N, h.nu), dtype=torch.float64, device=dev)
        x0 = torch.empty((B, h.nx), dtype=torch.float64, device=dev)
        ss = torch.empty((B, h.nx + h.nu), dtype=torch.float64, device=dev)
        st = torch.empty(B, dtype=torch.int32, device=dev)
        it = torch.empty(B, dtype=torch.int32, device=dev)
        var = layer._variant_tensor(B, dev)
        torch.cuda.current_stream(dev).synchronize()
        _native.solve_batch_device(h, B, x.data_ptr(), ref.data_ptr(), None if var is None else var.data_ptr(), u.data_ptr(), x0.data_ptr(),
                                   ss.data_ptr(), None, st.data_ptr(), it.data_ptr())
        _native.synchronize(h)
        layer.last_status, layer.last_iters = st, it
        ctx.layer = layer
        ctx.save_for_backward(x, ref, u, x0, ss, st)
        ctx.mark_non_differentiable(st)
        return u, x0, ss, st

    @staticmethod
    def backward(ctx, gu, gx0, gss, _gst):
        layer = ctx.layer
        h = layer.handle
        x, ref, u, x0, ss, st = ctx.saved_tensors
        B = x.shape[0]
        dev = x.device
        zero = lambda g, like: torch.zeros_like(like) if g is None else g.to(torch.float64)
        ybar = torch.cat([zero(gu, u).reshape(B, -1), zero(gx0, x0), zero(gss, ss)], dim=1).contiguous()
        # (the gradient of a NaN output is whatever the consumer made of it: a skipped instance must not poison the batch)
        ybar = torch.nan_to_num(ybar, nan=0.0, posinf=0.0, neginf=0.0)
        pbar = torch.empty((B, 2 * h.nx), dtype=torch.float64, device=dev)
        flag = torch.empty(B, dtype=torch.int32, device=dev)
        nact = torch.empty(B, dtype=torch.int32, device=dev)
        var = layer._variant_tensor(B, dev)
        torch.cuda.current_stream(dev).synchronize()
        _native.sens_vjp_device(h, B, x.data_ptr(), ref.data_ptr(), None if var is None else var.data_ptr(), u.data_ptr(), x0.data_ptr(),
                                ss.data_ptr(), st.data_ptr(), layer.act_tol, ybar.data_ptr(), pbar.data_ptr(), flag.data_ptr(), nact.data_ptr())
        _native.synchronize(h)
        layer.last_flag, layer.last_n_active = flag, nact
        skipped = (flag & _native.SENS_SKIPPED) != 0
        pbar = torch.where(skipped[:, None], torch.zeros_like(pbar), pbar)
        return None, pbar[:, :h.nx], pbar[:, h.nx:]


class MPCLayer(torch.nn.Module):
    """forward(x, ref) -> (u_nom (B, N, nu), x_nom0 (B, nx), xu_ss (B, nx + nu)); `variant`: None, or the problem variant of every
    instance (an int, or a uint8 tensor (B,) on the device) for an extended controller."""

    def __init__(self, mpc, variant=None, act_tol: float = 0.0):
        super().__init__()
        if getattr(mpc, "_handle", None) is None:
            raise RuntimeError("MPCLayer: the controller has no device problem (setup_optimization first)")
        self.mpc = mpc
        self.handle = mpc._handle
        self.variant = variant
        self.act_tol = float(act_tol)
        self.last_status = self.last_iters = self.last_flag = self.last_n_active = None

    def _variant_tensor(self, B, dev):
        if self.variant is None:
            return None
        if torch.is_tensor(self.variant):
            return self.variant.to(device=dev, dtype=torch.uint8).contiguous()
        return torch.full((B,), int(self.variant), dtype=torch.uint8, device=dev)

    def forward(self, x, ref):
        if x.dtype != torch.float64 or ref.dtype != torch.float64 or not x.is_cuda or not ref.is_cuda:
            raise TypeError("MPCLayer: x and ref are float64 tensors on the handle's device")
        x = x.reshape(-1, self.handle.nx)
        ref = ref.reshape(-1, self.handle.nx).expand(x.shape[0], self.handle.nx)
        u, x0, ss, _st = _MPCFunction.apply(self, x, ref)
        return u, x0, ss


class _TunableMPCFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layer, x, ref, Q, R, P, T):
        ctx.wdev = Q.device
        return _MPCFunction.forward(ctx, layer, x, ref)

    @staticmethod
    def backward(ctx, gu, gx0, gss, _gst):
        layer = ctx.layer
        h = layer.handle
        x, ref, u, x0, ss, st = ctx.saved_tensors
        B = x.shape[0]
        dev = x.device
        zero = lambda g, like: torch.zeros_like(like) if g is None else g.to(torch.float64)
        ybar = torch.cat([zero(gu, u).reshape(B, -1), zero(gx0, x0), zero(gss, ss)], dim=1).contiguous()
        ybar = torch.nan_to_num(ybar, nan=0.0, posinf=0.0, neginf=0.0)
        pbar = torch.empty((B, 2 * h.nx), dtype=torch.float64, device=dev)
        flag = torch.empty(B, dtype=torch.int32, device=dev)
        nact = torch.empty(B, dtype=torch.int32, device=dev)
        var = layer._variant_tensor(B, dev)
        torch.cuda.current_stream(dev).synchronize()
        w = _native.sens_vjp_weights_device(h, B, x.data_ptr(), ref.data_ptr(), None if var is None else var.data_ptr(), u.data_ptr(), x0.data_ptr(),
                                            ss.data_ptr(), st.data_ptr(), layer.act_tol, ybar.data_ptr(), pbar.data_ptr(), flag.data_ptr(), nact.data_ptr())
        _native.synchronize(h)
        layer.last_flag, layer.last_n_active = flag, nact
        skipped = (flag & _native.SENS_SKIPPED) != 0
        pbar = torch.where(skipped[:, None], torch.zeros_like(pbar), pbar)
        gw = [torch.from_numpy(w[k]).to(ctx.wdev) for k in ("Qbar", "Rbar", "Pbar", "Tbar")]
        return (None, pbar[:, :h.nx], pbar[:, h.nx:], *gw)


class TunableMPCLayer(MPCLayer):
    """MPCLayer with the weights of the QP as parameters: Q (nx, nx), R (nu, nu), P (nx, nx), T (nx, nx), float64, initialised from
    the controller.  forward(x, ref) re-creates the controller's handle through `mpc.set_cost_weights` when the parameters' values differ
    from those the handle was built with (a refusal of tmpc_create -- an indefinite H -- is raised with the library's message); backward
    returns gradients for x, ref and the four parameters (summed over the batch; the symmetric part, as the QP sees the weights).  The
    parameters live on the CPU: they enter the library through host memory."""

    def __init__(self, mpc, variant=None, act_tol: float = 0.0):
        super().__init__(mpc, variant=variant, act_tol=act_tol)
        self.Q, self.R, self.P, self.T = (torch.nn.Parameter(torch.from_numpy(np.array(W, dtype=np.float64)))
                                          for W in (mpc._Q, mpc._R, mpc._P, mpc._Tout))
        self._built = self._values()

    def _values(self):
        return tuple(p.detach().cpu().numpy().copy() for p in (self.Q, self.R, self.P, self.T))

    def forward(self, x, ref):
        now = self._values()
        if any(not np.array_equal(a, b) for a, b in zip(now, self._built)):
            self.mpc.set_cost_weights(*now)
            self.handle = self.mpc._handle
            self._built = now
        if x.dtype != torch.float64 or ref.dtype != torch.float64 or not x.is_cuda or not ref.is_cuda:
            raise TypeError("TunableMPCLayer: x and ref are float64 tensors on the handle's device")
        x = x.reshape(-1, self.handle.nx)
        ref = ref.reshape(-1, self.handle.nx).expand(x.shape[0], self.handle.nx)
        u, x0, ss, _st = _TunableMPCFunction.apply(self, x, ref, self.Q, self.R, self.P, self.T)
        return u, x0, ss
