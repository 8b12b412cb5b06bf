"""The optimizer tail of the reference's fine-tuning loops on the library's own kernels (include/sdc.h, sdc_optim_step):

    loss.backward(); clip_grad_norm_(params, 1.0); optimizer.step(); optimizer.zero_grad(); scheduler.step(); ema.update()

(1D/inference/inference_ft.py:189-226, the tokamak twin, 2d/inference_2d.py:261-281) becomes

    opt = sdc.FusedOptimizer(net.parameters(), kind="adam", lr=1e-4, betas=(0.9, 0.99), max_grad_norm=1.0)
    opt.attach_ema(ema_net, beta=0.995, update_every=10)
    loss.backward(); opt.step(); opt.zero_grad(); scheduler.step()

Gradient norm, clipping, SGD / Adam / AdamW and the EMA twin's update run as three launches over all parameters, whatever their
number.  Learning rate, step count, bias corrections and the every-N-th EMA decision are read from device memory, so a step
recorded by ``GraphedLossStep(optimizer=opt)`` follows a scheduler and counts its own steps.

Differences from the torch loop, all deliberate:
  * ``.grad`` is NOT rewritten by clipping (the clipped value is used, never stored);
  * bias corrections are computed in fp64 on the device (the value torch's non-capturable optimizers compute on the host);
  * the EMA covers parameters only: a twin's buffers are not handled (the drop-in nets have none that train).
"""
import ctypes as C

import torch

from . import _lib
from ._lib import SdcOptItem, check

__all__ = ["FusedOptimizer"]

_KINDS = {"sgd": 0, "adam": 1, "adamw": 2}
_CLIP, _SKIP_NONFINITE = 1, 2


def _check_tensor(t, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise RuntimeError(f"FusedOptimizer: {what} must be a contiguous fp32 tensor on a cuda (HIP) device; there is no CPU fallback")


class FusedOptimizer(torch.optim.Optimizer):
    """``FusedOptimizer(params, kind="adam"|"adamw"|"sgd", lr, betas, eps, weight_decay, momentum, max_grad_norm, skip_nonfinite)``.

    One param group; fp32, contiguous, CUDA parameters (RuntimeError otherwise).  SGD is torch's with ``momentum``, dampening 0, no
    Nesterov; Adam adds ``weight_decay * p`` to the gradient, AdamW decays the parameter; no amsgrad, no maximize.
    ``max_grad_norm > 0`` clips the total gradient norm every step like ``clip_grad_norm_`` (or arm one step with
    :meth:`clip_grad_norm_`); ``skip_nonfinite`` leaves parameters, moments, EMA and step count untouched when the norm is NaN / Inf
    (what GradScaler does for the reference's fp16 runs).  Moments live in ``opt.state[p]`` under torch's names; ``state_dict()``
    loads into the matching ``torch.optim`` class and back.
    """

    def __init__(self, params, kind="adam", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum=0.9, max_grad_norm=0.0,
                 skip_nonfinite=False):
        if kind not in _KINDS:
            raise ValueError(f"FusedOptimizer: kind {kind!r} (one of {sorted(_KINDS)})")
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or momentum < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("FusedOptimizer: negative or out-of-range hyper-parameter")
        # the keys of torch.optim.SGD / Adam / AdamW groups ride along so that state_dict() loads into those classes
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, momentum=momentum, max_grad_norm=max_grad_norm,
                        dampening=0.0, nesterov=False, amsgrad=False, maximize=False)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise RuntimeError("FusedOptimizer: one param group only")
        self.kind, self.skip_nonfinite = kind, bool(skip_nonfinite)
        ps = self.param_groups[0]["params"]
        for p in ps:
            _check_tensor(p, "every parameter")
        dev = ps[0].device
        if any(p.device != dev for p in ps):
            raise RuntimeError("FusedOptimizer: all parameters on one device")
        self.device = dev
        # SdcOptState: int64 step | float grad_norm, float clip_coef | int applied, int ema_mode
        self._state_dev = torch.zeros(3, dtype=torch.int64, device=dev)
        self._step = self._state_dev[0]
        self._norm, self._coef = self._state_dev[1:2].view(torch.float32).unbind(0)
        self._hp_dev = torch.zeros(9, dtype=torch.float64, device=dev)
        self._hp_sent = None
        self._clip_sent = 0.0
        self._armed = None
        self._ema, self._ema_cfg, self.ema_params = {}, (0.0, 0, 0), []
        self._key = self._table = self._table_host = self._work = self._spare = None
        self._plan = (0, 0, 0, 0)

    def __setstate__(self, state):
        super().__setstate__(state)
        for g in self.param_groups:                      # groups that come from a torch.optim state_dict lack this class's keys
            for k, v in self.defaults.items():
                g.setdefault(k, v)

    # ------------------------------------------------------------------ public surface
    @property
    def grad_norm(self):
        """device tensor: the total gradient norm of the last step that computed it (clipping or skip_nonfinite on)"""
        return self._norm

    @property
    def clip_coef(self):
        """device tensor: the factor the last step multiplied the gradients by"""
        return self._coef

    @property
    def step_count(self):
        """device tensor (int64): steps applied so far"""
        return self._step

    def clip_grad_norm_(self, max_norm):
        """Arm clipping to ``max_norm`` for the next ``step()`` only; returns the device tensor that will hold the total norm
        (the value ``accelerator.clip_grad_norm_`` returns)."""
        self._armed = float(max_norm)
        return self._norm

    def attach_ema(self, ema_model_or_params, beta=0.995, update_every=10, update_after_step=0):
        """Update an EMA twin inside ``step()``: on steps t with ``t % update_every == 0`` the twin's parameters are copied
        from the net while ``t <= update_after_step`` and moved by ``ema += (1 - beta)(p - ema)`` afterwards.  The twin is an
        nn.Module (or an object with ``.ema_model``) or an iterable of tensors, matched to the optimised parameters in order.
        Parameters only -- buffers are not handled."""
        src = getattr(ema_model_or_params, "ema_model", ema_model_or_params)
        twins = list(src.parameters()) if hasattr(src, "parameters") else list(src)
        ps = self.param_groups[0]["params"]
        if len(twins) != len(ps):
            raise RuntimeError(f"FusedOptimizer.attach_ema: {len(twins)} EMA tensors for {len(ps)} parameters")
        for i, (p, e) in enumerate(zip(ps, twins)):
            _check_tensor(e, f"EMA tensor {i}")
            if e.shape != p.shape or e.device != p.device:
                raise RuntimeError(f"FusedOptimizer.attach_ema: tensor {i} is {tuple(e.shape)} on {e.device}, the parameter "
                                   f"{tuple(p.shape)} on {p.device}")
        if not (0.0 <= beta <= 1.0) or update_every < 1 or update_after_step < 0:
            raise ValueError("FusedOptimizer.attach_ema: beta in [0, 1], update_every >= 1, update_after_step >= 0")
        self.ema_params = [e.detach() for e in twins]
        self._ema = {p: e for p, e in zip(ps, self.ema_params)}
        self._ema_cfg = (float(beta), int(update_every), int(update_after_step))
        self._key = None

    def sync_hyperparameters(self):
        """Upload the hyper-parameters (``param_groups[0]``, the EMA settings) when they differ from what the device holds: one
        stream-ordered copy of nine doubles.  ``step()`` does this itself; a caller that replays a captured ``step()`` calls it
        before the replay (GraphedLossStep does).  Returns whether the next ``step()`` clips."""
        g = self.param_groups[0]
        clip = self._armed if self._armed is not None else float(g["max_grad_norm"])
        if clip > 0.0:
            self._clip_sent = clip                       # with clipping off the slot is not read: keep it, spare the upload
        b1 = float(g["momentum"]) if self.kind == "sgd" else float(g["betas"][0])
        hp = (float(g["lr"]), b1, float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), self._clip_sent,
              self._ema_cfg[0], float(self._ema_cfg[1] if self._ema else 0), float(self._ema_cfg[2]))
        if hp != self._hp_sent:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedOptimizer: hyper-parameters changed inside a graph capture (the copy would be replayed "
                                   "with these values for ever): call sync_hyperparameters() before the capture")
            # a fresh pinned buffer per upload: an earlier copy may still be pending on the stream (the host allocator keeps a
            # buffer until the copies that read it have run)
            self._hp_dev.copy_(torch.tensor(hp, dtype=torch.float64).pin_memory(), non_blocking=True)
            self._hp_sent = hp
        return clip > 0.0

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # one comparison of a few hundred integers per step: the table (and the checks and the lazily created state behind it)
        # is redone only when a parameter or a gradient moved
        key = [(p.data_ptr(), p.grad.data_ptr(), p.numel()) for p in self.param_groups[0]["params"] if p.grad is not None]
        if not key:
            self._armed = None
            return loss
        if key != self._key:
            self._prepare([p for p in self.param_groups[0]["params"] if p.grad is not None])
            self._key = key
        flags = (_CLIP if self.sync_hyperparameters() else 0) | (_SKIP_NONFINITE if self.skip_nonfinite else 0)
        self._armed = None
        n, chunk, total, grid = self._plan
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            check(_lib.get_lib().sdc_optim_step(_KINDS[self.kind], self._table.data_ptr(), n, chunk, total, grid, self._hp_dev.data_ptr(),
                                                self._state_dev.data_ptr(), self._work.data_ptr(), flags, stream), "sdc_optim_step")
        return loss

    # ------------------------------------------------------------------ item table
    def _prepare(self, ps):
        """check the tensors, create missing state (zeros, as torch does in its first step) and (re)build and upload the
        SdcOptItem table: when the set of (parameter, gradient) addresses moved -- zero_grad(set_to_none=True) moves the gradients
        in eager use, a captured step keeps them -- or load_state_dict / attach_ema replaced tensors.  Moment tensors in
        ``opt.state`` are updated in place; replace one by hand and the table must be rebuilt (``load_state_dict`` does)."""
        adam = self.kind != "sgd"
        rows = []
        for p in ps:
            _check_tensor(p, "every parameter")
            _check_tensor(p.grad, "every gradient")
            st = self.state[p]
            st["step"] = self._step
            if adam:
                if "exp_avg" not in st:
                    st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
            elif st.get("momentum_buffer") is None:
                st["momentum_buffer"] = torch.zeros_like(p)
            m = st["exp_avg"] if adam else st["momentum_buffer"]
            v = st["exp_avg_sq"] if adam else None
            e = self._ema.get(p)
            for t, what in ((m, "first moment"), (v, "second moment")):
                if t is not None:
                    _check_tensor(t, what)
                    if t.shape != p.shape:
                        raise RuntimeError(f"FusedOptimizer: {what} of shape {tuple(t.shape)} for a parameter {tuple(p.shape)}")
            rows.append((p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr() if adam else 0, e.data_ptr() if e is not None else 0,
                         p.numel()))
        items = (SdcOptItem * len(rows))()
        for it, (pp, gg, mm, vv, ee, n) in zip(items, rows):
            it.p, it.g, it.m, it.v, it.ema, it.n = pp, gg, mm, vv or None, ee or None, n
        chunk, total, grid = C.c_int(), C.c_int(), C.c_int()
        lib = _lib.get_lib()
        check(lib.sdc_optim_plan(items, len(rows), _KINDS[self.kind], C.byref(chunk), C.byref(total), C.byref(grid)), "sdc_optim_plan")
        nbytes = C.sizeof(items)
        # A fresh pinned source per upload (an earlier copy may still be pending on the stream); it stays alive with the table,
        # because a captured step() replays this copy from it.  Inside a capture no pinned memory is allocated: the spare that
        # an earlier eager build (GraphedLossStep's warm-up step) set aside, never yet the source of a copy, is used.
        cap = C.sizeof(SdcOptItem) * len(self.param_groups[0]["params"])
        if torch.cuda.is_current_stream_capturing() and self._spare is not None:
            host, self._spare = self._spare, None
        else:
            host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
            if self._spare is None:
                self._spare = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
        host = host[:nbytes]
        C.memmove(host.data_ptr(), items, nbytes)
        table = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        table.copy_(host, non_blocking=True)
        need = lib.sdc_optim_bytes(total.value)
        if self._work is None or self._work.numel() * 8 < need:
            self._work = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
        self._table, self._table_host = table, host
        self._plan = (len(rows), chunk.value, total.value, grid.value)

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """torch's layout: per-parameter ``step`` entries are separate fp32 CPU scalars (what ``torch.optim.Adam`` writes), so
        the result loads into ``torch.optim.SGD`` / ``Adam`` / ``AdamW``.  Reads the device step counter (one synchronisation)."""
        sd = super().state_dict()
        t = float(self._step.item())
        sd["state"] = {k: dict(st) for k, st in sd["state"].items()}       # the packed entries ARE self.state's dicts
        for st in sd["state"].values():
            if "step" in st:
                st["step"] = torch.tensor(t, dtype=torch.float32)
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        steps = set()
        for p, st in self.state.items():
            if "step" in st:
                steps.add(int(float(st["step"])))
            for k in ("exp_avg", "exp_avg_sq", "momentum_buffer"):
                if torch.is_tensor(st.get(k)):
                    # a copy: torch's cast returns the SOURCE optimizer's tensor when device and dtype already match
                    st[k] = st[k].to(device=p.device, dtype=torch.float32).clone(memory_format=torch.contiguous_format)
        if len(steps) > 1:
            raise RuntimeError(f"FusedOptimizer.load_state_dict: parameters at different step counts {sorted(steps)}: one counter "
                               "serves all of them")
        self._step.fill_(steps.pop() if steps else 0)
        for st in self.state.values():
            st["step"] = self._step
        self._key = None
