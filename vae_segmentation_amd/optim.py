"""Multi-tensor optimiser steps on libvaeseg kernels: one launch per param group instead of the reference's
per-tensor torch.optim loops (main_source.py:279-294, main_target.py:347-352), and the EMA teacher update
(main_target.py:512-516).  Semantics and state keys follow torch.optim.SGD / torch.optim.Adam so optimizer
state_dicts stay interchangeable with the reference's checkpoints (main_source.py:827-843)."""
import collections

import torch

from . import ops
from ._lib import _stream, check, lib

_CHUNK = int(lib.vs_mt_chunk())      # VS_MT_CHUNK: the elements of one tensor a workgroup of the *_multi kernels owns (csrc/optim.hip)


class _Tables:
    """Device-side pointer / size / block tables for a list of tensor tuples; rebuilt only when an address changes."""

    def __init__(self):
        self.key = None
        self.dev = None
        self.n_blocks = 0

    def get(self, lists, device):
        key = tuple(t.data_ptr() for lst in lists for t in lst) + tuple(t.numel() for t in lists[0])
        if key != self.key:
            n = len(lists[0])
            ptrs = [torch.tensor([t.data_ptr() for t in lst], dtype=torch.int64) for lst in lists]
            sizes = torch.tensor([t.numel() for t in lists[0]], dtype=torch.int64)
            bm = []
            for i, t in enumerate(lists[0]):
                for start in range(0, t.numel(), _CHUNK):
                    bm += [i, start]
            bm = torch.tensor(bm, dtype=torch.int32)
            self.dev = [p.to(device) for p in ptrs] + [sizes.to(device), bm.to(device)]
            self.n_blocks = bm.numel() // 2
            self.key = key
        return self.dev, self.n_blocks


class LossScaler:
    """Dynamic loss scaling for fp16 storage (BASELINE configs[4]) with torch.cuda.amp.GradScaler's protocol, entirely on the device:
    the scale, the overflow flag and the growth counter are device scalars, so a captured HIP graph follows them and nothing syncs.

        loss.backward(gradient=scaler.seed)        # every gradient comes out `scale` times too large
        optimizer.step(scaler=scaler)              # checks the gradients, divides by the scale, skips the step on inf / nan, updates the scale
    """

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, device="cuda"):
        self.scale = torch.full((1,), float(init_scale), dtype=torch.float32, device=device)
        self.found_inf = torch.zeros(1, dtype=torch.float32, device=device)
        self.tracker = torch.zeros(1, dtype=torch.int32, device=device)
        self.cfg = (float(growth_factor), float(backoff_factor), int(growth_interval))
        self._tabs = {}                  # one table per caller slot (param group): alternating groups must not rebuild each other's table

    @property
    def seed(self):
        """0-dim view of the scale: pass it as the upstream gradient of the (scalar) loss"""
        return self.scale.view(())

    def prepare(self, grads, slot=0):
        """build the device-side table check(grads, slot) needs (a stream capture cannot contain the host-to-device copy)"""
        return self._tabs.setdefault(slot, _Tables()).get([grads], grads[0].device)

    def check(self, grads, slot=0):
        (gp, sizes, bm), nb = self.prepare(grads, slot)
        check(lib.vs_grad_finite_multi(gp.data_ptr(), sizes.data_ptr(), bm.data_ptr(), nb, self.found_inf.data_ptr(), _stream()), "grad_finite_multi")

    def update(self):
        g, b, i = self.cfg
        check(lib.vs_loss_scale_update(self.scale.data_ptr(), self.tracker.data_ptr(), self.found_inf.data_ptr(), g, b, i, _stream()), "loss_scale_update")


def poly_lr(base, epoch, n_epochs, power=0.9):
    """nnU-Net's polynomial decay, base * (1 - epoch / n_epochs) ** power for 0 <= epoch < n_epochs, in Python floats"""
    if not 0 <= epoch < n_epochs:
        raise ValueError("poly_lr: epoch %r outside [0, %r)" % (epoch, n_epochs))
    return base * (1 - epoch / n_epochs) ** power


class _Group(collections.namedtuple("_Group", "group index params grads params_ptr grads_ptr state_ptrs sizes block_map n_blocks device")):
    """One param group with work in this step: the group and its index, the parameters that have a gradient and those gradients, and the device tables
    of _Tables.get([params, grads, *state buffers]) by name."""
    __slots__ = ()

    @property
    def tables(self):
        """the leading arguments of every step entry point"""
        return tuple(t.data_ptr() for t in (self.params_ptr, self.grads_ptr) + self.state_ptrs + (self.sizes, self.block_map)) + (self.n_blocks,)


class _MultiTensor:
    """What SGD and Adam share: the walk over the param groups (_groups) and what happens before any group is updated (_check_and_norm).

    Global gradient-norm clipping (torch.nn.utils.clip_grad_norm_, 2-norm) for the multi-tensor optimisers, on the device: the norm spans EVERY param
    group, is taken after the all-reduce (the optimiser is handed the averaged views) and after unscaling, and is summed in one fixed order
    (vs_grad_sqnorm_multi + vs_grad_clip_finish: no atomics), so every data-parallel rank derives the same coefficient from the same bits.  The update
    launches read the coefficient from the device record; nothing in the step reads it back.

    ``max_norm`` is an attribute of the optimiser (None = off), not a param-group key: set it between steps and the record follows (a captured launch
    reads it from device memory).  Switching between None and a number adds / removes launches — capture_key says so and train.GraphedStep re-captures."""

    max_norm = None
    _clip = None                         # device float[4] = {max_norm, norm, coef, 0}
    _clip_host = None                    # the max_norm the record holds
    _partials = None                     # device double[chunks of all groups]

    @staticmethod
    def _check_max_norm(max_norm):
        if max_norm is not None and not float(max_norm) > 0.0:
            raise ValueError("max_norm must be positive or None, got %r" % (max_norm,))
        return max_norm

    @property
    def grad_norm(self):
        """0-dim DEVICE view of the unclipped, unscaled global gradient norm of the last clipped step (reading it is the caller's synchronisation);
        None before the first one"""
        return None if self._clip is None else self._clip[1]

    def _clip_prepare(self, n_partials, device):
        """the record and the partial buffer, built OUTSIDE a capture (prepare() or the first eager step), the record holding the current max_norm"""
        capturing = torch.cuda.is_current_stream_capturing()
        if self._clip is None or self._clip.device != device:
            if capturing:
                raise RuntimeError("the clip record must exist before a capture: call prepare() first")
            self._clip_host = float(self.max_norm)
            self._clip = torch.tensor([self._clip_host, 0.0, 0.0, 0.0], dtype=torch.float32).to(device)
        if self._partials is None or self._partials.device != device or self._partials.numel() < n_partials:
            if capturing:
                raise RuntimeError("the gradient set grew since prepare(): the partial-norm buffer cannot be rebuilt inside a capture")
            self._partials = torch.zeros(n_partials, dtype=torch.float64, device=device)
        if not capturing:
            self._clip_sync()            # (a captured step is synchronised by sync_hyper() before its replay)

    def _clip_sync(self):
        """max_norm moved: one float in device memory (stream-ordered before whatever is launched next).  -> 1 if rewritten"""
        if self.max_norm is None or self._clip is None or self._clip_host == float(self.max_norm):
            return 0
        self._clip_host = float(self.max_norm)
        self._clip[:1].copy_(torch.tensor([self._clip_host], dtype=torch.float32), non_blocking=False)
        return 1

    def _clip_launch(self, todo, scaler):
        """-> the device address of the coefficient"""
        off = 0
        for g in todo:
            check(lib.vs_grad_sqnorm_multi(g.grads_ptr.data_ptr(), g.sizes.data_ptr(), g.block_map.data_ptr(), g.n_blocks,
                                           self._partials.data_ptr() + 8 * off, _stream()), "grad_sqnorm_multi")
            off += g.n_blocks
        check(lib.vs_grad_clip_finish(self._partials.data_ptr(), off, self._clip.data_ptr(), None if scaler is None else scaler.scale.data_ptr(),
                                      _stream()), "grad_clip_finish")
        return self._clip.data_ptr() + 8

    def _groups(self, override, state_bufs):
        """The param groups with work, as _Group records: the parameters named by override ({id(p): gradient}) or, without one, those with a p.grad
        (made contiguous); state_bufs(params) creates and returns the optimiser's state buffers, a tuple of lists; the device tables come from the
        group's _Tables.  With clipping on, the clip record and the partial buffer are made ready for all of them."""
        todo = []
        for gi, group in enumerate(self.param_groups):
            if override is not None:
                ps = [p for p in group["params"] if id(p) in override]
                grads = [override[id(p)] for p in ps]
            else:
                ps = [p for p in group["params"] if p.grad is not None]
                grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in ps]
            if not ps:
                continue
            (pp, gp, *sp, sizes, bm), nb = self._tables.setdefault(gi, _Tables()).get([ps, grads, *state_bufs(ps)], ps[0].device)
            todo.append(_Group(group, gi, ps, grads, pp, gp, tuple(sp), sizes, bm, nb, ps[0].device))
        if self.max_norm is not None and todo:
            self._clip_prepare(sum(g.n_blocks for g in todo), todo[0].device)
        return todo

    def _check_and_norm(self, todo, scaler):
        """Every group is checked, and the norm of ALL groups taken (unscaled), before any group is updated.
        -> the device addresses (clip coefficient, loss scale, overflow flag), None where there is none"""
        if scaler is not None:
            for g in todo:
                scaler.check(g.grads, g.index)
        coef = self._clip_launch(todo, scaler) if self.max_norm is not None and todo else None
        return (coef,) + ((scaler.scale.data_ptr(), scaler.found_inf.data_ptr()) if scaler is not None else (None, None))


class SGD(_MultiTensor, torch.optim.Optimizer):
    """torch.optim.SGD(lr, momentum, weight_decay, nesterov) — dampening 0 — as one kernel per group, with torch.nn.utils.clip_grad_norm_(max_norm)
    folded in (_MultiTensor: two more launches per step, the update reads the coefficient on the device).  Constructed without nesterov / max_norm it
    launches exactly the plain step (vs_sgd_momentum_*_multi)."""

    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0, nesterov=False, max_norm=None):
        if nesterov and not momentum > 0:
            raise ValueError("Nesterov momentum requires a momentum")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=bool(nesterov)))
        self.max_norm = self._check_max_norm(max_norm)
        self._tables = {}
        self._hyper = {}                 # group index -> [device float[4] = (lr, momentum, weight_decay, nesterov), the host values it holds]

    @torch.no_grad()
    def step_with(self, params, grads, scaler=None, device_hyper=False):
        """step() with explicit gradient tensors (e.g. the views of a DDP flat bucket) instead of p.grad.
        device_hyper: the launch reads lr / momentum / weight decay from device memory (sync_hyper) instead of taking them as kernel
        arguments — the form a captured HIP graph needs to follow a schedule without re-capture."""
        return self.step(_override={id(p): g for p, g in zip(params, grads)}, scaler=scaler, _device_hyper=device_hyper)

    @torch.no_grad()
    def prepare(self, params, grads, scaler=None):
        """Build the device-side pointer tables, the momentum buffers and the device-resident hyperparameters for step_with(params, grads)
        WITHOUT updating anything: a stream capture that includes the optimiser (train.GraphedStep, captured tail) must find them ready —
        building them copies host tables to the device, which a capture cannot contain."""
        return self.step(_override={id(p): g for p, g in zip(params, grads)}, scaler=scaler, _dry=True)

    def hyper(self):
        return [(float(g["lr"]), float(g["momentum"]), float(g["weight_decay"]), 1.0 if g.get("nesterov", False) else 0.0) for g in self.param_groups]

    def _ext(self):
        """does the step need vs_sgd_step_*_multi (a clip coefficient or Nesterov momentum somewhere) — or is it the plain step, launched as it always was"""
        return self.max_norm is not None or any(g.get("nesterov", False) for g in self.param_groups)

    @torch.no_grad()
    def sync_hyper(self):
        """Write each group's current (lr, momentum, weight_decay, nesterov) into its device-resident record, and max_norm into the clip record, if a
        scheduler moved them (stream-ordered before whatever is launched next: a graph replay that follows reads the new values).
        -> number of records rewritten."""
        moved = self._clip_sync()
        for gi, vals in enumerate(self.hyper()):
            ent = self._hyper.get(gi)
            if ent is not None and ent[1] != vals:
                ent[0].copy_(torch.tensor(vals, dtype=torch.float32), non_blocking=False)
                ent[1] = vals
                moved += 1
        return moved

    def _hyper_dev(self, gi, device):
        vals = self.hyper()[gi]
        ent = self._hyper.get(gi)
        if ent is None or ent[0].device != device:
            ent = self._hyper[gi] = [torch.tensor(vals, dtype=torch.float32).to(device), vals]
        return ent

    def capture_key(self, params):
        """what a captured step_with(params, ...) launch has baked in besides the gradient addresses: the parameter set, the momentum buffers, and WHICH
        launches the step is made of (clipping on or off, the plain or the extended update) — not the values of max_norm / nesterov, which are device-resident"""
        return tuple((id(p), p.data_ptr(), self.state[p]["momentum_buffer"].data_ptr() if "momentum_buffer" in self.state.get(p, {}) else 0)
                     for p in params) + ((self.max_norm is not None, self._ext()),)

    def _momentum_buffers(self, ps):
        for p in ps:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("vae_segmentation_amd.optim.SGD needs contiguous fp32 CUDA parameters")
        bufs = []
        for p in ps:
            st = self.state[p]
            if "momentum_buffer" not in st or st["momentum_buffer"] is None:
                st["momentum_buffer"] = torch.zeros_like(p)      # buf = 0*m + g on the first step = torch's clone(g)
            bufs.append(st["momentum_buffer"])
        return (bufs,)

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0, _override=None, scaler=None, _dry=False, _device_hyper=False):
        ops.flush_wgrads()
        todo = self._groups(_override, self._momentum_buffers)
        if _dry:
            for g in todo:
                self._hyper_dev(g.index, g.device)
                if scaler is not None:
                    scaler.prepare(g.grads, g.index)
            return None
        coef, sp, fp = self._check_and_norm(todo, scaler)
        ext = self._ext()
        for g in todo:
            group = g.group
            if _device_hyper:
                hyp = self._hyper_dev(g.index, g.device)[0]
                if ext:
                    check(lib.vs_sgd_step_dev_multi(*g.tables, hyp.data_ptr(), coef, sp, fp, _stream()), "sgd_step_dev_multi")
                else:
                    check(lib.vs_sgd_momentum_dev_multi(*g.tables, hyp.data_ptr(), sp, fp, _stream()), "sgd_momentum_dev_multi")
            elif ext:
                check(lib.vs_sgd_step_multi(*g.tables, float(group["lr"]) * float(grad_scale), float(group["momentum"]), float(group["weight_decay"]),
                                            1 if group.get("nesterov", False) else 0, coef, sp, fp, _stream()), "sgd_step_multi")
            else:
                check(lib.vs_sgd_momentum_scaled_multi(*g.tables, float(group["lr"]) * float(grad_scale), float(group["momentum"]),
                                                       float(group["weight_decay"]), 0, sp, fp, _stream()), "sgd_momentum_multi")
        if scaler is not None:
            scaler.update()
        ops.weights_changed()
        return None


class Adam(_MultiTensor, torch.optim.Optimizer):
    """torch.optim.Adam(lr, betas, eps, weight_decay) as one kernel per group; ``max_norm``: torch.nn.utils.clip_grad_norm_ folded in (_MultiTensor).
    Deviation under a LossScaler (fp16 only; the reference has no mixed precision): when the device-side overflow flag skips an update the
    host-side ``state['step']`` has still advanced (reading the flag would sync), so after a skipped step the bias corrections run one step
    ahead of torch.cuda.amp.GradScaler's."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.max_norm = self._check_max_norm(max_norm)
        self._tables = {}

    @torch.no_grad()
    def step_with(self, params, grads, scaler=None):
        return self.step(_override={id(p): g for p, g in zip(params, grads)}, scaler=scaler)

    def _moments(self, ps):
        m1, m2 = [], []
        for p in ps:
            st = self.state[p]
            if "exp_avg" not in st:
                st["step"] = 0
                st["exp_avg"] = torch.zeros_like(p)
                st["exp_avg_sq"] = torch.zeros_like(p)
            st["step"] = int(st["step"]) + 1
            m1.append(st["exp_avg"])
            m2.append(st["exp_avg_sq"])
        return m1, m2

    @torch.no_grad()
    def step(self, closure=None, _override=None, scaler=None):
        ops.flush_wgrads()
        todo = self._groups(_override, self._moments)
        coef, sp, fp = self._check_and_norm(todo, scaler)
        for g in todo:
            group, (b1, b2), step = g.group, g.group["betas"], int(self.state[g.params[0]]["step"])
            if coef is not None:
                check(lib.vs_adam_clip_multi(*g.tables, float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                             float(group["weight_decay"]), step, coef, sp, fp, _stream()), "adam_clip_multi")
            else:
                check(lib.vs_adam_scaled_multi(*g.tables, float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                               float(group["weight_decay"]), step, sp, fp, _stream()), "adam_multi")
        if scaler is not None:
            scaler.update()
        ops.weights_changed()
        return None


_EMA_TABLES = {}


@torch.no_grad()
def ema_update(teacher, student, alpha):
    """teacher <- alpha*teacher + (1-alpha)*student over matching state_dict entries (main_target.py:512-516)."""
    sd_t, sd_s = teacher.state_dict(), student.state_dict()
    ts = [sd_t[k] for k in sd_s if sd_s[k].dtype == torch.float32]
    ss = [sd_s[k] for k in sd_s if sd_s[k].dtype == torch.float32]
    tab = _EMA_TABLES.setdefault((id(teacher), id(student)), _Tables())
    (tp, sp, sizes, bm), nb = tab.get([ts, ss], ts[0].device)
    check(lib.vs_ema_multi(tp.data_ptr(), sp.data_ptr(), sizes.data_ptr(), bm.data_ptr(), nb, float(alpha), _stream()), "ema_multi")
    ops.clear_pack_cache()      # the teacher's cached packed weights are stale now ...
    ops.refresh_frozen_packs(teacher)   # ... and are re-packed in place at once: captured graphs that replay the teacher hold these addresses
