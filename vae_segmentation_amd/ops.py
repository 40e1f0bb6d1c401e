"""torch.autograd.Function wrappers around the libvaeseg C ABI (include/vaeseg.h).

PyTorch supplies device memory, streams and the autograd graph; every byte of arithmetic on the hot path
is done by the HIP kernels.  Nothing here has a CPU path: tensors must live on the GPU.

Internal activations are channels-last ``(N, D, H, W, C)`` tensors in the kernel dtype (fp32 or bf16).
A *lazy* activation is the pair ``(raw, stats)``: ``raw`` is a conv output before InstanceNorm+ReLU and
``stats`` the fp64 ``(N, C, 2)`` (sum, sumsq) its producer accumulated; consumers normalise on load.
For autograd, ``stats`` is a non-differentiable side output and the gradient attached to ``raw`` is the
total derivative (the InstanceNorm+ReLU backward is applied by the consumer's backward).
"""
import ctypes as _ctypes
import numbers as _numbers
import os
import weakref as _weakref

import torch

from . import _lib
from ._lib import (VS_BF16, VS_CONV_K2S2, VS_CONV_K3, VS_CONV_UP, VS_F16, VS_F32, VS_PACK_ROWS_D0, VS_PACK_ROWS_D1_FLIP,
                   VS_PACK_SCATTER_D1, check, lib)

_DT_TORCH = {VS_F32: torch.float32, VS_BF16: torch.bfloat16, VS_F16: torch.float16}
_DT_VS = {v: k for k, v in _DT_TORCH.items()}
KERNEL_DTYPES = tuple(_DT_VS)
# PACK-ONLY dtype (include/vaeseg.h VS_F32X3): the three-bf16-limb image of an fp32 3x3x3 weight that the parity mode's limb kernels read
# (csrc/igemm_k3x.h; vs_conv_k3_f32_limbs).  Tensors stay float32; only pack_weight / pack_weight_cached accept the marker.
VS_F32X3 = 3
F32X3 = "f32x3"
_DT_TORCH[VS_F32X3] = F32X3
_DT_VS[F32X3] = VS_F32X3
_F32_LIMBS = bool(lib.vs_conv_k3_f32_limbs(96, 96, 96, 8))


def k3_pack_dtype(x):
    """the image format of a 3x3x3 weight applied to the channels-last tensor x: the limb image in the fp32 parity mode where the library runs
    that launch on the bf16 matrix cores (vs_conv_k3_f32_limbs: not the volumes up to 6^3 of the deep levels), the storage type itself otherwise"""
    if x.dtype == torch.float32 and lib.vs_conv_k3_f32_limbs(x.shape[1], x.shape[2], x.shape[3], x.shape[4]):
        return F32X3
    return x.dtype


def vs_of(dtype):
    """torch dtype -> VS_* enum of include/vaeseg.h"""
    try:
        return _DT_VS[dtype]
    except KeyError:
        raise TypeError("kernel dtype must be float32, bfloat16 or float16, got %s" % (dtype,)) from None

EPS_IN = 1e-5       # nn.InstanceNorm3d default eps (joint_model.py:11)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# Optional per-launch timing (bench.py roofline leg): when a list is installed here, every C-ABI launch below is
# bracketed by HIP events recorded on the stream the kernel is launched on; entries are
# (kernel id, algorithmic bytes, algorithmic flops, start event, end event).
PROFILE = None


def _esize(t):
    return 4 if t.dtype == torch.float32 else 2


class VsConfig(_ctypes.Structure):
    """vs_config (include/vaeseg.h): the library's tuning switches"""
    _fields_ = [(n, _ctypes.c_int) for n in ("k3_small", "k3_tall", "k3_wgs_per_cu", "k3t_wgs_per_cu", "k3f_min_wgs", "mt_min_wgs", "f32_limbs", "g1_limbs", "k3x_ck",
                                            "k3x_toeplitz", "fuse_wgrad", "epilogue_apply", "chain", "k2s2_stream", "k2s8_wgs_per_cu", "up_wgs_per_cu", "up_rb",
                                            "wgrad_uber", "wgrad_mpack", "wgrad_swap", "wgrad_big", "wgrad_xcd", "k3_short_tiles", "wgrad_bias_fold", "hist_form")] + \
               [(n, _ctypes.c_longlong) for n in ("wgrad_wgs", "wgrad_f32_tiles", "wgrad_group_wgs", "wgrad_big_min_voxels")]


def get_config():
    """-> dict of the active library's tuning switches (vs_get_config)"""
    if lib.vs_config_bytes() != _ctypes.sizeof(VsConfig):
        raise _lib.VaesegError("vs_config layout mismatch: the library's struct has %d bytes, this binding %d" % (lib.vs_config_bytes(), _ctypes.sizeof(VsConfig)))
    c = VsConfig()
    check(lib.vs_get_config(_ctypes.addressof(c)), "get_config")
    return {n: getattr(c, n) for n, _ in VsConfig._fields_ if n != "reserved_"}


def set_config(**kw):
    """Change tuning switches of the library (vs_set_config, the single writer; every loaded build gets the same values).  Call between launches.
    -> the previous values of the switches that were changed (hand them back to set_config to restore)."""
    cur = get_config()
    unknown = [k for k in kw if k not in cur]
    if unknown:
        raise KeyError("not a vs_config field: %s" % ", ".join(unknown))
    old = {k: cur[k] for k in kw}
    cur.update(kw)
    c = VsConfig(**cur)
    for l in lib.loaded():
        check(l.vs_set_config(_ctypes.addressof(c)), "set_config")
    return old


class config:
    """with ops.config(wgrad_mpack=0): ...  — tuning switches changed for a block (tests, A/B runs), restored on the way out"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = set_config(**self.kw)
        return self

    def __exit__(self, *exc):
        set_config(**self.old)
        return False


def _pick_mt(rows16, tiles):
    """mirror of pick_mt() in csrc/conv_api.hip (kernel instantiation naming only)."""
    min_wgs = get_config()["mt_min_wgs"]
    for mt in (64, 32, 16):
        if rows16 % mt:
            continue
        if tiles * (rows16 // mt) >= min_wgs or mt == 16:
            return mt
    return 16


def _k3_kid(tname, ck, mt, sums=False, geom=None, m=None, lazy=False):
    """kernel instantiation name of a 3x3x3 launch (mirrors g1_dispatch_k3_* / k3b_use_tall in csrc; rocprof prints the same
    string).  geom = (n, d, h, w) of the convolution's grid, m = stored output channels.  The 16-bit kernels carry their storage
    type as the LAST template argument."""
    if tname == "float":
        return "k3_kernel<float,%d,%d,0>" % (ck, mt)
    hs = "true" if (lazy and not sums) else "false"
    if ck == 8 and m == 8:
        return "k3t_kernel<0,%s,8,%s,%s>" % ("true" if sums else "false", hs, tname)
    cfg = get_config()
    if ck == 32 and geom is not None and (geom[1] + 2) * (geom[2] + 2) * (geom[3] + 2) <= 512 and cfg["k3_small"] != 0:
        tv = (geom[1] + 2) * (geom[2] + 2) * (geom[3] + 2)
        return "k3s_kernel<%s,%d,%s,%s>" % ("true" if sums else "false", 128 if tv <= 128 else 512, hs, tname)
    yt = 4
    if geom is not None and ck == 32 and mt == 16 and m is not None and cfg["k3_short_tiles"]:      # csrc/igemm_k3_h16.inc: short tiles for the under-filled launches
        n, d, h, w = geom
        rt = (m + 15) // 16
        zx = n * ((d + 3) // 4) * ((w + 15) // 16)
        if zx * ((h + 3) // 4) * rt <= 128 and zx * ((h + 1) // 2) * rt <= 256:
            yt = 1 if (cfg["k3_short_tiles"] >= 2 and zx * ((h + 1) // 2) * rt <= 128 and zx * h * rt <= 256) else 2
    if geom is not None and ck < 32 and mt == 16 and cfg["k3_tall"] != 0:
        n, d, h, w = geom
        tiles = n * ((d + 3) // 4) * ((h + 3) // 4) * ((w + 15) // 16)
        tall = n * ((d + 3) // 4) * ((h + 7) // 8) * ((w + 15) // 16)
        if cfg["k3_tall"] == 1 or (tall >= 256 and tiles <= 2048):
            yt = 8
    return "k3b_kernel<%d,%d,0,%s,%d,%s,%s>" % (ck, min(mt, 32), "true" if sums else "false", yt, hs, tname)


PROFILE_PRIME_US = 80
PROFILE_SPIN = [None]          # set by profiling.py (the measurement aid lives in tools/probe/libvsprobe.so, not in the product library)


class _timed:
    def __init__(self, kid, nbytes, flops, detail=""):
        self.rec = None if PROFILE is None else [kid, float(nbytes), float(flops), detail]

    def __enter__(self):
        if self.rec is not None:
            if PROFILE_PRIME_US:
                # keep the queue busy while the bracket is enqueued (tools/probe: vs_spin): the two event packets and
                # the kernel then run back to back, as the kernel does inside the replayed graph
                PROFILE_SPIN[0](PROFILE_PRIME_US, _stream())
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.rec.append(e)

    def __exit__(self, *exc):
        if self.rec is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.rec.append(e)
            PROFILE.append(tuple(self.rec))
        return False


def _p(t):
    return None if t is None else t.data_ptr()


def _tname(t):
    """the storage type as it appears in the profiler's kernel names"""
    return {torch.float32: "float", torch.bfloat16: "unsigned short", torch.float16: "_Float16"}[t.dtype]


def vs_dtype(t):
    return vs_of(t.dtype)


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("vae_segmentation_amd runs on the GPU only (libvaeseg HIP kernels); "
                               "got a CPU tensor — there is no CPU fallback")


def cpad(c):
    if c <= 8:
        return 8
    if c <= 16:
        return 16
    return (c + 31) // 32 * 32


# ------------------------------------------------------------------------------------------------
# weight packing (fragment order); frozen weights are packed once and cached
# ------------------------------------------------------------------------------------------------


def pack_weight(w, form, c_pad, dtype, out=None):
    """w: (d0, d1, k, k, k) fp32 parameter -> uint8 buffer holding the MFMA-fragment image (written into `out` when given)."""
    _require_cuda(w)
    w = w.detach()
    if not w.is_contiguous():
        w = w.contiguous()
    d0, d1 = w.shape[0], w.shape[1]
    ntaps = w[0, 0].numel()
    dt = vs_of(dtype)
    if form == VS_PACK_ROWS_D0:
        rows, gemm_taps = d0, ntaps
    elif form == VS_PACK_ROWS_D1_FLIP:
        rows, gemm_taps = d1, ntaps
    else:
        rows, gemm_taps = ntaps * d1, 1
    nbytes = lib.vs_packed_weight_bytes(rows, c_pad, gemm_taps, dt)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=w.device) if out is None else out
    if buf.numel() != nbytes:
        raise ValueError("pack_weight: out buffer holds %d bytes, image needs %d" % (buf.numel(), nbytes))
    check(lib.vs_pack_weight(w.data_ptr(), buf.data_ptr(), d0, d1, ntaps, c_pad, form, dt, _stream()), "pack_weight")
    return buf


def pack_weight_cached(param, form, c_pad, dtype):
    """Packed image of a conv weight.
    Frozen parameters: packed once per (tensor object, version, epoch); the cache lives on the tensor itself, so it dies
    with it and a recycled device address can never alias another weight.
    Trainable parameters: the first use registers (param, form, c_pad, dtype) in a repack plan and packs it; afterwards
    `repack_trainable()` — called by the native optimisers right after their update kernel — refreshes EVERY registered
    image in one multi-tensor launch, so a training step issues no per-layer pack launches.  An image is trusted only if
    it was packed at the parameter's current (version, epoch); otherwise it is re-packed on the spot."""
    dt = vs_of(dtype)
    key = (form, c_pad, dt)
    if not param.is_leaf:
        # a weight computed from a parameter in this very pass (GSConv3d's |w| / sum, the 1x1x1 conv embedded in a 3x3x3 one): a
        # temporary — packed on the spot, never registered anywhere
        return pack_weight(param, form, c_pad, dtype)
    if param.requires_grad:
        plan = getattr(param, "_vs_pack_plan", None)
        if plan is None:
            plan = {}
            param._vs_pack_plan = plan
        ent = plan.get(key)
        stamp = (param._version, param.data_ptr(), _TRAIN_EPOCH[0])
        if ent is None:
            buf = pack_weight(param, form, c_pad, dtype)
            plan[key] = [buf, stamp]
            _REPACK["params"][id(param)] = param
            _REPACK["dirty"] = True
            return buf
        if ent[1] != stamp:
            pack_weight(param, form, c_pad, dtype, out=ent[0])
            ent[1] = stamp
        return ent[0]
    cache = _frozen_cache(param)
    stamp = (param._version, param.data_ptr(), _PACK_EPOCH[0])
    ent = cache.get(key)
    if ent is None:
        cache[key] = [pack_weight(param, form, c_pad, dtype), stamp]
        return cache[key][0]
    if ent[1] != stamp:
        # re-pack INTO the existing buffer: a captured HIP graph holds this address (GraphedStep / TestTimeFinetune replay the
        # frozen VAE / teacher with pointer arguments only), so an invalidated image must be refreshed in place, never re-allocated
        pack_weight(param, form, c_pad, dtype, out=ent[0])
        ent[1] = stamp
    return ent[0]


def _frozen_cache(param):
    """{key: [buffer, stamp]} living on the tensor object itself: it dies with the tensor, so a recycled device address can
    never alias another weight; buffers are never replaced once handed out (see pack_weight_cached)."""
    cache = getattr(param, "_vs_pack_cache", None)
    if cache is None:
        cache = {}
        param._vs_pack_cache = cache
    return cache


def refresh_frozen_packs(module):
    """Re-pack, in place and now, every cached image of `module`'s frozen weights (call after writing them through raw
    pointers — optim.ema_update, load_state_dict on a network a captured graph replays): graph replays that follow read the
    new weights without an eager forward in between."""
    for prm in module.parameters():
        for dt, plan in (getattr(prm, "_vs_up_plan", None) or {}).items():       # composed Up images cached on the 3x3x3 weight (up_plan)
            wt, bt = plan["src"]
            with torch.no_grad():
                _up_compose_into(plan, wt.detach(), None if bt is None else bt.detach(), prm.detach(), dt)
                plan["stamp"] = _up_stamp(wt, bt, prm)
        cache = getattr(prm, "_vs_pack_cache", None)
        if not cache:
            continue
        stamp = (prm._version, prm.data_ptr(), _PACK_EPOCH[0])
        for key, ent in cache.items():
            if key[0] == "lin":
                ent[0].copy_(_linear_layout(prm, key[1], key[2], key[3]))
            else:
                form, c_pad, dt = key
                pack_weight(prm, form, c_pad, _DT_TORCH[dt], out=ent[0])
            ent[1] = stamp


_TRAIN_EPOCH = [0]
_REPACK = {"params": {}, "dirty": True, "descs": None, "blocks": 0, "n": 0, "entries": []}


def repack_trainable():
    """Re-pack every registered trainable weight image with ONE launch (call after the weights changed in place)."""
    import struct
    r = _REPACK
    _recompose_trainable_ups()
    live = [p for p in r["params"].values() if getattr(p, "_vs_pack_plan", None)]
    if not live:
        return
    if r["dirty"]:
        recs, entries, blocks = [], [], 0
        for p in live:
            d0, d1 = p.shape[0], p.shape[1]
            ntaps = p[0, 0].numel()
            for (form, c_pad, dt), ent in p._vs_pack_plan.items():
                total = ent[0].numel() // (4 if dt == VS_F32 else 2)
                recs.append(struct.pack("<QQiiiiiiiiq", p.data_ptr(), ent[0].data_ptr(), d0, d1, ntaps, c_pad, form, dt, blocks, 0, total))
                entries.append((p, ent))
                blocks += (total // (4 if dt == VS_F32 else 8) + 255) // 256        # 256-thread blocks of 16-byte fragments
        raw = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8)
        r["descs"] = raw.to(live[0].device)
        r["blocks"], r["n"], r["entries"], r["dirty"] = blocks, len(recs), entries, False
    check(lib.vs_pack_weight_multi(r["descs"].data_ptr(), r["n"], r["blocks"], _stream()), "pack_weight_multi")
    for p, ent in r["entries"]:
        ent[1] = (p._version, p.data_ptr(), _TRAIN_EPOCH[0])


def repack_table():
    """The descriptor table repack_trainable() launches with right now (a device tensor, or None).  A captured graph that contains the
    re-pack launch holds a reference to it: repack_trainable() REPLACES the table when other images register, it never rewrites one in place."""
    return _REPACK["descs"]


_PACK_EPOCH = [0]


def clear_pack_cache():
    """Invalidate every cached packed weight (call after writing frozen weights through raw pointers, e.g. EMA)."""
    _PACK_EPOCH[0] += 1


def frozen_linear_layout(param, kind, c, v):
    """Frozen fc weights re-laid ONCE for contiguous access (cached on the tensor like the packed conv images; trainable weights keep the
    reference layout and the permuting kernels).  The reference flattens NCDHW (k = c*V + v) while activations are channels-last
    (ph = v*C + c), so read in k order the activation is a 2-byte gather and fc2's backward walks a weight column with a 512-byte stride.
      "cols_cl"  : (J, K) -> the K columns in channels-last order          (fc_mean / fc_std forward, backward w.r.t. x)
      "rows_cl_t": (J, K) -> (K, J) transposed, the J rows in channels-last order   (fc2 backward w.r.t. z)"""
    key = ("lin", kind, c, v)
    cache = _frozen_cache(param)
    stamp = (param._version, param.data_ptr(), _PACK_EPOCH[0])
    ent = cache.get(key)
    if ent is None:
        cache[key] = [_linear_layout(param, kind, c, v), stamp]
        return cache[key][0]
    if ent[1] != stamp:
        ent[0].copy_(_linear_layout(param, kind, c, v))         # in place: see pack_weight_cached
        ent[1] = stamp
    return ent[0]


def _linear_layout(param, kind, c, v):
    w = param.detach()
    with torch.no_grad():
        if kind == "cols_cl":
            return w.view(w.shape[0], c, v).permute(0, 2, 1).contiguous().view(w.shape[0], c * v)
        return w.view(c, v, w.shape[1]).permute(2, 1, 0).contiguous().view(w.shape[1], c * v)


def weights_changed():
    """Called by the native optimisers after they updated parameters through raw pointers (torch's version counters do
    not see that): start a new epoch and refresh all registered trainable images in one launch."""
    _TRAIN_EPOCH[0] += 1
    repack_trainable()


# ------------------------------------------------------------------------------------------------
# raw launch helpers (no autograd)
# ------------------------------------------------------------------------------------------------
# The fp64 (sum, sumsq) buffers must be zero before their producer's atomics; allocating each with torch.zeros costs
# one ~4 us fill launch per layer (~170 per step).  Instead the top-level modules open an arena per forward: ONE zeroed
# fp64 buffer sized from the previous step's use, from which the per-layer buffers are carved as views (the views keep
# the arena's storage alive for backward; a new forward gets a new arena, so nothing is ever re-zeroed under a reader).
_ARENA = {"buf": None, "off": 0, "used": 0, "need": 1 << 17, "depth": 0}


def stats_arena_begin(device):
    """Start a new zeroed arena (call at the top of a forward pass; backward keeps carving from the same one).  Inside an
    arena_scope (Joint.forward: Segmentation then VAE) the inner forwards share the scope's arena: one zero-fill launch per step."""
    drop_stale_wgrads()
    a = _ARENA
    if a["depth"] > 0 and a["buf"] is not None and a["buf"].device == torch.device(device):
        return
    a["need"] = max(a["need"], a["used"])
    n = (a["need"] + (a["need"] >> 2) + 1) // 2 * 2                  # doubles, a multiple of 16 bytes
    a["buf"] = torch.empty(n, dtype=torch.float64, device=device)
    check(lib.vs_zero_fill(a["buf"].data_ptr(), n * 8, _stream()), "zero_fill")
    a["off"] = 0
    a["used"] = 0


class arena_scope:
    """with arena_scope(device): every forward inside shares one statistics arena (one zero fill)."""

    def __init__(self, device):
        self.device = device

    def __enter__(self):
        if _ARENA["depth"] == 0:
            stats_arena_begin(self.device)
        _ARENA["depth"] += 1

    def __exit__(self, *exc):
        _ARENA["depth"] -= 1
        return False


STAT_SLOTS = lib.vs_stat_slots()      # VS_STAT_SLOTS of the loaded library: partial copies of every statistics buffer; consumers add them


def _new_stats(n, c, device, width=2):
    """A zeroed statistics buffer double[STAT_SLOTS][n][c][2] (width 2), carved from the arena; width 1 = plain zeroed scratch [1][n][c][1]."""
    a = _ARENA
    slots = STAT_SLOTS if width == 2 else 1
    cnt = slots * n * c * width
    a["used"] += cnt
    buf = a["buf"]
    if buf is None or buf.device != device or a["off"] + cnt > buf.numel():
        a["fallbacks"] = a.get("fallbacks", 0) + 1
        return torch.zeros(slots, n, c, width, dtype=torch.float64, device=device)
    out = buf[a["off"]:a["off"] + cnt].view(slots, n, c, width)
    a["off"] += cnt
    return out


def set_deterministic(on=True):
    """Switch the package to the deterministic build of the library (libvaeseg_det.so, include/vaeseg.h vs_get_deterministic): every
    per-(n,c) statistic is accumulated with commuting integer atomics, so two runs on the same inputs agree bit for bit.  Parity runs use it
    (tests/conftest.py, env VS_DETERMINISTIC=1); the throughput default is the fp64-atomic build.  A statistics buffer must be produced and
    consumed by one build: switch between passes only (captured HIP graphs keep the kernels of the build they were captured under)."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    lib.use_deterministic(bool(on))


def is_deterministic():
    return bool(lib.vs_get_deterministic()) if hasattr(lib, "vs_get_deterministic") else False


def stats_total(stats):
    """(n, c, 2) totals of a statistics buffer (sum over its partial copies / its fixed-point limbs) — for tests / inspection"""
    if lib.vs_stat_interleaved():
        s, n, c, w = stats.shape
        stats = stats.reshape(n, c, s, w).permute(2, 0, 1, 3)
    if is_deterministic():
        limbs = stats.contiguous().view(torch.int64).double()
        return (limbs[0] * 2.0 ** 40 + limbs[1]) + (limbs[2] * 2.0 ** -40 + limbs[3] * 2.0 ** -80)
    return stats.sum(0)


def conv_gather(x, xs, wp, bias, m_out, kind, want_stats, real_channels=None):
    n, d, h, w, c = x.shape
    if kind == VS_CONV_K2S2:
        out_shape = (n, d // 2, h // 2, w // 2, m_out)
    else:
        out_shape = (n, d, h, w, m_out)
    y = torch.empty(out_shape, dtype=x.dtype, device=x.device)
    ys = _new_stats(n, m_out, x.device) if want_stats else None
    kid = nb = fl = None
    if PROFILE is not None:
        ck, taps = min(c, 32), (27 if kind == VS_CONV_K3 else 8)
        if kind == VS_CONV_K3:
            tiles = n * ((d + 3) // 4) * ((h + 3) // 4) * ((w + 15) // 16)
        else:
            tiles = n * ((y.numel() // (n * m_out) + 255) // 256)
        rows16 = (m_out + 15) // 16 * 16
        tname = _tname(x)
        if kind == VS_CONV_K3:
            kid = _k3_kid(tname, ck, _pick_mt(rows16, tiles), geom=(n, d, h, w), m=m_out, lazy=xs is not None)
        else:
            kid = "g1_kernel<%s,%d,%d,%d,0>" % (tname, ck, kind, _pick_mt(rows16, tiles))
        cr = real_channels[0] if real_channels else c
        mr = real_channels[1] if real_channels else m_out
        vox_out = y.numel() // m_out
        nb = (x.numel() // c * cr + vox_out * mr) * _esize(x) + cr * mr * taps * _esize(x)
        fl = 2.0 * vox_out * taps * cr * mr
    with _timed(kid, nb, fl, "x%s->m%d" % (tuple(x.shape), m_out)):
        check(lib.vs_conv_gather_fwd(x.data_ptr(), _p(xs), wp.data_ptr(), _p(bias), y.data_ptr(), _p(ys), n, d, h, w, c,
                                     m_out, kind, vs_dtype(x), EPS_IN, _stream()), "conv_gather_fwd")
    return y, ys


def conv_scatter(x, xs, wp, bias, m_out):
    n, d, h, w, c = x.shape
    y = torch.empty((n, 2 * d, 2 * h, 2 * w, m_out), dtype=x.dtype, device=x.device)
    kid = nb = fl = None
    if PROFILE is not None:
        tiles = n * ((d * h * w + 255) // 256)
        rows16 = (8 * m_out + 15) // 16 * 16
        kid = "g1_kernel<%s,%d,2,%d,2>" % (_tname(x), min(c, 32), _pick_mt(rows16, tiles))
        nb = (x.numel() + y.numel()) * _esize(x) + 8 * c * m_out * _esize(x)
        fl = 2.0 * (x.numel() // c) * 8 * c * m_out
    with _timed(kid, nb, fl, "x%s->m%d" % (tuple(x.shape), m_out)):
        check(lib.vs_conv_scatter_fwd(x.data_ptr(), _p(xs), wp.data_ptr(), _p(bias), y.data_ptr(), n, d, h, w, c, m_out,
                                      vs_dtype(x), EPS_IN, _stream()), "conv_scatter_fwd")
    return y


# An activation that feeds both the next encoder level (a lazy conv) and an additive U-Net skip (joint_model.py:380,382) receives two
# gradients.  The skip's (Materialize.backward, which runs first: the decoder is differentiated before the encoder) is parked here, keyed
# by the raw tensor, and summed in by the apply pass of the conv's backward (vs_instnorm_relu_bwd_apply_add) instead of by an ATen add
# launch of autograd's.  A gradient nobody collected by the end of the pass is an error (it would be lost), checked by an engine callback.
_PENDING = {"grads": {}, "callback": False}


def _park_gradient(x, g):
    _PENDING["grads"][(x.data_ptr(), tuple(x.shape))] = g
    if not _PENDING["callback"]:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(_pending_done)
            _PENDING["callback"] = True
        except RuntimeError:
            pass


def _collect_gradient(x):
    return _PENDING["grads"].pop((x.data_ptr(), tuple(x.shape)), None)


def _pending_done():
    _PENDING["callback"] = False
    left = len(_PENDING["grads"])
    _PENDING["grads"].clear()
    if left:
        raise RuntimeError("%d parked skip gradient(s) were never collected by the conv that shares their input: gradients lost" % left)


# Deferred IN-backward apply (the 8-channel full-resolution layers, igemm_k3t.h FA): where a lazy activation x is produced by an 8 -> 8 3x3x3
# conv and consumed by exactly one 3x3x3 conv (the modules mark x: mark_defer_apply), the consumer's backward hands over the UN-applied
# gradient g = dL/da together with (x, stats, sums) through this registry, and the producer's backward-data kernel applies
# rstd * (g*mask - m1 - xhat*m2) while it stages its input — the standalone apply launch (3 tensor passes at 96^3) disappears.
# An entry nobody took by the end of the pass means a consumer treated an un-applied gradient as applied: that is an error, not a fallback.
FUSE_APPLY = os.environ.get("VS_FUSE_APPLY", "1") != "0"
EPILOGUE_APPLY = os.environ.get("VS_EPILOGUE_APPLY", "1") != "0"      # A/B switch of k3b_kernel<..., EA> (the library reads the same variable)
EPILOGUE_APPLY_S2 = os.environ.get("VS_EPILOGUE_APPLY_S2", "1") != "0"      # ... of g1_kernel's epilogue apply alone (the stride-2 / transposed backward-data launches)
# channels of the activations whose producer has a fused-apply kernel: 8 / 16 (k3t, single-chunk k3b: the 96^3 / 48^3 levels).  The 32-channel
# form (k3b<32,...,FA>, the 24^3 / 12^3 levels) measured slower twice (round 4: 2.519 -> 2.566 ms per step, profiles/r04_ab_fused_apply_32ch.json)
# and left the library in round 5; so did 16-channel half stages of the same layers (two waves per SIMD, 19 launches fewer, +30..+43 us per step:
# profiles/r05_ab_fused_apply_half_stages.json).  The library has the last word (vs_conv_k3_fused_apply_supported).
_FA_CHANNELS = (8, 16)
_FA_CHANNELS_F32 = (8, 16)       # 16: k3x_kernel<8, 16, .., FA> (the 16 -> 16 layers of the 48^3 level; the library has the last word)
FUSE_APPLY_F32 = os.environ.get("VS_FUSE_APPLY_F32", "1") != "0"      # A/B switch of the parity mode's fused apply
_LAZY_APPLY = {"grads": {}, "callback": False}


def mark_defer_apply(x, producer):
    """x: the raw output of `producer` (an nn.Conv3d holder run by ConvK3, 3x3x3) about to be consumed, exactly once, by a conv op that honours
    the mark (ConvK3, ConvK3Softmax[CL], ConvK2S2, ConvT2S2).  Marked when the producer's backward-data launch has a fused-apply kernel
    (vs_conv_k3_fused_apply_supported: the single-chunk layers of the full- and half-resolution levels)."""
    # fp32 parity mode: the 8-channel full-resolution layers only (k3xt_kernel<..., FA>, csrc/igemm_k3x.h; round 5)
    chans = _FA_CHANNELS if x.dtype != torch.float32 else (_FA_CHANNELS_F32 if FUSE_APPLY_F32 else ())
    if FUSE_APPLY and x.shape[-1] in chans and tuple(producer.weight.shape[2:]) == (3, 3, 3):
        x._vs_defer_apply = True
    return x


def _fa_supported(gy, x, lazy_input):
    n, d, h, w, c = gy.shape
    return bool(lib.vs_conv_k3_fused_apply_supported(n, d, h, w, c, x.shape[-1], 1 if lazy_input else 0, vs_dtype(gy)))


def _defer_register(g, x, xs, sums):
    # g itself is kept in the entry: the key is its address, and a live reference is what guarantees that address cannot be recycled for another
    # gradient of the same shape before the producing conv's backward takes the entry
    _LAZY_APPLY["grads"][(g.data_ptr(), tuple(g.shape))] = (x, xs, sums, g)
    if not _LAZY_APPLY["callback"]:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(_lazy_apply_done)
            _LAZY_APPLY["callback"] = True
        except RuntimeError:
            pass


def _take_lazy(g):
    ent = _LAZY_APPLY["grads"].pop((g.data_ptr(), tuple(g.shape)), None) if _LAZY_APPLY["grads"] else None
    return None if ent is None else ent[:3]


def _lazy_apply_done():
    _LAZY_APPLY["callback"] = False
    left = len(_LAZY_APPLY["grads"])
    _LAZY_APPLY["grads"].clear()
    if left:
        raise RuntimeError("%d un-applied gradient(s) (deferred InstanceNorm-backward apply) were not taken by the producing conv: gradients wrong" % left)


def apply_lazy(g, lazy):
    """the standalone apply of a deferred gradient (a producer that cannot fuse it)"""
    x, xs, sums = lazy
    n, c = x.shape[0], x.shape[-1]
    check(lib.vs_instnorm_relu_bwd_apply(g.data_ptr(), x.data_ptr(), xs.data_ptr(), sums.data_ptr(), g.data_ptr(), n, x.numel() // (n * c), c,
                                         vs_dtype(x), EPS_IN, _stream()), "instnorm_relu_bwd_apply")
    return g


def _ea_sync(n, device):
    """the arrival counters of one epilogue-apply launch: 8 shards of 128 bytes per sample, 128-byte aligned, zeroed with the statistics arena"""
    cnt = 128 * n
    buf = _new_stats(1, cnt + 16, device, width=1).view(-1)
    off = ((-buf.data_ptr()) % 128) // 8
    return buf[off:off + cnt]


def conv_bwd_data_lazy(gy, wpb, x, xs, kind, scatter=False, real_channels=None, defer=False, lazy=None, want_dx=False, fuse_wgrad=None):
    """Gradient w.r.t. the raw tensor x of a lazy activation a = relu(instnorm(x)) that fed a conv:
    g = conv-backward-data(gy) with the InstanceNorm+ReLU-backward sums accumulated in the same kernel's epilogue,
    then the (in-place) apply pass.  kind / scatter select the backward-data form of the forward conv.
    lazy = (act_x, act_stats, act_sums): gy itself is an un-applied gradient (see _LAZY_APPLY) — its apply is fused into this launch's
    staging and the call returns (g, applied gy or None [want_dx]).  defer: leave g un-applied and register it for x's producer.
    fuse_wgrad = (weight, m_real, c_real): the launch also forms the layer's weight gradient (see _wgrad_fusable) and the call returns (g, gw)."""
    n, c = x.shape[0], x.shape[-1]
    sums = _new_stats(n, c, x.device)
    g = torch.empty_like(x)
    gn, gd, gh, gw, gc = gy.shape
    dt = vs_dtype(x)
    if fuse_wgrad is not None:
        weight, m_real, c_real = fuse_wgrad
        ax, axs, asums = lazy if lazy is not None else (None, None, None)
        nslabs = lib.vs_conv_k3_bwd_data_wgrad_slabs(gn, gd, gh, gw)
        slabs = torch.empty(nslabs * 1728, dtype=torch.float32, device=x.device)
        kid = nb = fl = None
        if PROFILE is not None:
            kid = "k3tw_kernel<%s,%s>" % (_tname(x), "true" if lazy is not None else "false")
            nb = ((3 if lazy is not None else 2) * gy.numel() + 2 * g.numel()) * _esize(x)
            fl = 2.0 * 2.0 * (g.numel() // c) * 27 * gc * c
        with _timed(kid, nb, fl, "bwd+wgrad gy%s->m%d" % (tuple(gy.shape), c)):
            check(lib.vs_conv_k3_bwd_data_wgrad(gy.data_ptr(), _p(ax), _p(axs), _p(asums), wpb.data_ptr(), g.data_ptr(), x.data_ptr(), xs.data_ptr(),
                                                sums.data_ptr(), slabs.data_ptr(), gn, gd, gh, gw, gc, c, dt, EPS_IN, _stream()), "conv_k3_bwd_data_wgrad")
        gw_t = _group_submit_slabs(weight, slabs, nslabs, m_real, c_real, (gy, x, xs))
        if defer:
            _defer_register(g, x, xs, sums)
        else:
            _apply_in_place(g, x, xs, sums)
        return g, gw_t
    if lazy is not None:
        ax, axs, asums = lazy
        dx = torch.empty_like(gy) if want_dx else None
        kid = nb = fl = None
        if PROFILE is not None:
            tiles = gn * ((gd + 3) // 4) * ((gh + 3) // 4) * ((gw + 15) // 16)
            kid = _k3_kid(_tname(x), min(gc, 32), _pick_mt((c + 15) // 16 * 16, tiles), sums=True, geom=(gn, gd, gh, gw), m=c) + "+apply"
            nb = (2 * gy.numel() + 2 * g.numel() + (gy.numel() if want_dx else 0)) * _esize(x) + gc * c * 27 * _esize(x)
            fl = 2.0 * (g.numel() // c) * 27 * gc * c
        with _timed(kid, nb, fl, "bwd+apply gy%s->m%d" % (tuple(gy.shape), c)):
            check(lib.vs_conv_k3_bwd_data_fused_apply(gy.data_ptr(), ax.data_ptr(), axs.data_ptr(), asums.data_ptr(), wpb.data_ptr(), g.data_ptr(),
                                                      x.data_ptr(), xs.data_ptr(), sums.data_ptr(), _p(dx), gn, gd, gh, gw, gc, c, dt, EPS_IN,
                                                      _stream()), "conv_k3_bwd_data_fused_apply")
        if defer:
            _defer_register(g, x, xs, sums)
        else:
            _apply_in_place(g, x, xs, sums)
        return g, dx
    if (not scatter and kind == VS_CONV_K3 and not defer and EPILOGUE_APPLY and (x.data_ptr(), tuple(x.shape)) not in _PENDING["grads"]
            and lib.vs_conv_k3_bwd_data_applied_supported(gn, gd, gh, gw, gc, c, dt)):
        # the 24^3 / 12^3 levels: the backward-data launch applies the InstanceNorm+ReLU backward to its own outputs (csrc/igemm_k3b.h EA): no apply launch
        sync = _ea_sync(gn, x.device)
        kid = nb = fl = None
        if PROFILE is not None:
            tiles = gn * ((gd + 3) // 4) * ((gh + 3) // 4) * ((gw + 15) // 16)
            kid = _k3_kid(_tname(x), min(gc, 32), 16, sums=True, geom=(gn, gd, gh, gw), m=c) + "+ea"
            nb = (gy.numel() + 2 * g.numel()) * _esize(x) + gc * c * 27 * _esize(x)
            fl = 2.0 * (g.numel() // c) * 27 * gc * c
        with _timed(kid, nb, fl, "bwd+ea gy%s->m%d" % (tuple(gy.shape), c)):
            check(lib.vs_conv_k3_bwd_data_applied(gy.data_ptr(), wpb.data_ptr(), g.data_ptr(), x.data_ptr(), xs.data_ptr(), sums.data_ptr(), sync.data_ptr(),
                                                  _chain_fault_word(x.device).data_ptr(), gn, gd, gh, gw, gc, c, dt, EPS_IN, _stream()), "conv_k3_bwd_data_applied")
        return g
    if (kind != VS_CONV_K3 and not defer and EPILOGUE_APPLY and EPILOGUE_APPLY_S2 and lib.vs_conv_s2_bwd_data_applied_supported(gn, gd, gh, gw, gc, c, 1 if scatter else 0, dt)):
        # the stride-2 / transposed launches of the <= 48^3 levels: g1_kernel applies the InstanceNorm+ReLU backward to its own outputs (csrc/igemm.h), the
        # skip's parked gradient of the same tensor summed in as the standalone apply would
        sync = _ea_sync(gn, x.device)
        add = _collect_gradient(x)
        kid = nb = fl = None
        if PROFILE is not None:
            tiles = gn * ((gd * gh * gw + 255) // 256) if scatter else n * ((g.numel() // (n * c) + 255) // 256)
            rows = (8 * c + 15) // 16 * 16 if scatter else (c + 15) // 16 * 16
            kid = "g1_kernel<%s,%d,%d,%d,%d>+ea" % (_tname(x), min(gc, 32), 2 if scatter else kind, _pick_mt(rows, tiles), 2 if scatter else 0)
            nb = (gy.numel() + (2 if add is None else 3) * g.numel()) * _esize(x) + 8 * gc * c * _esize(x)
            fl = 2.0 * ((gy.numel() // gc) if scatter else (g.numel() // c)) * 8 * gc * c
        with _timed(kid, nb, fl, "bwd+ea gy%s->m%d" % (tuple(gy.shape), c)):
            check(lib.vs_conv_s2_bwd_data_applied(gy.data_ptr(), wpb.data_ptr(), g.data_ptr(), x.data_ptr(), xs.data_ptr(), sums.data_ptr(), _p(add), sync.data_ptr(),
                                                  _chain_fault_word(x.device).data_ptr(), gn, gd, gh, gw, gc, c, 1 if scatter else 0, dt, EPS_IN, _stream()),
                  "conv_s2_bwd_data_applied")
        return g
    if scatter:
        kid = nb = fl = None
        if PROFILE is not None:
            tiles = gn * ((gd * gh * gw + 255) // 256)
            kid = "g1_kernel<%s,%d,2,%d,2>" % (_tname(x), min(gc, 32),
                                               _pick_mt((8 * c + 15) // 16 * 16, tiles))
            nb = (gy.numel() + 2 * g.numel()) * _esize(x) + 8 * gc * c * _esize(x)
            fl = 2.0 * (gy.numel() // gc) * 8 * gc * c
        with _timed(kid, nb, fl, "bwd gy%s->m%d" % (tuple(gy.shape), c)):
            check(lib.vs_conv_scatter_bwd_data(gy.data_ptr(), wpb.data_ptr(), g.data_ptr(), x.data_ptr(), xs.data_ptr(),
                                               sums.data_ptr(), gn, gd, gh, gw, gc, c, dt, EPS_IN, _stream()), "conv_scatter_bwd_data")
    else:
        kid = nb = fl = None
        if PROFILE is not None:
            taps = 27 if kind == VS_CONV_K3 else 8
            if kind == VS_CONV_K3:
                tiles = gn * ((gd + 3) // 4) * ((gh + 3) // 4) * ((gw + 15) // 16)
            else:
                tiles = n * ((g.numel() // (n * c) + 255) // 256)
            tname = _tname(x)
            if kind == VS_CONV_K3:
                kid = _k3_kid(tname, min(gc, 32), _pick_mt((c + 15) // 16 * 16, tiles), sums=True, geom=(gn, gd, gh, gw), m=c)
            else:
                kid = "g1_kernel<%s,%d,%d,%d,0>" % (tname, min(gc, 32), kind, _pick_mt((c + 15) // 16 * 16, tiles))
            cr = real_channels[0] if real_channels else gc
            mr = real_channels[1] if real_channels else c
            vox_out = g.numel() // c
            nb = (gy.numel() // gc * cr + 2 * vox_out * mr) * _esize(x) + cr * mr * taps * _esize(x)
            fl = 2.0 * vox_out * taps * cr * mr
        with _timed(kid, nb, fl, "bwd gy%s->m%d" % (tuple(gy.shape), c)):
            check(lib.vs_conv_gather_bwd_data(gy.data_ptr(), wpb.data_ptr(), g.data_ptr(), x.data_ptr(), xs.data_ptr(),
                                              sums.data_ptr(), gn, gd, gh, gw, gc, c, kind, dt, EPS_IN, _stream()), "conv_gather_bwd_data")
    if defer:
        _defer_register(g, x, xs, sums)
        return g
    return _apply_in_place(g, x, xs, sums)


def _apply_in_place(g, x, xs, sums):
    n, c = x.shape[0], x.shape[-1]
    voxels = x.numel() // (n * c)
    tname = _tname(x)
    add = _collect_gradient(x)                 # the skip's gradient of the same tensor, if one was parked
    with _timed("in_relu_bwd_apply_kernel<%s>" % tname, (3 if add is None else 4) * x.numel() * _esize(x), 6.0 * x.numel(), str(tuple(x.shape))):
        check(lib.vs_instnorm_relu_bwd_apply_add(g.data_ptr(), x.data_ptr(), xs.data_ptr(), sums.data_ptr(), _p(add), g.data_ptr(), n, voxels,
                                                 c, vs_dtype(x), EPS_IN, _stream()), "instnorm_relu_bwd_apply")
    return g


def conv_wgrad(p, ps, q, qs, m_real, c_real, kind, out_shape, out_ptr=None):
    """dW (fp32, reference layout [m][c][taps]) ; the voxel loop runs over p's grid.  With out_ptr the result goes to that
    preallocated fp32 buffer of out_shape (deferred side-stream launches) and nothing is returned."""
    n, dp, hp, wp_, m_ch = p.shape
    c_ch = q.shape[-1]
    nbytes = lib.vs_conv_wgrad_workspace_bytes(n, dp, hp, wp_, m_ch, c_ch, kind)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    dw = torch.empty(out_shape, dtype=torch.float32, device=p.device) if out_ptr is None else None
    dw_ptr = dw.data_ptr() if out_ptr is None else out_ptr
    kid = nb = fl = None
    if PROFILE is not None:
        taps = 27 if kind == VS_CONV_K3 else 8
        cb, kk = 16 if c_ch >= 16 else 8, 0 if kind == VS_CONV_K3 else 1
        kid = "g3_kernel<float,%d,%d>" % (cb, kk) if p.dtype == torch.float32 else "g3b_kernel<%d,%d>" % (cb, kk)
        nb = (p.numel() // m_ch * m_real + q.numel() // c_ch * c_real) * _esize(p) + m_real * c_real * taps * 4
        fl = 2.0 * (p.numel() // m_ch) * taps * m_real * c_real
    with _timed(kid, nb, fl, "p%s q%s" % (tuple(p.shape), tuple(q.shape))):
        check(lib.vs_conv_wgrad(p.data_ptr(), _p(ps), q.data_ptr(), _p(qs), dw_ptr, ws.data_ptr(), nbytes, n, dp, hp,
                                wp_, m_ch, c_ch, m_real, c_real, kind, vs_dtype(p), EPS_IN, _stream()), "conv_wgrad")
    return dw


def bias_grad(g, c_real, out_ptr=None):
    c_ch = g.shape[-1]
    rows = g.numel() // c_ch
    db = torch.empty(c_real, dtype=torch.float32, device=g.device) if out_ptr is None else None
    check(lib.vs_bias_grad(g.data_ptr(), db.data_ptr() if out_ptr is None else out_ptr, rows, c_ch, c_real, vs_dtype(g), _stream()),
          "bias_grad")
    return db


# ------------------------------------------------------------------------------------------------
# grouped weight gradients (default): one descriptor per layer during backward, a handful of launches at its end
# ------------------------------------------------------------------------------------------------
# A step has 34 weight-gradient kernels, 34 slab reductions and 9 bias gradients (+ their zero fills); most belong to layers
# with a few dozen workgroups and cost a launch round trip each (4.7 us minimum, 0.85 ms per 96^3 step together).  Nothing in
# backward reads them, so they are collected as vs_wgrad_desc records and issued by vs_conv_wgrad_multi when the pass ends
# (autograd-engine callback): layers of one kernel instantiation share one grid, every reduction shares one.
import ctypes as _ct


class WgradDesc(_ct.Structure):
    """vs_wgrad_desc (include/vaeseg.h)"""
    _fields_ = [("p", _ct.c_void_p), ("p_stats", _ct.c_void_p), ("q", _ct.c_void_p), ("q_stats", _ct.c_void_p),
                ("dw", _ct.c_void_p), ("bias_g", _ct.c_void_p), ("db", _ct.c_void_p), ("bias_rows", _ct.c_longlong),
                ("bias_c_ch", _ct.c_int), ("bias_c_real", _ct.c_int),
                ("n", _ct.c_int), ("dp", _ct.c_int), ("hp", _ct.c_int), ("wp", _ct.c_int), ("m_ch", _ct.c_int), ("c_ch", _ct.c_int),
                ("m_real", _ct.c_int), ("c_real", _ct.c_int), ("kind", _ct.c_int), ("reserved_", _ct.c_int)]


_GROUP = {"enabled": os.environ.get("VS_WGRAD_GROUP", "1") != "0", "descs": [], "keep": [], "callback": False, "dtype": None,
          "bytes": 0.0, "flops": 0.0, "split": None, "slots": {}}
# "slots": id(weight) -> (gw, gb) handed to autograd by the FIRST use of that weight in the current backward pass.  A weight used several
# times (the VAE inside Embed runs three times per forward, joint_model.py:469-500) queues one descriptor per use, all with the first use's
# destination: vs_conv_wgrad_multi sums the uses, and the later uses return None to autograd (nothing left to accumulate).


def _issue_wgrads(entries):
    descs = [x[0] for x in entries]
    arr = (WgradDesc * len(descs))(*descs)
    dt = vs_of(_GROUP["dtype"])
    dev = torch.device("cuda", torch.cuda.current_device())
    nbytes = lib.vs_conv_wgrad_multi_workspace_bytes(_ct.addressof(arr), len(descs), dt)
    if nbytes == 0:
        _GROUP["descs"], _GROUP["keep"] = [], []
        raise _lib.VaesegError("vs_conv_wgrad_multi: unsupported layer in the deferred weight-gradient list")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nb, fl = sum(x[2] for x in entries), sum(x[3] for x in entries)
    with _timed("wgrad_multi(%d layers)" % len(descs), nb, fl):
        check(lib.vs_conv_wgrad_multi(_ct.addressof(arr), len(descs), ws.data_ptr(), nbytes, dt, EPS_IN, _stream()), "conv_wgrad_multi")
    return ws


def set_wgrad_grouping(enabled=True):
    """Defer weight/bias gradients to the end of backward and issue them as grouped launches (default on)."""
    flush_wgrads()
    _GROUP["enabled"] = bool(enabled)


def set_wgrad_split(first=None):
    """Two-phase issue for the data-parallel step (ddp.FlatGradSync): with `first` = a predicate on a parameter, the launches at the end
    of backward cover only the layers whose weight satisfies it; the caller issues the rest with flush_wgrads() after it has started the
    all-reduce of the first bucket, so that the exchange runs under the remaining weight-gradient kernels.  None: one phase."""
    flush_wgrads()
    _GROUP["split"] = first


def drop_stale_wgrads():
    """Forget deferred descriptors left behind by a backward pass that raised before its end-of-pass callback ran (their raw pointers
    may be recycled by now).  Called at the top of every forward (stats_arena_begin)."""
    g = _GROUP
    if g["descs"] and not g["callback"]:
        return                                  # a caller-managed second phase (set_wgrad_split) is pending: not stale
    if g["descs"] or g["callback"]:
        g["descs"], g["keep"], g["callback"], g["bytes"], g["flops"] = [], [], False, 0.0, 0.0
    g["slots"] = {}
    _UP_JOBS.clear()
    # the same for gradients parked / handed over un-applied by a pass that died: their addresses may be recycled by now, and a later
    # backward must never mistake a fresh tensor at such an address for one of them
    for reg in (_PENDING, _LAZY_APPLY):
        reg["grads"].clear()
        reg["callback"] = False


def _group_submit(weight, keep, wgrad_args, bias_args, gw, gb, up_co=0):
    p, ps, q, qs, m_real, c_real, kind = wgrad_args
    g = _GROUP
    if g["descs"] and g["dtype"] != p.dtype:
        flush_wgrads()
    g["dtype"] = p.dtype
    n, dp, hp, wp_, m_ch = p.shape
    gw_ptr = gw if isinstance(gw, int) else gw.data_ptr()
    if kind == VS_CONV_UP:                   # p is the FINE gradient (n, 2dp, 2hp, 2wp, Co): the descriptor's grid is the coarse one, its rows the 8 Co view channels
        dp, hp, wp_, m_ch = dp // 2, hp // 2, wp_ // 2, 8 * up_co
    d = WgradDesc(p.data_ptr(), _p(ps), q.data_ptr(), _p(qs), gw_ptr, None, None, 0, 0, 0,
                  n, dp, hp, wp_, m_ch, q.shape[-1], m_real, c_real, kind, up_co)
    if bias_args is not None:
        bg = bias_args[0]
        gb_ptr = gb if isinstance(gb, int) else gb.data_ptr()
        d.bias_g, d.db, d.bias_rows, d.bias_c_ch, d.bias_c_real = bg.data_ptr(), gb_ptr, bg.numel() // bg.shape[-1], bg.shape[-1], bias_args[1]
        g["keep"].append(bg)
    taps = 8 if kind == VS_CONV_K2S2 else 27
    nb = (p.numel() + q.numel() // q.shape[-1] * c_real) * _esize(p) + m_real * c_real * taps * 4 if kind == VS_CONV_UP else \
        (p.numel() // m_ch * m_real + q.numel() // q.shape[-1] * c_real) * _esize(p) + m_real * c_real * taps * 4
    fl = 2.0 * (q.numel() // q.shape[-1]) * taps * m_real * c_real if kind == VS_CONV_UP else 2.0 * (p.numel() // m_ch) * taps * m_real * c_real
    first = g["split"] is None or bool(g["split"](weight))
    voxels = n * dp * hp * wp_
    g["descs"].append((d, first, nb, fl, voxels))
    g["keep"].extend(t for t in keep if t is not None)
    if not g["callback"]:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(_group_backward_done)
            g["callback"] = True
        except RuntimeError:
            flush_wgrads()                      # not inside a backward pass: nothing will call back


def _group_backward_done():
    _USE_EPOCH[0] += 1                          # a backward pass ended: the use counts of the next forward start over (_count_use)
    _GROUP["callback"] = False
    flush_wgrads(first_only=_GROUP["split"] is not None)
    _GROUP["slots"] = {}


def pending_wgrads():
    return len(_GROUP["descs"])


def flush_wgrads(first_only=False):
    """Issue the deferred weight/bias gradients on the current stream (vs_conv_wgrad_multi): all of them, or — under
    set_wgrad_split — only the first phase."""
    g = _GROUP
    if not g["descs"]:
        return
    now = [e for e in g["descs"] if e[1]] if first_only else g["descs"]
    later = [e for e in g["descs"] if not e[1]] if first_only else []
    g["descs"] = later
    if not now:
        return
    _issue_wgrads(now)
    if not later:
        _run_up_jobs()                          # parameter-space chain rule of the composed Up heads: reads the dWeff the launch above reduced
        g["keep"] = []                          # launched on the current stream: the allocator may recycle the inputs now


# Weight gradient fused into the backward-data launch (csrc/igemm_k3tw.h; round 5): the 8 -> 8 3x3x3 layers whose backward-data kernel already holds both
# operands of dW.  Taken when the weight is used exactly ONCE in this pass (counted at forward time; _USE_EPOCH moves on when a backward pass ends) and its
# gradient can be deferred like every grouped one; the slabs the launch writes join the grouped reduction as a VS_WGRAD_SLABS descriptor.
FUSE_WGRAD = os.environ.get("VS_FUSE_WGRAD", "1") != "0"
VS_WGRAD_SLABS = 16
_USE_EPOCH = [0]


def _count_use(weight):
    u = getattr(weight, "_vs_use", None)
    if u is None or u[0] != _USE_EPOCH[0]:
        weight._vs_use = [_USE_EPOCH[0], 1]
    else:
        u[1] += 1


def _wgrad_fusable(gy, x, weight):
    if not (FUSE_WGRAD and _GROUP["enabled"] and gy.dtype != torch.float32 and gy.shape[-1] == 8 and x.shape[-1] == 8):
        return False
    if getattr(weight, "_vs_use", None) != [_USE_EPOCH[0], 1] or _GROUP["slots"].get(id(weight)) is not None:
        return False
    if not (weight.is_leaf and weight.grad is None and not _has_hooks(weight) and not torch.is_grad_enabled()):
        return False                            # the conditions under which _side_grads defers a gradient
    n, d, h, w, _ = gy.shape
    return bool(lib.vs_conv_k3_bwd_data_wgrad_supported(n, d, h, w, 8, 8, vs_dtype(gy)))


def _group_submit_slabs(weight, slabs, nslabs, m_real, c_real, keep, bias=None):
    """register the slabs of a fused launch with the pass's grouped weight gradients; -> the (still unwritten) gradient tensor handed to autograd
    (bias = (parameter, partial sums double [nslabs][m_real]): -> (gw, gb))"""
    g = _GROUP
    if g["descs"] and g["dtype"] != keep[0].dtype:
        flush_wgrads()
    g["dtype"] = keep[0].dtype
    gw = _grad_slot(weight, weight.shape)
    gb = None
    d = WgradDesc(slabs.data_ptr(), None, None, None, gw.data_ptr(), None, None, 0, 0, 0, nslabs, 0, 0, 0, 8, 8, m_real, c_real, VS_WGRAD_SLABS, 0)
    if bias is not None:
        gb = _grad_slot(bias[0], (m_real,))
        d.bias_g, d.db, d.bias_rows, d.bias_c_ch, d.bias_c_real = bias[1].data_ptr(), gb.data_ptr(), nslabs, m_real, m_real
        g["keep"].append(bias[1])
    # third field: this destination belongs to a SLAB descriptor — vs_conv_wgrad_multi does not let a regular descriptor share it (the forward-time use
    # count can read 1 with two live uses when an unrelated backward pass ended between two forwards of the same weight); _side_grads gives a later use its own
    g["slots"][id(weight)] = (gw.data_ptr(), None if gb is None else gb.data_ptr(), True)
    first = g["split"] is None or bool(g["split"](weight))
    g["descs"].append((d, first, float(slabs.numel() * 4), 0.0, 0))
    g["keep"].append(slabs)
    if not g["callback"]:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(_group_backward_done)
            g["callback"] = True
        except RuntimeError:
            flush_wgrads()
    return gw if bias is None else (gw, gb)


def _grad_slot(param, shape):
    """Where a parameter's gradient is written: its slice of the data-parallel flat bucket when ddp.FlatGradSync registered one
    (the all-reduce then needs no gather launch; autograd adopts the view as .grad), a fresh tensor otherwise."""
    view = getattr(param, "_vs_grad_view", None)
    if view is not None and param.grad is None:
        return view.detach()                    # a fresh alias: AccumulateGrad adopts a gradient only if nobody else holds the tensor object
    return torch.empty(shape, dtype=torch.float32, device=param.device)


def _has_hooks(t):
    return bool(getattr(t, "_backward_hooks", None)) or bool(getattr(t, "_post_accumulate_grad_hooks", None))


def _side_grads(weight, keep, wgrad_args, bias_args, bias=None):
    """Allocate dW (and db) now; their kernels are deferred — grouped at the end of backward (default) — or run at once when grouping is
    off, the parameter already holds a gradient to accumulate into, carries hooks, or grad mode is on (autograd would then clone the
    still-unwritten tensor); -> (gw, gb)."""
    grouping = _GROUP["enabled"]
    slot = _GROUP["slots"].get(id(weight)) if grouping and weight.is_leaf else None
    if slot is not None and len(slot) > 2 and slot[2]:
        slot = None                             # the first use went into its backward-data launch (slabs): this use gets a destination of its own, autograd adds the two
    if slot is not None:
        # a later use of the same weight in this pass: one more descriptor with the first use's destination, nothing returned to autograd
        _group_submit(weight, keep, wgrad_args, bias_args if slot[1] is not None else None, slot[0], slot[1])
        return None, None
    gw = _grad_slot(weight, weight.shape)
    gb = None
    if bias_args is not None:
        gb = (_grad_slot(bias, (bias_args[1],)) if bias is not None else
              torch.empty(bias_args[1], dtype=torch.float32, device=keep[0].device))
    # deferring hands autograd a still-unwritten tensor: only sound when its consumer is the parameter's AccumulateGrad (a leaf), which keeps it
    # untouched until the pass ends; a non-leaf weight's gradient is read by the next backward node at once
    deferrable = (weight.is_leaf and weight.grad is None and not _has_hooks(weight) and not torch.is_grad_enabled()
                  and (bias is None or (bias.is_leaf and not _has_hooks(bias))))
    if grouping and deferrable:
        _GROUP["slots"][id(weight)] = (gw.data_ptr(), None if gb is None else gb.data_ptr())      # addresses, not tensors: see below
        # the descriptor holds raw pointers only: AccumulateGrad must find gw / gb unshared to adopt them as .grad without a copy
        _group_submit(weight, keep, wgrad_args, bias_args, gw, gb)
        return gw, gb
    conv_wgrad(*wgrad_args, weight.shape, out_ptr=gw.data_ptr())
    if bias_args is not None:
        bias_grad(bias_args[0], bias_args[1], out_ptr=gb.data_ptr())
    return gw, gb


def _dead_bias_grad(bias, n, device):
    """Gradient of a conv bias that feeds InstanceNorm (exactly zero): the parameter's (never written, zero) slot of
    the flat bucket when one is registered, else zeros carved from the statistics arena (no fill launch).  Later uses of the same
    bias in one pass return None (nothing to accumulate)."""
    if bias is not None and _GROUP["enabled"]:
        key = ("dead", id(bias))
        if key in _GROUP["slots"]:
            return None
        _GROUP["slots"][key] = True
        if not _GROUP["callback"]:
            try:
                torch.autograd.Variable._execution_engine.queue_callback(_group_backward_done)
                _GROUP["callback"] = True
            except RuntimeError:
                _GROUP["slots"].pop(key, None)
    view = getattr(bias, "_vs_grad_view", None) if bias is not None else None
    if view is not None and bias.grad is None:
        return view.detach()
    return _new_stats(1, (n + 1) // 2, device, width=1).view(-1).view(torch.float32)[:n]


def in_relu_bwd(g, x, xs, inplace=True):
    """gradient w.r.t. the raw tensor x of a = relu(instnorm(x)), given g = dL/da (same layout)."""
    if xs is None:
        return g
    n, c = x.shape[0], x.shape[-1]
    voxels = x.numel() // (n * c)
    sums = _new_stats(n, c, x.device)
    dt = vs_dtype(x)
    tname = _tname(x)
    with _timed("in_relu_bwd_reduce_kernel<%s>" % tname, 2 * x.numel() * _esize(x), 4.0 * x.numel(), str(tuple(x.shape))):
        check(lib.vs_instnorm_relu_bwd_reduce(g.data_ptr(), x.data_ptr(), xs.data_ptr(), sums.data_ptr(), n, voxels, c, dt,
                                              EPS_IN, _stream()), "instnorm_relu_bwd_reduce")
    gx = g if inplace else torch.empty_like(g)
    with _timed("in_relu_bwd_apply_kernel<%s>" % tname, 3 * x.numel() * _esize(x), 6.0 * x.numel(), str(tuple(x.shape))):
        check(lib.vs_instnorm_relu_bwd_apply(g.data_ptr(), x.data_ptr(), xs.data_ptr(), sums.data_ptr(), gx.data_ptr(), n,
                                             voxels, c, dt, EPS_IN, _stream()), "instnorm_relu_bwd_apply")
    return gx


def _contig(t):
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------------
# autograd Functions
# ------------------------------------------------------------------------------------------------
class ConvK3(torch.autograd.Function):
    """3x3x3 conv (pad 1) on a lazy input; output is lazy (raw + stats) — joint_model.py:40-48,106-108.
    The bias of a conv that feeds InstanceNorm is mathematically dead: it is neither added
    nor differentiated (its gradient is returned as zeros, the reference's is ~1e-7 noise)."""

    @staticmethod
    def forward(ctx, x, xs, weight, bias, live_bias=False):
        _require_cuda(x, weight)
        cout, cin = weight.shape[0], weight.shape[1]
        wp = pack_weight_cached(weight, VS_PACK_ROWS_D0, x.shape[-1], k3_pack_dtype(x))
        # live_bias: the general norm path (NormAct) — under BatchNorm in eval mode the bias is not cancelled by the normalisation
        ctx.live_bias = bool(live_bias) and bias is not None
        b_use = bias if ctx.live_bias else None
        if b_use is not None and cout < cpad(cout):
            b_use = torch.nn.functional.pad(b_use.detach().float(), (0, cpad(cout) - cout))      # the kernels read one bias per padded output row
        y, ys = conv_gather(x, xs, wp, b_use, cpad(cout), VS_CONV_K3, True, real_channels=(cin, cout))
        ctx.save_for_backward(x, xs, weight)
        ctx.has_bias = bias is not None
        ctx.bias_ref = bias                   # a Parameter (long-lived leaf): only its gradient slot is looked up in backward
        ctx.defer = bool(getattr(x, "_vs_defer_apply", False)) and xs is not None     # see _LAZY_APPLY
        if ctx.needs_input_grad[2]:
            _count_use(weight)                # see _wgrad_fusable
        ctx.mark_non_differentiable(ys)
        ctx.set_materialize_grads(False)      # otherwise autograd zero-fills a gradient for the stats output every backward
        return y, ys

    @staticmethod
    def backward(ctx, gy, _gys):
        x, xs, weight = ctx.saved_tensors
        if gy is None:
            return None, None, None, None, None
        gy = _contig(gy)
        cout, cin = weight.shape[0], weight.shape[1]
        gx = gw = gb = None
        lazy = _take_lazy(gy)                   # gy is an un-applied gradient handed over by the consumer of this conv's output
        if lazy is not None and not (ctx.needs_input_grad[0] and _fa_supported(gy, x, xs is not None)):
            gy, lazy = apply_lazy(gy, lazy), None     # no fused-apply kernel for this launch / no input gradient wanted: apply now
        if ctx.needs_input_grad[0]:
            wpb = pack_weight_cached(weight, VS_PACK_ROWS_D1_FLIP, gy.shape[-1], k3_pack_dtype(gy))
            want_gb0 = ctx.has_bias and ctx.needs_input_grad[3] and ctx.live_bias
            if xs is not None and ctx.needs_input_grad[2] and not want_gb0 and _wgrad_fusable(gy, x, weight):
                # the backward-data launch of this layer forms its weight gradient as well (nothing else reads the applied gradient)
                gx, gw = conv_bwd_data_lazy(gy, wpb, x, xs, VS_CONV_K3, real_channels=(cout, cin), defer=ctx.defer, lazy=lazy,
                                            fuse_wgrad=(weight, cout, cin))
                gb = _dead_bias_grad(ctx.bias_ref, ctx.bias_ref.shape[0], x.device) if ctx.has_bias and ctx.needs_input_grad[3] else None
                return gx, None, gw, gb, None
            if lazy is not None and xs is not None:
                gx, gy = conv_bwd_data_lazy(gy, wpb, x, xs, VS_CONV_K3, real_channels=(cout, cin), defer=ctx.defer, lazy=lazy,
                                            want_dx=ctx.needs_input_grad[2])
            elif lazy is not None:                # the conv's own input is a stored tensor (VAE.in_block on the prediction): no sums to fuse
                ax, axs, asums = lazy
                gx = torch.empty_like(x)
                dx = torch.empty_like(gy) if ctx.needs_input_grad[2] else None
                n_, d_, h_, w_, c_ = gy.shape
                check(lib.vs_conv_k3_bwd_data_fused_apply(gy.data_ptr(), ax.data_ptr(), axs.data_ptr(), asums.data_ptr(), wpb.data_ptr(), gx.data_ptr(),
                                                          None, None, None, _p(dx), n_, d_, h_, w_, c_, x.shape[-1], vs_dtype(x), EPS_IN, _stream()),
                      "conv_k3_bwd_data_fused_apply")
                gy = dx
            elif xs is not None:
                gx = conv_bwd_data_lazy(gy, wpb, x, xs, VS_CONV_K3, real_channels=(cout, cin), defer=ctx.defer)
            else:
                gx, _ = conv_gather(gy, None, wpb, None, x.shape[-1], VS_CONV_K3, False, real_channels=(cout, cin))
        want_gb = ctx.has_bias and ctx.needs_input_grad[3]
        if ctx.needs_input_grad[2]:
            gw, gb = _side_grads(weight, (gy, x, xs), (gy, None, x, xs, cout, cin, VS_CONV_K3),
                                 (gy, cout) if want_gb and ctx.live_bias else None, ctx.bias_ref if ctx.live_bias else None)
        elif want_gb and ctx.live_bias:
            gb = bias_grad(gy, cout)
        if want_gb and not ctx.live_bias:
            gb = _dead_bias_grad(ctx.bias_ref, ctx.bias_ref.shape[0], x.device)
        return gx, None, gw, gb, None


# ------------------------------------------------------------------------------------------------
# Chains (csrc/chain.h, round 6): the 3x3x3 convolutions of one DoubleConv at the small volumes of the deep levels as ONE launch each way.
# InstanceNorm3d is per (sample, channel), so consecutive layers of one sample hand their tensors over inside the launch instead of ending it.
# ------------------------------------------------------------------------------------------------
CHAIN = os.environ.get("VS_CHAIN", "1") != "0"


class ChainLayer(_ct.Structure):
    """vs_chain_layer (include/vaeseg.h)"""
    _fields_ = [("x", _ct.c_void_p), ("x_stats", _ct.c_void_p), ("w_packed", _ct.c_void_p), ("y", _ct.c_void_p), ("y_stats", _ct.c_void_p),
                ("mask_x", _ct.c_void_p), ("mask_stats", _ct.c_void_p), ("sums", _ct.c_void_p), ("c_in", _ct.c_int), ("m_out", _ct.c_int),
                ("apply", _ct.c_int), ("reserved_", _ct.c_int)]


_CHAIN_FAULT = {}


def _chain_fault_word(device):
    """the device word a chain kernel raises when one of its bounded waits gave up (never in a correct launch); read back by chain_fault()"""
    key = torch.device(device)
    t = _CHAIN_FAULT.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the chain fault word must exist before a capture starts: run the step eagerly once (GraphedStep warms up)")
        t = _CHAIN_FAULT[key] = torch.zeros(32, dtype=torch.int32, device=key)
    return t


def chain_fault():
    """Host check (synchronises): raises if any chain kernel of this process ever gave up a wait — its results, and everything after them, are invalid."""
    for dev, t in _CHAIN_FAULT.items():
        if int(t[0].item()) != 0:
            raise _lib.VaesegError("a chain kernel on %s gave up a bounded wait (workgroups of one sample not co-resident): results invalid; set VS_CHAIN=0" % (dev,))


def device_is_shared(shared=True):
    """The in-kernel hand-offs (csrc/chain.h: chain kernels, epilogue apply) need every workgroup of a sample resident while its peers wait for it — true for a
    launch that has the device to itself (one process per GPU, the step's one stream: the deployment model), NOT when another process or stream runs kernels of the
    same kind on the same GPU at the same time: two launches that each hold part of the chip and wait for workgroups the other one keeps out never finish their
    waits (the bounded spins give up and raise the fault word: wrong numbers, reported by chain_fault()).  A host that shares a GPU between ranks (the test-suite's
    gloo ranks on one card, bench.py --share-gpu) calls this first: both forms are switched off in the library (vs_set_config) and here."""
    global CHAIN, EPILOGUE_APPLY
    on = 0 if shared else 1
    set_config(chain=on, epilogue_apply=on)
    CHAIN = EPILOGUE_APPLY = not shared


def _chain_sync(n, device):
    cnt = lib.vs_conv_k3_chain_sync_bytes(n) // 8
    buf = _new_stats(1, cnt + 16, device, width=1).view(-1)
    off = ((-buf.data_ptr()) % 128) // 8
    return buf[off:off + cnt]


def chain_ok(x, xs, convs):
    """may these consecutive 3x3x3 convs (nn.Conv3d holders; InstanceNorm + ReLU between them) on the lazy input (x, xs) run as one chain?"""
    if not CHAIN or len(convs) < 2 or len(convs) > 3 or x.dtype not in KERNEL_DTYPES:
        return False
    if getattr(x, "_vs_defer_apply", False):
        return False                            # x's producer wants its gradient un-applied (the 8 / 16-channel layers): not these volumes
    if any(tuple(c.weight.shape[2:]) != (3, 3, 3) for c in convs):
        return False
    n, d, h, w, c = x.shape
    cmax = max([c] + [cpad(cv.weight.shape[0]) for cv in convs])
    return bool(lib.vs_conv_k3_chain_supported(n, d, h, w, cmax, vs_dtype(x)))


class ConvK3Chain(torch.autograd.Function):
    """2 or 3 consecutive [3x3x3 conv -> InstanceNorm3d -> ReLU] triples of a DoubleConv (joint_model.py:35-52) on a lazy input; the output is lazy.
    forward: ONE launch (vs_conv_k3_chain); backward: ONE launch for the backward-data convs and the InstanceNorm+ReLU backward applies between them,
    the weight gradients join the pass's grouped launch as those of ConvK3 do.  The biases are dead, as in ConvK3."""

    @staticmethod
    def forward(ctx, x, xs, *params):
        _require_cuda(x)
        nl = len(params) // 2
        weights, biases = params[0::2], params[1::2]
        n, d, h, w, _ = x.shape
        layers = (ChainLayer * nl)()
        cur, curs, outs, keep = x, xs, [], []
        nb = fl = 0.0
        for l in range(nl):
            wt = weights[l]
            m = cpad(wt.shape[0])
            wp = pack_weight_cached(wt, VS_PACK_ROWS_D0, cur.shape[-1], k3_pack_dtype(cur))
            y = torch.empty((n, d, h, w, m), dtype=x.dtype, device=x.device)
            ys = _new_stats(n, m, x.device)
            layers[l] = ChainLayer(cur.data_ptr(), _p(curs), wp.data_ptr(), y.data_ptr(), ys.data_ptr(), None, None, None, cur.shape[-1], m, 0, 0)
            keep.append(wp)
            nb += (cur.numel() + y.numel() + wt.numel()) * _esize(x)
            fl += 2.0 * n * d * h * w * 27 * wt.shape[0] * wt.shape[1]
            outs.append((y, ys))
            cur, curs = y, ys
            if ctx.needs_input_grad[2 + 2 * l]:
                _count_use(wt)
        sync = _chain_sync(n, x.device)
        with _timed("k3_chain<%s,fwd,%d>" % (_tname(x), nl), nb, fl, "x%s" % (tuple(x.shape),)):
            check(lib.vs_conv_k3_chain(_ct.addressof(layers), nl, 0, None, sync.data_ptr(), _chain_fault_word(x.device).data_ptr(), n, d, h, w,
                                       vs_dtype(x), EPS_IN, _stream()), "conv_k3_chain (forward)")
        ctx.nl = nl
        ctx.bias_refs = biases
        ctx.save_for_backward(x, xs, *[t for pair in outs[:-1] for t in pair], *weights)
        ctx.mark_non_differentiable(outs[-1][1])
        ctx.set_materialize_grads(False)
        return outs[-1]

    @staticmethod
    def backward(ctx, gy, _gys):
        nl = ctx.nl
        saved = ctx.saved_tensors
        none = (None,) * (2 + 2 * nl)
        if gy is None:
            return none
        acts = [(saved[0], saved[1])] + [(saved[2 + 2 * i], saved[3 + 2 * i]) for i in range(nl - 1)]      # the input of layer l
        weights = saved[2 * nl:]
        gy = _contig(gy)
        lazy = _take_lazy(gy)
        if lazy is not None:
            gy = apply_lazy(gy, lazy)
        n, d, h, w, _ = gy.shape
        dev = gy.device
        layers = (ChainLayer * nl)()
        applied = [None] * nl                      # dL/d(raw output of layer l): what layer l's weight gradient reads
        applied[nl - 1] = gy
        g_in, add, keep = gy, None, []
        nb = fl = 0.0
        for k, l in enumerate(range(nl - 1, -1, -1)):
            ax, axs = acts[l]
            wt = weights[l]
            wpb = pack_weight_cached(wt, VS_PACK_ROWS_D1_FLIP, g_in.shape[-1], k3_pack_dtype(g_in))
            g = torch.empty_like(ax)
            sums = _new_stats(n, ax.shape[-1], dev) if axs is not None else None
            if l == 0 and axs is not None:
                add = _collect_gradient(ax)         # a skip's gradient of the block's (lazy) input, parked by Materialize.backward
            layers[k] = ChainLayer(g_in.data_ptr(), None, wpb.data_ptr(), g.data_ptr(), None, ax.data_ptr() if axs is not None else None, _p(axs), _p(sums),
                                   g_in.shape[-1], ax.shape[-1], 1 if axs is not None else 0, 0)
            keep += [wpb, sums]
            nb += (g_in.numel() + (4 if axs is not None else 1) * g.numel() + wt.numel()) * _esize(gy)
            fl += 2.0 * n * d * h * w * 27 * wt.shape[0] * wt.shape[1]
            if l > 0:
                applied[l - 1] = g
            g_in = g
        sync = _chain_sync(n, dev)
        with _timed("k3_chain<%s,bwd,%d>" % (_tname(gy), nl), nb, fl, "gy%s" % (tuple(gy.shape),)):
            check(lib.vs_conv_k3_chain(_ct.addressof(layers), nl, 1, _p(add), sync.data_ptr(), _chain_fault_word(dev).data_ptr(), n, d, h, w,
                                       vs_dtype(gy), EPS_IN, _stream()), "conv_k3_chain (backward)")
        out = [g_in if ctx.needs_input_grad[0] else None, None]
        for l in range(nl):
            wt, bias = weights[l], ctx.bias_refs[l]
            gw = gb = None
            if ctx.needs_input_grad[2 + 2 * l]:
                ax, axs = acts[l]
                gw, _ = _side_grads(wt, (applied[l], ax, axs), (applied[l], None, ax, axs, wt.shape[0], wt.shape[1], VS_CONV_K3), None, None)
            if bias is not None and ctx.needs_input_grad[3 + 2 * l]:
                gb = _dead_bias_grad(bias, bias.shape[0], dev)
            out += [gw, gb]
        return tuple(out)


class ConvK3Softmax(torch.autograd.Function):
    """out_block (3x3x3 conv, live bias) + Softmax(dim=1) -> planar fp32 probabilities (joint_model.py:224-225,265-266 / 366-367,386-388):
    ONE fused launch for two classes (every BASELINE configuration), conv + softmax pass for 1 or 3..8 classes."""

    @staticmethod
    def forward(ctx, x, xs, weight, bias, drop_p=0.0, drop_seed=0):
        _require_cuda(x, weight)
        nc = weight.shape[0]
        if not 1 <= nc <= 8:
            raise NotImplementedError("out_block + softmax: n_class must be 1..8, got %d" % nc)
        n, d, h, w, c = x.shape
        wp = pack_weight_cached(weight, VS_PACK_ROWS_D0, c, k3_pack_dtype(x))
        prob = torch.empty((n, nc, d, h, w), dtype=torch.float32, device=x.device)
        ctx.fused2 = nc == 2 and c == 8          # the fused two-class kernel reads 8 stored input channels (n_fmaps[0] = 8); wider inputs: conv + softmax pass
        if ctx.fused2:
            check(lib.vs_conv_k3_softmax2_dropout_fwd(x.data_ptr(), _p(xs), wp.data_ptr(), _p(bias), prob.data_ptr(), n, d, h, w, c,
                                                      vs_dtype(x), EPS_IN, float(drop_p), drop_seed, _stream()), "conv_k3_softmax2_fwd")
        else:       # more structures than one (main_source.py:92-93), or a wider out_block input: the plain conv, then the softmax as its own pass
            bias8 = None if bias is None else torch.nn.functional.pad(bias.detach().float(), (0, 8 - nc))      # the conv kernels read one bias per padded row
            logits, _ = conv_gather(x, xs, wp, bias8, 8, VS_CONV_K3, False, real_channels=(weight.shape[1], nc))
            check(lib.vs_softmax_cl_fwd(logits.data_ptr(), prob.data_ptr(), n, d * h * w, 8, nc, vs_dtype(x), float(drop_p), drop_seed, _stream()),
                  "softmax_cl_fwd")
        ctx.save_for_backward(x, xs, weight, prob)
        ctx.has_bias = bias is not None
        ctx.bias_ref = bias
        ctx.drop = (float(drop_p), drop_seed)
        ctx.defer = bool(getattr(x, "_vs_defer_apply", False)) and xs is not None
        if ctx.needs_input_grad[2]:
            _count_use(weight)                # see _wgrad_fusable
        return prob

    @staticmethod
    def backward(ctx, gprob):
        x, xs, weight, prob = ctx.saved_tensors
        n, d, h, w, c = x.shape
        gprob = _contig(gprob.float())
        nc = weight.shape[0]
        if nc == 2 and x.dtype != torch.float32:
            fused = _out_block_bwd_fused(ctx, x, xs, weight, prob, gprob, None)      # the whole backward as one launch (csrc/igemm_k3tw.h SM)
            if fused is not None:
                return fused
        gl = torch.empty((n, d, h, w, 8), dtype=x.dtype, device=x.device)
        if ctx.fused2:
            check(lib.vs_softmax2_dropout_bwd(prob.data_ptr(), gprob.data_ptr(), gl.data_ptr(), n, d * h * w, 8, vs_dtype(x),
                                              ctx.drop[0], ctx.drop[1], _stream()), "softmax2_bwd")
        else:
            check(lib.vs_softmax_cl_bwd(prob.data_ptr(), gprob.data_ptr(), gl.data_ptr(), n, d * h * w, 8, nc, vs_dtype(x),
                                        ctx.drop[0], ctx.drop[1], _stream()), "softmax_cl_bwd")
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            wpb = pack_weight_cached(weight, VS_PACK_ROWS_D1_FLIP, 8, k3_pack_dtype(x))
            if xs is not None:
                gx = conv_bwd_data_lazy(gl, wpb, x, xs, VS_CONV_K3, real_channels=(nc, weight.shape[1]), defer=ctx.defer)
            else:
                gx, _ = conv_gather(gl, None, wpb, None, c, VS_CONV_K3, False)
        if ctx.needs_input_grad[2]:
            gw, gb = _side_grads(weight, (gl, x, xs), (gl, None, x, xs, nc, weight.shape[1], VS_CONV_K3),
                                 (gl, nc) if ctx.has_bias and ctx.needs_input_grad[3] else None, ctx.bias_ref)
        elif ctx.has_bias and ctx.needs_input_grad[3]:
            gb = bias_grad(gl, nc)
        return gx, None, gw, gb, None, None


class ConvK3SoftmaxCL(torch.autograd.Function):
    """ConvK3Softmax that ALSO returns the probabilities as the channels-last bf16 tensor the next network reads
    (Joint.forward: Segmentation's prediction is the VAE's input, joint_model.py:447-450) -> (prob, prob_cl).  Saves the
    vs_pack_planar launch in forward and, in backward, vs_unpack_planar and autograd's add of the two gradients of prob:
    the softmax backward takes both parts (vs_softmax2_cl_bwd).  bf16 kernels only."""

    @staticmethod
    def forward(ctx, x, xs, weight, bias, drop_p=0.0, drop_seed=0):
        _require_cuda(x, weight)
        if weight.shape[0] != 2 or x.dtype == torch.float32:
            raise NotImplementedError("fused out_block+softmax with a channels-last copy: n_class == 2, 16-bit storage")
        n, d, h, w, c = x.shape
        wp = pack_weight_cached(weight, VS_PACK_ROWS_D0, c, k3_pack_dtype(x))
        prob = torch.empty((n, 2, d, h, w), dtype=torch.float32, device=x.device)
        prob_cl = torch.empty((n, d, h, w, 8), dtype=x.dtype, device=x.device)
        check(lib.vs_conv_k3_softmax2_cl_fwd(x.data_ptr(), _p(xs), wp.data_ptr(), _p(bias), prob.data_ptr(), prob_cl.data_ptr(), n, d, h, w, c,
                                             vs_dtype(x), EPS_IN, float(drop_p), drop_seed, _stream()), "conv_k3_softmax2_cl_fwd")
        ctx.save_for_backward(x, xs, weight, prob)
        ctx.has_bias = bias is not None
        ctx.bias_ref = bias
        ctx.drop = (float(drop_p), drop_seed)
        ctx.defer = bool(getattr(x, "_vs_defer_apply", False)) and xs is not None
        if ctx.needs_input_grad[2]:
            _count_use(weight)                # see _wgrad_fusable
        ctx.set_materialize_grads(False)
        return prob, prob_cl

    @staticmethod
    def backward(ctx, gprob, gcl):
        x, xs, weight, prob = ctx.saved_tensors
        if gprob is None and gcl is None:
            return None, None, None, None, None, None
        n, d, h, w, c = x.shape
        gprob = None if gprob is None else _contig(gprob.float())
        gcl = None if gcl is None else _contig(gcl)
        fused = _out_block_bwd_fused(ctx, x, xs, weight, prob, gprob, gcl)
        if fused is not None:
            return fused
        gl = torch.empty((n, d, h, w, 8), dtype=x.dtype, device=x.device)
        check(lib.vs_softmax2_cl_bwd(prob.data_ptr(), _p(gprob), _p(gcl), gl.data_ptr(), n, d * h * w, 8, vs_dtype(x), ctx.drop[0], ctx.drop[1],
                                     _stream()), "softmax2_cl_bwd")
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            wpb = pack_weight_cached(weight, VS_PACK_ROWS_D1_FLIP, 8, k3_pack_dtype(x))
            if xs is not None:
                gx = conv_bwd_data_lazy(gl, wpb, x, xs, VS_CONV_K3, real_channels=(2, weight.shape[1]), defer=ctx.defer)
            else:
                gx, _ = conv_gather(gl, None, wpb, None, c, VS_CONV_K3, False)
        if ctx.needs_input_grad[2]:
            gw, gb = _side_grads(weight, (gl, x, xs), (gl, None, x, xs, 2, weight.shape[1], VS_CONV_K3),
                                 (gl, 2) if ctx.has_bias and ctx.needs_input_grad[3] else None, ctx.bias_ref)
        elif ctx.has_bias and ctx.needs_input_grad[3]:
            gb = bias_grad(gl, 2)
        return gx, None, gw, gb, None, None


FUSE_SOFTMAX_BWD = os.environ.get("VS_FUSE_SOFTMAX_BWD", "1") != "0"


def _out_block_bwd_fused(ctx, x, xs, weight, prob, gprob, gcl):
    """out_block's backward as ONE launch (vs_conv_k3_softmax2_bwd_data, csrc/igemm_k3tw.h SM): the softmax backward runs while the backward-data kernel stages
    its tile — the gradient of the logits is never stored — and a trainable layer's weight and bias gradients come out of the same launch (slabs + partials for the
    grouped reduction).  -> the tuple ConvK3SoftmaxCL.backward returns, or None when this launch does not apply (the three-launch path then runs)."""
    n, d, h, w, c = x.shape
    want_w, want_b = ctx.needs_input_grad[2], ctx.has_bias and ctx.needs_input_grad[3]
    if not (FUSE_SOFTMAX_BWD and ctx.needs_input_grad[0] and xs is not None and c == 8 and (gcl is None or gcl.shape[-1] == 8)):
        return None
    if not lib.vs_conv_k3_bwd_data_wgrad_supported(n, d, h, w, 8, 8, vs_dtype(x)):
        return None
    if want_w:
        if not _wgrad_fusable(x, x, weight):    # (the logits' gradient has x's grid, storage type and 8 stored channels)
            return None
        bias = ctx.bias_ref
        if want_b and not (bias.is_leaf and bias.grad is None and not _has_hooks(bias)):
            return None
    elif want_b:
        return None                             # a frozen weight under a trainable bias: not a configuration of the reference
    wpb = pack_weight_cached(weight, VS_PACK_ROWS_D1_FLIP, 8, k3_pack_dtype(x))
    sums = _new_stats(n, c, x.device)
    g = torch.empty_like(x)
    nslabs = lib.vs_conv_k3_bwd_data_wgrad_slabs(n, d, h, w) if want_w else 0
    slabs = torch.empty(nslabs * 1728, dtype=torch.float32, device=x.device) if want_w else None
    bpart = torch.empty(nslabs * 2, dtype=torch.float64, device=x.device) if (want_w and want_b) else None
    kid = nb = fl = None
    if PROFILE is not None:
        kid = "k3tw_kernel<%s,2,%s>" % (_tname(x), "true" if want_w else "false")
        nb = (4 * n * d * h * w * 4) + (0 if gcl is None else gcl.numel() * _esize(x)) + 2 * g.numel() * _esize(x)
        fl = (2.0 if want_w else 1.0) * 2.0 * (g.numel() // c) * 27 * 2 * weight.shape[1]
    with _timed(kid, nb, fl, "out_block bwd%s (%d, %d, %d, %d)" % ("+wgrad" if want_w else "", n, d, h, w)):
        check(lib.vs_conv_k3_softmax2_bwd_data(prob.data_ptr(), _p(gprob), _p(gcl), wpb.data_ptr(), g.data_ptr(), x.data_ptr(), xs.data_ptr(), sums.data_ptr(),
                                               _p(slabs), _p(bpart), n, d, h, w, vs_dtype(x), EPS_IN, ctx.drop[0], ctx.drop[1], _stream()),
              "conv_k3_softmax2_bwd_data")
    gw = gb = None
    if want_w:
        if want_b:
            gw, gb = _group_submit_slabs(weight, slabs, nslabs, 2, weight.shape[1], (x,), bias=(ctx.bias_ref, bpart))
        else:
            gw = _group_submit_slabs(weight, slabs, nslabs, 2, weight.shape[1], (x,))
    if ctx.defer:
        _defer_register(g, x, xs, sums)
    else:
        _apply_in_place(g, x, xs, sums)
    return g, None, gw, gb, None, None


def out_block_softmax(x, xs, weight, bias, drop_p=0.0, drop_seed=0):
    """out_block + softmax -> planar fp32 probabilities; in bf16 mode the tensor carries its channels-last copy as `_vs_cl`, which a
    network that takes it as input (VAE / Joint) uses instead of re-packing it (set VS_SOFTMAX_CL=0 to disable)."""
    if x.dtype != torch.float32 and weight.shape[0] == 2 and x.shape[-1] == 8 and os.environ.get("VS_SOFTMAX_CL", "1") != "0":
        prob, prob_cl = ConvK3SoftmaxCL.apply(x, xs, weight, bias, drop_p, drop_seed)
        prob._vs_cl = prob_cl
        return prob
    return ConvK3Softmax.apply(x, xs, weight, bias, drop_p, drop_seed)


def planar_input(x, dtype):
    """channels-last kernel-dtype view of a planar (N, C, D, H, W) input: the producer's own channels-last copy when it left one
    (out_block_softmax), vs_pack_planar otherwise."""
    cl = getattr(x, "_vs_cl", None)
    if cl is not None and cl.dtype == dtype and cl.shape[0] == x.shape[0] and tuple(cl.shape[1:4]) == tuple(x.shape[2:]):
        return cl
    return PackPlanar.apply(x, dtype)


class ConvK2S2(torch.autograd.Function):
    """Conv3d(C, C, 2, stride 2) with live bias on a lazy input; output is final (feeds a conv directly)
    — joint_model.py:130."""

    @staticmethod
    def forward(ctx, x, xs, weight, bias):
        _require_cuda(x, weight)
        wp = pack_weight_cached(weight, VS_PACK_ROWS_D0, x.shape[-1], x.dtype)
        y, _ = conv_gather(x, xs, wp, bias, cpad(weight.shape[0]), VS_CONV_K2S2, False)
        ctx.save_for_backward(x, xs, weight)
        ctx.has_bias = bias is not None
        ctx.bias_ref = bias
        ctx.defer = bool(getattr(x, "_vs_defer_apply", False)) and xs is not None     # see _LAZY_APPLY
        return y

    @staticmethod
    def backward(ctx, gy):
        x, xs, weight = ctx.saved_tensors
        gy = _contig(gy)
        cout, cin = weight.shape[0], weight.shape[1]
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            wpb = pack_weight_cached(weight, VS_PACK_SCATTER_D1, gy.shape[-1], gy.dtype)
            if xs is not None:
                gx = conv_bwd_data_lazy(gy, wpb, x, xs, VS_CONV_K2S2, scatter=True, defer=ctx.defer)
            else:
                gx = conv_scatter(gy, None, wpb, None, x.shape[-1])
        if ctx.needs_input_grad[2]:
            gw, gb = _side_grads(weight, (gy, x, xs), (gy, None, x, xs, cout, cin, VS_CONV_K2S2),
                                 (gy, cout) if ctx.has_bias and ctx.needs_input_grad[3] else None, ctx.bias_ref)
        elif ctx.has_bias and ctx.needs_input_grad[3]:
            gb = bias_grad(gy, cout)
        return gx, None, gw, gb


class ConvT2S2(torch.autograd.Function):
    """ConvTranspose3d(C, C, 2, stride 2) with live bias on a lazy input; final output — joint_model.py:118."""

    @staticmethod
    def forward(ctx, x, xs, weight, bias):
        _require_cuda(x, weight)
        wp = pack_weight_cached(weight, VS_PACK_SCATTER_D1, x.shape[-1], x.dtype)
        y = conv_scatter(x, xs, wp, bias, cpad(weight.shape[1]))
        ctx.save_for_backward(x, xs, weight)
        ctx.has_bias = bias is not None
        ctx.bias_ref = bias
        ctx.defer = bool(getattr(x, "_vs_defer_apply", False)) and xs is not None     # see _LAZY_APPLY
        return y

    @staticmethod
    def backward(ctx, gy):
        x, xs, weight = ctx.saved_tensors
        gy = _contig(gy)
        cin, cout = weight.shape[0], weight.shape[1]
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            wpb = pack_weight_cached(weight, VS_PACK_ROWS_D0, gy.shape[-1], gy.dtype)
            if xs is not None:
                gx = conv_bwd_data_lazy(gy, wpb, x, xs, VS_CONV_K2S2, defer=ctx.defer)
            else:
                gx, _ = conv_gather(gy, None, wpb, None, x.shape[-1], VS_CONV_K2S2, False)
        if ctx.needs_input_grad[2]:
            gw, gb = _side_grads(weight, (gy, x, xs), (x, xs, gy, None, cin, cout, VS_CONV_K2S2),
                                 (gy, cout) if ctx.has_bias and ctx.needs_input_grad[3] else None, ctx.bias_ref)
        elif ctx.has_bias and ctx.needs_input_grad[3]:
            gb = bias_grad(gy, cout)
        return gx, None, gw, gb


# ------------------------------------------------------------------------------------------------
# composed Up block head: ConvTranspose3d(C, C, 2, stride 2) -> Conv3d(C, Co, 3, padding 1) as one operator (csrc/igemm_k4.h)
# ------------------------------------------------------------------------------------------------
FUSE_UP = os.environ.get("VS_FUSE_UP", "1") != "0"
# composed where it is measured faster than the two-launch pair.  Same-box sweep of this threshold on the 96^3 step (frozen VAE heads only),
# coarse voxels per sample: 48^3 only 2.551 ms; + 24^3 2.531; + 12^3 2.517; + 6^3 2.523; + 3^3 2.550 — on the 6^3 / 3^3 grids the 4x4x16-tile
# kernels of igemm_k4.h are mostly padding and their backward walks 8 Co / 32 short chunk stages.  At 160^3 (coarse 80^3 / 40^3 / 20^3 ...):
# 6.99 -> 6.88 ms once the 40^3 level is in.  Isolated kernels, forward / backward-data: 48^3 x 16: 19.8 / 20.0 us (pair: 27.6 + 19.7 / 34 + 12.4).
FUSE_UP_MIN_VOXELS = int(os.environ.get("VS_FUSE_UP_MIN_VOXELS", "1000"))
# Trainable weights through the composed head (tests/test_gpu_up.py: dW3, dW2, db2 against autograd): the weight-gradient side gains (the largest
# layer of the 16-channel bucket leaves it, the transposed conv's weight gradient and its full-resolution operand disappear) and the per-step
# helpers cost ~80 us whatever the volume (re-composition 32, boundary sums 21, chain rule 28: microseconds of work in launches bound by
# their dependent round trips).  Measured, same box: 96^3 B=2 (2 x 48^3 coarse voxels) 2.69 vs 2.66 ms and 128^3 B=1 (64^3) 3.87 vs 3.84 — a loss;
# 160^3 B=2 (2 x 80^3) 6.84 vs 7.19 ms — a 5 % gain.  Enabled from FUSE_UP_TRAINABLE_MIN_VOXELS coarse voxels (batch included) up;
# VS_FUSE_UP_TRAINABLE=0 / 1 forces it off / on.
_FUT = os.environ.get("VS_FUSE_UP_TRAINABLE", "")
FUSE_UP_TRAINABLE = _FUT != "0"
FUSE_UP_TRAINABLE_MIN_VOXELS = 0 if _FUT == "1" else int(os.environ.get("VS_FUSE_UP_TRAINABLE_MIN_VOXELS", "500000"))     # coarse voxels of the whole batch


def _up_stamp(wt, bt, w3):
    return (wt._version, wt.data_ptr(), w3._version, w3.data_ptr(), None if bt is None else (bt._version, bt.data_ptr()),
            _TRAIN_EPOCH[0] if (w3.requires_grad or wt.requires_grad) else _PACK_EPOCH[0])


# (id(w3), dtype) -> weak references to (wt, bt, w3): the trainable Up heads whose composed images repack_trainable() re-composes after every
# optimiser step.  Weak: a model that has been dropped (TestTimeFinetune copies, test fixtures) leaves the registry with its parameters, the
# plan itself lives on w3 (`_vs_up_plan`).  Entries are NOT pruned by use: a captured graph replays the composed kernels without running up_plan.
_UP_TRAINABLE = {}


def _up_compose_into(plan, wt, bt, w3, dtype):
    """(re)compose in place; the caller sets plan["stamp"] from the PARAMETERS (detached aliases carry their own version counters)"""
    cin, cm, co = wt.shape[0], wt.shape[1], w3.shape[0]
    check(lib.vs_up_compose(wt.data_ptr(), _p(bt), w3.data_ptr(), plan["weff"].data_ptr(), plan["img_f"].data_ptr(), plan["img_b"].data_ptr(),
                            plan["taps_f"].data_ptr(), plan["taps_b"].data_ptr(), plan["btab"].data_ptr(), cin, cm, co, vs_of(dtype), _stream()), "up_compose")


def up_plan(wt, bt, w3, dtype):
    """The composed images of an Up block's first two layers (FROZEN weights: packed once, cached on the 3x3x3 weight tensor at stable
    addresses — a captured HIP graph holds the pointers — and re-composed IN PLACE when any of the three tensors changed:
    refresh_frozen_packs / clear_pack_cache, as for the packed conv weights)."""
    plans = getattr(w3, "_vs_up_plan", None)
    if plans is None:
        plans = {}
        w3._vs_up_plan = plans
    plan = plans.get(dtype)
    if plan is None:
        cin, cm, co = wt.shape[0], wt.shape[1], w3.shape[0]
        sz = (_ct.c_size_t * 6)()
        check(lib.vs_up_compose_sizes(cin, cm, co, _ct.addressof(sz)), "up_compose_sizes")
        dev = w3.device
        buf = lambda nbytes: torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        plan = {"weff": buf(sz[0]), "img_f": buf(sz[1]), "img_b": buf(sz[2]), "taps_f": buf(sz[3]), "taps_b": buf(sz[4]), "btab": buf(sz[5]),
                "stamp": None, "src": (wt, bt)}
        plans[dtype] = plan
    if (w3.requires_grad or wt.requires_grad) and (id(w3), dtype) not in _UP_TRAINABLE:
        _UP_TRAINABLE[(id(w3), dtype)] = (_weakref.ref(wt), None if bt is None else _weakref.ref(bt), _weakref.ref(w3))
    if plan["stamp"] != _up_stamp(wt, bt, w3):
        with torch.no_grad():
            _up_compose_into(plan, wt.detach(), None if bt is None else bt.detach(), w3.detach(), dtype)
            plan["stamp"] = _up_stamp(wt, bt, w3)
    return plan


def _recompose_trainable_ups():
    for key, (rwt, rbt, rw3) in list(_UP_TRAINABLE.items()):
        wt, bt, w3, dtype = rwt(), None if rbt is None else rbt(), rw3(), key[1]
        plan = None if w3 is None else (getattr(w3, "_vs_up_plan", None) or {}).get(dtype)
        if wt is None or plan is None or (rbt is not None and bt is None) or id(w3) != key[0]:
            del _UP_TRAINABLE[key]          # the model is gone
            continue
        with torch.no_grad():
            _up_compose_into(plan, wt.detach(), None if bt is None else bt.detach(), w3.detach(), dtype)
            plan["stamp"] = _up_stamp(wt, bt, w3)


def up_composed_ok(x, tconv, conv3):
    """Can this Up block head run as the composed operator?  16-bit storage, channel pairs the kernels are instantiated for
    (vs_up_supported), large enough a grid to win (FUSE_UP_MIN_VOXELS).  Trainable weights: their gradients come from the composed
    weight-gradient (VS_CONV_UP descriptor in the grouped end-of-pass launches) through the parameter-space chain rule (vs_up_chain) — needs
    the grouped, single-phase weight-gradient mode (the default)."""
    wt, w3 = tconv.weight, conv3.weight
    if not FUSE_UP or x.dtype == torch.float32:
        return False
    trainable = wt.requires_grad or w3.requires_grad or (tconv.bias is not None and tconv.bias.requires_grad)
    if trainable and (not FUSE_UP_TRAINABLE or not _GROUP["enabled"] or _GROUP["split"] is not None
                      or not (wt.is_leaf and w3.is_leaf)):
        return False
    if tuple(wt.shape[2:]) != (2, 2, 2) or tuple(w3.shape[2:]) != (3, 3, 3) or w3.shape[1] != wt.shape[1] or x.shape[-1] != wt.shape[0]:
        return False
    if x.shape[1] * x.shape[2] * x.shape[3] < FUSE_UP_MIN_VOXELS:
        return False
    if trainable and x.shape[0] * x.shape[1] * x.shape[2] * x.shape[3] < FUSE_UP_TRAINABLE_MIN_VOXELS:
        return False
    return bool(lib.vs_up_supported(wt.shape[0], wt.shape[1], w3.shape[0], vs_dtype(x)))


class UpConvK3(torch.autograd.Function):
    """relu(instnorm(x)) [lazy] -> ConvTranspose3d(C, C, 2, 2) + bias -> Conv3d(C, Co, 3, pad 1) as ONE launch on the coarse grid
    (joint_model.py:116-120 + 40); output lazy (raw + statistics) on the fine grid.  No intermediate tensor, 3.4x fewer multiply-adds."""

    @staticmethod
    def forward(ctx, x, xs, wt, bt, w3, b3=None):
        _require_cuda(x, wt, w3)
        n, d, h, w, c = x.shape
        co = w3.shape[0]
        plan = up_plan(wt, bt, w3, x.dtype)
        ctx.b3 = b3                                # the 3x3x3 conv's bias: dead (InstanceNorm follows) — its gradient is returned as zeros
        y = torch.empty((n, 2 * d, 2 * h, 2 * w, co), dtype=x.dtype, device=x.device)
        ys = _new_stats(n, co, x.device)
        kid = nb = fl = None
        if PROFILE is not None:
            kid = "k4t_kernel<%d,%s>" % (min(c, 32), _tname(x))
            nb = (x.numel() + y.numel()) * _esize(x) + 64 * co * c * _esize(x)
            fl = 2.0 * (x.numel() // c) * 64 * co * c
        with _timed(kid, nb, fl, "up x%s->m%d" % (tuple(x.shape), co)):
            check(lib.vs_up_conv_fwd(x.data_ptr(), _p(xs), plan["img_f"].data_ptr(), plan["taps_f"].data_ptr(), plan["btab"].data_ptr(), y.data_ptr(),
                                     ys.data_ptr(), n, d, h, w, c, co, vs_dtype(x), EPS_IN, _stream()), "up_conv_fwd")
        ctx.save_for_backward(x, xs)
        ctx.plan = plan
        ctx.co = co
        ctx.params = (wt, bt, w3)               # Parameters (long-lived leaves): read by the chain rule, their gradient slots looked up in backward
        ctx.defer = bool(getattr(x, "_vs_defer_apply", False)) and xs is not None
        ctx.mark_non_differentiable(ys)
        ctx.set_materialize_grads(False)
        return y, ys

    @staticmethod
    def backward(ctx, gy, _gys):
        x, xs = ctx.saved_tensors
        if gy is None:
            return None, None, None, None, None, None
        gy = _contig(gy)
        lazy = _take_lazy(gy)
        if lazy is not None:
            gy = apply_lazy(gy, lazy)
        gwt = gbt = gw3 = gb3 = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            gwt, gbt, gw3 = _up_weight_grads(gy, x, xs, ctx.params, ctx.co, ctx.needs_input_grad)
        if ctx.b3 is not None and ctx.needs_input_grad[5]:
            gb3 = _dead_bias_grad(ctx.b3, ctx.b3.shape[0], x.device)
        if not ctx.needs_input_grad[0]:
            return None, None, gwt, gbt, gw3, gb3
        n, d, h, w, c = x.shape
        gx = torch.empty_like(x)
        sums = _new_stats(n, c, x.device) if xs is not None else None
        plan = ctx.plan
        kid = nb = fl = None
        if PROFILE is not None:
            kid = "k4g_kernel<%s>" % _tname(x)
            nb = (gy.numel() + (2 if xs is not None else 1) * x.numel()) * _esize(x) + 64 * ctx.co * c * _esize(x)
            fl = 2.0 * (x.numel() // c) * 64 * ctx.co * c
        with _timed(kid, nb, fl, "up bwd gy%s->m%d" % (tuple(gy.shape), c)):
            check(lib.vs_up_conv_bwd_data(gy.data_ptr(), plan["img_b"].data_ptr(), plan["taps_b"].data_ptr(), gx.data_ptr(), _p(x if xs is not None else None),
                                          _p(xs), _p(sums), n, d, h, w, ctx.co, c, vs_dtype(x), EPS_IN, _stream()), "up_conv_bwd_data")
        if xs is not None:
            if ctx.defer:
                _defer_register(gx, x, xs, sums)
            else:
                _apply_in_place(gx, x, xs, sums)
        return gx, None, gwt, gbt, gw3, gb3


_UP_JOBS = {}       # id(w3) -> the pending chain-rule job of a trainable composed Up head in the current backward pass


def _up_weight_grads(gy, x, xs, params, co, needs):
    """Weight gradients of the composed head: dWeff27 from a VS_CONV_UP descriptor in the grouped end-of-pass launch, the boundary sums of gy
    now (vs_up_faces), and a chain-rule job that flush_wgrads() runs right after the grouped launch.  -> (g wt, g bt, g w3) for autograd
    (unwritten until then, like every deferred weight gradient); later uses of the same weights in one pass add to the first use's job."""
    wt, bt, w3 = params
    n, d, h, w, c = x.shape
    job = _UP_JOBS.get(id(w3))
    first = job is None
    if first:
        dev = x.device
        gwt = _grad_slot(wt, wt.shape) if needs[2] else None
        gbt = _grad_slot(bt, bt.shape) if (bt is not None and needs[3]) else None
        gw3 = _grad_slot(w3, w3.shape) if needs[4] else None
        # the job holds raw ADDRESSES of the gradients, not the tensors: AccumulateGrad adopts a gradient as .grad (no copy of the still
        # unwritten buffer) only if nobody else holds the tensor object; .grad keeps the storage alive until the chain rule has written it
        job = {"dweff": torch.empty(8 * co * c * 27, dtype=torch.float32, device=dev),
               "faces": _new_stats(1, 27 * co // 2, dev),          # zeroed, statistics format: vs_up_faces accumulates (every use of the weights)
               "gwt": _p(gwt), "gbt": _p(gbt), "gw3": _p(gw3), "params": params, "co": co}
        _UP_JOBS[id(w3)] = job
    check(lib.vs_up_faces(gy.data_ptr(), job["faces"].data_ptr(), n, 2 * d, 2 * h, 2 * w, co, vs_dtype(gy), _stream()), "up_faces")
    _group_submit(w3, (gy, x, xs), (gy, None, x, xs, 8 * co, c, VS_CONV_UP), None, job["dweff"], None, up_co=co)
    deferrable = all(p is None or (p.is_leaf and p.grad is None and not _has_hooks(p)) for p in (wt, bt, w3)) and not torch.is_grad_enabled()
    if not deferrable:
        flush_wgrads()                          # runs the chain rule too
    return (gwt, gbt, gw3) if first else (None, None, None)


def _run_up_jobs():
    for job in _UP_JOBS.values():
        wt, bt, w3 = job["params"]
        check(lib.vs_up_chain(job["dweff"].data_ptr(), job["faces"].data_ptr(), wt.data_ptr(), _p(bt), w3.data_ptr(), job["gwt"], job["gbt"],
                              job["gw3"], wt.shape[0], wt.shape[1], job["co"], _stream()), "up_chain")
    _UP_JOBS.clear()


class Materialize(torch.autograd.Function):
    """(raw, stats) [+ (raw2, stats2)] -> relu(instnorm(raw)) [+ relu(instnorm(raw2))] as a final tensor.
    With two operands this is the additive U-Net skip (joint_model.py:380,382)."""

    @staticmethod
    def forward(ctx, x, xs, x2, x2s, park_second=False):
        _require_cuda(x)
        ctx.park_second = bool(park_second)
        n, c = x.shape[0], x.shape[-1]
        voxels = x.numel() // (n * c)
        out = torch.empty_like(x)
        check(lib.vs_instnorm_relu_fwd(x.data_ptr(), _p(xs), _p(x2), _p(x2s), out.data_ptr(), n, voxels, c, vs_dtype(x),
                                       EPS_IN, _stream()), "instnorm_relu_fwd")
        ctx.save_for_backward(x, xs, x2, x2s)
        return out

    @staticmethod
    def backward(ctx, g):
        x, xs, x2, x2s = ctx.saved_tensors
        g = _contig(g)
        g1 = g2 = None
        if (x2 is not None and xs is not None and x2s is not None and ctx.needs_input_grad[0] and ctx.needs_input_grad[2] and PROFILE is None):
            # both operands lazy (the U-Net skips): reduce and apply of the two in one launch each
            n, c = x.shape[0], x.shape[-1]
            voxels = x.numel() // (n * c)
            s1, s2 = _new_stats(n, c, x.device), _new_stats(n, c, x.device)
            g1, g2 = torch.empty_like(g), torch.empty_like(g)
            check(lib.vs_instnorm_relu_bwd_pair(g.data_ptr(), x.data_ptr(), xs.data_ptr(), s1.data_ptr(), g1.data_ptr(), x2.data_ptr(),
                                                x2s.data_ptr(), s2.data_ptr(), g2.data_ptr(), n, voxels, c, vs_dtype(x), EPS_IN, _stream()),
                  "instnorm_relu_bwd_pair")
            if ctx.park_second and not torch.is_grad_enabled():
                _park_gradient(x2, g2)          # the encoder conv that shares x2 sums it into its own gradient (no autograd add launch)
                return g1, None, None, None, None
            return g1, None, g2, None, None
        if ctx.needs_input_grad[0]:
            g1 = in_relu_bwd(g, x, xs, inplace=False) if xs is not None else g
        if x2 is not None and ctx.needs_input_grad[2]:
            g2 = in_relu_bwd(g, x2, x2s, inplace=False) if x2s is not None else g
        return g1, None, g2, None, None


VS_NORM_INSTANCE, VS_NORM_BATCH, VS_NORM_BATCH_EVAL, VS_NORM_NONE = 0, 1, 2, 3
VS_ACT_RELU, VS_ACT_SOFTPLUS = 0, 1


class NormAct(torch.autograd.Function):
    """(raw conv output, its statistics) -> act(norm(raw) * gamma + beta) as a stored tensor: the block settings no entry point of the
    reference uses — BatchNorm3d (joint_model.py:13, with running statistics), Softplus (joint_model.py:38) — and InstanceNorm with
    either activation.  Unfused on purpose (vaeseg.h: general normalisation); the InstanceNorm + ReLU configuration of every entry point
    never comes here (it stays lazy, fused into the convs).  bn = the nn.BatchNorm3d holder (running buffers, momentum, eps, training)
    or None for InstanceNorm."""

    @staticmethod
    def forward(ctx, x, xs, gamma, beta, bn, act, c_real):
        _require_cuda(x)
        n, c = x.shape[0], x.shape[-1]
        voxels = x.numel() // (n * c)
        if bn is None:
            mode, eps, mom, rm, rv, nbt = VS_NORM_INSTANCE, EPS_IN, 0.0, None, None, None
        elif isinstance(bn, str):             # "none": activation only (the conv -> ReLU pairs of the *_GS blocks, joint_model.py:58-63)
            mode, eps, mom, rm, rv, nbt = VS_NORM_NONE, EPS_IN, 0.0, None, None, None
        else:
            track = bn.track_running_stats and bn.running_mean is not None
            mode = VS_NORM_BATCH if (bn.training or not track) else VS_NORM_BATCH_EVAL
            eps = float(bn.eps)
            mom = 0.0 if bn.momentum is None else float(bn.momentum)
            rm, rv, nbt = (bn.running_mean, bn.running_var, bn.num_batches_tracked) if track else (None, None, None)
            if bn.momentum is None and track and mode == VS_NORM_BATCH:
                raise NotImplementedError("BatchNorm3d(momentum=None) (cumulative average) has no native form; the reference uses momentum=0.1")
        tab = torch.empty(2, n, c, dtype=torch.float32, device=x.device)
        check(lib.vs_norm_tables(_p(xs), n, c, c_real, float(voxels), mode, eps, mom, _p(rm), _p(rv), _p(nbt), tab[0].data_ptr(), tab[1].data_ptr(),
                                 _stream()), "norm_tables")
        y = torch.empty_like(x)
        check(lib.vs_norm_act_fwd(x.data_ptr(), tab[0].data_ptr(), tab[1].data_ptr(), _p(gamma), _p(beta), y.data_ptr(), n, voxels, c, c_real, act,
                                  vs_dtype(x), _stream()), "norm_act_fwd")
        ctx.save_for_backward(x, tab, gamma, beta)
        ctx.mode, ctx.act, ctx.c_real = mode, act, c_real
        return y

    @staticmethod
    def backward(ctx, g):
        x, tab, gamma, beta = ctx.saved_tensors
        g = _contig(g)
        n, c = x.shape[0], x.shape[-1]
        voxels = x.numel() // (n * c)
        dt, st = vs_dtype(x), _stream()
        sums = _new_stats(n, c, x.device)
        check(lib.vs_norm_act_bwd_reduce(g.data_ptr(), x.data_ptr(), tab[0].data_ptr(), tab[1].data_ptr(), _p(gamma), _p(beta), sums.data_ptr(), n,
                                         voxels, c, ctx.c_real, ctx.act, dt, st), "norm_act_bwd_reduce")
        coef = torch.empty(n, c, 3, dtype=torch.float32, device=x.device)
        dgamma = torch.empty_like(gamma) if gamma is not None and ctx.needs_input_grad[2] else None
        dbeta = torch.empty_like(beta) if beta is not None and ctx.needs_input_grad[3] else None
        check(lib.vs_norm_act_bwd_finish(sums.data_ptr(), n, c, ctx.c_real, float(voxels), ctx.mode, tab[1].data_ptr(), _p(gamma), coef.data_ptr(),
                                         _p(dgamma), _p(dbeta), st), "norm_act_bwd_finish")
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            check(lib.vs_norm_act_bwd_apply(g.data_ptr(), x.data_ptr(), tab[0].data_ptr(), tab[1].data_ptr(), _p(gamma), _p(beta), coef.data_ptr(),
                                            dx.data_ptr(), n, voxels, c, ctx.c_real, ctx.act, dt, st), "norm_act_bwd_apply")
        return dx, None, dgamma, dbeta, None, None, None


class GSNorm(torch.autograd.Function):
    """GSNorm3d (joint_model.py:17-33) on a channels-last tensor: every channel divided by the sum over its group (+1e-4)"""

    @staticmethod
    def forward(ctx, x, num_group):
        _require_cuda(x)
        c = x.shape[-1]
        y = torch.empty_like(x)
        check(lib.vs_gsnorm_fwd(x.data_ptr(), y.data_ptr(), x.numel() // c, c, num_group, vs_dtype(x), _stream()), "gsnorm_fwd")
        ctx.save_for_backward(x)
        ctx.num_group = num_group
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = _contig(g)
        c = x.shape[-1]
        dx = torch.empty_like(x)
        check(lib.vs_gsnorm_bwd(g.data_ptr(), x.data_ptr(), dx.data_ptr(), x.numel() // c, c, ctx.num_group, vs_dtype(x), _stream()), "gsnorm_bwd")
        return dx, None


class UpsampleTrilinear(torch.autograd.Function):
    """torch.nn.Upsample(scale_factor=s, mode='trilinear') (joint_model.py:69,323-325) on a channels-last tensor"""

    @staticmethod
    def forward(ctx, x, scale):
        _require_cuda(x)
        n, d, h, w, c = x.shape
        y = torch.empty((n, d * scale, h * scale, w * scale, c), dtype=x.dtype, device=x.device)
        check(lib.vs_upsample_trilinear_fwd(x.data_ptr(), y.data_ptr(), n, d, h, w, c, scale, vs_dtype(x), _stream()), "upsample_trilinear_fwd")
        ctx.shape, ctx.scale = (n, d, h, w, c), scale
        return y

    @staticmethod
    def backward(ctx, g):
        g = _contig(g)
        n, d, h, w, c = ctx.shape
        dx = torch.empty(ctx.shape, dtype=g.dtype, device=g.device)
        scratch = torch.empty((n * d * h * w * c + 3) // 4 * 4, dtype=torch.float32, device=g.device)
        check(lib.vs_upsample_trilinear_bwd(g.data_ptr(), dx.data_ptr(), scratch.data_ptr(), n, d, h, w, c, ctx.scale, vs_dtype(g), _stream()),
              "upsample_trilinear_bwd")
        return dx, None


class Softmax2(torch.autograd.Function):
    """nn.Softmax(dim=1) as its own pass: channels-last logits (channels 0..n_class-1) -> planar fp32 (N, n_class, D, H, W); n_class 1..8"""

    @staticmethod
    def forward(ctx, x, n_class=2):
        _require_cuda(x)
        n, d, h, w, c = x.shape
        prob = torch.empty((n, n_class, d, h, w), dtype=torch.float32, device=x.device)
        if n_class == 2:
            check(lib.vs_softmax2_fwd(x.data_ptr(), prob.data_ptr(), n, d * h * w, c, vs_dtype(x), _stream()), "softmax2_fwd")
        else:
            check(lib.vs_softmax_cl_fwd(x.data_ptr(), prob.data_ptr(), n, d * h * w, c, n_class, vs_dtype(x), 0.0, 0, _stream()), "softmax_cl_fwd")
        ctx.save_for_backward(prob)
        ctx.c, ctx.dtype = c, x.dtype
        return prob

    @staticmethod
    def backward(ctx, gprob):
        (prob,) = ctx.saved_tensors
        gprob = _contig(gprob.float())
        n, nc, d, h, w = prob.shape
        g = torch.empty((n, d, h, w, ctx.c), dtype=ctx.dtype, device=prob.device)
        if nc == 2:
            check(lib.vs_softmax2_bwd(prob.data_ptr(), gprob.data_ptr(), g.data_ptr(), n, d * h * w, ctx.c, vs_of(ctx.dtype), _stream()), "softmax2_bwd")
        else:
            check(lib.vs_softmax_cl_bwd(prob.data_ptr(), gprob.data_ptr(), g.data_ptr(), n, d * h * w, ctx.c, nc, vs_of(ctx.dtype), 0.0, 0, _stream()),
                  "softmax_cl_bwd")
        return g, None


_DROPOUT_CALLS = [0]


def next_dropout_seed():
    """A fresh 64-bit seed per dropout site per call, a pure function of torch's seed and a call counter (host side: no
    device sync).  Under HIP-graph replay the captured seeds would repeat, so drawing one during capture raises; TestTimeFinetune
    runs models with dropout > 0 eagerly."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("dropout > 0 inside HIP-graph capture: the host-side mask seed would be baked into the graph and every replay "
                           "would reuse the same masks (the reference draws fresh ones per call) — run this model eagerly (graph=False)")
    _DROPOUT_CALLS[0] += 1
    return (torch.initial_seed() * 0x9E3779B97F4A7C15 + _DROPOUT_CALLS[0] * 0xD1B54A32D192ED03) % (1 << 64)


def dropout_mask(count, p, seed, device="cuda"):
    """The multipliers (0 or 1/(1-p)) a dropout site with this (p, seed) applies, in the site tensor's memory order (vs_dropout_mask)."""
    mask = torch.empty(count, dtype=torch.float32, device=device)
    check(lib.vs_dropout_mask(mask.data_ptr(), count, float(p), seed, _stream()), "dropout_mask")
    return mask


class Dropout(torch.autograd.Function):
    """F.dropout(x, p, training=True) on a final channels-last activation (joint_model.py:256-264,379-385)."""

    @staticmethod
    def forward(ctx, x, p, seed):
        _require_cuda(x)
        x = _contig(x)
        out = torch.empty_like(x)
        check(lib.vs_dropout(x.data_ptr(), out.data_ptr(), x.numel(), float(p), seed, vs_dtype(x), _stream()), "dropout")
        ctx.cfg = (float(p), seed)
        return out

    @staticmethod
    def backward(ctx, g):
        p, seed = ctx.cfg
        g = _contig(g)
        out = torch.empty_like(g)
        check(lib.vs_dropout(g.data_ptr(), out.data_ptr(), g.numel(), p, seed, vs_dtype(g), _stream()), "dropout")
        return out, None, None


class PackPlanar(torch.autograd.Function):
    """planar fp32 (N, C, D, H, W) -> channels-last (N, D, H, W, 8) in the kernel dtype (zero padded)."""

    @staticmethod
    def forward(ctx, x, dtype):
        _require_cuda(x)
        x = _contig(x.float())
        n, c, d, h, w = x.shape
        out = torch.empty((n, d, h, w, cpad(c)), dtype=dtype, device=x.device)
        check(lib.vs_pack_planar(x.data_ptr(), out.data_ptr(), n, d * h * w, c, cpad(c), vs_dtype(out), _stream()),
              "pack_planar")
        ctx.c = c
        return out

    @staticmethod
    def backward(ctx, g):
        g = _contig(g)
        n, d, h, w, cp = g.shape
        out = torch.empty((n, ctx.c, d, h, w), dtype=torch.float32, device=g.device)
        check(lib.vs_unpack_planar(g.data_ptr(), out.data_ptr(), n, d * h * w, ctx.c, cp, vs_dtype(g), _stream()),
              "unpack_planar")
        return out, None


class UnpackPlanar(torch.autograd.Function):
    """channels-last (N, D, H, W, Cp) -> planar fp32 (N, C, D, H, W), C <= Cp."""

    @staticmethod
    def forward(ctx, x, c):
        _require_cuda(x)
        x = _contig(x)
        n, d, h, w, cp = x.shape
        out = torch.empty((n, c, d, h, w), dtype=torch.float32, device=x.device)
        check(lib.vs_unpack_planar(x.data_ptr(), out.data_ptr(), n, d * h * w, c, cp, vs_dtype(x), _stream()), "unpack_planar")
        ctx.meta = (cp, x.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        cp, dtype = ctx.meta
        g = _contig(g.float())
        n, c, d, h, w = g.shape
        out = torch.empty((n, d, h, w, cp), dtype=dtype, device=g.device)
        check(lib.vs_pack_planar(g.data_ptr(), out.data_ptr(), n, d * h * w, c, cp, vs_dtype(out), _stream()), "pack_planar")
        return out, None


class LinearCL(torch.autograd.Function):
    """y = act(W x + b) where x is a channels-last activation read in the reference's NCDHW flatten order
    (joint_model.py:241-243).  y is fp32 (B, J)."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        _require_cuda(x, weight)
        n, d, h, w, c = x.shape
        k_in, j_out = c * d * h * w, weight.shape[0]
        y = torch.empty((n, j_out), dtype=torch.float32, device=x.device)
        ctx.cl = (not weight.requires_grad) and d * h * w > 1       # frozen: contiguous channels-last copy of the weight, no permutation
        wt = frozen_linear_layout(weight, "cols_cl", c, d * h * w) if ctx.cl else weight
        check(lib.vs_linear_fwd(x.data_ptr(), vs_dtype(x), wt.data_ptr(), _p(bias), y.data_ptr(), n, k_in, j_out, 0 if ctx.cl else c,
                                0 if ctx.cl else d * h * w, 1 if relu else 0, _stream()), "linear_fwd")
        ctx.save_for_backward(x, weight, y if relu else None)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, yrelu = ctx.saved_tensors
        gy = _contig(gy.float())
        n, d, h, w, c = x.shape
        k_in, j_out = c * d * h * w, weight.shape[0]
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gw = torch.empty_like(weight) if ctx.needs_input_grad[1] else None
        gb = torch.empty(j_out, dtype=torch.float32, device=x.device) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        cl = ctx.cl and gw is None
        wt = frozen_linear_layout(weight, "cols_cl", c, d * h * w) if cl else weight
        check(lib.vs_linear_bwd(x.data_ptr(), vs_dtype(x), wt.data_ptr(), gy.data_ptr(), _p(yrelu), _p(gx), _p(gw),
                                _p(gb), n, k_in, j_out, 0 if cl else c, 0 if cl else d * h * w, _stream()), "linear_bwd")
        return gx, gw, gb, None


class LinearCLPair(torch.autograd.Function):
    """(act1(W1 x + b1), act2(W2 x + b2)) for two layers of equal shape on the same channels-last input — fc_mean and fc_std
    (joint_model.py:241-243) — in one forward launch; the backward runs LinearCL's kernels for the outputs that received a gradient."""

    @staticmethod
    def forward(ctx, x, w1, b1, relu1, w2, b2, relu2):
        _require_cuda(x, w1, w2)
        if w1.shape != w2.shape:
            raise ValueError("LinearCLPair needs two layers of the same shape")
        n, d, h, w, c = x.shape
        k_in, j_out = c * d * h * w, w1.shape[0]
        y1 = torch.empty((n, j_out), dtype=torch.float32, device=x.device)
        y2 = torch.empty((n, j_out), dtype=torch.float32, device=x.device)
        ctx.cl = (not w1.requires_grad) and (not w2.requires_grad) and d * h * w > 1
        wa = frozen_linear_layout(w1, "cols_cl", c, d * h * w) if ctx.cl else w1
        wb = frozen_linear_layout(w2, "cols_cl", c, d * h * w) if ctx.cl else w2
        check(lib.vs_linear_fwd_pair(x.data_ptr(), vs_dtype(x), wa.data_ptr(), _p(b1), y1.data_ptr(), 1 if relu1 else 0, wb.data_ptr(), _p(b2),
                                     y2.data_ptr(), 1 if relu2 else 0, n, k_in, j_out, 0 if ctx.cl else c, 0 if ctx.cl else d * h * w, _stream()),
              "linear_fwd_pair")
        ctx.save_for_backward(x, w1, w2, y1 if relu1 else None, y2 if relu2 else None)
        ctx.has_bias = (b1 is not None, b2 is not None)
        ctx.set_materialize_grads(False)
        return y1, y2

    @staticmethod
    def backward(ctx, g1, g2):
        x, w1, w2, r1, r2 = ctx.saved_tensors
        n, d, h, w, c = x.shape
        k_in, j_out = c * d * h * w, w1.shape[0]
        out = [None] * 7
        gx_total = None
        for gy, wt, yrelu, iw, ib, hb in ((g1, w1, r1, 1, 2, ctx.has_bias[0]), (g2, w2, r2, 4, 5, ctx.has_bias[1])):
            if gy is None:
                continue
            gy = _contig(gy.float())
            gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            gw = torch.empty_like(wt) if ctx.needs_input_grad[iw] else None
            gb = torch.empty(j_out, dtype=torch.float32, device=x.device) if (hb and ctx.needs_input_grad[ib]) else None
            cl = ctx.cl and gw is None
            wuse = frozen_linear_layout(wt, "cols_cl", c, d * h * w) if cl else wt
            check(lib.vs_linear_bwd(x.data_ptr(), vs_dtype(x), wuse.data_ptr(), gy.data_ptr(), _p(yrelu), _p(gx), _p(gw), _p(gb), n, k_in,
                                    j_out, 0 if cl else c, 0 if cl else d * h * w, _stream()), "linear_bwd")
            out[iw], out[ib] = gw, gb
            if gx is not None:
                gx_total = gx if gx_total is None else gx_total + gx
        out[0] = gx_total
        return tuple(out)


class LinearToCL(torch.autograd.Function):
    """fc2 (joint_model.py:248-253): fp32 latent (B, K) -> channels-last activation (B, s, s, s, C) holding
    view(B, C, s, s, s) of the reference's output."""

    @staticmethod
    def forward(ctx, z, weight, bias, c, side, dtype):
        _require_cuda(z, weight)
        z = _contig(z.float())
        b, k_in = z.shape
        j_out = weight.shape[0]
        y = torch.empty((b, side, side, side, c), dtype=dtype, device=z.device)
        check(lib.vs_linear_fwd_perm_out(z.data_ptr(), weight.data_ptr(), _p(bias), y.data_ptr(), vs_dtype(y), b, k_in,
                                         j_out, c, side ** 3, _stream()), "linear_fwd_perm_out")
        ctx.save_for_backward(z, weight)
        ctx.has_bias = bias is not None
        ctx.geom = (c, side)
        return y

    @staticmethod
    def backward(ctx, gy):
        z, weight = ctx.saved_tensors
        gy = _contig(gy)
        c, side = ctx.geom
        b, k_in = z.shape
        j_out = weight.shape[0]
        gz = torch.empty_like(z) if ctx.needs_input_grad[0] else None
        gw = torch.empty_like(weight) if ctx.needs_input_grad[1] else None
        gb = torch.empty(j_out, dtype=torch.float32, device=z.device) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        if gz is not None and gw is None and gb is None and not weight.requires_grad and side > 1:
            # frozen fc2: gz[b][k] = sum_ph W2T[k][ph] * gy[b][ph] with the transposed, channels-last-ordered copy — the plain GEMV kernel,
            # every access contiguous (the permuting kernel walks a weight column with a 512-byte stride)
            wt = frozen_linear_layout(weight, "rows_cl_t", c, side ** 3)
            check(lib.vs_linear_fwd(gy.data_ptr(), vs_dtype(gy), wt.data_ptr(), None, gz.data_ptr(), b, j_out, k_in, 0, 0, 0, _stream()),
                  "linear_fwd (fc2 backward)")
            return gz, None, None, None, None, None
        check(lib.vs_linear_perm_out_bwd(z.data_ptr(), weight.data_ptr(), gy.data_ptr(), vs_dtype(gy), _p(gz), _p(gw),
                                         _p(gb), b, k_in, j_out, c, side ** 3, _stream()), "linear_perm_out_bwd")
        return gz, gw, gb, None, None, None


class Reparam(torch.autograd.Function):
    """z = mean + noise * std * scale (joint_model.py:248)."""

    @staticmethod
    def forward(ctx, mean, std, noise, scale):
        _require_cuda(mean, std, noise)
        z = torch.empty_like(mean)
        check(lib.vs_reparam_fwd(mean.data_ptr(), std.data_ptr(), noise.data_ptr(), float(scale), z.data_ptr(),
                                 mean.numel(), _stream()), "reparam_fwd")
        ctx.save_for_backward(noise)
        ctx.scale = float(scale)
        return z

    @staticmethod
    def backward(ctx, gz):
        (noise,) = ctx.saved_tensors
        gz = _contig(gz)
        gm = torch.empty_like(gz) if ctx.needs_input_grad[0] else None
        gs = torch.empty_like(gz) if ctx.needs_input_grad[1] else None
        check(lib.vs_reparam_bwd(gz.data_ptr(), noise.data_ptr(), ctx.scale, _p(gm), _p(gs), gz.numel(), _stream()),
              "reparam_bwd")
        return gm, gs, None, None


_U64 = 2 ** 64 - 1


def latent_normal(shape, seed, draw):
    """draw `draw` of the latent stream `seed`, fp32 on the device, shape (B, dim) (or any shape: element i is the i-th of the flattened tensor):
    pair q = i >> 1 from Philox4x32-10 under key `seed` and counter (q, draw low, 0x200, draw high), Box-Muller in fp64 as ops.philox_normal forms it,
    even i the cosine, odd i the sine, rounded to fp32 once (vs_latent_normal_philox) — the noise ReparamPhilox draws when its stream says (seed, draw)"""
    shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    if not shape or min(shape) < 1:
        raise ValueError("latent_normal: a shape of positive sizes, got %r" % (shape,))
    out = torch.empty(shape, dtype=torch.float32, device="cuda")
    check(lib.vs_latent_normal_philox(out.data_ptr(), out.numel(), int(seed) & _U64, int(draw) & _U64, _stream()), "latent_normal_philox")
    return out


class LatentStream:
    """The (seed, draw) of a latent noise stream, two unsigned 64-bit words in DEVICE memory: ReparamPhilox reads them in its forward launch and advances
    `draw` by one behind it, so a captured step draws a fresh, stated sample on every replay — the same bits an eager step draws at that state."""

    def __init__(self, seed, draw=0, device="cuda"):
        self.words = torch.zeros(2, dtype=torch.int64, device=device)       # the two words' bits (torch has no arithmetic on uint64; none is needed)
        self.set(seed, draw)

    def set(self, seed, draw=0):
        signed = [v - 2 ** 64 if v >= 2 ** 63 else v for v in (int(seed) & _U64, int(draw) & _U64)]
        self.words.copy_(torch.tensor(signed, dtype=torch.int64))

    def state(self):
        """(seed, draw) on the host: a read-back that synchronises — for tests and for a caller that wants to store the stream, never in a step
        (driver.save_checkpoint keeps the reference's three-key layout and does not store it: a resumed run starts its stream at draw 0 again)"""
        seed, draw = (int(v) & _U64 for v in self.words.tolist())
        return seed, draw


class ReparamPhilox(torch.autograd.Function):
    """z = mean + noise * std * scale with the noise drawn in the launch from the LatentStream's device-resident (seed, draw); the stream advances by one
    draw behind the forward.  -> (z, noise): the noise is saved for the backward (ops.Reparam's) and returned for whoever wants to see it."""

    @staticmethod
    def forward(ctx, mean, std, stream, scale):
        _require_cuda(mean, std, stream.words)
        if mean.dtype != torch.float32 or std.dtype != torch.float32 or not (mean.is_contiguous() and std.is_contiguous()) or mean.shape != std.shape:
            raise TypeError("ReparamPhilox: mean and std are contiguous float32 tensors of one shape")
        z, noise = torch.empty_like(mean), torch.empty_like(mean)
        check(lib.vs_reparam_philox_fwd(mean.data_ptr(), std.data_ptr(), stream.words.data_ptr(), float(scale), z.data_ptr(), noise.data_ptr(),
                                        mean.numel(), _stream()), "reparam_philox_fwd")
        check(lib.vs_latent_advance(stream.words.data_ptr(), _stream()), "latent_advance")
        ctx.save_for_backward(noise)
        ctx.mark_non_differentiable(noise)
        ctx.scale = float(scale)
        return z, noise

    @staticmethod
    def backward(ctx, gz, _gnoise):
        (noise,) = ctx.saved_tensors
        gz = _contig(gz)
        gm = torch.empty_like(gz) if ctx.needs_input_grad[0] else None
        gs = torch.empty_like(gz) if ctx.needs_input_grad[1] else None
        check(lib.vs_reparam_bwd(gz.data_ptr(), noise.data_ptr(), ctx.scale, _p(gm), _p(gs), gz.numel(), _stream()),
              "reparam_bwd")
        return gm, gs, None, None


class KL(torch.autograd.Function):
    """utils/evaluation.py:42-45."""

    @staticmethod
    def forward(ctx, mean, std):
        _require_cuda(mean, std)
        mean, std = _contig(mean.float()), _contig(std.float())
        out = torch.empty((), dtype=torch.float32, device=mean.device)
        check(lib.vs_kl_fwd(mean.data_ptr(), std.data_ptr(), out.data_ptr(), mean.shape[0], mean.shape[1], _stream()), "kl_fwd")
        ctx.save_for_backward(mean, std)
        return out

    @staticmethod
    def backward(ctx, g):
        mean, std = ctx.saved_tensors
        g = _contig(g.float())
        gm = torch.empty_like(mean) if ctx.needs_input_grad[0] else None
        gs = torch.empty_like(std) if ctx.needs_input_grad[1] else None
        check(lib.vs_kl_bwd(mean.data_ptr(), std.data_ptr(), g.data_ptr(), _p(gm), _p(gs), mean.shape[0], mean.shape[1],
                            _stream()), "kl_bwd")
        return gm, gs


def _pad_quads(x, b, c, value):
    """The Dice kernels read whole 16-byte quads of a plane.  A contiguous (b, c, ...) tensor whose planes hold a multiple of 4 voxels is returned as it
    is; any other is flattened to (b, c, V) and padded to the next multiple of 4 with `value` — 0 for a source or a tensor target (it adds nothing to
    I, S or T), -1 for a label volume (it matches no class)."""
    voxels = x.numel() // (b * c)
    if voxels % 4 == 0:
        return x
    return torch.nn.functional.pad(x.reshape(b, c, voxels), (0, (-voxels) % 4), value=value)


def _unpad_quads(g, shape):
    """the gradient of a tensor that _pad_quads padded, in the caller's shape (the padding's gradient is dropped)"""
    if g is None or tuple(g.shape) == tuple(shape):
        return g
    voxels = 1
    for d in shape[2:]:
        voxels *= d
    return g[:, :, :voxels].reshape(shape)


class Dice(torch.autograd.Function):
    """Soft Dice over channels [bot, top) of two planar fp32 (B, C, D, H, W) tensors; any voxel count (_pad_quads).
    return_mean=True -> scalar mean over (b, c); False -> per-sample (B,) means (utils/evaluation.py:68-79)."""

    @staticmethod
    def forward(ctx, s, t, bot, top, eps, return_mean):
        _require_cuda(s, t)
        s, t = _contig(s.float()), _contig(t.float())
        b, c = s.shape[0], s.shape[1]
        ctx.shape = tuple(s.shape)
        s, t = _pad_quads(s, b, c, 0.0), _pad_quads(t, b, c, 0.0)
        voxels = s.numel() // (b * c)
        sums = torch.empty((b, c, 3), dtype=torch.float64, device=s.device)
        per = torch.empty(b, dtype=torch.float32, device=s.device)
        mean = torch.empty((), dtype=torch.float32, device=s.device)
        check(lib.vs_dice_fwd(s.data_ptr(), t.data_ptr(), sums.data_ptr(), per.data_ptr(), mean.data_ptr(), b, c, voxels,
                              bot, top, float(eps), _stream()), "dice_fwd")
        ctx.save_for_backward(s, t, sums)
        ctx.cfg = (bot, top, float(eps), bool(return_mean))
        return mean if return_mean else per

    @staticmethod
    def backward(ctx, g):
        s, t, sums = ctx.saved_tensors
        bot, top, eps, return_mean = ctx.cfg
        g = _contig(g.float())
        b, c = s.shape[0], s.shape[1]
        voxels = s.numel() // (b * c)
        gs = torch.empty_like(s) if ctx.needs_input_grad[0] else None
        gt = torch.empty_like(t) if ctx.needs_input_grad[1] else None
        if gs is not None or gt is not None:
            check(lib.vs_dice_bwd(s.data_ptr(), t.data_ptr(), sums.data_ptr(), g.data_ptr(), 1 if return_mean else 0,
                                  _p(gs), _p(gt), b, c, voxels, bot, top, eps, _stream()), "dice_bwd")
        return _unpad_quads(gs, ctx.shape), _unpad_quads(gt, ctx.shape), None, None, None, None


class LabelTarget:
    """A Dice target given as its LABEL volume (B,1,D,H,W; values 0..n_class-1): dice_loss_sum evaluates the one-hot (main_source.py:449-451) on
    the fly inside the loss kernels, so the one-hot tensor is neither written nor read (vs_dice_loss_multi_labels_*)."""

    def __init__(self, label):
        _require_cuda(label)
        self.label = _contig(label.float())


class DiceLossSum(torch.autograd.Function):
    """final = sum_j w[j] * (1 - avg_dsc(s, t_j))  — the loss line of every train method (main_source.py:469-471,
    main_target.py:588-592) — in TWO forward launches (per-block partials, finish) and ONE backward launch: the source is read once
    for all targets, no atomics, fixed summation order (the unfused spelling costs ~18 launches of 4.7 us for two terms).  -> (final, terms[k]); terms are the individual (1 - Dice) values, not differentiable."""

    @staticmethod
    def forward(ctx, s, bot, top, eps, weights, *targets):
        # weights: one number per target, or (number, True) for a target that is a LABEL volume (LabelTarget: one-hot on the fly)
        is_lab = [isinstance(w, tuple) and bool(w[1]) for w in weights]
        weights = [w[0] if isinstance(w, tuple) else w for w in weights]
        _require_cuda(s, *targets)
        k = len(targets)
        s = _contig(s.float())
        ts = [_contig(t.float()) for t in targets]
        b, c = s.shape[0], s.shape[1]
        voxels = s.numel() // (b * c)
        for t, lab in zip(ts, is_lab):
            if lab and t.numel() != b * voxels:
                raise ValueError("label target: expected %d x %d labels, got %s" % (b, voxels, tuple(t.shape)))
        ctx.shapes = [tuple(s.shape)] + [tuple(t.shape) for t in ts]
        s = _pad_quads(s, b, c, 0.0)
        ts = [_pad_quads(t, b, 1, -1.0) if lab else _pad_quads(t, b, c, 0.0) for t, lab in zip(ts, is_lab)]
        voxels = s.numel() // (b * c)
        scratch = torch.empty(lib.vs_dice_loss_multi_scratch_doubles(k, b, c), dtype=torch.float64, device=s.device)
        terms = torch.empty(k, dtype=torch.float32, device=s.device)
        final = torch.empty((), dtype=torch.float32, device=s.device)
        tp = (_ct.c_void_p * k)(*[None if lab else t.data_ptr() for t, lab in zip(ts, is_lab)])
        lp = (_ct.c_void_p * k)(*[t.data_ptr() if lab else None for t, lab in zip(ts, is_lab)])
        wp = (_ct.c_float * k)(*[float(w) for w in weights])
        check(lib.vs_dice_loss_multi_labels_fwd(s.data_ptr(), _ct.addressof(tp), _ct.addressof(lp), _ct.addressof(wp), k, scratch.data_ptr(),
                                                terms.data_ptr(), final.data_ptr(), b, c, voxels, bot, top, float(eps), _stream()), "dice_loss_multi_fwd")
        ctx.save_for_backward(s, scratch, *ts)
        ctx.cfg = (bot, top, float(eps), [float(w) for w in weights], is_lab)
        ctx.mark_non_differentiable(terms)
        ctx.set_materialize_grads(False)      # no zero-fill launch for the terms' gradient
        return final, terms

    @staticmethod
    def backward(ctx, g, _gterms):
        s, scratch = ctx.saved_tensors[:2]
        ts = ctx.saved_tensors[2:]
        bot, top, eps, weights, is_lab = ctx.cfg
        if g is None:
            return (None,) * (5 + len(ts))
        k = len(ts)
        b, c = s.shape[0], s.shape[1]
        voxels = s.numel() // (b * c)
        g = _contig(g.float())
        gs = torch.empty_like(s) if ctx.needs_input_grad[0] else None
        gts = [torch.empty_like(t) if ctx.needs_input_grad[5 + j] and not is_lab[j] else None for j, t in enumerate(ts)]
        if gs is not None or any(x is not None for x in gts):
            tp = (_ct.c_void_p * k)(*[None if lab else t.data_ptr() for t, lab in zip(ts, is_lab)])
            lp = (_ct.c_void_p * k)(*[t.data_ptr() if lab else None for t, lab in zip(ts, is_lab)])
            gp = (_ct.c_void_p * k)(*[_p(x) for x in gts])
            wp = (_ct.c_float * k)(*weights)
            check(lib.vs_dice_loss_multi_labels_bwd(s.data_ptr(), _ct.addressof(tp), _ct.addressof(lp), _ct.addressof(wp), k, scratch.data_ptr(),
                                                    g.data_ptr(), _p(gs), _ct.addressof(gp), b, c, voxels, bot, top, eps, _stream()), "dice_loss_multi_bwd")
        return (_unpad_quads(gs, ctx.shapes[0]), None, None, None, None) + tuple(_unpad_quads(x, sh) for x, sh in zip(gts, ctx.shapes[1:]))


FUSED_LOSS = [os.environ.get("VS_FUSED_LOSS", "1") != "0"]


def dice_loss_sum(source, targets_and_weights, botindex=0, topindex=2, eps=1e-6):
    """sum_j w_j * (1 - avg_dsc(source, target_j, botindex, topindex)) -> (final, [1 - Dice_j ...]); channel selection as
    utils/evaluation.py:66-70.  VS_FUSED_LOSS=0 spells it with Dice.apply and torch scalar arithmetic, as the reference does."""
    channels = source.shape[1]
    bot, top = (botindex, min(topindex, channels)) if channels > 1 else (0, 1)
    if not FUSED_LOSS[0] or len(targets_and_weights) > 4:
        targets_and_weights = [(onehot(t.label, channels) if isinstance(t, LabelTarget) else t, w) for t, w in targets_and_weights]
        terms = [1 - Dice.apply(source, t, bot, top, eps, True) for t, _ in targets_and_weights]
        final = None
        for term, (_, w) in zip(terms, targets_and_weights):
            part = term if w == 1 else w * term
            final = part if final is None else final + part
        return final, terms
    final, terms = DiceLossSum.apply(source, bot, top, eps, [(w, isinstance(t, LabelTarget)) for t, w in targets_and_weights],
                                     *[t.label if isinstance(t, LabelTarget) else t for t, _ in targets_and_weights])
    return final, list(terms.unbind(0))


class BCE(torch.autograd.Function):
    """nn.BCELoss() (mean) — utils/evaluation.py:29-39."""

    @staticmethod
    def forward(ctx, p, t):
        _require_cuda(p, t)
        p, t = _contig(p.float()), _contig(t.float())
        out = torch.empty((), dtype=torch.float32, device=p.device)
        scratch = torch.empty(1, dtype=torch.float64, device=p.device)
        check(lib.vs_bce_fwd(p.data_ptr(), t.data_ptr(), out.data_ptr(), scratch.data_ptr(), p.numel(), _stream()), "bce_fwd")
        ctx.save_for_backward(p, t)
        return out

    @staticmethod
    def backward(ctx, g):
        p, t = ctx.saved_tensors
        gp = torch.empty_like(p)
        g = _contig(g.float())
        check(lib.vs_bce_bwd(p.data_ptr(), t.data_ptr(), g.data_ptr(), gp.data_ptr(), p.numel(), _stream()), "bce_bwd")
        return gp, None


# ------------------------------------------------------------------------------------------------
# non-differentiable helpers
# ------------------------------------------------------------------------------------------------
def onehot(label, n_class=2):
    """(B,1,D,H,W) labels (any real dtype, values 0..n_class-1) -> planar fp32 one-hot (main_source.py:449-451)."""
    _require_cuda(label)
    lab = _contig(label.float())
    b = lab.shape[0]
    out = torch.empty((b, n_class) + tuple(lab.shape[2:]), dtype=torch.float32, device=lab.device)
    check(lib.vs_onehot(lab.data_ptr(), out.data_ptr(), b, lab.numel() // b, n_class, _stream()), "onehot")
    return out


def hard_onehot(mask):
    """(B,C,D,H,W) scores -> planar fp32 one-hot of the channel argmax (utils/evaluation.py:58-64), any C >= 1, one launch."""
    _require_cuda(mask)
    m = _contig(mask.detach().float())
    b, c = m.shape[0], m.shape[1]
    out = torch.empty_like(m)
    check(lib.vs_hard_onehot(m.data_ptr(), out.data_ptr(), b, c, m.numel() // (b * c), _stream()), "hard_onehot")
    return out


def binarize(a, mode=0, lo=0.2, hi=0.8):
    _require_cuda(a)
    a = _contig(a.detach().float())
    out = torch.empty_like(a)
    check(lib.vs_binarize(a.data_ptr(), out.data_ptr(), a.numel(), mode, float(lo), float(hi), _stream()), "binarize")
    return out


# connected components (csrc/cc.hip).  Workspaces are cached per (shape, connectivity, device) and never freed or moved — as the packed
# weights are — so a captured graph that holds one stays valid.  Calls that share a workspace must be ordered on one stream.
_CC_WORKSPACES = {}


def cc_max_components(d, h, w, connectivity=26):
    """rows per plane of the size table (include/vaeseg.h): the most components a (d, h, w) plane can hold"""
    if connectivity == 26:
        return ((d + 1) // 2) * ((h + 1) // 2) * ((w + 1) // 2)
    return (d * h * w + 1) // 2


def _cc_prepare(mask, connectivity):
    _require_cuda(mask)
    if mask.requires_grad:
        raise RuntimeError("connected-component labelling is forward only: detach the input")
    if mask.dim() != 5:
        raise ValueError("expected a planar (N, C, D, H, W) tensor, got shape %s" % (tuple(mask.shape),))
    m = _contig(mask.float())
    if m.data_ptr() % 16:
        m = m.clone()
    n, c, d, h, w = m.shape
    key = (n, c, d, h, w, int(connectivity), m.device)
    ws = _CC_WORKSPACES.get(key)
    if ws is None:
        nbytes = lib.vs_cc_workspace_bytes(n, c, d, h, w, int(connectivity))
        check(min(nbytes, 0), "cc_workspace_bytes")
        ws = _CC_WORKSPACES[key] = torch.empty(nbytes, dtype=torch.uint8, device=m.device)
    return m, ws


def cc_label(mask, connectivity=26):
    """Connected components of every (n, c) plane of a planar (N, C, D, H, W) mask (foreground: value >= 0.5) — utils/utils.py:20-57.
    -> labels int32 (N, C, D, H, W): 0 background, 1..K in the order of each component's first voxel in raster order (scipy.ndimage.label's
    numbering); counts int32 (N, C) = K; sizes int32 (N, C, cc_max_components(D, H, W, connectivity)): sizes[..., label - 1] voxels, 0 beyond K."""
    m, ws = _cc_prepare(mask, connectivity)
    n, c, d, h, w = m.shape
    labels = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    counts = torch.empty((n, c), dtype=torch.int32, device=m.device)
    check(lib.vs_cc_label(m.data_ptr(), labels.data_ptr(), counts.data_ptr(), n, c, d, h, w, int(connectivity), ws.data_ptr(), _stream()), "cc_label")
    maxk = cc_max_components(d, h, w, connectivity)
    sizes = ws[:n * c * maxk * 4].view(torch.int32).view(n, c, maxk).clone()       # the table sits at the start of the workspace
    return labels, counts, sizes


def keep_largest(mask, k=1, min_size=0, connectivity=26, lo_channel=0, to_background=False):
    """utils/utils.py:776-796 (predict_vol step 2) per (n, c) plane: 1.0 on the k largest components that hold at least min_size voxels (equal
    sizes: the one whose first voxel comes first), 0.0 elsewhere.  Channels below lo_channel are copied; with to_background (and lo_channel >= 1)
    channel 0 gains every removed voxel, so a one-hot tensor stays one-hot."""
    m, ws = _cc_prepare(mask, connectivity)
    n, c, d, h, w = m.shape
    out = torch.empty_like(m)
    check(lib.vs_cc_keep_largest(m.data_ptr(), out.data_ptr(), n, c, d, h, w, int(connectivity), int(k), int(min(max(min_size, 0), 2 ** 31 - 1)),
                                 int(lo_channel), int(bool(to_background)), ws.data_ptr(), _stream()), "cc_keep_largest")
    return out


# surface distances (csrc/surface.hip).  The workspace of surface_distances is cached per (shape, path, device) like the CC one.
_EDT_WORKSPACES = {}
SURFACE_RECORD_FIELDS = ("count_ab", "count_ba", "sum_ab", "sum_ba", "max_sq", "lo_sq", "hi_sq", "assd", "hd", "hd95")      # vs_surface_record


def _spacing_array(spacing):
    """None, or the (sz, sy, sx) doubles the library reads on the host during the call"""
    if spacing is None:
        return None
    vals = [float(s) for s in spacing]
    if len(vals) != 3:
        raise ValueError("spacing is (sz, sy, sx), got %r" % (spacing,))
    return (_ctypes.c_double * 3)(*vals)


def _mask_prepare(mask, what):
    _require_cuda(mask)
    if mask.requires_grad:
        raise RuntimeError("%s is forward only: detach the input" % what)
    if mask.dim() != 5:
        raise ValueError("expected a planar (N, C, D, H, W) tensor, got shape %s" % (tuple(mask.shape),))
    m = _contig(mask.float())
    if m.data_ptr() % 16:
        m = m.clone()
    return m


def surface(mask, connectivity=6):
    """S(X) = X & ~binary_erosion(X) per (n, c) plane of a planar (N, C, D, H, W) mask (foreground: value >= 0.5): fp32, 1.0 on foreground voxels that have a
    background or out-of-volume neighbour among their 6 (default, medpy's) or 26 neighbours."""
    m = _mask_prepare(mask, "surface extraction")
    n, c, d, h, w = m.shape
    out = torch.empty_like(m)
    check(lib.vs_surface(m.data_ptr(), out.data_ptr(), n, c, d, h, w, int(connectivity), _stream()), "surface")
    return out


def edt(feature, spacing=None, squared=False):
    """Exact Euclidean distance of every voxel to the nearest voxel with feature >= 0.5, per (n, c) plane of a planar (N, C, D, H, W) tensor.
    spacing None and squared: int32 squared distances (2^31 - 1 in a plane without feature voxels).  Otherwise fp64 — squared or not — with
    spacing = (sz, sy, sx) or unit spacing; +inf in a plane without feature voxels."""
    m = _mask_prepare(feature, "the distance transform")
    n, c, d, h, w = m.shape
    sp = _spacing_array(spacing)
    out = torch.empty(m.shape, dtype=torch.int32 if sp is None else torch.float64, device=m.device)
    check(lib.vs_edt(m.data_ptr(), out.data_ptr(), n, c, d, h, w, sp, _stream()), "edt")
    if sp is None:
        if squared:
            return out
        sq = out.double()
        return torch.where(out == 2 ** 31 - 1, torch.full_like(sq, float("inf")), sq).sqrt_()
    return out if squared else out.sqrt_()


def surface_distances(pred, gt, spacing=None, connectivity=6):
    """The surface-distance record of every (n, c) plane (include/vaeseg.h vs_surface_record; A = pred, B = gt): a dict of (N, C) device tensors —
    count_ab, count_ba (int64), sum_ab, sum_ba, max_sq, lo_sq, hi_sq, assd, hd, hd95 (fp64).  A plane with an empty surface has counts 0 and NaN elsewhere."""
    a, b = _mask_prepare(pred, "surface distances"), _mask_prepare(gt, "surface distances")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("surface_distances: the two masks differ in shape or device: %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    n, c, d, h, w = a.shape
    sp = _spacing_array(spacing)
    key = (n, c, d, h, w, sp is not None, a.device)
    ws = _EDT_WORKSPACES.get(key)
    if ws is None:
        nbytes = lib.vs_edt_workspace_bytes(n, c, d, h, w, int(sp is not None))
        check(min(nbytes, 0), "edt_workspace_bytes")
        ws = _EDT_WORKSPACES[key] = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
    rec = torch.empty((n, c, len(SURFACE_RECORD_FIELDS)), dtype=torch.float64, device=a.device)
    check(lib.vs_surface_distances(a.data_ptr(), b.data_ptr(), rec.data_ptr(), n, c, d, h, w, int(connectivity), sp, ws.data_ptr(), _stream()),
          "surface_distances")
    out = {name: rec[..., i] for i, name in enumerate(SURFACE_RECORD_FIELDS)}
    counts = rec[..., :2].view(torch.int64)                     # the record's first two members are 64-bit integers
    out["count_ab"], out["count_ba"] = counts[..., 0], counts[..., 1]
    return out


# binary morphology and hole filling (csrc/morph.hip).  Workspaces are cached per (shape, connectivity, device) like the CC ones: never freed or moved.
MORPH_OPS = {"dilate": 0, "erode": 1, "open": 2, "close": 3}          # VS_MORPH_*
_MORPH_WORKSPACES = {}
_FILL_WORKSPACES = {}


def _check_connectivity(connectivity, what):
    if isinstance(connectivity, bool) or connectivity not in (6, 26):
        raise ValueError("%s: connectivity is 6 (generate_binary_structure(3, 1)) or 26 ((3, 3)), got %r" % (what, connectivity))
    return int(connectivity)


def _workspace(cache, key, query, what, device):
    ws = cache.get(key)
    if ws is None:
        nbytes = query()
        check(min(nbytes, 0), what)
        ws = cache[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    return ws


def morph(mask, op, iterations=1, connectivity=6, border_value=0):
    """scipy.ndimage.binary_dilation / binary_erosion / binary_opening / binary_closing (op "dilate" / "erode" / "open" / "close") per (n, c) plane of a
    planar (N, C, D, H, W) mask (foreground: value >= 0.5) -> fp32 0 / 1.  connectivity 6 is generate_binary_structure(3, 1), 26 is (3, 3); the
    structure is applied `iterations` >= 1 times (opening: erode^n then dilate^n, closing: dilate^n then erode^n); voxels outside the volume read as
    border_value (0 or 1) in both halves, as scipy passes it on.  Bit-packed on the device (csrc/morph.hip), no synchronisation."""
    if op not in MORPH_OPS:
        raise ValueError("morph: op is one of %s, got %r" % (sorted(MORPH_OPS), op))
    connectivity = _check_connectivity(connectivity, "morph")
    try:
        ok = not isinstance(iterations, bool) and int(iterations) == iterations and iterations >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("morph: iterations is an integer >= 1, got %r" % (iterations,))
    if isinstance(border_value, bool):
        border_value = int(border_value)
    if border_value not in (0, 1):
        raise ValueError("morph: border_value is 0 or 1, got %r" % (border_value,))
    m = _mask_prepare(mask, "binary morphology")
    n, c, d, h, w = m.shape
    ws = _workspace(_MORPH_WORKSPACES, (n, c, d, h, w, connectivity, m.device), lambda: lib.vs_morph_workspace_bytes(n, c, d, h, w),
                    "morph_workspace_bytes", m.device)
    out = torch.empty_like(m)
    check(lib.vs_morph(m.data_ptr(), out.data_ptr(), n, c, d, h, w, MORPH_OPS[op], connectivity, int(min(iterations, 2 ** 31 - 1)), int(border_value),
                       ws.data_ptr(), _stream()), "morph")
    return out


def binary_dilation(input, iterations=1, connectivity=6, border_value=0):
    """scipy.ndimage.binary_dilation(input, generate_binary_structure(3, 1 or 3), iterations, border_value=border_value) per plane (morph)"""
    return morph(input, "dilate", iterations=iterations, connectivity=connectivity, border_value=border_value)


def binary_erosion(input, iterations=1, connectivity=6, border_value=0):
    """scipy.ndimage.binary_erosion per plane (morph)"""
    return morph(input, "erode", iterations=iterations, connectivity=connectivity, border_value=border_value)


def binary_opening(input, iterations=1, connectivity=6, border_value=0):
    """scipy.ndimage.binary_opening per plane (morph)"""
    return morph(input, "open", iterations=iterations, connectivity=connectivity, border_value=border_value)


def binary_closing(input, iterations=1, connectivity=6, border_value=0):
    """scipy.ndimage.binary_closing per plane (morph)"""
    return morph(input, "close", iterations=iterations, connectivity=connectivity, border_value=border_value)


def fill_holes(mask, connectivity=6):
    """scipy.ndimage.binary_fill_holes(X, structure) per (n, c) plane of a planar (N, C, D, H, W) mask (foreground: value >= 0.5) -> fp32 0 / 1: the
    complement of the background voxels that reach the outside of the volume through `connectivity`-neighbours (6, scipy's default, or 26).
    The complement is labelled with the connected-component union-find on the device (csrc/morph.hip), no synchronisation."""
    connectivity = _check_connectivity(connectivity, "fill_holes")
    m = _mask_prepare(mask, "hole filling")
    n, c, d, h, w = m.shape
    ws = _workspace(_FILL_WORKSPACES, (n, c, d, h, w, connectivity, m.device), lambda: lib.vs_fill_holes_workspace_bytes(n, c, d, h, w, connectivity),
                    "fill_holes_workspace_bytes", m.device)
    out = torch.empty_like(m)
    check(lib.vs_fill_holes(m.data_ptr(), out.data_ptr(), n, c, d, h, w, connectivity, ws.data_ptr(), _stream()), "fill_holes")
    return out


# per-component measurements and contingency tables of label volumes (csrc/regions.hip).  No workspace: the outputs are the only buffers, and the
# kernels write their initial state themselves.
REGION_COLUMNS = ("count", "zmin", "ymin", "xmin", "zmax", "ymax", "xmax", "sum_z", "sum_y", "sum_x")      # vs_region_props
CONTINGENCY_MAX_CELLS = 1 << 22                                                                            # (rows_a + 1) * (rows_b + 1) per plane


def _rows(value, what, least):
    if isinstance(value, bool) or not isinstance(value, _numbers.Integral) or value < least or value > 2 ** 31 - 2:
        raise ValueError("%s is an integer >= %d, got %r" % (what, least, value))
    return int(value)


def _label_volume(t, what):
    """every check that needs no device; the tensor is used as it is — a label volume is never converted or copied behind the caller's back"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
        raise TypeError("%s: label volumes are int32 tensors (ops.cc_label's labels), got %s" % (what, getattr(t, "dtype", type(t))))
    if t.dim() != 5:
        raise ValueError("%s: expected a planar (N, C, D, H, W) label volume, got shape %s" % (what, tuple(t.shape)))
    if t.numel() == 0 or t.shape[2] * t.shape[3] * t.shape[4] >= 2 ** 31:
        raise ValueError("%s: an empty volume or a plane of 2^31 voxels or more, shape %s" % (what, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s: the label volume must be contiguous" % what)


def region_props(labels, max_components=4096):
    """Per-label measurements of every (n, c) plane of an int32 label volume (N, C, D, H, W) — 0 background, 1..K components, as ops.cc_label
    numbers them — for the labels 1..R, R = max_components; what scipy.ndimage.find_objects, np.bincount and center_of_mass give on the host.
    -> {"count": int64 (N, C, R) voxels; "bbox": int32 (N, C, R, 6) = (zmin, ymin, xmin, zmax, ymax, xmax), inclusive;
        "centroid": fp64 (N, C, R, 3) = (z, y, x) in voxels, sum / count; "sums": int64 (N, C, R, 3) the coordinate sums behind it;
        "overflow": int32 (N, C) voxels whose label is negative or above R — counted there and nowhere else}.
    A label that does not occur has count 0, box mins (D, H, W) and maxes -1, centroid NaN.  Two launches, no synchronisation."""
    r = _rows(max_components, "region_props: max_components", 1)
    _label_volume(labels, "region_props")
    _require_cuda(labels)
    n, c, d, h, w = labels.shape
    table = torch.empty((n, c, r, len(REGION_COLUMNS)), dtype=torch.int64, device=labels.device)
    overflow = torch.empty((n, c), dtype=torch.int32, device=labels.device)
    check(lib.vs_region_props(labels.data_ptr(), n, c, d, h, w, r, table.data_ptr(), overflow.data_ptr(), _stream()), "region_props")
    count, sums = table[..., 0], table[..., 7:10]
    return {"count": count, "bbox": table[..., 1:7].to(torch.int32), "centroid": sums.double() / count.double().unsqueeze(-1), "sums": sums,
            "overflow": overflow}


def contingency(a, b, rows_a, rows_b):
    """The contingency table of two int32 label volumes of one shape (N, C, D, H, W), per (n, c) plane:
    -> table int64 (N, C, rows_a + 1, rows_b + 1), table[..., i, j] = voxels with a == i and b == j (row / column 0: background), and
    overflow int32 (N, C): voxels with a label outside [0, rows_a] / [0, rows_b] on either side — counted there and in no cell.
    (rows_a + 1) * (rows_b + 1) <= 2^22.  Two launches, no synchronisation; np.bincount(a * (rows_b + 1) + b) without the host."""
    ra, rb = _rows(rows_a, "contingency: rows_a", 0), _rows(rows_b, "contingency: rows_b", 0)
    if (ra + 1) * (rb + 1) > CONTINGENCY_MAX_CELLS:
        raise ValueError("contingency: (rows_a + 1) * (rows_b + 1) = %d cells per plane, at most 2^22" % ((ra + 1) * (rb + 1)))
    _label_volume(a, "contingency")
    _label_volume(b, "contingency")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("contingency: the two label volumes differ in shape or device: %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    _require_cuda(a, b)
    n, c, d, h, w = a.shape
    table = torch.empty((n, c, ra + 1, rb + 1), dtype=torch.int64, device=a.device)
    overflow = torch.empty((n, c), dtype=torch.int32, device=a.device)
    check(lib.vs_contingency(a.data_ptr(), b.data_ptr(), n, c, d, h, w, ra, rb, table.data_ptr(), overflow.data_ptr(), _stream()), "contingency")
    return table, overflow


# intensity histograms, joint histograms and mutual information (csrc/hist.hip).  The outputs are the only buffers of the histogram calls; the kernels
# write their initial state themselves.
HISTOGRAM_MAX_BINS = 4096                      # vs_histogram
HISTOGRAM_MAX_CELLS = 1 << 22                  # (rows + 1) * bins, bins_x * bins_y per plane
MI_MAX_RADIUS = 64                             # int(4 * sigma + 0.5) of vs_mutual_information
MI_MAX_PLANES = 65535
_MI_WORKSPACES = {}


def _bins(value, what):
    if isinstance(value, bool) or not isinstance(value, _numbers.Integral) or value < 1:
        raise ValueError("%s is an integer >= 1, got %r" % (what, value))
    return int(value)


def _intensity_volume(t, what):
    """every check that needs no device; the tensor is used as it is — no conversion and no copy behind the caller's back"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError("%s: intensity volumes are float32 tensors, got %s" % (what, getattr(t, "dtype", type(t))))
    if t.dim() != 5:
        raise ValueError("%s: expected a planar (N, C, D, H, W) volume, got shape %s" % (what, tuple(t.shape)))
    if t.numel() == 0 or t.shape[2] * t.shape[3] * t.shape[4] >= 2 ** 31:
        raise ValueError("%s: an empty volume or a plane of 2^31 voxels or more, shape %s" % (what, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s: the volume must be contiguous" % what)


def _bounds(pair, what):
    """(lo, hi) as two Python floats with lo <= hi, both finite"""
    import math
    try:
        lo, hi = (float(v) for v in pair)
    except (TypeError, ValueError):
        raise ValueError("%s is a pair (lo, hi) of numbers, got %r" % (what, pair)) from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError("%s needs finite bounds with lo <= hi, got %r" % (what, (lo, hi)))
    return lo, hi


def histogram(x, bins, range=None, labels=None, rows=0):
    """np.histogram of every (n, c) plane of a planar fp32 volume (N, C, D, H, W) on the device, optionally one histogram per label.
    Edges: the fp64 values np.linspace(lo, hi, bins + 1) (product and sum rounded separately; lo == hi becomes lo - 0.5, hi + 0.5).  range=(lo, hi): the
    same host bounds for all planes; range=None: per plane the minimum and maximum over its finite voxels, found on the device ((0, 0) without any).
    A voxel x, promoted to fp64, is in bin i iff e_i <= x < e_{i+1}; x == e_bins is in the last bin.
    labels: an int32 volume of x's shape (ops.cc_label's labels, an argmax); row r of the table counts the voxels labelled r, 0 <= r <= rows.
    -> {"table": int64 (N, C, rows + 1, bins); "edges": fp64 (N, C, bins + 1); "outside": int64 (N, C), NaN, +-inf and out-of-range voxels, in no bin;
        "overflow": int32 (N, C), voxels whose label is negative or above rows — counted there and nowhere else}.
    bins <= 4096 and (rows + 1) * bins <= 2^22.  Three or four launches, no synchronisation (vs_histogram)."""
    b = _bins(bins, "histogram: bins")
    r = _rows(rows, "histogram: rows", 0)
    if b > HISTOGRAM_MAX_BINS or (r + 1) * b > HISTOGRAM_MAX_CELLS:
        raise ValueError("histogram: bins = %d, (rows + 1) * bins = %d; at most 4096 bins and 2^22 cells per plane" % (b, (r + 1) * b))
    lo, hi = (0.0, 0.0) if range is None else _bounds(range, "histogram: range")
    _intensity_volume(x, "histogram")
    if labels is None:
        if r != 0:
            raise ValueError("histogram: rows = %d without labels" % r)
    else:
        _label_volume(labels, "histogram")
        if labels.shape != x.shape or labels.device != x.device:
            raise ValueError("histogram: labels and x differ in shape or device: %s vs %s" % (tuple(labels.shape), tuple(x.shape)))
    _require_cuda(x, labels)
    n, c, d, h, w = x.shape
    table = torch.empty((n, c, r + 1, b), dtype=torch.int64, device=x.device)
    edges = torch.empty((n, c, b + 1), dtype=torch.float64, device=x.device)
    outside = torch.empty((n, c), dtype=torch.int64, device=x.device)
    overflow = torch.empty((n, c), dtype=torch.int32, device=x.device)
    check(lib.vs_histogram(x.data_ptr(), _p(labels), n, c, d, h, w, b, r, lo, hi, int(range is None), edges.data_ptr(), table.data_ptr(),
                           outside.data_ptr(), overflow.data_ptr(), _stream()), "histogram")
    return {"table": table, "edges": edges, "outside": outside, "overflow": overflow}


def joint_histogram(x, y, bins=(256, 256), range=None):
    """np.histogram2d of every (n, c) plane of two planar fp32 volumes of one shape (N, C, D, H, W) on the device, with histogram's binning rule per
    variable.  bins: an integer or (bins_x, bins_y); range: None (bounds from the data, per plane and variable) or ((lo_x, hi_x), (lo_y, hi_y)).
    -> {"table": int64 (N, C, bins_x, bins_y), table[..., i, j] = voxels with x in bin i and y in bin j; "edges_x": fp64 (N, C, bins_x + 1); "edges_y";
        "outside": int64 (N, C), voxels with either value NaN, +-inf or out of range — in no cell}.
    bins_x * bins_y <= 2^22.  Three or four launches, no synchronisation (vs_joint_histogram)."""
    if isinstance(bins, _numbers.Integral) and not isinstance(bins, bool):
        bins = (bins, bins)
    try:
        bx, by = bins
    except (TypeError, ValueError):
        raise ValueError("joint_histogram: bins is an integer or a pair, got %r" % (bins,)) from None
    bx, by = _bins(bx, "joint_histogram: bins_x"), _bins(by, "joint_histogram: bins_y")
    if bx * by > HISTOGRAM_MAX_CELLS:
        raise ValueError("joint_histogram: bins_x * bins_y = %d cells per plane, at most 2^22" % (bx * by))
    r4 = None
    if range is not None:
        try:
            rx, ry = range
        except (TypeError, ValueError):
            raise ValueError("joint_histogram: range is None or ((lo_x, hi_x), (lo_y, hi_y)), got %r" % (range,)) from None
        r4 = (_ctypes.c_double * 4)(*(_bounds(rx, "joint_histogram: range of x") + _bounds(ry, "joint_histogram: range of y")))
    _intensity_volume(x, "joint_histogram")
    _intensity_volume(y, "joint_histogram")
    if x.shape != y.shape or x.device != y.device:
        raise ValueError("joint_histogram: the two volumes differ in shape or device: %s vs %s" % (tuple(x.shape), tuple(y.shape)))
    _require_cuda(x, y)
    n, c, d, h, w = x.shape
    table = torch.empty((n, c, bx, by), dtype=torch.int64, device=x.device)
    edges_x = torch.empty((n, c, bx + 1), dtype=torch.float64, device=x.device)
    edges_y = torch.empty((n, c, by + 1), dtype=torch.float64, device=x.device)
    outside = torch.empty((n, c), dtype=torch.int64, device=x.device)
    check(lib.vs_joint_histogram(x.data_ptr(), y.data_ptr(), n, c, d, h, w, bx, by, None if r4 is None else _ctypes.addressof(r4), int(r4 is None),
                                 edges_x.data_ptr(), edges_y.data_ptr(), table.data_ptr(), outside.data_ptr(), _stream()), "joint_histogram")
    return {"table": table, "edges_x": edges_x, "edges_y": edges_y, "outside": outside}


def mutual_information(table, sigma=1.0, normalized=True):
    """The tail of the reference's mutual_information_3d (utils/utils.py:824-845) on an int64 joint histogram (N, C, bins_x, bins_y), in fp64 on the
    device: scipy.ndimage.gaussian_filter(jh, sigma, mode="constant") (sigma == 0: none), + eps, division by the total, the marginals s1 and s2, then
    (sum s1 log s1 + sum s2 log s2) / sum jh log jh - 1 when normalized, otherwise sum jh log jh - sum s1 log s1 - sum s2 log s2.
    -> fp64 (N, C).  Every sum runs in a fixed order: the same bits on every run.  No synchronisation (vs_mutual_information).
    sigma is a number >= 0 with int(4 * sigma + 0.5) <= 64; N * C <= 65535."""
    import math
    if isinstance(sigma, bool) or not isinstance(sigma, _numbers.Real) or not (sigma >= 0) or math.isinf(sigma) or int(4.0 * sigma + 0.5) > MI_MAX_RADIUS:
        raise ValueError("mutual_information: sigma is a number >= 0 with a kernel radius int(4 sigma + 0.5) <= %d, got %r" % (MI_MAX_RADIUS, sigma))
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int64:
        raise TypeError("mutual_information: the table is an int64 tensor (ops.joint_histogram's), got %s" % getattr(table, "dtype", type(table)))
    if table.dim() != 4 or table.numel() == 0:
        raise ValueError("mutual_information: expected a table (N, C, bins_x, bins_y), got shape %s" % (tuple(table.shape),))
    n, c, bx, by = table.shape
    if bx * by > HISTOGRAM_MAX_CELLS or n * c > MI_MAX_PLANES:
        raise ValueError("mutual_information: at most 2^22 cells per plane and %d planes, got shape %s" % (MI_MAX_PLANES, tuple(table.shape)))
    if not table.is_contiguous():
        raise ValueError("mutual_information: the table must be contiguous")
    _require_cuda(table)
    ws = _workspace(_MI_WORKSPACES, (n, c, bx, by, table.device), lambda: 8 * n * c * (2 * bx * by + 2 * bx + by), "mutual_information workspace",
                    table.device)
    mi = torch.empty((n, c), dtype=torch.float64, device=table.device)
    check(lib.vs_mutual_information(table.data_ptr(), n, c, bx, by, float(sigma), int(bool(normalized)), ws.data_ptr(), mi.data_ptr(), _stream()),
          "mutual_information")
    return mi


# sliding-window prediction (csrc/window.hip).  evaluation.sliding_window_predict drives these; nothing here synchronises.
SW_BLENDS = ("constant", "gaussian")
SW_GAUSSIAN_FLOOR = 1e-3


def sw_plan_host(shape, patch, overlap):
    """vs_sw_plan on the host: the window origins of a (D, H, W) volume tiled with cubic `patch` windows -> numpy int32 (nw, 3), D-major, then H, then W.
    Per axis step = max(1, floor(patch (1 - overlap))), n = 1 if S <= patch else ceil((S - patch) / step) + 1, origin i = min(i step, max(S - patch, 0))."""
    import numpy as np
    d, h, w = (int(s) for s in shape)
    nw = lib.vs_sw_plan(d, h, w, int(patch), float(overlap), None, 0)
    check(min(nw, 0), "sw_plan")
    table = np.empty((nw, 3), dtype=np.int32)
    check(min(lib.vs_sw_plan(d, h, w, int(patch), float(overlap), table.ctypes.data, nw), 0), "sw_plan")
    return table


def sw_plan(shape, patch, overlap, device="cuda"):
    """-> (origins: int32 (nw, 3) tensor on `device`, nw) — sw_plan_host's table where the kernels read it"""
    table = sw_plan_host(shape, patch, overlap)
    return torch.from_numpy(table).to(device), int(table.shape[0])


def sw_weights(patch, blend="gaussian", device="cuda"):
    """The separable importance map of a window as an fp32 (3, patch) tensor (rows: z, y, x; a voxel's weight is their fp32 product).
    "constant": ones.  "gaussian": exp(-((i - (patch - 1) / 2) / sigma)^2 / 2) with sigma = patch / 8 per axis, computed in float64, floored at
    1e-3 and rounded to fp32."""
    import numpy as np
    p = int(patch)
    if p <= 0:
        raise ValueError("sw_weights: patch must be positive, got %r" % (patch,))
    if blend == "constant":
        row = np.ones(p, dtype=np.float64)
    elif blend == "gaussian":
        i = np.arange(p, dtype=np.float64)
        row = np.maximum(np.exp(-0.5 * ((i - (p - 1) / 2.0) / (p / 8.0)) ** 2), SW_GAUSSIAN_FLOOR)
    else:
        raise ValueError("sw_weights: blend is one of %s, got %r" % (SW_BLENDS, blend))
    return torch.from_numpy(np.stack([row, row, row]).astype(np.float32)).to(device)


def _sw_common(origins, first, weights, patch):
    if origins.dtype != torch.int32 or origins.dim() != 2 or origins.shape[1] != 3 or not origins.is_contiguous():
        raise ValueError("sw: origins is the contiguous int32 (nw, 3) table of sw_plan")
    if first.dtype != torch.int32 or first.numel() != 1:
        raise ValueError("sw: first is one int32 device word")
    if weights is not None and (weights.dtype != torch.float32 or tuple(weights.shape) != (3, patch) or not weights.is_contiguous()):
        raise ValueError("sw: weights is the contiguous fp32 (3, %d) tensor of sw_weights" % patch)


def sw_flips(flips):
    """The flip codes of a mirror-TTA pass (bit 0 mirrors W, bit 1 H, bit 2 D) -> (nf, the codes packed three bits each, code i in bits [3 i, 3 i + 3)):
    how vs_sw_gather_tta and vs_sw_accumulate_tta take them.  1 to 8 distinct integers in 0..7, ValueError otherwise."""
    try:
        codes = [int(c) for c in flips]
        exact = all(c == f for c, f in zip(codes, flips))
    except (TypeError, ValueError):
        codes, exact = [], False
    if not exact or not 1 <= len(codes) <= 8 or any(c < 0 or c > 7 for c in codes) or len(set(codes)) != len(codes):
        raise ValueError("sw: flips is a sequence of 1 to 8 distinct codes in 0..7 (bit 0 mirrors W, bit 1 H, bit 2 D), got %r" % (flips,))
    return len(codes), sum(c << (3 * i) for i, c in enumerate(codes))


def sw_gather(volume, origins, first, batch, patch=None, cval=0.0, out=None, flips=None):
    """Windows [first, first + batch) of the plan, cut from the planar fp32 volume (C, D, H, W) -> (batch, C, P, P, P).  `first`: an int32 device word.
    Slots past the plan and positions past the volume read cval.  out: the batch tensor to fill (a fixed address for a captured launch).
    flips (a sequence of codes, sw_flips): `first` counts items — item j is window j // nf mirrored by flips[j % nf] — and each slot is written
    already mirrored (vs_sw_gather_tta)."""
    packed = None if flips is None else sw_flips(flips)
    _require_cuda(volume, origins, first, out)
    if volume.dim() != 4 or volume.dtype != torch.float32 or not volume.is_contiguous() or volume.data_ptr() % 16:
        raise ValueError("sw_gather: expected a contiguous, 16-byte aligned fp32 (C, D, H, W) volume, got %s %s" % (tuple(volume.shape), volume.dtype))
    c, d, h, w = volume.shape
    if out is None:
        out = torch.empty((int(batch), c) + (int(patch),) * 3, dtype=torch.float32, device=volume.device)
    p = out.shape[-1]
    if out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (int(batch), c, p, p, p) or (patch is not None and p != int(patch)):
        raise ValueError("sw_gather: out must be a contiguous fp32 (%d, %d, P, P, P) tensor, got %s" % (int(batch), c, tuple(out.shape)))
    _sw_common(origins, first, None, p)
    if packed is None:
        check(lib.vs_sw_gather(volume.data_ptr(), out.data_ptr(), origins.data_ptr(), first.data_ptr(), origins.shape[0], int(batch), c, d, h, w, p,
                               float(cval), _stream()), "sw_gather")
    else:
        check(lib.vs_sw_gather_tta(volume.data_ptr(), out.data_ptr(), origins.data_ptr(), first.data_ptr(), origins.shape[0], int(batch), c, d, h, w, p,
                                   float(cval), packed[0], packed[1], _stream()), "sw_gather_tta")
    return out


def sw_accumulate(prob, acc, wsum, origins, first, weights, flips=None):
    """acc (K, D, H, W) += w * prob (B, K, P, P, P) and wsum (D, H, W) += w for the windows [first, first + B) that lie in the plan, in place, every voxel's
    terms in ascending window index and without atomics: bit-identical for every B.  Batches are accumulated in ascending order of `first`.
    flips (as sw_gather): the slots are items, each probability is read mirrored back and weighted at the voxel's own position, terms in ascending item
    index (vs_sw_accumulate_tta)."""
    packed = None if flips is None else sw_flips(flips)
    _require_cuda(prob, acc, wsum, origins, first, weights)
    pr = _contig(prob.detach().float())
    if pr.data_ptr() % 16:
        pr = pr.clone()
    if pr.dim() != 5 or acc.dim() != 4 or wsum.dim() != 3 or pr.shape[1] != acc.shape[0] or tuple(acc.shape[1:]) != tuple(wsum.shape) or \
            not (pr.shape[2] == pr.shape[3] == pr.shape[4]):
        raise ValueError("sw_accumulate: prob (B, K, P, P, P), acc (K, D, H, W), wsum (D, H, W); got %s, %s, %s" % (tuple(prob.shape), tuple(acc.shape), tuple(wsum.shape)))
    for t in (acc, wsum):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("sw_accumulate: acc and wsum are contiguous fp32 tensors (they are updated in place)")
    b, k, p = pr.shape[0], pr.shape[1], pr.shape[2]
    _sw_common(origins, first, weights, p)
    d, h, w = wsum.shape
    if packed is None:
        check(lib.vs_sw_accumulate(pr.data_ptr(), acc.data_ptr(), wsum.data_ptr(), origins.data_ptr(), first.data_ptr(), origins.shape[0], b, k, d, h, w, p,
                                   weights[0].data_ptr(), weights[1].data_ptr(), weights[2].data_ptr(), _stream()), "sw_accumulate")
    else:
        check(lib.vs_sw_accumulate_tta(pr.data_ptr(), acc.data_ptr(), wsum.data_ptr(), origins.data_ptr(), first.data_ptr(), origins.shape[0], b, k, d, h, w,
                                       p, weights[0].data_ptr(), weights[1].data_ptr(), weights[2].data_ptr(), packed[0], packed[1], _stream()),
              "sw_accumulate_tta")


def sw_finalize(acc, wsum, label=True, onehot=False):
    """-> (prob = acc / wsum (K, D, H, W) fp32, label (D, H, W) uint8 or None, onehot (K, D, H, W) fp32 or None) in one pass.  The label is the channel
    argmax of prob, ties to the first maximal channel (vs_hard_onehot's rule)."""
    _require_cuda(acc, wsum)
    if acc.dim() != 4 or tuple(acc.shape[1:]) != tuple(wsum.shape) or acc.dtype != torch.float32 or wsum.dtype != torch.float32 or \
            not acc.is_contiguous() or not wsum.is_contiguous():
        raise ValueError("sw_finalize: acc (K, D, H, W) and wsum (D, H, W) are contiguous fp32 tensors; got %s, %s" % (tuple(acc.shape), tuple(wsum.shape)))
    k, d, h, w = acc.shape
    prob = torch.empty_like(acc)
    lab = torch.empty((d, h, w), dtype=torch.uint8, device=acc.device) if label else None
    hot = torch.empty_like(acc) if onehot else None
    check(lib.vs_sw_finalize(acc.data_ptr(), wsum.data_ptr(), prob.data_ptr(), _p(lab), _p(hot), k, d, h, w, _stream()), "sw_finalize")
    return prob, lab, hot


# a patch-space prediction pasted back into scan geometry (csrc/uncrop.hip)
UNCROP_INTERPS = ("nearest", "linear")


def uncrop(prob, geometry, shape, interp="linear", want_prob=False):
    """The probabilities (K, P, P, P), 1 <= K <= 8, that a network gave on a CropResize patch, resampled onto the scan grid `shape` = (D, H, W).
    geometry = (lo[3], hi[3], off[3], side) of data_gpu.crop_geometry: scan voxel v with lo <= v < hi has cube index u = v - lo + off and patch coordinate
    (u + 0.5) P / side - 0.5.  interp "linear": trilinear, edge replicate; "nearest": the order-0 zoom's rounding.  Outside the cube: background.
    -> {"label": (D, H, W) uint8 — argmax, ties to the first channel — and, with want_prob, "prob": (K, D, H, W) fp32, (1, 0, ..., 0) outside the cube}.
    One launch writes both outputs whole; it does not synchronise."""
    _require_cuda(prob)
    if interp not in UNCROP_INTERPS:
        raise ValueError("uncrop: interp is one of %s, got %r" % (UNCROP_INTERPS, interp))
    pr = _contig(prob.detach().float())
    if pr.data_ptr() % 16:
        pr = pr.clone()
    if pr.dim() != 4 or not (pr.shape[1] == pr.shape[2] == pr.shape[3]) or not 1 <= pr.shape[0] <= 8:
        raise ValueError("uncrop: expected probabilities (K, P, P, P) with 1 <= K <= 8, got %s" % (tuple(prob.shape),))
    lo, hi, off, side = geometry
    lo, hi, off = ([int(v) for v in t] for t in (lo, hi, off))
    d, h, w = (int(s) for s in shape)
    if not (len(lo) == len(hi) == len(off) == 3):
        raise ValueError("uncrop: geometry is (lo[3], hi[3], off[3], side), got %r" % (geometry,))
    label = torch.empty((d, h, w), dtype=torch.uint8, device=pr.device)
    out = torch.empty((pr.shape[0], d, h, w), dtype=torch.float32, device=pr.device) if want_prob else None
    check(lib.vs_uncrop(pr.data_ptr(), label.data_ptr(), _p(out), pr.shape[0], pr.shape[1], d, h, w, *lo, *hi, *off, int(side),
                        UNCROP_INTERPS.index(interp), _stream()), "uncrop")
    res = {"label": label}
    if want_prob:
        res["prob"] = out
    return res


# scan geometry: the array a scanner wrote <-> the re-oriented 1 mm grid (csrc/scan.hip; data_gpu.ScanGeometry does the host arithmetic)
SCAN_DTYPES = {torch.int16: _lib.VS_SCAN_I16, torch.uint8: _lib.VS_SCAN_U8, torch.int8: _lib.VS_SCAN_I8, torch.float32: _lib.VS_SCAN_F32}


def _scan_geometry(geometry, what):
    """-> (x, y, z, flip0, flip1, flip2, d1, h1, w1): a data_gpu.ScanGeometry or its as_tuple()"""
    g = geometry.as_tuple() if hasattr(geometry, "as_tuple") else tuple(geometry)
    if len(g) != 9:
        raise ValueError("%s: geometry is a data_gpu.ScanGeometry or its as_tuple() (x, y, z, flip0, flip1, flip2, d1, h1, w1), got %r" % (what, geometry))
    g = tuple(int(v) for v in g)
    if min(g[:3] + g[6:]) < 1:
        raise ValueError("%s: empty shape in geometry %r" % (what, g))
    return g


def _scan_tensor(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("%s: expected a CUDA tensor (libvaeseg HIP kernels; there is no CPU fallback), got %s" %
                        (what, "a %s tensor" % t.device.type if isinstance(t, torch.Tensor) else type(t).__name__))
    t = _contig(t.detach())
    return t.clone() if t.data_ptr() % 16 else t


def scan_orient(raw, geometry):
    """raw (X, Y, Z) int16 / uint8 / int8 / float32 as the scanner wrote it -> the oriented float32 volume (Y, X, Z) of data_process.py:29-30,
    transpose(raw, [1, 0, 2])[::ind[1], ::ind[0], ::ind[2]], exact values, one launch (vs_scan_orient)."""
    r = _scan_tensor(raw, "scan_orient")
    if r.dtype not in SCAN_DTYPES:
        raise TypeError("scan_orient: raw is int16, uint8, int8 or float32, got %s" % r.dtype)
    if r.dim() != 3:
        raise ValueError("scan_orient: expected a raw scan (X, Y, Z), got shape %s" % (tuple(r.shape),))
    x, y, z, f0, f1, f2 = _scan_geometry(geometry, "scan_orient")[:6]
    if tuple(r.shape) != (x, y, z):
        raise ValueError("scan_orient: the geometry's raw_shape %s is not the tensor's %s" % ((x, y, z), tuple(r.shape)))
    out = torch.empty((y, x, z), dtype=torch.float32, device=r.device)
    check(lib.vs_scan_orient(r.data_ptr(), SCAN_DTYPES[r.dtype], out.data_ptr(), x, y, z, f0, f1, f2, _stream()), "scan_orient")
    return out


def to_native(src, geometry, interp="linear", want_prob=False):
    """An answer on the 1 mm grid put back onto the voxel grid of the scan it came from, in that scan's axis order, orientation and spacing.
    src: planar probabilities (K, D1, H1, W1), 1 <= K <= 8 (any float dtype; resampled in fp32), or a uint8 label (D1, H1, W1), which is a copy of
    samples and takes interp="nearest" only.  Raw voxel (i0, i1, i2) has the oriented index (f(i1), f(i0), f(i2)), f the per-axis flip, and per axis the
    1 mm coordinate q = (o + 0.5) n_1mm / n_oriented - 0.5 (fp64).  "nearest": the sample at floor(q + 0.5) clamped to [0, n_1mm - 1]; "linear":
    trilinear with q mirrored at the borders, scipy.ndimage.zoom(order=1, mode="mirror", grid_mode=True).
    -> {"label": (X, Y, Z) uint8 — argmax, ties to the first channel — and, with want_prob, "prob": (K, X, Y, Z) fp32}.  One launch writes both outputs
    whole (vs_scan_to_native); it does not synchronise and can be captured in a graph."""
    s = _scan_tensor(src, "to_native")
    if interp not in UNCROP_INTERPS:
        raise ValueError("to_native: interp is one of %s, got %r" % (UNCROP_INTERPS, interp))
    is_label = s.dtype == torch.uint8
    if is_label:
        if s.dim() != 3:
            raise ValueError("to_native: expected a uint8 label (D1, H1, W1), got shape %s" % (tuple(s.shape),))
        if interp != "nearest" or want_prob:
            raise ValueError("to_native: a uint8 label is a copy of samples: interp=\"nearest\" and no probabilities")
        k = 1
    else:
        if not s.is_floating_point():
            raise TypeError("to_native: src is floating-point probabilities (K, D1, H1, W1) or a uint8 label (D1, H1, W1), got %s" % s.dtype)
        if s.dim() != 4 or not 1 <= s.shape[0] <= 8:
            raise ValueError("to_native: expected probabilities (K, D1, H1, W1) with 1 <= K <= 8, got shape %s" % (tuple(s.shape),))
        if s.dtype != torch.float32:
            s = s.float()
        k = int(s.shape[0])
    x, y, z, f0, f1, f2, d1, h1, w1 = _scan_geometry(geometry, "to_native")
    if tuple(s.shape[-3:]) != (d1, h1, w1):
        raise ValueError("to_native: the geometry's shape_1mm %s is not the tensor's %s" % ((d1, h1, w1), tuple(s.shape[-3:])))
    label = torch.empty((x, y, z), dtype=torch.uint8, device=s.device)
    out = torch.empty((k, x, y, z), dtype=torch.float32, device=s.device) if want_prob else None
    check(lib.vs_scan_to_native(s.data_ptr(), int(is_label), label.data_ptr(), _p(out), k, d1, h1, w1, x, y, z, f0, f1, f2, UNCROP_INTERPS.index(interp),
                                _stream()), "scan_to_native")
    res = {"label": label}
    if want_prob:
        res["prob"] = out
    return res


# ---- intensity augmentation (csrc/augment.hip; the transform lives in data_gpu.py) ---------------------------------------------------------------------
AUG_MAX_SIGMA = 2.0                 # radius int(4 sigma + 0.5) <= 8: what the blur kernel's LDS tile is sized for
AUG_OPS = {"none": 0, "contrast": 1, "power": 2, "restat": 3}


def _aug_planes(x, what):
    """a contiguous CUDA float32 tensor (..., D, H, W) -> (planes, d, h, w)"""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() < 3:
        raise TypeError("%s: a float32 tensor (..., D, H, W), got %s %s" % (what, getattr(x, "dtype", type(x)), tuple(getattr(x, "shape", ()))))
    d, h, w = (int(v) for v in x.shape[-3:])
    if x.numel() == 0 or d * h * w >= 2 ** 31:
        raise ValueError("%s: an empty tensor or a plane of 2^31 voxels or more, shape %s" % (what, tuple(x.shape)))
    if not x.is_contiguous():
        raise ValueError("%s: the tensor must be contiguous" % what)
    _require_cuda(x)
    return x.numel() // (d * h * w), d, h, w


def _aug_workspace(planes, d, h, w, device):
    return torch.empty(int(lib.vs_aug_stats_workspace_bytes(planes, d, h, w)) // 8, dtype=torch.float64, device=device)


def aug_stats(x):
    """{min, max, mean, population std} of every (D, H, W) plane of a float32 tensor (..., D, H, W) -> fp64 (..., 4) on the device.  fp64 sums shifted by
    the plane's first voxel, over a fixed chunking of the linear voxel index in chunk order: a function of the plane's bits alone (two launches, no
    atomics, no synchronisation) — the record vs_aug_stage's epilogue writes for the plane it stores."""
    planes, d, h, w = _aug_planes(x, "aug_stats")
    rec = torch.empty(tuple(x.shape[:-3]) + (4,), dtype=torch.float64, device=x.device)
    ws = _aug_workspace(planes, d, h, w, x.device)
    check(lib.vs_aug_stats(x.data_ptr(), rec.data_ptr(), ws.data_ptr(), planes, d, h, w, _stream()), "aug_stats")
    return rec


def philox_normal(shape, seed, sample, channel=0):
    """the standard normals of one plane `shape` = (D, H, W), fp64 on the device: Philox4x32-10 under key `seed` and counter (pair, 0x100 + channel,
    sample), Box-Muller in fp64 (vs_aug_normal_philox) — what a noise stage with the source (seed, sample) adds, times s"""
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError("philox_normal: shape is (D, H, W), got %r" % (shape,))
    out = torch.empty(shape, dtype=torch.float64, device="cuda")
    check(lib.vs_aug_normal_philox(out.data_ptr(), *shape, int(seed) & (2 ** 64 - 1), int(sample) & (2 ** 64 - 1), int(channel), _stream()),
          "aug_normal_philox")
    return out


def gaussian_weights(sigma):
    """scipy.ndimage's _gaussian_kernel1d(sigma, 0, int(4 sigma + 0.5)) from the centre outwards: w[k] is the weight of taps -k and +k (host, numpy)"""
    import numpy as np
    sigma = float(sigma)
    if not 0.0 < sigma <= AUG_MAX_SIGMA:
        raise ValueError("gaussian blur: 0 < sigma <= %g (radius <= 8), got %r" % (AUG_MAX_SIGMA, sigma))
    radius = int(4.0 * sigma + 0.5)
    k = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:], dtype=np.float64)


def blur_tile(sigma):
    """the (z, y, x) tile of outputs one workgroup of the blur kernel computes at this sigma"""
    t = (_ctypes.c_int * 3)()
    check(lib.vs_aug_blur_tile(float(sigma), t), "aug_blur_tile")
    return tuple(t)


def gaussian_blur3d(x, sigma):
    """scipy.ndimage.gaussian_filter(x, sigma, mode="reflect", truncate=4) of one float32 volume (D, H, W): passes along z, y, x, fp64 accumulation,
    rounded to fp32 after each; one launch, the three passes over an LDS tile (vs_aug_blur).  0 < sigma <= 2."""
    planes, d, h, w = _aug_planes(x, "gaussian_blur3d")
    if x.dim() != 3:
        raise ValueError("gaussian_blur3d: one volume (D, H, W), got shape %s" % (tuple(x.shape),))
    wts = gaussian_weights(sigma)
    out = torch.empty_like(x)
    check(lib.vs_aug_blur(x.data_ptr(), out.data_ptr(), d, h, w, float(sigma), wts.ctypes.data, _stream()), "aug_blur")
    return out


def aug_flip(x, mask):
    """every (D, H, W) plane of a float32 tensor (..., D, H, W) mirrored along z / y / x for the bits 4 / 2 / 1 of mask: a copy (vs_aug_flip)"""
    planes, d, h, w = _aug_planes(x, "aug_flip")
    mask = int(mask)
    if not 0 <= mask <= 7:
        raise ValueError("aug_flip: mask is 0..7 (z, y, x = 4, 2, 1), got %r" % (mask,))
    out = torch.empty_like(x)
    check(lib.vs_aug_flip(x.data_ptr(), out.data_ptr(), planes, d, h, w, mask, _stream()), "aug_flip")
    return out


def aug_stage(x, flip=0, flip_first=False, noise=None, s=0.0, channel=0, mult=None, op="none", p=0.0, flag=False, rec=None, rec0=None, mean0=0.0,
              std0=1.0, want_rec=False):
    """One pass of vs_aug_stage over one float32 volume (D, H, W) -> (y, record of y or None).  noise: None, an fp64 device tensor of x's shape, or a
    tuple (seed, sample) for the Philox normals of `channel`; rec / rec0: fp64 records (4,) on the device (aug_stats); see include/vaeseg.h for the
    order of the steps.  One launch, two with want_rec; nothing is synchronised or read back."""
    planes, d, h, w = _aug_planes(x, "aug_stage")
    if x.dim() != 3:
        raise ValueError("aug_stage: one volume (D, H, W), got shape %s" % (tuple(x.shape),))
    mode, narr, seed, sample = 0, None, 0, 0
    if isinstance(noise, tuple):
        mode, seed, sample = 2, int(noise[0]) & (2 ** 64 - 1), int(noise[1]) & (2 ** 64 - 1)
    elif noise is not None:
        if not (isinstance(noise, torch.Tensor) and noise.dtype == torch.float64 and noise.shape == x.shape and noise.is_cuda and noise.is_contiguous()):
            raise TypeError("aug_stage: noise is a contiguous CUDA float64 tensor of shape %s or a tuple (seed, sample)" % (tuple(x.shape),))
        mode, narr = 1, noise
    y = torch.empty_like(x)
    rec_out = torch.empty(4, dtype=torch.float64, device=x.device) if want_rec else None
    ws = _aug_workspace(1, d, h, w, x.device) if want_rec else None
    check(lib.vs_aug_stage(x.data_ptr(), y.data_ptr(), d, h, w, int(flip), int(bool(flip_first)), mode, _p(narr), float(s), seed, sample, int(channel),
                           int(mult is not None), 1.0 if mult is None else float(mult), AUG_OPS[op], float(p), int(bool(flag)), _p(rec), _p(rec0),
                           float(mean0), float(std0), _p(rec_out), _p(ws), _stream()), "aug_stage")
    return y, rec_out


# ---- zoom with edge boundaries, simulated low resolution (csrc/lowres.hip) ---------------------------------------------------------------
ZOOM_EDGE_ORDERS = (0, 1, 3)
ZOOM_EDGE_MAX_LEN = 512             # order 3: the longest line a workgroup's LDS bundle holds


def zoom_edge_bundle(m, n):
    """the lines one workgroup of an order-3 pass holds at input length m and output length n"""
    return int(lib.vs_zoom_edge_bundle(int(m), int(n)))


def _zoom_edge_shape(shape, what):
    try:
        out = tuple(int(v) for v in shape)
    except TypeError:
        raise TypeError("%s: a shape (D, H, W), got %r" % (what, shape))
    if len(out) != 3 or min(out) < 1:
        raise ValueError("%s: a shape (D, H, W) of positive lengths, got %r" % (what, shape))
    return out


def zoom_edge(x, out_shape, order=3, clip=True):
    """scipy.ndimage.zoom(x.astype(float64), out / in, order=order, mode="nearest", grid_mode=True) of one float32 volume (D, H, W), clipped to
    [x.min(), x.max()] when clip (and order > 0), rounded to float32 once.  order 0, 1 or 3; order 3: every axis of x and of out_shape at most 512.
    One launch for orders 0 and 1, three for order 3, two more for the clip's bounds, which stay on the device; nothing is synchronised or read back."""
    planes, d, h, w = _aug_planes(x, "zoom_edge")
    if x.dim() != 3:
        raise ValueError("zoom_edge: one volume (D, H, W), got shape %s" % (tuple(x.shape),))
    out_shape = _zoom_edge_shape(out_shape, "zoom_edge")
    if order not in ZOOM_EDGE_ORDERS:
        raise ValueError("zoom_edge: order is 0, 1 or 3, got %r" % (order,))
    order = int(order)
    if order == 3 and max((d, h, w) + out_shape) > ZOOM_EDGE_MAX_LEN:
        raise ValueError("zoom_edge: order 3 takes axes of at most %d voxels, got %s -> %s" % (ZOOM_EDGE_MAX_LEN, (d, h, w), out_shape))
    if out_shape[0] * out_shape[1] * out_shape[2] >= 2 ** 31:
        raise ValueError("zoom_edge: an output of 2^31 voxels or more, shape %s" % (out_shape,))
    y = torch.empty(out_shape, dtype=torch.float32, device=x.device)
    ws = torch.empty(int(lib.vs_zoom_edge_workspace_bytes(d, h, w, *out_shape, order)) // 8, dtype=torch.float64, device=x.device)
    check(lib.vs_zoom_edge(x.data_ptr(), y.data_ptr(), d, h, w, *out_shape, order, int(bool(clip)), ws.data_ptr(), _stream()), "zoom_edge")
    return y


def simulate_lowres(x, target_shape, order_down=0, order_up=3):
    """nnU-Net's simulated low resolution of one float32 volume (D, H, W): zoom_edge down to target_shape (order_down, clipped when order_down > 0), then
    zoom_edge back to x's shape (order_up, clipped to the down-sampled volume's range when order_up > 0).  The bits of the two calls."""
    planes, d, h, w = _aug_planes(x, "simulate_lowres")
    if x.dim() != 3:
        raise ValueError("simulate_lowres: one volume (D, H, W), got shape %s" % (tuple(x.shape),))
    target_shape = _zoom_edge_shape(target_shape, "simulate_lowres")
    for order in (order_down, order_up):
        if order not in ZOOM_EDGE_ORDERS:
            raise ValueError("simulate_lowres: an order is 0, 1 or 3, got %r" % (order,))
    t = zoom_edge(x, target_shape, order_down, clip=order_down > 0)
    return zoom_edge(t, (d, h, w), order_up, clip=order_up > 0)


# ---- exact percentiles and the piecewise-linear intensity map (csrc/quantile.hip) --------------------------------------------------------
QUANTILE_MAX_Q = 16
QUANTILE_WG_VOXELS = 16384          # csrc/quantile.hip QS_WG_VOXELS: the voxels of a plane one workgroup of a counting pass reads (a hand-kept mirror,
                                    # as INTENSITY_MAP_WG_VOXELS is of IM_WG_VOXELS: the library does not export them; change both files together)
INTENSITY_MAP_MAX_L = 16
INTENSITY_MAP_WG_VOXELS = 4096      # csrc/quantile.hip IM_WG_VOXELS
INTENSITY_MAP_EXTRAPOLATE = ("linear", "clamp")


def quantile(x, q, above=None, mask=None):
    """Exact percentiles of every (D, H, W) plane of a contiguous CUDA float32 tensor (..., D, H, W); q: 1 to 16 percentiles in [0, 100], host floats.
    A voxel is selected iff it is finite, `above` is None or x > np.float32(above) (strict), and `mask` (uint8 or bool, x's shape) is None or non-zero
    there.  With v the n selected values sorted, in fp64: h = (n - 1) * (p / 100), k = floor(h), t = h - k, a = v[k], b = v[min(k + 1, n - 1)] and
    t >= 0.5 ? b - (b - a) (1 - t) : a + (b - a) t, each operation rounded on its own — the bits of np.percentile(selected.astype(float64), p).
    -> {"q": fp64 (..., Q); "lo", "hi": float32 (..., Q), a and b; "count": int64 (...), n; "rejected": int64 (...), the non-finite voxels}, on the
    device; n == 0 gives NaN.  A radix select, nine launches whatever the data; nothing is synchronised or read back (vs_quantile)."""
    import math
    planes, d, h, w = _aug_planes(x, "quantile")
    try:
        ps = [float(v) for v in (q if hasattr(q, "__iter__") else [q])]
    except (TypeError, ValueError):
        raise ValueError("quantile: q is a percentile or a sequence of percentiles, got %r" % (q,)) from None
    if not 1 <= len(ps) <= QUANTILE_MAX_Q:
        raise ValueError("quantile: 1 to %d percentiles, got %d" % (QUANTILE_MAX_Q, len(ps)))
    if any(not math.isfinite(p) or p < 0.0 or p > 100.0 for p in ps):
        raise ValueError("quantile: percentiles are finite numbers in [0, 100], got %r" % (ps,))
    use_above, thr = 0, 0.0
    if above is not None:
        thr = float(above)
        if math.isnan(thr):
            raise ValueError("quantile: above is a number, got %r" % (above,))
        use_above = 1
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool):
            raise TypeError("quantile: mask is a uint8 or bool tensor, got %s" % getattr(mask, "dtype", type(mask)))
        if mask.shape != x.shape or mask.device != x.device or not mask.is_contiguous():
            raise ValueError("quantile: mask is a contiguous tensor of x's shape on x's device, got %s on %s" % (tuple(mask.shape), mask.device))
    nq, lead = len(ps), tuple(x.shape[:-3])
    p01 = (_ctypes.c_double * nq)(*[p / 100.0 for p in ps])
    out = {"q": torch.empty(lead + (nq,), dtype=torch.float64, device=x.device),
           "lo": torch.empty(lead + (nq,), dtype=torch.float32, device=x.device),
           "hi": torch.empty(lead + (nq,), dtype=torch.float32, device=x.device),
           "count": torch.empty(lead, dtype=torch.int64, device=x.device),
           "rejected": torch.empty(lead, dtype=torch.int64, device=x.device)}
    ws = torch.empty((int(lib.vs_quantile_workspace_bytes(planes, d * h * w, nq)) + 15) // 16 * 2, dtype=torch.float64, device=x.device)
    check(lib.vs_quantile(x.data_ptr(), _p(mask), use_above, thr, _ctypes.addressof(p01), nq, out["q"].data_ptr(), out["lo"].data_ptr(),
                          out["hi"].data_ptr(), out["count"].data_ptr(), out["rejected"].data_ptr(), ws.data_ptr(), planes, d, h, w, _stream()), "quantile")
    return out


def intensity_map(x, src, dst, extrapolate="linear", out=None):
    """The piecewise-linear map of every (D, H, W) plane of a contiguous CUDA float32 tensor (..., D, H, W) through landmarks on the device: src fp64
    (..., L), one ascending row per plane (quantile's "q", never copied to the host); dst fp64 (L,), strictly ascending, for all planes; 2 <= L <= 16.
    A finite voxel x with j the largest index in [0, L - 2] with src[j] <= x (0 below src[0]): y = dst[j] + (x - src[j]) * slope, slope =
    (dst[j+1] - dst[j]) / (src[j+1] - src[j]) or 0 for a segment of no width, in fp64, each operation rounded on its own, rounded to float32 once.
    extrapolate "linear": the end segments run on; "clamp": y is clamped to [dst[0], dst[L-1]].  A non-finite voxel and a plane with NaN landmarks
    are written unchanged.  -> float32 of x's shape (`out`, which may be x).  One launch, no synchronisation (vs_intensity_map)."""
    planes, d, h, w = _aug_planes(x, "intensity_map")
    if extrapolate not in INTENSITY_MAP_EXTRAPOLATE:
        raise ValueError("intensity_map: extrapolate is 'linear' or 'clamp', got %r" % (extrapolate,))
    for t, what in ((src, "src"), (dst, "dst")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
            raise TypeError("intensity_map: %s is a float64 tensor on the device, got %s" % (what, getattr(t, "dtype", type(t))))
        if t.device != x.device or not t.is_contiguous():
            raise ValueError("intensity_map: %s is contiguous and on x's device" % what)
    if dst.dim() != 1 or not 2 <= dst.shape[0] <= INTENSITY_MAP_MAX_L:
        raise ValueError("intensity_map: dst has shape (L,) with 2 <= L <= %d, got %s" % (INTENSITY_MAP_MAX_L, tuple(dst.shape)))
    nl = int(dst.shape[0])
    if tuple(src.shape) != tuple(x.shape[:-3]) + (nl,):
        raise ValueError("intensity_map: src has shape %s for x %s and L = %d, got %s" % (tuple(x.shape[:-3]) + (nl,), tuple(x.shape), nl, tuple(src.shape)))
    if out is None:
        out = torch.empty_like(x)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.shape == x.shape and out.device == x.device and out.is_contiguous()):
        raise ValueError("intensity_map: out is a contiguous float32 tensor of x's shape on x's device")
    check(lib.vs_intensity_map(x.data_ptr(), src.data_ptr(), dst.data_ptr(), nl, int(extrapolate == "clamp"), out.data_ptr(), planes, d, h, w, _stream()),
          "intensity_map")
    return out


def instnorm_stats(x):
    n, c = x.shape[0], x.shape[-1]
    st = _new_stats(n, c, x.device)
    check(lib.vs_instnorm_stats(x.data_ptr(), st.data_ptr(), n, x.numel() // (n * c), c, vs_dtype(x), _stream()),
          "instnorm_stats")
    return st
