#!/usr/bin/env python3
"""Record, in order, every call the package makes into libvaeseg (the C ABI of include/vaeseg.h) during one eager training step, for a set of
scenarios that together reach every form of the conv backward path of vae_segmentation_amd/ops.py — the check that a change to the HOST side
(ops.py) calls the library exactly as before.

    python tools/ops_call_trace.py run OUT.json            every scenario, on the deterministic build; needs a GPU
    python tools/ops_call_trace.py compare A.json B.json   call-for-call comparison of two runs (exit status 1 on any difference)

How a call is written down: the entry point's name, every scalar argument, the return value, and every pointer argument as "p0" for null or as
"p<index of that address's first appearance in the pass>" ("host" for the few arguments that point at host memory).  vs_conv_wgrad_multi[_workspace_bytes] and
vs_conv_k3_chain receive struct arrays by address: the array is decoded with ops.WgradDesc / ops.ChainLayer and every field written down the
same way.  Each scenario runs two passes on one model: a plain step, whose loss and parameter gradients are digested bit for bit, and a second
step with ops.PROFILE installed, which adds (kernel id, bytes, flops, detail) of each timed launch to the trace.

The tool works on any revision of the package whose library is reached through `_lib.lib` (it touches nothing else of ops.py than WgradDesc,
ChainLayer, PROFILE, the A/B flags and the public set_wgrad_* functions), so the same file runs against the parent and the changed tree.
It is a tool, not a test: pinning the call order in the suite would block the kernel projects that change it on purpose."""
import ctypes
import gc
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOST_ARGS = {"vs_up_compose_sizes": (3,), "vs_get_config": (0,), "vs_set_config": (0,), "vs_config_from_env": (0,)}
STRUCT_ARRAYS = {"vs_conv_wgrad_multi": "WgradDesc", "vs_conv_wgrad_multi_workspace_bytes": "WgradDesc", "vs_conv_k3_chain": "ChainLayer"}


class Recorder:
    """the trace of the pass that is running (None: calls go through unrecorded)"""

    def __init__(self):
        self.calls = None
        self.ptrs = None

    def begin(self):
        self.calls, self.ptrs = [], {}

    def end(self):
        calls, self.calls, self.ptrs = self.calls, None, None
        return calls

    def ptr(self, v):
        if not v:
            return "p0"
        return "p%d" % self.ptrs.setdefault(int(v), len(self.ptrs) + 1)

    def scalar(self, v):
        return repr(float(v)) if isinstance(v, float) else int(v)


REC = Recorder()


class Traced:
    """a loaded build (ctypes.CDLL) whose vs_* entry points write themselves down"""

    def __init__(self, cdll):
        self._cdll = cdll
        self._wrapped = {}

    def __getattr__(self, name):
        fn = getattr(self._cdll, name)
        if not name.startswith("vs_") or fn.restype is ctypes.c_char_p:
            return fn
        w = self._wrapped.get(name)
        if w is None:
            w = self._wrapped[name] = self._wrap(name, fn)
        return w

    @staticmethod
    def _wrap(name, fn):
        argtypes = fn.argtypes or []

        def call(*args):
            if REC.calls is None:
                return fn(*args)
            from vae_segmentation_amd import ops
            rec = [name]
            for i, (a, t) in enumerate(zip(args, argtypes)):
                if t is not ctypes.c_void_p:
                    rec.append(REC.scalar(a))
                elif i == 0 and name in STRUCT_ARRAYS:
                    cls = getattr(ops, STRUCT_ARRAYS[name])
                    arr = (cls * int(args[1])).from_address(a)
                    rec.append([[REC.ptr(getattr(s, f)) if ft is ctypes.c_void_p else REC.scalar(getattr(s, f)) for f, ft in cls._fields_] for s in arr])
                elif i in HOST_ARGS.get(name, ()):
                    rec.append("host" if a else "p0")
                else:
                    rec.append(REC.ptr(a))
            r = fn(*args)
            rec.append(["ret", 0 if r is None else (REC.ptr(r) if fn.restype is ctypes.c_void_p else REC.scalar(r))])
            REC.calls.append(rec)
            return r
        return call


def install():
    from vae_segmentation_amd import _lib
    l = _lib.lib
    l.use_deterministic(True)
    l._fast, l._det = Traced(l._fast), Traced(l._det)
    l._active = l._det


# ------------------------------------------------------------------------------------------------
# scenarios: name -> (build() -> (parameters, step), settings); step() -> loss after backward
# ------------------------------------------------------------------------------------------------
def _dtype(name):
    import torch
    return {"bf16": torch.bfloat16, "fp32": torch.float32}[name]


def _seg(side, dtype, n_class=2):
    import joint_model as M
    from vae_segmentation_amd import synthetic as S, train as T
    seg = S.deterministic_fill_(M.Segmentation(n_channels=1, n_class=n_class, norm_type=1), seed=0).cuda()
    M.set_kernel_dtype(seg, _dtype(dtype))
    img = S.synthetic_image(2, side, seed=2).cuda()
    if n_class == 2:
        lab = S.synthetic_label(2, side, seed=3).cuda()
    else:
        from oracle import ref_cpu as O
        lab = O.synthetic_label(2, side, 3, n_class=n_class).cuda()
    return list(seg.parameters()), lambda: T.seg_train_losses(seg, img, lab, n_class=n_class)[0]


def _joint(side, dtype):
    import joint_model as M
    from vae_segmentation_amd import synthetic as S, train as T
    joint = M.Joint(models=[M.Segmentation(n_channels=1, n_class=2, norm_type=1), M.VAE(n_channels=2, n_class=2, norm_type=1, dim=128, spatial=side)])
    S.deterministic_fill_(joint, seed=0)
    joint = joint.cuda()
    for p in joint.Vae.parameters():
        p.requires_grad = False
    joint.Vae.eval()
    M.set_kernel_dtype(joint, _dtype(dtype))
    img, lab = S.synthetic_image(2, side, seed=2).cuda(), S.synthetic_label(2, side, seed=3).cuda()
    return list(joint.Seg.parameters()), lambda: T.joint_train_losses(joint, img, lab)[0]


def _embed(side, dtype):
    import torch
    import joint_model as M
    from vae_segmentation_amd import synthetic as S, train as T
    emb = M.Embed(models=[M.Encoder(1, 128, norm_type=1, spatial=side), M.VAE(2, 2, norm_type=1, dim=128, spatial=side), M.Fusion(1, 2, 2, norm_type=1)])
    S.deterministic_fill_(emb, seed=8)
    emb = emb.cuda()
    M.set_kernel_dtype(emb, _dtype(dtype))
    img, lab = S.synthetic_image(1, side, seed=2).cuda(), S.synthetic_label(1, side, seed=3).cuda()
    noise = torch.zeros(1, 128, device="cuda")
    return list(emb.parameters()), lambda: T.embed_train_losses(emb, img, lab, noise=noise)[0]


def scenarios():
    s = {}
    for dt in ("bf16", "fp32"):
        s["seg32_" + dt] = (lambda dt=dt: _seg(32, dt), {})
        s["joint64_" + dt] = (lambda dt=dt: _joint(64, dt), {})       # 64^3: the smallest volume a VAE accepts
    s["seg96_bf16"] = (lambda: _seg(96, "bf16"), {})
    s["joint96_bf16"] = (lambda: _joint(96, "bf16"), {})
    s["embed64_fp32"] = (lambda: _embed(64, "fp32"), {})
    s["embed64_bf16"] = (lambda: _embed(64, "bf16"), {})
    s["multiclass32_c4_fp32"] = (lambda: _seg(32, "fp32", n_class=4), {})
    s["multiclass32_c4_bf16"] = (lambda: _seg(32, "bf16", n_class=4), {})
    s["seg32_bf16_up_trainable"] = (lambda: _seg(32, "bf16"), {"flags": {"FUSE_UP_TRAINABLE": True, "FUSE_UP_TRAINABLE_MIN_VOXELS": 0}})
    s["seg32_bf16_no_grouping"] = (lambda: _seg(32, "bf16"), {"grouping": False})
    s["seg32_bf16_split"] = (lambda: _seg(32, "bf16"), {"split": True})
    s["joint64_bf16_split"] = (lambda: _joint(64, "bf16"), {"split": True})
    for flag in ("FUSE_APPLY", "EPILOGUE_APPLY", "FUSE_WGRAD", "FUSE_SOFTMAX_BWD", "CHAIN"):
        s["seg32_bf16_no_" + flag] = (lambda: _seg(32, "bf16"), {"flags": {flag: False}})
    return s


def _digest(obj):
    return hashlib.sha256(json.dumps(obj, separators=(",", ":")).encode()).hexdigest()[:16]


def _bits(t):
    import torch
    return hashlib.sha256(t.detach().reshape(-1).contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def run_scenario(build, settings):
    import torch
    from vae_segmentation_amd import ops, optim
    torch.manual_seed(0)
    saved = {k: getattr(ops, k) for k in settings.get("flags", {})}
    out = {}
    try:
        for k, v in settings.get("flags", {}).items():
            setattr(ops, k, v)
        if "grouping" in settings:
            ops.set_wgrad_grouping(settings["grouping"])
        if settings.get("split"):
            ops.set_wgrad_split(lambda p: p.shape[0] <= 16)
        params, step = build()
        opt = optim.SGD(params, lr=1e-2, momentum=0.9)
        for which in ("plain", "profiled"):
            for p in params:
                p.grad = None
            prof = None
            if which == "profiled":
                prof = ops.PROFILE = []
                ops.PROFILE_PRIME_US, prime = 0, ops.PROFILE_PRIME_US
            gc.collect()
            gc.disable()                            # when the cycle collector frees a tensor decides which cached block the next allocation gets: keep it out of the pointer indices
            REC.begin()
            try:
                loss = step()
                loss.backward()
                if settings.get("split"):
                    ops.flush_wgrads()              # the caller's second phase
                if which == "plain":
                    torch.cuda.synchronize()
                    out["bits"] = {"loss": _bits(loss), "grads": _digest([None if p.grad is None else _bits(p.grad) for p in params]),
                                   "loss_value": float(loss.detach())}
                opt.step()
            finally:
                calls = REC.end()
                gc.enable()
                if prof is not None:
                    ops.PROFILE, ops.PROFILE_PRIME_US = None, prime
            torch.cuda.synchronize()
            ops.chain_fault()
            out[which] = {"calls": len(calls), "digest": _digest(calls), "trace": calls}
            if prof is not None:
                recs = [[r[0], r[1], r[2], r[3]] for r in prof]
                out[which].update({"launches": len(recs), "profile_digest": _digest(recs), "profile": recs})
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
        ops.PROFILE = None
        ops.drop_stale_wgrads()
        ops.set_wgrad_split(None)
        ops.set_wgrad_grouping(True)
    return out


def run(path, only=None):
    import torch
    install()
    result, fault = {}, False
    for name, (build, settings) in scenarios().items():
        if only and name not in only:
            continue
        try:
            result[name] = run_scenario(build, settings)
            r = result[name]
            print("%-28s plain %5d calls %s | profiled %5d calls %s, %4d launches %s | loss %s grads %s" % (
                name, r["plain"]["calls"], r["plain"]["digest"], r["profiled"]["calls"], r["profiled"]["digest"], r["profiled"]["launches"],
                r["profiled"]["profile_digest"], r["bits"]["loss"], r["bits"]["grads"]), flush=True)
        except Exception as e:                      # a scenario this revision cannot run is reported, the others still run
            result[name] = {"error": "%s: %s" % (type(e).__name__, e)}
            print("%-28s ERROR %s" % (name, result[name]["error"]), flush=True)
            if "illegal memory access" in str(e) or "HIP error" in str(e):
                fault = True                        # the device is not to be used after a fault
                break
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f)
    return 3 if fault else (1 if any("error" in r for r in result.values()) else 0)


def _nullness(trace):
    """the trace with every pointer index replaced by its null-ness"""
    def strip(v):
        if isinstance(v, list):
            return [strip(x) for x in v]
        return "p" if isinstance(v, str) and v[:1] == "p" and v != "p0" else v
    return strip(trace)


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    bad = 0
    print("%-28s %-9s %7s %-16s %7s %-16s  %s" % ("scenario", "pass", "calls A", "digest A", "calls B", "digest B", "verdict"))
    for name in a:
        ra, rb = a[name], b.get(name)
        if rb is None or "error" in ra or "error" in rb:
            print("%-28s not comparable: %s / %s" % (name, ra.get("error"), None if rb is None else rb.get("error")))
            bad += 1
            continue
        for which in ("plain", "profiled"):
            ta, tb = ra[which], rb[which]
            same = ta["trace"] == tb["trace"]
            verdict = "identical" if same else ("POINTER INDICES DIFFER" if _nullness(ta["trace"]) == _nullness(tb["trace"]) else "DIFFERENT")
            print("%-28s %-9s %7d %-16s %7d %-16s  %s" % (name, which, ta["calls"], ta["digest"], tb["calls"], tb["digest"], verdict))
            if not same:
                bad += 1
                for i, (ca, cb) in enumerate(zip(ta["trace"], tb["trace"])):
                    if ca != cb:
                        print("    first difference at call %d:\n      A %s\n      B %s" % (i, json.dumps(ca), json.dumps(cb)))
                        break
            if which == "profiled":
                same = ta["profile"] == tb["profile"]
                print("%-28s %-9s %7d %-16s %7d %-16s  %s" % (name, "profile", ta["launches"], ta["profile_digest"], tb["launches"], tb["profile_digest"],
                                                                "identical" if same else "DIFFERENT"))
                if not same:
                    bad += 1
                    for i, (ca, cb) in enumerate(zip(ta["profile"], tb["profile"])):
                        if ca != cb:
                            print("    first difference at launch %d:\n      A %s\n      B %s" % (i, ca, cb))
                            break
        same = ra["bits"] == rb["bits"]
        print("%-28s %-9s loss %s / %s, grads %s / %s  %s" % (name, "bits", ra["bits"]["loss"], rb["bits"]["loss"], ra["bits"]["grads"], rb["bits"]["grads"],
                                                            "identical" if same else "DIFFERENT"))
        bad += 0 if same else 1
    print("%d difference(s)" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        sys.exit(run(sys.argv[2], set(sys.argv[3:]) or None))
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
