"""The host answers of the grouped weight-gradient path (csrc/wgrad.hip, vs_conv_wgrad_multi) over a fixed set of descriptor lists: ctypes, integers, no tensors, no device.

usage: python tools/wgrad_plan_table.py OUT.npz            (VS_LIBVAESEG=... picks the build; default: the in-tree libvaeseg.so)
       python tools/wgrad_plan_table.py --dump-lists FILE  (the accepted lists x configurations x dtypes as raw structs, for tools/wgrad_trace.hip)

tests/golden/wgrad_plan.npz is this table made from a build of the commit BEFORE a change to the planning code; tests/test_host.py::test_wgrad_plan_answers_are_pinned
recomputes it from the loaded library and compares every entry.  The fixture is never regenerated from the code under test.

Arrays (integers only):
  multi_bytes   [K, L, 3]  vs_conv_wgrad_multi_workspace_bytes per configuration of CONFIGS, list of lists() and dtype (VS_F32, VS_BF16, VS_F16)
  single_bytes  [K, S]     vs_conv_wgrad_workspace_bytes of every distinct single layer of the lists
  singles       [S, 7]     (n, dp, hp, wp, m_ch, c_ch, kind) of those
  rejected      [R]        the code vs_conv_wgrad_multi gives each call of rejected(), default configuration
  rejected_bf16_bytes [R]  vs_conv_wgrad_multi_workspace_bytes (VS_BF16) of the rejected calls' lists: 0 unless the list itself is fine; -1: not recorded (no list,
                           or a list with slab descriptors, which the query before the planner existed sized without checking them)

Every rejected call returns before the first launch — the comment on each says where — so fake addresses are never read and the table is the same with and
without a device.
"""
import ctypes
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conv_plan_table import config_struct  # noqa: E402

VS_F32, VS_BF16, VS_F16 = 0, 1, 2
K3, K2S2, T2S2, UP, SLABS = 0, 1, 2, 3, 16
G3_GROUP_MAX, G3_RED_MAX, G3_BIAS_MAX = 24, 56, 16

# the default vs_config (no VS_* variable set) and single changes of it
CONFIGS = [{}, {"wgrad_uber": 0}, {"wgrad_mpack": 0}, {"wgrad_swap": 0}, {"wgrad_big": 0}, {"wgrad_bias_fold": 0}, {"wgrad_group_wgs": 6}, {"f32_limbs": 0}]
DTYPES = (VS_F32, VS_BF16, VS_F16)


class Desc(ctypes.Structure):
    """vs_wgrad_desc (include/vaeseg.h)"""
    _fields_ = [("p", ctypes.c_void_p), ("p_stats", ctypes.c_void_p), ("q", ctypes.c_void_p), ("q_stats", ctypes.c_void_p),
                ("dw", ctypes.c_void_p), ("bias_g", ctypes.c_void_p), ("db", ctypes.c_void_p), ("bias_rows", ctypes.c_longlong),
                ("bias_c_ch", ctypes.c_int), ("bias_c_real", ctypes.c_int),
                ("n", ctypes.c_int), ("dp", ctypes.c_int), ("hp", ctypes.c_int), ("wp", ctypes.c_int), ("m_ch", ctypes.c_int), ("c_ch", ctypes.c_int),
                ("m_real", ctypes.c_int), ("c_real", ctypes.c_int), ("kind", ctypes.c_int), ("reserved_", ctypes.c_int)]


def cpad(c):
    return 8 if c <= 8 else 16 if c <= 16 else (c + 31) // 32 * 32


class Maker:
    """descriptors with deterministic fake addresses: 16 MiB apart, 256-byte aligned, never dereferenced"""

    def __init__(self):
        self.at = 0x100000000

    def addr(self):
        self.at += 0x1000000
        return self.at

    def conv(self, kind, n, cin, cout, d, h, w, lazy=True, bias=None, dw=None, db=None):
        """one layer as ops._group_submit describes it; (d, h, w): the grid of the voxel loop (the coarse grid of the stride-2 kinds).
        k3: P = dL/dy, Q = x; k2: P = dL/dy (coarse), Q = x (fine); t2: P = x (coarse), Q = dL/dy (fine)"""
        x, gy = self.addr(), self.addr()
        stats = self.addr() if lazy else None
        dw = dw or self.addr()
        if bias is None:
            bias = kind != "k3"
        if kind == "t2":
            e = Desc(x, stats, gy, None, dw, None, None, 0, 0, 0, n, d, h, w, cpad(cin), cpad(cout), cin, cout, K2S2, 0)
            rows = n * d * h * w * 8
        else:
            e = Desc(gy, None, x, stats, dw, None, None, 0, 0, 0, n, d, h, w, cpad(cout), cpad(cin), cout, cin, K3 if kind == "k3" else K2S2, 0)
            rows = n * d * h * w
        if bias:
            e.bias_g, e.db, e.bias_rows, e.bias_c_ch, e.bias_c_real = gy, db or self.addr(), rows, cpad(cout), cout
        return e

    def up(self, n, c, co, d, h, w):
        return Desc(self.addr(), None, self.addr(), self.addr(), self.addr(), None, None, 0, 0, 0, n, d, h, w, 8 * co, cpad(c), 8 * co, c, UP, co)

    def slabs(self, nslabs, m_real=8, c_real=8, bias=False):
        e = Desc(self.addr(), None, None, None, self.addr(), None, None, 0, 0, 0, nslabs, 0, 0, 0, 8, 8, m_real, c_real, SLABS, 0)
        if bias:
            e.bias_g, e.db, e.bias_rows, e.bias_c_ch, e.bias_c_real = self.addr(), self.addr(), nslabs, m_real, m_real
        return e


def step96(m, n=2, side=96, f=(8, 16, 32, 64, 128)):
    """the 34 layers of one Segmentation step: in_block, four Down (stride-2 conv + three 3x3x3), four Up (transposed conv + three 3x3x3), out_block"""
    out = [m.conv("k3", n, 1, f[0], side, side, side, lazy=False)]
    s = side
    for a, b in zip(f[:-1], f[1:]):
        s //= 2
        out += [m.conv("k2", n, a, a, s, s, s), m.conv("k3", n, a, b, s, s, s), m.conv("k3", n, b, b, s, s, s), m.conv("k3", n, b, b, s, s, s)]
    for a, b in zip(f[:0:-1], f[-2::-1]):
        out.append(m.conv("t2", n, a, a, s, s, s))
        s *= 2
        out += [m.conv("k3", n, a, b, s, s, s), m.conv("k3", n, b, b, s, s, s), m.conv("k3", n, b, b, s, s, s)]
    out.append(m.conv("k3", n, f[0], 2, side, side, side, bias=True))
    assert len(out) == 34
    return out


def many_batches(m):
    """the list of tests/test_gpu_exact.py MANY_BATCHES: 40 + 18 weight and 18 bias reductions (> G3_RED_MAX), 18 biases (> G3_BIAS_MAX), 76 all-buckets entries"""
    return [m.conv("k3", 1, 8, 8, 4, 4, 16) for _ in range(40)] + [m.conv("k2" if i % 2 == 0 else "t2", 1, 8, 8, 2, 2, 2) for i in range(18)]


def lists():
    """-> [(name, [Desc])], every one a list vs_conv_wgrad_multi accepts under 16-bit storage (the fp32 mode refuses slab descriptors and VS_CONV_UP: 0 bytes)"""
    sys.path.insert(0, ROOT)
    try:
        from tests.test_gpu_exact import LIMB_GROUP
        from tests.test_gpu_ops import GROUP_LAYERS
    finally:
        sys.path.pop(0)
    m = Maker()
    out = [("step96", step96(m)), ("step160 B=1", step96(m, 1, 160)),
           ("GROUP_LAYERS", [m.conv(kind, n, cin, cout, *((d // 2, h // 2, w // 2) if kind == "k2" else (d, h, w))) for kind, n, cin, cout, d, h, w in GROUP_LAYERS]),
           ("LIMB_GROUP", [m.conv("k3", *case, lazy=lazy) for case, _, lazy in LIMB_GROUP])]
    dw, dw2, db2, dw3, db3 = m.addr(), m.addr(), m.addr(), m.addr(), m.addr()
    uses = [(2, 16, 16, 8, 8, 16), (2, 16, 16, 4, 6, 8), (2, 16, 16, 12, 4, 8)]
    out.append(("three uses k3", [m.conv("k3", *u, dw=dw) for u in uses]))
    out.append(("three uses of three weights", [e for u in uses for e in (m.conv("k3", *u, dw=dw), m.conv("k2", *u, dw=dw2, db=db2), m.conv("t2", *u, dw=dw3, db=db3))]
                + [m.conv("k3", 2, 32, 32, 6, 6, 6)]))
    out.append(("three uses 8 -> 8 with other layers", [m.conv("k3", 1, 8, 8, 24, 24, 24), m.conv("k3", 2, 8, 8, 16, 16, 32, dw=dw), m.conv("k2", 2, 8, 8, 4, 4, 4),
                                                        m.conv("k3", 2, 8, 8, 7, 9, 21, dw=dw), m.conv("k3", 2, 8, 8, 5, 5, 5, dw=dw)]))
    out.append(("slabs mixed in", step96(m)[1:-1] + [m.slabs(512), m.slabs(432, 2, 8, bias=True)]))
    out.append(("slabs alone", [m.slabs(512), m.slabs(27, 8, 1), m.slabs(64, 2, 8, bias=True)]))
    out.append(("one slab descriptor", [m.slabs(1)]))
    out.append(("composed Up", [m.up(2, 32, 16, 24, 24, 24), m.conv("k3", 2, 16, 16, 48, 48, 48), m.up(2, 16, 8, 12, 12, 12), m.conv("t2", 2, 32, 32, 24, 24, 24)]))
    out.append(("more than G3_GROUP_MAX in a bucket", [m.conv("k3", 2, 16, 16, 3 + i % 5, 4 + i % 3, 5 + i) for i in range(G3_GROUP_MAX + 6)]))
    out.append(("more than G3_RED_MAX", [m.conv("k3", 1, 8 << (i % 3), 8 << (i % 2), 4, 4 + i % 4, 16) for i in range(G3_RED_MAX + 4)]))
    out.append(("more than G3_BIAS_MAX", [m.conv("k2" if i % 3 else "t2", 2, 8 << (i % 4), 8 << (i % 4), 2 + i % 3, 3, 4) for i in range(G3_BIAS_MAX + 4)]))
    out.append(("MANY_BATCHES", many_batches(m)))
    out.append(("two samples of 16", [m.conv("k3", 16, 8, 8, 6, 6, 6), m.conv("k2", 16, 16, 16, 3, 3, 3)]))
    return out


def rejected():
    """-> [(name, [Desc] or None, count or None, workspace address, workspace bytes, dtype)]; csrc/wgrad.hip returns from each before its first launch:
    E = the entry checks of vs_conv_wgrad_multi; S = its loop over the slab descriptors, which ends before anything else runs; P = multi_plan, which the 16-bit
    path finishes before its first launch (every multi_validate arm, the 2 GiB bound, the shared-destination checks); V = the fp32 path's multi_validate loop
    over all descriptors; W = the workspace size and alignment checks that follow the plan.  fp32 calls whose list is valid are not here except where the
    FIRST non-empty group refuses (G): a later refusal would follow an earlier group's launch."""
    m = Maker()
    ws, big = 0x7f0000000000, 1 << 40
    ok = lambda: m.conv("k3", 2, 16, 16, 8, 8, 8)
    out = []

    def add(name, descs, dtype=VS_BF16, workspace=ws, nbytes=big, count=None):
        out.append((name, descs, count, workspace, nbytes, dtype))

    def edit(e, **kw):
        for k, v in kw.items():
            setattr(e, k, v)
        return e

    add("null descriptors", None, count=3)                                                                   # E
    add("count 0", [ok()], count=0)                                                                          # E
    add("count -1", [ok()], count=-1)                                                                        # E
    add("null workspace", [ok()], workspace=None)                                                            # E
    add("dtype 3", [ok()], dtype=3)                                                                          # E
    add("dtype -1", [ok()], dtype=-1)                                                                        # E
    add("slab descriptor under fp32", [ok(), m.slabs(8)], dtype=VS_F32)                                      # S
    add("slab descriptor alone under fp32", [m.slabs(8)], dtype=VS_F32)                                      # S
    s = m.slabs(8)
    add("slab descriptor sharing its dw with a layer", [m.conv("k3", 2, 8, 8, 8, 8, 8, dw=s.dw), s])         # S
    s = m.slabs(8)
    add("two slab descriptors sharing a dw", [s, edit(m.slabs(8), dw=s.dw)])                                 # S
    for name, kw in [("p null", dict(p=None)), ("dw null", dict(dw=None)), ("n 0", dict(n=0)), ("p at 8 bytes", dict(p=0x100008)),
                     ("m_real 0", dict(m_real=0)), ("m_real 9", dict(m_real=9)), ("c_real 0", dict(c_real=0)), ("c_real 9", dict(c_real=9)),
                     ("m_ch 16", dict(m_ch=16)), ("c_ch 16", dict(c_ch=16))]:
        add("slab descriptor: " + name, [ok(), edit(m.slabs(8), **kw)])                                      # S (slab_desc_validate)
    for name, kw in [("db null", dict(db=None)), ("bias_c_real 0", dict(bias_c_real=0)), ("bias_c_real 9", dict(bias_c_real=9)), ("bias_rows != n", dict(bias_rows=7)),
                     ("bias_g at 4 bytes", dict(bias_g=0x100004))]:
        add("slab descriptor with bias: " + name, [edit(m.slabs(8, bias=True), **kw), ok()])                 # S (slab_desc_validate)
    arms = [("p null", "k3", dict(p=None)), ("q null", "k3", dict(q=None)), ("dw null", "k3", dict(dw=None)), ("n 0", "k3", dict(n=0)), ("n 17", "k3", dict(n=17)),
            ("dp 0", "k3", dict(dp=0)), ("hp 0", "k3", dict(hp=0)), ("wp -1", "k3", dict(wp=-1)), ("m_ch 12", "k3", dict(m_ch=12, m_real=12)),
            ("c_ch 20", "k3", dict(c_ch=20)), ("m_real > m_ch", "k3", dict(m_real=17)), ("c_real > c_ch", "k3", dict(c_real=17)), ("m_real 0", "k3", dict(m_real=0)),
            ("c_real 0", "k3", dict(c_real=0)), ("kind VS_CONV_T2S2", "k3", dict(kind=T2S2)), ("kind 5", "k3", dict(kind=5)),
            ("bias without db", "k2", dict(db=None)), ("bias_rows 0", "k2", dict(bias_rows=0)), ("bias_c_real 0", "k2", dict(bias_c_real=0)),
            ("bias_c_real > bias_c_ch", "k2", dict(bias_c_real=17)), ("bias_c_ch 0", "k2", dict(bias_c_ch=0)), ("bias_c_ch 12", "k2", dict(bias_c_ch=12, bias_c_real=12)),
            ("bias_c_ch 2056", "k2", dict(bias_c_ch=2056)), ("bias_c_ch 24", "k2", dict(bias_c_ch=24))]
    for name, kind, kw in arms:
        for dtype in (VS_BF16, VS_F32):                                                                      # P (16-bit), V (fp32): multi_validate
            add("layer: %s, dtype %d" % (name, dtype), [ok(), edit(m.conv(kind, 2, 16, 16, 8, 8, 8), **kw)], dtype=dtype)
    for name, kw in [("reserved_ 0", dict(reserved_=0)), ("m_ch != 8 Co", dict(m_ch=64)), ("c_ch 8", dict(c_ch=8, c_real=8)), ("p_stats given", dict(p_stats=0x100000))]:
        for dtype in (VS_BF16, VS_F32):
            add("composed Up: %s, dtype %d" % (name, dtype), [edit(m.up(2, 32, 16, 8, 8, 8), **kw)], dtype=dtype)   # P, V
    add("P of 2 GiB", [m.conv("k3", 1, 8, 8, 512, 512, 512)])                                                # P (the 32-bit byte offsets)
    add("Q of 2 GiB, stride 2", [m.conv("k2", 1, 16, 16, 256, 256, 128)])                                    # P
    add("P of 2 GiB, fp32, the only layer", [m.conv("k3", 1, 8, 8, 512, 512, 512)], dtype=VS_F32)            # G: the plan of the first group the list fills
    add("P of 2 GiB in 4-byte elements, fp32, the only layer", [m.conv("k3", 1, 8, 8, 512, 512, 256)], dtype=VS_F32)    # G: after that group's plan and size check
    dw = m.addr()
    for name, other in [("other c_ch", m.conv("k3", 1, 16, 32, 8, 8, 8, dw=dw)), ("other kind", m.conv("k2", 1, 32, 32, 8, 8, 8, dw=dw, bias=False)),
                        ("other m_real", edit(m.conv("k3", 1, 32, 32, 8, 8, 8, dw=dw), m_real=31)), ("other channel block", m.conv("k3", 1, 8, 32, 8, 8, 8, dw=dw))]:
        add("same dw, " + name, [m.conv("k3", 1, 32, 32, 8, 8, 8, dw=dw), ok(), other])                      # P (shared-destination check)
    a = m.conv("k2", 2, 16, 16, 4, 4, 4)
    add("same db, other bias_c_real", [a, edit(m.conv("k2", 2, 16, 16, 4, 4, 4, db=a.db), bias_c_real=15)])  # P
    add("workspace of 16 bytes", [ok(), m.conv("k2", 2, 8, 8, 4, 4, 4)], nbytes=16)                         # W
    add("workspace one byte short", "step96", nbytes=-1)                                                     # W
    add("workspace of 16 bytes, fp32", [ok(), m.conv("k2", 2, 8, 8, 4, 4, 4)], dtype=VS_F32, nbytes=16)     # G: the first group's size check (3x3x3, 16-channel blocks)
    add("workspace of 16 bytes, fp32, stride-2 layers only", [m.conv("k2", 2, 8, 8, 4, 4, 4)], dtype=VS_F32, nbytes=16)    # G: the only non-empty group
    add("workspace at 8 bytes", [ok()], workspace=ws + 8)                                                    # W (after the size check)
    add("workspace at 8 bytes, fp16", [ok()], workspace=ws + 8, dtype=VS_F16)                                # W
    return out


def _array(descs):
    return (Desc * len(descs))(*descs)


def table(cdll):
    """-> the arrays of the module text; the library's configuration is put back before returning"""
    Cfg = config_struct()
    if cdll.vs_config_bytes() != ctypes.sizeof(Cfg):
        raise RuntimeError("vs_config layout mismatch")
    multi, single, launch = cdll.vs_conv_wgrad_multi_workspace_bytes, cdll.vs_conv_wgrad_workspace_bytes, cdll.vs_conv_wgrad_multi
    multi.restype, multi.argtypes = ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    single.restype, single.argtypes = ctypes.c_size_t, [ctypes.c_int] * 7
    launch.restype, launch.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float, ctypes.c_void_p]
    before, default = Cfg(), Cfg()
    if cdll.vs_get_config(ctypes.byref(before)):
        raise RuntimeError("vs_get_config failed")
    env = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("VS_")}       # the defaults, whatever this process was started with
    try:
        cdll.vs_config_from_env(ctypes.byref(default))
    finally:
        os.environ.update(env)
    named = lists()
    singles = list(dict.fromkeys((e.n, e.dp, e.hp, e.wp, e.m_ch, e.c_ch, e.kind) for _, descs in named for e in descs if e.kind in (K3, K2S2)))
    multi_bytes = np.empty((len(CONFIGS), len(named), len(DTYPES)), np.int64)
    single_bytes = np.empty((len(CONFIGS), len(singles)), np.int64)
    try:
        for k, change in enumerate(CONFIGS):
            cfg = Cfg.from_buffer_copy(default)
            for name, value in change.items():
                setattr(cfg, name, value)
            if cdll.vs_set_config(ctypes.byref(cfg)):
                raise RuntimeError("vs_set_config refused %r" % (change,))
            for i, (_, descs) in enumerate(named):
                arr = _array(descs)
                multi_bytes[k, i] = [multi(ctypes.addressof(arr), len(descs), dt) for dt in DTYPES]
            single_bytes[k] = [single(*t) for t in singles]
        cdll.vs_set_config(ctypes.byref(default))
        by_name = dict(named)
        codes, rej_bytes = [], []
        for name, descs, count, workspace, nbytes, dtype in rejected():
            if isinstance(descs, str):
                descs = by_name[descs]
            arr = _array(descs) if descs else None
            n = len(descs) if count is None else count
            need = multi(ctypes.addressof(arr), len(descs), VS_BF16) if arr is not None else -1
            if nbytes < 0:
                nbytes = need + nbytes
            codes.append(launch(ctypes.addressof(arr) if arr is not None else None, n, workspace, nbytes, dtype, 1e-5, None))
            if not -5 <= codes[-1] <= -1:                       # 0 or a HIP error: the call got as far as a launch
                raise RuntimeError("%s: code %d, not a refusal on the host" % (name, codes[-1]))
            rej_bytes.append(-1 if arr is None or any(e.kind == SLABS for e in descs) else need)
    finally:
        cdll.vs_set_config(ctypes.byref(before))
    return {"multi_bytes": multi_bytes, "single_bytes": single_bytes, "singles": np.asarray(singles, np.int32), "rejected": np.asarray(codes, np.int32),
            "rejected_bf16_bytes": np.asarray(rej_bytes, np.int64)}


def dump_lists(cdll, path):
    """every (configuration, list, dtype) as raw structs for the launch-trace program: int32 entries, then per entry int32 (dtype, count, config bytes), the
    vs_config and the descriptors"""
    Cfg = config_struct()
    default = Cfg()
    env = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("VS_")}
    try:
        cdll.vs_config_from_env(ctypes.byref(default))
    finally:
        os.environ.update(env)
    named = lists()
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(CONFIGS) * len(named) * len(DTYPES)))
        for change in CONFIGS:
            cfg = Cfg.from_buffer_copy(default)
            for name, value in change.items():
                setattr(cfg, name, value)
            for _, descs in named:
                for dt in DTYPES:
                    f.write(struct.pack("iii", dt, len(descs), ctypes.sizeof(cfg)))
                    f.write(bytes(cfg))
                    f.write(bytes(_array(descs)))


def report(t):
    named = lists()
    print("%d lists x %d configurations x %d dtypes, %d single layers, %d rejected calls" % (len(named), len(CONFIGS), len(DTYPES), len(t["singles"]), len(t["rejected"])))
    for i, (name, descs) in enumerate(named):
        print("%-40s %3d descriptors  fp32 %11d  bf16 %11d  fp16 %11d bytes by default" % ((name, len(descs)) + tuple(int(v) for v in t["multi_bytes"][0, i])))
    for k, change in enumerate(CONFIGS[1:], 1):
        print("%-22s %3d answers differ" % (", ".join("%s=%d" % kv for kv in change.items()), int((t["multi_bytes"][k] != t["multi_bytes"][0]).sum())))
    for (name, *_), code in zip(rejected(), t["rejected"]):
        print("%4d  %s" % (code, name))


def main():
    path = os.environ.get("VS_LIBVAESEG") or os.path.join(ROOT, "vae_segmentation_amd", "libvaeseg.so")
    cdll = ctypes.CDLL(path)
    if sys.argv[1] == "--dump-lists":
        dump_lists(cdll, sys.argv[2])
        return
    if sys.argv[1] == "--time":                   # host time of the size query over the 34-layer list: five repeats of 1000 calls, microseconds per call
        import json
        import time
        multi = cdll.vs_conv_wgrad_multi_workspace_bytes
        multi.restype, multi.argtypes = ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        arr = _array(lists()[0][1])
        out = {}
        for name, dt in (("fp32", VS_F32), ("bf16", VS_BF16)):
            reps = []
            for _ in range(6):                    # the first repeat warms up and is dropped
                t0 = time.perf_counter()
                for _ in range(1000):
                    multi(ctypes.addressof(arr), len(arr), dt)
                reps.append((time.perf_counter() - t0) * 1e3)
            out[name] = {"us_per_call": [round(r, 3) for r in reps[1:]], "median": round(sorted(reps[1:])[2], 3)}
        print(json.dumps(out))
        return
    t = table(cdll)
    report(t)
    np.savez_compressed(sys.argv[1], **t)


if __name__ == "__main__":
    main()
