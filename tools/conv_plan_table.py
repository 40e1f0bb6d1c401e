"""The answers of the convolution launch planner (csrc/conv_api.hip) over a grid of shapes, from the library's host queries alone: ctypes, no tensors, no device.

usage: python tools/conv_plan_table.py OUT.npz            (VS_LIBVAESEG=... picks the build; default: the in-tree libvaeseg.so)

tests/golden/conv_plan.npz is this table made from a build of the commit BEFORE a planner change; tests/test_host.py::test_conv_plan_answers_are_pinned
recomputes it from the loaded library and compares every entry.  The fixture is never regenerated from the code under test.

Arrays (integers only):
  tuples   [T, 7]      (n, d, h, w, c, m, dtype) in grid order
  answers  [K, T, 7]   per configuration of CONFIGS and tuple, the queries of QUERIES in order
"""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the default vs_config (no VS_* variable set) and single changes of it
CONFIGS = [{}, {"k3_small": 0}, {"k3_tall": 0}, {"k3_tall": 1}, {"mt_min_wgs": 256}, {"f32_limbs": 0}, {"k3x_ck": 16}, {"k3x_toeplitz": 0},
           {"epilogue_apply": 0}, {"fuse_wgrad": 0}, {"k3_short_tiles": 0}]
QUERIES = ["k3_fused_apply lazy=0", "k3_fused_apply lazy=1", "k3_bwd_data_applied", "s2_bwd_data_applied scatter=0", "s2_bwd_data_applied scatter=1",
           "k3_bwd_data_wgrad", "k3_f32_limbs"]


def grid():
    out, seen = [], set()
    for n in (1, 2, 4, 13):
        for s in (1, 2, 3, 4, 6, 7, 8, 12, 16, 24, 48, 96):
            for d, h, w in ((s, s, s), (s, 2 * s, s + 1)):
                for c in (8, 16, 32, 64, 128, 256, 512, 24):
                    for m in (c, max(8, c // 2), min(512, 2 * c)):
                        for dtype in (0, 1, 2):
                            t = (n, d, h, w, c, m, dtype)
                            if t not in seen:
                                seen.add(t)
                                out.append(t)
    return out


def config_struct():
    """ctypes mirror of vs_config, read from include/vaeseg.h"""
    src = open(os.path.join(ROOT, "include", "vaeseg.h")).read()
    body = re.search(r"typedef\s+struct\s+vs_config\s*\{(.*?)\}\s*vs_config\s*;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    kinds = {"int": ctypes.c_int, "long long": ctypes.c_longlong}
    fields = [(m.group(2), kinds[m.group(1)]) for m in re.finditer(r"\b(int|long long)\s+(\w+)\s*;", body)]
    return type("VsConfig", (ctypes.Structure,), {"_fields_": fields})


def answers(cdll, tuples):
    q = [cdll.vs_conv_k3_fused_apply_supported, cdll.vs_conv_k3_bwd_data_applied_supported, cdll.vs_conv_s2_bwd_data_applied_supported,
         cdll.vs_conv_k3_bwd_data_wgrad_supported, cdll.vs_conv_k3_f32_limbs]
    for f, nargs in zip(q, (8, 7, 8, 7, 4)):
        f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int] * nargs
    fa, ea, s2, wg, limbs = q
    out = np.empty((len(tuples), len(QUERIES)), np.int8)
    for i, (n, d, h, w, c, m, dt) in enumerate(tuples):
        out[i] = (fa(n, d, h, w, c, m, 0, dt), fa(n, d, h, w, c, m, 1, dt), ea(n, d, h, w, c, m, dt), s2(n, d, h, w, c, m, 0, dt),
                  s2(n, d, h, w, c, m, 1, dt), wg(n, d, h, w, c, m, dt), limbs(d, h, w, c))
    return out


def table(cdll):
    """-> {"tuples": [T, 7] int32, "answers": [K, T, 7] int8}; the library's configuration is put back before returning"""
    Cfg = config_struct()
    if cdll.vs_config_bytes() != ctypes.sizeof(Cfg):
        raise RuntimeError("vs_config layout mismatch")
    before, default = Cfg(), Cfg()
    if cdll.vs_get_config(ctypes.byref(before)):
        raise RuntimeError("vs_get_config failed")
    env = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("VS_")}       # the defaults, whatever this process was started with
    try:
        cdll.vs_config_from_env(ctypes.byref(default))
    finally:
        os.environ.update(env)
    tuples = grid()
    out = np.empty((len(CONFIGS), len(tuples), len(QUERIES)), np.int8)
    try:
        for k, change in enumerate(CONFIGS):
            cfg = Cfg.from_buffer_copy(default)
            for name, value in change.items():
                setattr(cfg, name, value)
            if cdll.vs_set_config(ctypes.byref(cfg)):
                raise RuntimeError("vs_set_config refused %r" % (change,))
            out[k] = answers(cdll, tuples)
    finally:
        cdll.vs_set_config(ctypes.byref(before))
    return {"tuples": np.asarray(tuples, np.int32), "answers": out}


def report(t):
    a = t["answers"]
    print("%d tuples" % len(t["tuples"]))
    for j, name in enumerate(QUERIES[:6]):
        print("default  %-32s %5d answer 1" % (name, int((a[0, :, j] == 1).sum())))
    for k, change in enumerate(CONFIGS[1:], 1):
        print("%-22s %5d tuples differ" % (", ".join("%s=%d" % kv for kv in change.items()), int((a[k, :, :6] != a[0, :, :6]).any(axis=1).sum())))


def main():
    path = os.environ.get("VS_LIBVAESEG") or os.path.join(ROOT, "vae_segmentation_amd", "libvaeseg.so")
    t = table(ctypes.CDLL(path))
    report(t)
    np.savez_compressed(sys.argv[1], **t)


if __name__ == "__main__":
    main()
