"""Integer test data and plain fp64 references for the convolution kernels, for comparisons WITHOUT a tolerance (tests/test_gpu_exact.py; pinned on the
host by tests/test_host_exact.py).  CPU only, fp64, no import of the package.

Why it works: every kernel multiplies stored operands and accumulates in fp32.  Small integers are exact in bf16, fp16 and fp32 (and have a single non-zero
limb in the three-limb fp32 kernels); while every partial sum of an output stays below 2^24 in magnitude, fp32 accumulation is exact in ANY order — any
tile walk, split-K, slab reduction or atomics order.  The result must then EQUAL the fp64 reference (after one round-to-nearest-even where it is stored in 16 bits).
Operands with two and three non-zero limbs — what the fp32 kernels' limb planes 1 and 2, the limb fragments of the packed weights and the second
accumulator carry — are the last section (LimbCase).

Lazy (InstanceNorm + ReLU fused) inputs: every (n, c) plane of the raw tensor gets mean exactly 0 and variance exactly 4 (unit_planes), so
relu((x - mean) * rstd) is one of {0, 0.5, 1, 2}.  Such operands are integer multiples of `unit` = 0.5; everything below is stated in units, i.e. the bound on
a sum of products is 2^24 * unit and on a sum of squares 2^24 * unit^2 (scaling by a power of two changes nothing in binary floating point).

The precondition (assert_exact_precondition), asserted for every case and never used to skip one:
  * for every output entry, sum_i |a_i| |b_i| < 2^24 * unit — checked through upper bounds of that sum (dot_bounds_*), which are cheap and sufficient;
  * for the epilogue statistics, per (n, c): sum |y| < 2^24 * unit and sum y^2 < 2^24 * unit^2 for the stored y of every storage type (the epilogues hold
    fp32 partial sums of the stored values and of their squares).

How the amplitudes are chosen (plan_k3 / plan_k2): A = amplitude_for(most products of any output) is the worst-case bound — 27 Cin (forward), 27 Cout
(backward data), N * voxels (weight gradient); it gives A^2 < 28 for the weight gradient of (4, 8, 8, 24, 48, 128), < 64 for (2, 16, 16, 32, 64, 64), < 2427
for a 256-channel forward.  The statistics bound is on a sum over the whole plane, E[sum y^2] = voxels * 27 Cin * E[a^2] * E[w^2]: the activation and
weight amplitudes are lowered together until that expectation is a third of the limit, and where amplitude 1 is still too much the WEIGHTS become
sparse ternary (activations and output gradients stay dense, so every product of a weight gradient is non-zero).
How sparse: the large shapes keep 1.2 % to 3 % of their weights with a lazy input — (2, 16, 16, 32, 64, 64) 1.2 %, (1, 8, 8, 32, 100, 48) 2.1 %,
(4, 8, 8, 24, 48, 128) and (2, 8, 8, 48, 48, 64) 2.2 % — and 10 % to 23 % with a materialised one: about five non-zero products per output, so y and gx of
those data sets would miss most single dropped (tap, channel) products.  Every case whose weights come out sparse therefore has a DENSE twin
(K3Case(..., dense=True): every weight non-zero, amplitudes from the worst-case bound alone) whose y, gx and dW are compared exactly and whose statistics
are not (their plane sums pass 2^24); the sparse set keeps the statistics.  tests/test_host_exact.py holds the densities to these figures."""
import functools
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
LIMIT = float(2 ** 24)
STORAGE = (torch.float32, torch.bfloat16, torch.float16)
LARGE_WGRAD = 2 ** 18          # a weight gradient summed over this many voxels or more takes amplitudes 1..2 (its bound allows A^2 < 64), elsewhere up to 8


# ------------------------------------------------------------------------------------------------ data makers
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def ints(shape, amp, seed, density=1.0):
    """fp64 tensor of integers: non-zero values uniform in +-{1..amp} (dense: no zero anywhere, so dropping ANY product changes a sum); density < 1 keeps that
    fraction and zeroes the rest (amp 1: sparse ternary)."""
    g = _gen(seed)
    shape = tuple(shape)
    v = torch.randint(1, int(amp) + 1, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g) < density)
    return v.to(F64)


def plane_values(v, kind):
    """the multiset of one zero-mean, variance-4 plane of v voxels: sum = 0, sum of squares = 4 v exactly"""
    if kind == "pm2":
        assert v % 2 == 0
        return [2.0] * (v // 2) + [-2.0] * (v // 2)
    if kind == "pm4":
        assert v % 8 == 0
        return [4.0] * (v // 8) + [-4.0] * (v // 8) + [0.0] * (v - v // 4)
    assert kind == "odd" and v % 2 == 1 and v >= 5, "no zero-mean variance-4 integer plane of %d voxels" % v
    return [2.0] * ((v - 5) // 2) + [-2.0] * ((v - 5) // 2) + [1.0, 1.0, 1.0, 1.0, -4.0]


def plane_kind(v, channel):
    if v % 2:
        return "odd"
    return "pm4" if v % 8 == 0 and channel % 2 == 1 else "pm2"


def unit_planes(n, c, vol, seed):
    """(n, c, *vol) fp64: every (n, c) plane a shuffle of plane_values — the patterns mixed over the channels"""
    v = int(math.prod(vol))
    base = torch.tensor([plane_values(v, plane_kind(v, j)) for j in range(c)], dtype=F64)
    perm = torch.rand(n, c, v, generator=_gen(seed)).argsort(-1)
    return base.expand(n, c, v).gather(2, perm).reshape(n, c, *vol)


def in_relu_exact(x):
    """relu(InstanceNorm(x)) of a unit_planes tensor at eps = 0: mean 0, rstd 1/2"""
    return torch.relu(x * 0.5)


def staged(x, dtype, eps, rstd_scale=1.0):
    """The normalised activation as a kernel stages it: fp32 arithmetic with rstd = fp32(1 / sqrt(4 + eps)) [times rstd_scale: the 16-bit kernels form it by
    rsqrt + one Newton step, ~1e-7 relative], ReLU, one rounding to the storage type."""
    rstd = torch.tensor(1.0 / math.sqrt(4.0 + eps), dtype=F64).float() * torch.tensor(rstd_scale, dtype=torch.float32)
    return torch.relu(x.float() * rstd).to(dtype).double()


def amplitude_for(products, other=None, cap=8):
    """the largest integer A <= cap with products * A * (other or A) < 2^24: an output that sums `products` products of operands bounded by A (and `other`,
    in units) has no partial sum at or above 2^24"""
    for a in range(int(cap), 0, -1):
        if products * a * (a if other is None else other) < LIMIT:
            return a
    raise AssertionError("no amplitude keeps %d products below 2^24" % products)


def _m2(a):
    """E[v^2] of ints(..., a): mean of 1^2 .. a^2"""
    return (a + 1) * (2 * a + 1) / 6.0


def plan_k3(case, lazy):
    """-> dict(A, ax, aw, pw) for a 3x3x3 case (N, Cin, Cout, D, H, W): A bounds the output gradient (and everything else); ax / aw / pw are the activation
    amplitude (materialised input), the weight amplitude and the weight density that keep the expected plane sum of y^2 at a third of its limit."""
    n, cin, cout, d, h, w = case
    vox = d * h * w
    a = amplitude_for(max(27 * cin, 27 * cout, n * vox), other=4 if lazy else None, cap=2 if n * vox >= LARGE_WGRAD else 8)
    if lazy:
        # E[a^2] = 1/2, plus the part of the mean: (E[a] * sum of the row's weights)^2 with E[a] <= 1/2 — a random-sign row sum squared averages the row's
        # energy, but the worst of up to 256 rows reaches about six times that
        t = LIMIT * 0.25 / (3.0 * vox * 27 * cin * (0.5 + 6 * 0.25))
        fit = [k for k in range(1, a + 1) if _m2(k) <= t]
        return dict(A=a, ax=None, aw=max(fit) if fit else 1, pw=1.0 if fit else t)
    t = LIMIT / (3.0 * vox * 27 * cin)
    fit = [k for k in range(1, a + 1) if _m2(k) ** 2 <= t]
    return dict(A=a, ax=max(fit) if fit else 1, aw=max(fit) if fit else 1, pw=1.0 if fit else t)


# ------------------------------------------------------------------------------------------------ plain fp64 references (planar tensors N, C, D, H, W)
def _cl(x):
    return x.permute(0, 2, 3, 4, 1)


def _planar(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


def _taps(k):
    return [(kz, ky, kx) for kz in range(k) for ky in range(k) for kx in range(k)]


def _row(xp, z0, y0, x0s, d, h, wd):
    """three x-taps of one (z, y) tap row side by side: (N, D, H, W, 3 C) from the padded channels-last tensor, channel index j * C + c for x offset x0s[j]
    (one product of depth 3 C per row instead of three of depth C: the references of the 8-channel layers spend their time in these copies)"""
    r = xp[:, z0:z0 + d, y0:y0 + h]
    return torch.cat([r[:, :, :, x0:x0 + wd] for x0 in x0s], -1)


def conv3d_k3(x, w):
    """y[n, m, v] = sum_{c, k} x[n, c, v + k - 1] w[m, c, k], zero outside the volume"""
    n, c, d, h, wd = x.shape
    xp = _cl(F.pad(x, (1, 1, 1, 1, 1, 1)))
    y = torch.zeros(n, d, h, wd, w.shape[0], dtype=F64)
    for kz in range(3):
        for ky in range(3):
            y += _row(xp, kz, ky, (0, 1, 2), d, h, wd) @ w[:, :, kz, ky].permute(2, 1, 0).reshape(3 * c, -1)
    return _planar(y)


def conv3d_k3_bwd_data(gy, w):
    """gx[n, c, u] = sum_{m, k} gy[n, m, u - k + 1] w[m, c, k]"""
    n, m, d, h, wd = gy.shape
    gp = _cl(F.pad(gy, (1, 1, 1, 1, 1, 1)))
    gx = torch.zeros(n, d, h, wd, w.shape[1], dtype=F64)
    for kz in range(3):
        for ky in range(3):
            gx += _row(gp, 2 - kz, 2 - ky, (2, 1, 0), d, h, wd) @ w[:, :, kz, ky].permute(2, 0, 1).reshape(3 * m, -1)
    return _planar(gx)


def conv3d_k3_wgrad(x, gy):
    """dW[m, c, k] = sum_{n, v} gy[n, m, v] x[n, c, v + k - 1]"""
    n, c, d, h, wd = x.shape
    m = gy.shape[1]
    xp = _cl(F.pad(x, (1, 1, 1, 1, 1, 1)))
    g2 = _cl(gy).reshape(-1, m).t().contiguous()
    dw = torch.zeros(m, c, 3, 3, 3, dtype=F64)
    for kz in range(3):
        for ky in range(3):
            dw[:, :, kz, ky] = (g2 @ _row(xp, kz, ky, (0, 1, 2), d, h, wd).reshape(-1, 3 * c)).view(m, 3, c).transpose(1, 2)
    return dw


def _fine(x, k, do, ho, wo):
    """the voxels 2 o + k of a fine tensor, o over the coarse grid (a floor-halved grid ignores an odd last plane)"""
    kz, ky, kx = k
    return x[:, :, kz:2 * do:2, ky:2 * ho:2, kx:2 * wo:2]


def conv3d_k2s2(x, w, b=None):
    """y[n, m, o] = b[m] + sum_{c, k} x[n, c, 2 o + k] w[m, c, k]"""
    n, c, d, h, wd = x.shape
    do, ho, wo = d // 2, h // 2, wd // 2
    y = torch.zeros(n, do, ho, wo, w.shape[0], dtype=F64)
    for k in _taps(2):
        y += _cl(_fine(x, k, do, ho, wo)) @ w[:, :, k[0], k[1], k[2]].t()
    if b is not None:
        y += b
    return _planar(y)


def conv3d_k2s2_bwd_data(gy, w, fine_shape):
    """gx[n, c, 2 o + k] = sum_m gy[n, m, o] w[m, c, k]; fine voxels no output reads get 0"""
    n, m, do, ho, wo = gy.shape
    gx = torch.zeros(n, w.shape[1], *fine_shape, dtype=F64)
    for k in _taps(2):
        _fine(gx, k, do, ho, wo).copy_(_planar(_cl(gy) @ w[:, :, k[0], k[1], k[2]]))
    return gx


def conv3d_k2s2_wgrad(x, gy):
    """dW[m, c, k] = sum_{n, o} gy[n, m, o] x[n, c, 2 o + k];  db[m] = sum_{n, o} gy[n, m, o]"""
    n, m, do, ho, wo = gy.shape
    c = x.shape[1]
    g2 = _cl(gy).reshape(-1, m).t().contiguous()
    dw = torch.zeros(m, c, 2, 2, 2, dtype=F64)
    for k in _taps(2):
        dw[:, :, k[0], k[1], k[2]] = g2 @ _cl(_fine(x, k, do, ho, wo)).reshape(-1, c)
    return dw, gy.sum((0, 2, 3, 4))


def conv_transpose3d_k2s2(x, w, b=None):
    """w: (Cin, Cout, 2, 2, 2).  y[n, m, 2 i + k] = b[m] + sum_c x[n, c, i] w[c, m, k]"""
    n, c, d, h, wd = x.shape
    y = torch.zeros(n, w.shape[1], 2 * d, 2 * h, 2 * wd, dtype=F64)
    for k in _taps(2):
        _fine(y, k, d, h, wd).copy_(_planar(_cl(x) @ w[:, :, k[0], k[1], k[2]]))
    if b is not None:
        y += b.view(1, -1, 1, 1, 1)
    return y


def conv_transpose3d_k2s2_bwd_data(gy, w):
    """gx[n, c, i] = sum_{m, k} gy[n, m, 2 i + k] w[c, m, k]"""
    n, m, d2, h2, w2 = gy.shape
    d, h, wd = d2 // 2, h2 // 2, w2 // 2
    gx = torch.zeros(n, d, h, wd, w.shape[0], dtype=F64)
    for k in _taps(2):
        gx += _cl(_fine(gy, k, d, h, wd)) @ w[:, :, k[0], k[1], k[2]].t()
    return _planar(gx)


def conv_transpose3d_k2s2_wgrad(x, gy):
    """dW[c, m, k] = sum_{n, i} x[n, c, i] gy[n, m, 2 i + k];  db[m] = sum gy[n, m, :]"""
    n, c, d, h, wd = x.shape
    m = gy.shape[1]
    x2 = _cl(x).reshape(-1, c).t().contiguous()
    dw = torch.zeros(c, m, 2, 2, 2, dtype=F64)
    for k in _taps(2):
        dw[:, :, k[0], k[1], k[2]] = x2 @ _cl(_fine(gy, k, d, h, wd)).reshape(-1, m)
    return dw, gy.sum((0, 2, 3, 4))


def plane_stats(y):
    """(N, C, 2): sum and sum of squares of every (n, c) plane — the epilogue statistics of a stored result"""
    y = y.double()
    return torch.stack((y.sum((2, 3, 4)), (y * y).sum((2, 3, 4))), -1)


def stored(ref, dtype):
    """an exact fp64 result as the kernel stores it: one round-to-nearest-even to the storage type (csrc/common.h pack2); fp32 holds it exactly"""
    out = ref.to(dtype)
    if dtype == torch.float32:
        assert torch.equal(out.double(), ref), "the exact result does not fit fp32: the precondition was not checked"
    return out


# ------------------------------------------------------------------------------------------------ the precondition
def _bound(a_max, b_rows):
    """max over outputs of sum |a| |b| <= max |a| * (the largest absolute row sum of b)"""
    return float(a_max) * float(b_rows.max())


def dot_bounds_gather(a, w, gy, b=None, transposed=False):
    """Upper bounds of sum_i |a_i| |b_i| over the products of ONE output entry, for a convolution (w: (M, C, taps...)) or — transposed — a 2x2x2 transposed
    convolution (w: (C, M, taps...): one tap per fine voxel).  -> dict y / gx / dw / db."""
    aw = w.abs()
    amax, gmax = a.abs().max(), gy.abs().max()
    if transposed:
        y_rows, gx_rows = aw.sum(0).amax((1, 2, 3)), aw.sum((1, 2, 3, 4))
    else:
        y_rows, gx_rows = aw.sum((1, 2, 3, 4)), aw.sum((0, 2, 3, 4))
    a_planes, g_planes = a.abs().sum((0, 2, 3, 4)), gy.abs().sum((0, 2, 3, 4))
    out = {"y": _bound(amax, y_rows) + (0.0 if b is None else float(b.abs().max())), "gx": _bound(gmax, gx_rows),
           "dw": min(_bound(gmax, a_planes), _bound(amax, g_planes)), "db": float(g_planes.max())}
    return out


def assert_exact_precondition(name, dots, unit=1.0, y=None):
    """dots: {label: upper bound of sum |a_i||b_i| over an output's products}; y: the exact result whose epilogue statistics are compared (or None).
    Raises AssertionError — a case that cannot meet the precondition is an error of the case list, never skipped."""
    for label, bound in dots.items():
        assert bound < LIMIT * unit, "%s: %s may reach %.0f units, not below 2^24" % (name, label, bound / unit)
    if y is not None:
        for dtype in STORAGE:
            st = plane_stats(y.to(dtype))
            s1, s2 = float(y.to(dtype).double().abs().sum((2, 3, 4)).max()), float(st[..., 1].max())
            assert s1 < LIMIT * unit, "%s: a plane's sum |y| is %.0f units (%s), not below 2^24" % (name, s1 / unit, dtype)
            assert s2 < LIMIT * unit * unit, "%s: a plane's sum y^2 is %.0f square units (%s), not below 2^24" % (name, s2 / unit ** 2, dtype)


# ------------------------------------------------------------------------------------------------ cases: data + references, built once and shared
class _Case:
    """x: the raw input (lazy: unit_planes); a: what the convolution multiplies (lazy: in_relu_exact(x)); w, b, gy; references as cached properties"""
    with_stats = False
    transposed = False

    def check(self):
        dots = dot_bounds_gather(self.a, self.w, self.gy, self.b, self.transposed)
        assert_exact_precondition(self.name, dots, self.unit, self.y if self.with_stats else None)
        return self

    @functools.cached_property
    def stats(self):
        return {dt: plane_stats(stored(self.y, dt)) for dt in STORAGE}


class K3Case(_Case):
    """3x3x3, padding 1, no bias: case = (N, Cin, Cout, D, H, W)"""
    with_stats = True

    def __init__(self, case, lazy, seed=0, dense=False):
        n, cin, cout, d, h, w = case
        self.case, self.lazy, self.unit, self.b = case, lazy, (0.5 if lazy else 1.0), None
        self.name = "k3 %s %s%s" % (case, "lazy" if lazy else "materialised", ", dense weights" if dense else "")
        self.plan = p = plan_k3(case, lazy)
        if dense:                                 # no statistics: nothing but the worst-case bound on a sum of products limits the amplitudes
            self.with_stats = False
            self.plan = p = dict(A=p["A"], ax=None if lazy else p["A"], aw=p["A"], pw=1.0)
        self.x = unit_planes(n, cin, (d, h, w), seed + 1) if lazy else ints((n, cin, d, h, w), p["ax"], seed + 1)
        self.a = in_relu_exact(self.x) if lazy else self.x
        self.w = ints((cout, cin, 3, 3, 3), p["aw"], seed + 2, p["pw"])
        self.gy = ints((n, cout, d, h, w), p["A"], seed + 3)

    y = functools.cached_property(lambda self: conv3d_k3(self.a, self.w))
    gx = functools.cached_property(lambda self: conv3d_k3_bwd_data(self.gy, self.w))
    dw = functools.cached_property(lambda self: conv3d_k3_wgrad(self.a, self.gy))


def plan_k2(n, coarse_vox, c_in_per_out, c_bwd, lazy):
    return amplitude_for(max(c_in_per_out + 1, c_bwd, n * coarse_vox * 8), other=4 if lazy else None)


class K2Case(_Case):
    """Conv3d(C, Co, 2, stride 2) with bias: case = (N, Cin, Cout, D, H, W)"""

    def __init__(self, case, lazy, seed=0):
        n, cin, cout, d, h, w = case
        self.case, self.lazy, self.unit = case, lazy, (0.5 if lazy else 1.0)
        self.name = "k2s2 %s %s" % (case, "lazy" if lazy else "materialised")
        amp = plan_k2(n, (d // 2) * (h // 2) * (w // 2), 8 * cin, cout, lazy)
        self.plan = dict(A=amp)
        self.x = unit_planes(n, cin, (d, h, w), seed + 1) if lazy else ints((n, cin, d, h, w), amp, seed + 1)
        self.a = in_relu_exact(self.x) if lazy else self.x
        self.w, self.b = ints((cout, cin, 2, 2, 2), amp, seed + 2), ints((cout,), amp, seed + 4)
        self.gy = ints((n, cout, d // 2, h // 2, w // 2), amp, seed + 3)

    y = functools.cached_property(lambda self: conv3d_k2s2(self.a, self.w, self.b))
    gx = functools.cached_property(lambda self: conv3d_k2s2_bwd_data(self.gy, self.w, self.x.shape[2:]))
    dw = functools.cached_property(lambda self: conv3d_k2s2_wgrad(self.a, self.gy)[0])
    db = functools.cached_property(lambda self: conv3d_k2s2_wgrad(self.a, self.gy)[1])


class T2Case(_Case):
    """ConvTranspose3d(C, Co, 2, stride 2) with bias: case = (N, Cin, Cout, D, H, W) of the COARSE input"""
    transposed = True

    def __init__(self, case, lazy, seed=0):
        n, cin, cout, d, h, w = case
        self.case, self.lazy, self.unit = case, lazy, (0.5 if lazy else 1.0)
        self.name = "t2s2 %s %s" % (case, "lazy" if lazy else "materialised")
        amp = plan_k2(n, d * h * w, cin, 8 * cout, lazy)
        self.plan = dict(A=amp)
        self.x = unit_planes(n, cin, (d, h, w), seed + 1) if lazy else ints((n, cin, d, h, w), amp, seed + 1)
        self.a = in_relu_exact(self.x) if lazy else self.x
        self.w, self.b = ints((cin, cout, 2, 2, 2), amp, seed + 2), ints((cout,), amp, seed + 4)
        self.gy = ints((n, cout, 2 * d, 2 * h, 2 * w), amp, seed + 3)

    y = functools.cached_property(lambda self: conv_transpose3d_k2s2(self.a, self.w, self.b))
    gx = functools.cached_property(lambda self: conv_transpose3d_k2s2_bwd_data(self.gy, self.w))
    dw = functools.cached_property(lambda self: conv_transpose3d_k2s2_wgrad(self.a, self.gy)[0])
    db = functools.cached_property(lambda self: conv_transpose3d_k2s2_wgrad(self.a, self.gy)[1])


# ------------------------------------------------------------------------------------------------ operands with several non-zero limbs (fp32 limb kernels)
# The fp32 parity mode splits each fp32 operand into three bf16 limbs by round-to-nearest (csrc/common.h vs_limb_split4; pack.hip for the weights) and keeps six
# of the nine limb products: x0 w0 + x0 w1 + x1 w0 + x0 w2 + x1 w1 + x2 w0.  The small integers above have one limb, so limb planes 1 and 2 carry zeros in those
# cases.  Here the operands are integers with two or three non-zero limbs, paired so that the three DROPPED products (x1 w2, x2 w1, x2 w2) are identically zero:
# a three-limb operand only ever meets a one-limb one, a two-limb operand a two-limb one.  The kept products are then all of x * w, every limb is an integer
# (times the unit), and while sum |x_l| |w_l'| over an output's products and kept limb pairs stays below 2^24 every partial sum of any accumulator arrangement —
# one accumulator or two, any tile walk, split-K, slabs, atomics — is an exact integer: the result must EQUAL the plain fp64 convolution, which stays the reference.
# That sum is taken over the limbs: with the dropped products zero it equals (sum_l |x_l|) * (sum_l' |w_l'|) summed over the products, and limbs of mixed sign
# make it slightly larger than sum |x| |w|.
ROLES = ("x3", "w3", "g3", "22")
THREE_BITS, TWO_BITS = (17, 19), (9, 10)
REDRAW_ROUNDS = 50


def bf16_rne(x):
    """round-to-nearest-even to bf16, as v_cvt_pk_bf16_f32 does it; x must be exact in fp32"""
    f = x.float()
    assert torch.equal(f.double(), x), "not exact in fp32"
    return f.to(torch.bfloat16).double()


def limbs_of(x):
    """the three bf16 limbs of an fp64 tensor of fp32 values, as common.h forms them: l0 = rne(x), l1 = rne(x - l0), l2 = rne(x - l0 - l1)"""
    l0 = bf16_rne(x)
    l1 = bf16_rne(x - l0)
    l2 = bf16_rne(x - l0 - l1)
    assert torch.equal(l0 + l1 + l2, x), "three bf16 limbs do not hold the value"
    return l0, l1, l2


def limb_abs(x):
    """sum_l |x_l|: what an entry can contribute to a partial sum, per unit of the other operand's limbs"""
    l0, l1, l2 = limbs_of(x)
    return l0.abs() + l1.abs() + l2.abs()


def limb_class_ok(v, limbs):
    """per entry: does v have exactly `limbs` (2 or 3) non-zero limbs — limb 1 non-zero, limb 2 non-zero (three) or zero (two)"""
    _, l1, l2 = limbs_of(v)
    return (l1 != 0) & ((l2 != 0) if limbs == 3 else (l2 == 0))


def limb_ints(shape, limbs, seed, density=1.0):
    """fp64 integers with exactly `limbs` non-zero limbs in EVERY non-zero entry: 3 -> 17 to 19 bits, 2 -> 9 to 10 bits, random sign.  Entries that miss the
    condition are drawn again (REDRAW_ROUNDS at the most: it is a condition, not a share); density < 1 zeroes the rest."""
    g = _gen(seed)
    shape = tuple(shape)
    lo, hi = THREE_BITS if limbs == 3 else TWO_BITS

    def draw(count):
        return (torch.randint(2 ** (lo - 1), 2 ** hi, (count,), generator=g) * (torch.randint(0, 2, (count,), generator=g) * 2 - 1)).to(F64)
    keep = (torch.rand(shape, generator=g) < density).reshape(-1).nonzero().view(-1) if density < 1.0 else torch.arange(math.prod(shape))
    vals = draw(keep.numel())
    bad = (~limb_class_ok(vals, limbs)).nonzero().view(-1)
    for _ in range(REDRAW_ROUNDS):
        if bad.numel() == 0:
            break
        new = draw(bad.numel())
        vals[bad] = new
        bad = bad[~limb_class_ok(new, limbs)]
    assert bool(limb_class_ok(vals, limbs).all()), "%d redraw rounds left entries without %d non-zero limbs" % (REDRAW_ROUNDS, limbs)
    v = torch.zeros(math.prod(shape), dtype=F64)
    v[keep] = vals
    return v.view(shape)


def _k2_wgrad(x, gy):
    return conv3d_k2s2_wgrad(x, gy)[0]


def _t2_wgrad(x, gy):
    return conv_transpose3d_k2s2_wgrad(x, gy)[0]


# kind -> (forward, backward data, weight gradient) on planar fp64 tensors; the bias is added apart
_LIMB_REFS = {"k3": (conv3d_k3, lambda gy, w, fine: conv3d_k3_bwd_data(gy, w), conv3d_k3_wgrad),
              "k2": (conv3d_k2s2, conv3d_k2s2_bwd_data, _k2_wgrad),
              "t2": (conv_transpose3d_k2s2, lambda gy, w, fine: conv_transpose3d_k2s2_bwd_data(gy, w), _t2_wgrad)}


def dot_bounds_limbs(kind, a, w, gy, b=None):
    """For every output entry the sum over its products and over the kept limb pairs of |x_l| |w_l'|, exactly (not an upper bound): the convolution of the
    operands' limb_abs.  -> dict y / gx / dw / db of the largest entry.  Holds for operand pairs whose dropped limb products are zero (LimbCase.check asserts it)."""
    fwd, bwd, wgr = _LIMB_REFS[kind]
    sa, sw, sg = limb_abs(a), limb_abs(w), limb_abs(gy)
    out = {"y": float(fwd(sa, sw).max()) + (0.0 if b is None else float(limb_abs(b).max())), "gx": float(bwd(sg, sw, a.shape[2:]).max()), "dw": float(wgr(sa, sg).max())}
    if b is not None:
        out["db"] = float(sg.sum((0, 2, 3, 4)).max())
    return out


class LimbCase(_Case):
    """One convolution (kind k3 / k2 / t2, case = (N, Cin, Cout, D, H, W) as K3Case / K2Case / T2Case take it) with operands of a ROLE:

      role   x                         w                    gy                    limb products it exercises
      x3     three-limb, dense         ternary, sparse      ternary, sparse       y: x1 w0, x2 w0;  dW: limbs 1, 2 of the activation planes
      w3     ternary, sparse           three-limb, dense    ternary, sparse       y: x0 w1, x0 w2;  gx: the same in the flipped weight image
             (lazy: unit planes)       (lazy: sparse)
      g3     ternary, sparse           ternary, sparse      three-limb, dense     gx: limbs 1, 2 of the staged gradient;  dW: of the gradient planes
             (lazy: unit planes)                            (lazy: sparse)
      22     two-limb, dense           two-limb, sparse     two-limb, sparse      y, gx, dW: x1 w1 with the two middle products

    A lazy case runs the same InstanceNorm + ReLU input as the one-limb cases (unit_planes: a in {0, 0.5, 1, 2}, one limb, dense).  The bias of the strided
    kinds is ternary.  The densities are not chosen by hand: every sparse operand starts at START / (products of the output it is summed into) and whichever
    operands feed an output whose limb bound (dot_bounds_limbs) reaches 2^24 are thinned (by THIN times 2^24 / bound) and drawn again until the precondition
    holds; an operand the role leaves dense is thinned only when nothing else feeds the output (the bias gradient of a dense three-limb gy)."""
    START = {"x3": 16.0, "w3": 16.0, "g3": 16.0, "22": 12.0}
    THIN = 0.75
    LAZY_ROLES = ("w3", "g3")

    def __init__(self, kind, case, role, lazy=False, seed=0):
        assert kind in _LIMB_REFS and role in ROLES and (not lazy or role in self.LAZY_ROLES)
        n, cin, cout, d, h, w = case
        self.kind, self.case, self.role, self.lazy, self.unit, self.seed = kind, case, role, lazy, (0.5 if lazy else 1.0), seed
        self.transposed = kind == "t2"
        self.name = "%s %s role %s %s" % ({"k3": "k3", "k2": "k2s2", "t2": "t2s2"}[kind], case, role, "lazy" if lazy else "materialised")
        vol = (d, h, w)
        out_vol = vol if kind == "k3" else (d // 2, h // 2, w // 2) if kind == "k2" else (2 * d, 2 * h, 2 * w)
        taps = 27 if kind == "k3" else 8
        per_dw = n * d * h * w if kind != "k2" else n * (d // 2) * (h // 2) * (w // 2)          # terms of a weight-gradient entry
        per_y = cin if kind == "t2" else taps * cin
        per_gx = taps * cout if kind != "k2" else cout
        self.shapes = {"x": (n, cin) + vol, "w": ((cin, cout) if kind == "t2" else (cout, cin)) + ((3,) * 3 if kind == "k3" else (2,) * 3), "gy": (n, cout) + out_vol}
        start = self.START[role]
        # the class of each operand (limbs; 1 = ternary) and its starting density
        cls = {"x3": (3, 1, 1), "w3": (1, 3, 1), "g3": (1, 1, 3), "22": (2, 2, 2)}[role]
        self.limbs = dict(zip(("x", "w", "gy"), cls))
        dens = {"x3": (1.0, start / per_y, start / per_dw), "w3": (start / per_y, 1.0, start / per_gx), "g3": (start / per_dw, start / per_gx, 1.0),
                "22": (1.0, start / max(per_y, per_gx), start / per_dw)}[role]
        self.density = {k: min(1.0, v) for k, v in zip(("x", "w", "gy"), dens)}
        if lazy:                                  # the dense one-limb activation takes the place of x; the three-limb operand becomes the sparse one
            self.density["x"] = 1.0
            self.density["w" if role == "w3" else "gy"] = min(1.0, start / (4.0 * (per_y if role == "w3" else per_dw)))
        self.b = None if kind == "k3" else ints((cout,), 1, seed + 4)
        feeds = {"y": ("x", "w"), "gx": ("gy", "w"), "dw": ("x", "gy"), "db": ("gy",)}
        for self.rounds in range(1, 41):
            self._draw(n, cin, vol)
            self.bounds = dot_bounds_limbs(kind, self.a, self.w, self.gy, self.b)
            over = [k for k, v in self.bounds.items() if not v < LIMIT * self.unit and not (lazy and k == "gx")]
            if not over:
                break
            for k in over:
                ops_ = [o for o in feeds[k] if not (lazy and o == "x")]
                sparse = [o for o in ops_ if self.density[o] < 1.0]
                for o in (sparse or ops_[-1:]):
                    self.density[o] *= self.THIN * min(1.0, LIMIT * self.unit / self.bounds[k])
        else:
            raise AssertionError("%s: no densities meet the precondition" % self.name)

    def _draw(self, n, cin, vol):
        def make(which, k):
            shape, limbs, p = self.shapes[which], self.limbs[which], self.density[which]
            return ints(shape, 1, self.seed + k, p) if limbs == 1 else limb_ints(shape, limbs, self.seed + k, p)
        self.x = unit_planes(n, cin, vol, self.seed + 1) if self.lazy else make("x", 1)
        self.a = in_relu_exact(self.x) if self.lazy else self.x
        self.w, self.gy = make("w", 2), make("gy", 3)

    def check(self):
        """the precondition over limbs, the limb condition of every operand class, and that the dropped limb products are zero"""
        dots = {k: v for k, v in self.bounds.items() if not (self.lazy and k == "gx")}              # the gradient through a lazy input is not integer arithmetic
        assert_exact_precondition(self.name, dots, self.unit)
        for which, t in (("x", self.a), ("w", self.w), ("gy", self.gy)):
            nz = t[t != 0]
            assert nz.numel() > 0, "%s: %s is all zero" % (self.name, which)
            if self.limbs[which] > 1 and not (self.lazy and which == "x"):
                assert bool(limb_class_ok(nz, self.limbs[which]).all()), "%s: %s has entries without %d non-zero limbs" % (self.name, which, self.limbs[which])
            else:
                l0, l1, l2 = limbs_of(nz)
                assert not bool(l1.any()) and not bool(l2.any()), "%s: %s is not a one-limb operand" % (self.name, which)
        for p, q in (("x", "w"), ("gy", "w"), ("x", "gy")):                                       # x1 w2, x2 w1, x2 w2 vanish for every pair that is multiplied
            assert 1 in (self.limbs[p], self.limbs[q]) or (self.limbs[p], self.limbs[q]) == (2, 2)
        return self

    def _biased(self, y):
        return y if self.b is None else y + self.b.view(1, -1, 1, 1, 1)

    y = functools.cached_property(lambda self: self._biased(_LIMB_REFS[self.kind][0](self.a, self.w)))
    gx = functools.cached_property(lambda self: _LIMB_REFS[self.kind][1](self.gy, self.w, self.x.shape[2:]))
    dw = functools.cached_property(lambda self: _LIMB_REFS[self.kind][2](self.a, self.gy))
    db = functools.cached_property(lambda self: self.gy.sum((0, 2, 3, 4)))
