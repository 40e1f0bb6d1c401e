"""tests/exact_util.py pinned on the host: its fp64 references against an int64 tap-by-tap einsum and against F.conv3d / F.conv_transpose3d autograd in
fp64; its planes have exactly (sum, sum of squares) = (0, 4 V); the value a kernel stages from them is one of {0, 0.5, 1, 2}; and every case of
tests/test_gpu_exact.py meets the exactness precondition.  For the operands with two and three non-zero limbs (exact_util.LimbCase): the limb split, the
operand classes, the precondition taken over limbs, which kernel instantiation each case reaches, and that the results are SENSITIVE to each of the small limb
products while the tolerance tests are not."""
import pytest
import torch
import torch.nn.functional as F

from tests import exact_util as X
from tests import test_gpu_exact as G

RAGGED = [(2, 3, 5, 4, 5, 7), (1, 8, 2, 1, 1, 2), (3, 1, 8, 3, 2, 9), (1, 5, 5, 2, 7, 1)]      # (N, Cin, Cout, D, H, W)


def _overlap(k, size):
    """destination and source ranges of tap offset k - 1 inside a volume axis"""
    o = k - 1
    return slice(max(0, -o), min(size, size - o)), slice(max(0, o), min(size, size + o))


def _k3_int64(x, w):
    """3x3x3, padding 1, in int64 with explicit index ranges (no padded copy): independent of the reference's slicing"""
    xi, wi = x.long(), w.long()
    n, c, d, h, wd = xi.shape
    y = torch.zeros(n, wi.shape[0], d, h, wd, dtype=torch.int64)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                (dz, sz), (dy, sy), (dx, sx) = _overlap(kz, d), _overlap(ky, h), _overlap(kx, wd)
                y[:, :, dz, dy, dx] += torch.einsum("ncdhw,mc->nmdhw", xi[:, :, sz, sy, sx], wi[:, :, kz, ky, kx])
    return y


@pytest.mark.parametrize("case", RAGGED)
def test_k3_references_against_int64_einsum(case):
    n, cin, cout, d, h, w = case
    x, wt, gy = X.ints((n, cin, d, h, w), 8, 1), X.ints((cout, cin, 3, 3, 3), 8, 2, 0.7), X.ints((n, cout, d, h, w), 8, 3)
    assert torch.equal(X.conv3d_k3(x, wt), _k3_int64(x, wt).double())
    # the input gradient is the same convolution with the taps mirrored and the channel axes exchanged
    assert torch.equal(X.conv3d_k3_bwd_data(gy, wt), _k3_int64(gy, wt.flip(2, 3, 4).transpose(0, 1)).double())
    dw = torch.zeros(cout, cin, 3, 3, 3, dtype=torch.int64)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                (dz, sz), (dy, sy), (dx, sx) = _overlap(kz, d), _overlap(ky, h), _overlap(kx, w)
                dw[:, :, kz, ky, kx] = torch.einsum("nmdhw,ncdhw->mc", gy.long()[:, :, dz, dy, dx], x.long()[:, :, sz, sy, sx])
    assert torch.equal(X.conv3d_k3_wgrad(x, gy), dw.double())


@pytest.mark.parametrize("case", [(2, 3, 5, 4, 6, 2), (1, 8, 8, 5, 7, 3), (2, 1, 2, 2, 2, 8)])
def test_strided_references_against_int64_einsum(case):
    n, cin, cout, d, h, w = case
    x, b = X.ints((n, cin, d, h, w), 8, 4), X.ints((cout,), 8, 5)
    do, ho, wo = d // 2, h // 2, w // 2
    wt = X.ints((cout, cin, 2, 2, 2), 8, 6)
    y = b.long().view(1, -1, 1, 1, 1).expand(n, cout, do, ho, wo).clone()
    for kz in range(2):
        for ky in range(2):
            for kx in range(2):
                y += torch.einsum("ncdhw,mc->nmdhw", x.long()[:, :, kz:2 * do:2, ky:2 * ho:2, kx:2 * wo:2], wt.long()[:, :, kz, ky, kx])
    assert torch.equal(X.conv3d_k2s2(x, wt, b), y.double())
    wtt = X.ints((cin, cout, 2, 2, 2), 8, 7)
    yt = b.long().view(1, -1, 1, 1, 1).expand(n, cout, 2 * d, 2 * h, 2 * w).clone()
    for kz in range(2):
        for ky in range(2):
            for kx in range(2):
                yt[:, :, kz::2, ky::2, kx::2] += torch.einsum("ncdhw,cm->nmdhw", x.long(), wtt.long()[:, :, kz, ky, kx])
    assert torch.equal(X.conv_transpose3d_k2s2(x, wtt, b), yt.double())


def _autograd(fn, x, w, b, gy):
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = None if b is None else b.clone().requires_grad_(True)
    y = fn(xr, wr, br)
    (y * gy).sum().backward()
    return y.detach(), xr.grad, wr.grad, None if b is None else br.grad


@pytest.mark.parametrize("case", RAGGED + [(2, 4, 6, 5, 6, 9)])
def test_references_against_fp64_autograd(case):
    n, cin, cout, d, h, w = case
    x = X.ints((n, cin, d, h, w), 8, 11)
    # 3x3x3
    wt, gy = X.ints((cout, cin, 3, 3, 3), 8, 12), X.ints((n, cout, d, h, w), 8, 13)
    y, gx, dw, _ = _autograd(lambda a, b_, c: F.conv3d(a, b_, c, padding=1), x, wt, None, gy)
    assert torch.equal(X.conv3d_k3(x, wt), y) and torch.equal(X.conv3d_k3_bwd_data(gy, wt), gx) and torch.equal(X.conv3d_k3_wgrad(x, gy), dw)
    assert torch.equal(X.plane_stats(y), torch.stack((y.sum((2, 3, 4)), y.pow(2).sum((2, 3, 4))), -1))
    # transposed 2x2x2, stride 2
    b = X.ints((cout,), 8, 14)
    wt, gy = X.ints((cin, cout, 2, 2, 2), 8, 15), X.ints((n, cout, 2 * d, 2 * h, 2 * w), 8, 16)
    y, gx, dw, db = _autograd(lambda a, b_, c: F.conv_transpose3d(a, b_, c, stride=2), x, wt, b, gy)
    rw, rb = X.conv_transpose3d_k2s2_wgrad(x, gy)
    assert torch.equal(X.conv_transpose3d_k2s2(x, wt, b), y) and torch.equal(X.conv_transpose3d_k2s2_bwd_data(gy, wt), gx)
    assert torch.equal(rw, dw) and torch.equal(rb, db)
    # 2x2x2, stride 2 (odd axes: the last fine plane is read by no output and gets a zero gradient)
    if min(d, h, w) >= 2:
        wt, gy = X.ints((cout, cin, 2, 2, 2), 8, 17), X.ints((n, cout, d // 2, h // 2, w // 2), 8, 18)
        y, gx, dw, db = _autograd(lambda a, b_, c: F.conv3d(a, b_, c, stride=2), x, wt, b, gy)
        rw, rb = X.conv3d_k2s2_wgrad(x, gy)
        assert torch.equal(X.conv3d_k2s2(x, wt, b), y) and torch.equal(X.conv3d_k2s2_bwd_data(gy, wt, (d, h, w)), gx)
        assert torch.equal(rw, dw) and torch.equal(rb, db)


@pytest.mark.parametrize("vol", [(2, 3, 4), (1, 1, 2), (3, 3, 3), (1, 1, 5), (5, 5, 5), (3, 5, 7), (2, 2, 2), (4, 6, 10), (1, 7, 16)])
def test_planes_have_mean_zero_and_variance_four_exactly(vol):
    """even V, odd V and V divisible by 8 (where the odd channels take the +-4 pattern)"""
    n, c = 2, 5
    v = vol[0] * vol[1] * vol[2]
    x = X.unit_planes(n, c, vol, seed=v)
    assert torch.equal(x, x.round())
    assert torch.equal(x.sum((2, 3, 4)), torch.zeros(n, c, dtype=torch.float64))
    assert torch.equal((x * x).sum((2, 3, 4)), torch.full((n, c), 4.0 * v, dtype=torch.float64))
    kinds = {X.plane_kind(v, j) for j in range(c)}
    assert kinds == ({"odd"} if v % 2 else {"pm2", "pm4"} if v % 8 == 0 else {"pm2"})
    assert not torch.equal(x[0], x[1])                                       # shuffled per plane
    # fp64 InstanceNorm + ReLU at eps = 0 is what in_relu_exact states in closed form
    assert torch.equal(torch.relu(F.instance_norm(x, eps=0.0)), X.in_relu_exact(x))
    assert set(X.in_relu_exact(x).unique().tolist()) <= {0.0, 0.5, 1.0, 2.0}
    with pytest.raises(AssertionError):
        X.plane_values(3, "odd")


def test_staged_value_is_exact_in_every_storage_type():
    """eps = 1e-5 (the library's) in the 16-bit kernels: 2 * fp32(1 / sqrt(4.00001)) = 0.99999875 still rounds to 1 in bf16 and fp16 — also with the
    rsqrt + Newton reciprocal root of those kernels a few fp32 ulps off; fp32 needs eps = 0"""
    raw = torch.tensor([-4.0, -2.0, 0.0, 1.0, 2.0, 4.0, 6.0], dtype=torch.float64)
    want = torch.relu(raw * 0.5)
    for dtype in (torch.bfloat16, torch.float16):
        for scale in (1.0, 1.0 - 4e-7, 1.0 + 4e-7):
            assert torch.equal(X.staged(raw, dtype, 1e-5, scale), want)
    assert torch.equal(X.staged(raw, torch.float32, 0.0), want)
    assert not torch.equal(X.staged(raw, torch.float32, 1e-5), want)        # why the fp32 lazy cases run at eps = 0


def test_amplitudes_follow_the_bound():
    assert X.amplitude_for(4 * 24 * 48 * 128, cap=100) == 5                  # A^2 < 28.4: weight gradient of (4, 8, 8, 24, 48, 128)
    assert X.amplitude_for(2 * 32 * 64 * 64, cap=100) == 7                   # A^2 < 64, strictly
    assert X.amplitude_for(27 * 256, cap=100) == 49                          # A^2 < 2427: forward of 256 channels
    assert X.amplitude_for(27 * 256) == 8
    with pytest.raises(AssertionError):
        X.amplitude_for(2 ** 24)
    with pytest.raises(AssertionError):                                      # the precondition refuses, it never skips
        X.assert_exact_precondition("too many products", {"dw": float(2 ** 24)})
    y = torch.full((1, 1, 1, 1, 5), 2048.0, dtype=torch.float64)             # sum y^2 = 5 * 2^22 >= 2^24
    with pytest.raises(AssertionError):
        X.assert_exact_precondition("statistics", {}, 1.0, y)
    X.assert_exact_precondition("statistics", {}, 1.0, y[..., :3])


@pytest.mark.parametrize("kind,runs", [("k3", G.K3_RUNS), ("k2", G.K2_RUNS), ("t2", G.T2_RUNS)])
def test_every_gpu_case_meets_the_precondition(kind, runs):
    for case, lazy in runs:
        c = G._KINDS[kind](case, lazy, seed=G._seed(kind, case, lazy)).check()          # as tests/test_gpu_exact.py builds it
        if kind == "k3" and case[0] * case[3] * case[4] * case[5] >= X.LARGE_WGRAD:
            assert c.plan["A"] <= 2 and float(c.gy.abs().min()) >= 1 and (lazy or float(c.x.abs().min()) >= 1)      # large weight gradients: small, DENSE operands


def test_grouped_and_slab_cases_meet_the_precondition():
    assert len(G._group_cases()) == len(G.GROUP_LAYERS)
    many = G._many_batches_cases()                           # more layers than a batch of any grouped launch holds (csrc/wgrad.hip G3_RED_MAX 56, G3_BIAS_MAX 16, G3_GROUP_MAX 24)
    assert len(many) == 58 and sum(c.b is not None for c in many) == 18 and 58 + 18 > 56 and 58 + 18 > 3 * 24
    assert all(float(c.gy.abs().min()) >= 1 for c in many)
    assert set(G._several_cases()) == {"k3", "k2", "t2"}
    assert G.SLAB_CASES == [(2, 12, 16, 40), (1, 9, 11, 33), (3, 5, 9, 33), (1, 4, 8, 32), (16, 4, 8, 32)]
    for n, d, h, w in G.SLAB_CASES:
        G._KINDS["k3"]((n, 8, 8, d, h, w), True, seed=G._seed("k3", (n, 8, 8, d, h, w), True)).check()


def test_sparse_weight_cases_have_a_dense_twin_and_a_floor_on_their_density():
    """where the statistics bound thins the weights out, y and gx see few products per output: the density never falls below 1 %, about three non-zero
    weights per output row at least, and every such case runs again with dense weights (statistics left out), whose sums of products meet the bound too"""
    sparse = [(c, lz) for c, lz in G.K3_RUNS if X.plan_k3(c, lz)["pw"] < 1.0]
    assert G.K3_DENSE_RUNS == sparse and len(sparse) >= 8
    for case, lazy in sparse:
        plan = X.plan_k3(case, lazy)
        assert plan["pw"] >= (0.01 if lazy else 0.09) and plan["pw"] * 27 * case[1] >= 3.0, (case, lazy, plan)
        c = X.K3Case(case, lazy, seed=G._seed("k3", case, lazy, "dense"), dense=True)
        assert not c.with_stats and float(c.w.abs().min()) >= 1 and float(c.gy.abs().min()) >= 1 and (lazy or float(c.x.abs().min()) >= 1)
        assert c.plan["aw"] == c.plan["A"] == X.amplitude_for(max(27 * case[1], 27 * case[2], case[0] * case[3] * case[4] * case[5]), other=4 if lazy else None,
                                                              cap=2 if case[0] * case[3] * case[4] * case[5] >= X.LARGE_WGRAD else 8)
        X.assert_exact_precondition(c.name, X.dot_bounds_gather(c.a, c.w, c.gy))          # cheap: no reference is computed here
    for c in G._group_cases():                                 # the grouped layers compare dW and db only: dense activations and output gradients
        assert float(c.gy.abs().min()) >= 1


# ------------------------------------------------------------------------------------------------ operands with two and three non-zero limbs
KEPT = [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)]                  # the limb products the fp32 kernels keep: (limb of the activation / gradient, limb of the weight)


def _six_products(a, w, drop=(), edit=None):
    """The kernels' sum restated on the host — F.conv3d over the kept limb pairs, fp64 — minus the pairs in `drop`; edit(limbs of a) may displace a limb plane.
    Only ever compared with itself and with the plain reference: the GPU tests compare the kernels with the plain reference alone."""
    al, wl = list(X.limbs_of(a)), X.limbs_of(w)
    if edit is not None:
        edit(al)
    y = torch.zeros(a.shape[0], w.shape[0], *a.shape[2:], dtype=torch.float64)
    for i, j in KEPT:
        if (i, j) not in drop and bool(al[i].any()) and bool(wl[j].any()):
            y += F.conv3d(al[i], wl[j], padding=1)
    return y


def _changed(a, b):
    return float((a != b).double().mean())


def _rel_l2(a, ref):
    return float((a - ref).norm() / ref.norm())


def test_limb_split_and_operand_classes():
    """limbs_of is the split of csrc/common.h (three round-to-nearest bf16 limbs that sum to the value); the makers give every non-zero entry its class"""
    v = torch.tensor([1.0, -3.0, 255.0, 257.0, 1023.0, 65537.0, 2.0 ** 18 + 2.0 ** 9 + 1.0, -(2.0 ** 19 - 1.0), 0.5, 0.0], dtype=torch.float64)
    l0, l1, l2 = X.limbs_of(v)
    assert torch.equal(l0, torch.tensor([1.0, -3.0, 255.0, 256.0, 1024.0, 65536.0, 2.0 ** 18, -(2.0 ** 19), 0.5, 0.0], dtype=torch.float64))
    assert torch.equal(l1, torch.tensor([0.0, 0.0, 0.0, 1.0, -1.0, 1.0, 2.0 ** 9, 1.0, 0.0, 0.0], dtype=torch.float64))
    assert torch.equal(l2, torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], dtype=torch.float64))
    for l in (l0, l1, l2):
        assert torch.equal(l.float().to(torch.bfloat16).double(), l)
    with pytest.raises(AssertionError):
        X.limbs_of(torch.tensor([2.0 ** 24 + 1.0], dtype=torch.float64))                        # not an fp32 value
    X.limbs_of(torch.tensor([float(2 ** 24 - 1), float(2 ** 23 + 2 ** 12 + 2 ** 4 + 1)], dtype=torch.float64))      # rounded limbs hold all 24 bits
    three, two = X.limb_ints((4, 5, 6, 7), 3, 1), X.limb_ints((4, 5, 6, 7), 2, 2)
    assert float(three.abs().min()) >= 2 ** 16 and float(three.abs().max()) < 2 ** 19 and bool(X.limb_class_ok(three, 3).all())
    assert float(two.abs().min()) >= 2 ** 8 and float(two.abs().max()) < 2 ** 10 and bool(X.limb_class_ok(two, 2).all())
    assert bool((three < 0).any()) and bool((three > 0).any())
    thin = X.limb_ints((4, 5, 6, 7), 3, 3, 0.25)
    assert 0.15 < float((thin != 0).double().mean()) < 0.35 and bool(X.limb_class_ok(thin[thin != 0], 3).all())
    assert not bool(X.limb_class_ok(X.ints((64,), 8, 4), 2).any())                              # the one-limb integers of the other cases have neither


def _limb_runs():
    """every (kind, case, role, lazy) the GPU tests build"""
    runs = [("k3", case, role, lazy) for _, case, role, lazy in G.LIMB_K3_RUNS] + [("k3", case, role, False) for _, case, role in G.LIMB_K3_FALLBACK]
    runs += [(kind, case, role, False) for kind, case, _, role in G.LIMB_G1_RUNS] + [G.LIMB_G1_FALLBACK + (role, False) for role in X.ROLES]
    runs += [("k3", case, role, lazy) for case, role, lazy in G.LIMB_GROUP]
    return list(dict.fromkeys(runs))


def test_every_limb_case_meets_the_precondition_and_its_limb_conditions():
    """LimbCase.check: the bound over limbs below 2^24 for every compared output, every non-zero entry of an operand in its class, the dropped products zero.
    And the operand each role is about is as dense as the role says, the thinned ones not empty."""
    runs = _limb_runs()
    assert len(runs) >= 100
    for kind, case, role, lazy in runs:
        c = G._limb_case.__wrapped__(kind, case, role, lazy)
        assert not c.with_stats and c.rounds <= 20 and max(c.bounds[k] for k in c.bounds if not (lazy and k == "gx")) < X.LIMIT * c.unit
        main = {"x3": "x", "w3": "w", "g3": "gy", "22": "x"}[role]
        if kind == "k3" and not lazy:
            assert c.density[main] == 1.0 and float(getattr(c, main).abs().min()) > 0, c.name
        for which in ("x", "w", "gy"):
            assert int((getattr(c, which) != 0).sum()) >= 8, c.name                               # a thinned operand still has entries to be wrong about
    # the issue's figures at 16 -> 16, 5 x 9 x 33: densities 16 / (27 Cin), 0.04, 12 / (27 Cin) and bounds of 0.5 .. 0.7 of 2^24
    for role, which, dens in (("x3", "w", 16 / 432), ("w3", "x", 16 / 432), ("22", "w", 12 / 432)):
        c = X.LimbCase("k3", (1, 16, 16, 5, 9, 33), role, seed=1)
        assert c.rounds == 1 and abs(c.density[which] - dens) < 1e-12 and 0.3 * X.LIMIT < c.bounds["y"] < 0.9 * X.LIMIT


def test_limb_cases_reach_the_instantiations_they_name():
    """the kernel each LIMB_K3 entry names for its forward and backward-data launch is what the dispatch's rules (restated in k3x_instantiation) give, and the
    list covers every instantiation of g1_dispatch_k3_x3 that takes a plain launch"""
    seen = set()
    for ck, case, fwd, bwd in G.LIMB_K3:
        n, cin, cout, d, h, w = case
        assert G.k3x_instantiation(n, cin, cout, d, h, w, ck) == fwd and G.k3x_instantiation(n, cout, cin, d, h, w, ck) == bwd, case
        seen |= {fwd, bwd}
    assert seen == {"k3xt", "k3x<8,16>", "k3x<8,32>", "k3x<8,16,MULTI>", "k3x<8,32,MULTI>", "k3x<8,16,MULTI,YT=1>", "k3x<8,16,MULTI,YT=2>",
                    "k3x<16,16>", "k3x<16,32>", "k3x<16,16,MULTI>", "k3x<16,32,MULTI>"}
    assert G.k3x_instantiation(1, 32, 32, 6, 6, 6) == "k3s<float>"                                # what a case must not fall to


@pytest.mark.parametrize("case", list(dict.fromkeys(c for _, c, _, _ in G.LIMB_K3)))
def test_limb_cases_are_sensitive_to_each_small_product(case):
    """What makes the GPU tests worth having.  (3) the six kept products equal the plain reference on these data: the dropped terms are zero.  (2) Removing
    x2 w0 changes role x3's y; removing x0 w2 changes role w3's y and gx; removing x1 w1 changes role 22's y; displacing a limb-2 plane by one voxel or one
    channel changes role x3's y — each in at least half of the entries (seen: 0.90 or more).  And each removal moves the result by less than the 2e-5 relative
    L2 the tolerance tests allow: they cannot stand in."""
    flip = lambda w: w.flip(2, 3, 4).transpose(0, 1).contiguous()
    c = G._limb_case.__wrapped__("k3", case, "x3")
    y = _six_products(c.a, c.w)
    assert torch.equal(y, c.y)
    gone = _six_products(c.a, c.w, drop=[(2, 0)])
    assert _changed(gone, y) >= 0.5 and 0 < _rel_l2(gone, y) < 2e-5

    def roll(axis):
        def edit(al):
            al[2] = al[2].roll(1, axis)
        return edit
    assert _changed(_six_products(c.a, c.w, edit=roll(4)), y) >= 0.5 and _changed(_six_products(c.a, c.w, edit=roll(1)), y) >= 0.5
    c = G._limb_case.__wrapped__("k3", case, "w3")
    y, gx = _six_products(c.a, c.w), _six_products(c.gy, flip(c.w))
    assert torch.equal(y, c.y) and torch.equal(gx, c.gx)
    gone_y, gone_gx = _six_products(c.a, c.w, drop=[(0, 2)]), _six_products(c.gy, flip(c.w), drop=[(0, 2)])
    assert _changed(gone_y, y) >= 0.5 and _changed(gone_gx, gx) >= 0.5 and 0 < _rel_l2(gone_y, y) < 2e-5 and 0 < _rel_l2(gone_gx, gx) < 2e-5
    c = G._limb_case.__wrapped__("k3", case, "22")
    y = _six_products(c.a, c.w)
    assert torch.equal(y, c.y) and torch.equal(_six_products(c.gy, flip(c.w)), c.gx)
    gone = _six_products(c.a, c.w, drop=[(1, 1)])
    assert _changed(gone, y) >= 0.5 and 0 < _rel_l2(gone, y) < 2e-5
    c = G._limb_case.__wrapped__("k3", case, "g3")
    assert torch.equal(_six_products(c.gy, flip(c.w)), c.gx)



@pytest.mark.parametrize("case", G.FULL_CASES)
def test_full_mantissa_bound_sees_a_lost_small_product(case):
    """test_conv_k3_limbs_full_mantissa allows FULL_K times the error of torch's CPU fp32 convolution.  On its operands the six kept products lie 6e-9 from
    the plain fp64 result (the dropped ones), far inside that; with x1 w1 — or x0 w2, or x2 w0 — removed the sum lies 2.4e-6 to 2.8e-6 away, 9 times the
    comparator or more (profiles/limb_exact_accuracy.txt), so the bound catches such a loss on full-mantissa data too, for y and for gx."""
    c = G.full_mantissa_case(case)
    flip = c["w"].double().flip(2, 3, 4).transpose(0, 1).contiguous()
    for name, a, w in (("y", c["x"].double(), c["w"].double()), ("gx", c["gy"].double(), flip)):
        limit = G.FULL_K * c["cpu32"][name]
        assert _rel_l2(_six_products(a, w), c[name]) < 0.1 * limit
        for drop in ((1, 1), (0, 2), (2, 0)):
            assert _rel_l2(_six_products(a, w, drop=[drop]), c[name]) > 2.0 * limit, (case, name, drop)
