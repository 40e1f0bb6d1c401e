"""Signed distance maps of a label volume and the boundary loss on them (csrc/sdm.hip: ops.signed_distance, ops.boundary_loss, ops.BoundaryLoss,
evaluation.signed_distance, train.seg_train_losses(boundary=...), --boundary_weight) against their fp64 restatement (tests/boundary_util.py: scipy's exact
transform, pinned on the host by tests/test_host_boundary.py), in both builds.

Units of work of the distance kernels.  x pass: a wave owns one row of the label and walks it in 64-wide segments, forward carrying the last voxel of each
set, then backward carrying the next one; four waves per workgroup take consecutive rows.  y and z passes: a workgroup stages a slab — the whole axis L x TX
consecutive x columns, and a flag per column that tells whether it holds a finite entry at all — in LDS; TX is a power of two: 32, halved down to 8 while
the slab passes 32 KB (values of 4 bytes, 8 with a spacing), while TX / 2 >= w and while the launch would hold fewer than 1024 slabs, and 4 where 8 columns
would pass 64 KB; a lane scans outward from its voxel four distances per trip, with clamped reads past the ends of the line.
Branch reached by each (D, H, W) (two samples; K = top - bot classes):
  (1, 1, 1)       one lane of one wave; no y pass; the z pass scans nothing
  (1, 1, 70)      two x segments: both carries cross the segment border, lane 63 of segment 0 is live
  (3, 2, 64)      a row of exactly one full segment; lines shorter than one trip of the scan
  (1, 130, 5)     one long y line; w < 8: TX = 8 with three idle columns; 130 > 256 / 8 = 32 lines per sweep of the workgroup
  (70, 3, 9)      one long z line; TX = 8, two tiles, the second one holding 1 column
  (1, 130, 70)    TX = 8, nine tiles, the last one holding 6 columns
  (20, 24, 71)    rows not 16-byte aligned, w over one segment, TX = 8, the last tile holding 7 columns
  (40, 48, 56)    a single voxel of the class in a corner: the outward scan runs the whole axis, max d^2 = 39^2 + 47^2 + 55^2; every column but one of the
                  y pass's map "to the class" is without a finite entry and is skipped; TX = 16 for K = 3 (1920 / 1152 slabs in y / z), 8 for K = 1
  (44, 88, 40)    K = 3: 1056 slabs of TX = 32 in y and in z, the second tile holding 8 columns
  (1024, 1, 5)    with a spacing only: the longest axis of doubles, the one case of TX = 4
Label sets: blocks of 4 voxels per class (distances of several voxels), classless values (-1, 255, NaN, C, -0.5) and fractional valid labels (x.5) sprinkled
over them, the last class of [bot, top) absent from sample 0; kind "full": sample 1 entirely of class bot (its plane 0, every other class absent).

Units of work of the loss kernels: an element is a quad of voxels (16-byte path: V a multiple of 4 and aligned volumes) or one voxel (dword path); a lane
takes one element per trip, a wave 64, a workgroup 256, and both grids hold min(ceil(elements / 256), 512) workgroups per sample: 131,072 elements per sweep.

Tolerances follow from the arithmetic, none is measured.  phi at unit spacing: exact int32 squares and a correctly rounded fp64 square root leave no room —
torch.equal with the oracle rounded to fp32.  With a spacing scipy adds its fp64 terms in another order (about 1e-16 relative), far inside one fp32 rounding:
2^-22 max(1, |phi|).  Loss: fp64 sums of exact products, one rounding: 1e-6 max(1, |term|); weighted 2e-6 |w| max(1, |term|); gradient norm-wise < 1e-6,
exactly 0 at classless voxels and outside [bot, top)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import boundary_util as BU

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

both = pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
SHAPES = [(1, 1, 1), (1, 1, 70), (3, 2, 64), (1, 130, 5), (70, 3, 9), (1, 130, 70), (20, 24, 71)]
CORNER = (40, 48, 56)
CFGS = [(2, 1, 2), (4, 1, 4), (8, 2, 5)]          # (C, bot, top)
SPACING = (2.5, 0.7, 1.3)


def _ops():
    from vae_segmentation_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _labels(shape, cfg, kind):
    """(2, 1, D, H, W) fp32 labels on the host, shared by every test of the shape"""
    c, bot, top = cfg
    rng = np.random.default_rng(1000 * sum(shape) + 10 * c + len(kind))
    if kind == "corner":                           # a single voxel of class bot: the first corner in sample 0, the last in sample 1
        lab = np.zeros((2, 1) + shape, np.float32)
        lab[0, 0, 0, 0, 0] = bot
        lab[1, 0, -1, -1, -1] = bot
        return lab
    lab = BU.sprinkle(rng, BU.blocky_labels(rng, 2, c, shape), c)
    s0 = lab[0]
    s0[s0 == top - 1] = 0.0                        # the last class of the window is absent from sample 0 ...
    s0[s0 == top - 0.5] = 0.5                      # ... its fractional spelling too
    if kind == "full":
        lab[1] = bot
    else:
        assert kind == "mixed"
    return lab


@functools.lru_cache(maxsize=None)
def _oracle(shape, cfg, kind, spacing):
    c, bot, top = cfg
    return BU.signed_distance_batch(_labels(shape, cfg, kind), c, bot, top, spacing)


def _check_phi(ops, shape, cfg, kind, spacing=None):
    c, bot, top = cfg
    lab = _labels(shape, cfg, kind)
    want = _oracle(shape, cfg, kind, spacing)
    got = ops.signed_distance(torch.from_numpy(lab).cuda(), c, bot, top, spacing=spacing)
    torch.cuda.synchronize()
    assert got.shape == (2, top - bot) + shape and got.dtype == torch.float32
    got = got.cpu().numpy()
    what = "shape %s cfg %s labels %s spacing %s" % (shape, cfg, kind, spacing)
    if spacing is None:
        bad = int((got != want.astype(np.float32)).sum())
        print(what, "differing voxels:", bad, "max |phi|", float(np.abs(want).max()))
        assert bad == 0, what
    else:
        err = float((np.abs(got.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))).max())
        print(what, "max scaled error %.3g (bound %.3g)" % (err, 2.0 ** -22))
        assert err <= 2.0 ** -22, what
    return got, want


@both
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_phi_unit_spacing_is_the_oracle_rounded_to_fp32(shape, cfg, lib_mode):
    ops = _ops()
    for kind in ("mixed", "full"):
        got, want = _check_phi(ops, shape, cfg, kind)
        if kind == "full":
            assert (got[1] == 0).all()             # sample 1: one class fills the volume, the others are absent
    c, bot, top = cfg
    if np.prod(shape) > 1:
        assert (got[0, top - 1 - bot] == 0).all()  # the class absent from sample 0


@both
@pytest.mark.parametrize("cfg", CFGS)
def test_phi_of_a_single_corner_voxel(cfg, lib_mode):
    got, want = _check_phi(_ops(), CORNER, cfg, "corner")
    far = np.float32(np.sqrt(39.0 ** 2 + 47.0 ** 2 + 55.0 ** 2))
    assert got[0, 0, -1, -1, -1] == far and got[1, 0, 0, 0, 0] == far and got[0, 0, 0, 0, 0] == 0.0 and got[1, 0, -1, -1, -1] == 0.0


@both
@pytest.mark.parametrize("shape", [(1, 1, 70), (70, 3, 9), (1, 130, 70), (20, 24, 71), (1024, 1, 5)])
def test_phi_with_a_spacing(shape, lib_mode):
    ops = _ops()
    for cfg in CFGS:
        _check_phi(ops, shape, cfg, "mixed", SPACING)
    _check_phi(ops, shape, CFGS[1], "full", SPACING)


@both
@pytest.mark.parametrize("cfg", CFGS[1:])
def test_phi_on_slabs_of_32_columns(cfg, lib_mode):
    ops = _ops()
    _check_phi(ops, (44, 88, 40), cfg, "mixed")
    _check_phi(ops, (44, 88, 40), cfg, "mixed", SPACING)


@both
def test_phi_of_a_single_corner_voxel_with_a_spacing(lib_mode):
    _check_phi(_ops(), CORNER, CFGS[0], "corner", SPACING)


def test_evaluation_signed_distance_takes_a_volume():
    from vae_segmentation_amd import evaluation as E
    shape, cfg = (20, 24, 71), (4, 1, 4)
    lab = _labels(shape, cfg, "mixed")[1, 0]
    got = E.signed_distance(torch.from_numpy(lab).cuda(), 4)
    assert got.shape == (4,) + shape
    assert (got.cpu().numpy() == BU.signed_distance(lab, 4).astype(np.float32)).all()
    sp = E.signed_distance(torch.from_numpy(lab).cuda(), 4, spacing=SPACING).cpu().numpy().astype(np.float64)
    want = BU.signed_distance(lab, 4, spacing=SPACING)
    assert (np.abs(sp - want) <= 2.0 ** -22 * np.maximum(1.0, np.abs(want))).all()
    with pytest.raises(ValueError):
        E.signed_distance(torch.zeros(1, 1, 2, 3, 4, device="cuda"), 2)


# ---- the loss -----------------------------------------------------------------------------------------------------------------------------------
VEC_QUADS = [1, 63, 64, 65, 255, 256, 257, 131071, 131072, 131073]
DWORD_VOXELS = [1, 63, 65, 255, 257, 131071, 131073]


@functools.lru_cache(maxsize=4)
def _loss_case(b, c, v, bot, top, kind="mixed", seed=0):
    rng = np.random.default_rng(100003 * seed + v + 7 * b + 13 * c + 3 * bot)
    p = torch.softmax(torch.from_numpy(rng.normal(size=(b, c, v)) * 2), 1).float().numpy()
    phi = (rng.normal(size=(b, top - bot, v)) * 5).astype(np.float32)
    lab = rng.integers(0, c, size=(b, 1, v)).astype(np.float32)
    if kind == "mixed":
        lab = BU.sprinkle(rng, lab, c)
    elif kind == "empty_sample":                   # the last sample has no valid voxel
        lab = BU.sprinkle(rng, lab, c)
        lab[-1] = np.where(rng.random(lab[-1].shape) < 0.5, -1.0, np.nan)
    else:
        assert kind == "plain"
    return {"p": p, "phi": phi, "lab": lab, "valid": BU.classify(lab, c)[0]}


def _check_loss(ops, b, c, v, bot, top, w=0.75, kind="mixed", seed=0, scale=None, misalign=False):
    case = _loss_case(b, c, v, bot, top, kind, seed)
    gout = 1.0 if scale is None else float(scale)
    term, weighted, grad = BU.boundary_loss(case["p"], case["lab"], case["phi"], bot, top, weight=np.float32(w), gout=gout)

    def dev(a):
        t = torch.from_numpy(a).cuda()
        if misalign:                               # the same values 4 bytes off a 16-byte boundary: the dword path at any voxel count
            buf = torch.empty(t.numel() + 1, device="cuda")
            buf[1:].copy_(t.reshape(-1))
            t = buf[1:].view(t.shape)
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t
    p = dev(case["p"]).requires_grad_(True)
    wt = torch.tensor(w, dtype=torch.float32, device="cuda")
    got_w, got_t = ops.BoundaryLoss.apply(p, dev(case["lab"]), dev(case["phi"]), wt, bot, top)
    assert not got_t.requires_grad and got_w.requires_grad
    (got_w if scale is None else got_w * scale).backward()
    torch.cuda.synchronize()
    gp = p.grad.cpu().numpy()
    what = "B %d C %d V %d [%d, %d) w %g labels %s misaligned %s" % (b, c, v, bot, top, w, kind, misalign)
    gmax = float(np.abs(grad).max())
    gerr = BU.relerr(gp, grad) if gmax > 0 else float(np.abs(gp).max())
    print(what, "term %.9g (%.3g off) weighted %.9g (%.3g off) grad relerr %.3g" % (got_t.item(), abs(got_t.item() - term), got_w.item(),
                                                                                     abs(got_w.item() - weighted), gerr))
    assert gp.shape == case["p"].shape and gp.dtype == np.float32
    assert abs(got_t.item() - term) <= 1e-6 * max(1.0, abs(term)), what
    assert abs(got_w.item() - weighted) <= 2e-6 * abs(w) * max(1.0, abs(term)), what
    assert np.isfinite(gp).all(), what
    if gmax > 0:
        assert gerr < 1e-6, what
    else:
        assert float(np.abs(gp).max()) == 0.0, what
    assert float(np.abs(gp * ~case["valid"]).max()) == 0.0, what                      # exactly 0 at every classless voxel, in every channel
    assert float(np.abs(gp[:, :bot]).sum()) == 0.0 and float(np.abs(gp[:, top:]).sum()) == 0.0, what
    return case, (got_w, got_t, gp)


@both
@pytest.mark.parametrize("quads", VEC_QUADS)
def test_loss_plane_sizes_on_the_16_byte_path(quads, lib_mode):
    _check_loss(_ops(), 2, 3, 4 * quads, 1, 3)


@both
@pytest.mark.parametrize("v", DWORD_VOXELS)
def test_loss_plane_sizes_on_the_dword_path(v, lib_mode):
    _check_loss(_ops(), 2, 3, v, 1, 3, kind="plain" if v == 1 else "mixed")


@both
@pytest.mark.parametrize("v", [4 * 64, 4 * 256, 4 * 257])
def test_loss_on_misaligned_volumes(v, lib_mode):
    _check_loss(_ops(), 2, 3, v, 1, 3, misalign=True)


@both
@pytest.mark.parametrize("cfg", CFGS + [(1, 0, 1), (3, 0, 3)])
@pytest.mark.parametrize("b", [1, 3])
def test_loss_batch_and_channel_configurations(b, cfg, lib_mode):
    c, bot, top = cfg
    _check_loss(_ops(), b, c, 4 * 321, bot, top, w=1.3)


@both
def test_loss_sample_without_a_valid_voxel_contributes_nothing(lib_mode):
    case, (got_w, got_t, gp) = _check_loss(_ops(), 2, 3, 4 * 300, 1, 3, kind="empty_sample")
    assert float(np.abs(gp[-1]).max()) == 0.0 and float(np.abs(gp[0]).max()) > 0
    assert not case["valid"][-1].any()


@both
@pytest.mark.parametrize("scale", [1024.0, 0.37])
def test_loss_upstream_gradient_and_weight_are_read_on_the_device(scale, lib_mode):
    s = torch.tensor(scale, device="cuda")
    _check_loss(_ops(), 2, 3, 4 * 300, 1, 3, w=0.02, scale=s, seed=1)


@both
def test_boundary_loss_makes_its_own_maps(lib_mode):
    """ops.boundary_loss on a volume: the maps of ops.signed_distance, then the loss, against the oracle end to end; a number as weight"""
    ops = _ops()
    shape, cfg = (20, 24, 71), (4, 1, 4)
    c, bot, top = cfg
    lab = _labels(shape, cfg, "mixed")
    rng = np.random.default_rng(5)
    p_host = torch.softmax(torch.from_numpy(rng.normal(size=(2, c) + shape)), 1).float().numpy()
    term, weighted, grad = BU.boundary_loss(p_host, lab, _oracle(shape, cfg, "mixed", None).astype(np.float32), bot, top, weight=np.float32(0.3))
    p = torch.from_numpy(p_host).cuda().requires_grad_(True)
    got_w, got_t = ops.boundary_loss(p, ops.LabelTarget(torch.from_numpy(lab).cuda()), 0.3, botindex=bot, topindex=top)
    got_w.backward()
    assert abs(got_t.item() - term) <= 1e-6 * max(1.0, abs(term)) and abs(got_w.item() - weighted) <= 2e-6 * 0.3 * max(1.0, abs(term))
    assert BU.relerr(p.grad.cpu().numpy(), grad) < 1e-6
    with pytest.raises(TypeError):
        ops.boundary_loss(p, torch.from_numpy(lab).cuda(), 0.3)
    with pytest.raises(TypeError):
        ops.boundary_loss(p, ops.LabelTarget(torch.from_numpy(lab).cuda()), torch.tensor([0.3], device="cuda"))


@both
def test_weight_zero_leaves_the_bits_of_the_regional_loss(lib_mode):
    """weight = 0.0 as a device tensor: seg_final + weighted and the summed gradient are those of ops.seg_loss alone"""
    ops = _ops()
    shape, cfg = (20, 24, 71), (4, 1, 4)
    c, bot, top = cfg
    lab = torch.from_numpy(_labels(shape, cfg, "mixed")).cuda()
    g = torch.Generator().manual_seed(3)
    p0 = torch.softmax(torch.randn((2, c) + shape, generator=g) * 2, 1).cuda()
    kw = dict(botindex=bot, topindex=top, eps=1e-4, ce_weight=1.0, batch_dice=True)
    pa = p0.clone().requires_grad_(True)
    fa, _ = ops.seg_loss(pa, ops.LabelTarget(lab), **kw)
    fa.backward()
    pb = p0.clone().requires_grad_(True)
    fb, _ = ops.seg_loss(pb, ops.LabelTarget(lab), **kw)
    weighted, term = ops.boundary_loss(pb, ops.LabelTarget(lab), torch.zeros((), device="cuda"), botindex=bot, topindex=top)
    (fb + weighted).backward()
    torch.cuda.synchronize()
    assert term.item() != 0.0 and weighted.item() == 0.0
    assert torch.equal((fb + weighted).detach(), fa.detach()) and torch.equal(pb.grad, pa.grad)


# ---- bad arguments ---------------------------------------------------------------------------------------------------------------------------------
@both
def test_argument_errors(lib_mode):
    import ctypes
    from vae_segmentation_amd._lib import VaesegError, lib
    ops = _ops()
    lab = torch.zeros(1, 1, 4, 5, 6, device="cuda")
    for bad in (lab[0], lab.expand(1, 2, 4, 5, 6)):
        with pytest.raises(ValueError):
            ops.signed_distance(bad, 2)
    for kw in (dict(n_class=0), dict(n_class=2, botindex=2), dict(n_class=2, botindex=1, topindex=1), dict(n_class=2, topindex=3), dict(n_class=2, botindex=-1),
               dict(n_class=2, spacing=(1.0, 2.0))):
        with pytest.raises(ValueError):
            ops.signed_distance(lab, **kw)
    for sp in ((1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (float("nan"), 1.0, 1.0), (1.0, 1.0, float("inf"))):
        with pytest.raises(VaesegError):
            ops.signed_distance(lab, 2, spacing=sp)
    with pytest.raises(RuntimeError):
        ops.signed_distance(lab.cpu(), 2)
    # the C interface itself: codes, answered on the host before any launch (nothing below may touch phi / terms / gp)
    EINVAL, ESHAPE, EALIGN = -1, -2, -5
    st = torch.cuda.current_stream().cuda_stream
    assert lib.vs_signed_distance_workspace_bytes(1, 1, 4, 5, 6, 0) == 256 * ((2 * 120 * 4 + 255) // 256)
    assert lib.vs_signed_distance_workspace_bytes(2, 3, 4, 5, 6, 1) == 256 * ((2 * 3 * 2 * 120 * 8 + 255) // 256)
    for args, code in (((0, 1, 4, 5, 6, 0), ESHAPE), ((1, 0, 4, 5, 6, 0), EINVAL), ((1, 1, 1025, 5, 6, 0), ESHAPE), ((1, 1, 4, 1025, 6, 0), ESHAPE),
                       ((1, 1, 1, 1, 46341, 0), ESHAPE), ((1, 1, 1024, 1024, 2048, 0), ESHAPE)):
        assert lib.vs_signed_distance_workspace_bytes(*args) == code, args
    assert lib.vs_signed_distance_workspace_bytes(1, 1, 1, 1, 46341, 1) > 0          # the fp64 path has no integer limit
    ws = torch.empty(lib.vs_signed_distance_workspace_bytes(1, 2, 4, 5, 6, 1), dtype=torch.uint8, device="cuda")
    phi = torch.full((1, 2, 4, 5, 6), -7.0, device="cuda")
    L, F, W = lab.data_ptr(), phi.data_ptr(), ws.data_ptr()
    good = (ctypes.c_double * 3)(2.5, 0.7, 1.3)

    def sd(l_=L, f_=F, n=1, nc=2, bot=0, top=2, d=4, h=5, w=6, sp=None, w_=W):
        return lib.vs_signed_distance(l_, f_, n, nc, bot, top, d, h, w, sp, w_, st)
    for bad, code in ((dict(l_=None), EINVAL), (dict(f_=None), EINVAL), (dict(w_=None), EINVAL), (dict(f_=L), EINVAL), (dict(w_=L), EINVAL),
                      (dict(l_=L + 4), EALIGN), (dict(f_=F + 8), EALIGN), (dict(w_=W + 4), EALIGN), (dict(n=0), ESHAPE), (dict(d=0), ESHAPE),
                      (dict(d=1025), ESHAPE), (dict(h=1025), ESHAPE), (dict(d=1, h=1, w=46341), ESHAPE), (dict(nc=0), EINVAL), (dict(bot=2), EINVAL),
                      (dict(bot=1, top=1), EINVAL), (dict(top=3), EINVAL), (dict(bot=-1), EINVAL),
                      (dict(sp=(ctypes.c_double * 3)(1.0, 0.0, 1.0)), EINVAL), (dict(sp=(ctypes.c_double * 3)(1.0, 1.0, float("nan"))), EINVAL),
                      (dict(sp=(ctypes.c_double * 3)(float("inf"), 1.0, 1.0)), EINVAL), (dict(sp=(ctypes.c_double * 3)(-1.0, 1.0, 1.0)), EINVAL)):
        assert sd(**bad) == code, bad
    torch.cuda.synchronize()
    assert float((phi + 7.0).abs().max()) == 0.0
    assert sd() == 0 and sd(sp=good) == 0
    torch.cuda.synchronize()
    assert float(phi.abs().max()) == 0.0                                              # an all-zero label: class 0 fills the volume, class 1 is absent

    p = torch.softmax(torch.randn(2, 3, 1, 4, 8, device="cuda"), 1)
    lab2 = torch.randint(0, 3, (2, 1, 1, 4, 8), device="cuda").float()
    f2 = torch.randn(2, 2, 1, 4, 8, device="cuda")
    wt = torch.ones((), device="cuda")
    with pytest.raises(ValueError):
        ops.BoundaryLoss.apply(p, lab2[:1], f2, wt, 1, 3)
    with pytest.raises(ValueError):
        ops.BoundaryLoss.apply(p, lab2, f2[:, :1], wt, 1, 3)
    with pytest.raises(TypeError):
        ops.BoundaryLoss.apply(p, lab2, f2, torch.ones(1, device="cuda"), 1, 3)
    with pytest.raises(VaesegError):
        ops.BoundaryLoss.apply(p, lab2, f2[:, :0], wt, 2, 2)
    assert lib.vs_boundary_loss_scratch_doubles(2, 3) == 2 * 2 * 513
    assert lib.vs_boundary_loss_scratch_doubles(0, 3) == 0 and lib.vs_boundary_loss_scratch_doubles(65, 3) == 0 and lib.vs_boundary_loss_scratch_doubles(2, 0) == 0
    scratch = torch.empty(lib.vs_boundary_loss_scratch_doubles(2, 3), dtype=torch.float64, device="cuda")
    terms = torch.full((2,), -7.0, device="cuda")
    gout = torch.ones((), device="cuda")
    gp = torch.full_like(p, -7.0)
    P, L2, F2, WT, S, TT, G, GP = (t.data_ptr() for t in (p, lab2, f2, wt, scratch, terms, gout, gp))

    def fwd(p_=P, l_=L2, f_=F2, w_=WT, s_=S, t_=TT, b=2, c=3, bot=1, top=3, v=32):
        return lib.vs_boundary_loss_fwd(p_, l_, f_, w_, s_, t_, b, c, bot, top, v, st)

    def bwd(l_=L2, f_=F2, w_=WT, s_=S, g_=G, gp_=GP, b=2, c=3, bot=1, top=3, v=32):
        return lib.vs_boundary_loss_bwd(l_, f_, w_, s_, g_, gp_, b, c, bot, top, v, st)
    for f in (fwd, bwd):
        for bad, code in ((dict(l_=None), EINVAL), (dict(f_=None), EINVAL), (dict(w_=None), EINVAL), (dict(s_=None), EINVAL), (dict(c=0), EINVAL),
                          (dict(bot=3, top=3), EINVAL), (dict(bot=2, top=1), EINVAL), (dict(bot=-1), EINVAL), (dict(top=4), EINVAL), (dict(b=0), EINVAL),
                          (dict(v=0), EINVAL), (dict(b=65), ESHAPE), (dict(v=1 << 31), ESHAPE), (dict(l_=L2 + 2), EALIGN), (dict(f_=F2 + 1), EALIGN),
                          (dict(s_=S + 4), EALIGN)):
            assert f(**bad) == code, (f.__name__, bad)
    assert fwd(p_=None) == EINVAL and fwd(t_=None) == EINVAL and fwd(p_=P + 2) == EALIGN
    assert bwd(g_=None) == EINVAL and bwd(gp_=None) == EINVAL and bwd(gp_=GP + 2) == EALIGN
    torch.cuda.synchronize()
    assert float(terms[0]) == -7.0 and float((gp + 7.0).abs().max()) == 0.0
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert float(terms[0]) != -7.0 and float((gp[:, 1:] + 7.0).abs().min()) > 0.0 and float(gp[:, 0].abs().max()) == 0.0


# ---- graph replay and training --------------------------------------------------------------------------------------------------------------------
def test_signed_distance_replayed_from_a_graph_gives_the_bits_of_an_eager_call():
    """captured once, replayed three times on fresh labels, on the deterministic build (the suite's default); and the other build gives the same bits"""
    ops = _ops()
    shape, cfg = (20, 24, 71), (4, 1, 4)
    c, bot, top = cfg
    labs = [torch.from_numpy(_labels(shape, cfg, kind)).cuda() for kind in ("mixed", "full", "mixed")]
    labs[2] = labs[2].flip(0)
    assert ops.is_deterministic()
    for spacing in (None, SPACING):
        eager = [ops.signed_distance(l, c, bot, top, spacing=spacing).clone() for l in labs]
        buf = torch.zeros_like(labs[0])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.signed_distance(buf, c, bot, top, spacing=spacing)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ops.signed_distance(buf, c, bot, top, spacing=spacing)
        for l, want in zip(labs, eager):
            buf.copy_(l)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want)
        del graph
        ops.set_deterministic(False)
        try:
            assert all(torch.equal(ops.signed_distance(l, c, bot, top, spacing=spacing), want) for l, want in zip(labs, eager))
        finally:
            ops.set_deterministic(True)


def _seg(seed=0):
    import joint_model as M
    from oracle import ref_cpu as O
    return O.deterministic_fill_(M.Segmentation(1, 2, norm_type=1), seed=seed).cuda()


def _train_inputs():
    from oracle import ref_cpu as O
    img, lab = O.synthetic_image(2, 32, 2).cuda(), O.synthetic_label(2, 32, 3).cuda()
    lab[1] = 0                                 # sample 1 all background: its maps are 0
    assert float(lab[0].sum()) > 0
    return img, lab


LOSS = {"dice_weight": 1.0, "ce_weight": 1.0, "batch_dice": True, "class_weights": [0.5, 2.0], "gamma": 0.0}


def test_captured_training_follows_the_weight_scalar_without_a_new_capture():
    """three GraphedStep replays of seg_train_losses(loss=..., boundary=...) at 32^3, batch 2, against three eager steps: the same loss and weights bit for
    bit; then the weight scalar is refilled and the next replay — same GraphedStep, no re-capture — equals an eager step at the new weight"""
    from vae_segmentation_amd import optim
    from vae_segmentation_amd import train as T
    img, lab = _train_inputs()
    seg_a, seg_c = _seg(), _seg()
    opt_a = optim.SGD(seg_a.parameters(), lr=1e-2, momentum=0.9)
    opt_c = optim.SGD(seg_c.parameters(), lr=1e-2, momentum=0.9)
    w_a = torch.full((), 0.05, device="cuda")
    w_c = torch.full((), 0.05, device="cuda")
    gs = T.GraphedStep(lambda: T.seg_train_losses(seg_a, img, lab, loss=LOSS, boundary={"weight": w_a, "spacing": None}), list(seg_a.parameters()), opt_a,
                       warmup=1)
    assert gs.tail
    graph = gs.graph
    seen = []
    for i in range(5):
        if i == 3:
            w_a.fill_(0.4)
            w_c.fill_(0.4)
        la = gs.step()
        opt_c.zero_grad()
        lc, aux = T.seg_train_losses(seg_c, img, lab, loss=LOSS, boundary={"weight": w_c, "spacing": None})
        lc.backward()
        opt_c.step()
        torch.cuda.synchronize()
        assert torch.equal(la.detach(), lc.detach()), i
        assert set(aux) == {"dice_loss", "ce_loss", "boundary_loss", "batch"}
        assert torch.equal(gs.aux["boundary_loss"], aux["boundary_loss"]) and aux["boundary_loss"].item() != 0.0
        seen.append((la.item(), aux["boundary_loss"].item(), aux["dice_loss"].item(), aux["ce_loss"].item()))
    assert gs.recaptures == 0 and gs.graph is graph
    for (n, p), q in zip(seg_a.named_parameters(), seg_c.parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    # the weight is in the loss: final = compound + w * L_B with the w of the step (fp32 sums of once-rounded terms)
    for (final, lb, d, ce), w in zip(seen, (0.05, 0.05, 0.05, 0.4, 0.4)):
        assert abs(final - (d + ce + w * lb)) <= 4e-6 * (1.0 + abs(ce) + abs(w * lb))


def test_joint_train_losses_with_the_boundary_term():
    import joint_model as M
    from oracle import ref_cpu as O
    from vae_segmentation_amd import ops
    from vae_segmentation_amd import train as T
    side = 64
    joint = M.Joint(models=[M.Segmentation(1, 2, norm_type=1), M.VAE(2, 2, norm_type=1, dim=128, spatial=side)])
    O.deterministic_fill_(joint, seed=0)
    joint = joint.cuda()
    img, lab = O.synthetic_image(1, side, 2).cuda(), O.synthetic_label(1, side, 3).cuda()
    final, aux = T.joint_train_losses(joint, img, lab, lambda_vae=0.1, loss=LOSS, boundary={"weight": 0.2, "spacing": None})
    final.backward()
    pred = aux["batch"]["pred"].detach()
    base, _ = T.joint_train_losses(joint, img, lab, lambda_vae=0.1, loss=LOSS)
    weighted, term = ops.boundary_loss(pred, ops.LabelTarget(lab), 0.2, botindex=1, topindex=2)
    assert torch.equal(final.detach(), base.detach() + weighted) and torch.equal(aux["boundary_loss"], term)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in joint.Seg.parameters())


def test_without_the_boundary_argument_a_step_makes_the_calls_it_made():
    """the library calls of an eager seg_train step (recorded as tools/ops_call_trace.py records them): boundary=None adds none and is call for call the
    step without the argument; boundary={...} adds exactly the calls of the map and the loss — three right behind the compound loss's forward, one in the
    backward — and changes no other call"""
    from tools import ops_call_trace as OT
    from vae_segmentation_amd import _lib
    from vae_segmentation_amd import train as T
    img, lab = _train_inputs()
    seg = _seg()
    l = _lib.lib
    saved = (l._fast, l._det, l._active)
    names = {}
    try:
        l._det = OT.Traced(l._det if l._det is not None else l._fast)
        l._active = l._det
        for key, kw in (("absent", {}), ("none", {"boundary": None}), ("on", {"boundary": {"weight": 0.1, "spacing": None}})):
            for _ in range(2):                 # the first pass of a variant builds its lazy state (packed weights, plans, workspaces)
                for p in seg.parameters():
                    p.grad = None
                OT.REC.begin()
                try:
                    loss, _ = T.seg_train_losses(seg, img, lab, loss=LOSS, **kw)
                    loss.backward()
                finally:
                    calls = OT.REC.end()
            torch.cuda.synchronize()
            names[key] = calls
    finally:
        l._fast, l._det, l._active = saved
    new = {"vs_signed_distance", "vs_boundary_loss_scratch_doubles", "vs_boundary_loss_fwd", "vs_boundary_loss_bwd"}
    assert OT._nullness(names["absent"]) == OT._nullness(names["none"])
    assert not any(c[0] in new or c[0] == "vs_signed_distance_workspace_bytes" for c in names["absent"])
    added = [c[0] for c in names["on"] if c[0] in new]
    assert added == ["vs_signed_distance", "vs_boundary_loss_scratch_doubles", "vs_boundary_loss_fwd", "vs_boundary_loss_bwd"]
    assert all(c[-1] == ["ret", 0] for c in names["on"] if c[0] in new and c[0] != "vs_boundary_loss_scratch_doubles")
    # names, scalars, return values and which pointers are null; pointer indices shift with the added buffers
    assert OT._nullness([c for c in names["on"] if c[0] not in new]) == OT._nullness(names["absent"])
    i_seg = [c[0] for c in names["on"]].index("vs_seg_loss_fwd")
    assert [c[0] for c in names["on"]][i_seg + 1:i_seg + 4] == ["vs_signed_distance", "vs_boundary_loss_scratch_doubles", "vs_boundary_loss_fwd"]


def test_entry_point_runs_the_boundary_term(tmp_path):
    common = ["--size", "32", "-b", "2", "-E", "2", "--eval_epoch", "1", "--save_epoch", "1", "--synthetic_train", "4", "--synthetic_val", "1",
              "--max_iters", "2", "--display_freq", "1", "--boundary_weight", "0.01", "--boundary_ramp", "0.01"]

    def run(seg_loss):
        return subprocess.run([sys.executable, os.path.join(REPO, "main_source.py"), "bl", "--method", "seg_train", "--seg_loss", seg_loss] + common,
                              cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=900)
    out = run("dice_ce")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Finished Training" in out.stdout and "boundary_loss" in out.stdout and "graph replay" in out.stdout
    assert out.stdout.count("train step captured as a HIP graph") == 1          # the second epoch's weight needed no new capture
    bad = run("dice")
    assert bad.returncode != 0 and "boundary" in bad.stderr and "--seg_loss dice_ce" in bad.stderr
