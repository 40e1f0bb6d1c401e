"""CPU-only checks of the host side: the C-ABI library loads and exports every symbol include/vaeseg.h declares,
argument validation rejects bad calls without touching a GPU, the host-side helpers, and the world_size-2
gradient exchange (gloo) used by the data-parallel step."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from vae_segmentation_amd import _lib
    protos = _lib.parse_header()
    assert len(protos) >= 85
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(raw, name), name
    for must in ("vs_conv_gather_fwd", "vs_conv_scatter_fwd", "vs_conv_k3_softmax2_fwd", "vs_conv_wgrad", "vs_pack_weight",
                 "vs_instnorm_relu_fwd", "vs_instnorm_relu_bwd_reduce", "vs_instnorm_relu_bwd_apply", "vs_softmax2_bwd",
                 "vs_dice_fwd", "vs_dice_bwd", "vs_kl_fwd", "vs_kl_bwd", "vs_reparam_fwd", "vs_linear_fwd", "vs_onehot",
                 "vs_binarize", "vs_bce_fwd", "vs_sgd_momentum_multi", "vs_adam_multi", "vs_ema_multi", "vs_strerror",
                 "vs_version", "vs_conv_wgrad_workspace_bytes", "vs_copy_scale_multi", "vs_conv_gather_bwd_data",
                 "vs_conv_scatter_bwd_data", "vs_pack_weight_multi", "vs_dropout", "vs_softmax2_dropout_bwd",
                 "vs_conv_k3_softmax2_dropout_fwd", "vs_softmax_cl_fwd", "vs_softmax_cl_bwd", "vs_conv_wgrad_multi", "vs_conv_wgrad_multi_workspace_bytes",
                 "vs_dice_loss_multi_fwd", "vs_dice_loss_multi_bwd", "vs_dice_loss_multi_scratch_doubles"):
        assert must in protos, must
    assert _lib.lib.vs_version() == 500
    assert b"dtype" in _lib.lib.vs_strerror(-3)


def test_argument_validation_without_gpu():
    """Bad arguments are rejected on the host before any launch (no compute call is made here)."""
    from vae_segmentation_amd._lib import lib
    assert lib.vs_conv_gather_fwd(None, None, None, None, None, None, 1, 4, 4, 4, 8, 8, 0, 0, 1e-5, None) == -1
    assert lib.vs_pack_weight(None, None, 8, 8, 27, 8, 0, 0, None) == -1
    assert lib.vs_dice_fwd(None, None, None, None, None, 1, 2, 64, 1, 2, 1e-4, None) == -1
    # packed-weight sizing is pure host arithmetic: 16 rows x (27 taps x 8 ch -> 7 k-groups of 32) bf16 fragments ...
    assert lib.vs_packed_weight_bytes(16, 8, 27, 1) == 1 * 1 * 7 * 64 * 8 * 2
    # ... except the 8-channel 3x3x3 layers (<= 8 rows, bf16), packed as 9 Toeplitz k-groups (tz, ty) for k3t_kernel
    assert lib.vs_packed_weight_bytes(8, 8, 27, 1) == 9 * 64 * 8 * 2
    assert lib.vs_packed_weight_bytes(8, 8, 27, 0) == 18 * 64 * 4 * 4                # fp32: 18 y-Toeplitz k-groups (36 window taps (dz, wy, dx), two per k-group) for k3_kernel<.., TY>
    assert lib.vs_packed_weight_bytes(16, 8, 27, 0) == 1 * 1 * 14 * 64 * 4 * 4       # more than 8 rows: the standard order
    assert lib.vs_packed_weight_bytes(64, 64, 27, 0) == 4 * 2 * 54 * 64 * 4 * 4
    assert lib.vs_conv_wgrad_workspace_bytes(2, 96, 96, 96, 8, 8, 0) > 0
    # maximum sizes: shapes the 32-bit offsets of the kernels cannot address are refused (VS_ESHAPE = -2), never mis-computed.
    # (fake, aligned, never dereferenced pointers: the check precedes every launch)
    fake = 0x10000
    assert lib.vs_conv_gather_fwd(fake, None, fake, None, fake, None, 1, 2048, 1024, 1024, 8, 8, 0, 1, 1e-5, None) == -2     # >= 2^31 elements
    assert lib.vs_conv_gather_fwd(fake, None, fake, None, fake, None, 1, 512, 512, 512, 8, 8, 0, 1, 1e-5, None) == -2        # bf16 3x3x3: >= 2 GiB
    assert lib.vs_conv_gather_fwd(fake, None, fake, None, fake, None, 1, 5, 5, 5, 8, 8, 1, 1, 1e-5, None) == -2              # stride-2 conv on odd sizes
    assert lib.vs_conv_gather_fwd(fake, None, fake, None, fake, None, 1, 4, 4, 4, 24, 8, 0, 1, 1e-5, None) == -2             # channel count not 8 / 16 / 32k
    assert lib.vs_conv_gather_fwd(fake + 4, None, fake, None, fake, None, 1, 4, 4, 4, 8, 8, 0, 1, 1e-5, None) == -5          # VS_EALIGN
    assert lib.vs_conv_gather_fwd(fake, None, fake, None, fake, None, 0, 4, 4, 4, 8, 8, 0, 1, 1e-5, None) == -2              # empty batch
    # every launcher of csrc/conv_api.hip refuses on the host, with the code of the FIRST check that fails (-1 EINVAL, -2 ESHAPE, -3 EDTYPE, -5 EALIGN);
    # none of these argument lists is one a launcher accepts
    ea = lib.vs_conv_k3_bwd_data_applied                   # (x, w, y, mask_x, mask_stats, sums, sync, fault, n, d, h, w, c, m, dtype, eps, stream)
    assert ea(fake, fake, fake, None, fake, fake, fake, fake, 2, 24, 24, 24, 32, 32, 1, 1e-5, None) == -1                    # without mask
    assert ea(fake, fake, fake, fake, fake, fake, fake + 64, fake, 2, 24, 24, 24, 32, 32, 1, 1e-5, None) == -5               # sync not 128-byte aligned
    assert ea(fake, fake, fake, fake, fake, fake, fake, fake, 2, 24, 24, 24, 8, 8, 1, 1e-5, None) == -2                      # 8 -> 8: no epilogue-apply kernel
    assert ea(fake, fake, fake, fake, fake, fake, fake, fake, 2, 96, 96, 96, 32, 32, 1, 1e-5, None) == -2                    # more than one resident round
    s2 = lib.vs_conv_s2_bwd_data_applied                   # (x, w, y, mask_x, mask_stats, sums, add, sync, fault, n, d, h, w, c, m, scatter, dtype, eps, stream)
    assert s2(fake, fake, fake, fake, fake, fake, fake + 8, fake, fake, 2, 24, 24, 24, 32, 32, 0, 1, 1e-5, None) == -5       # add misaligned
    assert s2(fake, fake, fake, fake, fake, fake, None, fake, fake, 2, 4, 4, 4, 512, 512, 0, 1, 1e-5, None) == -2            # wider than 256 channels
    assert s2(fake, fake, fake, fake, fake, fake, None, fake, fake, 2, 96, 96, 96, 8, 8, 1, 1, 1e-5, None) == -2             # full resolution: never resident
    fa = lib.vs_conv_k3_bwd_data_fused_apply               # (g, act_x, act_stats, act_sums, w, y, mask_x, mask_stats, sums, dx_out, n, d, h, w, c, m, dtype, eps, stream)
    assert fa(fake, fake, fake, fake, fake, fake, fake, fake, None, None, 2, 96, 96, 96, 8, 8, 1, 1e-5, None) == -1          # mask without sums
    assert fa(fake, fake, None, fake, fake, fake, None, None, None, None, 2, 96, 96, 96, 8, 8, 1, 1e-5, None) == -1          # no activation statistics
    assert fa(fake, fake, fake, fake, fake, fake, None, None, None, None, 2, 24, 24, 24, 32, 32, 1, 1e-5, None) == -2        # 32-channel chunks keep the standalone apply
    assert fa(fake, fake, fake, fake, fake, fake, None, None, None, None, 2, 24, 24, 24, 32, 32, 0, 1e-5, None) == -2        # ... in fp32 too
    wg = lib.vs_conv_k3_bwd_data_wgrad                     # (g, act_x, act_stats, act_sums, w, y, mask_x, mask_stats, sums, slabs, n, d, h, w, c, m, dtype, eps, stream)
    assert wg(fake, None, None, None, fake, fake, fake, fake, fake, fake, 2, 48, 48, 48, 16, 16, 1, 1e-5, None) == -2        # 8 -> 8 only
    assert wg(fake, fake, None, fake, fake, fake, fake, fake, fake, fake, 2, 96, 96, 96, 8, 8, 1, 1e-5, None) == -1          # act_x without its statistics
    assert lib.vs_conv_gather_bwd_data(fake, fake, fake, fake, fake, None, 2, 24, 24, 24, 32, 32, 0, 1, 1e-5, None) == -1    # without sums
    assert lib.vs_conv_gather_fwd(fake, None, fake, None, fake, None, 1, 4, 4, 4, 8, 12, 0, 1, 1e-5, None) == -1             # m_out not a multiple of 8
    assert lib.vs_conv_gather_fwd(fake, None, fake, None, fake, None, 1, 4, 4, 4, 8, 8, 2, 1, 1e-5, None) == -1              # kind: neither K3 nor K2S2
    assert lib.vs_conv_gather_fwd(fake, None, fake, None, fake, None, 1, 4, 4, 4, 8, 1024, 0, 1, 1e-5, None) == -2           # more than 512 output channels
    assert lib.vs_conv_scatter_fwd(fake, None, fake, None, fake + 8, 1, 4, 4, 4, 8, 8, 1, 1e-5, None) == -1                  # y at +8 bytes
    assert lib.vs_conv_scatter_bwd_data(fake, fake, fake, None, fake, fake, 1, 4, 4, 4, 8, 8, 1, 1e-5, None) == -1           # without mask
    sb = lib.vs_conv_k3_softmax2_bwd_data                  # (prob, gprob, gprob_cl, w, y, mask_x, mask_stats, sums, slabs, bias_part, n, d, h, w, dtype, eps, drop_p, seed, stream)
    assert sb(fake, fake, None, fake, fake, fake, fake, fake, None, fake, 1, 16, 16, 16, 1, 1e-5, 0.0, 0, None) == -1        # bias partials without slabs
    assert sb(fake, fake, None, fake, fake, fake, fake, fake, fake, fake, 1, 16, 16, 16, 0, 1e-5, 0.0, 0, None) == -2        # fp32
    sf = lib.vs_conv_k3_softmax2_cl_fwd                    # (x, x_stats, w, bias, prob, prob_cl, n, d, h, w, c, dtype, eps, drop_p, seed, stream)
    assert sf(fake, None, fake, None, fake, None, 1, 16, 16, 16, 8, 1, 1e-5, 1.0, 0, None) == -1                             # drop_p 1.0
    assert sf(fake, None, fake, None, fake, None, 1, 16, 16, 16, 16, 1, 1e-5, 0.0, 0, None) == -2                            # 16 input channels
    assert sf(fake, None, fake, None, fake, fake, 1, 16, 16, 16, 8, 0, 1e-5, 0.0, 0, None) == -3                             # channels-last copy in fp32


def test_conv_plan_answers_are_pinned():
    """The conv launch planner's answers (csrc/conv_api.hip; the host queries of tools/conv_plan_table.py) over 6336 shapes under the default vs_config
    and ten single changes of it equal tests/golden/conv_plan.npz, a table made from the build BEFORE planning was split from launching: every entry, no exceptions."""
    import numpy as np
    from vae_segmentation_amd._lib import lib
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import conv_plan_table as P
    finally:
        sys.path.pop(0)
    want = np.load(os.path.join(REPO, "tests", "golden", "conv_plan.npz"), allow_pickle=False)
    got = P.table(lib.loaded()[0])
    assert want["answers"].shape == (len(P.CONFIGS), 6336, len(P.QUERIES))
    assert np.array_equal(got["tuples"], want["tuples"])
    assert got["answers"].dtype == want["answers"].dtype and (got["answers"] == want["answers"]).all()
    # the fixture itself is the table that was recorded then: tuples answering 1 by default, tuples whose six support answers move per configuration change
    a = want["answers"]
    assert [int((a[0, :, j] == 1).sum()) for j in range(6)] == [1114, 906, 1075, 1380, 2223, 192]
    assert [int((a[k, :, :6] != a[0, :, :6]).any(axis=1).sum()) for k in range(1, len(P.CONFIGS))] == [387, 14, 178, 32, 598, 502, 96, 3167, 192, 0]


def test_wgrad_plan_answers_are_pinned():
    """The host answers of the grouped weight-gradient path (csrc/wgrad.hip; tools/wgrad_plan_table.py): vs_conv_wgrad_multi_workspace_bytes of 16 descriptor
    lists under three storage types, the default vs_config and seven single changes of it, vs_conv_wgrad_workspace_bytes of their single layers, and the code
    of 96 rejected vs_conv_wgrad_multi calls (each refused on the host before its first launch: fake addresses) equal tests/golden/wgrad_plan.npz, a table made
    from the build BEFORE one planner served the size query and the launcher: every entry."""
    import numpy as np
    from vae_segmentation_amd._lib import lib
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import wgrad_plan_table as P
    finally:
        sys.path.pop(0)
    want = np.load(os.path.join(REPO, "tests", "golden", "wgrad_plan.npz"), allow_pickle=False)
    got = P.table(lib.loaded()[0])
    assert sorted(want.files) == sorted(got) == ["multi_bytes", "rejected", "rejected_bf16_bytes", "single_bytes", "singles"]
    assert want["multi_bytes"].shape == (len(P.CONFIGS), 16, 3) and want["rejected"].shape == (96,) and want["single_bytes"].shape == (len(P.CONFIGS), len(want["singles"]))
    for name in want.files:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape and (got[name] == want[name]).all(), name
    # the fixture itself: every accepted list has a size in 16-bit storage, the fp32 mode refuses exactly the three lists with slab descriptors, every
    # configuration change moves some answer, and every rejected call was refused with one of the library's own codes
    mb = want["multi_bytes"]
    assert (mb[:, :, 1:] > 0).all() and (mb[:, :, 1] == mb[:, :, 2]).all() and [int((mb[k, :, 0] == 0).sum()) for k in range(len(P.CONFIGS))] == [3] * len(P.CONFIGS)
    assert all(int((mb[k] != mb[0]).sum()) > 0 for k in range(1, len(P.CONFIGS)))
    assert sorted(set(want["rejected"].tolist())) == [-4, -3, -2, -1]


def test_grouped_weight_gradient_planning_without_gpu():
    """vs_conv_wgrad_multi's host side: descriptor layout (ctypes mirror == C struct), workspace planning and rejection of bad
    descriptors happen before any launch."""
    from vae_segmentation_amd import ops
    from vae_segmentation_amd._lib import lib, VS_BF16, VS_F32, VS_CONV_K3, VS_CONV_K2S2
    assert ctypes.sizeof(ops.WgradDesc) == 112
    fake = 0x10000

    counter = [0]

    def desc(n, d, h, w, m_ch, c_ch, kind, m_real=None, c_real=None, bias=False, dw=None):
        counter[0] += 1
        dst = dw if dw is not None else fake + 0x100000 * counter[0]          # a destination of its own: descriptors sharing dw are parts of one gradient
        x = ops.WgradDesc(fake, None, fake, None, dst, None, None, 0, 0, 0, n, d, h, w, m_ch, c_ch, m_real or m_ch, c_real or c_ch, kind, 0)
        if bias:
            x.bias_g, x.db, x.bias_rows, x.bias_c_ch, x.bias_c_real = fake, dst + 0x80000, n * d * h * w, m_ch, m_real or m_ch
        return x

    layers = [desc(2, 96, 96, 96, 8, 8, VS_CONV_K3), desc(2, 48, 48, 48, 16, 16, VS_CONV_K3), desc(2, 6, 6, 6, 128, 128, VS_CONV_K3),
              desc(2, 24, 24, 24, 32, 32, VS_CONV_K2S2, bias=True), desc(2, 48, 48, 48, 8, 8, VS_CONV_K2S2, bias=True)]
    arr = (ops.WgradDesc * len(layers))(*layers)
    grouped = lib.vs_conv_wgrad_multi_workspace_bytes(ctypes.addressof(arr), len(layers), VS_BF16)
    single = [lib.vs_conv_wgrad_workspace_bytes(x.n, x.dp, x.hp, x.wp, x.m_ch, x.c_ch, x.kind) for x in layers]
    # grouped: every layer owns a slab region (they run in one grid); fp32 mode: the 3x3x3 layers likewise (grouped limb launches, csrc/wgrad.hip
    # g3x_group_kernel) and, since round 4, the stride-2 layers (g3_group_kernel: one grid per channel-block width, <= 8 tiles per workgroup)
    assert grouped > 0 and grouped % 16 == 0
    assert grouped >= 128 * 128 * 27 * 4                       # at least one slab of the 128x128 layer
    f32 = lib.vs_conv_wgrad_multi_workspace_bytes(ctypes.addressof(arr), len(layers), VS_F32)
    k2 = (ops.WgradDesc * 2)(*layers[3:])
    k2_f32 = lib.vs_conv_wgrad_multi_workspace_bytes(ctypes.addressof(k2), 2, VS_F32)
    nobias = (ops.WgradDesc * 2)(desc(2, 24, 24, 24, 32, 32, VS_CONV_K2S2), desc(2, 48, 48, 48, 8, 8, VS_CONV_K2S2))
    k2_nobias = lib.vs_conv_wgrad_multi_workspace_bytes(ctypes.addressof(nobias), 2, VS_F32)
    # 32 -> 32 at 24^3: 2 x 6 x 6 x 2 = 144 tiles x 4 block pairs, <= 8 tiles per workgroup -> >= 18 slabs of 4 x 8 taps x 256 floats; plus the 8 -> 8 layer's
    assert k2_nobias >= 18 * 4 * 8 * 256 * 4 and k2_nobias % 16 == 0
    assert k2_nobias < k2_f32 <= k2_nobias + 2 * 256 * 32 * 8 + 512                    # + the two bias layers' partial sums
    assert f32 >= k2_f32 + 128 * 128 * 27 * 4 and f32 % 16 == 0
    assert lib.vs_conv_wgrad_multi(ctypes.addressof(arr), len(layers), None, 0, VS_BF16, 1e-5, None) == -1      # no workspace
    assert lib.vs_conv_wgrad_multi(ctypes.addressof(arr), len(layers), fake, 16, VS_BF16, 1e-5, None) == -4      # VS_EWORKSPACE
    # a weight used several times in one pass: descriptors with the same destination are summed — their slabs lie side by side
    one = (ops.WgradDesc * 1)(desc(1, 24, 24, 24, 32, 32, VS_CONV_K3, dw=fake))
    two = (ops.WgradDesc * 2)(desc(1, 24, 24, 24, 32, 32, VS_CONV_K3, dw=fake), desc(1, 12, 12, 12, 32, 32, VS_CONV_K3, dw=fake))
    for dt in (VS_BF16, VS_F32):
        assert lib.vs_conv_wgrad_multi_workspace_bytes(ctypes.addressof(two), 2, dt) > lib.vs_conv_wgrad_multi_workspace_bytes(ctypes.addressof(one), 1, dt) > 0
    mixed = (ops.WgradDesc * 2)(desc(1, 8, 8, 8, 32, 32, VS_CONV_K3, dw=fake), desc(1, 8, 8, 8, 32, 16, VS_CONV_K3, dw=fake))   # same destination, other layer
    assert lib.vs_conv_wgrad_multi_workspace_bytes(ctypes.addressof(mixed), 2, VS_BF16) == 0
    assert lib.vs_conv_wgrad_multi(ctypes.addressof(mixed), 2, fake, 1 << 24, VS_BF16, 1e-5, None) == -1
    bad = (ops.WgradDesc * 1)(desc(2, 8, 8, 8, 12, 8, VS_CONV_K3))                                               # channels not a multiple of 8
    assert lib.vs_conv_wgrad_multi_workspace_bytes(ctypes.addressof(bad), 1, VS_BF16) == 0
    assert lib.vs_conv_wgrad_multi(ctypes.addressof(bad), 1, fake, 1 << 20, VS_BF16, 1e-5, None) == -2
    # fused Dice-loss sum: scratch sizing and argument checks
    assert lib.vs_dice_loss_multi_scratch_doubles(2, 2, 2) == 3 * 2 * 2 * 2 + 2 * 2 * 5 * 256
    assert lib.vs_dice_loss_multi_fwd(None, None, None, 2, None, None, None, 2, 2, 64, 1, 2, 1e-4, None) == -1
    tp = (ctypes.c_void_p * 5)(*[fake] * 5)
    wp = (ctypes.c_float * 5)(*[1.0] * 5)
    assert lib.vs_dice_loss_multi_fwd(fake, ctypes.addressof(tp), ctypes.addressof(wp), 5, fake, fake, fake, 2, 2, 64, 1, 2, 1e-4, None) == -1   # k > 4
    assert lib.vs_dice_loss_multi_fwd(fake, ctypes.addressof(tp), ctypes.addressof(wp), 2, fake, fake, fake, 2, 2, 63, 1, 2, 1e-4, None) == -5   # voxels % 4


def test_host_helpers():
    from vae_segmentation_amd import ops
    assert [ops.cpad(c) for c in (1, 2, 8, 9, 16, 17, 32, 33, 256)] == [8, 8, 8, 16, 16, 32, 32, 64, 256]
    from tests import golden_util as G
    assert G.is_dead_bias("in_block.conv.0.bias") and G.is_dead_bias("up5.conv.1.conv.6.bias")
    assert not G.is_dead_bias("down1.conv.0.bias") and not G.is_dead_bias("out_block.bias") and not G.is_dead_bias("fc2.bias")
    with pytest.raises(RuntimeError):
        ops._require_cuda(torch.zeros(1))


def test_stat_pair_helpers_decode_both_builds_and_match_two_pass_numpy():
    """tests/stats_util.py, the per-(n, c) statistics gate of the GPU suite: ops.stats_total decodes a hand-built buffer of each build (four
    fp64 partial copies / four fixed-point limbs), the pair_to_mean_rstd arithmetic on it matches numpy's two-pass mean and rstd at channel
    offsets R up to 300, and the gate rejects a pair that lost one tile's partial or took its neighbour's."""
    import numpy as np
    from vae_segmentation_amd import ops
    from vae_segmentation_amd._lib import lib
    from tests import stats_util as SU
    rng = np.random.default_rng(5)
    n, c, V = 2, 8, 4096
    R = np.array([0.0, 4.0, 30.0, 300.0] * 2) * np.array([1, 1, -1, -1, 1, -1, 1, -1])
    y = rng.standard_normal((n, c, V)) * 0.7
    y = (y - y.mean(-1, keepdims=True)) / y.std(-1, keepdims=True) * 2.5 + (R * 2.5)[None, :, None]
    ref = SU.two_pass(torch.from_numpy(y))
    assert np.allclose(ref["mean"].numpy(), y.mean(-1), rtol=0, atol=1e-12 * np.abs(y).max())
    assert np.allclose(ref["std"].numpy(), y.std(-1), rtol=1e-12)
    assert np.allclose(ref["R"].numpy(), np.abs(R)[None, :].repeat(n, 0), rtol=1e-9, atol=1e-9)
    tot = torch.from_numpy(np.stack([y.sum(-1), (y * y).sum(-1)], -1))
    m, r = SU.pair_mean_rstd(tot, V)
    assert np.allclose(m.numpy(), y.mean(-1), rtol=1e-13, atol=1e-13)
    assert np.abs(r.numpy() * np.sqrt(y.var(-1) + 1e-5) - 1).max() < 1e-9          # one-pass fp64: ~R^2 * 2^-52 relative in var
    was = ops.is_deterministic()
    try:
        ops.set_deterministic(True)
        det = ops.stats_total(SU.pack_limbs(tot, interleaved=bool(lib.vs_stat_interleaved())))
        assert det.shape == (n, c, 2) and float(((det - tot).abs() / tot.abs()).max()) < 1e-15
        ops.set_deterministic(False)
        parts = torch.stack([tot * 0.5, tot * 0.25, -tot * 0.125, tot * 0.375])         # four partial copies that add up to tot
        if lib.vs_stat_interleaved():
            parts = parts.permute(1, 2, 0, 3).contiguous().view(4, n, c, 2)
        assert float(((ops.stats_total(parts) - tot).abs() / tot.abs()).max()) < 1e-15
    finally:
        ops.set_deterministic(was)
    SU.check_stats(det, ref, "exact pairs")
    # one 16x16 tile's partial of (0, 2) lost; one of (1, 5) credited to (0, 5) — the R = 30 channels
    for (nn, cc, src) in ((0, 2, None), (0, 5, 1)):
        bad = tot.clone()
        part = torch.from_numpy(np.stack([y[nn if src is None else src, cc, :256].sum(), (y[nn if src is None else src, cc, :256] ** 2).sum()]))
        bad[nn, cc] += part if src is not None else -part
        if src is not None:
            bad[src, cc] -= part
        with pytest.raises(AssertionError, match="per-\\(n, c\\) statistics off"):
            SU.check_stats(bad, ref, "lost partial")
    # at the realistic scale: one 64-voxel tile of 1700 (a 96^3 sample has ~1700 tiles).  At R = 30 the mean and sum bounds fire ten times over;
    # in a centred channel (R = 0) the same loss moves mean and sum by the tile's noise only, ~1e-5: marginal — why the GPU suite offsets its data
    V = 64 * 1700
    z = rng.standard_normal((1, 2, V))
    z = (z - z.mean(-1, keepdims=True)) / z.std(-1, keepdims=True) + np.array([0.0, 30.0])[None, :, None]
    zt = torch.from_numpy(np.stack([z.sum(-1), (z * z).sum(-1)], -1))
    zref = SU.two_pass(torch.from_numpy(z))
    lost = zt - torch.from_numpy(np.stack([z[..., :64].sum(-1), (z[..., :64] ** 2).sum(-1)], -1))
    err = SU.stat_errors(lost, zref)
    assert float(err["mean"][0, 1]) > 1e-5 * 31 * 10 and float(err["sum"][0, 1]) > 1e-5 * 10      # R = 30: 10x over both bounds
    assert float(err["mean"][0, 0]) < float(err["mean"][0, 1]) / 50 and float(err["sum"][0, 0]) < float(err["sum"][0, 1]) / 50     # R = 0
    with pytest.raises(AssertionError, match="mean at"):
        SU.check_stats(lost[:, 1:], {k: (v[:, 1:] if torch.is_tensor(v) else v) for k, v in zref.items()}, "one tile of 1700 lost, R = 30")


def test_module_surface_on_cpu_is_constructible_but_not_runnable():
    import joint_model as M
    seg = M.Segmentation(1, 2, norm_type=1)
    vae = M.VAE(2, 2, norm_type=1, dim=128, spatial=96)
    assert vae.fc_mean.weight.shape == (128, 6912) and vae.fc2.weight.shape == (6912, 128)
    joint = M.Joint(models=[seg, vae])
    assert [n.split(".")[0] for n, _ in joint.named_parameters()][0] == "Seg"
    with pytest.raises(RuntimeError):
        joint({"x": torch.zeros(1, 1, 96, 96, 96)}, "x", "p", "r")
    bn = M.Segmentation(1, 2)                                # the constructors' default norm_type=2: BatchNorm3d holders, reference state_dict keys
    assert "in_block.conv.1.running_var" in bn.state_dict() and isinstance(M.DoubleConv(8, 8, norm_type=1, soft=True).conv[2], torch.nn.Softplus)
    gs = M.Segmentation(1, 2, norm_type=3)                   # GSNorm3d holders (joint_model.py:14-15): parameter-less, same state_dict keys as norm_type=1
    assert list(gs.state_dict().keys()) == list(M.Segmentation(1, 2, norm_type=1).state_dict().keys())
    with pytest.raises(ValueError):
        M.Segmentation(1, 2, norm_type=4)
    assert M.Segmentation(1, 3, norm_type=1).out_block.weight.shape[0] == 3 and M.VAE(5, 5, norm_type=1, dim=128).in_block.conv[0].weight.shape[1] == 5
    with pytest.raises(NotImplementedError):                 # the probabilities travel in one 8-channel fragment
        M.Segmentation(1, 9, norm_type=1)


WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
from vae_segmentation_amd.ddp import FlatGradSync
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.manual_seed(0)
params = [torch.nn.Parameter(torch.randn(3, 4)), torch.nn.Parameter(torch.randn(7))]
if rank == 1:
    for p in params: p.data.add_(1.0)          # replicas start different; broadcast must fix that
sync = FlatGradSync(params)
sync.broadcast_parameters(0)
ref0 = [torch.randn(3, 4, generator=torch.Generator().manual_seed(10)), torch.randn(7, generator=torch.Generator().manual_seed(11))]
ref1 = [torch.randn(3, 4, generator=torch.Generator().manual_seed(20)), torch.randn(7, generator=torch.Generator().manual_seed(21))]
mine = ref0 if rank == 0 else ref1
views = sync([g.clone() for g in mine])
for v, a, b in zip(views, ref0, ref1):
    assert torch.allclose(v, (a + b) / 2, atol=1e-6), "rank %%d: averaged gradient mismatch" %% rank
chk = torch.cat([p.data.reshape(-1) for p in params])
gathered = [torch.zeros_like(chk) for _ in range(world)]
dist.all_gather(gathered, chk)
assert torch.equal(gathered[0], gathered[1]), "parameters differ across ranks after broadcast"
dist.destroy_process_group()
print("rank %%d ok" %% rank)
"""


def test_ddp_flat_grad_sync_gloo_world2(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER % REPO)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
    assert all("ok" in o for o in outs)


def test_capture_safe_accumulators_detects_graphs_of_earlier_passes():
    """train.capture_safe_accumulators (GraphedStep's guard): gradient accumulators nobody owns are re-created under the caller's stream,
    ones it tagged earlier are accepted, ones an older autograd graph keeps alive are reported instead of being captured over."""
    import torch
    from vae_segmentation_amd import train as T
    ps = [torch.nn.Parameter(torch.randn(3)) for _ in range(3)] + [torch.nn.Parameter(torch.randn(2), requires_grad=False)]
    a = T.capture_safe_accumulators(ps)
    assert len(a) == 3
    b = T.capture_safe_accumulators(ps)                      # the first call's nodes are alive and tagged
    assert all(x is y for x, y in zip(a, b))
    del a, b
    loss = sum((p * 2).sum() for p in ps[:3])
    with pytest.raises(RuntimeError, match="earlier eager pass"):
        T.capture_safe_accumulators(ps)
    del loss
    assert len(T.capture_safe_accumulators(ps)) == 3


def test_main_target_parses_every_reference_flag_with_the_reference_defaults(capsys):
    """VERDICT r04 (missing 7): a reference command line must not abort in argparse.  The table is the reference's parser
    (main_target.py:29-81: option strings, defaults) as data."""
    import main_target
    ref_defaults = {
        "target_phase": "arterial", "GPU": "0,1,2,3", "batch_size": 4, "max_epoch": 1600, "save_epoch": 50, "eval_epoch": 50, "turn_epoch": -1,
        "softrelu": 0, "method": "vae_train", "data_root": "../nih_data/numpy_data/", "val_data_root": "../nih_data/numpy_data/",
        "pseudo_data_root": "../nih_data/numpy_data/", "data_path": "Multi_all.json", "train_list": "NIH_train", "val_list": "NIH_val",
        "pseudo_list": None, "load_prefix": None, "checkpoint_name": "best_model.ckpt", "load_prefix_vae": None, "load_prefix_encoder": None,
        "load_prefix_joint": None, "pan_index": "1", "pseudo_pan_index": "1", "lambda_vae": 0.1, "lambda_vae_warmup": 0, "lr_seg": 1e-2, "lr_vae": 0,
        "test_only": False, "resume": False, "save_more_reference": False, "save_eval_result": False, "no_aug": False, "only_pseudo": False,
        "fix_layer": False, "use_confident_binarize": False, "analysis_figure_name": None, "pseudo_save_epoch": 0, "domain_loss_type": 0,
        "vae_mont_number": 1, "vae_forward_scale": 0.0, "vae_decoder_dropout": 0.0, "seg_dropout": 0.0, "val_finetune": 0, "lr_finetune": 1e-2,
        "tag": False, "from_scratch": False, "adam": False, "kl": False, "alpha": 0.995, "update_every_iteration": False,
        "generate_bounding_boxes": False, "shift": 0}
    a = main_target.parse(["run0"])
    assert a.prefix == "run0"
    for k, v in ref_defaults.items():
        assert getattr(a, k) == v, (k, getattr(a, k), v)
    # a command line that uses every remaining option string of the reference at once (pseudo_list aside: see below)
    a = main_target.parse(["run1", "-P", "venous", "-G", "0", "-b", "2", "-E", "10", "--save_epoch", "5", "--eval_epoch", "5", "--turn_epoch", "2", "-S", "1",
                           "-M", "domain_adaptation", "--data_root", "d", "--val_data_root", "v", "--pseudo_data_root", "p", "-l", "x.json",
                           "--train_list", "T", "--val_list", "V", "--load_prefix", "a", "--checkpoint_name", "c.ckpt", "--load_prefix_vae", "b",
                           "--load_prefix_encoder", "e", "--load_prefix_joint", "j", "--pan_index", "1,2", "--pseudo_pan_index", "1", "--lambda_vae", "1.0",
                           "--lambda_vae_warmup", "3", "--lr_seg", "1e-3", "--lr_vae", "0", "--resume", "--save_more_reference", "--save_eval_result",
                           "--no_aug", "--fix_layer", "--use_confident_binarize", "--analysis_figure_name", "fig", "--pseudo_save_epoch", "1",
                           "--domain_loss_type", "8", "--vae_mont_number", "2", "--vae_forward_scale", "0.35", "--vae_decoder_dropout", "0.1",
                           "--seg_dropout", "0.1", "--val_finetune", "1", "--lr_finetune", "1e-3", "--tag", "--from_scratch", "--adam", "--kl",
                           "--alpha", "0.99", "--update_every_iteration", "--generate_bounding_boxes", "--shift", "4"])
    assert a.fix_layer and a.from_scratch and a.vae_mont_number == 2 and a.vae_forward_scale == 0.35 and a.shift == 4 and a.load_prefix_encoder == "e"
    assert "accepted and ignored" in capsys.readouterr().err                       # the dump / figure flags say what happens to them
    with pytest.raises(SystemExit, match="inconsistent flags"):                                            # main_target.py:145: more than one pass needs a forward scale
        main_target.parse(["r", "--vae_mont_number", "2"])
    a = main_target.parse(["r", "-M", "domain_adaptation", "--pseudo_list", "NIH_pseudo", "--pseudo_pan_index", "1"])     # main_target.py:228-307,615-692
    assert a.pseudo_list == "NIH_pseudo"
    with pytest.raises(SystemExit, match="pseudo_list"):                           # the reference's other methods never read the second loader (:689)
        main_target.parse(["r", "-M", "domain_adaptation_dis", "--pseudo_list", "NIH_pseudo"])


def test_synthetic_matches_the_oracle_generators():
    """bench.py builds its workload from vae_segmentation_amd/synthetic.py (product code, no oracle import in the benchmark's set-up); the values are
    the oracle's fixtures' (oracle/ref_cpu.py), so `final_loss` in the bench line stays comparable with the goldens' inputs."""
    import torch
    from oracle import ref_cpu as O
    from vae_segmentation_amd import synthetic as S
    assert torch.equal(S.synthetic_image(2, 12, 7), O.synthetic_image(2, 12, 7))
    assert torch.equal(S.synthetic_label(2, 12, 9), O.synthetic_label(2, 12, 9))
    a, b = O.Segmentation(1, 2, norm_type=1), O.Segmentation(1, 2, norm_type=1)
    S.deterministic_fill_(a, seed=3)
    O.deterministic_fill_(b, seed=3)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    src = open(os.path.join(REPO, "bench.py")).read()
    build_src = src[src.index("def build("):src.index("def usable_cores")]
    assert "oracle" not in build_src.replace("the oracle is imported by cpu_baseline only", "")


def test_config_struct_layout_and_single_entry_point():
    """include/vaeseg.h vs_config: the Python binding's struct is the library's, the environment seeds it once, vs_set_config is the only writer and
    validates what it is given (no GPU needed)."""
    from vae_segmentation_amd import ops
    import ctypes
    assert ops.lib.vs_config_bytes() == ctypes.sizeof(ops.VsConfig)
    cfg = ops.get_config()
    assert cfg["chain"] in (0, 1) and cfg["wgrad_wgs"] >= 1 and cfg["k3x_ck"] in (8, 16)
    old = ops.set_config(wgrad_mpack=0, wgrad_big_min_voxels=123)
    try:
        now = ops.get_config()
        assert now["wgrad_mpack"] == 0 and now["wgrad_big_min_voxels"] == 123 and now["chain"] == cfg["chain"]
        assert ops.lib.vs_conv_k3_chain_supported(2, 6, 6, 6, 128, 1) == (1 if cfg["chain"] else 0)
        ops.set_config(chain=0)
        assert ops.lib.vs_conv_k3_chain_supported(2, 6, 6, 6, 128, 1) == 0
        ops.set_config(chain=cfg["chain"])
        with pytest.raises(KeyError):
            ops.set_config(no_such_switch=1)
        with pytest.raises(RuntimeError):
            ops.set_config(k3x_ck=12)                     # rejected by the library, nothing installed
        assert ops.get_config()["k3x_ck"] == cfg["k3x_ck"]
    finally:
        ops.set_config(**old)
    assert ops.get_config() == cfg
    src = "".join(open(os.path.join(REPO, "vae_segmentation_amd", "csrc", f)).read() for f in os.listdir(os.path.join(REPO, "vae_segmentation_amd", "csrc"))
                  if f.endswith((".h", ".hip", ".inc")) and f != "config.hip")
    assert src.count("getenv(") == 2, "launchers read vs_cfg(), not the environment (the two left sit inside the VS_G3B_ABLATE diagnostic build)"


def test_wgrad_xcd_rank_model_is_a_bijection():
    """csrc/wgrad.hip g3_xcd_rank (round 6): a layer's workgroups [b0, b0 + count) of the grouped weight-gradient grid are re-ranked so that XCD x (= workgroup
    id mod 8) owns one contiguous run of ranks.  The same arithmetic in Python: every rank is hit exactly once for any start and count, and the ranks of one XCD
    are consecutive (what puts the channel-block pairs of a tile, rank = k-split * pairs + pair, into one L2)."""
    import random

    def rank(b0, local, count):
        x = (b0 + local) & 7
        start = 0
        for xx in range(8):
            first = (xx - b0) & 7
            cnt = (count - first + 7) >> 3 if first < count else 0
            if xx < x:
                start += cnt
        return start + ((local - ((x - b0) & 7)) >> 3)

    src = open(os.path.join(REPO, "vae_segmentation_amd", "csrc", "wgrad.hip")).read()
    assert "const int first = (xx - b0) & 7;" in src and "return start + ((local - ((x - b0) & 7)) >> 3);" in src      # the model is the kernel's formula
    rng = random.Random(1)
    for _ in range(300):
        b0, count = rng.randrange(0, 5000), rng.randrange(16, 1500)
        ranks = [rank(b0, l, count) for l in range(count)]
        assert sorted(ranks) == list(range(count)), (b0, count)
        for x in range(8):
            mine = sorted(r for l, r in enumerate(ranks) if (b0 + l) & 7 == x)
            assert mine == list(range(mine[0], mine[0] + len(mine))) if mine else True


def test_isa_phase_counts_finds_the_tile_loop_of_k3t():
    """tools/isa_phase_counts.py (no GPU: device-only compile to assembly): the persistent loop of the 8-channel full-resolution kernel holds the tile's 72 MFMAs
    (9 k-groups x 8 output rows), two barriers per tile plus the statistics flush's, and a vector instruction count in the range DESIGN.md section 9 reasons with."""
    import re
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "isa_phase_counts.py"), os.path.join(REPO, "vae_segmentation_amd", "csrc", "igemm_k3_bf16.hip"),
                          "k3t_kernel<0, false, 8, true, unsigned short, false>"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"loop: (\d+) instructions, (\d+) barriers", out.stdout)
    assert m and int(m.group(2)) == 3, out.stdout
    tot = [ln for ln in out.stdout.splitlines() if ln.startswith("loop total")][0].split()
    valu, packed, mfma = int(tot[2]), int(tot[3]), int(tot[4])
    assert mfma == 72 and 300 <= valu + packed <= 800, out.stdout


def test_isa_diff_verdicts_on_inline_assembly():
    """tools/isa_diff.py's comparison (no compile): equal text is `identical`, scalar moves that traded places are `equivalent` (the same count of every
    mnemonic, the same descriptor), one extra instruction is DIFFERENT, and a symbol that only one side has is reported as such.  A file split into
    several (--moved) is compared against the union of their symbols; a symbol two of them carry counts once if its text is equal and is DIFFERENT if not."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import isa_diff
    finally:
        sys.path.pop(0)

    def asm(body, ident="a", extra=""):
        return ("\t.file\t\"%s.hip\"\n\t.type\tkern,@function\nkern:\n%s\ts_endpgm\n.Lfunc_end0:\n\t.size\tkern, .Lfunc_end0-kern\n"
                "\t.amdhsa_kernel kern\n\t\t.amdhsa_next_free_vgpr 4\n\t\t.amdhsa_group_segment_fixed_size 0\n\t.end_amdhsa_kernel\n%s\t.ident\t\"%s\"\n"
                % (ident, body, extra, ident))

    base = "\ts_mov_b32 s0, s2\n\ts_mov_b32 s1, s3\n\tv_add_f32_e32 v0, v1, v2\n"
    swapped = "\ts_mov_b32 s1, s3\n\ts_mov_b32 s4, s2\n\tv_add_f32_e32 v0, v1, v2\n"
    longer = base + "\tv_add_f32_e32 v0, v0, v0\n"
    assert isa_diff.compare(asm(base), asm(base, ident="b")) == {"kern": "identical"}
    assert isa_diff.compare(asm(base), asm(swapped)) == {"kern": "equivalent"}
    assert isa_diff.compare(asm(base), asm(longer)) == {"kern": "DIFFERENT"}
    assert isa_diff.compare(asm(base), asm(base).replace("next_free_vgpr 4", "next_free_vgpr 5")) == {"kern": "DIFFERENT"}
    other = "\t.type\tlone,@function\nlone:\n\ts_endpgm\n\t.size\tlone, 4\n"
    assert isa_diff.compare(asm(base), asm(base, extra=other)) == {"kern": "identical", "lone": "only in new"}
    # --moved: one old file against the union of the files its code went to.  `shared` stands for a static kernel of a header both new files include
    shared = "\t.type\tshared,@function\nshared:\n\ts_nop 0\n\ts_endpgm\n\t.size\tshared, 8\n"
    old = asm(base, extra=other + shared)
    new_a, new_b = asm(swapped, extra=shared), shared + other + "\t.ident\t\"b\"\n"
    assert isa_diff.compare_moved(old, [new_a, new_b]) == {"kern": "equivalent", "lone": "identical", "shared": "identical"}
    assert isa_diff.compare_moved(old, [new_b, new_a]) == isa_diff.compare_moved(old, [new_a, new_b])
    assert isa_diff.compare_moved(old, [new_a]) == {"kern": "equivalent", "lone": "only in old", "shared": "identical"}
    assert isa_diff.compare_moved(asm(base), [new_a, new_b]) == {"kern": "equivalent", "shared": "only in new", "lone": "only in new"}
    unequal = new_b.replace("s_nop 0", "s_nop 1")
    assert isa_diff.compare_moved(old, [new_a, unequal]) == {"kern": "equivalent", "lone": "identical", "shared": "DIFFERENT"}
    assert isa_diff.compare_moved(asm(base), [new_a, unequal])["shared"] == "DIFFERENT"      # whatever the old file held


def test_bench_dump_outputs_budget_and_fixed_sample(tmp_path):
    """bench.py --dump-outputs (no GPU: the writer alone): float32 .npy files, 64 MB in all; outputs that fit are written whole, the larger ones as a
    sample of positions that are the same in every run (two builds compare output for output), in ascending order."""
    import numpy as np
    sys.path.insert(0, REPO)
    import bench
    n = 2 * 2 * 160 ** 3                         # the prediction of one GPU's share of configs[4]: two of them do not fit
    outs = {"loss": torch.tensor(0.25, dtype=torch.float64), "w": torch.randn(1000), "pred": torch.randn(n).bfloat16().view(2, 2, 160, 160, 160),
            "recon": torch.arange(n, dtype=torch.float32).view(2, 2, 160, 160, 160)}          # values = positions (exact below 2^24)
    for d in ("a", "b"):
        bench.dump_outputs(outs, str(tmp_path / d))
    a, b = ({f[:-4]: np.load(tmp_path / d / f) for f in os.listdir(tmp_path / d)} for d in ("a", "b"))
    assert set(a) == set(outs) and all(x.dtype == np.float32 for x in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_BYTES == 64 * 10**6
    assert a["loss"].shape == () and float(a["loss"]) == 0.25 and np.array_equal(a["w"], outs["w"].numpy())
    assert all(np.array_equal(a[k], b[k]) for k in a)
    r = a["recon"]
    assert r.ndim == 1 and n // 4 < r.size < n and np.all(np.diff(r) > 0) and np.array_equal(r, np.round(r)) and r[-1] < n


VOLUME_NAMES = (
    "cc_max_components", "cc_label", "keep_largest",
    "SURFACE_RECORD_FIELDS", "surface", "edt", "surface_distances",
    "MORPH_OPS", "morph", "binary_dilation", "binary_erosion", "binary_opening", "binary_closing", "fill_holes",
    "REGION_COLUMNS", "CONTINGENCY_MAX_CELLS", "region_props", "contingency",
    "HISTOGRAM_MAX_BINS", "HISTOGRAM_MAX_CELLS", "MI_MAX_RADIUS", "MI_MAX_PLANES", "histogram", "joint_histogram", "mutual_information",
    "SW_BLENDS", "SW_GAUSSIAN_FLOOR", "sw_plan_host", "sw_plan", "sw_weights", "sw_flips", "sw_gather", "sw_accumulate", "sw_finalize",
    "UNCROP_INTERPS", "uncrop",
    "SCAN_DTYPES", "scan_orient", "to_native",
    "AUG_MAX_SIGMA", "AUG_OPS", "aug_stats", "philox_normal", "gaussian_weights", "blur_tile", "gaussian_blur3d", "aug_flip", "aug_stage",
    "ZOOM_EDGE_ORDERS", "ZOOM_EDGE_MAX_LEN", "zoom_edge_bundle", "zoom_edge", "simulate_lowres",
    "QUANTILE_MAX_Q", "QUANTILE_WG_VOXELS", "INTENSITY_MAP_MAX_L", "INTENSITY_MAP_WG_VOXELS", "INTENSITY_MAP_EXTRAPOLATE", "quantile", "intensity_map")


def test_volume_names_reexported():
    """the forward-only volume utilities live in volume.py; ops re-exports its public names, the very objects, and none of its private ones"""
    from vae_segmentation_amd import ops, volume
    assert len(VOLUME_NAMES) == len(set(VOLUME_NAMES)) == 60
    for name in VOLUME_NAMES:
        assert getattr(ops, name) is getattr(volume, name), name
    assert set(volume.__all__) == set(VOLUME_NAMES)
    assert not hasattr(ops, "_check_connectivity") and not hasattr(ops, "_rows")


def test_volume_imports_without_ops():
    """the data pipeline and the volume utilities load without the autograd wrappers"""
    code = ("import sys; sys.path.insert(0, %r); import vae_segmentation_amd.volume, vae_segmentation_amd.data_gpu; "
            "assert 'vae_segmentation_amd.ops' not in sys.modules; print('ok')" % REPO)
    run = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert run.returncode == 0 and run.stdout.decode().strip().endswith("ok"), run.stdout.decode()


# ---- ops._PENDING: what one backward pass owns, and its one end-of-pass callback (CPU tensors and a toy Function: no device) ----
class _InPass(torch.autograd.Function):
    """identity whose backward runs fn() — inside a backward pass of the autograd engine"""

    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        return x * 2

    @staticmethod
    def backward(ctx, g):
        ctx.fn()
        return g * 2, None


def _run_pass(fn):
    x = torch.ones(3, requires_grad=True)
    _InPass.apply(x, fn).sum().backward()
    return x


def _pass_is_empty(ops):
    p = ops._PENDING
    return not (p["grads"] or p["unapplied"] or p["slots"] or p["dead_biases"] or p["up_jobs"] or p["queued"])


@pytest.fixture
def pass_ops():
    from vae_segmentation_amd import ops
    ops.drop_stale_wgrads()
    assert _pass_is_empty(ops) and ops.pending_wgrads() == 0
    yield ops
    ops._GROUP["descs"], ops._GROUP["keep"] = [], []
    ops.drop_stale_wgrads()


def _unapplied(ops, seed):
    """register an un-applied gradient as a conv backward does -> g"""
    g, x = torch.full((2, 3), float(seed)), torch.zeros(2, 3)
    assert ops._finish(g, x, torch.zeros(4), torch.zeros(4), True) is g
    return g


def test_pass_state_nothing_queued_outside_a_pass(pass_ops):
    ops = pass_ops
    assert ops._PENDING.join() is False and ops._PENDING["queued"] is False
    ops._park_gradient(torch.zeros(2), torch.ones(2))           # stored, but no callback: nothing will call back
    assert len(ops._PENDING["grads"]) == 1 and ops._PENDING["queued"] is False
    ops.drop_stale_wgrads()
    assert _pass_is_empty(ops)


def test_pass_state_callback_queued_once_runs_once_after_the_pass(pass_ops, monkeypatch):
    """the callback is queued once per pass however many parts register, and runs once, after backward() returned from the last node"""
    ops = pass_ops
    ran, seen, done = [], [], ops._pass_done
    monkeypatch.setattr(ops, "_pass_done", lambda: (ran.append(1), done())[1])
    x0, held = torch.zeros(2), []

    def parts():
        first = ops._PENDING.join()
        ops._park_gradient(x0, torch.ones(2))
        held.append(_unapplied(ops, 1))
        seen.append((first, ops._PENDING.join(), ops._PENDING["queued"], len(ran)))
        assert ops._collect_gradient(x0) is not None and ops._take_lazy(held[0]) is not None

    assert ops._PENDING.join() is False and ops._PENDING["queued"] is False and not ran
    x = torch.ones(3, requires_grad=True)
    y = _InPass.apply(x, parts).sum()
    assert not seen and not ran
    y.backward()
    assert seen == [(True, True, True, 0)]                   # queued by the first call alone, and not run before backward() returned
    assert ran == [1] and _pass_is_empty(ops)                # run once, after the pass; it clears the mark with everything else
    assert torch.equal(x.grad, torch.full((3,), 2.0))


def test_pass_state_parked_gradient(pass_ops):
    ops = pass_ops
    x0, g0 = torch.zeros(2), torch.ones(2)
    _run_pass(lambda: (ops._park_gradient(x0, g0), ops._collect_gradient(x0)))
    assert _pass_is_empty(ops)
    with pytest.raises(RuntimeError, match=r"1 parked skip gradient\(s\) were never collected by the conv that shares their input: gradients lost"):
        _run_pass(lambda: ops._park_gradient(x0, g0))
    assert _pass_is_empty(ops)


def test_pass_state_unapplied_gradient(pass_ops):
    ops = pass_ops
    taken = []
    _run_pass(lambda: taken.append(ops._take_lazy(_unapplied(ops, 1))))
    assert len(taken[0]) == 3 and _pass_is_empty(ops)
    held = []
    with pytest.raises(RuntimeError, match=r"1 un-applied gradient\(s\) \(deferred InstanceNorm-backward apply\) were not taken by the producing conv: gradients wrong$"):
        _run_pass(lambda: held.append(_unapplied(ops, 2)))
    assert _pass_is_empty(ops)


def test_pass_state_both_kinds_left_over_one_error(pass_ops):
    ops = pass_ops
    held = []

    def leave():
        ops._park_gradient(torch.zeros(2), torch.ones(2))
        held.extend([_unapplied(ops, 1), _unapplied(ops, 2)])

    with pytest.raises(RuntimeError, match=r"^2 un-applied gradient\(s\) .* were not taken by the producing conv: gradients wrong \(and 1 parked skip gradient\(s\) were never collected\)$"):
        _run_pass(leave)
    assert _pass_is_empty(ops)


def test_pass_state_dropped_after_a_pass_that_died(pass_ops):
    ops = pass_ops
    held, x0 = [], torch.zeros(2)

    def die():
        ops._park_gradient(x0, torch.ones(2))
        held.append(_unapplied(ops, 1))
        ops._PENDING["slots"][1] = ops._Slot(1, None, False)
        ops._PENDING["dead_biases"].add(2)
        ops._PENDING["up_jobs"][3] = {}
        raise ValueError("midway")

    with pytest.raises(ValueError, match="midway"):
        _run_pass(die)
    ops.drop_stale_wgrads()
    assert _pass_is_empty(ops) and ops.pending_wgrads() == 0
    e0 = ops._PENDING["epoch"]
    _run_pass(lambda: (ops._park_gradient(x0, torch.ones(2)), ops._collect_gradient(x0)))       # the next pass works
    assert _pass_is_empty(ops) and ops._PENDING["epoch"] == e0 + 1


def test_queued_second_phase_survives_drop_stale(pass_ops):
    """descriptors queued with no callback pending are the caller's second phase (set_wgrad_split), not leftovers of a pass that died"""
    ops = pass_ops
    entry = (ops.WgradDesc(), False, 0.0, 0.0, 0)
    ops._GROUP["descs"].append(entry)
    ops._PENDING["slots"][1] = ops._Slot(1, None, False)
    ops.drop_stale_wgrads()
    assert ops.pending_wgrads() == 1 and ops._GROUP["descs"][0] is entry and 1 in ops._PENDING["slots"]
    ops._PENDING["queued"] = True                                  # the same queue behind a pass that died: stale
    ops.drop_stale_wgrads()
    assert ops.pending_wgrads() == 0 and _pass_is_empty(ops)


def test_use_epoch_and_use_counts(pass_ops):
    """the use epoch advances once per pass; a weight counted once in a forward is "not once" after a second forward, and once again in the next epoch"""
    ops = pass_ops
    e0, w = ops._PENDING["epoch"], torch.ones(1)
    ops._count_use(w)
    assert w._vs_use == [e0, 1]
    ops._count_use(w)
    assert w._vs_use != [e0, 1] and w._vs_use == [e0, 2]
    x0 = torch.zeros(2)
    for k in (1, 2):
        _run_pass(lambda: (ops._PENDING.join(), ops._park_gradient(x0, torch.ones(2)), ops._PENDING.join(), ops._collect_gradient(x0)))
        assert ops._PENDING["epoch"] == e0 + k
    ops._count_use(w)
    assert w._vs_use == [e0 + 2, 1]
