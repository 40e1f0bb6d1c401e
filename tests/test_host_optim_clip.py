"""Host: the numpy oracle of the clipped / Nesterov SGD step (tests/optim_util.py) pinned against torch.nn.utils.clip_grad_norm_ + torch.optim.SGD on the
CPU, the clip coefficient's NaN / inf rule, and optim.poly_lr."""
import numpy as np
import pytest
import torch

from tests import optim_util as OU

SHAPES = [(1,), (2,), (4097,), (3, 4100), (16, 8, 2, 2, 2)]


def _tensors(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) * scale for s in SHAPES]


@pytest.mark.parametrize("momentum,wd,nesterov", [(0.99, 3e-5, True), (0.9, 0.0, True), (0.9, 3e-5, False), (0.0, 1e-3, False)])
def test_oracle_matches_torch_clip_grad_norm_and_sgd(momentum, wd, nesterov):
    """three steps; max_norm is half the first step's norm (that step clips) and the third step's gradients are small enough not to be clipped"""
    lr = 1e-2
    ref = [torch.nn.Parameter(t.clone()) for t in _tensors(1)]
    o_ref = torch.optim.SGD(ref, lr=lr, momentum=momentum, weight_decay=wd, nesterov=nesterov)
    ps = [t.numpy().copy() for t in _tensors(1)]
    ms = [np.zeros_like(p) for p in ps]
    max_norm = 0.5 * OU.global_norm([t.numpy() for t in _tensors(20, 0.1)])
    coefs = []
    for step in range(3):
        grads = _tensors(20 + step, 0.1 if step < 2 else 0.01)
        for p, g in zip(ref, grads):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(ref, max_norm)
        o_ref.step()
        coef = OU.clip_coef(np.float32(OU.global_norm([g.numpy() for g in grads])), max_norm)
        coefs.append(float(coef))
        for i, g in enumerate(grads):
            ps[i], ms[i] = OU.sgd_step(ps[i], g.numpy(), ms[i], lr, momentum, wd, nesterov, coef)
    assert coefs[0] < 0.51 and coefs[2] == 1.0                       # one step clips, one does not
    for p, q in zip(ref, ps):
        assert float(np.abs(q - p.detach().numpy()).max()) <= 1e-6 * float(p.detach().abs().max()) + 1e-7


def test_clip_coef_nan_gives_one_and_inf_gives_zero():
    assert OU.clip_coef(np.float32("nan"), 12.0) == np.float32(1.0)
    assert OU.clip_coef(np.float32("inf"), 12.0) == np.float32(0.0)
    assert OU.clip_coef(np.float32(24.0), 12.0) == np.float32(12.0) / (np.float32(24.0) + np.float32(1e-6))
    assert OU.clip_coef(np.float32(3.0), 12.0) == np.float32(1.0)
    assert OU.clip_coef(np.float32(1.0), 1e30) == np.float32(1.0)


def test_poly_lr_closed_form_and_monotone():
    from vae_segmentation_amd import optim
    assert optim.poly_lr(1e-2, 0, 1000) == 1e-2
    assert optim.poly_lr(3e-4, 0, 7, power=2.0) == 3e-4
    for epoch, n, power in [(1, 4, 0.9), (250, 1000, 0.9), (999, 1000, 0.9), (3, 10, 2.0)]:
        assert optim.poly_lr(1e-2, epoch, n, power) == 1e-2 * (1 - epoch / n) ** power
    lrs = [optim.poly_lr(1e-2, e, 50) for e in range(50)]
    assert all(a > b for a, b in zip(lrs, lrs[1:])) and lrs[-1] > 0
    with pytest.raises(ValueError):
        optim.poly_lr(1e-2, 50, 50)


def test_optimisers_take_torch_s_keys_and_reject_what_torch_rejects():
    """nesterov is a param-group key (torch's), max_norm an attribute of the optimiser (the norm spans groups); a checkpoint written before the key
    existed loads and means no Nesterov momentum"""
    from vae_segmentation_amd import optim
    ps = [torch.nn.Parameter(torch.zeros(3))]
    o = optim.SGD(ps, lr=1e-2, momentum=0.99, weight_decay=3e-5, nesterov=True, max_norm=12.0)
    assert o.param_groups[0]["nesterov"] is True and o.max_norm == 12.0 and "max_norm" not in o.param_groups[0]
    assert o.grad_norm is None                                       # no clipped step yet
    t = torch.optim.SGD(ps, lr=1e-2, momentum=0.99, weight_decay=3e-5, nesterov=True)
    t.load_state_dict(o.state_dict())                                # interchangeable both ways
    o.load_state_dict(t.state_dict())
    old = o.state_dict()
    for grp in old["param_groups"]:
        del grp["nesterov"]
    plain = optim.SGD(ps, lr=1e-2, momentum=0.9)
    plain.load_state_dict(old)
    assert plain.hyper()[0][3] == 0.0 and not plain._ext()
    assert optim.SGD(ps, lr=1e-2, momentum=0.9).hyper()[0] == (1e-2, 0.9, 0.0, 0.0)
    with pytest.raises(ValueError):
        optim.SGD(ps, lr=1e-2, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError):
        optim.Adam(ps, max_norm=0.0)
    assert optim.Adam(ps, max_norm=3.0).max_norm == 3.0


def test_chunk_size_has_one_source_and_the_block_map_follows_it():
    """VS_MT_CHUNK of include/vaeseg.h is what the library reports and what optim._Tables cuts tensors by: one entry {tensor, first element} per chunk,
    a tensor of exactly one chunk has one entry and one element more starts a second"""
    import re
    from vae_segmentation_amd import _lib, optim
    header = int(re.search(r"^#define\s+VS_MT_CHUNK\s+(\d+)\s*$", open(_lib.HEADER).read(), re.M).group(1))
    assert _lib.lib.vs_mt_chunk() == 4096 == header == optim._CHUNK
    a, b, c = torch.zeros(1), torch.zeros(4096), torch.zeros(4097)
    (ptrs, sizes, bm), nb = optim._Tables().get([[a, b, c]], "cpu")
    assert nb == 4 and bm.dtype == torch.int32 and bm.view(-1, 2).tolist() == [[0, 0], [1, 0], [2, 0], [2, 4096]]
    assert sizes.tolist() == [1, 4096, 4097] and ptrs.tolist() == [t.data_ptr() for t in (a, b, c)]


def test_entry_points_parse_the_optimiser_flags():
    import main_source
    import main_target
    a = main_source.parse(["r"])
    assert (a.momentum, a.weight_decay, a.nesterov, a.grad_clip, a.lr_schedule, a.poly_power) == (0.9, 0.0, False, 0.0, "constant", 0.9)
    for mod in (main_source, main_target):
        a = mod.parse(["r", "--nesterov", "--momentum", "0.99", "--weight_decay", "3e-5", "--grad_clip", "12", "--lr_schedule", "poly", "--poly_power", "0.8"])
        assert (a.momentum, a.weight_decay, a.nesterov, a.grad_clip, a.lr_schedule, a.poly_power) == (0.99, 3e-5, True, 12.0, "poly", 0.8)
        with pytest.raises(SystemExit):
            mod.parse(["r", "--nesterov", "--adam"])
        with pytest.raises(SystemExit):
            mod.parse(["r", "--nesterov", "--momentum", "0"])
