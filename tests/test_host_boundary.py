"""The fp64 restatement of the signed distance maps and the boundary loss (tests/boundary_util.py) pinned on the host, before tests/test_gpu_boundary.py
compares the kernels with it; the weight schedule and the entry points' flag checks."""
import importlib

import numpy as np
import pytest

from tests import boundary_util as BU


def _volume(seed, shape, n_class, classless=True):
    rng = np.random.default_rng(seed)
    lab = BU.blocky_labels(rng, 1, n_class, shape, block=2)
    return (BU.sprinkle(rng, lab, n_class) if classless else lab)[0, 0]


@pytest.mark.parametrize("shape", [(5, 6, 7), (1, 1, 9), (3, 1, 4), (8, 2, 5)])
@pytest.mark.parametrize("n_class", [2, 4])
def test_oracle_equals_brute_force_at_unit_spacing(shape, n_class):
    """scipy's exact transform and a search over all pairs agree bit for bit: integer squares, one fp64 square root each"""
    for seed in range(3):
        lab = _volume(10 * n_class + seed, shape, n_class)
        a, b = BU.signed_distance(lab, n_class), BU.brute_force(lab, n_class)
        assert a.shape == (n_class,) + shape and a.dtype == np.float64
        assert (a == b).all()


def test_scipy_agrees_with_brute_force_bit_for_bit_on_5x6x7():
    from scipy.ndimage import distance_transform_edt as edt
    rng = np.random.default_rng(7)
    mask = rng.random((5, 6, 7)) < 0.6
    assert mask.any() and not mask.all()
    lab = mask.astype(np.float32)
    want = BU.brute_force(lab, 2, 1, 2)[0]                     # class 1 = mask
    assert (np.where(mask, -(edt(mask) - 1.0), edt(~mask)) == want).all()


def test_oracle_equals_kervadecs_expression():
    """one_hot2dist: edt(neg) * neg - (edt(pos) - 1) * pos, where neither set is empty"""
    from scipy.ndimage import distance_transform_edt as edt
    for spacing in (None, (2.5, 0.7, 1.3)):
        lab = _volume(3, (6, 7, 9), 3, classless=False)
        got = BU.signed_distance(lab, 3, spacing=spacing)
        for c in range(3):
            pos = lab == c
            assert pos.any() and not pos.all()
            neg = ~pos
            assert (got[c] == edt(neg, sampling=spacing) * neg - (edt(pos, sampling=spacing) - 1) * pos).all()


def test_sign_and_the_degenerate_planes():
    lab = _volume(5, (6, 8, 10), 4)
    _, cls = BU.classify(lab, 4)
    phi = BU.signed_distance(lab, 4)
    for c in range(4):
        inside = cls == c
        assert inside.any() and (phi[c][inside] <= 0).all() and (phi[c][~inside] > 0).all()
        assert phi[c][inside].max() == 0.0                     # a voxel with a neighbour outside the class is at distance 1: phi = 0
    # classless voxels are outside every class, and a class of the label that n_class leaves out belongs to none
    assert (phi[:, ~BU.classify(lab, 4)[0]] > 0).all()
    empty = BU.signed_distance(np.zeros((3, 4, 5), np.float32), 3)
    assert (empty == 0).all()                                  # class 0 fills the volume, 1 and 2 are absent
    nothing = BU.signed_distance(np.full((3, 4, 5), np.nan, np.float32), 2)
    assert (nothing == 0).all()
    assert (BU.signed_distance(lab, 4, 1, 3) == phi[1:3]).all()


def test_loss_and_gradient_restatement():
    rng = np.random.default_rng(11)
    p = rng.random((2, 3, 2, 3, 4))
    phi = rng.normal(size=(2, 2, 2, 3, 4)) * 3
    lab = rng.integers(0, 3, size=(2, 1, 2, 3, 4)).astype(np.float32)
    lab[0, 0, 0, 0, :2] = (-1.0, np.nan)
    lab[1] = 255.0                                              # sample 1 has no valid voxel: contributes 0
    term, weighted, grad = BU.boundary_loss(p, lab, phi, 1, 3, weight=0.25, gout=2.0)
    valid = BU.classify(lab[0, 0], 3)[0]
    want = (p[0, 1:3] * phi[0])[:, valid].sum() / valid.sum() / (2 * 2)
    assert abs(term - want) < 1e-15 and weighted == 0.25 * term
    assert (grad[1] == 0).all() and (grad[:, 0] == 0).all() and (grad[0, 1:3][:, ~valid] == 0).all()
    h = 1e-6                                                    # the loss is linear in p: a difference quotient is exact up to rounding
    q = p.copy()
    q[0, 2, 1, 2, 3] += h
    assert abs((BU.boundary_loss(q, lab, phi, 1, 3, weight=0.25)[1] - weighted) / h * 2.0 - grad[0, 2, 1, 2, 3]) < 1e-9


def test_boundary_weight_schedule():
    from vae_segmentation_amd import train as T
    assert T.boundary_weight(0, 0.01) == 0.01 and T.boundary_weight(7, 0.01) == 0.01
    assert T.boundary_weight(3, 0.01, 0.01) == 0.01 + 3 * 0.01
    assert T.boundary_weight(100, 0.01, 0.01, 0.5) == 0.5 and T.boundary_weight(2, 0.0, 0.25, 1.0) == 0.5
    assert T.boundary_weight(0, 0.0, 0.01) == 0.0 and T.boundary_weight(5, 2.0, 0.0, 1.0) == 1.0


def test_loss_functions_refuse_a_boundary_term_without_the_compound_loss():
    from vae_segmentation_amd import train as T
    for fn in (T.seg_train_losses, T.joint_train_losses):
        with pytest.raises(TypeError, match="loss="):
            fn(None, None, None, boundary={"weight": 0.1, "spacing": None})
        with pytest.raises(TypeError, match="boundary"):
            fn(None, None, None, loss={"ce_weight": 1.0}, boundary={"weigth": 0.1})
    with pytest.raises(TypeError, match="unknown"):             # it does not go inside `loss`, whose unknown-key check stays
        T._seg_loss_args({"ce_weight": 1.0, "boundary": 0.1})


def test_entry_point_flags():
    src, tgt = importlib.import_module("main_source"), importlib.import_module("main_target")
    from vae_segmentation_amd import driver
    a = src.parse(["run", "--method", "seg_train"])
    assert a.boundary_weight == 0.0 and a.boundary_ramp == 0.0 and a.boundary_max is None and not driver.boundary_enabled(a)
    a = src.parse(["run", "--method", "seg_train", "--seg_loss", "dice_ce", "--boundary_weight", "0.01", "--boundary_ramp", "0.02", "--boundary_max", "0.5"])
    assert (a.boundary_weight, a.boundary_ramp, a.boundary_max) == (0.01, 0.02, 0.5) and driver.boundary_enabled(a)
    a = src.parse(["run", "--method", "joint_train", "--seg_loss", "dice_ce", "--boundary_ramp", "0.01"])        # a ramp from 0 is a schedule too
    assert a.boundary_weight == 0.0 and driver.boundary_enabled(a)
    for bad in (["--method", "seg_train", "--boundary_weight", "0.01"],                                         # without --seg_loss dice_ce
                ["--method", "seg_train", "--seg_loss", "dice", "--boundary_weight", "0.01"],
                ["--method", "joint_train", "--boundary_ramp", "0.01"],
                ["--method", "vae_train", "--seg_loss", "dice_ce", "--boundary_weight", "0.01"],
                ["--method", "vae_train", "--boundary_weight", "0.01"],
                ["--method", "sep_joint_train", "--boundary_max", "1"],
                ["--method", "seg_train", "--seg_loss", "dice_ce", "--boundary_max", "1"],                    # a cap with nothing to cap
                ["--method", "seg_train", "--seg_loss", "dice_ce", "--boundary_weight", "-0.1"],
                ["--method", "seg_train", "--seg_loss", "dice_ce", "--boundary_ramp", "nan"]):
        with pytest.raises(SystemExit):
            src.parse(["run"] + bad)
    assert tgt.parse(["run", "--method", "joint_train"]).boundary_weight == 0.0
    for method in ("joint_train", "domain_adaptation"):
        with pytest.raises(SystemExit):
            tgt.parse(["run", "--method", method, "--boundary_weight", "0.01"])
