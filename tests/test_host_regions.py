"""Host-side checks of the region measurements (no GPU): the scipy / numpy restatement of tests/regions_util.py against hand-written answers,
argument validation in ops, evaluation and the C ABI, the entry points' --val_lesion flag and the published record fields."""
import ctypes

import numpy as np
import pytest
import torch

from tests import regions_util as RU


def test_two_cubes_measure_as_stated():
    mask, want = RU.two_cubes()
    lab, k = RU.ref_label(mask)
    assert k == 2
    props = RU.ref_region_props(lab, 4)
    for i, (count, box, centroid) in enumerate(want):
        assert props["count"][i] == count and tuple(props["bbox"][i]) == box and tuple(props["centroid"][i]) == centroid
        assert tuple(props["sums"][i]) == tuple(int(c * count) for c in centroid)
    # absent labels: count 0, mins (d, h, w), maxes -1, sums 0, centroid NaN
    assert props["count"][2:].tolist() == [0, 0] and props["bbox"][2:].tolist() == [[12, 10, 70, -1, -1, -1]] * 2
    assert not props["sums"][2:].any() and np.isnan(props["centroid"][2:]).all() and props["overflow"] == 0
    # a table of one row: the second cube and nothing else overflows
    one = RU.ref_region_props(lab, 1)
    assert one["count"].tolist() == [27] and one["overflow"] == 160
    assert RU.ref_region_props(np.where(lab == 1, -3, lab), 2)["overflow"] == 27


def test_three_class_table_and_scores():
    pred, gt, table = RU.three_class_pair()
    got, overflow = RU.ref_contingency(pred, gt, 2, 2)
    assert np.array_equal(got, table) and overflow == 0 and got.sum() == pred.size
    conf = RU.ref_confusion(pred, gt, 3)
    assert np.array_equal(conf["table"], table)
    assert conf["dice"].tolist() == [0.8, 0.75, 4 / 6] and conf["iou"].tolist() == [4 / 6, 3 / 5, 2 / 4]
    assert conf["sensitivity"].tolist() == [4 / 5, 3 / 5, 1.0] and conf["precision"].tolist() == [4 / 5, 1.0, 2 / 4]
    # classes out of range go to overflow only
    got, overflow = RU.ref_contingency(pred, gt, 1, 2)
    assert overflow == 4 and np.array_equal(got, table[:2]) and got.sum() == pred.size - 4
    # a class nobody has scores 1.0; one side only: 0.0
    conf = RU.ref_confusion(pred, gt, 4)
    assert [conf[k][3] for k in ("dice", "iou", "sensitivity", "precision")] == [1.0] * 4
    only = RU.ref_confusion(np.full((1, 2, 2), 1), np.zeros((1, 2, 2), int), 2)
    assert only["dice"].tolist() == [0.0, 0.0] and only["sensitivity"].tolist() == [0.0, 0.0] and only["precision"].tolist() == [0.0, 0.0]


def test_lesion_scene_counts_as_stated():
    pred, gt, want = RU.lesion_scene()
    assert RU.ref_label(pred)[1] == 5 and RU.ref_label(gt)[1] == 5
    for (min_overlap, min_size), (n_gt, n_pred, tp, fn, fp) in want.items():
        rec = RU.ref_lesion(pred, gt, min_overlap=min_overlap, min_size=min_size)
        assert tuple(rec[k] for k in ("n_gt", "n_pred", "tp", "fn", "fp")) == (n_gt, n_pred, tp, fn, fp), (min_overlap, min_size)
        assert rec["sensitivity"] == tp / n_gt and rec["precision"] == (n_pred - fp) / n_pred and rec["f1"] == 2 * tp / (2 * tp + fp + fn)
    assert tuple(RU.ref_lesion(pred, gt)) == RU.LESION_FIELDS
    # the bridge is ONE predicted component that detects two lesions; g3 is ONE detection by two components
    P, G = RU.ref_label(pred)[0], RU.ref_label(gt)[0]
    T = RU.ref_contingency(P, G, 5, 5)[0][1:, 1:]
    assert sorted((T > 0).sum(1).tolist()) == [0, 0, 1, 1, 2] and sorted((T > 0).sum(0).tolist()) == [0, 0, 1, 1, 2]


def test_empty_conventions():
    empty, one = np.zeros((3, 4, 5), bool), np.zeros((3, 4, 5), bool)
    one[1, 1, 1:3] = True
    both = RU.ref_lesion(empty, empty)
    assert (both["n_gt"], both["n_pred"], both["tp"], both["fn"], both["fp"]) == (0, 0, 0, 0, 0)
    assert (both["sensitivity"], both["precision"], both["f1"]) == (1.0, 1.0, 1.0)
    missed = RU.ref_lesion(empty, one)
    assert (missed["tp"], missed["fn"], missed["fp"]) == (0, 1, 0) and (missed["sensitivity"], missed["precision"], missed["f1"]) == (0.0, 0.0, 0.0)
    spurious = RU.ref_lesion(one, empty)
    assert (spurious["tp"], spurious["fn"], spurious["fp"]) == (0, 0, 1)
    assert (spurious["sensitivity"], spurious["precision"], spurious["f1"]) == (0.0, 0.0, 0.0)
    assert RU.ref_lesion(one, one, min_size=3)["n_gt"] == 0 and RU.ref_lesion(one, one, min_size=3)["f1"] == 1.0
    assert RU.ref_lesion(one, one, min_overlap=3)["tp"] == 0 and RU.ref_lesion(one, one, min_overlap=2)["tp"] == 1


def test_the_library_answers_bad_arguments_on_the_host():
    from vae_segmentation_amd._lib import lib
    EINVAL, ESHAPE, EALIGN = -1, -2, -5
    bufs = [ctypes.create_string_buffer(4096 + 16) for _ in range(4)]
    pa, pb, pt, po = ((ctypes.addressof(x) + 15) & ~15 for x in bufs)
    ok = (1, 1, 2, 3, 4)

    def props(labels=pa, shape=ok, rows=4, table=pt, overflow=po):
        return lib.vs_region_props(labels, *shape, rows, table, overflow, None)

    def cont(a=pa, b=pb, shape=ok, ra=2, rb=2, table=pt, overflow=po):
        return lib.vs_contingency(a, b, *shape, ra, rb, table, overflow, None)

    for kw in ({"labels": None}, {"table": None}, {"overflow": None}, {"rows": 0}, {"rows": -5}):
        assert props(**kw) == EINVAL, kw
    for kw in ({"a": None}, {"b": None}, {"table": None}, {"overflow": None}, {"ra": -1}, {"rb": -1}):
        assert cont(**kw) == EINVAL, kw
    for shape in ((1, 1, 0, 3, 4), (0, 1, 2, 3, 4), (1, 1, 2048, 2048, 512)):
        assert props(shape=shape) == ESHAPE and cont(shape=shape) == ESHAPE, shape
    # (rows_a + 1) * (rows_b + 1) <= 2^22 per plane; 2048 * 2048 is the last table that fits (that call is not made here: it would launch)
    assert cont(ra=2047, rb=2048) == ESHAPE and cont(ra=2 ** 22, rb=0) == ESHAPE and cont(ra=2 ** 31 - 2, rb=2 ** 31 - 2) == ESHAPE
    assert props(table=pt + 4) == EALIGN and cont(table=pt + 4) == EALIGN and props(labels=pa + 2) == EALIGN and cont(b=pb + 1) == EALIGN


def test_wrappers_raise_before_the_device_check():
    from vae_segmentation_amd import evaluation, ops
    lab = torch.zeros(1, 1, 4, 5, 6, dtype=torch.int32)
    with pytest.raises(TypeError, match="int32"):
        ops.region_props(lab.long())
    with pytest.raises(TypeError, match="int32"):
        ops.contingency(lab, lab.float(), 2, 2)
    with pytest.raises(ValueError, match="shape"):
        ops.region_props(lab[0])
    with pytest.raises(ValueError, match="contiguous"):
        ops.region_props(lab.transpose(3, 4))
    with pytest.raises(ValueError, match="contiguous"):
        ops.contingency(lab, torch.zeros(1, 1, 4, 6, 5, dtype=torch.int32).transpose(3, 4), 2, 2)
    with pytest.raises(ValueError, match="empty"):
        ops.region_props(lab[:, :, :0])
    for bad in (0, -1, 1.5, True, None, 2 ** 31):
        with pytest.raises(ValueError, match="max_components"):
            ops.region_props(lab, max_components=bad)
    for ra, rb in ((-1, 2), (2, -1), (2.0, 2), (True, 2)):
        with pytest.raises(ValueError, match="rows_"):
            ops.contingency(lab, lab, ra, rb)
    with pytest.raises(ValueError, match="2\\^22"):
        ops.contingency(lab, lab, 2047, 2048)
    with pytest.raises(ValueError, match="differ in shape"):
        ops.contingency(lab, torch.zeros(1, 1, 4, 5, 7, dtype=torch.int32), 2, 2)
    # valid arguments get as far as the device check — 2048 x 2048 cells is within the bound
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.region_props(lab)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.contingency(lab, lab, 2047, 2047)

    x5, x3 = torch.zeros(1, 2, 4, 5, 6), torch.zeros(4, 5, 6)
    for x in (x5, x3):
        for kw in ({"spacing": (1, 2)}, {"spacing": (1, 0, 1)}, {"spacing": (1, float("inf"), 1)}, {"spacing": "abc"}, {"connectivity": 18},
                   {"max_components": 0}):
            with pytest.raises(ValueError):
                evaluation.region_props(x, **kw)
        for kw in ({"connectivity": 8}, {"min_overlap": 0}, {"min_size": -1}, {"max_components": 0}, {"min_overlap": 1.5}):
            with pytest.raises(ValueError):
                evaluation.lesion_metrics(x, x, **kw)
        with pytest.raises(RuntimeError, match="GPU only"):
            evaluation.region_props(x, spacing=(1.0, 0.5, 0.5))
        with pytest.raises(RuntimeError, match="GPU only"):
            evaluation.lesion_metrics(x, x, min_overlap=2, min_size=3)
        with pytest.raises(RuntimeError, match="GPU only"):
            evaluation.confusion(x.long(), x.long(), 3)
        with pytest.raises(ValueError, match="n_class"):
            evaluation.confusion(x.long(), x.long(), 0)
    with pytest.raises(ValueError, match="differ in shape"):
        evaluation.lesion_metrics(x3, torch.zeros(4, 5, 7))
    with pytest.raises(ValueError, match="differ in shape"):
        evaluation.confusion(x3.long(), torch.zeros(4, 5, 7).long(), 2)
    with pytest.raises(ValueError, match="shape"):
        evaluation.region_props(torch.zeros(4, 5))
    with pytest.raises(TypeError, match="bool"):
        evaluation.confusion(x3 > 0, x3.long(), 2)


def test_record_fields_are_what_the_docs_say():
    import os
    from vae_segmentation_amd import driver, evaluation, ops
    assert evaluation.LESION_RECORD_FIELDS == ("n_gt", "n_pred", "tp", "fn", "fp", "sensitivity", "precision", "f1", "overflow") == RU.LESION_FIELDS
    assert ops.REGION_COLUMNS == ("count", "zmin", "ymin", "xmin", "zmax", "ymax", "xmax", "sum_z", "sum_y", "sum_x")
    assert driver.LESION_LOG_FIELDS == evaluation.LESION_RECORD_FIELDS + ("dice", "iou", "class_sensitivity", "class_precision", "confusion_overflow")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    design, header = open(os.path.join(root, "DESIGN.md")).read(), open(os.path.join(root, "include", "vaeseg.h")).read()
    assert "`" + ", ".join(evaluation.LESION_RECORD_FIELDS) + "`" in design
    assert ", ".join(ops.REGION_COLUMNS) in header and ", ".join(ops.REGION_COLUMNS) in design
    host = evaluation.lesion_record_to_host({k: torch.tensor([[3, 0]]) for k in evaluation.LESION_RECORD_FIELDS if k != "overflow"} | {"overflow": torch.zeros(1, 2)})
    assert host["tp"] == [[3, 0]] and tuple(host) == evaluation.LESION_RECORD_FIELDS
    with pytest.raises(RuntimeError, match="beyond the table"):
        evaluation.lesion_record_to_host({k: torch.tensor([[1, 7]]) for k in evaluation.LESION_RECORD_FIELDS})


def test_val_lesion_flag():
    import main_source
    import main_target
    from vae_segmentation_amd import driver
    for mod, script, side in ((main_source, "main_source.py", "source"), (main_target, "main_target.py", "target")):
        a = mod.parse(["run", "-M", "seg_train"])
        assert a.val_lesion is False
        driver.check_lesion_flags(a, script)
        a = mod.parse(["run", "-M", "seg_train", "--val_lesion", "--val_min_component", "5", "--val_keep_largest", "2", "--val_closing", "1", "--val_fill_holes"])
        assert a.val_lesion is True and a.val_min_component == 5
        driver.check_lesion_flags(a, script)
        driver.check_lesion_flags(mod.parse(["run", "-M", "seg_train", "--val_min_component", "-1"]), script)       # without the flag nothing new is refused
        with pytest.raises(SystemExit, match="%s: inconsistent flags.*--val_lesion" % script):
            driver.check_lesion_flags(mod.parse(["run", "-M", "discriminator_train", "--val_lesion"]), script)
        with pytest.raises(SystemExit, match="%s: inconsistent flags.*--val_min_component" % script):
            driver.check_lesion_flags(mod.parse(["run", "-M", "seg_train", "--val_lesion", "--val_min_component", "-1"]), script)
        with pytest.raises(SystemExit, match="%s: inconsistent flags.*--val_lesion" % script):       # run() refuses before it touches a device
            driver.run(mod.parse(["run", "-M", "discriminator_train", "--val_lesion"]), side=side)
    with pytest.raises(SystemExit, match="main_target.py: inconsistent flags.*--val_finetune"):
        driver.check_lesion_flags(main_target.parse(["run", "-M", "domain_adaptation", "--val_lesion", "--val_finetune", "2"]), "main_target.py")
