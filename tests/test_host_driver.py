"""Host: the parts of vae_segmentation_amd/driver.py that need no device — the table of the flags only main_target.py declares, the key of the
captured step, and run()'s flag checks ahead of the GPU check."""
import itertools

import pytest


def _raw(mod, argv, monkeypatch):
    """the namespace of the entry point's own parser: parse() without what driver.check_aug_flags adds to it"""
    from vae_segmentation_amd import driver
    with monkeypatch.context() as m:
        m.setattr(driver, "check_aug_flags", lambda parser, a, **kw: a)
        return mod.parse(argv)


def test_flag_table_matches_the_parsers(monkeypatch):
    import main_source
    import main_target
    from vae_segmentation_amd import driver
    table = driver.TARGET_ONLY_DEFAULTS
    source, target = vars(_raw(main_source, ["x"], monkeypatch)), vars(_raw(main_target, ["x"], monkeypatch))
    assert table and not set(table) & set(source) and set(table) <= set(target)
    for name, default in table.items():
        assert target[name] == default and type(target[name]) is type(default), name
    # every flag of main_target.py alone that driver.py reads is in the table: what is left out drives nothing here (check_target_flags reports it)
    assert set(target) - set(source) - set(table) == {"analysis_figure_name", "generate_bounding_boxes"}
    a = main_source.parse(["x"])
    assert all(getattr(a, name) == default for name, default in table.items())
    a = main_target.parse(["x", "-M", "domain_adaptation", "--seg_dropout", "0.1"])
    assert a.seg_dropout == 0.1 and all(getattr(a, name) == default for name, default in table.items() if name != "seg_dropout")


def _expected_key(method, epoch, warmup, turn_epoch, loss_type, only_pseudo):
    if method == "embed_train":
        return epoch % 2
    if method == "domain_adaptation_dis":
        return min(epoch, warmup)
    if method == "domain_adaptation" and loss_type == 0 and not only_pseudo:
        return (epoch // turn_epoch) % 2 if turn_epoch != -1 else min(epoch, warmup)
    return 0


def test_loss_key_follows_the_epoch_only_where_the_loss_does():
    import main_source
    import main_target
    from vae_segmentation_amd import driver
    source = ("vae_train", "seg_train", "joint_train", "sep_joint_train", "embed_train", "refine_vae")
    for method, warmup, turn_epoch in itertools.product(source + ("domain_adaptation", "domain_adaptation_dis", "discriminator_train"), (0, 3), (-1, 2)):
        common = ["x", "-M", method, "--lambda_vae_warmup", str(warmup), "--turn_epoch", str(turn_epoch)]
        variants = [[]] if method != "domain_adaptation" else [[], ["--only_pseudo"], ["--domain_loss_type", "8"]]
        for extra in variants:
            a = (main_source if method in source else main_target).parse(common + extra)
            keys = [driver.loss_key(a, method, epoch) for epoch in range(6)]
            assert keys == [_expected_key(method, epoch, warmup, turn_epoch, a.domain_loss_type, a.only_pseudo) for epoch in range(6)], (method, extra)
    a = main_target.parse(["x", "-M", "domain_adaptation", "--turn_epoch", "2"])                 # the table, written out where it is not constant
    assert [driver.loss_key(a, "domain_adaptation", e) for e in range(6)] == [0, 0, 1, 1, 0, 0]
    a = main_target.parse(["x", "-M", "domain_adaptation_dis", "--lambda_vae_warmup", "3"])
    assert [driver.loss_key(a, "domain_adaptation_dis", e) for e in range(6)] == [0, 1, 2, 3, 3, 3]
    assert [driver.loss_key(main_source.parse(["x"]), "embed_train", e) for e in range(6)] == [0, 1, 0, 1, 0, 1]


@pytest.mark.parametrize("flags, message", [
    (["--val_fine_whole"], "--val_fine_whole"),                                           # check_fine_whole_flags
    (["--val_tta", "w"], "--val_tta"),                                                    # check_whole_volume_flags
    (["-M", "discriminator_train", "--val_lesion"], "--val_lesion"),                      # check_lesion_flags
    (["--val_intensity", "100000"], "--val_intensity"),                                   # check_intensity_flags
])
def test_run_refuses_inconsistent_flags_before_it_asks_for_a_device(flags, message):
    import main_source
    import main_target
    from vae_segmentation_amd import driver
    for mod, side in ((main_source, "source"), (main_target, "target")):
        with pytest.raises(SystemExit, match="main_%s.py: inconsistent flags.*%s" % (side, message)):
            driver.run(mod.parse(["x", "-M", "seg_train"] + flags), side=side)
