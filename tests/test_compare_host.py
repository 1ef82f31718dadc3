"""The mask agreement without a GPU (csrc/gsa_compare.h; mask_ops.compare / apply_filters / check_filters; metrics.MaskAgreement;
SegSolver.evaluate_masks; the EVAL_MASK_CHAINS and EVAL_BAND keys).

``rule_compare`` is the rule of the header restated in numpy, with the distances of ``tests.test_boundary_host.rule_boundary``; it is
what tests/test_gpu_compare.py holds every word of every row to.  The hand cases below pin the rule and the metric definitions."""
import numpy as np
import pytest

from gan_segmentation_amd.metrics import MaskAgreement, SegmentationMetric
from tests.test_boundary_host import rule_boundary
from tests.test_downscale_host import _ModelLoaded, _config, no_models  # noqa: F401  (no_models is a fixture)

SLOTS, BANDS, ROW = 9, 4, 324
VALS = np.array([0, 1, 2, 3, 4, 5, 6, 7, 255], np.uint8)
ALL_BINS_RADII = (1, 2, 5)


# -- the rule ------------------------------------------------------------------------------------------------------------------
def rule_compare(target, pred, R, dist2=None):
    """target, pred (H, W) or (n, H, W) u8 -> (n, 324) int64: word f * 81 + min(target, 8) * 9 + min(pred, 8) counts the pixels with
    f = (target_dist2 <= R*R) + 2 * (pred_dist2 <= R*R), and f = 0 everywhere for R = 0.  ``dist2``: the two int16 planes to read in
    place of ``rule_boundary``'s (any numbers)."""
    target, pred = np.asarray(target), np.asarray(pred)
    assert target.dtype == pred.dtype == np.uint8 and target.shape == pred.shape and target.ndim in (2, 3) and 0 <= R <= 32
    if target.ndim == 2:
        target, pred = target[None], pred[None]
        dist2 = None if dist2 is None else (np.asarray(dist2[0])[None], np.asarray(dist2[1])[None])
    n = target.shape[0]
    f = np.zeros(target.shape, np.int64)
    if R:
        dt, dp = (rule_boundary(target, R), rule_boundary(pred, R)) if dist2 is None else dist2
        assert dt.dtype == dp.dtype == np.int16 and dt.shape == dp.shape == target.shape
        f = (dt.astype(np.int64) <= R * R) + 2 * (dp.astype(np.int64) <= R * R)
    bins = f * 81 + np.minimum(target, 8).astype(np.int64) * 9 + np.minimum(pred, 8)
    rows = np.zeros((n, ROW), np.int64)
    for i in range(n):
        rows[i] = np.bincount(bins[i].reshape(-1), minlength=ROW)
    return rows


def all_bins_pair():
    """108 x 108: vertical stripes of the nine values, 12 wide, against horizontal ones shifted by 6: every (target, pred) pair meets
    in a 12 x 12 cell whose corners lie near both masks' boundaries, whose edge centres near one, and whose middle near none."""
    y, x = np.mgrid[:108, :108]
    return VALS[(x // 12) % 9], VALS[((y + 6) // 12) % 9]


def test_the_rule_on_a_4x4_case_by_hand():
    """Target: columns 0-1 hold 0, columns 2-3 hold 1, pixel (0, 0) holds 255.  Prediction: column 3 holds 1, the rest 0.  R = 1.
    Target band: columns 1 and 2, and (0, 0) with its two neighbours; prediction band: columns 2 and 3."""
    target = np.array([[255, 0, 1, 1], [0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 1, 1]], np.uint8)
    pred = np.array([[0, 0, 0, 1]] * 4, np.uint8)
    row = rule_compare(target, pred, 1)[0]
    want = {0 * 81 + 0 * 9 + 0: 2,          # (2, 0), (3, 0): in no band
            1 * 81 + 0 * 9 + 0: 5,          # column 1, and (1, 0) beside the 255
            1 * 81 + 8 * 9 + 0: 1,          # the 255 itself: slot 8
            3 * 81 + 1 * 9 + 0: 4,          # column 2: target 1, predicted 0, in both bands
            2 * 81 + 1 * 9 + 1: 4}          # column 3: in the prediction's band only
    assert {int(k): int(row[k]) for k in np.nonzero(row)[0]} == want
    flat = rule_compare(target, pred, 0)[0]
    assert {int(k): int(flat[k]) for k in np.nonzero(flat)[0]} == {0: 7, 72: 1, 9: 4, 10: 4} and flat[81:].sum() == 0


def test_the_dist2_planes_are_read_as_numbers():
    """Negative and zero distances are inside every band; 32767 is outside."""
    target, pred = np.zeros((1, 4), np.uint8), np.array([[0, 1, 2, 9]], np.uint8)
    dt, dp = np.array([[-5, 0, 4, 5]], np.int16), np.array([[32767, 4, 5, -32768]], np.int16)
    row = rule_compare(target, pred, 2, dist2=(dt, dp))[0]
    assert {int(k): int(row[k]) for k in np.nonzero(row)[0]} == {81 + 0: 1, 243 + 1: 1, 81 + 2: 1, 162 + 8: 1}


def test_the_108_pair_fills_all_324_bins():
    target, pred = all_bins_pair()
    assert target.shape == pred.shape == (108, 108) and set(np.unique(target)) == set(np.unique(pred)) == set(VALS.tolist())
    for R in ALL_BINS_RADII:
        row = rule_compare(target, pred, R)[0]
        assert int((row > 0).sum()) == ROW, "R = %d: %d bins are empty" % (R, int((row == 0).sum()))
        assert int(row.sum()) == 108 * 108
    flat = rule_compare(target, pred, 0)[0]
    assert int((flat > 0).sum()) == 81 and flat[81:].sum() == 0 and flat.sum() == 108 * 108


def test_batches_are_planes_of_their_own():
    a, b = np.zeros((1, 6, 7), np.uint8), np.ones((1, 6, 7), np.uint8)
    rows = rule_compare(np.concatenate([a, b]), np.concatenate([b, b]), 3)
    assert rows.shape == (2, ROW) and rows[0, 0 * 9 + 1] == 42 and rows[1, 1 * 9 + 1] == 42 and rows.sum() == 84


# -- the metric bookkeeping ------------------------------------------------------------------------------------------------------
def _tables(entries):
    t = np.zeros((BANDS, SLOTS, SLOTS), np.int64)
    for (f, target, pred), v in entries.items():
        t[f, target, pred] = v
    return t


HAND = {(0, 0, 0): 50, (0, 1, 1): 30, (0, 0, 1): 2, (0, 1, 0): 3,
        (1, 0, 0): 4, (1, 1, 0): 1,
        (2, 0, 1): 2, (2, 1, 1): 5,
        (3, 0, 0): 6, (3, 1, 1): 7, (3, 0, 1): 1, (3, 1, 0): 2,
        (0, 8, 0): 11, (1, 8, 1): 3, (2, 5, 1): 9,              # ignored: target >= nclass
        (3, 0, 8): 4, (3, 1, 8): 2, (0, 1, 3): 1}               # abstained: prediction >= nclass


@pytest.mark.parametrize("skip_bg", [True, False])
def test_mask_agreement_on_hand_built_rows(skip_bg):
    m = MaskAgreement(2, skip_bg=skip_bg)
    rows = _tables(HAND).reshape(ROW)
    m.update_rows(rows)
    names, values = m.get()
    assert names == ["accuracy", "mean-iou", "band-accuracy", "boundary-iou", "abstained"]
    got = dict(zip(names, values))
    ref = SegmentationMetric(2, skip_bg=skip_bg)
    ref.update_confusion(np.array([[60, 5], [6, 42]]))
    assert [got["accuracy"], got["mean-iou"]] == ref.get()[1]
    assert got["band-accuracy"] == 17 / 21                      # T[1] + T[3] = [[10, 1], [3, 7]]
    ious = [6 / 13, 7 / 18]                                     # gt 11, 10; pred 8, 15; inter 6, 7
    assert got["boundary-iou"] == pytest.approx(np.mean(ious[1:] if skip_bg else ious), rel=1e-15)
    assert got["abstained"] == 7 / 120
    assert m.get_name_value() == list(zip(names, values))
    # rows of any leading shape are summed, and updates accumulate
    m.update_rows(np.stack([rows, rows]).reshape(2, 1, ROW))
    assert np.array_equal(m.tables, 3 * _tables(HAND))
    assert m.get()[1][2:] == values[2:]
    m.reset()
    assert not m.tables.any()


@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_accuracy_and_mean_iou_equal_segmentation_metric_on_the_same_confusion(k):
    rng = np.random.default_rng(k)
    m, ref = MaskAgreement(k), SegmentationMetric(k)
    for _ in range(3):
        rows = rng.integers(0, 1000, (2, ROW))
        rows[:, rng.integers(0, ROW, 40)] = 0
        m.update_rows(rows)
        ref.update_confusion(rows.reshape(2, BANDS, SLOTS, SLOTS)[:, :, :k, :k].sum(axis=(0, 1)))
    assert m.get()[1][:2] == ref.get()[1]


def test_mask_agreement_empty_unions_and_nan():
    m = MaskAgreement(2)
    names, values = m.get()
    assert values[0] == 0.0 and all(np.isnan(v) for v in values[1:])           # nothing at all
    m.update_rows(_tables({(0, 0, 0): 5}).reshape(1, ROW))                      # no band, class 1 nowhere
    got = dict(m.get_name_value())
    assert got["accuracy"] == pytest.approx(1.0) and np.isnan(got["mean-iou"]) and np.isnan(got["band-accuracy"]) \
        and np.isnan(got["boundary-iou"]) and got["abstained"] == 0.0
    m.reset()
    m.update_rows(_tables({(3, 1, 1): 3}).reshape(ROW))                         # class 0 has no boundary pixel: dropped, then class 1 skipped
    got = dict(m.get_name_value())
    assert np.isnan(got["boundary-iou"]) and got["band-accuracy"] == 1.0
    assert dict(MaskAgreement(2, skip_bg=False).get_name_value())["accuracy"] == 0.0
    keep = MaskAgreement(2, skip_bg=False)
    keep.update_rows(_tables({(3, 1, 1): 3}).reshape(ROW))
    assert dict(keep.get_name_value())["boundary-iou"] == 1.0
    m.reset()
    m.update_rows(_tables({(0, 8, 1): 4, (1, 2, 0): 4}).reshape(ROW))           # every target ignored
    got = dict(m.get_name_value())
    assert got["accuracy"] == 0.0 and np.isnan(got["abstained"]) and np.isnan(got["band-accuracy"])


def test_mask_agreement_rejects():
    for bad in (0, 9, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="nclass"):
            MaskAgreement(bad)
    m = MaskAgreement(3)
    for bad in (np.zeros(323, np.int64), np.zeros((2, 81), np.int64), np.zeros(ROW, np.float64), 5):
        with pytest.raises(ValueError, match="rows"):
            m.update_rows(bad)
    doc = MaskAgreement.__doc__
    assert "Cheng" in doc and "Euclidean" in doc and "image edge makes no boundary" in doc


# -- the python surface ----------------------------------------------------------------------------------------------------------
def test_constants():
    from gan_segmentation_amd import mask_ops
    assert (mask_ops.COMPARE_ROW, mask_ops.COMPARE_SLOTS, mask_ops.COMPARE_BANDS) == (ROW, SLOTS, BANDS) == (324, 9, 4)
    assert (MaskAgreement.ROW, MaskAgreement.SLOTS, MaskAgreement.BANDS) == (ROW, SLOTS, BANDS)


BAD_FILTER_KEYWORDS = [("refine", -1), ("refine", 9), ("refine", 1.0), ("refine", True), ("refine_radius", 0), ("refine_radius", 6),
                       ("refine_sigma_space", 0), ("refine_sigma_colour", "wide"), ("morph", 1), ("morph", None), ("morph", "yes"),
                       ("min_area", -1), ("min_area", 2 ** 31), ("min_area", 2.0), ("connectivity", 6), ("fill", "nearest"), ("fill", 256),
                       ("ignore_band", 33), ("ignore_band", -1), ("ignore_band", True), ("ignore_label", 256), ("ignore_label", "x")]


@pytest.mark.parametrize("name,value", BAD_FILTER_KEYWORDS)
def test_apply_filters_refuses_bad_keywords_before_any_device_work(name, value):
    """No tensor is looked at before the keywords are: None stands in for both."""
    from gan_segmentation_amd import mask_ops
    with pytest.raises(ValueError, match=name):
        mask_ops.apply_filters(None, None, 3, **{name: value})
    with pytest.raises(ValueError, match=name):
        mask_ops.check_filters(**{name: value})


def test_check_filters_fills_in_the_defaults_and_knows_its_names():
    import inspect
    from gan_segmentation_amd import mask_ops
    full = mask_ops.check_filters()
    params = inspect.signature(mask_ops.apply_filters).parameters
    assert list(params)[:3] == ["img", "mask", "classes"] and list(params)[3:] == list(full) == list(mask_ops.FILTER_DEFAULTS)
    assert {k: p.default for k, p in params.items() if k in full} == full
    assert full == dict(refine=0, refine_radius=3, refine_sigma_space=2.0, refine_sigma_colour=32.0, morph=False, min_area=0,
                        connectivity=8, fill="neighbour", ignore_band=0, ignore_label=255)
    assert mask_ops.check_filters(morph=True, min_area=np.int64(30), fill=7) == dict(full, morph=True, min_area=30, fill=7)
    with pytest.raises(ValueError, match="mask_morph"):
        mask_ops.check_filters(mask_morph=True)
    with pytest.raises(ValueError, match="chain 'a'"):
        mask_ops.check_filters("chain 'a'", morph=1)
    for bad in (1, 9, 3.0, None, True):
        with pytest.raises(ValueError, match="classes"):
            mask_ops.apply_filters(None, None, bad)
    with pytest.raises(ValueError, match="mask"):
        mask_ops.apply_filters(None, None, 3)


def test_compare_checks_its_arguments_before_any_gpu_work():
    import torch
    from gan_segmentation_amd import mask_ops
    cpu = torch.zeros((4, 4), dtype=torch.uint8)
    for pred, target in ((cpu, cpu), (None, None), (np.zeros((4, 4), np.uint8), cpu)):
        with pytest.raises(ValueError):
            mask_ops.compare(pred, target)


def test_evaluate_masks_checks_the_chains_before_it_reads_a_sample(tmp_path):
    """Nothing of the solver is touched before the chains are checked: None stands in for it, and the directory does not exist."""
    from gan_segmentation_amd.seg_solver import SegSolver
    missing = str(tmp_path / "missing")
    for chains, match in (({"a": {"morph": 1}}, "morph"), ({"a": {}, "b": {"ignore_band": 40}}, "ignore_band"), ({"a": {"blur": 2}}, "blur"),
                          ({}, "chains"), (None, "chains"), ({"a": None}, "chain 'a'"), ({"a": [("morph", True)]}, "chain 'a'")):
        with pytest.raises(ValueError, match=match):
            SegSolver.evaluate_masks(None, missing, chains)
    for band in (-1, 33, 2.0, True, None):
        with pytest.raises(ValueError, match="band"):
            SegSolver.evaluate_masks(None, missing, {"raw": {}}, band=band)


# -- the CLI -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys,match", [(dict(EVAL_MASK_CHAINS=[]), "EVAL_MASK_CHAINS"), (dict(EVAL_MASK_CHAINS={}), "EVAL_MASK_CHAINS"),
                                        (dict(EVAL_MASK_CHAINS="morph"), "EVAL_MASK_CHAINS"), (dict(EVAL_MASK_CHAINS={"a": True}), "EVAL_MASK_CHAINS"),
                                        (dict(EVAL_MASK_CHAINS={"a": {"morph": "yes"}}), "morph"), (dict(EVAL_MASK_CHAINS={"a": {"MASK_MORPH": True}}), "MASK_MORPH"),
                                        (dict(EVAL_MASK_CHAINS={"a": {}, "b": {"refine": 9}}), "refine"), (dict(EVAL_BAND=33), "EVAL_BAND"),
                                        (dict(EVAL_BAND=-1), "EVAL_BAND"), (dict(EVAL_BAND=2.5), "EVAL_BAND"), (dict(EVAL_BAND=True), "EVAL_BAND"),
                                        (dict(EVAL_BAND="2"), "EVAL_BAND"), (dict(EVAL_MASK_CHAINS={"raw": {}}, EVAL_BAND=40), "EVAL_BAND")])
def test_cli_rejects_a_bad_key_before_loading_a_model(tmp_path, no_models, keys, match):
    from gan_segmentation_amd import main as cli
    with pytest.raises(ValueError, match=match):
        cli.main(["evaluate", "--config", _config(tmp_path, **keys)])


def test_cli_accepts_the_keys_and_their_defaults(tmp_path, no_models):
    from gan_segmentation_amd import main as cli
    for keys in ({}, {"EVAL_BAND": 0}, {"EVAL_BAND": 32}, {"EVAL_MASK_CHAINS": {"raw": {}}}, {"EVAL_MASK_CHAINS": {"raw": None, "morph": {"morph": True}}},
                 {"EVAL_MASK_CHAINS": {"all": {"refine": 2, "refine_radius": 4, "refine_sigma_space": 3, "refine_sigma_colour": 40.5, "morph": True,
                                               "min_area": 64, "connectivity": 4, "fill": 0, "ignore_band": 3, "ignore_label": 254}}, "EVAL_BAND": 5}):
        with pytest.raises(_ModelLoaded):
            cli.main(["evaluate", "--config", _config(tmp_path, **keys)])
    assert cli.check_eval_mask_chains(None) is None and cli.check_eval_band(2) == 2
    assert cli.check_eval_mask_chains({"raw": None}) == {"raw": cli.check_eval_mask_chains({"raw": {}})["raw"]}
    for key in ("EVAL_MASK_CHAINS", "EVAL_BAND"):
        assert key in cli.__doc__
