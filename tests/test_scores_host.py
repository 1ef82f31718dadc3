"""The score histograms without a device (csrc/gsa_scores.h): ``rule_scores``, the numpy restatement of the
header's rule that tests/test_gpu_scores.py holds the kernel to; ``metrics.ScoreCurves`` against brute force over expanded scores;
the EVAL_SCORES and EVAL_SCORE_SHIFT keys; ``SegSolver.evaluate_scores``' argument checks."""
import math

import numpy as np
import pytest

from gan_segmentation_amd.metrics import ScoreCurves
from tests.test_downscale_host import _ModelLoaded, _config, no_models  # noqa: F401  (no_models is a fixture)

BINS = 1024


# -- the rule ------------------------------------------------------------------------------------------------------------------
def rule_bins(logits, shift):
    """logits (n, K, HW) float32 -> (n, K, HW) int64, the bin of every class's margin.  float32 throughout: one subtraction, one
    exact scaling, ceil, then the clamp; NaN (a NaN logit among the pixel's, inf - inf) goes to bin 0."""
    z = np.asarray(logits)
    assert z.dtype == np.float32 and z.ndim == 3
    n, K, HW = z.shape
    bins = np.zeros((n, K, HW), np.int64)
    scale = np.float32(2 ** shift)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(K):
            others = np.delete(z, c, axis=1).max(axis=1)            # numpy's max hands a NaN on, as the rule does
            m = z[:, c] - others
            assert m.dtype == np.float32
            t = np.ceil(m * scale)
            assert t.dtype == np.float32
            b = np.where(np.isnan(t) | ~(t > np.float32(-511)), 0, np.where(t >= np.float32(512), BINS - 1, 0))
            mid = ~np.isnan(t) & (t > np.float32(-511)) & (t < np.float32(512))
            b[mid] = t[mid].astype(np.int64) + 511
            bins[:, c] = b
    return bins


def rule_scores(logits, labels, shift):
    """logits (n, K, HW) float32, labels (n, HW) integers -> rows (n, K, 2, 1024) int64 by the header's rule."""
    z, y = np.asarray(logits), np.asarray(labels).astype(np.int64)
    n, K, HW = z.shape
    assert y.shape == (n, HW)
    bins = rule_bins(z, shift)
    rows = np.zeros((n, K, 2, BINS), np.int64)
    valid = (y >= 0) & (y < K)
    for i in range(n):
        for c in range(K):
            own = (y[i] == c)[valid[i]]
            rows[i, c] = np.bincount(own.astype(np.int64) * BINS + bins[i, c][valid[i]], minlength=2 * BINS).reshape(2, BINS)
    return rows


def test_rule_bins_edges():
    """The half-open bins, the clamps and the specials, spelled out for shift 0 and 5 on two classes: z_1 = 0, z_0 = the margin."""
    def bins0(margins, shift):
        m = np.asarray(margins, np.float32)
        z = np.stack([m, np.zeros_like(m)])[None]
        return rule_bins(z, shift)[0, 0].tolist()
    tiny, inf, nan = np.float32(1e-45), np.float32(np.inf), np.float32(np.nan)
    assert tiny > 0 and tiny < np.finfo(np.float32).tiny, "a subnormal"
    assert bins0([0.0, -0.0, tiny, -tiny, 1.0, np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0))], 0) \
        == [511, 511, 512, 511, 512, 513, 512]
    assert bins0([512.0, 511.0, 511.5, 1e30, inf, -510.0, -510.5, -511.0, -512.0, -1e30, -inf, nan], 0) \
        == [1023, 1022, 1023, 1023, 1023, 1, 1, 0, 0, 0, 0, 0]
    assert bins0([1 / 32, 1 / 32 + 1e-6, 16.0, 16.0 - 1e-5, 16.01, -15.97, -16.0, 3e38], 5) == [512, 513, 1023, 1023, 1023, 0, 0, 1023]
    assert bins0([3e38], 8) == [1023], "the scaled margin overflows to +inf"
    z = np.array([[[inf, inf, -inf, nan, 1.0, inf], [inf, 1.0, -inf, 1.0, nan, -inf]]], np.float32)
    assert rule_bins(z, 5)[0].tolist() == [[0, 1023, 0, 0, 0, 1023], [0, 0, 0, 0, 0, 0]]
    # three classes: ties among two and among all, and one NaN makes every margin of the pixel NaN
    z = np.array([[[2.0, 1.0, nan], [2.0, 1.0, 5.0], [0.0, 1.0, 7.0]]], np.float32)
    assert rule_bins(z, 0)[0].tolist() == [[511, 511, 0], [511, 511, 0], [509, 511, 0]]


def test_rule_scores_counts_every_valid_pixel_once_a_class():
    rng = np.random.default_rng(0)
    z = (rng.standard_normal((2, 3, 500)) * 4).astype(np.float32)
    y = rng.integers(-2, 5, (2, 500))
    rows = rule_scores(z, y, 5)
    valid = ((y >= 0) & (y < 3)).sum(axis=1)
    assert np.array_equal(rows.sum(axis=(2, 3)), np.repeat(valid[:, None], 3, axis=1))
    assert np.array_equal(rows[:, :, 1].sum(axis=2), np.stack([(y == c).sum(axis=1) for c in range(3)], axis=1))
    # b >= 512 <=> the strict winner
    strict = np.stack([z[:, c] > np.delete(z, c, axis=1).max(axis=1) for c in range(3)], axis=1)
    assert np.array_equal(rule_bins(z, 5) >= 512, strict)


# -- ScoreCurves against brute force -------------------------------------------------------------------------------------------
def _random_hist(rng, nclass, occupied, top):
    h = np.zeros((nclass, 2, BINS), np.int64)
    for c in range(nclass):
        for r in range(2):
            where = rng.choice(BINS, size=occupied, replace=False)
            h[c, r, where] = rng.integers(1, top, occupied)
    return h


def _expand(h):
    """(scores of the negatives, scores of the positives): every pixel's bin."""
    return np.repeat(np.arange(BINS), h[0]), np.repeat(np.arange(BINS), h[1])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_auc_is_the_pair_count_with_ties_counted_half(seed):
    rng = np.random.default_rng(seed)
    h = _random_hist(rng, 3, 12, 6)
    h[1, :, :] = 0
    h[1, 0, [5, 9, 700]] = [3, 4, 2]            # ties inside a bin on purpose
    h[1, 1, [9, 700, 1023]] = [2, 5, 1]
    curves = ScoreCurves(3, skip_bg=False)
    curves.update_rows(h)
    for c in range(3):
        neg, pos = _expand(h[c])
        wins = sum(int((p > neg).sum()) for p in pos)
        ties = sum(int((p == neg).sum()) for p in pos)
        assert curves.roc_auc(c) == (2 * wins + ties) / (2 * len(pos) * len(neg))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_average_precision_is_the_direct_definition(seed):
    from fractions import Fraction
    rng = np.random.default_rng(10 + seed)
    h = _random_hist(rng, 2, 15, 9)
    curves = ScoreCurves(2, skip_bg=False)
    curves.update_rows(h)
    for c in range(2):
        neg, pos = _expand(h[c])
        ap, last_recall = Fraction(0), Fraction(0)
        for t in sorted(set(neg.tolist()) | set(pos.tolist()), reverse=True):       # every distinct score, descending
            tp, fp = int((pos >= t).sum()), int((neg >= t).sum())
            recall, precision = Fraction(tp, len(pos)), Fraction(tp, tp + fp)
            ap += (recall - last_recall) * precision
            last_recall = recall
        assert abs(curves.average_precision(c) - float(ap)) <= 4 * np.spacing(float(ap))


def test_curves_sum_leading_axes_and_big_counts_do_not_overflow():
    rng = np.random.default_rng(3)
    rows = rng.integers(0, 50, (4, 3, 2, 2, BINS))
    a, b = ScoreCurves(2), ScoreCurves(2)
    a.update_rows(rows)
    for r in rows.reshape(-1, 2, 2, BINS):
        b.update_rows(r)
    assert np.array_equal(a.hist, rows.sum(axis=(0, 1))) and np.array_equal(a.hist, b.hist)
    big = ScoreCurves(2, skip_bg=False)
    h = np.zeros((2, 2, BINS), np.int64)
    h[:, 0, 100], h[:, 1, 900], h[:, 0, 900] = 2 ** 40, 2 ** 40, 2 ** 39        # P * N = 2^80 * 1.5: Python integers
    big.update_rows(h)
    assert big.roc_auc(0) == (2 ** 40 * 2 ** 40 + 2 ** 40 * 2 ** 39 / 2) / (2 ** 40 * (2 ** 40 + 2 ** 39))
    for bad in (np.zeros((2, 2, 1023), np.int64), np.zeros((3, 2, BINS), np.int64), np.zeros((2, 2, BINS), np.float32), np.zeros(BINS, np.int64)):
        with pytest.raises(ValueError, match="rows"):
            a.update_rows(bad)
    for args in ((1,), (9,), (True,), (2.0,), (2, 9), (2, -1), (2, True)):
        with pytest.raises(ValueError):
            ScoreCurves(*args)


def test_degenerate_classes_are_nan_and_left_out_of_the_means():
    h = np.zeros((3, 2, BINS), np.int64)
    h[0, 0, 100] = 7                    # class 0: no positives
    h[1, 1, 600] = 7                    # class 1: no negatives
    h[2, 0, 100], h[2, 1, 600], h[2, 0, 600] = 3, 4, 1
    curves = ScoreCurves(3, skip_bg=False)
    curves.update_rows(h)
    for c in (0, 1):
        assert math.isnan(curves.roc_auc(c)) and math.isnan(curves.average_precision(c))
    auc2, ap2 = curves.roc_auc(2), curves.average_precision(2)
    assert auc2 == (4 * 3 + 4 * 1 / 2) / 16 and ap2 == 4 / 5
    values = dict(curves.get_name_value())
    assert values["mean-auc"] == auc2 and values["mean-ap"] == ap2
    assert values["100*(1-mean-auc)"] == 100 * (1 - auc2) and values["100*(1-mean-ap)"] == 100 * (1 - ap2)
    assert curves.best(0)["threshold"] is None and math.isnan(curves.best(0)["iou"])
    empty = ScoreCurves(2)
    values = dict(empty.get_name_value())
    assert all(math.isnan(values[k]) for k in ("mean-auc", "mean-ap", "clamped", "1-iou@0", "1-best-margin"))
    assert list(values) == ["mean-auc", "mean-ap", "100*(1-mean-auc)", "100*(1-mean-ap)", "1-best-margin", "1-iou@best", "1-iou@0", "clamped"]
    assert [k for k, _v in ScoreCurves(3, skip_bg=False).get_name_value()][4:7] == ["0-best-margin", "0-iou@best", "0-iou@0"]


def test_sweep_at_best_and_clamped():
    h = np.zeros((2, 2, BINS), np.int64)
    # class 1: negatives at bins 0, 500, 520; positives at 500, 520, 1023
    h[1, 0, [0, 500, 520]] = [10, 4, 2]
    h[1, 1, [500, 520, 1023]] = [1, 3, 6]
    curves = ScoreCurves(2, shift=5)
    curves.update_rows(h)
    tp, fp, fn = curves.sweep(1)
    assert tp.shape == fp.shape == fn.shape == (BINS + 1,) and tp.dtype == np.int64
    for t in (0, 1, 500, 501, 520, 521, 1023, 1024):
        assert (tp[t], fp[t], fn[t]) == (h[1, 1, t:].sum(), h[1, 0, t:].sum(), h[1, 1, :t].sum()), t
    at0 = curves.at(1, 0.0)
    assert (at0["threshold"], at0["margin"], at0["tp"], at0["fp"], at0["fn"]) == (512, 0.0, 9, 2, 1)
    assert at0["precision"] == 9 / 11 and at0["recall"] == 9 / 10 and at0["iou"] == 9 / 12 and at0["dice"] == 18 / 21
    assert curves.at(1, 0.26)["threshold"] == 520 and curves.at(1, 0.26)["margin"] == 0.25           # the nearest edge: 8 / 32
    assert curves.at(1, 1e9)["threshold"] == 1024 and curves.at(1, -1e9)["threshold"] == 0
    assert math.isnan(curves.at(1, 1e9)["precision"]) and curves.at(1, 1e9)["recall"] == 0.0
    # iou by threshold: t <= 0: 10/26; 1..500: 10/16; 501..520: 9/12 = 0.75; 521..1023: 6/10; 1024: 0 -- the lowest t of the best
    best = curves.best(1)
    assert (best["threshold"], best["iou"], best["margin"]) == (501, 0.75, -11 / 32)
    assert best["probability"] == 1.0 / (1.0 + math.exp(11 / 32))
    assert curves.best(1, "dice")["threshold"] == 501 and curves.best(1, "dice")["dice"] == 18 / 21
    assert "probability" not in ScoreCurves(3).best(1)
    assert curves.clamped(1) == 16 / 26 and math.isnan(curves.clamped(0))
    assert curves.margin_of(512) == 0.0 and ScoreCurves(2, shift=0).margin_of(1024) == 512.0
    for bad in (-1, 2, 1.0, True):
        with pytest.raises(ValueError, match="class"):
            curves.roc_auc(bad)
    with pytest.raises(ValueError, match="metric"):
        curves.best(1, "accuracy")


def test_ties_in_best_take_the_lowest_threshold():
    h = np.zeros((2, 2, BINS), np.int64)
    h[1, 1, 800], h[1, 0, 100] = 5, 5           # every t in 101..800 separates the two perfectly
    curves = ScoreCurves(2)
    curves.update_rows(h)
    assert curves.best(1)["threshold"] == 101 and curves.best(1)["iou"] == 1.0


@pytest.mark.parametrize("shift", [0, 5, 8])
def test_at_zero_is_the_argmax_confusion_for_two_classes(shift):
    """Class 1 of two: margin > 0 <=> z_1 > z_0 <=> the first-maximum argmax is 1, ties included."""
    rng = np.random.default_rng(shift)
    z = np.round(rng.standard_normal((3, 2, 2000)) * 2, 1).astype(np.float32)          # one decimal: plenty of ties
    y = rng.integers(-1, 2, (3, 2000))
    assert (z[:, 0] == z[:, 1]).sum() > 20
    curves = ScoreCurves(2, shift=shift)
    curves.update_rows(rule_scores(z, y, shift))
    pred, ok = np.argmax(z, axis=1), y >= 0
    conf = np.zeros((2, 2), np.int64)
    np.add.at(conf, (y[ok], pred[ok]), 1)
    at0 = curves.at(1, 0)
    assert (at0["tp"], at0["fp"], at0["fn"]) == (conf[1, 1], conf[0, 1], conf[1, 0])
    assert at0["iou"] == conf[1, 1] / (conf[1, 1] + conf[0, 1] + conf[1, 0])


# -- arguments and config keys -------------------------------------------------------------------------------------------------
def test_evaluate_scores_checks_its_arguments_before_it_reads_a_sample(tmp_path):
    """Nothing of the solver is touched before the arguments are checked: None stands in for it, and the directory does not exist."""
    from gan_segmentation_amd.seg_solver import SegSolver
    missing = str(tmp_path / "missing")
    for shift in (-1, 9, 5.0, True, None, "5"):
        with pytest.raises(ValueError, match="shift"):
            SegSolver.evaluate_scores(None, missing, shift=shift)
    for path in (None, 3):
        with pytest.raises(ValueError, match="input_dir"):
            SegSolver.evaluate_scores(None, path)


def test_score_ops_constants_and_shift_check():
    from gan_segmentation_amd import score_ops
    assert score_ops.SCORE_BINS == BINS == ScoreCurves.BINS and score_ops.SCORE_MAX_SHIFT == 8 and score_ops.DEFAULT_SHIFT == 5
    assert [score_ops.check_shift(v) for v in (0, 5, 8, np.int64(3))] == [0, 5, 8, 3]
    for bad in (-1, 9, 1.0, True, None):
        with pytest.raises(ValueError, match="shift"):
            score_ops.check_shift(bad)


@pytest.mark.parametrize("keys,match", [(dict(EVAL_SCORES=1), "EVAL_SCORES"), (dict(EVAL_SCORES="yes"), "EVAL_SCORES"),
                                        (dict(EVAL_SCORES=None), "EVAL_SCORES"), (dict(EVAL_SCORE_SHIFT=9), "EVAL_SCORE_SHIFT"),
                                        (dict(EVAL_SCORE_SHIFT=-1), "EVAL_SCORE_SHIFT"), (dict(EVAL_SCORE_SHIFT=5.0), "EVAL_SCORE_SHIFT"),
                                        (dict(EVAL_SCORE_SHIFT=True), "EVAL_SCORE_SHIFT"), (dict(EVAL_SCORE_SHIFT="5"), "EVAL_SCORE_SHIFT"),
                                        (dict(EVAL_SCORES=True, EVAL_SCORE_SHIFT=12), "EVAL_SCORE_SHIFT"),
                                        (dict(EVAL_SCORES=False, EVAL_SCORE_SHIFT=12), "EVAL_SCORE_SHIFT")])
def test_cli_rejects_a_bad_key_before_loading_a_model(tmp_path, no_models, keys, match):
    from gan_segmentation_amd import main as cli
    with pytest.raises(ValueError, match=match):
        cli.main(["evaluate", "--config", _config(tmp_path, **keys)])


def test_cli_accepts_the_keys_and_their_defaults(tmp_path, no_models):
    from gan_segmentation_amd import main as cli
    for keys in ({}, {"EVAL_SCORES": True}, {"EVAL_SCORES": False}, {"EVAL_SCORE_SHIFT": 0}, {"EVAL_SCORES": True, "EVAL_SCORE_SHIFT": 8}):
        with pytest.raises(_ModelLoaded):
            cli.main(["evaluate", "--config", _config(tmp_path, **keys)])
    assert cli.check_eval_scores(False) is False and cli.check_eval_score_shift(5) == 5
    for key in ("EVAL_SCORES", "EVAL_SCORE_SHIFT"):
        assert key in cli.__doc__
