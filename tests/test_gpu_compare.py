"""The mask agreement on the GPU (csrc/gsa_compare.h gsa_mask_compare; mask_ops.compare / apply_filters; SegSolver.evaluate_masks):
bit for bit the rule of tests/test_compare_host.py, every word of every row."""
import os

import numpy as np
import pytest

from tests.test_boundary_host import class_blobs, rule_boundary
from tests.test_compare_host import ALL_BINS_RADII, ROW, all_bins_pair, rule_compare

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The tile of csrc/gsa_compare.hip: the seam shapes below are chosen for it (asserted against the source text).
TILE_W, TILE_H, PIX, WAVE_ROWS = 256, 32, 4, 8


def _bin(word):
    f, code = divmod(int(word), 81)
    return "band %d target %d pred %d" % ((f,) + divmod(code, 9))


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.int64, what
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d of %d words differ from the rule, first in sample %d at %s: got %d, rule %d" % (
        what, len(bad), want.size, bad[0][0], _bin(bad[0][1]), got[tuple(bad[0])], want[tuple(bad[0])])


def _shifted(torch, a, off):
    """``a`` on the device as a view ``off`` ELEMENTS into a larger buffer."""
    t = torch.from_numpy(a)
    buf = torch.zeros(off + a.size + 8, dtype=t.dtype, device="cuda")
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(t)
    return v


def _entry(torch, target, pred, R, dist2=None, offsets=(0, 0, 0, 0), fill=None):
    """gsa_mask_compare itself on (n, H, W) numpy masks: dist2 planes from the rule (or the given pair), every input ``offsets``
    elements into its buffer -> rows (n, 324) on the host.  The inputs are checked to be unwritten."""
    from gan_segmentation_amd._runtime import launch
    n, H, W = target.shape
    dt = dp = None
    if R:
        dt, dp = (rule_boundary(target, R), rule_boundary(pred, R)) if dist2 is None else dist2
    arrays = [target, pred] + ([dt, dp] if R else [])
    dev = [_shifted(torch, a, off) for a, off in zip(arrays, offsets)]
    rows = torch.full((n, ROW), -7 if fill is None else fill, dtype=torch.int64, device="cuda")
    launch("gsa_mask_compare", rows.device, n, H, W, R, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr() if R else None,
           dev[3].data_ptr() if R else None, rows.data_ptr())
    got = rows.cpu().numpy()
    for a, d in zip(arrays, dev):
        assert np.array_equal(d.cpu().numpy(), a), "an input was written to"
    return got


def _pair(seed, shape, classes=3, with255=True):
    """Two class-blob masks of one shape that differ along their boundaries; 255 present in both with ``with255``."""
    return class_blobs(seed, shape, classes, sigma=2.0, with255=with255), class_blobs(seed + 1000, shape, classes, sigma=2.5, with255=with255)


def _check(torch, target, pred, R, what, **kw):
    want = rule_compare(target, pred, R)
    assert (want.sum(axis=1) == target.shape[1] * target.shape[2]).all()
    got = _entry(torch, target, pred, R, **kw)
    _same(got, want, "%s %s R=%d" % (what, target.shape, R))
    return got


# ---- the tile --------------------------------------------------------------------------------------------------------------------
def test_the_tile_is_the_one_these_tests_assume():
    src = open(os.path.join(ROOT, "gan-segmentation_amd", "csrc", "gsa_compare.hip")).read()
    for line in ("constexpr int kTileW = %d;" % TILE_W, "constexpr int kTileH = %d;" % TILE_H, "constexpr int kPix = %d;" % PIX,
                 "constexpr int kWaveRows = %d;" % WAVE_ROWS, "constexpr int kThreads = 256;"):
        assert line in src, line
    assert "const unsigned blocks = (unsigned)(planes * tiles_per_plane);" in src       # one workgroup per tile: no grid cap to cross


SMALL = [(1, 1), (1, 5), (7, 1), (3, 4), (2, 8)]
SEAMS = [(TILE_H - 1, TILE_W - 1), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1), (TILE_H + 1, TILE_W - 4), (WAVE_ROWS + 1, TILE_W + 4),
         (WAVE_ROWS - 1, 2 * TILE_W)]


@pytest.mark.parametrize("H,W", SMALL + SEAMS)
def test_small_shapes_and_tile_seams(torch_cuda, H, W):
    """From one pixel up, and the tile's width and height at one below, exact and one above; widths that are and are not multiples of
    4; with bands and without."""
    target, pred = _pair(H + W, (2, H, W))
    for R in (0, 1, 3):
        _check(torch_cuda, target, pred, R, "seam")


@pytest.mark.parametrize("n", [1, 2, 5])
def test_two_tiles_plus_one(torch_cuda, n):
    target, pred = _pair(n, (n, 2 * TILE_H + 1, 2 * TILE_W + 1))
    got = _check(torch_cuda, target, pred, 2, "two tiles plus one")
    assert (got[:, 81:].sum(axis=1) > 0).all() and (got[:, :81].sum(axis=1) > 0).all()
    _check(torch_cuda, target, pred, 0, "two tiles plus one")


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ALL_BINS_RADII + (0,))
def test_all_324_bins(torch_cuda, R):
    target, pred = all_bins_pair()
    got = _check(torch_cuda, np.stack([target, pred]), np.stack([pred, target]), R, "all bins")
    assert (got > 0).sum(axis=1).tolist() == ([ROW, ROW] if R else [81, 81])
    assert np.array_equal(got[0].reshape(4, 9, 9)[[0, 2, 1, 3]].transpose(0, 2, 1), got[1].reshape(4, 9, 9)), "swapping the masks transposes the table"


@pytest.mark.parametrize("H,W", [(64, 300), (37, 50)])
def test_noise_masks_fall_into_the_both_bands_table(torch_cuda, H, W):
    """Uniform noise of 3 classes: next to every pixel lies another value, in both masks, so f = 3 everywhere, and every row of the
    wave holds all nine bins."""
    rng = np.random.default_rng(H)
    target, pred = rng.integers(0, 3, (2, 2, H, W)).astype(np.uint8)
    got = _check(torch_cuda, target, pred, 3, "noise")
    assert (got[:, :243] == 0).all() and ((got[:, 243:] > 0).sum(axis=1) == 9).all()
    _check(torch_cuda, target, pred, 0, "noise")


@pytest.mark.parametrize("k", range(1, 10))
def test_rows_of_every_bin_count(torch_cuda, k):
    """One tile's width, k vertical stripes: every row of every wave holds exactly k bins, and the stripes' edges fall inside a lane's
    four pixels as well as between lanes; then one wide stripe and k - 1 stripes of three pixels (narrower than a lane's four); each
    with a prediction that splits every stripe again, so that a lane holds up to four keys."""
    H, W = 2 * WAVE_ROWS + 1, TILE_W
    x = np.arange(W)
    for stripe in ((x * k) // W, np.minimum(x // 3, k - 1)[::-1]):
        target = np.broadcast_to(stripe.astype(np.uint8), (2, H, W)).copy()
        assert len(np.unique(target)) == k
        pred = np.zeros_like(target)
        got = _check(torch_cuda, target, pred, 0, "%d stripes" % k)
        assert ((got > 0).sum(axis=1) == k).all()
        pred[:, :, 1::2] = 1
        _check(torch_cuda, target, pred, 0, "%d stripes, two predictions" % k)
        _check(torch_cuda, target, pred, 1, "%d stripes, two predictions" % k)


@pytest.mark.parametrize("values", [(0, 0), (2, 5), (255, 7), (8, 200)])
def test_a_constant_pair_fills_one_bin(torch_cuda, values):
    shape = (2, TILE_H + 3, TILE_W + 8)
    target, pred = np.full(shape, values[0], np.uint8), np.full(shape, values[1], np.uint8)
    for R in (0, 4):
        got = _check(torch_cuda, target, pred, R, "constant")
        assert (got > 0).sum(axis=1).tolist() == [1, 1] and got[0, min(values[0], 8) * 9 + min(values[1], 8)] == shape[1] * shape[2]


@pytest.mark.parametrize("classes", [2, 5, 8])
def test_class_blobs_with_255(torch_cuda, classes):
    target, pred = _pair(classes, (3, 70, 132), classes)
    assert (target == 255).any() and (pred == 255).any()
    for R in (2, 32):
        got = _check(torch_cuda, target, pred, R, "%d classes" % classes)
    assert (got.reshape(3, 4, 9, 9)[:, :, 8, :].sum(axis=(1, 2)) == (target == 255).reshape(3, -1).sum(axis=1)).all()


# ---- access forms ------------------------------------------------------------------------------------------------------------------
def test_widths_that_are_no_multiple_of_four(torch_cuda):
    for W in (49, 50, 51, 259):
        target, pred = _pair(W, (2, 21, W))
        _check(torch_cuda, target, pred, 2, "W % 4 != 0")


@pytest.mark.parametrize("offsets", [(1, 0, 0, 0), (0, 2, 0, 0), (3, 3, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0, 0, 1, 1), (0, 0, 2, 2), (0, 0, 0, 2),
                                     (1, 2, 3, 1), (0, 0, 4, 4), (4, 8, 4, 8)])
def test_views_that_are_not_aligned_for_the_wide_loads(torch_cuda, offsets):
    """W is a multiple of 4, but a mask lies 1..3 bytes into its buffer, or a dist2 plane 2 bytes (2 mod 4) or 4 bytes (4 mod 8) into
    its own: the byte and int16 loads.  The last two are aligned again: the wide loads at an offset."""
    target, pred = _pair(sum(offsets), (3, 19, 24))
    _check(torch_cuda, target, pred, 2, "offsets %s" % (offsets,), offsets=offsets)
    if not any(offsets[2:]):
        _check(torch_cuda, target, pred, 0, "offsets %s" % (offsets,), offsets=offsets)


def test_the_dist2_planes_are_read_as_numbers(torch_cuda):
    """Any int16 planes: negative values are inside every band, 32767 outside, the comparison is with R * R inclusive."""
    rng = np.random.default_rng(3)
    shape = (2, 33, 68)
    target, pred = _pair(4, shape)
    dist2 = tuple(rng.choice(np.array([-32768, -1, 0, 1, 8, 9, 10, 1024, 1025, 32767], np.int16), shape) for _ in range(2))
    for R in (3, 32):
        _same(_entry(torch_cuda, target, pred, R, dist2=dist2), rule_compare(target, pred, R, dist2=dist2), "dist2 as numbers, R=%d" % R)


# ---- batch and stream --------------------------------------------------------------------------------------------------------------
def test_images_of_a_batch_do_not_leak_into_each_other(torch_cuda):
    """Planes smaller than a tile, so a workgroup's loads would reach into the next image; the last row of one image and the first
    of the next differ everywhere."""
    shape = (1, 20, 36)
    a, b = np.full(shape, 1, np.uint8), class_blobs(3, shape, 3)
    pa, pb = class_blobs(5, shape, 2), np.full(shape, 2, np.uint8)
    both = _check(torch_cuda, np.concatenate([a, b, a]), np.concatenate([pa, pb, pa]), 2, "batch")
    alone = [_entry(torch_cuda, a, pa, 2)[0], _entry(torch_cuda, b, pb, 2)[0]]
    assert np.array_equal(both[0], alone[0]) and np.array_equal(both[1], alone[1]) and np.array_equal(both[2], alone[0])
    assert not np.array_equal(both[0], both[1])


def test_rows_are_fully_overwritten(torch_cuda):
    target, pred = _pair(6, (3, 40, 56))
    for fill in (-1, 0x7F7F7F7F7F7F7F7F, -2 ** 63):
        _check(torch_cuda, target, pred, 2, "rows filled with %d" % fill, fill=fill)
        _check(torch_cuda, target, pred, 0, "rows filled with %d" % fill, fill=fill)


def test_the_result_is_on_the_callers_stream(torch_cuda):
    """On a side stream the inputs are produced by that stream's own work (a long chain of fills, then the copies): the passes must
    run behind it, and an event recorded on that stream covers the rows."""
    from gan_segmentation_amd import mask_ops
    torch = torch_cuda
    target, pred = _pair(12, (4, 256, 256))
    want = rule_compare(target, pred, 2)
    src_t, src_p = torch.from_numpy(target).cuda(), torch.from_numpy(pred).cuda()
    dt, dp = torch.zeros_like(src_t), torch.zeros_like(src_p)
    ballast = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for k in range(20):
            ballast.fill_(k)
        dt.copy_(src_t)
        dp.copy_(src_p)
        rows = mask_ops.compare(dp, dt, band=2)
        done = torch.cuda.Event()
        done.record(side)
    done.synchronize()
    host = torch.empty(rows.shape, dtype=rows.dtype).pin_memory()
    with torch.cuda.stream(side):
        host.copy_(rows, non_blocking=True)
        side.synchronize()
    _same(host.numpy(), want, "side stream")


# ---- full size -------------------------------------------------------------------------------------------------------------------
def test_full_size(torch_cuda):
    target, pred = _pair(21, (2, 1024, 1024), classes=4)
    got = _check(torch_cuda, target, pred, 2, "1024 x 1024")
    assert (got.reshape(2, 4, 81).sum(axis=2) > 0).all()
    _check(torch_cuda, target, pred, 0, "1024 x 1024")


# ---- mask_ops --------------------------------------------------------------------------------------------------------------------
def test_compare_wrapper(torch_cuda):
    from gan_segmentation_amd import mask_ops
    torch = torch_cuda
    target, pred = _pair(8, (3, 45, 70))
    dt, dp = torch.from_numpy(target).cuda(), torch.from_numpy(pred).cuda()
    for band in (1, 2, 7):
        rows = mask_ops.compare(dp, dt, band=band)
        assert rows.shape == (3, ROW) and rows.dtype == torch.int64 and rows.is_contiguous() and rows.device == dt.device
        _same(rows.cpu().numpy(), rule_compare(target, pred, band), "compare, band %d" % band)
    flat = mask_ops.compare(dp, dt).cpu().numpy()
    _same(flat, rule_compare(target, pred, 0), "compare, no band")
    assert (flat[:, 81:] == 0).all() and (flat[:, :81].sum(axis=1) == 45 * 70).all()
    assert np.array_equal(dt.cpu().numpy(), target) and np.array_equal(dp.cpu().numpy(), pred), "an input was written to"
    # out and scratch: the caller's tensors are used, and the scratch holds the two distance planes afterwards
    out = torch.full((3, ROW), -1, dtype=torch.int64, device="cuda")
    scratch = (torch.empty(dt.shape, dtype=torch.int16, device="cuda"), torch.empty(dt.shape, dtype=torch.int16, device="cuda"))
    assert mask_ops.compare(dp, dt, band=3, out=out, scratch=scratch) is out
    _same(out.cpu().numpy(), rule_compare(target, pred, 3), "out and scratch")
    assert np.array_equal(scratch[0].cpu().numpy(), rule_boundary(target, 3)) and np.array_equal(scratch[1].cpu().numpy(), rule_boundary(pred, 3))
    # 2-D masks give one row; an empty batch gives none
    one = mask_ops.compare(dp[1], dt[1], band=2)
    assert one.shape == (ROW,)
    _same(one.cpu().numpy()[None], rule_compare(target[1], pred[1], 2), "2-D masks")
    assert mask_ops.compare(dp[:0], dt[:0], band=2).shape == (0, ROW)
    # a mask against itself: the diagonal only, and both bands or none
    own = mask_ops.compare(dt, dt, band=2).cpu().numpy().reshape(3, 4, 9, 9)
    assert (own[:, 1:3] == 0).all() and (own.sum(axis=1) * (1 - np.eye(9, dtype=np.int64)) == 0).all()
    for bad in (dict(pred=dp, target=dt[:2]), dict(pred=dp, target=dt.int()), dict(pred=dp, target=dt.cpu()), dict(pred=dp[:, :, ::2], target=dt[:, :, ::2]),
                dict(pred=dp, target=dt, band=33), dict(pred=dp, target=dt, band=-1), dict(pred=dp, target=dt, band=1.0), dict(pred=dp, target=dt, out=out[:2]),
                dict(pred=dp, target=dt, out=out.int()), dict(pred=dp, target=dt, out=out.cpu()), dict(pred=dp, target=dt, band=2, scratch=scratch[:1]),
                dict(pred=dp, target=dt, band=2, scratch=(scratch[0], scratch[0])), dict(pred=dp, target=dt, band=2, scratch=(scratch[0], scratch[1].int()))):
        with pytest.raises(ValueError):
            mask_ops.compare(**bad)


def test_apply_filters_is_the_chain_composed_by_hand(torch_cuda):
    from gan_segmentation_amd import mask_ops
    from tests.test_refine_host import case
    torch = torch_cuda
    img, mask = case(5, 2, 60, 76, 3, 3, frozen=0.0)
    di, dm = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()
    assert mask_ops.apply_filters(di, dm, 3) is dm
    assert mask_ops.apply_filters(di, dm, 3, min_area=1, refine_radius=5, connectivity=4, fill=0, ignore_label=9) is dm
    step = mask_ops.refine(di, dm, 2, 2, 3, sigma_space=1.5, sigma_colour=20.0)
    assert torch.equal(mask_ops.apply_filters(di, dm, 3, refine=2, refine_radius=2, refine_sigma_space=1.5, refine_sigma_colour=20.0), step)
    assert torch.equal(mask_ops.apply_filters(None, dm, 3, morph=True), mask_ops.morph_mask(dm))
    assert torch.equal(mask_ops.apply_filters(None, dm, 3, min_area=12, connectivity=4, fill=2), mask_ops.despeckle(dm, 12, 4, 2))
    assert torch.equal(mask_ops.apply_filters(None, dm, 3, ignore_band=2, ignore_label=250), mask_ops.ignore_band(dm, 2, 250))
    step = mask_ops.morph_mask(step)
    step = mask_ops.despeckle(step, 12, 8, "neighbour")
    step = mask_ops.ignore_band(step, 3, 255)
    full = mask_ops.apply_filters(di, dm, 3, refine=2, refine_radius=2, refine_sigma_space=1.5, refine_sigma_colour=20.0, morph=True, min_area=12,
                                  ignore_band=3)
    assert torch.equal(full, step) and not torch.equal(full, dm) and full.data_ptr() != dm.data_ptr()
    assert np.array_equal(dm.cpu().numpy(), mask) and np.array_equal(di.cpu().numpy(), img), "an input was written to"


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_solver_evaluate_masks_end_to_end(tmp_path, oracle_lib):
    """The set-up of tests/test_metrics.py::test_solver_evaluate_end_to_end.  The raw chain reproduces ``evaluate``'s accuracy and mIoU
    to the bit; the morph chain equals MaskAgreement fed by the rule on morph_mask's output; the band chain abstains."""
    import torch
    from PIL import Image
    from gan_segmentation_amd import annotation_io, mask_ops, params as P, weights as W
    from gan_segmentation_amd.metrics import MaskAgreement
    from gan_segmentation_amd.seg_solver import SegSolver
    from tests.common import reduced_setup
    gcfg, gp, dcfg, dp, z, noise = reduced_setup(6, batch=3)
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp)
    _rgb, img, feats = o.generator(z, noise)
    R = img.shape[1]
    rng = np.random.default_rng(5)
    data = tmp_path / "data"
    labels = []
    for i in range(3):
        annotation_io.export_sample(str(data), i, img[i], [f[i] for f in feats])
        m = rng.choice(np.array([20, 128, 230], np.uint8), size=(R, R), p=[0.2, 0.4, 0.4])   # ignore / background / class 1
        Image.fromarray(m, "L").save(str(data / ("mask_%06d.png" % i)))
        labels.append(annotation_io.preprocess_mask(m))
    ckpt = tmp_path / "checkpoints"
    ckpt.mkdir()
    P.save_params(str(ckpt / "checkpoint_last.params"), W.complete_decoder_params(dcfg, dp))
    solver = SegSolver(6, str(data), str(ckpt), gpu_ids=[0], in_channels=W.generator_channels(gcfg))
    nclass = dcfg["num_classes"]
    plain = dict(solver.evaluate(str(data)))
    band = 2
    result = solver.evaluate_masks(str(data), {"raw": {}, "morph": {"morph": True}, "band": {"ignore_band": 2}}, band=band)
    assert list(result) == ["raw", "morph", "band"]
    names = ["accuracy", "mean-iou", "band-accuracy", "boundary-iou", "abstained", "changed"]
    assert all([k for k, _v in values] == names for values in result.values())
    raw, morph, banded = (dict(result[k]) for k in ("raw", "morph", "band"))
    assert raw["accuracy"] == plain["accuracy"] and raw["mean-iou"] == plain["mean-iou"]
    assert raw["changed"] == 0.0 and raw["abstained"] == 0.0
    # the morph chain by hand: the decoder's mask per sample, morph_mask on the device, the rule on the host
    want, moved, pixels = MaskAgreement(nclass), 0, 0
    for i in range(3):
        _logits, mask = solver.net(*[f[i] for f in feats], want_mask=True)
        cleaned = mask_ops.morph_mask(mask).cpu().numpy()
        target = np.where(labels[i] < 0, 255, labels[i]).astype(np.uint8)[None]
        want.update_rows(rule_compare(target, cleaned, band))
        moved += int((cleaned != mask.cpu().numpy()).sum())
        pixels += cleaned.size
    for name, value in want.get_name_value():
        assert morph[name] == value or (np.isnan(morph[name]) and np.isnan(value)), name
    assert morph["changed"] == moved / pixels and moved > 0
    assert banded["abstained"] > 0 and banded["changed"] > 0
    assert not np.isnan(raw["band-accuracy"]) and not np.isnan(raw["boundary-iou"])
    torch.cuda.synchronize()
