"""The pair previews without a GPU (csrc/gsa_overlay.h, gan_segmentation_amd/preview.py): ``rule_overlay``,
the numpy restatement of the header's rule that tests/test_gpu_overlay.py and tests/test_host_emu_overlay.py compare the kernel with,
held to what the reference's get_draw_mask returned (tests/golden/draw_mask_golden.npz); ``make_lut``; the thumbnail rounding at its
extremes; the geometry of a sheet; the two generate keys; and the command-line tool's file naming with the device call replaced."""
import os

import numpy as np
import pytest

from gan_segmentation_amd import preview
from tests.test_boundary_host import class_blobs, rule_boundary

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "draw_mask_golden.npz")
FACTORS = (1, 2, 4, 8, 16)


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def rule_edges(mask):
    """(n, H, W) u8 -> bool: whether a 4-neighbour inside the same plane holds another raw value."""
    e = np.zeros(mask.shape, bool)
    d = mask[:, 1:, :] != mask[:, :-1, :]
    e[:, 1:, :] |= d
    e[:, :-1, :] |= d
    d = mask[:, :, 1:] != mask[:, :, :-1]
    e[:, :, 1:] |= d
    e[:, :, :-1] |= d
    return e


def rule_blend(img, mask, lut):
    """img (n, H, W, C) u8, mask (n, H, W) u8, lut (256, 6) u8 -> int64 (n, H, W, C): b of the header."""
    C = img.shape[-1]
    rows = lut[mask].astype(np.int64)
    w = np.minimum(np.where(rule_edges(mask), rows[..., 5], rows[..., 4]), 128)[..., None]
    return (w * rows[..., :C] + (128 - w) * img.astype(np.int64)) >> 7


def rule_overlay(img, mask, lut, factor=1, cols=1):
    """The header's rule, whole: -> the sheet (ceil(n / cols) * H/f, cols * W/f, C) u8.  Integer arithmetic in int64 throughout."""
    img, mask, lut = np.asarray(img), np.asarray(mask), np.asarray(lut)
    assert img.dtype == mask.dtype == lut.dtype == np.uint8 and img.ndim == 4 and mask.shape == img.shape[:3] and lut.shape == (256, 6)
    n, H, W, C = img.shape
    f = int(factor)
    assert f in FACTORS and H % f == 0 and W % f == 0 and cols >= 1 and 1 <= C <= 4
    h, w = H // f, W // f
    b = rule_blend(img, mask, lut)
    t = (b.reshape(n, h, f, w, f, C).sum(axis=(2, 4)) + f * f // 2) >> (2 * FACTORS.index(f))
    assert t.min(initial=0) >= 0 and t.max(initial=0) <= 255
    rows = -(-n // cols)
    sheet = np.zeros((rows * h, cols * w, C), np.uint8)
    for i in range(n):
        y, x = (i // cols) * h, (i % cols) * w
        sheet[y:y + h, x:x + w] = t[i]
    return sheet


# ---- inputs the GPU and emulation tests share --------------------------------------------------------------------------------------
def random_image(seed, n, H, W, C):
    """Random bytes with blocks of the extreme values 0 and 255 in them."""
    rng = np.random.default_rng([seed, n, H, W, C])
    img = rng.integers(0, 256, (n, H, W, C)).astype(np.uint8)
    img[:, : max(1, H // 5), : max(1, W // 4)] = 255
    img[:, H - max(1, H // 6):, W - max(1, W // 3):] = 0
    return img


def blob_masks(seed, n, H, W, classes=4):
    """Class blobs a few pixels across (they cross every tile border of a plane larger than a tile), value 255 among them."""
    return np.stack([class_blobs(seed + i, (H, W), classes, sigma=3.0, with255=True) for i in range(n)])


def random_lut(seed):
    """A table with a colour and two weights for every value: weights over the whole byte range (those above 128 are clamped),
    w_edge drawn apart from w_in, and the weights 0, 1, 64, 127, 128 and 200 on the first rows."""
    rng = np.random.default_rng([seed, 6])
    lut = rng.integers(0, 256, (256, 6)).astype(np.uint8)
    lut[:, 4:] = rng.integers(0, 160, (256, 2))
    special = [0, 1, 64, 127, 128, 200]
    lut[:6, 4] = special
    lut[:6, 5] = special[::-1]
    lut[255, 4:] = (128, 0)
    return lut


def dataset_lut():
    """What generate's previews use."""
    return preview.make_lut(preview.DATASET_COLOURS, alpha=0.5, outline=1.0)


# ---- the rule against the reference and against the boundary distance ------------------------------------------------------------
def test_rule_and_make_lut_give_what_get_draw_mask_gave():
    """The reference's float blend at alpha = k/128, truncated to u8, is (k*c + (128-k)*p) >> 7: every golden output, byte for byte,
    from make_lut(REFERENCE_COLOURS, alpha, skip_background) without an outline."""
    with np.load(GOLDEN) as z:
        img, mask = z["img"], z["mask"]
        assert img.shape == (24, 20, 3) and set(np.unique(mask)) == {0, 1, 2, 3} and img.min() == 0 and img.max() == 255
        assert {int(v): tuple(int(x) for x in c) for v, c in zip(z["colour_values"], z["colours"])} == preview.REFERENCE_COLOURS
        seen = 0
        for alpha in z["alphas"]:
            for skip in (True, False):
                want = z["drawn_%03d_%s" % (round(float(alpha) * 100), "skip" if skip else "all")]
                lut = preview.make_lut(preview.REFERENCE_COLOURS, alpha=float(alpha), skip_background=skip)
                got = rule_overlay(img[None], mask[None], lut)
                assert got.shape == img.shape and np.array_equal(got, want), "alpha %s skip %s" % (alpha, skip)
                assert np.array_equal(got[mask == 3], img[mask == 3]) and (skip or alpha < 1 or (got[mask == 0] == 0).all())
                seen += not np.array_equal(want, img)
        assert seen == 8


def test_an_edge_pixel_is_a_pixel_at_boundary_distance_one():
    for seed, shape in ((1, (2, 37, 41)), (2, (1, 1, 9)), (3, (1, 9, 1)), (4, (3, 16, 16))):
        mask = blob_masks(seed, *shape)
        assert np.array_equal(rule_edges(mask), rule_boundary(mask, 1) == 1)
    facing = np.zeros((2, 4, 6), np.uint8)
    facing[1] = 5                                         # the last row of sample 0 and the first of sample 1 differ: no edge
    assert not rule_edges(facing).any()


def test_rule_blend_weights():
    """w = 0 leaves the pixel, 128 gives the colour, 64 the truncated mean; a weight above 128 is 128; the edge weight applies on
    edge pixels only."""
    img = random_image(5, 1, 8, 12, 4)
    mask = np.zeros((1, 8, 12), np.uint8)
    mask[0, :, 6:] = 1
    edge = rule_edges(mask)[0]
    assert edge[:, 5:7].all() and not edge[:, :5].any() and not edge[:, 7:].any()
    lut = np.zeros((256, 6), np.uint8)
    lut[0] = (10, 20, 30, 40, 0, 128)
    lut[1] = (250, 0, 255, 3, 64, 200)
    got = rule_overlay(img, mask, lut)
    assert np.array_equal(got[:, :5], img[0, :, :5]) and (got[:, 5] == (10, 20, 30, 40)).all()
    assert (got[:, 6] == (250, 0, 255, 3)).all()
    assert np.array_equal(got[:, 7:], ((np.array([250, 0, 255, 3]) + img[0, :, 7:].astype(np.int64)) >> 1).astype(np.uint8))


# ---- make_lut ----------------------------------------------------------------------------------------------------------------
def test_make_lut_tables():
    lut = preview.make_lut()
    assert lut.shape == (256, 6) and lut.dtype == np.uint8
    assert tuple(lut[1]) == (13, 198, 20, 255, 64, 64) and tuple(lut[2]) == (54, 30, 211, 255, 64, 64)
    assert not lut[0].any() and not lut[3:].any()
    lut = preview.make_lut(skip_background=False, alpha=1.0)
    assert tuple(lut[0]) == (0, 0, 0, 255, 128, 128)
    lut = preview.make_lut(preview.DATASET_COLOURS, alpha=0.25, outline=1.0)
    assert set(np.flatnonzero(lut[:, 4])) == {1, 2, 3, 4, 5, 6, 7, 255} and (lut[lut[:, 4] > 0, 4:] == (32, 128)).all()
    assert not lut[0].any() and not lut[8].any(), "a value without a colour keeps both weights 0, outline included"
    assert tuple(lut[255, :3]) == (128, 128, 128)
    assert len({tuple(c) for c in preview.DATASET_COLOURS.values()}) == len(preview.DATASET_COLOURS)
    assert all(preview.DATASET_COLOURS[v] == c for v, c in preview.REFERENCE_COLOURS.items())
    lut = preview.make_lut({7: (9,), 8: (1, 2, 3, 4)}, alpha=0, outline=1 / 128)
    assert tuple(lut[7]) == (9, 255, 255, 255, 0, 1) and tuple(lut[8]) == (1, 2, 3, 4, 0, 1)


@pytest.mark.parametrize("kw", [dict(alpha=0.3), dict(alpha=-0.5), dict(alpha=1.5), dict(alpha=None), dict(alpha=True), dict(outline=0.501),
                                dict(outline=2), dict(outline="1"), dict(colours={256: (1, 2, 3)}), dict(colours={-1: (1, 2, 3)}),
                                dict(colours={1: ()}), dict(colours={1: (1, 2, 3, 4, 5)}), dict(colours={1: (1, 2, 256)}),
                                dict(colours={1: (1.5, 2, 3)})])
def test_make_lut_refusals(kw):
    with pytest.raises(ValueError) as e:
        preview.make_lut(**kw)
    if "colours" not in kw:
        assert "multiple of 1/128" in str(e.value)


# ---- thumbnails and sheets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", FACTORS)
def test_thumbnail_rounding_at_the_extremes(f):
    """All 255 stays 255 and all 0 stays 0 at every factor (the rounding term never carries past a byte); a block of half 0 and
    half 255 rounds half up; one pixel of 1 in a block of 16 x 16 zeros rounds down."""
    lut = np.zeros((256, 6), np.uint8)
    mask = np.zeros((1, 32, 32), np.uint8)
    for v in (0, 255):
        img = np.full((1, 32, 32, 3), v, np.uint8)
        assert (rule_overlay(img, mask, lut, f) == v).all()
    lut[0] = (255, 255, 255, 255, 128, 128)
    assert (rule_overlay(np.zeros((1, 32, 32, 2), np.uint8), mask, lut, f) == 255).all()
    if f > 1:
        img = np.zeros((1, 32, 32, 1), np.uint8)
        img[0, ::2] = 255
        assert (rule_overlay(img, mask, np.zeros((256, 6), np.uint8), f) == 128).all()          # 127.5 rounds up
        img[:] = 0
        img[0, 0, 0] = f * f // 2 - 1
        img[0, 0, f] = f * f // 2
        got = rule_overlay(img, mask, np.zeros((256, 6), np.uint8), f)
        assert got[0, 0, 0] == 0 and got[0, 1, 0] == 1 and got.sum() == 1


@pytest.mark.parametrize("n,cols", [(5, 1), (5, 2), (5, 3), (5, 5), (5, 7), (1, 1), (4, 2)])
def test_sheet_geometry(n, cols):
    """Sample i in the cell at row i // cols, column i % cols; the cells behind the last sample are 0; cols = 1 is the batch."""
    H, W, C, f = 8, 12, 3, 2
    img, mask, lut = random_image(n, n, H, W, C), blob_masks(n, n, H, W), random_lut(1)
    sheet = rule_overlay(img, mask, lut, f, cols)
    rows = -(-n // cols)
    assert sheet.shape == preview.sheet_shape(n, H, W, C, cols, f) == (rows * 4, cols * 6, C)
    each = rule_overlay(img, mask, lut, f, 1).reshape(n, 4, 6, C)
    for cell in range(rows * cols):
        got = sheet[(cell // cols) * 4:(cell // cols + 1) * 4, (cell % cols) * 6:(cell % cols + 1) * 6]
        assert np.array_equal(got, each[cell]) if cell < n else not got.any()
    assert each.any(axis=(1, 2, 3)).all()


# ---- the generate keys -------------------------------------------------------------------------------------------------------
def test_preview_keys():
    assert [preview.check_preview_every(v) for v in (0, 1, 7, np.int64(3))] == [0, 1, 7, 3]
    assert [preview.check_preview_downscale(v) for v in (1, 2, 4, 8, 16)] == [1, 2, 4, 8, 16]
    for bad in (-1, 1.0, "2", None, True, [1]):
        with pytest.raises(ValueError, match="PREVIEW_EVERY"):
            preview.check_preview_every(bad)
    for bad in (0, 3, 32, -2, 2.0, "4", None, True):
        with pytest.raises(ValueError, match="PREVIEW_DOWNSCALE"):
            preview.check_preview_downscale(bad)
    assert preview.preview_indices(10, 4, 0) == [] and preview.preview_indices(10, 4, 1) == [0, 1, 2, 3]
    assert preview.preview_indices(10, 4, 3) == [2] and preview.preview_indices(0, 5, 2) == [0, 2, 4] and preview.preview_indices(7, 3, 11) == []


def test_generate_refuses_a_bad_preview_key_before_it_loads_a_model(tmp_path):
    """No GPU, no model files: the key is what fails, as the other additive keys do."""
    from gan_segmentation_amd import main as cli
    cfg = {"BASE_DIR": str(tmp_path), "GAN": "ffhq", "GAN_DIR": str(tmp_path / "none"), "GAN_GPU_IDS": [0], "GAN_BATCH_SIZE_PER_GPU": 2}
    with pytest.raises(ValueError, match="PREVIEW_EVERY"):
        cli.generate(dict(cfg, PREVIEW_EVERY=-2))
    with pytest.raises(ValueError, match="PREVIEW_DOWNSCALE"):
        cli.generate(dict(cfg, PREVIEW_EVERY=2, PREVIEW_DOWNSCALE=3))


# ---- the command-line tool -------------------------------------------------------------------------------------------------------
def _write_dataset(directory, n, H=16, W=32, first=0):
    from PIL import Image
    img, mask = random_image(n, n, H, W, 3), blob_masks(n, n, H, W)
    for i in range(n):
        Image.fromarray(img[i], "RGB").save(str(directory / ("img_%06d.jpg" % (first + i))), quality=95)
        Image.fromarray(mask[i], "L").save(str(directory / ("mask_%06d.png" % (first + i))))
    return mask


def test_cli_names_a_sheet_by_its_first_sample(tmp_path, monkeypatch, capsys):
    """11 samples, --cols 2: sheets of 4, 4 and 3 samples named 0, 4 and 8, each (2 * h, 2 * w); --first / --count select a range;
    the masks reach the device call as written.  The device call is replaced by the rule."""
    from PIL import Image
    masks = _write_dataset(tmp_path, 11)
    calls = []

    def on_host(imgs, m, cols, lut, factor):
        calls.append((imgs.shape, m.copy(), cols, factor))
        return rule_overlay(imgs, m, lut, factor, cols)

    monkeypatch.setattr(preview, "_sheet_on_device", on_host)
    assert preview.main([str(tmp_path), "--cols", "2", "--downscale", "4"]) == 0
    sheets = sorted(p.name for p in tmp_path.glob("preview_sheet_*"))
    assert sheets == ["preview_sheet_000000.jpg", "preview_sheet_000004.jpg", "preview_sheet_000008.jpg"]
    assert [c[0] for c in calls] == [(4, 16, 32, 3), (4, 16, 32, 3), (3, 16, 32, 3)] and all(c[2:] == (2, 4) for c in calls)
    assert np.array_equal(np.concatenate([c[1] for c in calls]), masks)
    for name in sheets:
        im = Image.open(str(tmp_path / name))
        assert im.size == (16, 8) and im.mode == "RGB"
    assert "samples 8..10" in capsys.readouterr().out
    assert len(list(tmp_path.iterdir())) == 22 + 3

    del calls[:]
    assert preview.main([str(tmp_path), "--cols", "2", "--downscale", "1", "--first", "3", "--count", "5", "--alpha", "0.25", "--outline", "0"]) == 0
    assert [c[0][0] for c in calls] == [4, 1] and np.array_equal(np.concatenate([c[1] for c in calls]), masks[3:8])
    assert (tmp_path / "preview_sheet_000003.jpg").exists() and (tmp_path / "preview_sheet_000007.jpg").exists()
    assert Image.open(str(tmp_path / "preview_sheet_000007.jpg")).size == (64, 16)


def test_cli_refusals(tmp_path, monkeypatch):
    monkeypatch.setattr(preview, "_sheet_on_device", lambda *a: pytest.fail("nothing to overlay"))
    assert preview.main([str(tmp_path)]) == 1                                        # no pair
    assert preview.main([str(tmp_path), "--downscale", "3"]) == 2
    assert preview.main([str(tmp_path), "--alpha", "0.3"]) == 2
    assert preview.main([str(tmp_path), "--cols", "0"]) == 2
    _write_dataset(tmp_path, 2)
    assert preview.main([str(tmp_path), "--first", "2"]) == 1
