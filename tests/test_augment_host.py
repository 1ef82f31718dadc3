"""The training stream on the host side, without a GPU: the numpy restatement of the canonical rule of include/gsa_augment.h
(``rule_augment``, which tests/test_gpu_augment.py holds the kernel to bit for bit), the augmentation plan and the stream's index
arithmetic of gan-segmentation_amd/augment.py, the C ABI against the library's exports, and the keyword validation."""
import numpy as np
import pytest

F = np.float32


def bf16_rne(v):
    """fp32 array -> the fp32 values of its round-to-nearest-even bf16 (low 16 bits zero)."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) << np.uint64(16)
    return r.astype(np.uint32).view(np.float32)


def rule_augment(img, mask, matrices, out_size, scale, bias, ignore=255, bf16=False):
    """img (N, H, W, C) u8, mask (N, H, W) u8, matrices (N, 6) fp32 -> (image (N, C, oh, ow) fp32, label (N, oh, ow) u8).
    Every multiply and every add is one numpy float32 operation, in the order the header writes them."""
    img, mask = np.asarray(img), np.asarray(mask)
    assert img.dtype == np.uint8 and mask.dtype == np.uint8
    N, H, W, C = img.shape
    oh, ow = (out_size, out_size) if np.isscalar(out_size) else out_size
    matrices = np.asarray(matrices)
    assert matrices.dtype == np.float32 and matrices.shape == (N, 6)
    scale, bias = np.asarray(scale), np.asarray(bias)
    assert scale.dtype == np.float32 and bias.dtype == np.float32 and len(scale) == C and len(bias) == C
    X = np.arange(ow, dtype=np.float32)[None, :]
    Y = np.arange(oh, dtype=np.float32)[:, None]
    image = np.empty((N, C, oh, ow), np.float32)
    label = np.empty((N, oh, ow), np.uint8)
    one, half, zero = F(1.0), F(0.5), F(0.0)
    for n in range(N):
        a, b, c, d, e, f = (F(v) for v in matrices[n])
        xs = (a * X + b * Y) + c
        ys = (d * X + e * Y) + f
        x0, y0 = np.floor(xs), np.floor(ys)
        fx, fy = xs - x0, ys - y0
        src = img[n].astype(np.float32)

        def tap(yf, xf):
            inside = (xf >= zero) & (xf <= F(W - 1)) & (yf >= zero) & (yf <= F(H - 1))       # decided on the floats
            yi = np.where(inside, yf, zero).astype(np.int64)
            xi = np.where(inside, xf, zero).astype(np.int64)
            return np.where(inside[:, :, None], src[yi, xi], zero)

        p00, p01, p10, p11 = tap(y0, x0), tap(y0, x0 + one), tap(y0 + one, x0), tap(y0 + one, x0 + one)
        top = p00 + fx[:, :, None] * (p01 - p00)
        bot = p10 + fx[:, :, None] * (p11 - p10)
        v = top + fy[:, :, None] * (bot - top)
        out = v * scale[None, None, :] + bias[None, None, :]
        assert out.dtype == np.float32
        image[n] = out.transpose(2, 0, 1)
        xn, yn = np.floor(xs + half), np.floor(ys + half)
        inside = (xn >= zero) & (xn <= F(W - 1)) & (yn >= zero) & (yn <= F(H - 1))
        yi = np.where(inside, yn, zero).astype(np.int64)
        xi = np.where(inside, xn, zero).astype(np.int64)
        label[n] = np.where(inside, mask[n][yi, xi], np.uint8(ignore))
    return (bf16_rne(image) if bf16 else image), label


def random_pair(seed, n, H, W, C, classes=3):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, H, W, C), dtype=np.uint8), rng.integers(0, classes, (n, H, W), dtype=np.uint8)


def _rows(n, row):
    return np.tile(np.asarray(row, np.float32)[None, :], (n, 1))


def _norm(C=3):
    from gan_segmentation_amd import augment
    return augment.normalisation(augment.IMAGENET_MEAN[:C], augment.IMAGENET_STD[:C])


# -- the rule ------------------------------------------------------------------------------------------------------------------
def test_identity_is_scale_and_bias():
    img, mask = random_pair(0, 2, 512, 512, 3)
    scale, bias = _norm()
    image, label = rule_augment(img, mask, _rows(2, [1, 0, 0, 0, 1, 0]), 512, scale, bias)
    want = img.astype(np.float32) * scale + bias
    assert np.array_equal(image.view(np.uint32), np.ascontiguousarray(want.transpose(0, 3, 1, 2)).view(np.uint32))
    assert np.array_equal(label, mask)


def test_mirror_matrix_is_the_exact_mirror_image():
    img, mask = random_pair(1, 2, 512, 512, 3)
    scale, bias = _norm()
    ident = rule_augment(img, mask, _rows(2, [1, 0, 0, 0, 1, 0]), 512, scale, bias)
    flipped = rule_augment(img, mask, _rows(2, [-1, 0, 511, 0, 1, 0]), 512, scale, bias)
    assert np.array_equal(flipped[0], ident[0][:, :, :, ::-1])
    assert np.array_equal(flipped[1], mask[:, :, ::-1])


def test_centre_crop_and_centred_padding():
    from gan_segmentation_amd import augment
    img, mask = random_pair(2, 1, 512, 512, 3)
    scale, bias = _norm()
    m = augment.plan_matrices(0, 0, 1, 512, 512, 480, mode="center")
    assert np.array_equal(m, _rows(1, [1, 0, 16, 0, 1, 16]))
    image, label = rule_augment(img, mask, m, 480, scale, bias)
    assert np.array_equal(label, mask[:, 16:496, 16:496])
    assert np.array_equal(image, (img.astype(np.float32) * scale + bias).transpose(0, 3, 1, 2)[:, :, 16:496, 16:496])
    img, mask = random_pair(3, 1, 256, 256, 3)
    m = augment.plan_matrices(0, 0, 1, 256, 256, 480, mode="center")
    assert np.array_equal(m, _rows(1, [1, 0, -112, 0, 1, -112]))
    image, label = rule_augment(img, mask, m, 480, scale, bias)
    assert int((label == 255).sum()) == 480 * 480 - 256 * 256          # exactly 1 - (256/480)^2 of the canvas
    assert np.array_equal(label[:, 112:368, 112:368], mask)
    assert np.array_equal(image[0, :, 0, 0], bias)                     # the image border is 0 before the normalisation


def test_half_pixel_boundaries_by_hand():
    """A shift of exactly half a pixel: the bilinear value is the mean of four taps, the label takes floor(x + 0.5) -- the pixel to
    the right / below -- where rint (half to even) would take the left one at 0.5 and stay inside at 2.5."""
    img = np.array([[10, 20, 50], [30, 40, 90], [0, 0, 0]], np.uint8)[None, :, :, None]
    mask = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.uint8)[None]
    one, zero = np.array([1.0], np.float32), np.array([0.0], np.float32)
    image, label = rule_augment(img, mask, _rows(1, [1, 0, 0.5, 0, 1, 0.5]), 4, one, zero)
    assert image[0, 0, 0, 0] == 25.0                   # (10 + 20 + 30 + 40) / 4
    assert image[0, 0, 0, 1] == 50.0                   # (20 + 50 + 40 + 90) / 4
    assert image[0, 0, 0, 2] == 35.0                   # x taps 2 and 3: (50 + 0)/2 = 25, (90 + 0)/2 = 45, their mean
    assert image[0, 0, 1, 0] == 17.5                   # rows 1 and 2: (35 + 0) / 2
    assert image[0, 0, 3, 3] == 0.0
    assert label[0, 0, 0] == 5 and np.rint(0.5) == 0   # floor(0.5 + 0.5) = 1 in both axes: mask[1, 1]
    assert label[0, 1, 1] == 9                         # 1.5 -> 2
    assert label[0, 2, 0] == 255 and np.rint(2.5) == 2  # 2.5 -> 3: outside, where rint would stay at 2
    assert label[0, 0, 2] == 255
    # a quarter-pixel shift by hand: 10 + 0.25 * (20 - 10)
    image, label = rule_augment(img, mask, _rows(1, [1, 0, 0.25, 0, 1, 0]), 4, one, zero)
    assert image[0, 0, 0, 0] == 12.5 and label[0, 0, 0] == 1
    # far-off and non-finite coordinates are outside, never wrapped
    image, label = rule_augment(img, mask, _rows(1, [1, 0, 3e9, 0, 1, -3e38]), 4, one, zero)
    assert np.all(image == 0.0) and np.all(label == 255)
    image, label = rule_augment(img, mask, _rows(1, [1, 0, 2.0 ** 32, 0, 1, 0]), 4, one, zero, ignore=7)
    assert np.all(image == 0.0) and np.all(label == 7)


def test_bf16_rounding_is_nearest_even():
    just_above = np.nextafter(F(1.00390625), F(2.0))
    v = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, just_above, 0.0], np.float32)     # 1 + 2^-8 ties to even (down), 1 + 3*2^-8 ties up
    assert np.array_equal(bf16_rne(v), np.array([1.0, 1.0, 1.015625, -1.0, 1.0078125, 0.0], np.float32))


def test_normalisation_constants():
    from gan_segmentation_amd import augment
    scale, bias = augment.normalisation()
    assert scale.dtype == np.float32 and bias.dtype == np.float32
    assert np.array_equal(scale, (1.0 / (255.0 * np.array([0.229, 0.224, 0.225]))).astype(np.float32))
    assert np.array_equal(bias, (-np.array([0.485, 0.456, 0.406]) / np.array([0.229, 0.224, 0.225])).astype(np.float32))
    for bad in (((0.5,), (0.0,)), ((0.5, 0.5), (1.0,)), ((0.1,) * 5, (1.0,) * 5), ((np.nan,), (1.0,))):
        with pytest.raises(ValueError):
            augment.normalisation(*bad)


# -- the plan ------------------------------------------------------------------------------------------------------------------
def test_plan_is_deterministic_and_shard_invariant():
    from gan_segmentation_amd import augment
    a = augment.plan_matrices(5, 0, 16, 512, 512, 480)
    assert a.dtype == np.float32 and a.shape == (16, 6)
    assert np.array_equal(a, augment.plan_matrices(5, 0, 16, 512, 512, 480))
    assert np.array_equal(a[8:], augment.plan_matrices(5, 8, 8, 512, 512, 480))
    assert not np.array_equal(a, augment.plan_matrices(6, 0, 16, 512, 512, 480))
    assert len({tuple(r) for r in a}) == 16
    # the draws are the documented chain
    from gan_segmentation_amd.style_mix import splitmix64
    u = splitmix64(np.uint64(5 ^ augment.AUGMENT_SEED_XOR) ^ np.uint64(3))
    r = augment.uniforms(5, 3, 1)[0]
    for k in range(7):
        assert r[k] == float(int(u) >> 11) * 2.0 ** -53
        u = splitmix64(u)


def test_drawn_parameters_stay_within_their_limits():
    from gan_segmentation_amd import augment
    n = 10000
    p = augment.plan_parameters(9, 0, n, 512, 512, 480)
    assert abs(p["flip"].mean() - 0.5) <= 0.02
    assert np.all(np.abs(p["angle"]) <= 15.0) and p["angle"].min() < -14.0 and p["angle"].max() > 14.0
    assert np.all((p["scale"] >= 0.75) & (p["scale"] <= 1.25)) and p["scale"].min() < 0.76 and p["scale"].max() > 1.24
    for k in ("dx", "dy"):
        assert np.all(np.abs(p[k]) <= 0.0625 * 512) and p[k].min() < -31.0 and p[k].max() > 31.0
    for k in ("ox", "oy"):
        assert p[k].min() == 0 and p[k].max() == 32 and set(np.unique(p[k])) == set(range(33))
    assert p["pad_x"] == 0 and p["pad_y"] == 0
    q = augment.plan_parameters(9, 0, n, 256, 256, 480, rotate=5, scale=0.1, shift=0.5, flip=0.25)
    assert abs(q["flip"].mean() - 0.25) <= 0.02 and np.all(np.abs(q["angle"]) <= 5.0) and np.all(np.abs(q["scale"] - 1.0) <= 0.1)
    assert np.all(np.abs(q["dx"]) <= 128.0) and np.all(q["ox"] == 0) and np.all(q["oy"] == 0) and q["pad_x"] == 112 and q["pad_y"] == 112
    assert np.array_equal(q["flip"], augment.uniforms(9, 0, n)[:, 0] < 0.25)


def test_all_limits_zero_is_the_identity():
    from gan_segmentation_amd import augment
    m = augment.plan_matrices(3, 100, 64, 512, 384, None, rotate=0, scale=0, shift=0, flip=0)
    assert np.array_equal(m, _rows(64, [1, 0, 0, 0, 1, 0]))
    assert not np.any(np.signbit(m))
    assert augment.output_size(512, 384, None) == (512, 384)
    # flip alone is the exact mirror matrix
    m = augment.plan_matrices(3, 100, 64, 512, 384, None, rotate=0, scale=0, shift=0, flip=1)
    assert np.array_equal(m, _rows(64, [-1, 0, 383, 0, 1, 0]))


def test_center_mode_gives_integer_translations():
    from gan_segmentation_amd import augment
    for H, W, crop in ((512, 512, 480), (256, 256, 480), (1024, 1024, 1024), (300, 500, 480), (128, 128, None)):
        m = augment.plan_matrices(1, 7, 5, H, W, crop, mode="center")
        assert np.array_equal(m[:, [0, 1, 3, 4]], _rows(5, [1, 0, 0, 1]))
        assert np.array_equal(m[:, [2, 5]], np.round(m[:, [2, 5]]))
        assert np.array_equal(m, _rows(5, m[0]))
        cw, ch = (W, H) if crop is None else (crop, crop)
        PW, PH = max(W, cw), max(H, ch)
        assert m[0, 2] == (PW - cw) // 2 - (PW - W) // 2 and m[0, 5] == (PH - ch) // 2 - (PH - H) // 2


@pytest.mark.parametrize("H,W,crop", [(512, 512, 480), (256, 256, 480), (300, 500, 480)])
def test_forward_map_of_the_returned_inverse_is_the_identity(H, W, crop):
    """Rounding the six entries to fp32 moves a crop corner by at most half an ulp of each entry times its coordinate: 6.6e-5 px at
    crop 480 with |c|, |f| < 1024.  The bound here is 1e-4 px, for the sources that keep that premise (a 1024 px source cropped at
    480 does not: its translations pass 1024, where an ulp is twice as large)."""
    from gan_segmentation_amd import augment
    n = 2000
    inv = augment.plan_matrices(11, 0, n, H, W, crop).astype(np.float64).reshape(n, 2, 3)
    fwd = augment.forward_matrices(augment.plan_parameters(11, 0, n, H, W, crop), H, W)
    assert np.all(np.abs(inv[:, :, 2]) < 1024.0)
    worst = 0.0
    for X in (0.0, crop - 1.0):
        for Y in (0.0, crop - 1.0):
            sx = inv[:, 0, 0] * X + inv[:, 0, 1] * Y + inv[:, 0, 2]
            sy = inv[:, 1, 0] * X + inv[:, 1, 1] * Y + inv[:, 1, 2]
            bx = fwd[:, 0, 0] * sx + fwd[:, 0, 1] * sy + fwd[:, 0, 2]
            by = fwd[:, 1, 0] * sx + fwd[:, 1, 1] * sy + fwd[:, 1, 2]
            worst = max(worst, float(np.abs(bx - X).max()), float(np.abs(by - Y).max()))
    assert worst < 1e-4, worst


def test_forward_map_is_the_documented_chain():
    """forward_matrices against the five steps of the module docstring, applied one after the other to a point."""
    from gan_segmentation_amd import augment
    H, W, crop = 300, 500, 480
    p = augment.plan_parameters(2, 40, 50, H, W, crop)
    fwd = augment.forward_matrices(p, H, W)
    x, y = 123.25, 77.5
    for i in range(50):
        px = (W - 1) - x if p["flip"][i] else x
        th = np.deg2rad(p["angle"][i])
        cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
        qx = p["scale"][i] * (np.cos(th) * (px - cx) - np.sin(th) * (y - cy)) + cx + p["dx"][i]
        qy = p["scale"][i] * (np.sin(th) * (px - cx) + np.cos(th) * (y - cy)) + cy + p["dy"][i]
        qx, qy = qx + p["pad_x"] - p["ox"][i], qy + p["pad_y"] - p["oy"][i]
        got = fwd[i] @ np.array([x, y, 1.0])
        assert abs(got[0] - qx) < 1e-9 and abs(got[1] - qy) < 1e-9
    assert p["pad_x"] == 0 and p["pad_y"] == 90 and p["ox"].max() <= 20 and np.all(p["oy"] == 0)


# -- the stream's index arithmetic ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,batch,num", [(0, 8, 100), (17, 4, 64), (5, 3, 1), (0, 8, 0), (3, 5, 39)])
def test_ranks_of_a_world_produce_the_batches_of_world_one(first, batch, num):
    from gan_segmentation_amd import augment
    whole = list(augment.stream_batches(first, batch, num))
    assert sum(s for _, s in whole) == num
    assert [f for f, _ in whole] == [first + k * batch for k in range(len(whole))]
    assert all(s == batch for _, s in whole[:-1]) and (not whole or 1 <= whole[-1][1] <= batch)
    for world in (2, 4):
        parts = [list(augment.stream_batches(first, batch, num, rank=r, world=world)) for r in range(world)]
        assert sorted(b for part in parts for b in part) == whole           # each batch once, the short last one included
        for r, part in enumerate(parts):
            assert part == whole[r::world]


def test_endless_stream_and_bad_arguments():
    import itertools
    from gan_segmentation_amd import augment
    got = list(itertools.islice(augment.stream_batches(10, 4, None, rank=1, world=3), 4))
    assert got == [(14, 4), (26, 4), (38, 4), (50, 4)]
    for kw in (dict(batch=0), dict(batch=4, rank=2, world=2), dict(batch=4, world=0), dict(batch=4, rank=-1), dict(batch=4, num_samples=-1),
               dict(batch=4, first_index=-1)):
        with pytest.raises(ValueError):
            augment.stream_batches(kw.pop("first_index", 0), **kw)


# -- the C ABI and the keyword validation --------------------------------------------------------------------------------------
def test_augment_header_symbols_are_exported(hip_library):
    """include/gsa_augment.h declares the one entry; bad arguments are GSA_ERR_INVALID before any device work."""
    from gan_segmentation_amd._lib import load_library
    from tests.common import header_declarations
    assert set(header_declarations("gsa_augment.h")[1]) == {"gsa_augment_pairs"}
    fn = load_library().fn("gsa_augment_pairs")
    buf = np.zeros(64, np.float32)          # stands in for every pointer: no argument set below gets as far as a launch
    p = buf.ctypes.data
    good = dict(n=1, H=8, W=8, C=3, img=p, mask=p, m=p, scale=p, bias=p, oh=8, ow=8, bf=0, ignore=255, out=p, label=p)

    def call(**kw):
        a = dict(good, **kw)
        return fn(None, a["n"], a["H"], a["W"], a["C"], a["img"], a["mask"], a["m"], a["scale"], a["bias"], a["oh"], a["ow"], a["bf"],
                  a["ignore"], a["out"], a["label"])
    for bad in (dict(C=5), dict(C=0), dict(n=-1), dict(H=0), dict(W=0), dict(W=(1 << 24) + 1), dict(oh=6), dict(ow=0), dict(ow=10),
                dict(bf=2), dict(ignore=256), dict(ignore=-1), dict(img=None), dict(mask=None), dict(m=None), dict(scale=None),
                dict(bias=None), dict(out=None), dict(label=None), dict(out=p + 4), dict(label=p + 1), dict(bf=1, out=p + 4),
                dict(H=1 << 16, W=1 << 16)):
        assert call(**bad) == -1, bad
    assert call(n=0) == 0                   # an empty batch is a successful no-op


def test_keyword_validation_comes_before_any_gpu_work():
    from gan_segmentation_amd import augment
    for crop in (482, 0, -4, 3, 480.0, "480", True):
        with pytest.raises(ValueError, match="crop"):
            augment.check_crop(crop)
        with pytest.raises(ValueError, match="crop"):
            augment.plan_matrices(0, 0, 1, 512, 512, crop)
    assert augment.check_crop(480) == 480 and augment.check_crop(np.int64(64)) == 64 and augment.check_crop(None) is None
    with pytest.raises(ValueError, match="mode"):
        augment.plan_matrices(0, 0, 1, 512, 512, 480, mode="val")
    with pytest.raises(ValueError, match="channels"):
        augment.check_shapes(512, 512, 5, 480)
    with pytest.raises(ValueError, match="multiples of 4"):
        augment.check_shapes(512, 512, 3, (480, 482))
    assert augment.check_shapes(512, 256, 3, 480) == (480, 480) and augment.check_shapes(512, 256, 1, (64, 32)) == (64, 32)
    for limits in (dict(rotation=3), dict(flip=1.5), dict(scale=1.0), dict(rotate=-1), dict(shift=-0.1)):
        with pytest.raises(ValueError):
            augment.plan_matrices(0, 0, 1, 512, 512, 480, **limits)


class _Net:
    def __init__(self, nc):
        self.nc = nc


def _bare_generator(nc=3, max_res_log2=9, downscale=1):
    """An ImageGenerator with no device behind it: whatever touches the GPU fails with AttributeError."""
    from gan_segmentation_amd.image_generator import ImageGenerator
    gen = ImageGenerator.__new__(ImageGenerator)
    gen.max_res_log2, gen.output_downscale, gen.netG, gen._decoder = max_res_log2, downscale, _Net(nc), object()
    return gen


def test_training_batches_checks_its_keywords_at_the_call():
    import torch
    for nc, kw, word in ((3, dict(crop=482), "crop"), (3, dict(mode="val"), "mode"), (5, dict(mean=(0.5,) * 5, std=(1.0,) * 5), "channels"),
                         (5, dict(mean=(0.5,) * 4, std=(1.0,) * 4), "channels"), (1, dict(), "per image channel"),
                         (3, dict(labels="int32"), "labels"), (3, dict(dtype=torch.float16), "dtype"), (3, dict(rotation=2), "limit"),
                         (3, dict(world=2, rank=2), "rank"), (3, dict(ignore_label=300), "ignore_label")):
        with pytest.raises(ValueError, match=word):
            _bare_generator(nc).training_batches(4, **kw)
    stream = _bare_generator(3).training_batches(4, crop=480, num_samples=8)       # valid: nothing runs until the first next()
    with pytest.raises(AttributeError):
        next(stream)
    gen = _bare_generator(3)
    gen._decoder = None
    with pytest.raises(RuntimeError, match="attach_decoder"):
        gen.training_batches(4)
