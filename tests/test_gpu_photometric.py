"""The photometric augmentation on the GPU (include/gsa_photometric.h gsa_photometric; photometric.photometric;
ImageGenerator.training_batches(photometric=...)): byte for byte the rule of tests/test_photometric_host.py, over ALL pixels."""
import os

import numpy as np
import pytest

from tests.test_gpu_augment import _build, _host, _same_bits
from tests.test_photometric_host import IDENTITY_W, random_images, row, rule_photometric

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The tile of csrc/gsa_photometric.hip: TILE_B bytes of a row (W * C of them) by TILE_H rows.  The seam shapes below are derived
# from it (asserted against the source text).
TILE_B, TILE_H = 256, 16


def _seam_shapes():
    """(H, W, C, n): one tile exactly and one tile plus one pixel / row, each way, for every channel count whose pixels pack a tile;
    for C = 3 the widths around the seam that splits a pixel (85 px = 255 bytes, 86 px = 258 bytes)."""
    shapes = []
    for C in (1, 2, 4):
        shapes += [(TILE_H, TILE_B // C, C, 1), (TILE_H + 1, TILE_B // C + 1, C, 2)]
    shapes += [(TILE_H, TILE_B // 3, 3, 2), (TILE_H + 1, TILE_B // 3 + 1, 3, 1), (2 * TILE_H + 1, 2 * TILE_B // 3 + 1, 3, 1)]
    return shapes


def _rows(n, seed, first):
    """Planned contrast and offsets (wide limits) with every stage on: blur sigmas spread over 0.4 .. 1.5 (the widest the plan can
    give), noise sigmas over 1 .. 9; from three samples on, sample 1 has no blur and sample 2 no noise (the kernel's two uniform
    switches, mixed inside one launch)."""
    from gan_segmentation_amd import photometric as ph
    rows = ph.photometric_plan(seed, first, n, contrast=0.4, brightness=0.2, rgb_shift=30.0)
    rows[:, 6:13] = ph.blur_weights(np.linspace(1.5, 0.4, n))
    rows[:, 5] = np.linspace(9.0, 1.0, n)
    assert (rows[:, 9] < 1).all() and (rows[:, 6] > 0).all(), "every tap of every sample counts"
    if n >= 3:
        rows[1, 6:13] = IDENTITY_W
        rows[2, 5] = 0.0
    return rows


def _run(torch, img, rows, seed, first):
    from gan_segmentation_amd import photometric as ph
    d = torch.from_numpy(img).cuda()
    out = ph.photometric(d, rows, seed, first)
    assert out.shape == d.shape and out.dtype == torch.uint8 and out.is_contiguous() and out.data_ptr() != d.data_ptr()
    got = out.cpu().numpy()
    assert np.array_equal(d.cpu().numpy(), img), "the input was written to"
    return got


def _check(torch, img, rows, seed, first, what=""):
    got, want = _run(torch, img, rows, seed, first), rule_photometric(img, rows, seed, first)
    bad = got != want
    assert not bad.any(), "%s %s: %d of %d bytes differ from the rule, first at %s (got %d, want %d)" % (
        what, img.shape, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])
    return got


@pytest.mark.parametrize("H,W,C,n", [(4, 4, 1, 1), (5, 7, 3, 2), (37, 91, 4, 3), (64, 64, 2, 1), (130, 70, 3, 3), (256, 256, 3, 8)])
def test_kernel_matches_the_rule(torch_cuda, H, W, C, n):
    """The smallest image (every tap but the centre is a reflection), odd sizes, 1..4 channels, partial tiles, several tiles each
    way, batch 8; blur, colour and noise all on."""
    img = random_images(H + W + C, n, H, W, C)
    got = _check(torch_cuda, img, _rows(n, 7, 1000), 7, 1000)
    assert not np.array_equal(got, img)


def test_the_tile_is_the_one_these_tests_assume():
    src = open(os.path.join(ROOT, "gan-segmentation_amd", "csrc", "gsa_photometric.hip")).read()
    assert "constexpr int kTileB = %d;" % TILE_B in src and "constexpr int kTileH = %d;" % TILE_H in src
    assert "const dim3 grid((unsigned)(tiles_per_sample * n)), block(kThreads);" in src      # one workgroup per tile: no grid cap to cross
    shapes = _seam_shapes()
    for C in (1, 2, 4):
        assert any(W * c == TILE_B and H == TILE_H for H, W, c, _n in shapes if c == C)
        assert any(W * c == TILE_B + c and H == TILE_H + 1 for H, W, c, _n in shapes if c == C)
    assert any(c == 3 and W * c == TILE_B - 1 for _H, W, c, _n in shapes) and any(c == 3 and W * c == TILE_B + 2 for _H, W, c, _n in shapes)


@pytest.mark.parametrize("H,W,C,n", _seam_shapes())
def test_tile_seams(torch_cuda, H, W, C, n):
    img = random_images(H * W + C, n, H, W, C)
    _check(torch_cuda, img, _rows(n, 3, 50), 3, 50)


def test_stages_alone(torch_cuda):
    """Colour only, blur only, noise only at (37, 91, 3, 3): each against the rule, and each changes the image."""
    from gan_segmentation_amd import photometric as ph
    torch = torch_cuda
    img = random_images(12, 3, 37, 91, 3)
    w = ph.blur_weights([0.4, 0.9, 1.5])
    cases = {
        "colour": np.stack([row(alpha=0.83, offset=(7.25, -11.5, 3.0, 99.0)), row(alpha=1.19, offset=(-20, 0.5, 20, 0)), row(alpha=1.0, offset=(1, 2, 3, 4))]),
        "blur": np.stack([row(w=w[k]) for k in range(3)]),
        "noise": np.stack([row(noise=s) for s in (0.5, 7.0, 30.0)]),
    }
    for what, rows in cases.items():
        got = _check(torch, img, rows, 21, 5, what)
        for k in range(3):
            assert not np.array_equal(got[k], img[k]), "%s: sample %d is unchanged" % (what, k)


def test_saturation(torch_cuda):
    """An image of 0 and 255 with alpha 1.2 and offsets +-60: both clamps, on every channel."""
    rng = np.random.default_rng(2)
    img = (rng.integers(0, 2, (2, 20, 33, 4)) * 255).astype(np.uint8)
    rows = np.stack([row(alpha=1.2, offset=(60, -60, 60, -60)), row(alpha=1.2, offset=(-60, 60, -60, 60))])
    got = _check(torch_cuda, img, rows, 0, 0)
    assert np.array_equal(got[0, ..., 0], np.where(img[0, ..., 0] == 0, 60, 255)) and np.array_equal(got[0, ..., 1], np.where(img[0, ..., 1] == 0, 0, 246))


def test_zero_limits_return_the_input_bytes(torch_cuda):
    from gan_segmentation_amd import photometric as ph
    for shape in ((2, 37, 91, 3), (1, 64, 64, 4), (3, 4, 5, 1)):
        img = random_images(5, *shape)
        rows = ph.photometric_plan(8, 70, shape[0], **ph.ZERO_LIMITS)
        assert np.array_equal(_run(torch_cuda, img, rows, 8, 70), img)


def test_high_counter_and_key_words(torch_cuda):
    """first_index = 2^33 + 5 and seed = 2^40 + 3: the high counter word and the high key word are not zero, and each matters."""
    img = random_images(4, 2, 21, 30, 3)
    seed, first = 2 ** 40 + 3, 2 ** 33 + 5
    rows = _rows(2, seed, first)
    got = _check(torch_cuda, img, rows, seed, first)
    assert not np.array_equal(got, _run(torch_cuda, img, rows, seed & 0xFFFFFFFF, first)), "the high key word does not reach the noise"
    assert not np.array_equal(got, _run(torch_cuda, img, rows, seed, first & 0xFFFFFFFF)), "the high counter word does not reach the noise"


def test_four_samples_equal_one_plus_three(torch_cuda):
    from gan_segmentation_amd import photometric as ph
    torch = torch_cuda
    img = random_images(6, 4, 40, 52, 3)
    rows = ph.photometric_plan(13, 200, 4, blur_prob=1.0, noise_prob=1.0)
    whole = _check(torch, img, rows, 13, 200)
    parts = np.concatenate([_run(torch, img[:1], rows[:1], 13, 200), _run(torch, img[1:], rows[1:], 13, 201)])
    assert np.array_equal(parts, whole)
    dev_rows = torch.from_numpy(rows).cuda()
    assert np.array_equal(ph.photometric(torch.from_numpy(img).cuda(), dev_rows, 13, 200).cpu().numpy(), whole), "a device tensor of rows"
    empty = ph.photometric(torch.from_numpy(img[:0]).cuda(), rows[:0], 13, 200)
    assert empty.shape == (0, 40, 52, 3) and empty.dtype == torch.uint8


def test_value_errors(torch_cuda):
    from gan_segmentation_amd import photometric as ph
    torch = torch_cuda
    d = torch.from_numpy(random_images(1, 2, 8, 8, 3)).cuda()
    rows = ph.photometric_plan(0, 0, 2)
    for bad in (dict(img=d.float()), dict(img=d[:, :, ::2]), dict(img=d.cpu()), dict(img=d[0]), dict(params=rows[:1]), dict(params=rows[:, :6]),
                dict(params=torch.from_numpy(rows)), dict(params=torch.from_numpy(rows).cuda().double()), dict(params=None),
                dict(img=d[:, :3]), dict(img=torch.zeros((1, 8, 8, 5), dtype=torch.uint8, device="cuda"), params=rows[:1])):
        with pytest.raises(ValueError):
            ph.photometric(**dict(dict(img=d, params=rows, seed=0, first_index=0), **bad))


# ---- the stream --------------------------------------------------------------------------------------------------------------
LIMITS = dict(contrast=0.3, brightness=0.15, rgb_shift=25.0, blur_prob=0.7, blur_sigma=1.3, noise_prob=0.7, noise_sigma=9.0)


@pytest.fixture(scope="module")
def streams(torch_cuda):
    """Seven global samples (indices 10..16, seed 4, crop 96) of the reduced generator (128 px pairs) through every stream the
    tests below compare, drawn once."""
    gen = _build("reduced", 3)
    kw = dict(crop=96, seed=4, first_index=10, num_samples=7)

    def draw(batch, **more):
        return [(_host(image, label), first) for image, label, first in gen.training_batches(batch, **dict(kw, **more))]

    return dict(gen=gen, kw=kw, plain=draw(3), none=draw(3, photometric=None), on=draw(3, photometric=LIMITS),
                on_q95=draw(3, photometric=LIMITS, jpeg_quality=95), default=draw(3, photometric=True),
                world=[draw(3, photometric=LIMITS, rank=r, world=2) for r in (0, 1)])


def _by_hand(torch, gen, first, n, limits, jpeg_quality=None):
    from gan_segmentation_amd import augment, jpeg
    from gan_segmentation_amd import photometric as ph
    img, mask = gen.generate_indexed(first, n, seed=4)
    if jpeg_quality is not None:
        img = jpeg.roundtrip(img, jpeg_quality)
    rows = ph.photometric_plan(4, first, n, **limits)
    changed = ph.photometric(img, rows, 4, first)
    assert np.array_equal(changed.cpu().numpy(), rule_photometric(img.cpu().numpy(), rows, 4, first)), "the kernel on generated pixels"
    matrices = augment.plan_matrices(4, first, n, 128, 128, 96, "train")
    return _host(*augment.augment_pairs(changed, mask, matrices, augment.output_size(128, 128, 96)))


@pytest.mark.parametrize("name,limits,quality", [("on", LIMITS, None), ("on_q95", LIMITS, 95), ("default", {}, None)])
def test_stream_is_the_hand_composition(torch_cuda, streams, name, limits, quality):
    """training_batches(photometric=...) == generate_indexed -> [jpeg.roundtrip] -> photometric -> augment_pairs, and it differs
    from the plain stream in the image only."""
    got = streams[name]
    assert [f for _, f in got] == [10, 13, 16]
    for ((image, label), first), ((image0, label0), _f) in zip(got, streams["plain"]):
        want, want_label = _by_hand(torch_cuda, streams["gen"], first, min(3, 17 - first), limits, quality)
        _same_bits(image, want, "%s: image of batch %d" % (name, first))
        _same_bits(label, want_label, "%s: label of batch %d" % (name, first))
        _same_bits(label, label0, "%s: the mask must not change" % name)
        assert not np.array_equal(image, image0), "%s: batch %d equals the plain stream" % (name, first)


def test_none_is_the_stream_without_the_keyword(streams):
    for ((image, label), first), ((image0, label0), first0) in zip(streams["none"], streams["plain"]):
        assert first == first0
        _same_bits(image, image0, "image of batch %d" % first)
        _same_bits(label, label0, "label of batch %d" % first)


def test_world_two_equals_world_one(streams):
    whole = {first: pair for pair, first in streams["on"]}
    parts = {}
    for rank in (0, 1):
        for pair, first in streams["world"][rank]:
            assert first not in parts
            parts[first] = pair
    assert sorted(parts) == sorted(whole) == [10, 13, 16]
    assert [f for _, f in streams["world"][0]] == [10, 16] and [f for _, f in streams["world"][1]] == [13]
    for first in whole:
        _same_bits(parts[first][0], whole[first][0], "image of batch %d" % first)
        _same_bits(parts[first][1], whole[first][1], "label of batch %d" % first)


def test_keyword_is_checked_before_any_gpu_work(streams):
    gen = streams["gen"]
    for bad in (dict(photometric=dict(hue=0.1)), dict(photometric=dict(blur_sigma=2.0)), dict(photometric=False), dict(photometric=1),
                dict(photometric=LIMITS, hue=0.1), dict(contrast=0.2)):
        with pytest.raises(ValueError):
            gen.training_batches(3, **dict(streams["kw"], **bad))
