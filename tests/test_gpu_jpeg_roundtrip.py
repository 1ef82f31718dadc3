"""The JPEG round trip on the GPU (include/gsa_jpeg_roundtrip.h gsa_jpeg_roundtrip; jpeg.roundtrip;
ImageGenerator.training_batches(jpeg_quality=...)): bit for bit the rule of tests/test_jpeg_roundtrip_host.py, over ALL pixels."""
import io
import os

import numpy as np
import pytest

from tests.test_gpu_augment import _build, _host, _same_bits
from tests.test_jpeg_roundtrip_host import checker, noise, rule_roundtrip, saturated, smooth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pictures(n, H, W, seed):
    """n pairwise different pictures: smooth ones (each with its own phase and noise), white noise, saturated noise, the checker."""
    out = []
    for i in range(n):
        kind = i % 4
        if kind == 0:
            rng = np.random.default_rng([seed, i])
            img = (np.roll(smooth(H, W), i * 5 + 1, axis=1).astype(np.int64) + rng.integers(-6, 7, (H, W, 3))).clip(0, 255).astype(np.uint8)
        elif kind == 1:
            img = noise(seed * 1000 + i, H, W)
        elif kind == 2:
            img = saturated(seed * 1000 + i, H, W)
        else:
            img = np.roll(checker(H, W), i // 4, axis=1)
            img[:, :, 0] = np.random.default_rng([seed, i]).integers(0, 256, (H, W))       # a checker with a noisy red channel
        out.append(np.ascontiguousarray(img))
    assert len({a.tobytes() for a in out}) == n, "the pictures of a batch must all differ"
    return np.stack(out)


def _roundtrip(torch, batch, quality):
    from gan_segmentation_amd import jpeg
    d = torch.from_numpy(batch).cuda()
    out = jpeg.roundtrip(d, quality)
    assert out.shape == d.shape and out.dtype == torch.uint8 and out.is_contiguous() and out.data_ptr() != d.data_ptr()
    got = out.cpu().numpy()
    assert np.array_equal(d.cpu().numpy(), batch), "the input was written to"
    return got


def _check(torch, batch, quality):
    got, want = _roundtrip(torch, batch, quality), rule_roundtrip(batch, quality)
    bad = got != want
    assert not bad.any(), "q%d %s: %d of %d bytes differ from the rule, first at %s" % (
        quality, batch.shape, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))
    return got


@pytest.mark.parametrize("n,H,W", [(1, 16, 16),      # one MCU: all four image edges of the upsampler in one block
                                   (1, 16, 64),      # one MCU high, interior MCU borders along the row
                                   (1, 64, 16)])     # one MCU wide, interior MCU borders down the column
def test_single_image_edges_and_mcu_borders(torch_cuda, n, H, W):
    _check(torch_cuda, noise(H + W, H, W)[None], 95)
    _check(torch_cuda, smooth(H, W)[None], 95)


def test_images_of_a_batch_do_not_leak_into_each_other(torch_cuda):
    """n=3, 32x32, three different images: interior borders both ways; the chroma rows above image 1 belong to image 0 and those
    below to image 2 in the workspace, and must not be read."""
    batch = np.stack([noise(11, 32, 32), saturated(12, 32, 32), smooth(32, 32)])
    got = _check(torch_cuda, batch, 95)
    alone = _roundtrip(torch_cuda, batch[1:2], 95)
    assert np.array_equal(got[1], alone[0]), "image 1 of the batch differs from the round trip of image 1 alone"


@pytest.mark.parametrize("quality", [75, 95, 100])
def test_a_batch_whose_mcu_count_is_no_multiple_of_the_workgroup(torch_cuda, quality):
    """n=5, 48x80: 75 MCUs, the last workgroup has one active wave of four."""
    assert (5 * 3 * 5) % 4
    _check(torch_cuda, pictures(5, 48, 80, quality), quality)


@pytest.mark.parametrize("quality", [100, 50])
def test_extreme_inputs_clamps_and_int32_headroom(torch_cuda, quality):
    """The 1-px checker and saturated noise at 32x32 against the int64 rule: the largest coefficients and the values furthest
    outside 0..255 the decoder meets."""
    batch = np.stack([checker(32, 32), saturated(21, 32, 32), 255 - checker(32, 32), saturated(22, 32, 32)])
    got = _check(torch_cuda, batch, quality)
    assert got.min() == 0 and got.max() == 255


# ---- beyond one pass of the two kernels ------------------------------------------------------------------------------------------
# gsa_jpeg_roundtrip (csrc/gsa_jpeg.hip) caps stage 1 at 2048 workgroups of 4 MCUs (16x16 px) and stage 2 at 1024 workgroups of
# 256 threads x 8 px: either way one pass covers 8192 MCUs = 2 Mpx, and a larger call makes a workgroup walk on, splitting its index
# into (image, row, column) again.
ROUNDTRIP_MCUS_PER_PASS = 2048 * 4
ROUNDTRIP_PIXELS_PER_PASS = 1024 * 256 * 8


def test_the_roundtrip_grid_caps_are_the_ones_these_tests_assume():
    src = open(os.path.join(ROOT, "gan-segmentation_amd", "csrc", "gsa_jpeg.hip")).read()
    assert "const int rgrid = (total_mcus + 3) / 4 < 2048 ? (total_mcus + 3) / 4 : 2048;" in src
    assert "const int mgrid = (groups + 255) / 256 < 1024 ? (int)((groups + 255) / 256) : 1024;" in src
    assert "const long long groups = (long long)(plane / 8);" in src
    assert ROUNDTRIP_PIXELS_PER_PASS == ROUNDTRIP_MCUS_PER_PASS * 256


def test_beyond_one_pass_of_either_kernel(torch_cuda):
    """n=33 at 256x256, pairwise different pictures: 8448 MCUs, the smallest batch of that size past 8192; 64 workgroups of each
    stage take a second trip."""
    n, H, W = 33, 256, 256
    assert n * (H // 16) * (W // 16) > ROUNDTRIP_MCUS_PER_PASS >= (n - 1) * (H // 16) * (W // 16)
    assert n * H * W > ROUNDTRIP_PIXELS_PER_PASS
    batch = pictures(n, H, W, 7)
    got, want = _roundtrip(torch_cuda, batch, 95), rule_roundtrip(batch, 95)
    wrong = [i for i in range(n) if not np.array_equal(got[i], want[i])]
    assert not wrong, "images %s differ from the rule" % wrong


def test_roundtrip_equals_pillows_decode_of_the_hip_encoders_files(torch_cuda):
    """The feature's promise in one assertion: what a reader decodes from the files JpegEncoder writes == jpeg.roundtrip."""
    features = pytest.importorskip("PIL.features")
    if not features.check("jpg"):
        pytest.skip("Pillow without JPEG support")
    from PIL import Image
    from gan_segmentation_amd import jpeg
    batch = np.stack([noise(31, 32, 48), smooth(32, 48)])
    d = torch_cuda.from_numpy(batch).cuda()
    files = jpeg.JpegEncoder(2, 32, 48, "cuda:0").files(d)
    decoded = np.stack([np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files])
    assert np.array_equal(jpeg.roundtrip(d).cpu().numpy(), decoded)


def test_out_argument_and_the_empty_batch(torch_cuda):
    from gan_segmentation_amd import jpeg
    batch = pictures(2, 32, 32, 9)
    d = torch_cuda.from_numpy(batch).cuda()
    out = torch_cuda.empty_like(d)
    assert jpeg.roundtrip(d, 95, out=out) is out
    assert np.array_equal(out.cpu().numpy(), rule_roundtrip(batch, 95))
    with pytest.raises(ValueError, match="out"):
        jpeg.roundtrip(d, 95, out=d)
    assert jpeg.roundtrip(d[:0], 95).shape == (0, 32, 32, 3)
    for bad in (d[:, :, :, :2], d.float(), d[:, :24].contiguous()):
        with pytest.raises(ValueError):
            jpeg.roundtrip(bad)


# ---- the stream --------------------------------------------------------------------------------------------------------------
# The reduced synthetic generator of the augment tests: 128 px pairs, the smallest configuration there, and a multiple of 16.
def _by_hand(torch, gen, first, n, seed, crop, quality, dtype):
    from gan_segmentation_amd import augment, jpeg
    img, mask = gen.generate_indexed(first, n, seed=seed)
    R = img.shape[1]
    matrices = augment.plan_matrices(seed, first, n, R, R, crop, "train")
    coded = jpeg.roundtrip(img, quality)
    assert not torch.equal(coded, img), "the codec changed nothing: the case does not test the option"
    return _host(*augment.augment_pairs(coded, mask, matrices, augment.output_size(R, R, crop), dtype=dtype))


@pytest.fixture(scope="module")
def streams(torch_cuda):
    """Six global samples (indices 10..15, seed 4, crop 96) through every stream the tests below compare, drawn once."""
    torch = torch_cuda
    gen = _build("reduced", 3)
    assert (2 ** gen.max_res_log2 // gen.output_downscale) % 16 == 0
    kw = dict(crop=96, seed=4, first_index=10, num_samples=6)

    def draw(batch, **more):
        return [(_host(image, label), first) for image, label, first in gen.training_batches(batch, **dict(kw, **more))]

    return dict(gen=gen, plain=draw(3), none=draw(3, jpeg_quality=None), q95=draw(3, jpeg_quality=95), q95_by2=draw(2, jpeg_quality=95),
                q95_bf16=draw(3, jpeg_quality=95, dtype=torch.bfloat16))


@pytest.mark.parametrize("name,bf16", [("q95", False), ("q95_bf16", True)])
def test_stream_is_augment_of_the_roundtrip_of_generate_indexed(torch_cuda, streams, name, bf16):
    dtype = torch_cuda.bfloat16 if bf16 else torch_cuda.float32
    assert [first for _, first in streams[name]] == [10, 13]
    for (image, label), first in streams[name]:
        want, want_label = _by_hand(torch_cuda, streams["gen"], first, 3, 4, 96, 95, dtype)
        _same_bits(image, want, "image of batch %d" % first)
        _same_bits(label, want_label, "label of batch %d" % first)


def test_stream_without_the_option_is_unchanged_and_labels_agree(streams):
    for (plain, f0), (none, f1), (coded, f2) in zip(streams["plain"], streams["none"], streams["q95"]):
        assert f0 == f1 == f2
        _same_bits(none[0], plain[0], "image of batch %d, jpeg_quality=None" % f0)
        _same_bits(none[1], plain[1], "label of batch %d, jpeg_quality=None" % f0)
        _same_bits(coded[1], plain[1], "label of batch %d, jpeg_quality=95" % f0)
        assert not np.array_equal(coded[0], plain[0]), "jpeg_quality=95 changed no pixel"


def test_stream_sample_does_not_depend_on_the_batch_size(streams):
    by3 = np.concatenate([image for (image, _), _ in streams["q95"]]), np.concatenate([label for (_, label), _ in streams["q95"]])
    by2 = np.concatenate([image for (image, _), _ in streams["q95_by2"]]), np.concatenate([label for (_, label), _ in streams["q95_by2"]])
    assert [first for _, first in streams["q95_by2"]] == [10, 12, 14] and by3[0].shape[0] == 6
    _same_bits(by2[0], by3[0], "images, batch 2 vs batch 3")
    _same_bits(by2[1], by3[1], "labels, batch 2 vs batch 3")
