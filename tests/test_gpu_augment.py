"""The training stream on the GPU (include/gsa_augment.h gsa_augment_pairs; augment.augment_pairs;
ImageGenerator.training_batches): bit for bit the rule of tests/test_augment_host.py, over ALL output pixels, image and label."""
import numpy as np
import pytest

from tests.common import gan_setup, lively, odd_setup, reduced_setup
from tests.test_augment_host import random_pair, rule_augment

pytestmark = pytest.mark.gpu


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s vs %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    a = got.view(np.uint32) if got.dtype == np.float32 else got
    b = want.view(np.uint32) if want.dtype == np.float32 else want
    assert np.array_equal(a, b), "%s: %d of %d values differ" % (what, int((a != b).sum()), a.size)


def _host(image, label):
    """Device results -> (fp32 image, label) numpy arrays; a bf16 image widens exactly."""
    return image.float().cpu().numpy(), label.cpu().numpy()


def _norm(C):
    from gan_segmentation_amd import augment
    mean, std = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
    return augment.normalisation(mean[:C], std[:C])


def _check_kernel(torch, img, mask, matrices, out_size, ignore=255):
    """augment_pairs == rule_augment in fp32 and in bf16 (the RNE rounding of the rule's fp32) on these inputs."""
    from gan_segmentation_amd import augment
    scale, bias = _norm(img.shape[-1])
    di, dm = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()
    want, want_label = rule_augment(img, mask, matrices, out_size, scale, bias, ignore=ignore)
    want_bf, _ = rule_augment(img, mask, matrices, out_size, scale, bias, ignore=ignore, bf16=True)
    for dtype, w in ((torch.float32, want), (torch.bfloat16, want_bf)):
        image, label = augment.augment_pairs(di, dm, matrices, out_size, scale=scale, bias=bias, dtype=dtype, ignore_label=ignore)
        assert image.dtype == dtype and label.dtype == torch.uint8 and image.is_contiguous() and label.is_contiguous()
        got, got_label = _host(image, label)
        _same_bits(got, w, "image %s" % dtype)
        _same_bits(got_label, want_label, "label %s" % dtype)
    return want, want_label


@pytest.mark.parametrize("H,W,C,n,crop,mode", [
    (512, 512, 3, 8, 480, "train"), (512, 512, 3, 3, 480, "center"), (512, 512, 1, 1, 480, "train"),
    (1024, 1024, 3, 3, 480, "train"), (1024, 1024, 3, 1, None, "train"), (1024, 1024, 1, 1, 480, "center"),
    (256, 256, 3, 8, 480, "train"), (256, 256, 1, 3, 480, "center"), (256, 256, 3, 1, 480, "center"),
    (300, 500, 3, 3, 480, "train"), (500, 300, 1, 8, 480, "train"), (37, 91, 4, 3, 64, "train"), (64, 64, 2, 1, None, "train")])
def test_kernel_matches_the_rule(torch_cuda, H, W, C, n, crop, mode):
    """Seeded random u8 pairs through planned matrices: 512 -> 480 (train and centre), 1024 -> 480 and -> 1024, 256 -> 480
    (padding), non-square sources, 1..4 channels, batch 1, 3 and 8, fp32 and bf16 output."""
    from gan_segmentation_amd import augment
    img, mask = random_pair(100 + H + C + n, n, H, W, C, classes=5)
    matrices = augment.plan_matrices(7, 1000, n, H, W, crop, mode)
    out_size = augment.output_size(H, W, crop)
    image, label = _check_kernel(torch_cuda, img, mask, matrices, out_size)
    if crop is not None and (H < crop or W < crop):
        assert np.any(label == 255) and np.any(label != 255), "a padded canvas must hold both source and border pixels"


def test_kernel_on_hand_made_matrices(torch_cuda):
    """Identity, mirror, half-pixel shifts, a zoom, a quarter turn, and coordinates far outside (which must not wrap), one per
    sample; another ignore label."""
    H, W = 64, 96
    rows = np.array([[1, 0, 0, 0, 1, 0], [-1, 0, W - 1, 0, 1, 0], [1, 0, 0.5, 0, 1, 0.5], [1, 0, -0.5, 0, 1, 2.5],
                     [0.37, 0, 3.25, 0, 0.41, -7.75], [0, -1, 80.5, 1, 0, -10.25], [1, 0, 3e9, 0, 1, 0], [1, 0, 0, 0, 1, -3e38],
                     [1, 0, 2.0 ** 32, 0, 1, 2.0 ** 31], [4.0e7, 0, -1.0e7, 0, 1, 0]], np.float32)
    img, mask = random_pair(5, len(rows), H, W, 3)
    image, label = _check_kernel(torch_cuda, img, mask, rows, (64, 96), ignore=7)
    assert np.array_equal(label[0], mask[0]) and np.array_equal(label[1], mask[1][:, ::-1])
    assert np.all(label[6:9] == 7)


def _setup(kind, batch):
    if kind == "reduced":
        gcfg, gp, dcfg, dp, _z, _noise = reduced_setup(7, batch=batch)
    elif kind == "odd":
        gcfg, gp, dcfg, dp, _z, _noise = odd_setup(batch)
    else:
        gcfg, gp, dcfg, dp, _z, _noise = gan_setup(kind, batch)
    return gcfg, lively(gp), dcfg, dp


def _build(kind, batch, **kw):
    from gan_segmentation_amd.image_generator import ImageGenerator
    gcfg, gp, dcfg, dp = _setup(kind, batch)
    return ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=batch, **kw)


def _expected(gen, first, n, seed, crop, mode, bf16=False, **limits):
    """rule_augment on generate_indexed of the same indices, with the plan of the same seed."""
    from gan_segmentation_amd import augment
    img, mask = [t.cpu().numpy() for t in gen.generate_indexed(first, n, seed=seed)]
    R = img.shape[1]
    scale, bias = augment.normalisation()
    matrices = augment.plan_matrices(seed, first, n, R, R, crop, mode, **limits)
    return rule_augment(img, mask, matrices, augment.output_size(R, R, crop), scale, bias, bf16=bf16)


def _check_stream(gen, batch, crop, mode, seed, first_index, num_samples, dtype=None, **limits):
    import torch
    kw = dict(limits)
    if dtype is not None:
        kw["dtype"] = dtype
    got = [(_host(image, label), first) for image, label, first in
           gen.training_batches(batch, crop=crop, mode=mode, seed=seed, first_index=first_index, num_samples=num_samples, **kw)]
    assert [f for _, f in got] == list(range(first_index, first_index + num_samples, batch))
    seen = 0
    for (image, label), first in got:
        n = min(batch, num_samples - (first - first_index))
        want, want_label = _expected(gen, first, n, seed, crop, mode, bf16=dtype is torch.bfloat16, **limits)
        _same_bits(image, want, "image of batch %d" % first)
        _same_bits(label, want_label, "label of batch %d" % first)
        seen += n
    assert seen == num_samples
    return got


@pytest.mark.parametrize("kind,crop,mode", [("reduced", 96, "train"), ("reduced", 160, "train"), ("reduced", 160, "center"),
                                            ("odd", 96, "train"), ("odd", None, "train")])
def test_stream_is_the_rule_on_generate_indexed(torch_cuda, kind, crop, mode):
    """The reduced and the odd-channel configurations (128 px pairs): cropped, padded, and at the pair's own size; fp32 and bf16
    batches; a short last batch."""
    gen = _build(kind, 3)
    _check_stream(gen, 3, crop, mode, seed=4, first_index=20, num_samples=7)
    _check_stream(gen, 3, crop, mode, seed=4, first_index=20, num_samples=4, dtype=torch_cuda.bfloat16, rotate=30, shift=0.2)


def test_stream_on_ffhq_downscaled(torch_cuda):
    """FFHQ with output_downscale=2 and crop 480: the reference's experiment."""
    gen = _build("ffhq", 2, output_downscale=2)
    got = _check_stream(gen, 2, 480, "train", seed=1, first_index=6, num_samples=3)
    (image, label), _first = got[0]
    assert image.shape == (2, 3, 480, 480) and label.shape == (2, 480, 480)
    _check_stream(gen, 2, 480, "center", seed=1, first_index=6, num_samples=2)


def test_stream_with_style_mixing_and_bf16_precision(torch_cuda):
    gen = _build("reduced", 4, style_mix_prob=1.0)
    _check_stream(gen, 4, 96, "train", seed=9, first_index=0, num_samples=6)
    plain = _build("reduced", 4)
    a = gen.generate_indexed(0, 4, seed=9)[0].cpu().numpy()
    b = plain.generate_indexed(0, 4, seed=9)[0].cpu().numpy()
    assert not np.array_equal(a, b), "style mixing changed nothing: the case does not test the mixed path"
    _check_stream(_build("reduced", 4, precision="bf16"), 4, 96, "train", seed=9, first_index=0, num_samples=4)


def test_stream_leaves_the_dataset_path_alone(torch_cuda):
    """generate_indexed returns the same pair before and after a stream was drawn from the same ImageGenerator."""
    gen = _build("reduced", 3)
    before = [t.cpu().numpy() for t in gen.generate_indexed(5, 3, seed=2)]
    for _ in gen.training_batches(3, crop=96, seed=2, first_index=0, num_samples=9):
        pass
    after = [t.cpu().numpy() for t in gen.generate_indexed(5, 3, seed=2)]
    _same_bits(after[0], before[0], "image")
    _same_bits(after[1], before[1], "mask")
    assert before[0].shape == (3, 128, 128, 3)


def test_world_two_equals_world_one_and_int64_labels(torch_cuda):
    """Ranks 0 and 1 of world 2 together yield the batches of world 1, sample for sample; labels="int64" has -1 exactly where
    the u8 labels have 255 and the same class everywhere else."""
    import torch
    gen = _build("reduced", 2)
    kw = dict(crop=160, seed=3, first_index=10, num_samples=9)
    whole = {first: _host(image, label) for image, label, first in gen.training_batches(2, **kw)}
    assert sorted(whole) == [10, 12, 14, 16, 18] and whole[18][0].shape[0] == 1
    parts = {}
    for rank in (0, 1):
        for image, label, first in gen.training_batches(2, rank=rank, world=2, **kw):
            assert first not in parts
            parts[first] = _host(image, label)
    assert sorted(parts) == sorted(whole)
    for first in whole:
        _same_bits(parts[first][0], whole[first][0], "image of batch %d" % first)
        _same_bits(parts[first][1], whole[first][1], "label of batch %d" % first)
    wide = {first: (image, label) for image, label, first in gen.training_batches(2, labels="int64", **kw)}
    for first in whole:
        image, label = wide[first]
        assert label.dtype == torch.int64
        l64, l8 = label.cpu().numpy(), whole[first][1]
        assert np.any(l8 == 255)
        assert np.array_equal(l64 == -1, l8 == 255)
        assert np.array_equal(l64[l8 != 255], l8[l8 != 255].astype(np.int64))
        _same_bits(image.cpu().numpy(), whole[first][0], "image of the int64 batch %d" % first)


def test_yielded_tensors_are_the_consumer_s_to_keep(torch_cuda):
    """Every batch comes in tensors of its own: holding all of them changes none."""
    gen = _build("reduced", 2)
    held = list(gen.training_batches(2, crop=96, seed=5, num_samples=8))
    ptrs = {t.data_ptr() for image, label, _ in held for t in (image, label)}
    assert len(ptrs) == 2 * len(held)
    for image, label, first in held:
        want, want_label = _expected(gen, first, 2, 5, 96, "train")
        _same_bits(image.cpu().numpy(), want, "held image %d" % first)
        _same_bits(label.cpu().numpy(), want_label, "held label %d" % first)
