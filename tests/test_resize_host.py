"""Host-side checks of the pair resize (csrc/gsa_resize.h, resize_ops.py, the OUTPUT_SIZE keys): the rule's
weights against a brute-force statement, the two forms of tests/resize_ref.py against each other, the vote's ties by hand, and every
argument check, which must answer before any GPU work."""
import numpy as np
import pytest

from gan_segmentation_amd import resize_ops
from gan_segmentation_amd.resize_ops import axis_weights, check_mask_mode, check_size, resize_pair
from tests import resize_ref as ref
from tests.test_downscale_host import _ModelLoaded, _config, no_models  # noqa: F401  (no_models is a fixture)


# ---- axis_weights -----------------------------------------------------------------------------------------------------------------
def test_axis_weights_are_the_overlaps_counted_one_by_one():
    """Cut both axes into L * l unit cells: a(i, y) is the number of cells that lie in source pixel y and in output pixel i."""
    for L in range(1, 41):
        for l in range(1, L + 1):
            brute = np.zeros((l, L), np.int64)
            for cell in range(L * l):
                brute[cell // L, cell // l] += 1
            assert np.array_equal(axis_weights(L, l), brute), (L, l)


@pytest.mark.parametrize("L,l", [(1, 1), (7, 7), (8, 4), (9, 4), (47, 16), (300, 19), (64, 4), (100, 37), (259, 65), (1024, 384), (512, 384)])
def test_axis_weights_sums_taps_and_identity(L, l):
    a = axis_weights(L, l)
    assert a.dtype == np.int64 and a.shape == (l, L) and (a >= 0).all()
    assert (a.sum(axis=1) == L).all() and (a.sum(axis=0) == l).all()
    i = np.arange(l)
    first, last = i * L // l, ((i + 1) * L - 1) // l
    y = np.arange(L)[None, :]
    assert np.array_equal(a > 0, (y >= first[:, None]) & (y <= last[:, None])), "non-zero exactly between the rule's first and last tap"
    assert ((a > 0).sum(axis=1) <= -(-L // l) + 1).all()
    if l == L:
        assert np.array_equal(a, L * np.eye(L, dtype=np.int64))


@pytest.mark.parametrize("bad", [(4, 5), (4, 0), (0, 0), (4, -1), (4.0, 2), (True, 1)])
def test_axis_weights_refuses(bad):
    with pytest.raises(ValueError):
        axis_weights(*bad)


@pytest.mark.parametrize("shape,size", ref.SHAPES)
def test_matrix_form_is_the_repeat_form(shape, size):
    """Two statements of the same sums, on random images and on the nine slot planes of random masks; and so of the outputs."""
    H, W = shape
    img, mask = ref.random_pair(H * W, 2, H, W, 3)
    planes = np.moveaxis(img, -1, 1)
    assert np.array_equal(ref.weighted_sums(planes, *size), ref.repeat_sums(planes, *size))
    slots = ref.slot_planes(mask)
    assert np.array_equal(ref.weighted_sums(slots, *size), ref.repeat_sums(slots, *size))
    assert np.array_equal(ref.weighted_sums(planes, *size), ref.prefix_sums(planes, *size))
    assert np.array_equal(ref.weighted_sums(slots, *size), ref.prefix_sums(slots, *size))
    assert np.array_equal(ref.resize_image(img, size), ref.resize_image(img, size, sums=ref.repeat_sums))
    assert np.array_equal(ref.resize_mask(mask, size), ref.resize_mask(mask, size, sums=ref.repeat_sums))


def test_identity_and_constant_planes():
    img, mask = ref.random_pair(3, 2, 7, 5, 4, values=(0, 1, 7))
    assert np.array_equal(ref.resize_image(img, (7, 5)), img)
    assert np.array_equal(ref.resize_mask(mask, (7, 5)), mask)
    assert np.array_equal(ref.resize_mask(mask, (7, 5), "nearest"), mask)
    for v in (0, 1, 127, 254, 255):
        assert (ref.resize_image(np.full((1, 33, 47, 2), v, np.uint8), (16, 16)) == v).all()


def test_image_rounds_half_up():
    img = np.asarray([[[[0], [1]], [[1], [0]]]], np.uint8)             # mean 0.5 -> 1
    assert ref.resize_image(img, (1, 1)).tolist() == [[[[1]]]]
    img = np.asarray([[[[0], [1]], [[0], [0]]]], np.uint8)             # mean 0.25 -> 0
    assert ref.resize_image(img, (1, 1)).tolist() == [[[[0]]]]
    img = np.asarray([[[[10], [11], [13]]]], np.uint8)                  # 3 -> 2: (2 * 10 + 11) / 3 = 10.33, (11 + 2 * 13) / 3 = 12.33
    assert ref.resize_image(img, (1, 2)).tolist() == [[[[10], [12]]]]


# ---- the vote ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(ref.hand_cases())))
def test_vote_by_hand(k):
    mask, size, want = ref.hand_cases()[k]
    assert np.array_equal(ref.resize_mask(mask, size), want)
    assert np.array_equal(ref.resize_mask(mask, size, sums=ref.repeat_sums), want)


def test_vote_maps_values_from_8_up_to_255_and_nearest_passes_them():
    mask = ref.every_value_mask(1, 1, 12, 18)
    assert set(np.unique(ref.resize_mask(mask, (12, 18))).tolist()) <= set(range(8)) | {255}
    assert np.array_equal(ref.resize_mask(mask, (12, 18)), np.where(mask >= 8, 255, mask))
    assert np.array_equal(ref.resize_mask(mask, (12, 18), "nearest"), mask)
    near = ref.resize_mask(mask, (5, 7), "nearest")
    assert all(near[0, i, j] == mask[0, i * 12 // 5, j * 18 // 7] for i in range(5) for j in range(7))


# ---- argument checks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [True, 4.0, 0, -4, 65, (4, 65), (65, 4), 3, (3, 8), (8, 3), (8,), (8, 8, 8), "8", None, (8.0, 8), (True, 8), [8, "8"]])
def test_check_size_refuses(size):
    """On a 64 x 64 source: a bool, a float, zero, larger than the source, less than 1/16 of it, a wrong length."""
    with pytest.raises(ValueError, match="the_name"):
        check_size(size, 64, 64, "the_name")


def test_check_size_accepts():
    assert check_size(4, 64, 64) == (4, 4) and check_size(64, 64, 64) == (64, 64)
    assert check_size((4, 64), 64, 64) == (4, 64) and check_size([48, 16], 64, 128) == (48, 16)
    assert check_size(np.int64(7), 100, 100) == (7, 7)
    assert check_size((4096, 16), 65535, 256) == (4096, 16)


@pytest.mark.parametrize("mode", ["bilinear", "VOTE", 0, 1, None, True, b"vote"])
def test_check_mask_mode_refuses(mode):
    with pytest.raises(ValueError, match="mask_mode"):
        check_mask_mode(mode)


def test_check_mask_mode_and_the_header_macros():
    import os
    import re
    from gan_segmentation_amd import _lib
    assert (check_mask_mode("vote"), check_mask_mode("nearest")) == (0, 1)
    text = open(os.path.join(os.path.dirname(_lib.HIP_LIBRARY), "gsa_resize.h")).read()
    macros = dict(re.findall(r"#define\s+(GSA_RESIZE_[A-Z_]+)[ \t]+(\d+)", text))
    assert macros == {"GSA_RESIZE_VOTE": "0", "GSA_RESIZE_NEAREST": "1", "GSA_RESIZE_MAX_RATIO": "16", "GSA_RESIZE_MAX_PIXELS": str(1 << 24)}
    assert (resize_ops.RESIZE_VOTE, resize_ops.RESIZE_NEAREST, resize_ops.RESIZE_MAX_RATIO, resize_ops.RESIZE_MAX_PIXELS) == (0, 1, 16, 1 << 24)
    flat = " ".join(text.replace(" * ", " ").split())
    assert "every input value 8..254 comes out as 255" in flat
    assert "8..254 comes out as 255" in " ".join(resize_pair.__doc__.split())


def test_resize_pair_refuses_before_any_gpu_work():
    """None / None, a CPU tensor, a wrong dtype, a non-contiguous tensor, a mismatched n: ValueError, with no device in sight."""
    import torch
    img, mask = torch.zeros((2, 8, 8, 3), dtype=torch.uint8), torch.zeros((2, 8, 8), dtype=torch.uint8)
    bad = [dict(), dict(img=None, mask=None), dict(img=img), dict(mask=mask), dict(img=img, mask=mask),
           dict(img=img.float()), dict(mask=mask.to(torch.int8)), dict(img=img[:, :, ::2]), dict(mask=mask[:, ::2]),
           dict(img=img.numpy()), dict(mask=mask.numpy()), dict(img=img, mask=mask[:1]), dict(img=img[..., 0]), dict(mask=mask[0])]
    for kw in bad:
        with pytest.raises(ValueError):
            resize_pair(size=4, **kw)


# ---- the config keys ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys,name", [({"OUTPUT_SIZE": 100}, "OUTPUT_SIZE"), ({"OUTPUT_SIZE": 8}, "OUTPUT_SIZE"), ({"OUTPUT_SIZE": 0}, "OUTPUT_SIZE"),
                                       ({"OUTPUT_SIZE": 272}, "OUTPUT_SIZE"), ({"OUTPUT_SIZE": [128, 272]}, "OUTPUT_SIZE"),
                                       ({"OUTPUT_SIZE": 144, "OUTPUT_DOWNSCALE": 2}, "OUTPUT_SIZE"), ({"OUTPUT_SIZE": [128]}, "OUTPUT_SIZE"),
                                       ({"OUTPUT_SIZE": 128.0}, "OUTPUT_SIZE"), ({"OUTPUT_SIZE": True}, "OUTPUT_SIZE"),
                                       ({"OUTPUT_SIZE": "128"}, "OUTPUT_SIZE"), ({"OUTPUT_SIZE": [128, 100]}, "OUTPUT_SIZE"),
                                       ({"OUTPUT_SIZE": 128, "OUTPUT_MASK_RESIZE": "bilinear"}, "OUTPUT_MASK_RESIZE"),
                                       ({"OUTPUT_MASK_RESIZE": "bilinear"}, "OUTPUT_MASK_RESIZE"), ({"OUTPUT_MASK_RESIZE": 1}, "OUTPUT_MASK_RESIZE")])
def test_cli_rejects_a_bad_key_before_loading_a_model(tmp_path, no_models, keys, name):
    """bedrooms is 256 px: not a multiple of 16, 8, larger than R / f, and an unknown mask filter."""
    from gan_segmentation_amd import main as cli
    with pytest.raises(ValueError, match=name):
        cli.main(["generate", "--config", _config(tmp_path, **keys)])


def test_output_size_ratio_limit():
    """No generator here is larger than 1024 px, so 16 px -- the least the encoders take -- is within 1/16 of R / f only from 256 px down:
    the ratio limit is checked on the function the CLI calls."""
    assert resize_ops.check_output_size(16, 256) == (16, 16)
    for side in (512, 1024):
        with pytest.raises(ValueError, match="OUTPUT_SIZE"):
            resize_ops.check_output_size(16, side)
        with pytest.raises(ValueError, match="OUTPUT_SIZE"):
            resize_ops.check_output_size([side, 16], side)
    assert resize_ops.check_output_size(None, 1024) is None
    assert resize_ops.check_output_size([384, 640], 1024) == (384, 640)


def test_cli_accepts_the_keys_and_their_absence(tmp_path, no_models):
    from gan_segmentation_amd import main as cli
    for keys in ({}, {"OUTPUT_SIZE": None}, {"OUTPUT_SIZE": 256}, {"OUTPUT_SIZE": 16}, {"OUTPUT_SIZE": [96, 112]},
                 {"OUTPUT_SIZE": 96, "OUTPUT_DOWNSCALE": 2, "OUTPUT_MASK_RESIZE": "nearest"}, {"OUTPUT_MASK_RESIZE": "vote"},
                 {"OUTPUT_SIZE": 128, "OUTPUT_MASK_RESIZE": "vote", "MASK_MORPH": True, "PAIR_STATS": True}):
        with pytest.raises(_ModelLoaded):
            cli.main(["generate", "--config", _config(tmp_path, **keys)])
    doc = cli.__doc__
    assert "OUTPUT_SIZE" in doc and "OUTPUT_MASK_RESIZE" in doc
