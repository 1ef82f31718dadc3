"""Downscaled pairs on the host side, without a GPU: the numpy restatement of the canonical rule (include/gsa.h
gsa_generate_downscaled) and the validation of the `output_downscale` keyword and the `OUTPUT_DOWNSCALE` key."""
import numpy as np
import pytest


def block_sum(a, f):
    """S_f over the last two axes: a pairwise quad tree in fp32, every add rounded."""
    a = np.asarray(a, np.float32)
    while f > 1:
        a = (a[..., 0::2, 0::2] + a[..., 0::2, 1::2]) + (a[..., 1::2, 0::2] + a[..., 1::2, 1::2])
        f //= 2
    return a


def rule_image(rgb, f):
    """rgb (N, nc, R, R) fp32 toRGB values -> (N, R/f, R/f, nc) u8: the block mean of u = 255 * clamp((v + 1) / 2, 0, 1), truncated."""
    rgb = np.asarray(rgb, np.float32)
    u = np.float32(255.0) * np.clip((rgb + np.float32(1.0)) * np.float32(0.5), np.float32(0.0), np.float32(1.0))
    m = block_sum(u, f) * np.float32(1.0 / (f * f))
    return np.ascontiguousarray(m.astype(np.uint8).transpose(0, 2, 3, 1))


def rule_mask(logits, f):
    """logits (N, K, R, R) fp32 -> (N, R/f, R/f) u8: the first maximum over classes of the block sums."""
    return block_sum(logits, f).argmax(axis=1).astype(np.uint8)


def test_factor_one_is_the_full_size_transform():
    from gan_segmentation_amd.image_generator import ImageGenerator
    rgb = np.random.default_rng(0).uniform(-1.5, 1.5, (2, 3, 16, 16)).astype(np.float32)
    want = ImageGenerator._transform_gan_back(rgb, {"imrange": (-1, 1)})
    assert np.array_equal(rule_image(rgb, 1), want)
    logits = np.random.default_rng(1).standard_normal((2, 3, 16, 16)).astype(np.float32)
    assert np.array_equal(rule_mask(logits, 1), logits.argmax(axis=1))


def test_block_sum_is_the_pairwise_quad_tree():
    a = np.random.default_rng(2).standard_normal((3, 8, 8)).astype(np.float32) * np.float32(1e4)
    s2 = block_sum(a, 2)
    assert s2.shape == (3, 4, 4)
    y, x = 1, 2
    b = a[:, 2 * y:2 * y + 2, 2 * x:2 * x + 2]
    assert np.array_equal(s2[:, y, x], (b[:, 0, 0] + b[:, 0, 1]) + (b[:, 1, 0] + b[:, 1, 1]))
    assert np.array_equal(block_sum(a, 8), block_sum(block_sum(block_sum(a, 2), 2), 2))
    # the order is part of the rule: a sequential row-major sum rounds differently on the same values
    c = np.array([[1.0, 1e8], [-1e8, 1.0]], np.float32)[None]
    assert block_sum(c, 2)[0, 0, 0] == np.float32(0.0)
    assert np.float32(np.float32(np.float32(np.float32(1.0) + np.float32(1e8)) - np.float32(1e8)) + np.float32(1.0)) == np.float32(1.0)


def test_mean_before_truncation_and_first_maximum():
    # u of the four pixels: 127.63, 127.88, 128.14, 128.39 -- their mean truncates to 128, the mean of their truncations to 127
    v = np.array([[0.001, 0.003], [0.005, 0.007]], np.float32)
    rgb = np.broadcast_to(v, (1, 3, 2, 2)).copy()
    u = np.float32(255.0) * np.clip((rgb + np.float32(1.0)) * np.float32(0.5), 0, 1)
    img = rule_image(rgb, 2)
    assert img[0, 0, 0, 0] == np.uint8(block_sum(u, 2)[0, 0, 0, 0] * np.float32(0.25))
    after = (block_sum(u.astype(np.uint8).astype(np.float32), 2) * np.float32(0.25)).astype(np.uint8)
    assert img[0, 0, 0, 0] != after[0, 0, 0, 0]          # 128.02.. -> 128 vs mean(127, 127, 128, 128) = 127.5 -> 127
    # a tie between the block sums of two classes goes to the first; the top-left pixel alone would pick the other one
    logits = np.zeros((1, 2, 2, 2), np.float32)
    logits[0, 1, 0, 0] = 1.0
    logits[0, 0, 1, 1] = 1.0
    assert rule_mask(logits, 2)[0, 0, 0] == 0
    assert logits[0, :, 0, 0].argmax() == 1


@pytest.mark.parametrize("f", [1, 2, 4, 8, np.int64(2)])
def test_output_downscale_accepts(f):
    from gan_segmentation_amd.image_generator import ImageGenerator
    assert ImageGenerator.check_output_downscale(f, 7) == int(f)
    assert type(ImageGenerator.check_output_downscale(f, 7)) is int


@pytest.mark.parametrize("max_res_log2", [2, 3, 4])
def test_factor_one_passes_at_every_size(max_res_log2):
    """No downscale, no 16 px floor: ImageGenerator.from_params builds the 4 and 8 px generators the library accepts
    (tests/test_gpu_output_forms.py runs them)."""
    from gan_segmentation_amd.image_generator import ImageGenerator
    assert ImageGenerator.check_output_downscale(1, max_res_log2) == 1
    if max_res_log2 < 5:
        with pytest.raises(ValueError, match="output_downscale"):
            ImageGenerator.check_output_downscale(2, max_res_log2)


@pytest.mark.parametrize("f,max_res_log2", [(3, 10), (16, 10), (0, 10), (-2, 10), (2.0, 10), ("2", 10), (True, 10), (None, 10),
                                            (8, 6), (4, 5), (2, 4)])
def test_output_downscale_rejects(f, max_res_log2):
    """A factor outside {1, 2, 4, 8}, or one that leaves less than 16 px, is refused -- also by from_params before any device
    work."""
    from gan_segmentation_amd import weights as W
    from gan_segmentation_amd.image_generator import ImageGenerator
    with pytest.raises(ValueError, match="output_downscale"):
        ImageGenerator.check_output_downscale(f, max_res_log2)
    gcfg = W.reduced_generator_config(max_res_log2)
    with pytest.raises(ValueError, match="output_downscale"):
        ImageGenerator.from_params(gcfg, {}, gpu_ids=[0], output_downscale=f)


def _config(tmp_path, **keys):
    import yaml
    cfg = {"BASE_DIR": str(tmp_path / "exp"), "GAN": "bedrooms", "GAN_DIR": str(tmp_path / "models"), "GAN_GPU_IDS": [0],
           "GAN_BATCH_SIZE_PER_GPU": 2, "SOLVER_GPU_IDS": [0], "ANNOTATION": "segmentation", "GENERATE_NUM": 3}
    cfg.update(keys)
    path = tmp_path / "config.yml"
    path.write_text(yaml.safe_dump(cfg))
    return str(path)


class _ModelLoaded(Exception):
    pass


@pytest.fixture
def no_models(monkeypatch):
    """`main.py generate` stops where it would load the first model."""
    from gan_segmentation_amd import seg_solver

    def refuse(*args, **kwargs):
        raise _ModelLoaded()
    monkeypatch.setattr(seg_solver, "SegSolver", refuse)


@pytest.mark.parametrize("value", [3, 16, "2", 0.5])
def test_cli_rejects_a_bad_key_before_loading_a_model(tmp_path, no_models, value):
    from gan_segmentation_amd import main as cli
    with pytest.raises(ValueError, match="output_downscale"):
        cli.main(["generate", "--config", _config(tmp_path, OUTPUT_DOWNSCALE=value)])


def test_cli_accepts_the_key_and_its_default(tmp_path, no_models):
    from gan_segmentation_amd import main as cli
    for keys in ({}, {"OUTPUT_DOWNSCALE": 1}, {"OUTPUT_DOWNSCALE": 2}, {"OUTPUT_DOWNSCALE": 8}):
        with pytest.raises(_ModelLoaded):
            cli.main(["generate", "--config", _config(tmp_path, **keys)])
    with pytest.raises(ValueError, match="output_downscale"):      # bedrooms: 256 / 32 < 16
        cli.main(["generate", "--config", _config(tmp_path, OUTPUT_DOWNSCALE=32)])
