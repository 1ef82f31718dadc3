"""Counter-based inputs (gsa_fill_inputs)."""
import numpy as np
import pytest

from oracle import ref_philox


def test_philox_known_answers():
    """Random123's published known-answer vectors for philox4x32-10 pin the restatement."""
    kat = [
        ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ]
    for ctr, key, expect in kat:
        got = ref_philox.philox4x32_10(np.array(ctr, np.uint32), key)
        assert tuple(int(v) for v in got) == expect


def test_restated_normals_are_standard_normal():
    x = ref_philox.fill_normal(4, 1 << 16, 7, 3, 12345)
    assert abs(x.mean()) < 0.01 and abs(x.var() - 1.0) < 0.02 and np.isfinite(x).all()
    assert not np.array_equal(x[0], x[1])
    assert np.array_equal(ref_philox.fill_normal(1, 64, 8, 3, 12345)[0], x[1, :64])      # keyed on the sample index


@pytest.mark.gpu
def test_device_inputs_match_restatement_and_do_not_depend_on_the_shard():
    import torch
    from gan_segmentation_amd.image_generator import ImageGenerator
    from tests.common import reduced_setup
    gcfg, gp, dcfg, dp, _z, _noise = reduced_setup(7, batch=6)
    gen = ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=6)
    z, noise = gen.netG.draw_indexed(10, 6, seed=99)
    z_ref = ref_philox.fill_normal(6, gcfg["latent_size"], 10, 0xFFFF, 99)
    assert np.abs(z.cpu().numpy() - z_ref).max() <= 2e-5
    for l, a in enumerate(noise):
        R = a.shape[-1]
        ref = ref_philox.fill_normal(6, R * R, 10, l, 99).reshape(6, 1, R, R)
        assert np.abs(a.cpu().numpy() - ref).max() <= 2e-5, "plane %d" % l
    # a sample is the same bytes whatever batch produces it
    img, mask = gen.generate_indexed(10, 6, seed=99)
    img_a, mask_a = gen.generate_indexed(10, 2, seed=99)
    img_b, mask_b = gen.generate_indexed(12, 4, seed=99)
    assert torch.equal(img, torch.cat([img_a, img_b])) and torch.equal(mask, torch.cat([mask_a, mask_b]))
    img_c, _ = gen.generate_indexed(10, 2, seed=100)
    assert not torch.equal(img_c, img_a)
    big = gen.netG.draw_indexed(2 ** 33 + 5, 1, seed=1)[0]          # 64-bit sample indices
    assert np.abs(big.cpu().numpy() - ref_philox.fill_normal(1, gcfg["latent_size"], 2 ** 33 + 5, 0xFFFF, 1)).max() <= 2e-5


# ---- full size: the stride loop of fill_normal_kernel ------------------------------------------------------------------
# launch_fill_normal (csrc/gsa_kernels.hip) caps the grid at 4096 workgroups of 256 threads, one quad of values each; beyond
# FILL_QUADS_PER_PASS quads per plane a thread walks several quads and splits each index into (sample, quad) again.
FILL_QUADS_PER_PASS = 4096 * 256
FFHQ_PLANE = 1024 * 1024


def test_the_fill_grid_cap_is_the_one_these_tests_assume():
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gan-segmentation_amd", "csrc", "gsa_kernels.hip")).read()
    assert "const int grid = (int)std::min<long>((total + 255) / 256, 4096);" in src


def test_float64_box_muller_against_the_fp32_restatement():
    """tests/f64_ref.fill_normal_f64 and oracle/ref_philox.fill_normal share the uniforms and nothing after them: 2 x 1024^2 draws
    (first index 2^32 - 1: the second sample has carried into the high counter word) agree within the 2e-5 the device is held to."""
    from tests import f64_ref
    args = (2, FFHQ_PLANE, 2 ** 32 - 1, 17, 99)
    x32, x64 = ref_philox.fill_normal(*args), f64_ref.fill_normal_f64(*args)
    d = np.abs(x32 - x64).max()
    print("fp32 restatement vs float64 Box-Muller over %d draws: max %.3e" % (x64.size, d))
    assert d <= 2e-5
    assert np.isfinite(x64).all() and np.abs(x64).max() <= f64_ref.NORMAL_ABS_MAX
    N = x64.size
    assert abs(x64.mean()) <= 5 / np.sqrt(N) and abs(x64.var() - 1) <= 5 * np.sqrt(2 / N)


@pytest.fixture(scope="module")
def ffhq_generator(torch_cuda):
    """An FFHQ-configured generator reserved for ONE sample: draw_indexed needs loaded parameters but no forward pass, so the
    workspace stays small whatever n is drawn."""
    from gan_segmentation_amd.image_generator import ImageGenerator
    from tests.common import gan_setup
    gcfg, gp, dcfg, dp, _z, _noise = gan_setup("ffhq", 1)
    gen = ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=1)
    yield gen.netG
    del gen
    torch_cuda.cuda.empty_cache()


def _planes(g, first, n, seed):
    """draw_indexed as host arrays: [(plane id, (n, per_sample) fp32)], z first (plane id 0xFFFF)."""
    z, noise = g.draw_indexed(first, n, seed=seed)
    return [(0xFFFF, z.cpu().numpy())] + [(l, a.cpu().numpy().reshape(n, -1)) for l, a in enumerate(noise)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 5])
def test_full_size_inputs_against_float64(ffhq_generator, n):
    """z and all 18 noise planes of an FFHQ generator at n = 8 (the 1024^2 planes have 2 097 152 quads: two full passes of the
    capped grid) and n = 5 (1 310 720 quads: a partial second pass) within 2e-5 of the float64 Box-Muller of the same uniforms.
    Measured on an MI355X: max |device - float64| over z and the 18 planes = 1.87e-6 at n = 8 and at n = 5 (the fp32 numpy restatement
    over 2 x 1024^2 draws: 1.6e-6).  The bound stays the 2e-5 this module has always used."""
    from tests import f64_ref
    first, seed = 10, 99
    assert n * FFHQ_PLANE // 4 > FILL_QUADS_PER_PASS, "the largest planes must take the stride loop"
    worst = 0.0
    for plane, got in _planes(ffhq_generator, first, n, seed):
        ref = f64_ref.fill_normal_f64(n, got.shape[1], first, plane, seed)
        d = float(np.abs(got - ref).max())
        worst = max(worst, d)
        assert d <= 2e-5, "plane %d (%d values per sample): max |device - float64| = %.3e" % (plane, got.shape[1], d)
    print("n = %d: max |device - float64| over z and 18 planes = %.3e" % (n, worst))


@pytest.mark.gpu
def test_full_size_batch_is_the_single_fills_bit_for_bit(ffhq_generator):
    """What generate_indexed rests on, at full size and without a tolerance: every plane of a batch of 8 equals the eight one-sample
    fills of the same indices; a batch that carries from the low into the high counter word (first index 2^32 - 2, n = 4) equals its
    four single fills, and the reference; two planes, and two seeds, of the same sample differ."""
    from tests import f64_ref
    g = ffhq_generator
    for first, n, seed in ((10, 8, 99), (2 ** 32 - 2, 4, 7)):
        batch = _planes(g, first, n, seed)
        for k in range(n):
            for (plane, b), (_p, s) in zip(batch, _planes(g, first + k, 1, seed)):
                assert np.array_equal(b[k], s[0]), "first index %d, plane %d: sample %d of the batch differs from its single fill" % (first, plane, k)
        if first != 10:
            for plane, b in batch:
                assert np.abs(b - f64_ref.fill_normal_f64(n, b.shape[1], first, plane, seed)).max() <= 2e-5, "plane %d across the carry" % plane
            assert not np.array_equal(batch[-1][1][1], batch[-1][1][2])         # indices 2^32 - 1 and 2^32: not the same stream
    batch = dict(_planes(g, 10, 8, 99))
    other = dict(_planes(g, 10, 8, 100))
    assert batch[16].shape == batch[17].shape == (8, FFHQ_PLANE)
    for k in range(8):
        assert not np.array_equal(batch[16][k], batch[17][k]), "planes 16 and 17 of sample %d are the same" % k
        assert not np.array_equal(batch[17][k], other[17][k]), "seeds 99 and 100 give sample %d the same plane" % k
        assert np.abs(batch[16][k] - batch[17][k]).mean() > 0.5 and np.abs(batch[17][k] - other[17][k]).mean() > 0.5


@pytest.mark.gpu
def test_full_size_plane_is_standard_normal(ffhq_generator):
    """One 1024^2 x 8 plane, N = 8 388 608 values: all finite; max |x| <= sqrt(-2 ln 2^-25) (1 + 2^-20), the largest value the formula
    can give; |mean| <= 5 / sqrt(N) and |var - 1| <= 5 sqrt(2 / N), five standard deviations of the estimators."""
    from tests import f64_ref
    _z, noise = ffhq_generator.draw_indexed(10, 8, seed=99)
    x = noise[17].cpu().numpy().astype(np.float64).reshape(-1)
    N = x.size
    assert N == 8 * FFHQ_PLANE
    print("plane 17, N = %d: max |x| %.4f (bound %.4f), mean %.3e (bound %.3e), var - 1 %.3e (bound %.3e)" % (
        N, np.abs(x).max(), f64_ref.NORMAL_ABS_MAX, x.mean(), 5 / np.sqrt(N), x.var() - 1, 5 * np.sqrt(2 / N)))
    assert np.isfinite(x).all()
    assert np.abs(x).max() <= f64_ref.NORMAL_ABS_MAX
    assert abs(x.mean()) <= 5 / np.sqrt(N)
    assert abs(x.var() - 1.0) <= 5 * np.sqrt(2.0 / N)
