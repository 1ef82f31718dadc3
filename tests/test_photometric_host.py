"""The photometric augmentation without a GPU (include/gsa_photometric.h; photometric.photometric_plan / photometric;
ImageGenerator.training_batches(photometric=...)).

``rule_photometric(img, params, seed, first_index)`` is the canonical rule in numpy fp32, one rounding per operation: a separable
7-tap blur with a reflect-101 border accumulated in tap order, ``c = b*alpha + offset[ch]``, ``v = c + noise_sigma*g`` with ``g`` from
the byte sum of one Philox4x32-10 block per value (oracle/ref_philox.py), ``uint8(floor(clamp(v, 0, 255) + 0.5))``.  The GPU tests
(tests/test_gpu_photometric.py) hold the kernel to it byte for byte.  Also here: identity and constant images, the plan (the
splitmix chain, batch independence, the weights, the gates, the limits' checks), the noise source's moments, the header's entry
and row length, and the C entry's argument checks with a null stream."""
import numpy as np
import pytest

from oracle.ref_philox import philox4x32_10

INV_STD = np.float32(1.0 / 295.6010825419961)
COUNTER_TAG = 0x50480000
IDENTITY_W = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)


# -- the rule ------------------------------------------------------------------------------------------------------------------
def noise_unit(seed, index, H, W, C):
    """float32 (H, W, C): g of the header for the global sample ``index`` -- (byte sum of the Philox block - 2040) / 295.601."""
    seed, index = int(seed) & (2 ** 64 - 1), int(index) & (2 ** 64 - 1)
    ctr = np.zeros((H * W, C, 4), np.uint32)
    ctr[..., 0] = np.arange(H * W, dtype=np.uint32)[:, None]
    ctr[..., 1] = (COUNTER_TAG | np.arange(C)).astype(np.uint32)[None, :]
    ctr[..., 2] = index & 0xFFFFFFFF
    ctr[..., 3] = index >> 32
    block = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    S = np.ascontiguousarray(block).view(np.uint8).reshape(H * W, C, 16).astype(np.int32).sum(axis=-1)
    return ((S - 2040).astype(np.float32) * INV_STD).reshape(H, W, C)


def _taps(a, w, axis):
    """sum_k w[k] * a[reflect101(i + k - 3)] along ``axis`` in fp32, accumulated in tap order."""
    n = a.shape[axis]
    idx = np.arange(n)[None, :] + np.arange(-3, 4)[:, None]
    idx = np.abs(idx)
    idx = np.where(idx > n - 1, 2 * (n - 1) - idx, idx)
    acc = None
    for k in range(7):
        term = np.float32(w[k]) * np.take(a, idx[k], axis=axis)
        acc = term if acc is None else acc + term
        assert acc.dtype == np.float32
    return acc


def rule_photometric(img, params, seed, first_index):
    """img (n, H, W, C) u8, params (n, 16) fp32 -> (n, H, W, C) u8: the rule of include/gsa_photometric.h."""
    img, params = np.asarray(img), np.asarray(params)
    assert img.dtype == np.uint8 and img.ndim == 4 and params.dtype == np.float32 and params.shape == (img.shape[0], 16)
    n, H, W, C = img.shape
    assert H >= 4 and W >= 4 and 1 <= C <= 4
    out = np.empty_like(img)
    for s in range(n):
        alpha, offset, sigma, w = params[s, 0], params[s, 1:5], params[s, 5], params[s, 6:13]
        p = img[s].astype(np.float32)
        b = _taps(_taps(p, w, axis=1), w, axis=0)
        c = b * alpha + offset[None, None, :C]
        v = c + sigma * noise_unit(seed, int(first_index) + s, H, W, C)
        assert v.dtype == np.float32
        out[s] = np.floor(np.minimum(np.maximum(v, np.float32(0)), np.float32(255)) + np.float32(0.5)).astype(np.uint8)
    return out


def random_images(seed, n, H, W, C):
    """Seeded u8 images with structure at every scale: smooth ramps, hard edges and noise, so that a blur, a wrong border or a
    shifted tap all change bytes."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    img = np.empty((n, H, W, C), np.uint8)
    for s in range(n):
        for ch in range(C):
            ramp = 255.0 * ((x * (ch + 1) + 2 * y + 7 * s) % (W + H)) / (W + H)
            edges = 120.0 * (((x // 3 + y // 5 + ch) % 2) == 0)
            img[s, :, :, ch] = np.clip(0.5 * ramp + 0.5 * edges + rng.integers(-40, 41, (H, W)), 0, 255)
    return img


def row(alpha=1.0, offset=(0, 0, 0, 0), noise=0.0, w=IDENTITY_W):
    r = np.zeros(16, np.float32)
    r[0], r[1:5], r[5], r[6:13] = alpha, offset, noise, w
    return r


# -- identity and constants ----------------------------------------------------------------------------------------------------
def test_zero_limits_are_the_identity():
    from gan_segmentation_amd import photometric as ph
    rows = ph.photometric_plan(5, 100, 3, **ph.ZERO_LIMITS)
    assert np.array_equal(rows, np.stack([row()] * 3))
    for shape in ((3, 4, 4, 1), (3, 9, 13, 3), (3, 32, 20, 4)):
        img = random_images(3, *shape)
        assert np.array_equal(rule_photometric(img, rows, 5, 100), img)
    assert np.array_equal(rule_photometric(np.full((1, 5, 5, 2), 255, np.uint8), rows[:1], 5, 100), np.full((1, 5, 5, 2), 255, np.uint8))


def test_identity_weights_reproduce_every_byte_value_in_each_tap_sum():
    p = np.arange(256, dtype=np.float32).reshape(16, 16)
    assert np.array_equal(_taps(p, IDENTITY_W, 0), p) and np.array_equal(_taps(p, IDENTITY_W, 1), p)


def test_a_constant_image_stays_constant_under_every_planned_weight_set():
    """Weights of a dense sweep of sigma over (0, 1.5] and of 2000 planned rows: in fp32 the two 7-tap sums of a constant c give a
    value that quantises back to c, for every c."""
    from gan_segmentation_amd import photometric as ph
    sweep = ph.blur_weights(np.concatenate([np.linspace(1e-3, 1.5, 3000), [1e-12, 0.1, 0.25, 1.5]]))
    planned = ph.photometric_plan(11, 0, 2000, blur_prob=1.0, blur_sigma=1.5)[:, 6:13]
    values = np.arange(256, dtype=np.float32)
    for w in np.unique(np.concatenate([sweep, planned]), axis=0):
        acc = None
        for k in range(7):
            acc = w[k] * values if acc is None else acc + w[k] * values
        h = acc
        acc = None
        for k in range(7):
            acc = w[k] * h if acc is None else acc + w[k] * h
        assert np.array_equal(np.floor(acc + np.float32(0.5)), values), w
    img = np.full((1, 6, 7, 3), 201, np.uint8)
    assert np.array_equal(rule_photometric(img, row(w=sweep[1500])[None], 0, 0), img)


def test_the_rule_blurs_shifts_and_saturates():
    img = random_images(9, 2, 12, 15, 3)
    from gan_segmentation_amd import photometric as ph
    w = ph.blur_weights([1.0])[0]
    blurred = rule_photometric(img, np.stack([row(w=w)] * 2), 0, 0)
    assert not np.array_equal(blurred, img)
    # reflect-101 at a corner, by hand in float64: the centre pixel of the 7x7 window is (0, 0)
    idx = np.abs(np.arange(-3, 4))
    want = sum(float(w[a]) * float(w[b]) * float(img[0, idx[a], idx[b], 1]) for a in range(7) for b in range(7))
    assert abs(float(blurred[0, 0, 0, 1]) - want) <= 0.51
    shifted = rule_photometric(img, np.stack([row(offset=(10, -10, 300, 0))] * 2), 0, 0)
    assert np.array_equal(shifted[..., 0], np.minimum(img[..., 0].astype(int) + 10, 255))
    assert np.array_equal(shifted[..., 1], np.maximum(img[..., 1].astype(int) - 10, 0)) and (shifted[..., 2] == 255).all()
    noisy = rule_photometric(img, np.stack([row(noise=5.0)] * 2), 3, 40)
    d = noisy.astype(int) - img
    assert 3.0 < d[(img > 30) & (img < 225)].std() < 7.0
    assert not np.array_equal(noisy[0], rule_photometric(img[:1], row(noise=5.0)[None], 3, 41)[0]), "the index does not reach the noise"
    assert np.array_equal(noisy[1], rule_photometric(img[1:], row(noise=5.0)[None], 3, 41)[0]), "sample k is the global sample first + k"


# -- the plan ------------------------------------------------------------------------------------------------------------------
def test_draws_are_the_stated_splitmix_chain():
    from gan_segmentation_amd import photometric as ph
    M = 2 ** 64 - 1

    def sm(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    for seed, first in ((0, 0), (7, 1000), (123456789012345, 2 ** 33 + 5), (2 ** 64 - 1, 2 ** 63)):
        r = ph.uniforms(seed, first, 3)
        assert r.shape == (3, 10)
        for s in range(3):
            u = sm(((seed ^ 0x50484F544F4D4554) ^ (first + s)) & M)
            for k in range(10):
                if k:
                    u = sm(u)
                assert r[s, k] == (u >> 11) * 2.0 ** -53
    assert ph.PHOTOMETRIC_SEED_XOR == int.from_bytes(b"PHOTOMET", "big")


def test_rows_follow_the_table():
    from gan_segmentation_amd import photometric as ph
    lim = dict(contrast=0.3, brightness=0.1, rgb_shift=12.0, blur_prob=0.6, blur_sigma=1.2, noise_prob=0.4, noise_sigma=9.0)
    r, rows = ph.uniforms(21, 50, 64), ph.photometric_plan(21, 50, 64, **lim)
    assert rows.shape == (64, 16) and rows.dtype == np.float32 and not rows[:, 13:].any()
    beta = 255.0 * 0.1 * (2 * r[:, 1] - 1)
    assert np.array_equal(rows[:, 0], (1 + 0.3 * (2 * r[:, 0] - 1)).astype(np.float32))
    assert np.array_equal(rows[:, 1:5], (beta[:, None] + 12.0 * (2 * r[:, 2:6] - 1)).astype(np.float32))
    blur_on, noise_on = r[:, 6] < 0.6, r[:, 8] < 0.4
    assert blur_on.any() and (~blur_on).any() and noise_on.any() and (~noise_on).any()
    assert np.array_equal(rows[:, 5], np.where(noise_on, 9.0 * r[:, 9], 0.0).astype(np.float32))
    assert np.array_equal(rows[~blur_on, 6:13], np.stack([IDENTITY_W] * int((~blur_on).sum())))
    for s in np.flatnonzero(blur_on):
        w = np.exp(-np.arange(-3, 4) ** 2 / (2 * (1.2 * r[s, 7]) ** 2))
        w[w < 2.0 ** -64] = 0
        assert np.array_equal(rows[s, 6:13], (w / w.sum()).astype(np.float32))
    defaults = ph.plan_parameters(21, 50, 64)
    assert np.array_equal(defaults["alpha"], 1 + 0.2 * (2 * r[:, 0] - 1)) and np.array_equal(defaults["beta"], 255 * 0.2 * (2 * r[:, 1] - 1))
    assert np.array_equal(defaults["sigma"], np.where(r[:, 6] < 0.5, 1.0 * r[:, 7], 0.0))
    assert np.array_equal(defaults["noise"], np.where(r[:, 8] < 0.5, 7.0 * r[:, 9], 0.0))
    assert ph.DEFAULT_LIMITS == dict(contrast=0.2, brightness=0.2, rgb_shift=20.0, blur_prob=0.5, blur_sigma=1.0, noise_prob=0.5,
                                     noise_sigma=7.0)


def test_rows_do_not_depend_on_how_the_range_is_cut():
    from gan_segmentation_amd import photometric as ph
    whole = ph.photometric_plan(9, 2 ** 33, 11)
    parts = [ph.photometric_plan(9, 2 ** 33 + lo, n) for lo, n in ((0, 1), (1, 4), (5, 0), (5, 6))]
    assert np.array_equal(np.concatenate(parts), whole)
    assert not np.array_equal(whole, ph.photometric_plan(10, 2 ** 33, 11)) and ph.photometric_plan(9, 0, 0).shape == (0, 16)


def test_weights_are_symmetric_non_negative_and_sum_to_one():
    from gan_segmentation_amd import photometric as ph
    w = ph.photometric_plan(4, 0, 3000, blur_prob=1.0, blur_sigma=1.5)[:, 6:13]
    assert np.array_equal(w, w[:, ::-1]) and (w >= 0).all()
    assert np.abs(w.astype(np.float64).sum(axis=1) - 1.0).max() < 1e-6
    assert (w[:, 3] >= w[:, 2]).all() and (w[:, 2] >= w[:, 1]).all() and (w[:, 1] >= w[:, 0]).all()
    nz = w[w > 0]
    assert nz.min() >= 2.0 ** -65, "a weight small enough for a denormal product"
    tiny = ph.blur_weights([1e-300, 1e-3, 0.05])
    assert np.array_equal(tiny, np.stack([IDENTITY_W] * 3))
    assert ph.blur_weights([1.5])[0, 0] > 0.01


def test_gates_off_give_identity_weights_and_zero_sigma():
    from gan_segmentation_amd import photometric as ph
    rows = ph.photometric_plan(4, 0, 200, blur_prob=0.0, noise_prob=0.0)
    assert np.array_equal(rows[:, 6:13], np.stack([IDENTITY_W] * 200)) and not rows[:, 5].any()
    assert len(np.unique(rows[:, 0])) == 200, "contrast is still drawn"
    rows = ph.photometric_plan(4, 0, 200, blur_prob=1.0, noise_prob=1.0, blur_sigma=0.0, noise_sigma=0.0)
    assert np.array_equal(rows[:, 6:13], np.stack([IDENTITY_W] * 200)) and not rows[:, 5].any()
    on = ph.photometric_plan(4, 0, 200, blur_prob=1.0, noise_prob=1.0)
    # sigma = r_7 is uniform in [0, 1); below about 0.17 the side taps vanish in fp32 beside a centre of 1, above 0.25 they cannot
    assert (on[:, 5] > 0).all() and (on[:, 9] < 1).sum() >= 120


@pytest.mark.parametrize("bad", [dict(blur_prob=-0.1), dict(blur_prob=1.1), dict(noise_prob=-1e-9), dict(noise_prob=2), dict(contrast=-0.1),
                                 dict(contrast=1.0), dict(brightness=-1), dict(rgb_shift=-0.5), dict(noise_sigma=-1), dict(blur_sigma=-0.1),
                                 dict(blur_sigma=1.5001), dict(hue=0.1), dict(rotate=3), dict(contrast=float("nan")), dict(noise_sigma=float("inf")),
                                 dict(brightness="0.2"), dict(blur_prob=None), dict(contrast=True)])
def test_every_bad_limit_raises(bad):
    from gan_segmentation_amd import photometric as ph
    with pytest.raises(ValueError):
        ph.photometric_plan(0, 0, 2, **bad)
    with pytest.raises(ValueError):
        ph.check_keyword(bad)


def test_limits_at_their_bounds_and_the_keyword():
    from gan_segmentation_amd import photometric as ph
    ph.photometric_plan(0, 0, 2, blur_prob=1, noise_prob=0, contrast=0.999, blur_sigma=1.5, brightness=0, rgb_shift=0, noise_sigma=0)
    assert ph.check_keyword(None) is None and ph.check_keyword(True) == ph.DEFAULT_LIMITS
    assert ph.check_keyword({}) == ph.DEFAULT_LIMITS and ph.check_keyword(dict(contrast=0))["contrast"] == 0.0
    for bad in (False, 1, "on", 0.5, [("contrast", 0.1)]):
        with pytest.raises(ValueError, match="photometric"):
            ph.check_keyword(bad)
    with pytest.raises(ValueError):
        ph.photometric_plan(0, 0, -1)


def test_training_batches_takes_the_keyword_in_front_of_the_limits():
    import inspect
    from gan_segmentation_amd.image_generator import ImageGenerator
    params = list(inspect.signature(ImageGenerator.training_batches).parameters.values())
    names = [p.name for p in params]
    assert names[-1] == "limits" and params[-1].kind is inspect.Parameter.VAR_KEYWORD
    assert "photometric" in names and params[names.index("photometric")].default is None


# -- the noise source ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,index", [(0, 0), (7, 1000), (123456789012345, 2 ** 33 + 5)])
def test_noise_source_has_zero_mean_and_unit_variance(seed, index):
    g = noise_unit(seed, index, 64, 64, 3)
    print("seed %d index %d: mean %.4f std %.4f" % (seed, index, g.mean(), g.std()))
    assert g.dtype == np.float32 and abs(float(g.mean())) < 0.05 and abs(float(g.std()) - 1.0) < 0.05
    assert np.abs(g).max() <= 2040 / 295.6
    assert 16 * (256 ** 2 - 1) / 12 == 87380 and abs(295.6010825419961 ** 2 - 87380) < 1e-6


def test_noise_blocks_differ_by_pixel_channel_index_and_seed():
    base = noise_unit(5, 9, 8, 8, 4)
    assert len(np.unique(base)) > 200
    assert np.array_equal(noise_unit(5, 9, 8, 8, 2), base[..., :2]), "the channel is a counter word, not a stride"
    for other in (noise_unit(6, 9, 8, 8, 4), noise_unit(5, 10, 8, 8, 4), noise_unit(5 + 2 ** 32, 9, 8, 8, 4), noise_unit(5, 9 + 2 ** 32, 8, 8, 4)):
        assert (other != base).mean() > 0.9


# -- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_photometric_header_symbols_are_exported(hip_library):
    """include/gsa_photometric.h declares the one entry, of ten arguments, and the row length of photometric."""
    from gan_segmentation_amd import _lib, photometric as ph
    from tests.common import header_declarations
    header, declared = header_declarations("gsa_photometric.h")
    assert set(declared) == {"gsa_photometric"}
    assert "#define GSA_PHOTOMETRIC_ROW %d" % ph.ROW in header
    assert len(declared["gsa_photometric"][1]) == len(_lib.load_library().fn("gsa_photometric").argtypes) == 10


def test_photometric_rejects_bad_arguments_before_touching_the_gpu(hip_library):
    """Argument validation of gsa_photometric happens on the host (no HIP call precedes it, the stream is null): channels outside
    1..4, H or W below 4, more than 2^31 pixels, null pointers, out == img; an empty batch is a successful no-op."""
    from gan_segmentation_amd._lib import load_library
    fn = load_library().fn("gsa_photometric")
    good = dict(n=2, H=32, W=48, C=3, img=1 << 20, params=4 << 20, out=2 << 20)

    def call(**kw):
        a = dict(good, **kw)
        return fn(None, a["n"], a["H"], a["W"], a["C"], a["img"], a["params"], 7, 9, a["out"])

    for bad in (dict(C=0), dict(C=5), dict(C=-1), dict(H=3), dict(W=3), dict(H=0), dict(W=-8), dict(H=1 << 16, W=(1 << 15) + 1),
                dict(H=46341, W=46341), dict(img=None), dict(params=None), dict(out=None), dict(out=1 << 20), dict(n=-1),
                dict(out=(1 << 20) + 2 * 32 * 48 * 3 - 1), dict(img=(2 << 20) + 1), dict(params=(4 << 20) + 2)):
        assert call(**bad) == -1, bad
    assert call(n=0) == 0 and call(n=0, img=None, params=None, out=None) == 0
    assert call(n=0, C=5) == -1 and call(n=0, H=3) == -1


def test_photometric_checks_its_tensors_before_any_gpu_work():
    import torch
    from gan_segmentation_amd import photometric as ph
    rows = ph.photometric_plan(0, 0, 1)
    for bad in (torch.zeros((1, 8, 8, 3), dtype=torch.uint8), torch.zeros((8, 8, 3), dtype=torch.uint8), np.zeros((1, 8, 8, 3), np.uint8), None):
        with pytest.raises(ValueError, match="photometric takes"):
            ph.photometric(bad, rows, 0, 0)
    for shape in ((8, 3, 1), (3, 8, 1), (8, 8, 5), (8, 8, 0)):
        with pytest.raises(ValueError):
            ph.check_shape(*shape)
    ph.check_shape(4, 4, 1)
    ph.check_shape(1 << 16, 1 << 15, 4)
    with pytest.raises(ValueError):
        ph.check_shape(1 << 16, (1 << 15) + 1, 1)
