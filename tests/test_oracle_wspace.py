"""The C oracle's W-space entries (gsao_mapping_forward / gsao_generator_forward_w / gsao_generate_w) on weights whose w depends
on z (tests.common.lively): against the reference-order torch restatement (oracle/ref_semantic.py), against the oracle's own z
path, and their argument checks.  The synthetic weights' mapping output is the same for every z, so these checks need the
live mapping layers to mean anything; each asserts that precondition itself."""
import numpy as np
import pytest
import torch

from oracle import ref_semantic as S
from tests.common import odd_setup, reduced_setup, w_spread

# Oracle vs restatement on live weights: rgb / every feature / logits within 1e-3 (measured: 4.2e-4 at worst, the last feature
# of the odd config; rgb 1.4e-4 of a range of about 18).  The z path's 2e-4 bar of test_c_oracle_matches_semantic_oracle is for
# the synthetic weights, whose styles hardly vary; live styles widen the AdaIN scales and the rounding differences with them.
TOL = 1e-3


def _setup(kind, batch):
    if kind == "reduced":
        return reduced_setup(7, batch=batch, live_mapping=True)
    return odd_setup(batch, live_mapping=True)


def _layers(gcfg):
    return 2 * (gcfg["max_res_log2"] - 1)


def _rows(n, L, scale, seed):
    """Independent standard-normal rows per (sample, layer), at w's scale."""
    return (np.random.default_rng(seed).standard_normal((n, L, 512)) * scale).astype(np.float32)


def _psi(L):
    """Per-layer truncation with 0, 1, 1.5 and a negative value among ordinary ones."""
    return np.array([0.0, 1.0, 1.5, -0.5] + list(np.linspace(0.3, 1.2, L - 4)), np.float32)


@pytest.mark.parametrize("kind", ["reduced", "odd"])
def test_mapping_matches_the_restatement_and_depends_on_z(oracle_lib, kind):
    gcfg, gp, dcfg, dp, z, _noise = _setup(kind, 4)
    w = oracle_lib.Oracle(gcfg, gp, dcfg, dp).mapping(z)
    assert w.shape == z.shape and w.dtype == np.float32
    assert w_spread(w) > 0.1, "precondition: w must depend on z"
    with torch.no_grad():
        sw = S.SemanticGenerator(gcfg, gp).mapping(torch.from_numpy(z)).numpy()
    assert np.abs(w - sw).max() <= 1e-4 * max(1.0, float(np.abs(sw).max()))          # measured 7.6e-6 (max |w| 6.9)


@pytest.mark.parametrize("kind", ["reduced", "odd"])
def test_generator_w_matches_the_restatement(oracle_lib, kind):
    """Independent rows per (sample, layer) and a per-layer psi holding 0, 1, 1.5 and -0.5: rgb, every feature and the logits
    within TOL of the reference-order restatement."""
    gcfg, gp, dcfg, dp, z, noise = _setup(kind, 3)
    L = _layers(gcfg)
    w = oracle_lib.Oracle(gcfg, gp, dcfg, dp).mapping(z)
    assert w_spread(w) > 0.1
    gp = dict(gp, truncation_psi=_psi(L))
    dl = _rows(3, L, float(w.std()), seed=7)
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp)
    rgb, img, feats = o.generator_w(dl, noise)
    logits, mask = o.decoder(feats)
    srgb, sfeats, slog = S.synthesis(gcfg, gp, dcfg, dp, dl, noise)
    assert np.abs(rgb - srgb).max() <= TOL
    for i, (a, b) in enumerate(zip(feats, sfeats)):
        assert np.abs(a - b).max() <= TOL, "feature %d" % i
    assert np.abs(logits - slog).max() <= TOL
    # and the fused entry is the two calls
    img2, mask2 = o.generate_w(dl, noise)
    assert np.array_equal(img2, img) and np.array_equal(mask2, mask)


@pytest.mark.parametrize("kind", ["reduced", "odd"])
def test_z_path_with_live_weights_matches_the_restatement(oracle_lib, kind):
    gcfg, gp, dcfg, dp, z, noise = _setup(kind, 2)
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp)
    assert w_spread(o.mapping(z)) > 0.1
    rgb, _img, feats = o.generator(z, noise)
    logits, _mask = o.decoder(feats)
    _i, _m, srgb, sfeats, slog = S.generate(gcfg, gp, dcfg, dp, z, noise)
    assert np.abs(rgb - srgb).max() <= TOL
    for i, (a, b) in enumerate(zip(feats, sfeats)):
        assert np.abs(a - b).max() <= TOL, "feature %d" % i
    assert np.abs(logits - slog).max() <= TOL


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["reduced", "odd"])
def test_broadcast_w_path_equals_the_z_path(oracle_lib, kind, precision):
    """generator_w(broadcast(mapping(z))) == generator(z) and generate_w == generate, bit for bit; a row changed at layer l
    changes the sample's features from level l // 2 on and nothing before it or in the other samples."""
    gcfg, gp, dcfg, dp, z, noise = _setup(kind, 2)
    L = _layers(gcfg)
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp, precision=precision)
    w = o.mapping(z)
    assert w_spread(w) > 0.1
    dl = np.repeat(w[:, None, :], L, axis=1)
    rgb, img, feats = o.generator(z, noise)
    rgb_w, img_w, feats_w = o.generator_w(dl, noise)
    assert np.array_equal(rgb_w, rgb) and np.array_equal(img_w, img)
    for a, b in zip(feats_w, feats):
        assert np.array_equal(a, b)
    i1, m1 = o.generate(z, noise)
    i2, m2 = o.generate_w(dl, noise)
    assert np.array_equal(i1, i2) and np.array_equal(m1, m2)
    layer = L - 3
    dl2 = dl.copy()
    dl2[1, layer] = _rows(1, 1, float(w.std()), seed=3)[0, 0]
    _rgb2, _img2, feats2 = o.generator_w(dl2, noise)
    for lv, (a, b) in enumerate(zip(feats2, feats)):
        assert np.array_equal(a[0], b[0])
        assert np.array_equal(a[1], b[1]) == (lv < layer // 2), lv


def test_w_entries_validate_their_arguments(oracle_lib):
    gcfg, gp, dcfg, dp, z, noise = _setup("reduced", 2)
    L = _layers(gcfg)
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp)
    w = o.mapping(z)
    good = np.repeat(w[:, None, :], L, axis=1)
    for bad in (L - 1, L + 1):
        dl = np.ascontiguousarray(good[:, :bad] if bad < L else np.concatenate([good, good[:, :1]], axis=1))
        with pytest.raises(oracle_lib.OracleError, match="layers"):
            o.generator_w(dl, noise)
        with pytest.raises(oracle_lib.OracleError, match="layers"):
            o.generate_w(dl, noise)
    with pytest.raises(oracle_lib.OracleError):
        o.generator_w(good[:, :, :256], noise)                 # wrong latent size
    with pytest.raises(oracle_lib.OracleError):
        o.mapping(z[:, :100])
    lib, h = o.lib, o._h
    nz = oracle_lib._ptrs([np.ascontiguousarray(a, np.float32) for a in noise])
    img = np.empty((2, 128, 128, 3), np.uint8)
    mask = np.empty((2, 128, 128), np.uint8)
    rgb = np.empty((2, 3, 128, 128), np.float32)
    assert lib.gsao_generator_forward_w(h, None, 2, None, L, nz, len(noise), rgb.ctypes.data, None, None, 0) == -1
    assert b"null" in lib.gsao_last_error(h)
    assert lib.gsao_generate_w(h, None, 2, None, L, nz, len(noise), img.ctypes.data, mask.ctypes.data) == -1
    assert lib.gsao_generator_forward_w(h, None, 2, good.ctypes.data, L, nz, len(noise) - 1, rgb.ctypes.data, None, None, 0) == -1
    assert lib.gsao_mapping_forward(h, None, 2, None, w.ctypes.data) == -1
    assert lib.gsao_mapping_forward(h, None, 2, z.ctypes.data, None) == -1
    bare = oracle_lib.Oracle()                                 # nothing committed: a state error
    assert bare.lib.gsao_mapping_forward(bare._h, None, 2, z.ctypes.data, w.ctypes.data) == -2
    assert bare.lib.gsao_generator_forward_w(bare._h, None, 2, good.ctypes.data, L, nz, len(noise), rgb.ctypes.data, None, None, 0) == -2
    assert bare.lib.gsao_generate_w(bare._h, None, 2, good.ctypes.data, L, nz, len(noise), img.ctypes.data, mask.ctypes.data) == -2
    # the context is still usable and still right
    i1, m1 = o.generate_w(good, noise)
    i2, m2 = o.generate(z, noise)
    assert np.array_equal(i1, i2) and np.array_equal(m1, m2)
