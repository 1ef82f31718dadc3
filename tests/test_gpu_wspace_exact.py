"""The mapping network, the per-sample styles and the W path, bit for bit against the C oracle, on weights whose w depends on z
(tests.common.lively).  With the synthetic weights w is the same for every z, so a mapping or style fault -- a stale word of an
earlier launch, a wrong ping-pong buffer or chunk, a style row of the wrong layer or sample -- turns into the same w and the
other bit-exact tests cannot see it.  Every test here asserts that its inputs do vary (w_spread)."""
import os

import numpy as np
import pytest

from tests.common import gan_setup, odd_setup, reduced_setup, w_spread

pytestmark = pytest.mark.gpu


def _first_diff(a, b):
    idx = np.argwhere(a != b)
    return "%d of %d differ, first at %s: %r vs %r" % (len(idx), a.size, tuple(idx[0]), a[tuple(idx[0])], b[tuple(idx[0])])


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, "%s: shape %s vs %s" % (what, a.shape, b.shape)
    assert np.array_equal(a, b), "%s: %s" % (what, _first_diff(a, b))


def _setup(kind, batch):
    if kind == "reduced":
        return reduced_setup(7, batch=batch, live_mapping=True)
    if kind == "odd":
        return odd_setup(batch, live_mapping=True)
    return gan_setup(kind, batch, live_mapping=True)


def _build(gcfg, gp, dcfg, dp, batch, **kw):
    from gan_segmentation_amd.image_generator import ImageGenerator
    return ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=batch, **kw)


def _layers(gcfg):
    return 2 * (gcfg["max_res_log2"] - 1)


def _rows(n, L, scale, seed):
    """Independent standard-normal rows per (sample, layer), at w's scale."""
    return (np.random.default_rng(seed).standard_normal((n, L, 512)) * scale).astype(np.float32)


def _latents(n, seed):
    return np.random.default_rng(seed).standard_normal((n, 512)).astype(np.float32)


def _noise(gcfg, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, 1, 4 << (i // 2), 4 << (i // 2))).astype(np.float32) for i in range(_layers(gcfg))]


def _w_scale(oracle):
    """The scale of w under these weights (its std over a few latents); asserts that w depends on z."""
    w = oracle.mapping(_latents(4, 1))
    assert w_spread(w) > 0.1, "precondition: w must depend on z"
    return float(w.std())


# -- z path ---------------------------------------------------------------------------------------------------------------

def test_mapping_is_bit_exact_over_slices_and_chunks(torch_cuda, oracle_lib):
    """Generator.mapping == Oracle.mapping at batches 1 (one chunk), 16, 17 (two slices), 64, 65 (four slices + a fifth chunk
    looped inside slice 0) and 130 (chunks looped in every slice), one after another on the same context -- each launch must
    read its own words, never those an earlier launch or layer left in the exchange buffers -- and again at 17 after 130."""
    gcfg, gp, dcfg, dp, _z, _noise = _setup("reduced", 1)
    o = oracle_lib.Oracle(gcfg, gp)
    gen = _build(gcfg, gp, dcfg, dp, 1)
    for k, n in enumerate([1, 16, 17, 64, 65, 130, 17]):
        z = _latents(n, 100 + k)
        want = o.mapping(z)
        if n > 1:
            assert w_spread(want) > 0.1, "precondition: w must depend on z"
        _same(gen.netG.mapping(z).cpu().numpy(), want, "w at batch %d" % n)


@pytest.mark.parametrize("kind,batch", [("reduced", 5), ("odd", 3), ("ffhq", 2)])
def test_z_path_with_live_mapping_is_bit_exact(torch_cuda, oracle_lib, kind, batch):
    """rgb, every feature, logits, image and mask of the z path == the oracle, with a w that differs per sample."""
    gcfg, gp, dcfg, dp, z, noise = _setup(kind, batch)
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp)
    assert w_spread(o.mapping(z)) > 0.1
    rgb_o, img_o, feats_o = o.generator(z, noise)
    logits_o, mask_o = o.decoder(feats_o)
    gen = _build(gcfg, gp, dcfg, dp, batch)
    img, mask = gen.generate_batch(z, noise)
    _same(img.cpu().numpy(), img_o, "image")
    _same(mask.cpu().numpy(), mask_o, "mask")
    rgb, feats = gen.netG(z, noise=noise)
    _same(rgb.cpu().numpy(), rgb_o, "rgb")
    for i, (a, b) in enumerate(zip(feats, feats_o)):
        _same(a.cpu().numpy(), b, "feature %d" % i)
    logits, _mask = gen._decoder(*feats, want_mask=True)
    _same(logits.cpu().numpy(), logits_o, "logits")


_MAPPING_WORKER = r'''
import sys
import numpy as np
sys.path.insert(0, ROOT_DIR)
import torch
from tests.common import reduced_setup, w_spread
from gan_segmentation_amd.image_generator import ImageGenerator
from oracle.binding import Oracle
gcfg, gp, dcfg, dp, _z, _noise = reduced_setup(7, batch=1, live_mapping=True)
o = Oracle(gcfg, gp)
gen = ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=1)
for n in (1, 17, 130):
    z = np.random.default_rng(n).standard_normal((n, 512)).astype(np.float32)
    want = o.mapping(z)
    assert n == 1 or w_spread(want) > 0.1
    got = gen.netG.mapping(z).cpu().numpy()
    assert np.array_equal(got, want), "w at batch %d: %d values differ" % (n, int((got != want).sum()))
print("MAPPING_OK")
'''


def test_unfused_mapping_is_bit_exact(torch_cuda, tmp_path):
    """GSA_MAPFUSE=0 (the ten-launch PixelNorm + dense form; read once per process, hence a child) == Oracle.mapping."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "mapping_worker.py"
    script.write_text(_MAPPING_WORKER.replace("ROOT_DIR", repr(root)))
    out = subprocess.run([sys.executable, str(script)], env=dict(os.environ, GSA_MAPFUSE="0"), capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "MAPPING_OK" in out.stdout, out.stdout[-800:] + out.stderr[-2500:]


def test_graph_replay_with_live_mapping_matches_the_oracle(torch_cuda, oracle_lib, monkeypatch):
    """test_graph_replay_of_small_steps_matches_the_oracle with latents whose w differ: z is rewritten in place between replays,
    so a replayed mapping launch that read the previous launch's words, or its own stale launch number, would produce the
    other sample pair's image."""
    monkeypatch.setenv("GSA_GRAPH", "1")
    gcfg, gp, dcfg, dp, z, noise = _setup("reduced", 4)
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp)
    w = o.mapping(z)
    assert np.abs(w[:2] - w[2:]).max() > 0.1, "precondition: the two latent pairs must map to different w"
    want = [o.generate(z[k:k + 2], [a[k:k + 2] for a in noise]) for k in (0, 2)]
    assert not np.array_equal(want[0][0], want[1][0])
    gen = _build(gcfg, gp, dcfg, dp, 2)
    zt = torch_cuda.from_numpy(z[:2].copy()).cuda()
    nt = [torch_cuda.from_numpy(a[:2].copy()).cuda() for a in noise]
    out = (torch_cuda.empty((2, 128, 128, 3), dtype=torch_cuda.uint8, device="cuda"),
           torch_cuda.empty((2, 128, 128), dtype=torch_cuda.uint8, device="cuda"))
    model = gen.netG._model
    for it in range(40):                                 # the 32nd identical call is captured, the later ones are replays
        k = 0 if it % 2 == 0 else 2
        zt.copy_(torch_cuda.from_numpy(z[k:k + 2].copy()))
        for t, a in zip(nt, noise):
            t.copy_(torch_cuda.from_numpy(a[k:k + 2].copy()))
        out[0].zero_(); out[1].zero_()
        img, mask = gen.generate_batch(zt, nt, out=out)
        _same(img.cpu().numpy(), want[k // 2][0], "image, call %d" % it)
        _same(mask.cpu().numpy(), want[k // 2][1], "mask, call %d" % it)
    assert len(model.__dict__.get("_graphs", {})) == 1, "the repeated call was never captured"


# -- W path ---------------------------------------------------------------------------------------------------------------

def _w_path_vs_oracle(gen, o, dl, noise, what, samples=None):
    """synthesis (rgb, every feature) and generate_w (image, mask) of dlatents dl on the GPU == the oracle's generator_w /
    generate_w, on all samples or on the listed ones (the oracle runs them independently)."""
    g = gen.netG
    rgb, feats = g.synthesis(dl, noise=noise)
    img, mask = gen.generate_batch_w(dl, noise)
    sel = list(range(dl.shape[0])) if samples is None else list(samples)
    rgb_o, img_o, feats_o = o.generator_w(dl[sel], [a[sel] for a in noise])
    logits_o, mask_o = o.decoder(feats_o)
    _same(rgb.cpu().numpy()[sel], rgb_o, "%s rgb" % what)
    for i, (a, b) in enumerate(zip(feats, feats_o)):
        _same(a.cpu().numpy()[sel], b, "%s feature %d" % (what, i))
    _same(img.cpu().numpy()[sel], img_o, "%s image" % what)
    _same(mask.cpu().numpy()[sel], mask_o, "%s mask" % what)
    return feats, logits_o


@pytest.mark.parametrize("kind,batch", [("reduced", 3), ("reduced", 17), ("odd", 3), ("ffhq", 1)])
def test_independent_rows_are_bit_exact(torch_cuda, oracle_lib, kind, batch):
    """dlatents with an independent row per (sample, layer): every layer's styles come from its own row.  The odd config has
    96 style columns per layer (a 64-wide tile and a 32-wide one); ffhq has 32-column layers at 1024 px and 1024-column
    layers at 512 channels."""
    gcfg, gp, dcfg, dp, _z, noise = _setup(kind, batch)
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp)
    dl = _rows(batch, _layers(gcfg), _w_scale(o), seed=batch)
    gen = _build(gcfg, gp, dcfg, dp, batch)
    _w_path_vs_oracle(gen, o, dl, noise, "%s b%d" % (kind, batch))


def test_per_layer_psi_is_bit_exact(torch_cuda, oracle_lib):
    """A per-layer truncation_psi holding 0, 1, 1.5 and a negative value: the W path and the z path == the oracle loaded with
    the same vector."""
    gcfg, gp, dcfg, dp, z, noise = _setup("reduced", 3)
    L = _layers(gcfg)
    psi = [0.0, 1.0, 1.5, -0.5] + [float(v) for v in np.linspace(0.3, 1.2, L - 4)]
    o = oracle_lib.Oracle(gcfg, dict(gp, truncation_psi=np.asarray(psi, np.float32)), dcfg, dp)
    dl = _rows(3, L, _w_scale(o), seed=5)
    gen = _build(gcfg, gp, dcfg, dp, 3, truncation_psi=psi)
    _w_path_vs_oracle(gen, o, dl, noise, "per-layer psi")
    img, mask = gen.generate_batch(z, noise)
    img_o, mask_o = o.generate(z, noise)
    _same(img.cpu().numpy(), img_o, "per-layer psi, z path image")
    _same(mask.cpu().numpy(), mask_o, "per-layer psi, z path mask")


def test_batch_130_styles_reach_every_sample(torch_cuda, oracle_lib):
    """130 samples: the style kernel's grid covers 8 x 16 samples and loops for the rest; samples on both sides of every
    chunk and loop boundary == the oracle."""
    gcfg, gp, dcfg, dp, _z, _nz = _setup("reduced", 1)
    n = 130
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp)
    dl = _rows(n, _layers(gcfg), _w_scale(o), seed=130)
    noise = _noise(gcfg, n, seed=131)
    gen = _build(gcfg, gp, dcfg, dp, n)
    _w_path_vs_oracle(gen, o, dl, noise, "batch 130", samples=[0, 15, 16, 127, 128, 129])


def test_each_row_feeds_only_its_own_layer(torch_cuda, oracle_lib):
    """For every layer l, changing only row l of one sample leaves the features of levels < l // 2 and every other sample
    bit-identical and changes level l // 2: the tile table maps each layer's columns to that layer's row, without the oracle."""
    import torch
    gcfg, gp, dcfg, dp, _z, noise = _setup("reduced", 3)
    L = _layers(gcfg)
    scale = _w_scale(oracle_lib.Oracle(gcfg, gp))
    dl = _rows(3, L, scale, seed=21)
    fresh = _rows(1, L, scale, seed=22)[0]
    g = _build(gcfg, gp, dcfg, dp, 3).netG
    base = [f.cpu().numpy() for f in g.synthesis(torch.from_numpy(dl), noise=noise)[1]]
    s = 1
    for l in range(L):
        dl2 = dl.copy()
        dl2[s, l] = fresh[l]
        feats = [f.cpu().numpy() for f in g.synthesis(torch.from_numpy(dl2), noise=noise)[1]]
        for lv, (a, b) in enumerate(zip(feats, base)):
            for other in (0, 2):
                _same(a[other], b[other], "layer %d changed: sample %d level %d" % (l, other, lv))
            if lv < l // 2:
                _same(a[s], b[s], "layer %d changed: level %d" % (l, lv))
        assert not np.array_equal(feats[l // 2][s], base[l // 2][s]), "row %d of the sample did not reach level %d" % (l, l // 2)


def test_style_mixed_dataset_equals_the_oracle(torch_cuda, oracle_lib):
    """generate_indexed(first_index=5, n=11, seed=3) with style_mix_prob 0.5, in chunks of the batch size 4, == Oracle.generate_w
    on the dlatents assembled on the host from Oracle.mapping of the indexed latents, mix_plan and layer_select."""
    from gan_segmentation_amd import style_mix as M
    gcfg, gp, dcfg, dp, _z, _noise = _setup("reduced", 1)
    first, n, seed, bs = 5, 11, 3, 4
    L = _layers(gcfg)
    gen = _build(gcfg, gp, dcfg, dp, bs, style_mix_prob=0.5)
    imgs, masks = [], []
    for lo in range(0, n, bs):
        img, mask = gen.generate_indexed(first + lo, min(bs, n - lo), seed=seed)
        imgs.append(img.cpu().numpy())
        masks.append(mask.cpu().numpy())
    g = gen.netG
    z, noise = g.draw_indexed(first, n, seed)
    z_b = g.draw_indexed_latents(first, n, M.mix_seed(seed))
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp)
    w_a, w_b = o.mapping(z.cpu().numpy()), o.mapping(z_b.cpu().numpy())
    mix, cutoff = M.mix_plan(seed, first, n, 0.5, L)
    assert 0 < mix.sum() < n, "precondition: the range holds mixed and unmixed samples"
    assert w_spread(w_a) > 0.1 and np.abs(w_a - w_b).max() > 0.1, "precondition: the latent sets map to different w"
    sel = M.layer_select(mix, cutoff, L)
    dl = np.where(sel[:, :, None], w_b[:, None, :], w_a[:, None, :]).astype(np.float32)
    img_o, mask_o = o.generate_w(dl, [a.cpu().numpy() for a in noise])
    _same(np.concatenate(imgs), img_o, "image")
    _same(np.concatenate(masks), mask_o, "mask")
