"""W-space synthesis on the GPU: the mapping network alone, per-layer dlatents (gsa_generator_forward_w / gsa_generate_w),
style mixing with its shard-invariant plan, the truncation override, and the two config keys of `main.py generate`."""
import ctypes

import numpy as np
import pytest

from tests.common import gan_setup, lively, odd_setup, reduced_setup

pytestmark = pytest.mark.gpu


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    assert np.array_equal(a, b), "%s: %d of %d values differ" % (what, int((a != b).sum()), a.size)


def _setup(kind, batch):
    if kind == "reduced":
        gcfg, gp, dcfg, dp, z, noise = reduced_setup(7, batch=batch)
    elif kind == "odd":
        gcfg, gp, dcfg, dp, z, noise = odd_setup(batch)
    else:
        gcfg, gp, dcfg, dp, z, noise = gan_setup("ffhq", batch)
    return gcfg, lively(gp), dcfg, dp, z, noise


def _build(gcfg, gp, dcfg, dp, batch, **kw):
    from gan_segmentation_amd.image_generator import ImageGenerator
    return ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=kw.pop("gpu_ids", [0]), batch_size=batch, **kw)


def _broadcast(w, L):
    return w[:, None, :].expand(w.shape[0], L, w.shape[1]).contiguous()


def _mixed(w_a, w_b, cutoffs, L):
    """dlatents whose sample i takes w_a for the layers l < cutoffs[i] and w_b for the rest."""
    import torch
    from gan_segmentation_amd import style_mix as M
    sel = torch.from_numpy(M.layer_select(np.ones(w_a.shape[0], bool), np.asarray(cutoffs), L)).to(w_a.device)
    return torch.where(sel[:, :, None], w_b[:, None, :], w_a[:, None, :]).contiguous()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,batch", [("reduced", 3), ("odd", 3), ("ffhq", 2)])
def test_broadcast_dlatents_equal_the_z_path(torch_cuda, kind, batch, precision):
    """dlatents[:, l] = mapping(z) for every l: synthesis == Generator(z) bit for bit (rgb, every feature, u8 image) -- the
    per-layer style kernel reproduces the z path's styles exactly, and mapping() its w."""
    gcfg, gp, dcfg, dp, z, noise = _setup(kind, batch)
    gen = _build(gcfg, gp, dcfg, dp, batch, precision=precision)
    g = gen.netG
    rgb, feats, img = g(z, noise=noise, want_image=True)
    w = g.mapping(z)
    assert tuple(w.shape) == (batch, 512)
    rgb_w, feats_w, img_w = g.synthesis(_broadcast(w, g.num_style_layers), noise=noise, want_image=True)
    _same(rgb_w.cpu().numpy(), rgb.cpu().numpy(), "rgb")
    _same(img_w.cpu().numpy(), img.cpu().numpy(), "image")
    assert len(feats_w) == len(feats) == gcfg["max_res_log2"] - 1
    for i, (a, b) in enumerate(zip(feats_w, feats)):
        _same(a.cpu().numpy(), b.cpu().numpy(), "feature %d" % i)


def test_fused_w_step_equals_two_calls(torch_cuda):
    """gsa_generate_w == gsa_generator_forward_w + gsa_decoder_forward, bitwise, on mixed dlatents."""
    import torch
    gcfg, gp, dcfg, dp, z, noise = _setup("reduced", 4)
    gen = _build(gcfg, gp, dcfg, dp, 4)
    g = gen.netG
    zb = torch.from_numpy(np.random.default_rng(5).standard_normal(z.shape).astype(np.float32))
    dl = _mixed(g.mapping(z), g.mapping(zb), [1, 4, 7, g.num_style_layers - 1], g.num_style_layers)
    img, mask = gen.generate_batch_w(dl, noise)
    rgb, feats, img2 = g.synthesis(dl, noise=noise, want_image=True)
    _logits, mask2 = gen._decoder(*feats, want_mask=True)
    _same(img.cpu().numpy(), img2.cpu().numpy(), "image")
    _same(mask.cpu().numpy(), mask2.cpu().numpy(), "mask")
    # the z path is not what ran: the mixed samples differ from it
    img_z, _mask_z = gen.generate_batch(z, noise)
    assert not np.array_equal(img.cpu().numpy(), img_z.cpu().numpy())


def _semantic_mixed(gcfg, gp, dcfg, dp, z_a, z_b, cutoffs, noise):
    """Torch composition of the reference-order restatement: per-sample layer routing of mapping(z_a) / mapping(z_b)."""
    import torch
    from gan_segmentation_amd import style_mix as M
    from oracle import ref_semantic as S
    with torch.no_grad():
        G = S.SemanticGenerator(gcfg, gp)
        w_a, w_b = G.mapping(torch.from_numpy(z_a)).numpy(), G.mapping(torch.from_numpy(z_b)).numpy()
    L = 2 * (gcfg["max_res_log2"] - 1)
    sel = M.layer_select(np.ones(len(cutoffs), bool), np.asarray(cutoffs), L)
    dl = np.where(sel[:, :, None], w_b[:, None, :], w_a[:, None, :])
    rgb, _feats, logits = S.synthesis(gcfg, gp, dcfg, dp, dl, noise)
    return rgb, logits


@pytest.mark.parametrize("kind,cutoffs", [("reduced", [1, 2, 3, 11]), ("ffhq", [8, 8])])
def test_style_routing(torch_cuda, kind, cutoffs):
    """Mixed dlatents with the given cutoffs: the features of the levels fed only by layers < cutoff are those of the pure
    z_a run bit for bit, a later level differs, rgb / logits are within 1e-3 of the torch composition of the
    reference-order restatement (the bar of test_semantic_tolerance), and rgb / features / logits equal Oracle.generator_w."""
    import torch
    n = len(cutoffs)
    gcfg, gp, dcfg, dp, z, noise = _setup(kind, n)
    z_b = np.random.default_rng(9).standard_normal(z.shape).astype(np.float32)
    gen = _build(gcfg, gp, dcfg, dp, n)
    g = gen.netG
    L = g.num_style_layers
    assert max(cutoffs) == L - 1 or kind == "ffhq"
    dl = _mixed(g.mapping(z), g.mapping(torch.from_numpy(z_b)), cutoffs, L)
    rgb, feats = g.synthesis(dl, noise=noise)
    logits, _mask = gen._decoder(*feats, want_mask=True)
    _rgb_a, feats_a = g(z, noise=noise)
    for i, c in enumerate(cutoffs):
        for lv in range(len(feats)):
            a, b = feats[lv][i].cpu().numpy(), feats_a[lv][i].cpu().numpy()
            if lv < c // 2:
                _same(a, b, "sample %d level %d (cutoff %d)" % (i, lv, c))
        assert not np.array_equal(feats[-1][i].cpu().numpy(), feats_a[-1][i].cpu().numpy()), "sample %d: w_b unused" % i
    srgb, slog = _semantic_mixed(gcfg, gp, dcfg, dp, np.asarray(z, np.float32), z_b, cutoffs, noise)
    assert np.abs(rgb.cpu().numpy() - srgb).max() <= 1e-3
    assert np.abs(logits.cpu().numpy() - slog).max() <= 1e-3
    # and bit for bit the C oracle on the same dlatents (full size: the first sample only, to bound the oracle's time)
    from oracle.binding import Oracle
    o = Oracle(gcfg, gp, dcfg, dp)
    k = n if kind == "reduced" else 1
    rgb_o, _img_o, feats_o = o.generator_w(dl[:k].cpu().numpy(), [np.asarray(a)[:k] for a in noise])
    logits_o, _mask_o = o.decoder(feats_o)
    _same(rgb.cpu().numpy()[:k], rgb_o, "rgb vs the oracle")
    for lv, f in enumerate(feats_o):
        _same(feats[lv].cpu().numpy()[:k], f, "feature %d vs the oracle" % lv)
    _same(logits.cpu().numpy()[:k], logits_o, "logits vs the oracle")


@pytest.mark.parametrize("psi", [0.5, "per-layer"])
def test_truncation_override_matches_the_oracle(torch_cuda, oracle_lib, psi):
    """from_params(truncation_psi=v) == the C oracle loaded with truncation_psi = v, bit for bit, through the z path and
    through gsa_generate_w with broadcast dlatents."""
    gcfg, gp, dcfg, dp, z, noise = _setup("reduced", 3)
    from gan_segmentation_amd import weights as W
    L = W.num_style_layers(gcfg)
    v = 0.5 if psi == 0.5 else list(np.linspace(0.25, 1.1, L))
    gen = _build(gcfg, gp, dcfg, dp, 3, truncation_psi=v)
    img, mask = gen.generate_batch(z, noise)
    gp_v = dict(gp)
    gp_v["truncation_psi"] = np.broadcast_to(np.asarray(v, np.float32), (L,)).copy()
    img_o, mask_o = oracle_lib.Oracle(gcfg, gp_v, dcfg, dp).generate(z, noise)
    _same(img.cpu().numpy(), img_o, "image (z path)")
    _same(mask.cpu().numpy(), mask_o, "mask (z path)")
    img_w, mask_w = gen.generate_batch_w(_broadcast(gen.netG.mapping(z), L), noise)
    _same(img_w.cpu().numpy(), img_o, "image (W path)")
    _same(mask_w.cpu().numpy(), mask_o, "mask (W path)")
    img_d, _ = oracle_lib.Oracle(gcfg, gp, dcfg, dp).generate(z, noise)
    assert not np.array_equal(img_d, img_o)       # the override changed what was sampled


def test_style_mixed_dataset_is_shard_invariant(torch_cuda):
    """generate_indexed with style_mix_prob 0.5: the batch of 6 == 2 ++ 4 == the same call over two replicas; the unmixed
    samples equal the z path, the mixed ones do not."""
    from gan_segmentation_amd import style_mix as M
    gcfg, gp, dcfg, dp, _z, _noise = _setup("reduced", 1)
    seed = 0
    mix, _cut = M.mix_plan(seed, 0, 6, 0.5, 12)
    assert 0 < mix.sum() < 6
    gen = _build(gcfg, gp, dcfg, dp, 6, style_mix_prob=0.5)
    img, mask = [t.cpu().numpy() for t in gen.generate_indexed(0, 6, seed=seed)]
    parts = [gen.generate_indexed(0, 2, seed=seed), gen.generate_indexed(2, 4, seed=seed)]
    _same(np.concatenate([p[0].cpu().numpy() for p in parts]), img, "image 0..5 vs 0..1 ++ 2..5")
    _same(np.concatenate([p[1].cpu().numpy() for p in parts]), mask, "mask 0..5 vs 0..1 ++ 2..5")
    two = _build(gcfg, gp, dcfg, dp, 6, style_mix_prob=0.5, gpu_ids=[0, 0])
    img2, mask2 = two.generate_indexed(0, 6, seed=seed)
    _same(img2.cpu().numpy(), img, "image over two replicas")
    _same(mask2.cpu().numpy(), mask, "mask over two replicas")
    plain = _build(gcfg, gp, dcfg, dp, 6)
    img_z = plain.generate_indexed(0, 6, seed=seed)[0].cpu().numpy()
    for i in range(6):
        assert np.array_equal(img[i], img_z[i]) != bool(mix[i]), i


def test_w_entries_validate_their_arguments(torch_cuda):
    """Wrong num_layers or a null dlatents pointer: GSA_ERR_INVALID; a batch above the reserve: GSA_ERR_STATE; the context
    stays usable."""
    import torch
    gcfg, gp, dcfg, dp, z, noise = _setup("reduced", 2)
    gen = _build(gcfg, gp, dcfg, dp, 2)
    g = gen.netG
    L = g.num_style_layers
    w = g.mapping(z)                                  # reserves 2
    dl = _broadcast(w, L)
    ctx = g._model.ctx
    api, h = ctx.api, ctx._h
    dev = g._model.device
    s = torch.cuda.current_stream(dev).cuda_stream
    nz = [torch.from_numpy(a).to(dev) for a in noise]
    nzp = (ctypes.c_void_p * len(nz))(*[a.data_ptr() for a in nz])
    R = 2 ** gcfg["max_res_log2"]
    img = torch.empty((2, R, R, 3), device=dev, dtype=torch.uint8)
    mask = torch.empty((2, R, R), device=dev, dtype=torch.uint8)
    rgb = torch.empty((2, 3, R, R), device=dev, dtype=torch.float32)
    big = torch.zeros((3, L, 512), device=dev)
    assert api.generate_w(h, s, 2, dl.data_ptr(), L + 1, nzp, len(nz), img.data_ptr(), mask.data_ptr()) == -1
    assert api.generate_w(h, s, 2, None, L, nzp, len(nz), img.data_ptr(), mask.data_ptr()) == -1
    assert api.generate_w(h, s, 3, big.data_ptr(), L, nzp, len(nz), img.data_ptr(), mask.data_ptr()) == -2
    assert api.generator_forward_w(h, s, 2, dl.data_ptr(), L - 1, nzp, len(nz), rgb.data_ptr(), None, None, 0) == -1
    assert api.generator_forward_w(h, s, 2, None, L, nzp, len(nz), rgb.data_ptr(), None, None, 0) == -1
    assert api.generator_forward_w(h, s, 3, big.data_ptr(), L, nzp, len(nz), rgb.data_ptr(), None, None, 0) == -2
    assert api.mapping_forward(h, s, 3, big.data_ptr(), big.data_ptr()) == -2
    assert api.mapping_forward(h, s, 2, None, w.data_ptr()) == -1
    assert b"layers" in api.last_error(h) or b"null" in api.last_error(h)
    img_w, mask_w = gen.generate_batch_w(dl, noise)
    img_z, mask_z = gen.generate_batch(z, noise)
    _same(img_w.cpu().numpy(), img_z.cpu().numpy(), "image after the refused calls")
    _same(mask_w.cpu().numpy(), mask_z.cpu().numpy(), "mask after the refused calls")
    ctx.check()


def _cli_dirs(tmp_path, name):
    import yaml
    from gan_segmentation_amd import params as P
    from gan_segmentation_amd import weights as W
    gcfg, dcfg = W.generator_config(8), W.decoder_config(8)      # bedrooms, 256 px
    root = tmp_path / name
    gan_dir, base = root / "stylegan-models", root / "exp"
    gan_dir.mkdir(parents=True)
    (base / "checkpoints").mkdir(parents=True)
    gp, dp = lively(W.synthetic_generator_params(gcfg)), W.synthetic_decoder_params(dcfg)
    P.save_params(str(gan_dir / "stylegan-bedrooms.params"), W.generator_names_to_scheme_s(gp))
    P.save_params(str(base / "checkpoints" / "checkpoint_last.params"), dp)
    cfg = {"BASE_DIR": str(base), "GAN": "bedrooms", "GAN_DIR": str(gan_dir), "GAN_GPU_IDS": [0],
           "GAN_BATCH_SIZE_PER_GPU": 2, "SOLVER_GPU_IDS": [0], "ANNOTATION": "segmentation", "GENERATE_NUM": 3}

    def run(**keys):
        c = dict(cfg, **keys)
        (root / "config.yml").write_text(yaml.safe_dump(c))
        from gan_segmentation_amd import main as cli
        assert cli.main(["generate", "--config", str(root / "config.yml")]) == 0
        return base / "dataset" / "train_generated"
    return gcfg, gp, dcfg, dp, run


def test_cli_style_mix_and_truncation_keys(torch_cuda, tmp_path):
    """STYLE_MIX_PROB / TRUNCATION_PSI of `main.py generate`: the masks written equal the API run with the same plan; a run
    with STYLE_MIX_PROB 0 writes the same bytes as one without the key."""
    from PIL import Image
    gcfg, gp, dcfg, dp, run = _cli_dirs(tmp_path, "mixed")
    out = run(STYLE_MIX_PROB=1.0, TRUNCATION_PSI=0.6)
    gen = _build(gcfg, gp, dcfg, dp, 2, truncation_psi=0.6, style_mix_prob=1.0)
    masks = np.concatenate([gen.generate_indexed(0, 2)[1].cpu().numpy(), gen.generate_indexed(2, 1)[1].cpu().numpy()])
    for i in range(3):
        _same(np.asarray(Image.open(out / ("mask_%06d.png" % i))), masks[i], "mask %d" % i)
    plain = _build(gcfg, gp, dcfg, dp, 2)
    assert not np.array_equal(plain.generate_indexed(0, 2)[1].cpu().numpy(), masks[:2])

    _g, _p, _d, _q, run_a = _cli_dirs(tmp_path, "without_key")
    _g, _p, _d, _q, run_b = _cli_dirs(tmp_path, "prob_zero")
    out_a, out_b = run_a(), run_b(STYLE_MIX_PROB=0)
    names = sorted(p.name for p in out_a.iterdir())
    assert names == sorted(p.name for p in out_b.iterdir()) and len(names) == 6
    for nm in names:
        assert (out_a / nm).read_bytes() == (out_b / nm).read_bytes(), nm
