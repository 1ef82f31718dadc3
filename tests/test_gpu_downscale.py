"""Downscaled pairs on the GPU (include/gsa.h gsa_generate_downscaled; ImageGenerator(output_downscale=f); the OUTPUT_DOWNSCALE
key of `main.py generate`): bit for bit the rule of tests/test_downscale_host.py applied to the full-size fp32 outputs -- toRGB's
rgb and the decoder's logits -- of the C oracle and of the GPU's own unfused entries."""
import ctypes

import numpy as np
import pytest

from gan_segmentation_amd import weights as W
from tests.common import gan_setup, lively, odd_setup, reduced_setup
from tests.test_downscale_host import block_sum, rule_image, rule_mask

pytestmark = pytest.mark.gpu


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, "%s: shape %s vs %s" % (what, a.shape, b.shape)
    assert np.array_equal(a, b), "%s: %d of %d values differ" % (what, int((a != b).sum()), a.size)


def _setup(kind, batch, ncls=2):
    if kind == "reduced":
        gcfg, gp, dcfg, dp, z, noise = reduced_setup(7, batch=batch)
    elif kind == "odd":
        gcfg, gp, dcfg, dp, z, noise = odd_setup(batch)
    else:
        gcfg, gp, dcfg, dp, z, noise = gan_setup(kind, batch)
    if ncls != dcfg["features"][-1]:
        dcfg = dict(dcfg, features=list(dcfg["features"][:-1]) + [ncls])
        dp = W.synthetic_decoder_params(dcfg, seed=7)
    return gcfg, lively(gp), dcfg, dp, z, noise


def _build(gcfg, gp, dcfg, dp, batch, **kw):
    from gan_segmentation_amd.image_generator import ImageGenerator
    return ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=kw.pop("gpu_ids", [0]), batch_size=batch, **kw)


def _unfused(gen, z, noise):
    """rgb and logits of the GPU's own full-size entries (gsa_generator_forward + gsa_decoder_forward)."""
    rgb, feats = gen.netG(z, noise=noise)
    logits = gen._decoder(*feats)
    return rgb.cpu().numpy(), logits.cpu().numpy()


def _pair(gen, *args, **kw):
    img, mask = gen.generate_batch(*args, **kw)
    return img.cpu().numpy(), mask.cpu().numpy()


@pytest.mark.parametrize("ncls", [2, 3])
@pytest.mark.parametrize("kind", ["reduced", "odd"])
def test_downscaled_pair_matches_the_rule_on_the_oracle(torch_cuda, oracle_lib, kind, ncls):
    """generate_batch at f = 2, 4, 8 == the rule on Oracle.generator's rgb and Oracle.decoder's logits, bit for bit; and the test
    tells the rule from nearest subsampling of the mask and from averaging the truncated image."""
    gcfg, gp, dcfg, dp, z, noise = _setup(kind, 3, ncls)
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp)
    rgb_o, img_o, feats_o = o.generator(z, noise)
    logits_o, mask_o = o.decoder(feats_o)
    nearest_differs = after_truncation_differs = False
    for f in (2, 4, 8):
        img, mask = _pair(_build(gcfg, gp, dcfg, dp, 3, output_downscale=f), z, noise)
        R = 2 ** gcfg["max_res_log2"] // f
        assert img.shape == (3, R, R, gcfg["channels"]) and mask.shape == (3, R, R)
        _same(img, rule_image(rgb_o, f), "image f=%d" % f)
        _same(mask, rule_mask(logits_o, f), "mask f=%d" % f)
        nearest_differs |= not np.array_equal(mask, mask_o[:, ::f, ::f])
        mean_u8 = (block_sum(img_o.transpose(0, 3, 1, 2).astype(np.float32), f) * np.float32(1.0 / (f * f))).astype(np.uint8)
        after_truncation_differs |= not np.array_equal(img, mean_u8.transpose(0, 2, 3, 1))
    assert nearest_differs, "no block's mask differs from its top-left pixel's class: the test cannot tell the rules apart"
    assert after_truncation_differs, "no image value differs from the mean of the u8 image: the test cannot tell the rules apart"


@pytest.mark.parametrize("gan,factors,batch", [("ffhq", (2, 4), 2), ("cars", (2,), 2), ("bedrooms", (2,), 2)])
def test_full_size_configs_match_the_rule(torch_cuda, gan, factors, batch):
    """The real resolutions (16 / 32 / 64 channels at the last level), fp32: the rule on the GPU's own rgb and logits."""
    gcfg, gp, dcfg, dp, z, noise = _setup(gan, batch)
    gen = _build(gcfg, gp, dcfg, dp, batch)
    rgb, logits = _unfused(gen, z, noise)
    for f in factors:
        img, mask = _pair(_build(gcfg, gp, dcfg, dp, batch, output_downscale=f), z, noise)
        _same(img, rule_image(rgb, f), "%s image f=%d" % (gan, f))
        _same(mask, rule_mask(logits, f), "%s mask f=%d" % (gan, f))


@pytest.mark.parametrize("kind,ncls", [("reduced", 2), ("odd", 3)])
def test_bf16_downscaled_pair(torch_cuda, oracle_lib, kind, ncls):
    """bf16 mode: bit for bit the rule on the bf16 GPU's own rgb and logits.  The bf16 oracle is not the GPU's bits (the matrix
    cores sum in their own order: tests/test_gpu_bf16.py), so against the rule on its outputs the bars of that file apply: the
    masks agree on >= 99.5 % of the pixels, the images within 1 level on average."""
    gcfg, gp, dcfg, dp, z, noise = _setup(kind, 3, ncls)
    rgb, logits = _unfused(_build(gcfg, gp, dcfg, dp, 3, precision="bf16"), z, noise)
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp, precision="bf16")
    rgb_o, _img_o, feats_o = o.generator(z, noise)
    logits_o, _mask_o = o.decoder(feats_o)
    for f in (2, 4, 8):
        img, mask = _pair(_build(gcfg, gp, dcfg, dp, 3, precision="bf16", output_downscale=f), z, noise)
        _same(img, rule_image(rgb, f), "bf16 image f=%d" % f)
        _same(mask, rule_mask(logits, f), "bf16 mask f=%d" % f)
        agree = float(np.mean(mask == rule_mask(logits_o, f)))
        d = np.abs(img.astype(np.int32) - rule_image(rgb_o, f).astype(np.int32)).mean()
        assert agree >= 0.995 and d <= 1.0, "f=%d vs the bf16 oracle: masks agree on %.4f, images differ by %.3f on average" % (f, agree, d)


def _device_inputs(gen, z, noise):
    import torch
    dev = gen.netG._model.device
    return torch.from_numpy(np.asarray(z)).to(dev), [torch.from_numpy(np.asarray(a)).to(dev) for a in noise]


def test_factor_one_is_generate_and_generate_w(torch_cuda):
    """gsa_generate_downscaled at factor 1 writes the bytes of gsa_generate (z) and of gsa_generate_w (dlatents)."""
    import torch
    gcfg, gp, dcfg, dp, z, noise = _setup("odd", 3)
    gen = _build(gcfg, gp, dcfg, dp, 3)
    g = gen.netG
    ctx, dev = g._model.ctx, g._model.device
    zt, nt = _device_inputs(gen, z, noise)
    g._model.ensure_batch(3)
    s = torch.cuda.current_stream(dev).cuda_stream
    nptrs = [a.data_ptr() for a in nt]
    R, L = 2 ** gcfg["max_res_log2"], g.num_style_layers
    outs = [(torch.full((3, R, R, 3), 7, device=dev, dtype=torch.uint8), torch.full((3, R, R), 7, device=dev, dtype=torch.uint8))
            for _ in range(4)]
    dl = torch.from_numpy(np.random.default_rng(4).standard_normal((3, L, 512)).astype(np.float32)).to(dev)
    ctx.generate(s, 3, zt.data_ptr(), nptrs, outs[0][0].data_ptr(), outs[0][1].data_ptr())
    ctx.generate_downscaled(s, 3, zt.data_ptr(), None, 0, nptrs, 1, outs[1][0].data_ptr(), outs[1][1].data_ptr())
    ctx.generate_w(s, 3, dl.data_ptr(), L, nptrs, outs[2][0].data_ptr(), outs[2][1].data_ptr())
    ctx.generate_downscaled(s, 3, None, dl.data_ptr(), L, nptrs, 1, outs[3][0].data_ptr(), outs[3][1].data_ptr())
    o = [(a.cpu().numpy(), b.cpu().numpy()) for a, b in outs]
    _same(o[1][0], o[0][0], "image, z")
    _same(o[1][1], o[0][1], "mask, z")
    _same(o[3][0], o[2][0], "image, dlatents")
    _same(o[3][1], o[2][1], "mask, dlatents")
    assert not np.array_equal(o[0][0], o[2][0])


def test_style_mixed_indexed_batches(torch_cuda):
    """A style-mixed generate_indexed at f = 2 == the rule on the W path's unfused outputs; (0, 4) == (0, 2) ++ (2, 2)."""
    gcfg, gp, dcfg, dp, _z, _noise = _setup("reduced", 1)
    gen = _build(gcfg, gp, dcfg, dp, 4, style_mix_prob=0.5, output_downscale=2)
    img, mask = [t.cpu().numpy() for t in gen.generate_indexed(0, 4, seed=3)]
    g = gen.netG
    dl, noise = gen._mixed_dlatents(g, 0, 4, 3)
    rgb, feats = g.synthesis(dl, noise=noise)
    logits = gen._decoder(*feats).cpu().numpy()
    _same(img, rule_image(rgb.cpu().numpy(), 2), "mixed image")
    _same(mask, rule_mask(logits, 2), "mixed mask")
    parts = [gen.generate_indexed(0, 2, seed=3), gen.generate_indexed(2, 2, seed=3)]
    _same(np.concatenate([p[0].cpu().numpy() for p in parts]), img, "image 0..3 vs 0..1 ++ 2..3")
    _same(np.concatenate([p[1].cpu().numpy() for p in parts]), mask, "mask 0..3 vs 0..1 ++ 2..3")
    plain = _build(gcfg, gp, dcfg, dp, 4, output_downscale=2)
    img_p, mask_p = [t.cpu().numpy() for t in plain.generate_indexed(0, 4, seed=3)]
    parts = [plain.generate_indexed(0, 2, seed=3), plain.generate_indexed(2, 2, seed=3)]
    _same(np.concatenate([p[0].cpu().numpy() for p in parts]), img_p, "z path image 0..3 vs 0..1 ++ 2..3")
    _same(np.concatenate([p[1].cpu().numpy() for p in parts]), mask_p, "z path mask 0..3 vs 0..1 ++ 2..3")
    two = _build(gcfg, gp, dcfg, dp, 4, style_mix_prob=0.5, output_downscale=2, gpu_ids=[0, 0])
    img2, mask2 = two.generate_indexed(0, 4, seed=3)
    _same(img2.cpu().numpy(), img, "image over two replicas")
    _same(mask2.cpu().numpy(), mask, "mask over two replicas")


def test_graph_replay_of_downscaled_steps(torch_cuda, monkeypatch):
    """GSA_GRAPH=1: 40 calls at batch 2 into the same tensors, rewritten in place -- the captured replays equal the eager step."""
    monkeypatch.setenv("GSA_GRAPH", "1")
    gcfg, gp, dcfg, dp, z, noise = _setup("reduced", 4)
    eager = _build(gcfg, gp, dcfg, dp, 2, output_downscale=2)
    eager.graph_mode = "0"
    want = [_pair(eager, z[k:k + 2], [a[k:k + 2] for a in noise]) for k in (0, 2)]
    gen = _build(gcfg, gp, dcfg, dp, 2, output_downscale=2)
    zt = torch_cuda.from_numpy(z[:2].copy()).cuda()
    nt = [torch_cuda.from_numpy(a[:2].copy()).cuda() for a in noise]
    out = (torch_cuda.empty((2, 64, 64, 3), dtype=torch_cuda.uint8, device="cuda"),
           torch_cuda.empty((2, 64, 64), dtype=torch_cuda.uint8, device="cuda"))
    for it in range(40):
        k = 0 if it % 2 == 0 else 2
        zt.copy_(torch_cuda.from_numpy(z[k:k + 2].copy()))
        for t, a in zip(nt, noise):
            t.copy_(torch_cuda.from_numpy(a[k:k + 2].copy()))
        out[0].zero_(); out[1].zero_()
        img, mask = gen.generate_batch(zt, nt, out=out)
        _same(img.cpu().numpy(), want[k // 2][0], "image, call %d" % it)
        _same(mask.cpu().numpy(), want[k // 2][1], "mask, call %d" % it)
    assert len(gen.netG._model.__dict__.get("_graphs", {})) == 1, "the repeated call was never captured"


def test_downscaled_entry_validates_its_arguments(torch_cuda):
    """Factors 3 and 16, an output under 16 px, both or neither of z and dlatents, a wrong num_layers: GSA_ERR_INVALID; wrong out
    shapes: ValueError.  The context stays usable."""
    import torch
    gcfg, gp, dcfg, dp, z, noise = _setup("reduced", 2)
    gen = _build(gcfg, gp, dcfg, dp, 2, output_downscale=2)
    img0, mask0 = _pair(gen, z, noise)
    g = gen.netG
    ctx, dev = g._model.ctx, g._model.device
    api, h = ctx.api, ctx._h
    zt, nt = _device_inputs(gen, z, noise)
    s = torch.cuda.current_stream(dev).cuda_stream
    nzp = (ctypes.c_void_p * len(nt))(*[a.data_ptr() for a in nt])
    L = g.num_style_layers
    dl = torch.zeros((2, L, 512), device=dev)
    img = torch.empty((2, 128, 128, 3), device=dev, dtype=torch.uint8)
    mask = torch.empty((2, 128, 128), device=dev, dtype=torch.uint8)
    ip, mp = img.data_ptr(), mask.data_ptr()
    for f in (3, 16, 0, -2):
        assert api.generate_downscaled(h, s, 2, zt.data_ptr(), None, 0, nzp, len(nt), f, ip, mp) == -1, f
    assert b"factor" in api.last_error(h)
    assert api.generate_downscaled(h, s, 2, zt.data_ptr(), dl.data_ptr(), L, nzp, len(nt), 2, ip, mp) == -1
    assert api.generate_downscaled(h, s, 2, None, None, L, nzp, len(nt), 2, ip, mp) == -1
    assert api.generate_downscaled(h, s, 2, None, dl.data_ptr(), L + 1, nzp, len(nt), 2, ip, mp) == -1
    assert b"layers" in api.last_error(h)
    assert api.generate_downscaled(h, s, 2, zt.data_ptr(), None, 0, nzp, len(nt) - 1, 2, ip, mp) == -1
    # an output under 16 px: 64 px at factor 8
    sg = _setup_small()
    small = _build(*sg[:4], 2)
    sctx = small.netG._model.ctx
    small.netG._model.ensure_batch(2)
    szt, snt = _device_inputs(small, sg[4], sg[5])
    sp = (ctypes.c_void_p * len(snt))(*[a.data_ptr() for a in snt])
    assert sctx.api.generate_downscaled(sctx._h, s, 2, szt.data_ptr(), None, 0, sp, len(snt), 8, ip, mp) == -1
    assert b"16" in sctx.api.last_error(sctx._h)
    for bad in ((img, mask), (img[:, :64, :64].contiguous(), mask), (torch.empty((2, 64, 64, 3), device=dev, dtype=torch.uint8),
                                                                        torch.empty((2, 64, 63), device=dev, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            gen.generate_batch(z, noise, out=bad)
    img1, mask1 = _pair(gen, z, noise)
    _same(img1, img0, "image after the refused calls")
    _same(mask1, mask0, "mask after the refused calls")
    ctx.check()


def _setup_small():
    gcfg, gp, dcfg, dp, z, noise = reduced_setup(6, batch=2, seed=6)
    return gcfg, gp, dcfg, dp, z, noise


def test_profile_labels_of_the_downscaled_launches(torch_cuda):
    """Profile level 2 labels the two new launches by their demangled gsa:: kernels; the full-size toRGB and final conv do not run."""
    import re
    for precision in ("fp32", "bf16"):
        gcfg, gp, dcfg, dp, z, noise = _setup("reduced", 2)
        gen = _build(gcfg, gp, dcfg, dp, 2, precision=precision, output_downscale=4)
        ctx = gen.netG._model.ctx
        gen.generate_batch(z, noise)
        ctx.profile_enable(2)
        ctx.profile_reset()
        gen.generate_batch(z, noise)
        torch_cuda.cuda.synchronize()
        entries = ctx.profile_entries()
        ctx.profile_enable(0)
        layers = {}
        for e in entries:
            kernel, _, layer = e["name"].partition(" | ")
            assert re.match(r"^(void )?gsa::\S.*\)$", kernel), e["name"]
            layers[layer] = kernel
        last = gcfg["max_res_log2"] - 2
        assert "torgb_down_kernel<4, %s>" % ("true" if precision == "bf16" else "false") in layers["g.torgb_down"], layers
        assert "final_conv_down_kernel<2, 4, " in layers["d.final_%d_down" % last], layers
        assert "g.torgb" not in layers and "d.final_%d" % last not in layers and not any("+torgb" in k for k in layers), layers


def _cli_dirs(tmp_path, name):
    import yaml
    from gan_segmentation_amd import params as P
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

    def run(action="generate", extra=(), **keys):
        c = dict(cfg, **keys)
        (root / "config.yml").write_text(yaml.safe_dump(c))
        from gan_segmentation_amd import main as cli
        assert cli.main([action, "--config", str(root / "config.yml")] + list(extra)) == 0
        return base
    return gcfg, gp, dcfg, dp, run


def test_cli_output_downscale_key(torch_cuda, tmp_path):
    """OUTPUT_DOWNSCALE: 2 on bedrooms writes 128 x 128 img_*.jpg / mask_*.png; each mask is generate_indexed's at the same seed;
    `annotation --count` stays at 256 px."""
    from PIL import Image
    gcfg, gp, dcfg, dp, run = _cli_dirs(tmp_path, "down")
    base = run(OUTPUT_DOWNSCALE=2)
    out = base / "dataset" / "train_generated"
    gen = _build(gcfg, gp, dcfg, dp, 2, output_downscale=2)
    masks = np.concatenate([gen.generate_indexed(0, 2)[1].cpu().numpy(), gen.generate_indexed(2, 1)[1].cpu().numpy()])
    assert masks.shape == (3, 128, 128)
    for i in range(3):
        im = Image.open(out / ("img_%06d.jpg" % i))
        assert im.size == (128, 128) and im.mode == "RGB"
        _same(np.asarray(Image.open(out / ("mask_%06d.png" % i))), masks[i], "mask %d" % i)
    assert len(list(out.iterdir())) == 6
    base = run("annotation", ["--count", "1"], OUTPUT_DOWNSCALE=2)
    assert Image.open(base / "data" / "img_000000.jpg").size == (256, 256)
