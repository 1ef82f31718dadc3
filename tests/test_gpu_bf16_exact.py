"""The bf16 path bit for bit against the bf16 oracle, on exactly summable models (tests/exact_bf16.py).

On general weights the bf16 HIP path and the oracle's bf16 mode agree only within a tolerance (tests/test_gpu_bf16.py): the matrix core
adds its products in an order of its own, and instance norm amplifies each flipped rounding.  On the fixtures used here every
matrix-core accumulation is exactly summable -- all products multiples of one power of two q, sum|product| < 2^22 q, asserted on the
oracle alone by tests/test_exact_bf16_host.py -- so no order of summation can change a bit, and everything else is the same fp32 code
on both sides.  Every tensor of every level must then have the oracle's bytes: a weight repack that swaps two channels on one tap, a
border pixel staged from the wrong row, a store that truncates instead of rounding, a stale AdaIN coefficient all show up here, at the
level where they happen.

A failure names the first differing tensor, the kernels the profile labels (level 2) give for that level, and the count and position of
the differing values.  The coverage test at the end holds the set of convolution kernels these fixtures launch against what cars 512^2
launches in bf16 mode.
"""
import functools
import re

import numpy as np
import pytest

from tests.dispatch_map import PATHS, path_map
from tests.exact_bf16 import EXACT_CASES, checked_samples, exact_dlatents, exact_setup, take
from tests.test_downscale_host import rule_image, rule_mask

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _expected(name, batch):
    """The oracle's tensors for checked_samples(batch): z path, W path."""
    from oracle.binding import Oracle
    gcfg, gp, dcfg, dp, z, noise = exact_setup(name, batch)
    o = Oracle(gcfg, gp, dcfg, dp, precision="bf16", witness=True)
    idx = checked_samples(batch)
    zc, nc = take(z, noise, idx)
    out = {}
    dl = exact_dlatents(o, gcfg, batch)
    for path in ("z", "w"):
        rgb, img, feats = o.generator(zc, nc) if path == "z" else o.generator_w(dl[idx], nc)
        logits, mask = o.decoder(feats)
        out[path] = dict(rgb=rgb, img=img, feats=feats, logits=logits, mask=mask)
    out["headroom"] = o.exact_headroom()
    assert out["headroom"] >= 2.0, "the fixture is not exactly summable: headroom %.2f bits" % out["headroom"]
    out["dlatents"] = dl
    return out


@functools.lru_cache(maxsize=None)
def _built(name, batch):
    """(generator, inputs on the device) of a case, eager; one per module run."""
    import torch
    from gan_segmentation_amd.image_generator import ImageGenerator
    gcfg, gp, dcfg, dp, z, noise = exact_setup(name, batch)
    gen = ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=batch, precision="bf16")
    gen.graph_mode = "0"
    dev = gen.netG._model.device
    return gen, torch.from_numpy(z).to(dev), [torch.from_numpy(a).to(dev) for a in noise]


def _kernels_of(pairs, what):
    """The launched kernels (profile labels) that belong to a tensor: those of its resolution level, or all of a stage."""
    m = re.match(r"feature (\d+)", what)
    res = "%d" % (4 << int(m.group(1))) if m else None
    hit = sorted("%s <- %s" % (layer, kernel) for layer, kernel in pairs if res is None or re.search(r"(?<!\d)%s(?!\d)" % res, layer))
    return "\n    ".join(hit if hit else sorted("%s <- %s" % p for p in pairs))


def _assert_same(tensors, idx, pairs, case):
    """tensors: [(what, got (device tensor or array), want)] in the order the step computes them; the first that differs fails."""
    for what, got, want in tensors:
        got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
        got = got[idx] if idx is not None else got
        assert got.shape == want.shape and got.dtype == want.dtype, "%s %s: %s %s vs %s %s" % (case, what, got.dtype, got.shape, want.dtype, want.shape)
        if np.array_equal(got, want):
            continue
        d = np.argwhere(got != want)
        first = tuple(int(v) for v in d[0])
        planes = sorted({(int(a), int(b)) for a, b in d[:, :2]})
        raise AssertionError(
            "%s: %s is the first tensor that differs from the bf16 oracle: %d of %d values, first at %s (%r vs %r), last at %s, in %d "
            "(sample, channel or row) planes starting %s\n  launched for it:\n    %s" % (
                case, what, len(d), got.size, first, got[first], want[first], tuple(int(v) for v in d[-1]), len(planes), planes[:8],
                _kernels_of(pairs, what) if pairs else "(not profiled)"))


def _two_call(gen, z, noise):
    rgb, feats, img = gen.netG(z, noise=noise, want_image=True)
    logits, mask = gen._decoder(*feats, want_mask=True)
    return rgb, feats, img, logits, mask


def _ordered(rgb, feats, img, logits, mask, want):
    t = [("feature %d (%d px)" % (i, 4 << i), f, w) for i, (f, w) in enumerate(zip(feats, want["feats"]))]
    t += [("rgb", rgb, want["rgb"])]
    if img is not None:
        t += [("image", img, want["img"])]
    return t + [("logits", logits, want["logits"]), ("mask", mask, want["mask"])]


@pytest.mark.parametrize("name,batch", EXACT_CASES)
def test_two_call_path_has_the_oracles_bytes(torch_cuda, name, batch):
    """Every feature level, rgb, the u8 image, logits and the mask of netG(...) + decoder."""
    want = _expected(name, batch)
    gen, z, noise = _built(name, batch)
    rgb, feats, img, logits, mask = _two_call(gen, z, noise)
    pairs = path_map(gen, "two_call", z, noise, batch)
    _assert_same(_ordered(rgb, feats, img, logits, mask, want["z"]), checked_samples(batch), pairs, "%s batch %d, two calls" % (name, batch))


@pytest.mark.parametrize("name,batch", EXACT_CASES)
def test_fused_pair_has_the_oracles_bytes(torch_cuda, name, batch):
    """generate_batch: the fused z step."""
    want = _expected(name, batch)["z"]
    gen, z, noise = _built(name, batch)
    img, mask = gen.generate_batch(z, noise)
    pairs = path_map(gen, "generate", z, noise, batch)
    _assert_same([("image", img, want["img"]), ("mask", mask, want["mask"])], checked_samples(batch), pairs, "%s batch %d, generate_batch" % (name, batch))


@pytest.mark.parametrize("name,batch", EXACT_CASES)
def test_w_path_has_the_oracles_bytes(torch_cuda, name, batch):
    """synthesis() from independent per-layer rows, then the decoder, against generator_w; generate_batch_w's pair too."""
    exp = _expected(name, batch)
    want, dl = exp["w"], exp["dlatents"]
    gen, _z, noise = _built(name, batch)
    rgb, feats = gen.netG.synthesis(dl, noise=noise)
    logits, mask = gen._decoder(*feats, want_mask=True)
    case = "%s batch %d, W path" % (name, batch)
    _assert_same(_ordered(rgb, feats, None, logits, mask, want), checked_samples(batch), None, case)
    img, mask = gen.generate_batch_w(dl, noise)
    _assert_same([("image", img, want["img"]), ("mask", mask, want["mask"])], checked_samples(batch), None, case + " (generate_batch_w)")


@pytest.mark.parametrize("name,batch", EXACT_CASES)
def test_downscaled_pair_follows_the_rule_on_the_oracles_tensors(torch_cuda, name, batch):
    """gsa_generate_downscaled at f = 2: the box-filtered image and the logit-averaged mask of the ORACLE's rgb and logits."""
    import torch
    want = _expected(name, batch)["z"]
    gen, z, noise = _built(name, batch)
    g = gen.netG
    ctx, dev = g._model.ctx, g._model.device
    R = 2 ** g.max_res_log2 // 2
    g._model.ensure_batch(batch)
    img = torch.full((batch, R, R, g.nc), 7, device=dev, dtype=torch.uint8)
    mask = torch.full((batch, R, R), 7, device=dev, dtype=torch.uint8)
    ctx.generate_downscaled(torch.cuda.current_stream(dev).cuda_stream, batch, z.data_ptr(), None, 0, [a.data_ptr() for a in noise], 2,
                            img.data_ptr(), mask.data_ptr())
    _assert_same([("image f=2", img, rule_image(want["rgb"], 2)), ("mask f=2", mask, rule_mask(want["logits"], 2).astype(np.uint8))],
                 checked_samples(batch), None, "%s batch %d, downscaled" % (name, batch))


def test_default_graph_replay_has_the_oracles_bytes(torch_cuda):
    """E128 with the bf16 mode's default: the repeated fused step is captured as a hipGraph and replayed."""
    from gan_segmentation_amd.image_generator import ImageGenerator
    name, batch = "E128", 3
    want = _expected(name, batch)["z"]
    gcfg, gp, dcfg, dp, z, noise = exact_setup(name, batch)
    gen = ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=batch, precision="bf16")
    gen.graph_after = 2
    dev = gen.netG._model.device
    zt, nt = torch_cuda.from_numpy(z).to(dev), [torch_cuda.from_numpy(a).to(dev) for a in noise]
    R = 2 ** gcfg["max_res_log2"]
    out = (torch_cuda.empty((batch, R, R, 3), dtype=torch_cuda.uint8, device=dev), torch_cuda.empty((batch, R, R), dtype=torch_cuda.uint8, device=dev))
    for it in range(6):
        out[0].zero_(); out[1].zero_()
        img, mask = gen.generate_batch(zt, nt, out=out)
        _assert_same([("image", img, want["img"]), ("mask", mask, want["mask"])], None, None, "E128 batch 3, call %d" % it)
    assert gen.graphs_captured() == 1, "the repeated call was never captured"


def test_a_weight_step_on_the_device_is_the_oracles_weight_step(torch_cuda):
    """The control of the comparison itself: with one 3x3 weight of the generator and one of the decoder a step further on BOTH sides the
    bytes agree again, and they are not the unstepped model's -- the device reads those weights, and bit equality sees one step."""
    from gan_segmentation_amd.image_generator import ImageGenerator
    from oracle.binding import Oracle
    from tests.exact_bf16 import STEP
    name, batch = "E128", 3
    base = _expected(name, batch)["z"]
    gcfg, gp, dcfg, dp, z, noise = exact_setup(name, batch)
    gp2, dp2 = dict(gp), dict(dp)
    for params, key in ((gp2, "8_conv_2_weight"), (dp2, "main_block_2.1.base_layers.3.weight")):
        params[key] = params[key].copy()
        params[key][1, 2, 0, 0] += np.float32(STEP)
    o = Oracle(gcfg, gp2, dcfg, dp2, precision="bf16", witness=True)
    rgb_o, img_o, feats_o = o.generator(z, noise)
    logits_o, mask_o = o.decoder(feats_o)
    assert o.exact_headroom() >= 2.0
    assert not np.array_equal(feats_o[1], base["feats"][1]) and not np.array_equal(rgb_o, base["rgb"])
    assert not np.array_equal(o.decoder(base["feats"])[0], base["logits"]), "the decoder step alone must show in the logits"
    gen = ImageGenerator.from_params(gcfg, gp2, dcfg, dp2, gpu_ids=[0], batch_size=batch, precision="bf16")
    gen.graph_mode = "0"
    rgb, feats, img, logits, mask = _two_call(gen, z, noise)
    _assert_same(_ordered(rgb, feats, img, logits, mask, dict(rgb=rgb_o, img=img_o, feats=feats_o, logits=logits_o, mask=mask_o)), None, None,
                 "E128 batch 3, one weight step")


# ---- coverage: what cars 512^2 launches in bf16 mode, these fixtures launch too -------------------------------------------------------

_FAMILIES = ("conv3x3", "subpixel", "deconv", "post", "up2")     # convolution, stride-2 and post families

# kernel signature (as the profile labels spell it) -> why no fixture launches it.  Nothing named conv3x3 / subpixel / deconv may stand here.
_NOT_COVERED = {}


def _signatures(gen, z, noise, batch):
    sig = set()
    for p in PATHS:
        sig |= {kernel for _layer, kernel in path_map(gen, p, z, noise, batch)}
    return {k for k in sig if any(f in k for f in _FAMILIES)}


def test_fixtures_launch_every_convolution_kernel_cars_512_launches(torch_cuda):
    import torch
    from gan_segmentation_amd.image_generator import ImageGenerator
    from tests.common import gan_setup
    ours = set()
    for name, batch in EXACT_CASES:
        gen, z, noise = _built(name, batch)
        ours |= _signatures(gen, z, noise, batch)
    assert any("bf16_lean" in k for k in ours) and any("subpixel_res" in k for k in ours) and any("ksplit" in k for k in ours), sorted(ours)
    cars = set()
    for batch in (1, 4):
        gcfg, gp, dcfg, dp, z, noise = gan_setup("cars", batch)
        gen = ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=batch, precision="bf16")
        gen.graph_mode = "0"
        dev = gen.netG._model.device
        cars |= _signatures(gen, torch.from_numpy(z).to(dev), [torch.from_numpy(a).to(dev) for a in noise], batch)
        del gen
        torch.cuda.empty_cache()
    for k in _NOT_COVERED:
        assert not any(f in k for f in ("conv3x3", "subpixel", "deconv")), "a convolution kernel may not be left out: %s" % k
        assert k in cars and k not in ours, "stale entry in _NOT_COVERED: %s" % k
    missing = sorted(cars - ours - set(_NOT_COVERED))
    assert not missing, "cars 512^2 bf16 launches kernels no exact fixture launches:\n  " + "\n  ".join(missing)
