"""Every kind of output the library accepts, on the GPU: 1-8 classes, 1-4 colours, 4-128 px (include/gsa.h gsa_generator_init,
gsa_decoder_init), over the forms of tests.common.OUTPUT_FORMS.

fp32: rgb, image, every feature, logits and mask are the C oracle's, bit for bit (the bar of tests/test_gpu_parity.py), on weights whose
w depends on z (tests.common.lively).  bf16: the oracle is not the GPU's bits there (tests/test_gpu_bf16.py), so the exact checks are the
slice property -- a model that keeps the first nc colours and the first k classes of a 4-colour, 8-class model gives that model's outputs
sliced, because every output row is a chain of its own (tests/test_oracle.py shows it on the oracle) -- and the downscale rule of
tests/test_downscale_host.py on the GPU's own rgb and logits.

Every test that runs a model also takes the (layer, kernel) pairs of one eager, profiled step (tests.dispatch_map.path_map);
test_the_module_ran_every_output_kernel_form, the last test, counts them.  It reads what the tests above it recorded in this process: it
is meant for a run of the whole module.

Conditions on the inputs, checked on the oracle's outputs where a case is made (_case): w depends on z, every colour holds image bytes
strictly between 0 and 255, every class occurs in the mask of a case with two or more classes.  Decoder seeds were chosen for the last
one (_DECODER_SEED); no seed depends on what the GPU computes."""
import ctypes
import re

import numpy as np
import pytest

from tests.common import colours_for, form_setup, sliced_model, unsaturated_colours, w_spread
from tests.dispatch_map import path_map
from tests.test_downscale_host import rule_image, rule_mask

pytestmark = pytest.mark.gpu

# decoder seeds at which every class occurs in the oracle's mask (the default, 3, leaves one out): {(form, classes): seed}
_DECODER_SEED = {("M128", 7): 4, ("M128", 8): 4, ("ODD", 8): 14}

_SEEN = {"fp32": set(), "bf16": set()}      # (layer, kernel signature) pairs of the module's profiled steps
_CASES = {}


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, "%s: shape %s vs %s" % (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        idx = tuple(np.argwhere(a != b)[0])
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (what, int((a != b).sum()), a.size, idx, a[idx], b[idx]))


def _case(oracle_lib, form, nc, k, batch, precision="fp32", **kw):
    """The setup of one case and the C oracle's outputs on it, computed once and shared (read only); the input conditions are checked
    here, on the oracle, so that a dull input cannot hide a kernel."""
    key = (form, nc, k, batch, precision, tuple(sorted(kw.items())))
    if key in _CASES:
        return _CASES[key]
    setup = form_setup(form, batch, nc, k or 2, decoder_seed=_DECODER_SEED.get((form, k)), **kw)
    gcfg, gp, dcfg, dp, z, noise = setup
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp, precision=precision)
    w = o.mapping(np.random.default_rng(1).standard_normal((4, 512)).astype(np.float32))
    assert w_spread(w) > 0.0, "precondition: w must depend on z"
    rgb, img, feats = o.generator(z, noise)
    assert unsaturated_colours(img) == list(range(nc)), "precondition: every colour needs bytes strictly between 0 and 255"
    c = {"setup": setup, "rgb": rgb, "img": img, "feats": feats, "logits": None, "mask": None}
    if dcfg is not None:
        c["logits"], c["mask"] = o.decoder(feats)
        if k >= 2:
            assert sorted(np.unique(c["mask"]).tolist()) == list(range(k)), "precondition: every class must occur in the oracle's mask"
    for v in [rgb, img, c["logits"], c["mask"]] + feats:
        if v is not None:
            v.setflags(write=False)
    _CASES[key] = c
    return c


def _build(setup, batch, precision="fp32"):
    from gan_segmentation_amd.image_generator import ImageGenerator
    gcfg, gp, dcfg, dp, _z, _noise = setup
    gen = ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=batch, precision=precision)
    gen.graph_mode = "0"        # eager: the profiled step is the step that was checked
    return gen


def _two_call(gen, z, noise):
    rgb, feats, img = gen.netG(z, noise=noise, want_image=True)
    out = {"rgb": rgb.cpu().numpy(), "img": img.cpu().numpy(), "feats": [f.cpu().numpy() for f in feats], "logits": None, "mask": None}
    if gen._decoder is not None:
        logits, mask = gen._decoder(*feats, want_mask=True)
        out["logits"], out["mask"] = logits.cpu().numpy(), mask.cpu().numpy()
    return out


def _record(gen, precision, z, noise, batch, paths=("two_call", "generate")):
    pairs = set()
    for path in paths:
        pairs |= path_map(gen, path, z, noise, batch)
    _SEEN[precision] |= pairs
    return pairs


def _check_against_oracle(gen, case, n, what, lo=0):
    """Samples lo..n-1 of the case through the two-call path == the oracle's, every output; generate_batch == the two-call path."""
    _gcfg, _gp, dcfg, _dp, z, noise = case["setup"]
    zs, ns = z[lo:n], [a[lo:n] for a in noise]
    got = _two_call(gen, zs, ns)
    for i, (a, b) in enumerate(zip(got["feats"], case["feats"])):
        _same(a, b[lo:n], "%s: feature %d" % (what, i))
    _same(got["rgb"], case["rgb"][lo:n], what + ": rgb")
    _same(got["img"], case["img"][lo:n], what + ": image")
    if dcfg is not None:
        _same(got["logits"], case["logits"][lo:n], what + ": logits")
        _same(got["mask"], case["mask"][lo:n], what + ": mask")
        img, mask = gen.generate_batch(zs, ns)
        _same(img.cpu().numpy(), got["img"], what + ": generate_batch image")
        _same(mask.cpu().numpy(), got["mask"], what + ": generate_batch mask")
    return got


# ---------------------------------------------------------------------------------------------------------------- fp32, oracle-exact

# (form, classes, colours): 128 px with 16 channels in front of toRGB and the final conv (M128, D2: the one-pixel-per-thread toRGB),
# 48 (ODD: toRGB in chunks of 32 + 16) and 64 px with 32 (M64: one chunk)
_CLASS_CASES = [("M128", k, colours_for(k)) for k in range(1, 9)] + [("ODD", 5, 1), ("ODD", 8, 2), ("ODD", 1, 4), ("M64", 6, 4), ("D2", 4, 2)]


@pytest.mark.parametrize("form,k,nc", _CLASS_CASES, ids=["%s-k%d-nc%d" % c for c in _CLASS_CASES])
def test_fp32_every_class_and_colour_count_matches_the_oracle(torch_cuda, oracle_lib, form, k, nc):
    """final_conv_kernel at every class count (the packed class pairs at 2, 4, 6, 8) and toRGB at every colour count, batch 3."""
    case = _case(oracle_lib, form, nc, k, 3)
    gen = _build(case["setup"], 3)
    _check_against_oracle(gen, case, 3, "%s k=%d nc=%d" % (form, k, nc))
    pairs = _record(gen, "fp32", case["setup"][4], case["setup"][5], 3)
    assert any(re.match(r"^d\.final_\d+$", layer) for layer, _k in pairs) and any(layer == "g.torgb" for layer, _k in pairs)


# (form, classes, colours, batches): 16 and 32 px, three and four decoder levels
_SMALL_CASES = [("S16a", 7, 4, (1, 3, 17)), ("S16b", 3, 1, (1, 3, 17)), ("S16c", 2, 2, (2,)),
                ("S32a", 5, 1, (1, 3, 17)), ("S32b", 6, 2, (1, 3, 17)), ("S32c", 8, 3, (2,))]


@pytest.mark.parametrize("form,k,nc,batches", _SMALL_CASES, ids=[c[0] for c in _SMALL_CASES])
def test_fp32_small_outputs_match_the_oracle(torch_cuda, oracle_lib, form, k, nc, batches):
    """16 px (one 16 x 16 tile of the final conv, a three-level decoder) and 32 px, at 16 / 64 / 512 channels: the first b samples of
    one draw at every batch b."""
    case = _case(oracle_lib, form, nc, k, max(batches))
    gen = _build(case["setup"], max(batches))
    for b in batches:
        _check_against_oracle(gen, case, b, "%s batch %d" % (form, b))
        _record(gen, "fp32", case["setup"][4], case["setup"][5], b)


_GENERATOR_ONLY = [("S4a", 1, (1, 3, 17)), ("S4a", 4, (1, 3, 17)), ("S8a", 1, (1, 3, 17)), ("S8a", 4, (1, 3, 17)),
                   ("S4b", 2, (2,)), ("S4b", 3, (2,)), ("S8b", 2, (2,)), ("S8b", 3, (2,)), ("S4d", 3, (1, 3)), ("S8d", 1, (1, 3))]


@pytest.mark.parametrize("form,nc,batches", _GENERATOR_ONLY, ids=["%s-nc%d" % c[:2] for c in _GENERATOR_ONLY])
def test_fp32_generators_of_4_and_8_px_match_the_oracle(torch_cuda, oracle_lib, form, nc, batches):
    """A one-level generator (4 px: no conv_1 at all) and a two-level one.  16 and 64 pixels per sample are less than toRGB's 256-pixel
    block, so these are the cases that run its partial blocks: torgb_kernel's `npx = min(256, HW - p0)` / `tid < npx` at 64 and 512
    channels (S4a, S4b, S8a, S8b), torgb_direct_kernel's `pix >= HW` at 16 (S4d, S8d)."""
    case = _case(oracle_lib, form, nc, None, max(batches))
    gen = _build(case["setup"], max(batches))
    assert gen._decoder is None
    for b in batches:
        _check_against_oracle(gen, case, b, "%s nc=%d batch %d" % (form, nc, b))


@pytest.mark.parametrize("form,k,nc", [("S4a", None, 4), ("S16a", 7, 4), ("S32a", 5, 1)])
def test_fp32_batch_composition_at_small_sizes(torch_cuda, oracle_lib, form, k, nc):
    """Samples 3.. of a batch of 5 equal the same samples run alone (and the oracle's)."""
    case = _case(oracle_lib, form, nc, k, 5)
    gen = _build(case["setup"], 5)
    _gcfg, _gp, _dcfg, _dp, z, noise = case["setup"]
    whole = _check_against_oracle(gen, case, 5, form + " batch of 5")
    alone = _check_against_oracle(gen, case, 5, form + " samples 3.. alone", lo=3)
    for name in ("rgb", "img", "logits", "mask"):
        if whole[name] is not None:
            _same(alone[name], whole[name][3:], "%s: %s of samples 3.. alone" % (form, name))
    for i, (a, b) in enumerate(zip(alone["feats"], whole["feats"])):
        _same(a, b[3:], "%s: feature %d of samples 3.. alone" % (form, i))


@pytest.mark.parametrize("nc", [3, 2, 4])
@pytest.mark.parametrize("form,last_feature", [("S32a", 16), ("M64d", 16), ("M128", 16), ("M128", None)])
def test_fp32_fused_torgb_gate(torch_cuda, oracle_lib, form, last_feature, nc):
    """The fused step lets the decoder's last cvt conv write the image only where that conv is the 16 -> 16 lean Winograd kernel and
    there are 3 colours; the separate toRGB launch runs otherwise: at 2 and 4 colours, with the 32-wide last decoder level of
    tests.common's default decoder (last_feature None), and at 32 px (S32a), where a 16-channel conv is not in Winograd form by the
    canonical rule (64 px and up: oracle/c/gsa_oracle.c use_wino).  M64d, 4 x 4 tiles, is the fused kernel's minimum.  The image is the
    oracle's either way."""
    kw = {} if last_feature is None else {"last_feature": last_feature}
    case = _case(oracle_lib, form, nc, 2, 3, **kw)
    gen = _build(case["setup"], 3)
    gcfg, _gp, dcfg, _dp, z, noise = case["setup"]
    _check_against_oracle(gen, case, 3, "%s nc=%d" % (form, nc))
    pairs = path_map(gen, "generate", z, noise, 3)
    _SEEN["fp32"] |= pairs
    layers = {layer for layer, _k in pairs}
    last = len(dcfg["in_channels"]) - 1
    fused = nc == 3 and last_feature == 16 and gcfg["max_res_log2"] >= 6
    assert ("d.cvt_%d+torgb" % last in layers) == fused and ("d.cvt_%d" % last in layers) == (not fused), sorted(layers)
    assert ("g.torgb" in layers) == (not fused), sorted(layers)


def test_fp32_overlap_settings_give_identical_bytes(torch_cuda, oracle_lib):
    """A three-level decoder (S16a): the default puts every level but the last -- two -- on the second stream; 0 and 1 levels there
    give the same pair, the oracle's."""
    case = _case(oracle_lib, "S16a", 4, 7, 3)
    gen = _build(case["setup"], 3)
    _gcfg, _gp, _dcfg, _dp, z, noise = case["setup"]
    ctx = gen.netG._model.ctx
    for levels in (-1, 0, 1):
        ctx.set_overlap(levels)
        img, mask = gen.generate_batch(z, noise)
        _same(img.cpu().numpy(), case["img"], "image, overlap %d" % levels)
        _same(mask.cpu().numpy(), case["mask"], "mask, overlap %d" % levels)
    ctx.set_overlap(-1)


def test_fp32_without_wscale_matches_the_oracle(torch_cuda, oracle_lib):
    """use_wscale=False (no std factors anywhere) on the 64 px form."""
    case = _case(oracle_lib, "M64", 3, 3, 2, use_wscale=False)
    _check_against_oracle(_build(case["setup"], 2), case, 2, "M64 without wscale")


# ---------------------------------------------------------------------------------------------------------------- downscaled pairs

def _device_inputs(gen, z, noise):
    import torch
    dev = gen.netG._model.device
    return torch.from_numpy(np.ascontiguousarray(z)).to(dev), [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in noise]


def _downscaled(gen, zt, nt, f):
    """(image, mask) of the context's gsa_generate_downscaled at factor f on one built model."""
    import torch
    g = gen.netG
    ctx, dev = g._model.ctx, g._model.device
    n, R = zt.shape[0], 2 ** g.max_res_log2 // f
    g._model.ensure_batch(n)
    img = torch.full((n, R, R, g.nc), 7, device=dev, dtype=torch.uint8)
    mask = torch.full((n, R, R), 7, device=dev, dtype=torch.uint8)
    ctx.generate_downscaled(torch.cuda.current_stream(dev).cuda_stream, n, zt.data_ptr(), None, 0, [a.data_ptr() for a in nt], f,
                            img.data_ptr(), mask.data_ptr())
    return img.cpu().numpy(), mask.cpu().numpy()


def _record_downscaled(gen, precision, zt, nt, f):
    """The profiled eager step at factor f: generate_batch of a model whose output_downscale is f runs the same entry."""
    gen.output_downscale = f
    try:
        pairs = path_map(gen, "generate", zt, nt, zt.shape[0])
    finally:
        gen.output_downscale = 1
    _SEEN[precision] |= pairs
    layers = {layer for layer, _k in pairs}
    assert "g.torgb_down" in layers and any(re.match(r"^d\.final_\d+_down$", layer) for layer in layers), sorted(layers)
    assert "g.torgb" not in layers and not any("+torgb" in layer for layer in layers), sorted(layers)


_DOWN_CASES = [("M128", k, colours_for(k), (2, 4, 8)) for k in range(1, 9)] + [("S32a", 5, 1, (2,)), ("M64", 6, 4, (2, 4))]


@pytest.mark.parametrize("form,k,nc,factors", _DOWN_CASES, ids=["%s-k%d-nc%d" % c[:3] for c in _DOWN_CASES])
def test_fp32_downscaled_pairs_match_the_rule_on_the_oracle(torch_cuda, oracle_lib, form, k, nc, factors):
    """final_conv_down_kernel at every class count and factor, torgb_down_kernel at every colour count: one built model per class count,
    every factor through gsa_generate_downscaled, against the rule on the oracle's rgb and logits.  S32a at factor 2 is the smallest
    output the entry accepts (16 px)."""
    case = _case(oracle_lib, form, nc, k, 3)
    gen = _build(case["setup"], 3)
    zt, nt = _device_inputs(gen, case["setup"][4], case["setup"][5])
    nearest_differs = False
    for f in factors:
        img, mask = _downscaled(gen, zt, nt, f)
        _same(img, rule_image(case["rgb"], f), "%s k=%d image f=%d" % (form, k, f))
        _same(mask, rule_mask(case["logits"], f), "%s k=%d mask f=%d" % (form, k, f))
        nearest_differs |= not np.array_equal(mask, case["mask"][:, ::f, ::f])
        _record_downscaled(gen, "fp32", zt, nt, f)
    assert nearest_differs or k == 1, "no block's mask differs from its top-left pixel's class: the test cannot tell the rules apart"


@pytest.mark.parametrize("form,k,nc,f", [("S32a", 5, 1, 4), ("S16a", 7, 4, 2)])
def test_downscaling_below_16_px_is_refused(torch_cuda, oracle_lib, form, k, nc, f):
    """GSA_ERR_INVALID, and the context stays usable."""
    import torch
    case = _case(oracle_lib, form, nc, k, 3)
    gen = _build(case["setup"], 3)
    zt, nt = _device_inputs(gen, case["setup"][4], case["setup"][5])
    g = gen.netG
    ctx, dev = g._model.ctx, g._model.device
    g._model.ensure_batch(3)
    R = 2 ** g.max_res_log2
    img = torch.zeros((3, R, R, nc), device=dev, dtype=torch.uint8)        # full size: room for whatever a wrong acceptance would write
    mask = torch.zeros((3, R, R), device=dev, dtype=torch.uint8)
    nzp = (ctypes.c_void_p * len(nt))(*[a.data_ptr() for a in nt])
    s = torch.cuda.current_stream(dev).cuda_stream
    assert ctx.api.generate_downscaled(ctx._h, s, 3, zt.data_ptr(), None, 0, nzp, len(nt), f, img.data_ptr(), mask.data_ptr()) == -1
    assert b"16" in ctx.api.last_error(ctx._h)
    _check_against_oracle(gen, case, 3, form + " after the refused call")
    ctx.check()


# ---------------------------------------------------------------------------------------------------------------- bf16, exact

@pytest.mark.parametrize("form", ["M128", "S32a", "S16c"])
def test_bf16_outputs_of_a_sliced_model_are_slices(torch_cuda, oracle_lib, form):
    """The slice property in bf16 mode, byte for byte: rgb, image, logits and mask of the first nc colours / k classes, k = 1..8, against
    the 4-colour, 8-class model's; generate_batch gives the two-call bytes."""
    full = _case(oracle_lib, form, 4, 8, 3)["setup"]        # the input conditions, on the fp32 oracle
    z, noise = full[4], full[5]
    gen8 = _build(full, 3, "bf16")
    want = _two_call(gen8, z, noise)
    for k in range(1, 9):
        nc = colours_for(k)
        gen = gen8 if k == 8 and nc == 4 else _build(sliced_model(*full[:4], nc, k) + (z, noise), 3, "bf16")
        got = _two_call(gen, z, noise)
        what = "%s bf16 k=%d nc=%d" % (form, k, nc)
        _same(got["rgb"], want["rgb"][:, :nc], what + ": rgb")
        _same(got["img"], want["img"][..., :nc], what + ": image")
        _same(got["logits"], want["logits"][:, :k], what + ": logits")
        _same(got["mask"], want["logits"][:, :k].argmax(1).astype(np.uint8), what + ": mask")
        img, mask = gen.generate_batch(z, noise)
        _same(img.cpu().numpy(), got["img"], what + ": generate_batch image")
        _same(mask.cpu().numpy(), got["mask"], what + ": generate_batch mask")
        _record(gen, "bf16", z, noise, 3)


@pytest.mark.parametrize("k", [1, 4, 5, 8])
def test_bf16_downscaled_pairs_match_the_rule_on_the_gpus_own_outputs(torch_cuda, oracle_lib, k):
    """bf16 mode at every factor: the rule on the bf16 GPU's own rgb and logits, bit for bit (M128)."""
    nc = colours_for(k)
    setup = _case(oracle_lib, "M128", nc, k, 3)["setup"]       # the fp32 test's case: its input conditions hold
    gen = _build(setup, 3, "bf16")
    own = _two_call(gen, setup[4], setup[5])
    zt, nt = _device_inputs(gen, setup[4], setup[5])
    nearest_differs = False
    for f in (2, 4, 8):
        img, mask = _downscaled(gen, zt, nt, f)
        _same(img, rule_image(own["rgb"], f), "bf16 k=%d image f=%d" % (k, f))
        _same(mask, rule_mask(own["logits"], f), "bf16 k=%d mask f=%d" % (k, f))
        nearest_differs |= not np.array_equal(mask, own["mask"][:, ::f, ::f])
        _record_downscaled(gen, "bf16", zt, nt, f)
    assert nearest_differs or k == 1


@pytest.mark.parametrize("form,k,nc", [("S16a", 7, 4), ("S32b", 6, 2)])
def test_bf16_small_outputs_against_the_bf16_oracle(torch_cuda, oracle_lib, form, k, nc):
    """The contract of tests/test_gpu_bf16.py at 16 and 32 px: the 4 x 4 level to fp32 rounding, rgb and logits within 3 % (max) and
    0.3 % (mean) of the bf16 oracle's range.  No share-of-pixels bar on the mask: at 256-1024 pixels a handful of pixels decides it, and
    the masks are held exactly by the slice and downscale tests above."""
    from tests.test_gpu_bf16 import _rel, check_first_level
    case = _case(oracle_lib, form, nc, k, 3, precision="bf16")
    got = _two_call(_build(case["setup"], 3, "bf16"), case["setup"][4], case["setup"][5])
    flips, d0 = check_first_level(got["feats"][0], case["feats"][0], isolated_flips=False)
    figures = {"rgb": _rel(got["rgb"], case["rgb"]), "logits": _rel(got["logits"], case["logits"])}
    print("%s bf16 HIP vs bf16 oracle: 4x4 level %d beyond 2e-6, max %.3e; rgb max %.3e mean %.3e; logits max %.3e mean %.3e"
          % ((form, flips, d0) + figures["rgb"] + figures["logits"]))
    for name, (mx, mean) in figures.items():
        assert mx <= 3e-2 and mean <= 3e-3, "%s %s: max %.3e mean %.3e of the oracle's range" % (form, name, mx, mean)


# ---------------------------------------------------------------------------------------------------------------- what ran

def _kernels(precision, layer_pattern):
    return {kernel for layer, kernel in _SEEN[precision] if re.match(layer_pattern, layer)}


def test_the_module_ran_every_output_kernel_form():
    """Distinct kernel signatures the tests above launched, by layer: the final conv at 8 class counts in fp32 and in bf16, the
    downscaled final conv at 8 class counts x 3 factors in fp32 and at 4 x 3 in bf16, the downscaled toRGB at 3 factors in both, and
    both full-size toRGB kernels.  Counted, not spelled: a renamed template argument does not break this, a form that stopped running
    does."""
    assert len(_kernels("fp32", r"^d\.final_\d+$")) == 8, sorted(_kernels("fp32", r"^d\.final_\d+$"))
    assert len(_kernels("bf16", r"^d\.final_\d+$")) == 8, sorted(_kernels("bf16", r"^d\.final_\d+$"))
    assert len(_kernels("fp32", r"^d\.final_\d+_down$")) == 24, sorted(_kernels("fp32", r"^d\.final_\d+_down$"))
    assert len(_kernels("bf16", r"^d\.final_\d+_down$")) == 12, sorted(_kernels("bf16", r"^d\.final_\d+_down$"))
    assert len(_kernels("fp32", r"^g\.torgb_down$")) == 3 and len(_kernels("bf16", r"^g\.torgb_down$")) == 3
    assert not (_kernels("fp32", r"^d\.final") & _kernels("bf16", r"^d\.final")), "fp32 and bf16 run different final-conv instances"
    for precision in ("fp32", "bf16"):
        torgb = _kernels(precision, r"^g\.torgb$")
        assert any("torgb_direct_kernel" in k for k in torgb) and any("torgb_kernel" in k for k in torgb), sorted(torgb)
    assert any(re.match(r"^d\.cvt_\d+\+torgb$", layer) for layer, _k in _SEEN["fp32"])
