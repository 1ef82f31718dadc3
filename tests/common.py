"""Shared builders for the parity tests."""
import numpy as np

from gan_segmentation_amd import weights as W


def lively(gp):
    """The synthetic weights with the mapping layers scaled by 1/lr_mult (100), as trained StyleGAN files hold them: drawn at
    unit scale, the eight lr_mult-0.01 layers shrink z away and w comes out the same to the last bit for every z."""
    out = dict(gp)
    for i in range(8):
        out["mp_dense_%d_weight" % i] = gp["mp_dense_%d_weight" % i] * 100.0
    return out


def reduced_setup(max_res_log2=7, batch=2, trivial_norm=False, seed=2, live_mapping=False):
    """live_mapping=True: the mapping layers of lively(), so that w depends on z."""
    gcfg = W.reduced_generator_config(max_res_log2)
    gp = W.synthetic_generator_params(gcfg, seed=seed, trivial_norm=trivial_norm)
    if live_mapping:
        gp = lively(gp)
    dcfg = W.decoder_config(max_res_log2, in_channels=W.generator_channels(gcfg))
    dp = W.synthetic_decoder_params(dcfg, seed=seed + 1)
    z, noise = W.synthetic_inputs(gcfg, batch)
    return gcfg, gp, dcfg, dp, z, noise


def gan_setup(gan="ffhq", batch=1, live_mapping=False):
    mr = W.GAN_MAX_RES_LOG2[gan]
    gcfg = W.generator_config(mr)
    gp = W.synthetic_generator_params(gcfg, seed=2)
    if live_mapping:
        gp = lively(gp)
    dcfg = W.decoder_config(mr)
    dp = W.synthetic_decoder_params(dcfg, seed=3)
    z, noise = W.synthetic_inputs(gcfg, batch)
    return gcfg, gp, dcfg, dp, z, noise


def odd_setup(batch, live_mapping=False):
    """128 px with 48-channel levels: 96 style columns per layer (one 64-wide tile + one 32-wide) and odd decoder widths."""
    gcfg = W.generator_config(max_res_log2=7, fmap_base=3072, fmap_max=48)
    dcfg = W.decoder_config(7, in_channels=W.generator_channels(gcfg))
    dcfg["features"] = [48, 32, 48, 80, 16, 48, 2]
    gp = W.synthetic_generator_params(gcfg, seed=11, trivial_norm=False)
    if live_mapping:
        gp = lively(gp)
    dp = W.synthetic_decoder_params(dcfg, seed=12)
    z, noise = W.synthetic_inputs(gcfg, batch)
    return gcfg, gp, dcfg, dp, z, noise


# Output configurations the library accepts beside the trained models': generator_config keywords per name.  Channels per level:
# S4a [64], S4b [512], S8a [64, 64], S8b [512, 512] (generator only: a decoder needs 16 px), S16a [64, 32, 16], S16b [64] x 3,
# S16c [512] x 3, S32a [64, 64, 32, 16], S32b [64] x 4, S32c [512] x 4, M64 [64, 64, 64, 64, 32], M128 = reduced_setup(7)'s
# [64, 64, 64, 64, 32, 16], ODD = odd_setup's 48 everywhere, D2 [64 x 5, 16] (a 4:1 step between the last two levels).
# S4d [16] and S8d [16, 16] put the one-pixel-per-thread toRGB (16 channels) on a partial block; M64d [64, 64, 64, 32, 16] is the
# smallest output whose last level has 16 channels and takes the Winograd form (64 px: the fused cvt+toRGB kernel's minimum).
OUTPUT_FORMS = {
    "S4a": dict(max_res_log2=2, fmap_base=1024, fmap_max=64), "S4b": dict(max_res_log2=2, fmap_base=8192, fmap_max=512),
    "S4d": dict(max_res_log2=2, fmap_base=1024, fmap_max=16),
    "S8a": dict(max_res_log2=3, fmap_base=1024, fmap_max=64), "S8b": dict(max_res_log2=3, fmap_base=8192, fmap_max=512),
    "S8d": dict(max_res_log2=3, fmap_base=1024, fmap_max=16),
    "S16a": dict(max_res_log2=4, fmap_base=128, fmap_max=64), "S16b": dict(max_res_log2=4, fmap_base=1024, fmap_max=64),
    "S16c": dict(max_res_log2=4, fmap_base=8192, fmap_max=512),
    "S32a": dict(max_res_log2=5, fmap_base=256, fmap_max=64), "S32b": dict(max_res_log2=5, fmap_base=1024, fmap_max=64),
    "S32c": dict(max_res_log2=5, fmap_base=8192, fmap_max=512),
    "M64": dict(max_res_log2=6, fmap_base=1024, fmap_max=64), "M64d": dict(max_res_log2=6, fmap_base=512, fmap_max=64),
    "M128": dict(max_res_log2=7, fmap_base=1024, fmap_max=64),
    "ODD": dict(max_res_log2=7, fmap_base=3072, fmap_max=48),
    "D2": dict(max_res_log2=7, fmap_base=65536, fmap_max=64, fmap_decay=2.0),
}


def colours_for(k):
    """The colour count paired with class count k: 1, 2, 4, 3, 1, 2, 4, 3 for k = 1..8."""
    return (1, 2, 4, 3)[(k - 1) % 4]


def form_setup(name, batch, channels=3, classes=2, live_mapping=True, decoder_seed=None, last_feature=None, **overrides):
    """(gcfg, gp, dcfg, dp, z, noise) of OUTPUT_FORMS[name] with `channels` colours and a `classes`-class decoder (None below 16 px):
    the synthetic weights of reduced_setup / odd_setup (generator seed 2, ODD 11; decoder seed 3, ODD 12; loaded norm parameters),
    the mapping layers of lively() unless live_mapping=False.  last_feature: the decoder's width at the output resolution (16 as in the
    1024 px decoder, instead of 32).  overrides: further generator_config keys (use_wscale=False)."""
    odd = name == "ODD"
    gcfg = W.generator_config(channels=channels, **dict(OUTPUT_FORMS[name], **overrides))
    gp = W.synthetic_generator_params(gcfg, seed=11 if odd else 2, trivial_norm=False)
    if live_mapping:
        gp = lively(gp)
        if not gcfg["use_wscale"]:      # no std factor at run time: a trained file holds it inside the weights (unscaled, w overflows)
            for i in range(8):
                gp["mp_dense_%d_weight" % i] = gp["mp_dense_%d_weight" % i] * W.formula_constants(gcfg)["mp_dense_%d_std" % i]
    dcfg = dp = None
    mrl = gcfg["max_res_log2"]
    if mrl >= 4:
        dcfg = W.decoder_config(mrl, num_classes=classes, in_channels=W.generator_channels(gcfg))
        if odd:
            dcfg["features"] = [48, 32, 48, 80, 16, 48, classes]
        if last_feature is not None:
            dcfg["features"][-2] = last_feature
        dp = W.synthetic_decoder_params(dcfg, seed=decoder_seed if decoder_seed is not None else (12 if odd else 3))
    z, noise = W.synthetic_inputs(gcfg, batch)
    return gcfg, gp, dcfg, dp, z, noise


def sliced_model(gcfg, gp, dcfg, dp, channels, classes):
    """The model that keeps the first `channels` toRGB rows and the first `classes` rows of the decoder's final conv of
    (gcfg, gp, dcfg, dp): every output row is a chain of its own, so its rgb / image / logits are the slices of the full model's and
    its mask is the first maximum over the sliced logits."""
    R = 2 ** gcfg["max_res_log2"]
    last = len(dcfg["in_channels"]) - 1
    g = dict(gcfg, channels=channels)
    d = dict(dcfg, num_classes=classes, features=list(dcfg["features"][:-1]) + [classes])
    p, q = dict(gp), dict(dp)
    for key in ("%d_conv_to_rgb_weight" % R, "%d_conv_to_rgb_bias" % R):
        p[key] = np.ascontiguousarray(gp[key][:channels])
    for key in ("main_block_%d.0.weight" % last, "main_block_%d.0.bias" % last):
        q[key] = np.ascontiguousarray(dp[key][:classes])
    return g, p, d, q


def unsaturated_colours(img):
    """Colours of the u8 image (N, R, R, nc) that hold a byte strictly between 0 and 255."""
    img = np.asarray(img)
    return [c for c in range(img.shape[-1]) if ((img[..., c] > 0) & (img[..., c] < 255)).any()]


def w_spread(w):
    """max |w_i - w_0| over the samples of w (N, latent): how much the mapping output depends on z."""
    w = np.asarray(w, np.float64)
    return float(np.abs(w - w[:1]).max())


def bench_setup(gan="ffhq", batch=8, rank=0):
    """Exactly bench.py's weights and inputs (synthetic weights seeds 2/3, inputs seeds 1000+rank / 2000+rank)."""
    mr = W.GAN_MAX_RES_LOG2[gan]
    gcfg, dcfg = W.generator_config(mr), W.decoder_config(mr)
    gp, dp = W.synthetic_generator_params(gcfg, seed=2), W.synthetic_decoder_params(dcfg, seed=3)
    z, noise = W.synthetic_inputs(gcfg, batch, seed_z=1000 + rank, seed_noise=2000 + rank)
    return gcfg, gp, dcfg, dp, z, noise


def golden_bench_outputs():
    """tests/golden/bench_outputs.json: SHA-256 of the C oracle's (image, mask) for the first samples of bench.py's inputs."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bench_outputs.json")) as f:
        return json.load(f)


def pair_digest(img, mask):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(img).tobytes() + np.ascontiguousarray(mask).tobytes()).hexdigest()


SWEEP_MAX_BATCH = 64      # every model is swept over 1..64, and the first 64 sweep inputs are one draw (sweep_setup)

# The largest batch tests/test_gpu_batch_sweep.py and tests/dispatch_map.py run per model.  Beyond 64 only the batch is new: bedrooms at
# 256 (64 channels x 256^2 px) and cars at 128 (32 x 512^2) hold 2^30 elements in their largest tensor, exactly what ffhq holds at 64
# (16 x 1024^2), and ffhq stays there.  Workspace gsa_reserve asks for at these batches, from its sizing code (fp32, generator + decoder,
# summed over its dev_alloc calls: activations x2 / t_raw / x1, decoder din / cvt / ya / prev / scb, and the small rows): bedrooms 256:
# 33 GiB, cars 128: 42 GiB, ffhq 64: 46 GiB -- each below a third of the card's 288 GB, so no maximum is halved.
SWEEP_MAX = {"ffhq": 64, "cars": 128, "bedrooms": 256}


def sweep_setup(gan):
    """tests/test_gpu_batch_sweep.py's model and inputs: the full-size config with z-dependent mapping weights (lively) and
    SWEEP_MAX[gan] distinct samples.  Samples 0..63 are one draw (inputs seeds 3000 / 4000) whatever the maximum is -- the noise planes
    of a draw depend on its batch size, and sample 0 is what tests/golden/sweep_anchors.json digests; samples 64.. are a second draw
    (seeds 3001 / 4001)."""
    gcfg, gp, dcfg, dp, _z, _noise = gan_setup(gan, 1, live_mapping=True)
    z, noise = W.synthetic_inputs(gcfg, SWEEP_MAX_BATCH, seed_z=3000, seed_noise=4000)
    more = SWEEP_MAX[gan] - SWEEP_MAX_BATCH
    if more > 0:
        z2, noise2 = W.synthetic_inputs(gcfg, more, seed_z=3001, seed_noise=4001)
        z = np.concatenate([z, z2])
        noise = [np.concatenate([a, b]) for a, b in zip(noise, noise2)]
    return gcfg, gp, dcfg, dp, z, noise


# ---- the C headers against the ctypes table (tests/test_abi_and_host.py; the per-module tests take their declared sets from here) ----
_C_KINDS = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "uint64_t": "u64", "uint32_t": "u32", "float": "float", "double": "double",
            "void": "void"}


def c_kind(text):
    """The kind of a C type as written in a header: "pointer" for anything with a *, else one of _C_KINDS' values."""
    return "pointer" if "*" in text else _C_KINDS[text.replace("const", "").strip()]


def ctypes_kind(t):
    """The kind of a ctypes result or argument type, in c_kind's terms."""
    import ctypes as c
    if t is None:
        return "void"
    if t in (c.c_void_p, c.c_char_p) or issubclass(t, c._Pointer):
        return "pointer"
    return {c.c_int: "i32", c.c_int32: "i32", c.c_int64: "i64", c.c_uint64: "u64", c.c_uint32: "u32", c.c_float: "float",
            c.c_double: "double"}[t]


def header_declarations(name):
    """include/<name> -> (text without comments, {function: (result kind, [argument kinds])}) of every gsa_* function it declares."""
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", name)) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    out = {}
    for res, fn, args in re.findall(r"(?:^|[;{}])\s*((?:const\s+)?\w+[\s*]+)(gsa_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        args = [] if args.strip() == "void" else [re.sub(r"\w+\s*$", "", a) for a in args.split(",")]
        out[fn] = (c_kind(res), [c_kind(a) for a in args])
    return text, out
