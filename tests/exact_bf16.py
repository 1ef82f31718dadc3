"""Exactly summable bf16 models: fixtures on which the bf16 HIP path must equal the bf16 oracle in every byte.

In bf16 mode the HIP path and the C oracle differ only in the order in which the matrix core adds the products of an accumulation;
every other step is the same fp32 code or is order independent ("bf16 parity").  If, in every such accumulation, all
products are multiples of one power of two q and sum|product| < 2^24 * q, every partial sum in every order is exactly representable
and the order cannot matter.  The models built here meet that condition with room to spare; the oracle's witness
(Oracle.exact_headroom, oracle/c/gsa_oracle.c wit_scan) measures the room, and tests/test_exact_bf16_host.py asserts it on the oracle
alone -- never on the code under test.

Generator: every 3x3 / 4x4 weight is one of {-1, 0, 1} / 8 (use_wscale=False: the file's value is the effective weight); the AdaIN
affine is a narrow gain (ys + 1 = 1/16) around yb = 1.5 with small but nonzero dense weights, so the conv operands
fmaf(x, A, B) sit in about [0.75, 4.6) -- a bf16 quantum of 2^-8 or coarser -- and still depend on w; instance-norm gamma / beta are
the identity; noise scale factors, biases, blur taps and the (live) mapping layers keep their synthetic values.

Decoder: conv and shortcut weights are small integers times a power of two; the folded BatchNorm of every conv is calibrated per
channel so that each stored activation lrelu(fmaf(v, s, k)) lies in [1, 4), each shortcut in [1, 3.5] and each residual sum in
about [1.25, 6.75] on the inputs the suite runs (z path and W path).  The scale comes from the measured spread of v (an exact
float64 restatement of the decoder on the oracle's features, `_Calibrator`), not from a worst-case bound, so the stored values use the
bf16 mantissa.  The final conv and toRGB keep ordinary random weights (both sides run them as the same sequential chain); their random
biases are shifted by the output's mean, since sums over all-positive operands would otherwise saturate the image and give every pixel
to one class.
"""
import functools

import numpy as np

from gan_segmentation_amd import weights as W
from tests.common import OUTPUT_FORMS, lively

# name -> generator_config keywords: the smallest shapes that reach each bf16 kernel form (the plan rules are subpixel_plan in
# csrc/gsa_kernels.hip and bf16_lean_nt in csrc/gsa_bf16_lean.hip; tests/test_gpu_bf16_exact.py holds the outcome against cars 512^2).
#   E128  [64, 64, 64, 64, 32, 16] at 4..128 px, batch 3: K-split at 4 / 8 px, direct at 16 px, conv3x3_bf16_lean from 32 px, the plain
#         stride-2 kernel for up+conv (16..64 px) and the deconvolution (128 px), the whole decoder, toRGB over 16 channels
#   E32c  [512] x 4 at 4..32 px, batch 1: the same forms over 512 channels
#   E256  [64] x 6 + [32] at 4..256 px.  Batch 8: 512 tiles at 128 px, 2048 at 256 px -- the plain stride-2 kernel with 64 channels per
#         workgroup, the streamed-weight stride-2 kernel, the 2- and 4-group lean launches.  Batch 16: 4096 tiles at 256 px -- the
#         resident-panel stride-2 kernel (generator and decoder), the streamed one with 64 channels per workgroup.  Batch 1: one-tile grids.
EXACT_FORMS = {
    "E128": OUTPUT_FORMS["M128"],
    "E32c": OUTPUT_FORMS["S32c"],
    "E256": dict(max_res_log2=8, fmap_base=4096, fmap_max=64),
}
# (fixture, batch) pairs the suite runs
EXACT_CASES = [("E128", 3), ("E32c", 1), ("E256", 1), ("E256", 8), ("E256", 16)]

SEED = 5                        # of the fixtures' weights (and, + 100, of their W-path rows)
STEP = 0.125                    # one weight step of the 3x3 / 4x4 convolutions
GAIN = 1.0 / 16                 # AdaIN gain ys + 1
YB = 1.5
STORED = (1.0625, 3.75)         # target range of a stored decoder activation
BRANCH = (0.25, 3.25)           # ... of the residual branch (conv b, fp32, never stored on its own)
SHORTCUT = (1.0, 3.5)           # ... of the shortcut


def bf16r(x):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_codes(x):
    """The count of distinct bf16 codes in x after rounding."""
    return int(np.unique(bf16r(x).view(np.uint32) >> 16).size)


def checked_samples(batch):
    """The samples of a batch the oracle runs: all of a small batch, the first and the last of a large one (a sample does not
    depend on its batch)."""
    return list(range(batch)) if batch <= 3 else [0, batch - 1]


def take(z, noise, idx):
    return np.ascontiguousarray(z[idx]), [np.ascontiguousarray(a[idx]) for a in noise]


def exact_generator(name, seed):
    gcfg = W.generator_config(use_wscale=False, **EXACT_FORMS[name])
    gp = lively(W.synthetic_generator_params(gcfg, seed=2, trivial_norm=False))
    consts = W.formula_constants(gcfg)
    for i in range(8):      # no std factor at run time: the weights hold it, as tests.common.form_setup does
        gp["mp_dense_%d_weight" % i] = gp["mp_dense_%d_weight" % i] * consts["mp_dense_%d_std" % i]
    rng = np.random.Generator(np.random.PCG64(seed))
    for key in sorted(gp):
        v = gp[key]
        if key.endswith(("_conv_1_weight", "_conv_2_weight", "_deconv_1_weight")):
            gp[key] = (rng.integers(-1, 2, size=v.shape) * STEP).astype(np.float32)
        elif key.endswith("dense_affine_weight"):
            gp[key] = (v * (0.01 / np.sqrt(512.0))).astype(np.float32)
        elif key.endswith("dense_affine_bias"):
            C = v.shape[0] // 2
            gp[key] = np.concatenate([np.full(C, GAIN - 1.0), np.full(C, YB)]).astype(np.float32)
        elif key.endswith("norm_gamma"):
            gp[key] = np.ones_like(v)
        elif key.endswith("norm_beta"):
            gp[key] = np.zeros_like(v)
    return gcfg, gp


def exact_dlatents(oracle, gcfg, batch, seed=SEED):
    """Independent rows per (sample, layer) at w's scale, for the W path."""
    w = oracle.mapping(np.random.default_rng(1).standard_normal((4, 512)).astype(np.float32))
    L = 2 * (gcfg["max_res_log2"] - 1)
    return (np.random.default_rng(seed + 100).standard_normal((batch, L, 512)) * w.std()).astype(np.float32)


class _Calibrator:
    """The decoder of oracle/c/gsa_oracle.c in bf16 mode, restated in float64 on exactly summable operands (every convolution sum is
    exact in float64 whatever its order), walking the levels once and fixing each BatchNorm from the spread it meets."""

    def __init__(self, dcfg, rng):
        self.dcfg, self.rng, self.dp = dcfg, rng, {}

    @staticmethod
    def _conv(x, w, pad):
        import torch
        return torch.nn.functional.conv2d(torch.from_numpy(x), torch.from_numpy(np.asarray(w, np.float64)), padding=pad).numpy()

    def _weights(self, key, shape, density):
        w = (self.rng.integers(-1, 2, size=shape) * (self.rng.random(shape) < density) * STEP).astype(np.float32)
        self.dp[key] = w
        return w

    def _bn(self, prefix, bias_key, v, lo, hi):
        """BatchNorm (running_mean 0, running_var 1, conv bias 0) mapping the measured [min, max] of each channel of v onto [lo, hi];
        returns lrelu(fmaf(v, s, k)) with the oracle's fp32 s and k."""
        vmin, vmax = v.min(axis=(0, 2, 3)), v.max(axis=(0, 2, 3))
        assert (vmax > vmin).all(), "%s: a channel is constant" % prefix
        gamma = ((hi - lo) / (vmax - vmin)).astype(np.float32)
        s = gamma / np.sqrt(np.float32(1.0) + np.float32(1e-5))          # load_bn(): g / sqrtf(v + 1e-5f)
        beta = (lo - vmin * s.astype(np.float64)).astype(np.float32)
        C = v.shape[1]
        self.dp[bias_key] = np.zeros(C, np.float32)
        self.dp[prefix + ".gamma"], self.dp[prefix + ".beta"] = gamma, beta
        self.dp[prefix + ".running_mean"], self.dp[prefix + ".running_var"] = np.zeros(C, np.float32), np.ones(C, np.float32)
        y = (v * s.astype(np.float64)[None, :, None, None] + beta.astype(np.float64)[None, :, None, None]).astype(np.float32)
        return np.where(y > 0, y, np.float32(0.2) * y)

    def run(self, feats, final_seed):
        d, F, I = self.dcfg, self.dcfg["features"], self.dcfg["in_channels"]
        n = len(I)
        prev = None
        for i in range(n):
            x = bf16r(feats[i]).astype(np.float64)
            w = self._weights("cvt_block_%d.0.weight" % i, (F[i], I[i], 3, 3), 1.0 if I[i] <= 64 else 0.5)
            act = bf16r(self._bn("cvt_block_%d.1" % i, "cvt_block_%d.0.bias" % i, self._conv(x, w, 1), *STORED))
            cat = act if prev is None else np.concatenate([prev, act], axis=1)
            in_c, cs = cat.shape[1], F[i + 1]
            if i == n - 1:
                ref = W.synthetic_decoder_params(d, seed=final_seed)
                wf, bf = ref["main_block_%d.0.weight" % i], ref["main_block_%d.0.bias" % i]
                # the operands are all positive, so a class's logit sits on (sum of its weights) x (mean activation): the random bias is
                # shifted by the class's mean logit, or one class would win every pixel
                mean = self._conv(cat.astype(np.float64), wf, 1).mean(axis=(0, 2, 3))
                self.dp["main_block_%d.0.weight" % i], self.dp["main_block_%d.0.bias" % i] = wf, (bf - mean).astype(np.float32)
                break
            up = cat.repeat(2, axis=2).repeat(2, axis=3).astype(np.float64)
            b = "main_block_%d.1.base_layers" % i
            wa = self._weights(b + ".0.weight", (cs, in_c, 3, 3), 1.0)
            ya = bf16r(self._bn(b + ".1", b + ".0.bias", self._conv(up, wa, 1), *STORED))
            wb = self._weights(b + ".3.weight", (cs, cs, 3, 3), 1.0)
            yb = self._bn(b + ".4", b + ".3.bias", self._conv(ya.astype(np.float64), wb, 1), *BRANCH)
            if cs != in_c:
                # four inputs per output, +-1/4 each: a spread of at most 4 * (3.75 - 1.0625) / 4, shifted onto SHORTCUT by the bias
                wsc = np.zeros((cs, in_c, 1, 1), np.float32)
                for o in range(cs):
                    wsc[o, self.rng.choice(in_c, 4, replace=False), 0, 0] = np.array([0.25, 0.25, -0.25, -0.25], np.float32)
                acc = self._conv(up, wsc, 0)
                mid = 0.5 * (acc.min(axis=(0, 2, 3)) + acc.max(axis=(0, 2, 3)))
                bias = (np.round((0.5 * (SHORTCUT[0] + SHORTCUT[1]) - mid) * 64) / 64).astype(np.float32)
                self.dp["main_block_%d.1.shortcut.0.weight" % i], self.dp["main_block_%d.1.shortcut.0.bias" % i] = wsc, bias
                sc = bf16r((acc + bias[None, :, None, None].astype(np.float64)).astype(np.float32))
            else:
                sc = up.astype(np.float32)
            prev = bf16r((sc.astype(np.float32) + yb).astype(np.float32))
        order = W.decoder_param_shapes(d)
        return {k: np.ascontiguousarray(self.dp[k], np.float32) for k in order}


@functools.lru_cache(maxsize=None)
def _exact_setup(name, batch, seed):
    from oracle.binding import Oracle
    gcfg, gp = exact_generator(name, seed)
    dcfg = W.decoder_config(gcfg["max_res_log2"], num_classes=2, in_channels=W.generator_channels(gcfg))
    z, noise = W.synthetic_inputs(gcfg, batch)
    o = Oracle(gcfg, gp, precision="bf16")
    idx = checked_samples(batch)
    zc, nc = take(z, noise, idx)
    rgb, _img, feats_z = o.generator(zc, nc)
    # toRGB sums positive operands too: its random bias is shifted by each colour's mean, so that the u8 image does not saturate
    key = "%d_conv_to_rgb_bias" % 2 ** gcfg["max_res_log2"]
    gp[key] = (gp[key] - rgb.mean(axis=(0, 2, 3))).astype(np.float32)
    feats_w = o.generator_w(exact_dlatents(o, gcfg, batch, seed)[idx], nc)[2]
    feats = [np.concatenate([a, b]) for a, b in zip(feats_z, feats_w)]
    dp = _Calibrator(dcfg, np.random.Generator(np.random.PCG64(seed + 1))).run(feats, final_seed=3)
    return gcfg, gp, dcfg, dp, z, noise


def exact_setup(name, batch, seed=SEED):
    """(gcfg, gp, dcfg, dp, z, noise) of the exactly summable fixture `name` (EXACT_FORMS) for `batch` samples, as
    tests.common.form_setup returns them, with use_wscale=False.  The decoder is calibrated on checked_samples(batch) of the z path and of
    the W path (exact_dlatents): those are the samples whose exactness tests/test_exact_bf16_host.py asserts and the GPU tests compare.
    Cached; the caller must not modify what it gets (copy a dict before changing a weight)."""
    return _exact_setup(name, batch, seed)
