"""Every batch-dependent launch form at full size, fp32 and bf16.

DESIGN.md section 1: the dataset is byte-identical for any batch size, rank count or GPU count.  The canonical arithmetic is static
(Winograd, K-split and sub-pixel rules depend on a layer's shape only), but the launch form that runs a layer depends on the batch
size n: pick_geom, launch_conv_t, subpixel_cout_tile / subpixel_res_lds / subpixel_wst_lds, launch_wino_t, the persistent tile ranges
of gsa_wino_lean.hip's launch_t / launch_stream_t, bf16_lean_nt.  The reduced configurations (<= 64 channels) never reach the forms of
the 256- and 512-channel layers, so this module runs ffhq 1024, cars 512 and bedrooms 256 at every batch of SWEEP -- and cars up to 128 and
bedrooms up to 256 samples at the batches of SWEEP_BEYOND (tests/common.py SWEEP_MAX) -- in both modes:

 * coverage guard: the (layer, kernel) pairs of the model's sweep batches include every pair any batch in 1..SWEEP_MAX[gan] launches
   (tests/dispatch_map.py);
 * batch composition: every sample of every sweep batch has the bytes of the same sample run alone (torch.equal on the device) --
   the fused step's u8 pair, the two-call path's fp32 rgb and logits, and all features of the batch's first and last sample;
 * the batch-1 run against the C oracle: the digests of tests/golden/sweep_anchors.json (fp32), the contract of
   tests/test_gpu_bf16.py against Oracle(precision="bf16") (bf16);
 * the downscaled pair (f = 2) at the largest batch and at a breakpoint batch: the rule of tests/test_downscale_host.py on that batch's
   own two-call rgb and logits;
 * hipGraph replay at full size in the configurations that replay by default (ffhq fp32 batch 2, cars bf16 batch 4).
"""
import gc
import hashlib
import json
import os

import numpy as np
import pytest

from tests import dispatch_map as DM
from tests.common import SWEEP_MAX, gan_setup, sweep_setup
from tests.test_downscale_host import rule_image, rule_mask
from tests.test_gpu_bf16 import _check_against, check_first_level

pytestmark = pytest.mark.gpu

# The batches every test below runs: 1, 2, 8, 16, 32 and 64, and both sides of every rule that changes a layer's launch form with the
# batch n.  The measured dispatch map (`python -m tests.dispatch_map <gan> <precision>`, MI355X) changes at 2, 4, 8, 16, 32 and 64 for
# ffhq, cars and bedrooms in fp32 and in bf16.  The grid thresholds below are derived from the launch helpers for 256 CUs; t = 16x16
# tiles per sample (1 at 16 px, 4 at 32, 16 at 64, 64 at 128, 256 at 256); "a/b" = the last batch of one form and the first of the next.
SWEEP = [
    1, 2,    # map 1/2: g.128.deconv_1 / d.main_5.a 16 -> 32-channel sub-pixel tile, g.256.deconv_1 streamed; bf16_lean_nt of g.128 / g.256.conv_2,
    #          d.cvt_6, d.main_5.b.  Grids: launch_stream_t d.cvt_6 (256n > 256 slots), launch_t d.main_5.b (256n > 256)
    3, 4,    # map 3/4: g.64.conv_1 32-channel tile, g.128.deconv_1 streamed, g.512.deconv_1 resident panel (1024n >= 4096 tiles).  Grids 2/3:
    #          launch_stream_t g.64.conv_2 (16n > 32 slots); bf16 g.64.conv_2 NT=1 (16n > 32), g.128.conv_2 NT=2 (64n > 128), g.256.conv_2
    #          NT=4 (256n > 512), d.main_5.b NT=2 (256n > 512).  3/4: bf16 d.cvt_6 NT=2 (256n > 768)
    5,       # grids 4/5: launch_stream_t g.32.conv_2 (4n > 16) and d.cvt_5 (64n > 256), launch_t d.main_4.b (64n > 256); bf16 g.32.conv_2 NT=1
    #          (4n > 16), g.64.conv_2 NT=2 (16n > 64), g.128.conv_2 NT=4 (64n > 256)
    6, 7,    # grids 6/7: bf16 d.cvt_5 / d.main_4.b NT=1 (64n > 384 slots)
    8, 9,    # map 7/8: g.32.conv_1 32-channel tile, g.64.conv_1 streamed, bf16_lean_nt of g.32 / g.64.conv_2, d.cvt_5, d.main_4.b, pick_geom of the
    #          bf16 g.16.conv_2.  Grids 8/9: bf16 g.32.conv_2 NT=2 (4n > 32), g.64.conv_2 NT=4 (16n > 128), d.main_4.b NT=2 (64n > 512)
    12, 13,  # grids 12/13: bf16 d.cvt_5 NT=2 (64n > 768)
    15, 16,  # map 15/16: g.32.conv_1 / d.main_4.a streamed, bf16 g.32.conv_2 NT=4, bf16 g.16.conv_2 tile geometry
    17,      # grids 16/17: launch_stream_t g.16.conv_2 (n > 16 slots) and d.cvt_4 (16n > 256); launch_t d.main_3.b (16n > 256); bf16 g.32.conv_2
    #          NT=4 (4n > 64)
    24, 25,  # grids 24/25: bf16 d.cvt_4 / d.main_3.b NT=1 (16n > 384)
    31, 32,  # map 31/32: g.16.conv_1 / d.main_3.a 32-channel tile, pick_geom of d.main_2.b (conv3x3_mfma, 16n x 2 groups >= 512), bf16_lean_nt of
    #          d.cvt_4 / d.main_3.b
    33,      # grids 32/33: bf16 d.main_3.b NT=2 (16n > 512)
    48, 49,  # grids 48/49: launch_conv_t d.main_2.b persistent (16n tiles > 256 CUs x 3 workgroups: LDS-bound); bf16 d.cvt_4 NT=2 (16n > 768)
    63, 64,  # map 63/64: g.16.conv_1 / d.main_3.a streamed (fp32: the lean sub-pixel kernel), pick_geom of d.main_2.b and the bf16 g.16.conv_2
]

# Beyond 64 (tests/common.py SWEEP_MAX: cars to 128, bedrooms to 256, ffhq stays at 64): both sides of every batch at which the measured
# map of the model changes there, in either mode, plus 65, 128, 129 and the maximum.  Measured (`python -m tests.dispatch_map <gan> <precision>`,
# MI355X): beyond 64 the map changes at 128 for cars and at 128 and 256 for bedrooms, in fp32 and in bf16 alike.
SWEEP_BEYOND = {
    "ffhq": [],
    "cars": [
        65,          # the first batch beyond the swept 1..64 (five 16-sample chunks for four mapping slices: tests/test_gpu_large_batch.py)
        127, 128,    # map 127/128, the only change in 65..128, fp32 and bf16: d.main_1.b conv3x3_mfma<8, 8, 4, 1, 1 -> 2, 2>, d.main_2.a subpixel_mfma<1 -> 2,
        #              2>, d.main_2.b conv3x3_mfma<16, 16, 4, 1, 1 -> 2, 2> (bf16: conv3x3_bf16_lean NT 1 -> 2); bf16 g.16.conv_1 subpixel_mfma -> subpixel_res.
        #              128 is the maximum (and the last batch with one round of the style kernels)
    ],
    "bedrooms": [
        65,          # the first batch beyond the swept 1..64 (five 16-sample chunks for four mapping slices)
        127, 128,    # map 127/128: the same changes as cars at 128 (d.main_1.b, d.main_2.a, d.main_2.b geometry; bf16 g.16.conv_1 -> subpixel_res)
        129,         # the style kernels' second round (grid.y = 8 rows of 16 samples), a ninth mapping chunk
        255, 256,    # map 255/256, the only other change in 65..256: d.main_1.b conv3x3_mfma<8, 8, 4, 1, 2, 2> -> <16, 16, 4, 1, 1, 2>, d.main_2.a
        #              subpixel_mfma<2, 2> -> lean::subpixel_lean (bf16: subpixel_res<.., 1, true>), bf16 d.main_3.a subpixel_res<.., 1, true> -> <.., 2,
        #              false>.  256 is the maximum
    ],
}


def sweep_batches(gan):
    return SWEEP + SWEEP_BEYOND[gan]


def test_sweep_lists_reach_each_models_maximum():
    for gan, top in SWEEP_MAX.items():
        bs = sweep_batches(gan)
        assert bs == sorted(set(bs)) and bs[-1] == top
        if top > 64:
            assert {b for b in (65, 128, 129, top) if b <= top} <= set(bs)


CASES = [(g, p) for g in ("ffhq", "cars", "bedrooms") for p in ("fp32", "bf16")]


def _digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def _golden_anchors():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_anchors.json")) as f:
        return json.load(f)


class Sweep:
    """One GAN in one mode: the generator reserved for the model's sweep maximum, the sweep inputs on the device, and what each sample
    gives alone."""

    def __init__(self, gan, precision):
        self.gan, self.precision = gan, precision
        self.gen, self.z, self.noise = DM.build(gan, precision)
        self.max_batch, self.batches = SWEEP_MAX[gan], sweep_batches(gan)
        self._maps = {}
        self._alone = {}

    def sl(self, lo, hi):
        return self.z[lo:hi], [a[lo:hi] for a in self.noise]

    def map(self, b):
        if b not in self._maps:
            self._maps[b] = DM.dispatch_map(self.gen, self.z, self.noise, b)
        return self._maps[b]

    def alone(self, i):
        """Sample i at batch 1: (image, mask) of the fused step, (rgb, logits, features) of the two-call path (the features only for
        the first and last samples of the SWEEP batches)."""
        if i not in self._alone:
            img, mask = DM.run_path(self.gen, "generate", *self.sl(i, i + 1))
            rgb, feats, _img, logits, _mask = DM.run_path(self.gen, "two_call", *self.sl(i, i + 1))
            self._alone[i] = (img, mask, rgb, logits, feats if i == 0 or i + 1 in self.batches else None)
        return self._alone[i]

    def release(self):
        del self.gen, self.z, self.noise
        self._alone.clear()
        gc.collect()
        import torch
        torch.cuda.empty_cache()


@pytest.fixture(scope="module", params=CASES, ids=["%s-%s" % c for c in CASES])
def sweep(request, torch_cuda):
    s = Sweep(*request.param)
    yield s
    s.release()


def test_sweep_covers_every_dispatch_form(sweep):
    """Every (layer, kernel) pair that some batch in 1..SWEEP_MAX[gan] launches is launched by a batch of the model's sweep list."""
    first = {}
    for b in range(1, sweep.max_batch + 1):
        for pair in sweep.map(b):
            first.setdefault(pair, b)
    covered = frozenset().union(*(sweep.map(b) for b in sweep.batches))
    missing = sorted((b, layer, kernel) for (layer, kernel), b in first.items() if (layer, kernel) not in covered)
    assert not missing, "%s %s: pairs no SWEEP batch launches:\n%s" % (
        sweep.gan, sweep.precision, "\n".join("  %s  %s  (first at batch %d)" % (layer, kernel, b) for b, layer, kernel in missing))


def test_batch_composition_at_every_sweep_batch(sweep):
    """Each sample of a batch of the model's sweep list == the same sample at batch 1: the fused u8 pair, the two-call rgb and logits,
    and every feature map of the batch's first and last sample."""
    import torch
    for B in sweep.batches:
        img, mask = DM.run_path(sweep.gen, "generate", *sweep.sl(0, B))
        rgb, feats, _img2, logits, _mask2 = DM.run_path(sweep.gen, "two_call", *sweep.sl(0, B))
        for i in range(B):
            a_img, a_mask, a_rgb, a_logits, a_feats = sweep.alone(i)
            what = "%s %s batch %d sample %d" % (sweep.gan, sweep.precision, B, i)
            assert torch.equal(img[i:i + 1], a_img), what + ": fused image differs from the sample alone"
            assert torch.equal(mask[i:i + 1], a_mask), what + ": fused mask differs from the sample alone"
            assert torch.equal(rgb[i:i + 1], a_rgb), what + ": rgb differs from the sample alone"
            assert torch.equal(logits[i:i + 1], a_logits), what + ": logits differ from the sample alone"
            if i in (0, B - 1):
                for k, (f, a) in enumerate(zip(feats, a_feats)):
                    assert torch.equal(f[i:i + 1], a), "%s: feature %d (%d px) differs from the sample alone" % (what, k, f.shape[-1])
        del img, mask, rgb, feats, logits


# rgb max of test_batch1_against_the_oracle (bf16).  The contract's 3 % does not hold on these z-dependent mapping weights, as it does not
# for cars in tests/test_gpu_bf16.py's _LIVE_BARS: live styles amplify flipped bf16 roundings, and the bf16 oracle itself is as far from
# the fp32 oracle as the HIP path is.  Sample 0, batch 1, rgb max / mean of the range, mask agreement:
#   HIP bf16 vs bf16 oracle      ffhq 4.58 % / 0.089 % / 99.62 %   cars 3.08 % / 0.18 % / 99.61 %   bedrooms 3.03 % / 0.19 % / 99.86 %
#   bf16 oracle vs fp32 oracle   ffhq 8.27 % / 0.13 % / 99.35 %    cars 5.26 % / 0.27 % / 99.44 %   bedrooms 4.21 % / 0.28 % / 99.76 %
#   HIP bf16 vs HIP fp32         ffhq 5.26 % / 0.13 % / 99.37 %    cars 5.34 % / 0.27 % / 99.46 %   bedrooms 4.74 % / 0.28 % / 99.79 %
# The 4x4 level holds the contract (one isolated flip of 8192 values, 3.3e-6 of the range, in each GAN); the per-level distance to the
# fp32 path grows alike in both (7e-3 at 4x4 to 5-13e-2 at the last level).  Mean and mask agreement keep the contract's bars.
_SWEEP_BF16_MAX = {"ffhq": 6e-2, "cars": 4e-2, "bedrooms": 4e-2}


def test_batch1_against_the_oracle(sweep, oracle_lib):
    """fp32: sample 0 at batch 1 has the C oracle's digests (tests/golden/sweep_anchors.json, make_sweep_anchors.py).
    bf16: against Oracle(precision="bf16") under tests/test_gpu_bf16.py's contract -- the 4x4 level to fp32 rounding (with the
    isolated-flip allowance of its 512 channels), end to end rgb mean 0.3 % of the range, masks agree on 99.5 %, rgb max as
    _SWEEP_BF16_MAX states."""
    img, mask, rgb, logits, feats = sweep.alone(0)
    if sweep.precision == "fp32":
        want = _golden_anchors()[sweep.gan]
        got = {"image_u8": img, "mask_u8": mask, "rgb_f32": rgb, "logits_f32": logits, "feature_last_f32": feats[-1],
               "feature_second_last_f32": feats[-2]}
        for k, t in got.items():
            assert _digest(t) == want[k], "%s batch 1 sample 0: %s differs from the oracle's" % (sweep.gan, k)
        return
    gcfg, gp, dcfg, dp, z, noise = sweep_setup(sweep.gan)
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp, precision="bf16")
    rgb_o, _img_o, feats_o = o.generator(z[:1], [a[:1] for a in noise])
    _logits_o, mask_o = o.decoder(feats_o)
    f0, f0_o = feats[0].cpu().numpy(), feats_o[0]
    n_off, d_max = check_first_level(f0, f0_o, isolated_flips=True)
    rgb_np, mask_np = rgb.cpu().numpy(), mask.cpu().numpy()
    d = np.abs(rgb_np.astype(np.float64) - rgb_o) / np.abs(rgb_o).max()
    print("%s bf16 vs bf16 oracle: 4x4 %d values beyond 2e-6 (max %.2e); rgb max %.3e mean %.3e; masks %.5f" % (
        sweep.gan, n_off, d_max, d.max(), d.mean(), float(np.mean(mask_np == mask_o))))
    _check_against(rgb_np, mask_np, rgb_o, mask_o, _SWEEP_BF16_MAX[sweep.gan], 3e-3, 0.995, "%s bf16 HIP vs bf16 oracle" % sweep.gan)


@pytest.mark.parametrize("B", [SWEEP[-1], 32])
def test_downscaled_pair_at_sweep_batches(sweep, B):
    """At the largest SWEEP batch and at a breakpoint batch: the f = 2 pair of gsa_generate_downscaled, in the generator's own
    context and workspace, == the rule on the same batch's two-call rgb and logits."""
    import torch
    gen = sweep.gen
    g = gen.netG
    ctx, dev = g._model.ctx, g._model.device
    z, noise = sweep.sl(0, B)
    R = 2 ** gen.max_res_log2 // 2
    img = torch.empty((B, R, R, 3), device=dev, dtype=torch.uint8)
    mask = torch.empty((B, R, R), device=dev, dtype=torch.uint8)
    ctx.generate_downscaled(torch.cuda.current_stream(dev).cuda_stream, B, z.data_ptr(), None, 0, [a.data_ptr() for a in noise], 2,
                            img.data_ptr(), mask.data_ptr())
    rgb, feats, _img, logits, _mask = DM.run_path(gen, "two_call", z, noise)
    del feats
    want_img, want_mask = rule_image(rgb.cpu().numpy(), 2), rule_mask(logits.cpu().numpy(), 2)
    got_img, got_mask = img.cpu().numpy(), mask.cpu().numpy()
    assert np.array_equal(got_img, want_img), "%s %s batch %d: %d image values differ from the rule" % (
        sweep.gan, sweep.precision, B, int((got_img != want_img).sum()))
    assert np.array_equal(got_mask, want_mask), "%s %s batch %d: %d mask values differ from the rule" % (
        sweep.gan, sweep.precision, B, int((got_mask != want_mask).sum()))


@pytest.mark.parametrize("gan,precision,batch", [("ffhq", "fp32", 2), ("cars", "bf16", 4)])
def test_graph_replay_at_full_size(torch_cuda, monkeypatch, gan, precision, batch):
    """The configurations that replay a captured hipGraph by default (fp32 at batch <= 2, bf16 at every batch), at full size: the
    same input tensors rewritten in place between calls, capture after 3 calls -- every step has the eager bytes of its inputs."""
    from gan_segmentation_amd.image_generator import ImageGenerator
    torch = torch_cuda
    monkeypatch.delenv("GSA_GRAPH", raising=False)
    gcfg, gp, dcfg, dp, _z, _noise = gan_setup(gan, 1, live_mapping=True)
    _gcfg, _gp, _dcfg, _dp, z, noise = sweep_setup(gan)
    gen = ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=batch, precision=precision)
    gen.graph_mode = "0"
    want = [[t.cpu().numpy() for t in gen.generate_batch(z[k:k + batch], [a[k:k + batch] for a in noise])] for k in (0, batch)]
    gen.graph_mode, gen.graph_after = None, 3
    zt = torch.from_numpy(z[:batch].copy()).cuda()
    nt = [torch.from_numpy(a[:batch].copy()).cuda() for a in noise]
    R = 2 ** gcfg["max_res_log2"]
    out = (torch.empty((batch, R, R, 3), dtype=torch.uint8, device="cuda"), torch.empty((batch, R, R), dtype=torch.uint8, device="cuda"))
    for it in range(10):                                  # calls 0-1 eager, call 2 captured and replayed, 3-9 replays
        k = 0 if it % 2 == 0 else batch
        zt.copy_(torch.from_numpy(z[k:k + batch].copy()))
        for t, a in zip(nt, noise):
            t.copy_(torch.from_numpy(a[k:k + batch].copy()))
        out[0].zero_(); out[1].zero_()
        img, mask = gen.generate_batch(zt, nt, out=out)
        assert np.array_equal(img.cpu().numpy(), want[it % 2][0]), "%s %s batch %d: image of call %d" % (gan, precision, batch, it)
        assert np.array_equal(mask.cpu().numpy(), want[it % 2][1]), "%s %s batch %d: mask of call %d" % (gan, precision, batch, it)
    assert gen.graphs_captured() == 1, "the repeated call was never captured"
    assert not np.array_equal(want[0][0], want[1][0])
