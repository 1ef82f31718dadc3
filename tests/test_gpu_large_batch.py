"""More than 64 samples in one call, on the reduced 128 px model, against the C oracle.

The reduced configuration has latent size 512, so it takes the mapping and style launches of the real models.  Beyond 64 samples
these launches change form (csrc/gsa_kernels.hip launch_mapping / launch_styles, csrc/gsa_wspace.hip launch_styles_dlatents):

 * mapping_kernel runs slices = min(ceil(n/16), kMapSlices, (CUs/2) / (L/16)) copies of the tag exchange side by side -- 4 on the
   256 CUs of an MI355X at L = 512 -- so from n = 65 on a slice walks more than one 16-sample chunk inside ONE launch: chunk
   y, then y + slices, ... with the same launch number in its tags;
 * dense_lds_kernel<STYLE> and dlatent_styles_kernel run grid.y = min(ceil(n/16), 8), so from n = 129 on a workgroup takes a
   second round of `for (n0 = 16*blockIdx.y; n0 < n; n0 += 16*gridDim.y)`.

BATCHES: 65 (slice 0 walks a second chunk, which holds a single sample), 80 (a full second chunk for slice 0, none for the others),
128 (two chunks for every slice; the last batch with one round of the style kernels), 129 (a ninth chunk: slice 0 walks three, the
style kernels' second round holds one sample) and 160 (ten chunks: two slices walk three, two rounds for two rows of the style grids).
Weights whose w depends on z (tests.common.lively), every sample different; fp32 bit for bit against the oracle as
tests/test_gpu_wspace_exact.py does for small batches, bf16 under the contract of tests/test_gpu_bf16.py."""
import os
import re

import numpy as np
import pytest

from tests.common import reduced_setup, w_spread
from tests.test_gpu_bf16 import _check_against, check_first_level
from tests.test_gpu_wspace_exact import _layers, _rows, _same, _w_scale

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = [65, 80, 128, 129, 160]
STYLE_GRID_ROWS = 8          # launch_styles / launch_styles_dlatents: grid.y = min(ceil(n/16), 8)


def _source(name):
    with open(os.path.join(ROOT, "gan-segmentation_amd", "csrc", name)) as f:
        return f.read()


def map_slices_limit():
    """kMapSlices of csrc/gsa_kernels.h."""
    return int(re.search(r"constexpr int kMapSlices = (\d+);", _source("gsa_kernels.h")).group(1))


def mapping_slices(n, L, cus):
    """launch_mapping's rule, restated: the slices of one mapping_kernel launch."""
    return max(1, min(min((n + 15) // 16, map_slices_limit()), (cus // 2) // (L // 16)))


def test_the_launch_rules_are_the_ones_these_tests_assume():
    k = _source("gsa_kernels.hip")
    assert "const int slices = std::max(1, std::min(std::min((n + 15) / 16, kMapSlices), (device_cus(device) / 2) / (L / 16)));" in k
    assert "dim3((J + 63) / 64, std::min((n + 15) / 16, 8))" in k
    assert "dim3(num_tiles, std::min((n + 15) / 16, 8))" in _source("gsa_wspace.hip")
    # on 256 CUs at L = 512: 4 slices, so every batch of BATCHES has more chunks than slices
    for n in BATCHES:
        assert (n + 15) // 16 > mapping_slices(n, 512, 256) == 4


class Large:
    """The reduced model with live mapping weights, 160 different samples, the oracle and one generator in one mode."""

    def __init__(self, oracle_lib, precision):
        import torch
        from gan_segmentation_amd.image_generator import ImageGenerator
        self.gcfg, gp, dcfg, dp, self.z, self.noise = reduced_setup(7, batch=max(BATCHES), live_mapping=True)
        self.o = oracle_lib.Oracle(self.gcfg, gp, dcfg, dp, precision=precision)
        self.gen = ImageGenerator.from_params(self.gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=max(BATCHES), precision=precision)
        self.gen.graph_mode = "0"
        self.scale = _w_scale(self.o)
        self.cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert self.gcfg["latent_size"] == 512

    def inputs(self, n):
        """z, noise and per-layer dlatents (an independent row per sample and layer, at w's scale) of samples 0..n-1."""
        return self.z[:n], [a[:n] for a in self.noise], _rows(n, _layers(self.gcfg), self.scale, seed=n)

    def assert_second_form(self, n):
        """The case really runs the forms this module is about: fewer mapping slices than 16-sample chunks (a change of kMapSlices or
        of the co-residency rule must not quietly turn it into the one-chunk-per-slice form), and beyond 128 samples more chunks
        than the style grids have rows."""
        chunks = (n + 15) // 16
        slices = mapping_slices(n, self.gcfg["latent_size"], self.cus)
        assert slices < chunks, "batch %d: %d mapping slices for %d chunks on %d CUs -- no slice walks a second chunk" % (n, slices, chunks, self.cus)
        assert (chunks > STYLE_GRID_ROWS) == (n > 128)


@pytest.fixture(scope="module")
def large_fp32(torch_cuda, oracle_lib):
    return Large(oracle_lib, "fp32")


@pytest.fixture(scope="module")
def large_bf16(torch_cuda, oracle_lib):
    return Large(oracle_lib, "bf16")


@pytest.mark.gpu
@pytest.mark.parametrize("n", BATCHES)
def test_large_batch_is_bit_exact(large_fp32, n):
    """gsa_mapping_forward's w, the fused generate pair and the W path's pair (generate_w on independent rows per layer) of ALL n
    samples == the oracle; gsa_check stays clean (no mapping time-out word)."""
    s = large_fp32
    s.assert_second_form(n)
    z, noise, dl = s.inputs(n)
    w_o = s.o.mapping(z)
    assert w_spread(w_o) > 0.1, "precondition: w must depend on z"
    assert w_spread(dl[:, 0]) > 0.1 and np.abs(dl[:, 0] - dl[:, 1]).max() > 0.1, "precondition: the rows differ per sample and per layer"
    _same(s.gen.netG.mapping(z).cpu().numpy(), w_o, "w at batch %d" % n)
    img, mask = s.gen.generate_batch(z, noise)
    img_o, mask_o = s.o.generate(z, noise)
    _same(img.cpu().numpy(), img_o, "batch %d: image" % n)
    _same(mask.cpu().numpy(), mask_o, "batch %d: mask" % n)
    img, mask = s.gen.generate_batch_w(dl, noise)
    img_o, mask_o = s.o.generate_w(dl, noise)
    _same(img.cpu().numpy(), img_o, "batch %d: W path image" % n)
    _same(mask.cpu().numpy(), mask_o, "batch %d: W path mask" % n)
    s.gen.netG._model.ctx.check()


def _boundary_samples(n):
    """Both sides of every chunk, slice-loop and style-round boundary that n has."""
    return sorted(i for i in {0, 15, 16, 63, 64, 79, 80, 127, 128, 143, 144, n - 1} if i < n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", BATCHES)
def test_large_batch_in_bf16_mode(large_bf16, n):
    """bf16 mode (the mapping and style arithmetic stays fp32): w == the oracle's bit for bit; the z path and the W path on the
    samples beside every chunk and round boundary hold the contract of tests/test_gpu_bf16.py against Oracle(precision="bf16") --
    the 4x4 level to fp32 rounding (isolated bf16 flips as check_first_level allows them), rgb max 3 % / mean 0.3 % of the range, masks
    agree on 99.5 %; and every sample of the 4x4 level and of the fused pairs has the bytes it has in a batch of at most 16 (one chunk,
    one slice, one round: the forms tested before)."""
    import torch
    s = large_bf16
    s.assert_second_form(n)
    z, noise, dl = s.inputs(n)
    g = s.gen.netG
    _same(g.mapping(z).cpu().numpy(), s.o.mapping(z), "bf16 mode: w at batch %d" % n)
    sel = _boundary_samples(n)
    for path in ("z", "w"):
        if path == "z":
            rgb, feats = g(z, noise=noise)
            rgb_o, _img_o, feats_o = s.o.generator(z[sel], [a[sel] for a in noise])
        else:
            rgb, feats = g.synthesis(dl, noise=noise)
            rgb_o, _img_o, feats_o = s.o.generator_w(dl[sel], [a[sel] for a in noise])
        _logits, mask = s.gen._decoder(*feats, want_mask=True)
        _logits_o, mask_o = s.o.decoder(feats_o)
        # the 4x4 level with the isolated-flip allowance of check_first_level, as the full-size bf16 tests use it: where the matrix core's
        # summation order flips the bf16 rounding of ONE stored value, that value is one bf16 step off (measured here: one value among
        # the compared samples, 5.6e-5 of the range at 65..128 and 5.2e-5 at 129 and 160; the three samples of tests/test_gpu_bf16.py hold
        # none).  A flip belongs to a sample's values, not to the batch's launch form: the level has the same bytes in batches of 16 (below).
        f0 = feats[0]
        check_first_level(f0.cpu().numpy()[sel], feats_o[0], isolated_flips=True)
        for lo in range(0, n, 16):
            hi = min(lo + 16, n)
            part = g(z[lo:hi], noise=[a[lo:hi] for a in noise])[1][0] if path == "z" else g.synthesis(dl[lo:hi], noise=[a[lo:hi] for a in noise])[1][0]
            assert torch.equal(f0[lo:hi], part), "batch %d, %s path: the 4x4 level of samples %d..%d differs from their own batch" % (n, path, lo, hi - 1)
        # sample by sample: a sample that took another one's styles must not hide in the batch's mean
        for k, i in enumerate(sel):
            _check_against(rgb[i:i + 1].cpu().numpy(), mask[i:i + 1].cpu().numpy(), rgb_o[k:k + 1], mask_o[k:k + 1], 3e-2, 3e-3, 0.995,
                           "batch %d sample %d, %s path: bf16 HIP vs bf16 oracle" % (n, i, path))
        del rgb, feats, mask, f0
    img, mask = s.gen.generate_batch(z, noise)
    img_w, mask_w = s.gen.generate_batch_w(dl, noise)
    for lo in range(0, n, 16):
        hi = min(lo + 16, n)
        a_img, a_mask = s.gen.generate_batch(z[lo:hi], [a[lo:hi] for a in noise])
        assert torch.equal(img[lo:hi], a_img) and torch.equal(mask[lo:hi], a_mask), "batch %d: samples %d..%d differ from their own batch" % (n, lo, hi - 1)
        a_img, a_mask = s.gen.generate_batch_w(dl[lo:hi], [a[lo:hi] for a in noise])
        assert torch.equal(img_w[lo:hi], a_img) and torch.equal(mask_w[lo:hi], a_mask), "batch %d: W path samples %d..%d differ from their own batch" % (n, lo, hi - 1)
    s.gen.netG._model.ctx.check()
