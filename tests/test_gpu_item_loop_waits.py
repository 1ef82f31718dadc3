"""The item loops of the lean convolution kernels after their vector-memory waits moved: the wait
for the prefetched activations -- and, in the streamed forms, for the LDS-DMA weight pieces -- sits behind an item's MFMA phase, the
closing barrier no longer drains the tile-end stores and the statistics atomics, and the next item stages while they are in flight.
None of that is arithmetic: every output equals the C oracle bit for bit, through the C ABI, on shapes where every touched loop runs
at least three items per persistent workgroup (256 CUs: at most 512 workgroups per launch) and some workgroup's range crosses an
item that ends a tile, one that does not, and a sample boundary:

  * 16 channels at 512^2 and 32 at 256^2, batch 3: conv3x3_wino_lean 16 -> 16 (3072 tiles: 6 per workgroup, 1024 per sample) in its
    synthesis, decoder + residual and fused-toRGB decoder forms, 32 -> 32 (768 tiles of two blocks: 3 tiles = 6 items per workgroup,
    256 per sample), post_dma -- and the STREAMED subpixel_lean: a stride-2 layer keeps its panel resident from 4096 tiles on
    (subpixel_plan), which 1024 tiles per sample reach at batch 4;
  * the same model, and one with 32 channels at 512^2 and 64 at 256^2, at batch 5 (5120 tiles: 20 per workgroup, 10 per half): the
    resident subpixel_lean forms with two blocks per item (32 -> 16) and with one (64 -> 32: the panel leaves room for no more);
  * 128 channels up to 128^2 with a 64-wide decoder, batch 3: the streamed four-wave and paired kernels (at 128^2: 192 tiles per output
    group over 64 workgroups = 3 tiles of 8 or 4 blocks each, 64 tiles per sample), once with GSA_WINO_PAIR=2 (paired wherever the
    groups pair up) and once with 0 (never).  (Its stride-2 layers are too small for the persistent forms: subpixel_mfma.)

Each model generates twice on the same context: the second pass equals the oracle only if the direct-statistics rows the first one
accumulated into were back at zero (the atomics that fill them are what now stays in flight across the barrier)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 3


def resident_setup():
    """Channels 64 x 6, 32, 16 at 4 .. 512 px; the decoder's last level 16 wide, as the 1024 px decoder's."""
    from gan_segmentation_amd import weights as W
    gcfg = W.generator_config(max_res_log2=9, fmap_base=4096, fmap_max=64)
    dcfg = W.decoder_config(9, in_channels=W.generator_channels(gcfg))
    dcfg["features"][-2] = 16
    return gcfg, dcfg


def streamed_setup():
    """128 channels at every level up to 128 px, a decoder 64 wide at every level."""
    from gan_segmentation_amd import weights as W
    gcfg = W.generator_config(max_res_log2=7, fmap_base=8192, fmap_max=128)
    dcfg = W.decoder_config(7, in_channels=W.generator_channels(gcfg))
    dcfg["features"] = [64] * 6 + [2]
    return gcfg, dcfg


def resident_wide_setup():
    """Channels 64 x 7, 32 at 4 .. 512 px: the 64 -> 32 stride-2 layer at 512^2 holds its panel with one block per item."""
    from gan_segmentation_amd import weights as W
    gcfg = W.generator_config(max_res_log2=9, fmap_base=8192, fmap_max=64)
    dcfg = W.decoder_config(9, in_channels=W.generator_channels(gcfg))
    return gcfg, dcfg


def model(setup, batch=BATCH):
    from gan_segmentation_amd import weights as W
    gcfg, dcfg = setup()
    gp = W.synthetic_generator_params(gcfg, seed=2, trivial_norm=False)
    dp = W.synthetic_decoder_params(dcfg, seed=3)
    z, noise = W.synthetic_inputs(gcfg, batch)
    return gcfg, gp, dcfg, dp, z, noise


def generate_twice(setup, img_o, mask_o, batch=BATCH):
    """Two passes on one context against the oracle's pair; returns the kernels the second pass launched."""
    import torch
    from gan_segmentation_amd.image_generator import ImageGenerator
    gcfg, gp, dcfg, dp, z, noise = model(setup, batch)
    gen = ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=batch)
    ctx = gen.netG._model.ctx
    kernels = []
    for k in range(2):
        if k == 1:
            ctx.profile_enable(2)
            ctx.profile_reset()
        img, mask = gen.generate_batch(z, noise)
        torch.cuda.synchronize()
        if k == 1:
            kernels = sorted({e["name"].partition(" | ")[0] for e in ctx.profile_entries()})
            ctx.profile_enable(0)
        img, mask = img.cpu().numpy(), mask.cpu().numpy()
        assert img.shape == img_o.shape and mask.shape == mask_o.shape
        assert np.array_equal(img, img_o), "pass %d: image differs from the oracle in %d bytes" % (k, int((img != img_o).sum()))
        assert np.array_equal(mask, mask_o), "pass %d: mask differs from the oracle in %d pixels" % (k, int((mask != mask_o).sum()))
    return kernels


def has(kernels, *parts):
    return any(all(p in k for p in parts) for k in kernels)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def test_resident_item_loops_equal_the_oracle_twice(torch_cuda, oracle_lib):
    gcfg, gp, dcfg, dp, z, noise = model(resident_setup)
    img_o, mask_o = oracle_lib.Oracle(gcfg, gp, dcfg, dp).generate(z, noise)
    kernels = generate_twice(resident_setup, img_o, mask_o)
    print("\n".join(kernels))
    # template arguments: <EPI (1 synthesis, 2 decoder), AFF, RES, NB, GW, DB, PF, RGB>
    assert has(kernels, "lean::conv3x3_wino_lean<1, ", ", 1, 1, true, 1, false>"), "16 -> 16, synthesis epilogue"
    assert has(kernels, "lean::conv3x3_wino_lean<2, ", "true, 1, 1, true, 1, false>"), "16 -> 16, decoder epilogue + residual"
    assert has(kernels, "lean::conv3x3_wino_lean<2, true, false, 1, 1, true, 1, true>"), "16 -> 16, decoder epilogue with toRGB inside"
    assert has(kernels, "lean::conv3x3_wino_lean<1, ", ", 2, 2, true, 1, false>"), "32 -> 32, synthesis epilogue"
    assert has(kernels, "lean::conv3x3_wino_lean<2, ", ", 2, 2, true, 1, false>"), "32 -> 32, decoder epilogue"
    # <NT, EPI, SC, AFF, KB, WST, CNT>
    assert has(kernels, "lean::subpixel_lean<", ", 1, true, false>"), "streamed subpixel_lean"
    assert has(kernels, "post_dma"), "post_dma"


@pytest.mark.parametrize("setup,kb", [(resident_setup, 2), (resident_wide_setup, 1)])
def test_resident_stride2_item_loops_equal_the_oracle_twice(torch_cuda, oracle_lib, setup, kb):
    gcfg, gp, dcfg, dp, z, noise = model(setup, 5)
    img_o, mask_o = oracle_lib.Oracle(gcfg, gp, dcfg, dp).generate(z, noise)
    kernels = generate_twice(setup, img_o, mask_o, 5)
    print("\n".join(kernels))
    assert has(kernels, "lean::subpixel_lean<", ", %d, false, false>" % kb), "resident subpixel_lean, %d block(s) per item" % kb


_WORKER = r'''
import sys
import numpy as np
sys.path.insert(0, ROOT_DIR)
from tests.test_gpu_item_loop_waits import generate_twice, has, streamed_setup
ref = np.load(REF_FILE)
kernels = generate_twice(streamed_setup, ref["img"], ref["mask"])
print("\n".join(kernels))
paired, four_wave = has(kernels, "lean::conv3x3_wino_stream_pair<"), has(kernels, "lean::conv3x3_wino_stream<")
assert paired == (PAIR == "2"), "paired streamed kernel launched: %s" % paired
assert four_wave or PAIR == "2", "four-wave streamed kernel"
print("ITEM_LOOPS_OK")
'''


@pytest.fixture(scope="module")
def streamed_reference(oracle_lib, tmp_path_factory):
    gcfg, gp, dcfg, dp, z, noise = model(streamed_setup)
    img_o, mask_o = oracle_lib.Oracle(gcfg, gp, dcfg, dp).generate(z, noise)
    path = tmp_path_factory.mktemp("item_loops") / "streamed_reference.npz"
    np.savez(path, img=img_o, mask=mask_o)
    return path


@pytest.mark.parametrize("pair", ["2", "0"])
def test_streamed_item_loops_equal_the_oracle_twice(torch_cuda, streamed_reference, tmp_path, pair):
    """A child process each: GSA_WINO_PAIR is read once per process."""
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.replace("ROOT_DIR", repr(ROOT)).replace("REF_FILE", repr(str(streamed_reference))).replace("PAIR", repr(pair)))
    out = subprocess.run([sys.executable, str(script)], env=dict(os.environ, GSA_WINO_PAIR=pair), capture_output=True, text=True, timeout=300)
    print(out.stdout[-4000:])
    assert out.returncode == 0 and "ITEM_LOOPS_OK" in out.stdout, "GSA_WINO_PAIR=%s: %s" % (pair, out.stdout[-1500:] + out.stderr[-3000:])
