"""The pair previews on the GPU (csrc/gsa_overlay.h gsa_overlay; preview.overlay / contact_sheet / write_previews; the
PREVIEW_EVERY key; `annotation --count`): bit for bit the rule of tests/test_preview_host.py, every byte of every sheet.  Every
output is pre-filled with 0xAA, so a byte the call does not write shows, and every input must come back unchanged."""
import os

import numpy as np
import pytest

from tests.test_boundary_host import class_blobs
from tests.test_preview_host import blob_masks, dataset_lut, random_image, random_lut, rule_overlay

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xAA
FACTORS = (1, 2, 4, 8, 16)


def _behind(torch, array, offset):
    """``array`` on the device, ``offset`` bytes into a larger buffer (a fresh allocation is aligned far beyond 4 bytes)."""
    buf = torch.full((array.size + 8,), FILL, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + array.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(array).reshape(-1)))
    assert view.data_ptr() % 4 == offset % 4
    return buf, view


def _call(torch, img, mask, lut, factor=1, cols=1, offsets=(0, 0, 0)):
    """The C entry on raw addresses -> the sheet as a host array; asserts the inputs and the bytes around the output unchanged."""
    from gan_segmentation_amd import _runtime
    n, H, W, C = img.shape
    want_shape = (-(-n // cols) * (H // factor), cols * (W // factor), C)
    size = int(np.prod(want_shape))
    _bi, di = _behind(torch, img, offsets[0])
    _bm, dm = _behind(torch, mask, offsets[1])
    dl = torch.from_numpy(lut).cuda()
    bo = torch.full((size + 8,), FILL, dtype=torch.uint8, device="cuda")
    do = bo[offsets[2]:offsets[2] + size]
    _runtime.launch("gsa_overlay", do.device, n, H, W, C, di.data_ptr(), dm.data_ptr(), dl.data_ptr(), factor, cols, do.data_ptr())
    host = bo.cpu().numpy()
    assert (host[:offsets[2]] == FILL).all() and (host[offsets[2] + size:] == FILL).all(), "bytes around the sheet were written"
    assert np.array_equal(di.cpu().numpy(), img.reshape(-1)) and np.array_equal(dm.cpu().numpy(), mask.reshape(-1)), "an input was written to"
    assert np.array_equal(dl.cpu().numpy(), lut)
    return host[offsets[2]:offsets[2] + size].reshape(want_shape)


def _check(torch, img, mask, lut, factor=1, cols=1, offsets=(0, 0, 0)):
    got, want = _call(torch, img, mask, lut, factor, cols, offsets), rule_overlay(img, mask, lut, factor, cols)
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(want)), "overlay %s f %d cols %d offsets %s: %d of %d bytes differ, first at %s" % (
        img.shape, factor, cols, offsets, int((got != want).sum()), want.size, tuple(np.argwhere(got != want)[0]))
    return want


def _inputs(seed, n, H, W, C):
    return random_image(seed, n, H, W, C), blob_masks(seed, n, H, W), random_lut(seed)


# ---- shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (70, 1)])
def test_thin_planes(torch_cuda, shape):
    _check(torch_cuda, *_inputs(sum(shape), 2, *shape, 3))


@pytest.mark.parametrize("shape", [(16, 16), (63, 65), (65, 63), (64, 64), (66, 131), (32, 128), (33, 129), (31, 127)])
def test_tile_edges(torch_cuda, shape):
    """The issue's shapes, and the sides of the kernel's own 128 x 32 tile and one pixel either way (asserted against the source)."""
    src = open(os.path.join(ROOT, "gan-segmentation_amd", "csrc", "gsa_overlay.hip")).read()
    assert "kTileW = 128;" in src and "kTileH = 32;" in src
    _check(torch_cuda, *_inputs(sum(shape), 2, *shape, 3))


@pytest.mark.parametrize("factor", FACTORS)
def test_every_factor(torch_cuda, factor):
    """(32, 48) and (96, 80) -- more than one tile down, a partial tile across -- and (16, 16), one block at f = 16; W % 4 == 2 in
    the byte form at f = 1 and 2, where a thread's second block lies outside."""
    for H, W in ((32, 48), (96, 80), (16, 16), (64, 272)):
        _check(torch_cuda, *_inputs(factor + H, 2, H, W, 3), factor=factor, cols=2)
    if factor <= 2:
        _check(torch_cuda, *_inputs(factor, 1, 6, 134, 3), factor=factor)


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_channels_and_batch(torch_cuda, C):
    """n = 5 with cols 1, 2 and 5 (3 and 7 as well): with 2 the sixth cell is empty and must be 0; both access forms."""
    for cols in (1, 2, 3, 5, 7):
        for (H, W), f in (((32, 48), 2), ((18, 21), 1), ((16, 32), 1), ((64, 160), 8)):
            want = _check(torch_cuda, *_inputs(C + cols, 5, H, W, C), factor=f, cols=cols)
            if cols == 2:
                assert not want[2 * (H // f):, W // f:].any() and want[2 * (H // f):, : W // f].any()


# ---- masks and weights -----------------------------------------------------------------------------------------------------------
def test_masks(torch_cuda):
    """A checkerboard (every pixel an edge), class blobs across tile borders, a constant plane (no edge), all 256 values, and two
    samples whose facing rows differ (no edge between them)."""
    H, W = 72, 264
    img, lut = random_image(3, 1, H, W, 3), random_lut(3)
    yy, xx = np.mgrid[:H, :W]
    checker = ((yy + xx) & 1).astype(np.uint8)[None]
    constant = np.full((1, H, W), 2, np.uint8)
    every = (np.arange(H * W) % 256).astype(np.uint8).reshape(1, H, W)
    for mask in (checker, constant, every, blob_masks(9, 1, H, W, 6)):
        _check(torch_cuda, img, mask, lut)
        _check(torch_cuda, img, mask, dataset_lut(), factor=4)
    got = _check(torch_cuda, img, checker, dataset_lut())
    assert (got[checker[0] == 1] == (13, 198, 20)).all() and np.array_equal(got[checker[0] == 0], img[0][checker[0] == 0])
    facing = np.zeros((2, 8, 12), np.uint8)
    facing[1] = 1
    lut = np.zeros((256, 6), np.uint8)
    lut[:2] = ((1, 2, 3, 4, 0, 128), (5, 6, 7, 8, 0, 128))
    img = random_image(4, 2, 8, 12, 3)
    assert np.array_equal(_check(torch_cuda, img, facing, lut), img.reshape(16, 12, 3))


def test_lut_weights(torch_cuda):
    """The weights 0, 1, 64, 127, 128 and 200 (clamped to 128) inside and, in the reverse order, on the outline, on a mask of
    exactly those six rows; then a table of random weights over all 256 values."""
    img = random_image(6, 1, 48, 132, 4)
    mask = class_blobs(6, (48, 132), 6, sigma=3.0)[None]
    lut = random_lut(6)
    assert list(lut[:6, 4]) == [0, 1, 64, 127, 128, 200] and list(lut[:6, 5]) == [200, 128, 127, 64, 1, 0] and set(np.unique(mask)) == set(range(6))
    _check(torch_cuda, img, mask, lut)
    _check(torch_cuda, img, mask, lut, factor=2)
    every = np.random.default_rng(8).integers(0, 256, (1, 48, 132)).astype(np.uint8)
    _check(torch_cuda, img, every, lut)


@pytest.mark.parametrize("offsets", [(1, 0, 0), (0, 2, 0), (0, 0, 3), (3, 1, 2), (2, 3, 1)], ids=lambda o: "-".join(map(str, o)))
def test_behind_unaligned_addresses(torch_cuda, offsets):
    """(2, 32, 64): W is a multiple of 4; img, mask and out 1 to 3 bytes into a larger buffer.  Each must take the byte form -- out
    at f = 1 only, thumbnails are stored as bytes."""
    img, mask, lut = _inputs(11, 2, 32, 64, 3)
    for f, cols in ((1, 1), (2, 3), (8, 2)):
        _check(torch_cuda, img, mask, lut, f, cols, offsets)


def test_full_size(torch_cuda):
    """2 x 1024 x 1024 x 3 at f = 1, and at f = 8 with cols = 2: blobs of 8 x 8 blocks with single pixels of other values in them."""
    rng = np.random.default_rng(14)
    mask = blob_masks(14, 2, 128, 128).repeat(8, axis=1).repeat(8, axis=2)
    speck = rng.random(mask.shape) < 0.01
    mask[speck] = rng.integers(0, 8, int(speck.sum()))
    img, lut = random_image(14, 2, 1024, 1024, 3), random_lut(14)
    _check(torch_cuda, img, mask, lut)
    _check(torch_cuda, img, mask, lut, factor=8, cols=2)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_raise_and_write_nothing(torch_cuda):
    from gan_segmentation_amd import _lib, _runtime
    torch = torch_cuda
    img, mask, lut = _inputs(2, 2, 16, 16, 3)
    buf = torch.full((2 * 16 * 16 * 3 * 2 + 2048,), FILL, dtype=torch.uint8, device="cuda")
    di, dm, dl = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(lut).cuda()
    good = dict(n=2, H=16, W=16, C=3, img=di.data_ptr(), mask=dm.data_ptr(), lut=dl.data_ptr(), factor=1, cols=1, out=buf.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        _runtime.launch("gsa_overlay", buf.device, a["n"], a["H"], a["W"], a["C"], a["img"], a["mask"], a["lut"], a["factor"], a["cols"], a["out"])

    bad = [dict(n=-1), dict(img=None), dict(mask=None), dict(lut=None), dict(out=None), dict(C=0), dict(C=5), dict(factor=0), dict(factor=3),
           dict(factor=32), dict(H=6, factor=4), dict(W=6, factor=4), dict(cols=0), dict(cols=-3), dict(H=0), dict(W=65536), dict(n=1 << 21, C=4),
           dict(n=1 << 24, H=1, W=1, C=1), dict(cols=1 << 27)]
    for kw in bad:
        with pytest.raises(_lib.GsaError, match=r"gsa_overlay failed \(-1\)"):
            call(**kw)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == FILL).all(), "a refused call wrote something"
    # out over an input: each of the three in turn at byte 2000 of the buffer, out with its last byte on the input's first and with
    # its first byte on the input's last -- refused; one byte further either way there is no overlap
    sizes, at = dict(img=img.size, mask=mask.size, lut=lut.size), 2000
    base, out_bytes = buf.data_ptr(), img.size
    for name, t in (("img", di), ("mask", dm), ("lut", dl)):
        buf.fill_(FILL)
        buf[at:at + sizes[name]].copy_(t.reshape(-1))
        before = buf.cpu().numpy().copy()
        for out in (at - out_bytes + 1, at + sizes[name] - 1, at):
            with pytest.raises(_lib.GsaError, match=r"gsa_overlay failed \(-1\)"):
                call(out=base + out, **{name: base + at})
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), before), "a call refused for overlapping %s wrote something" % name
        for out in (at - out_bytes, at + sizes[name]):
            call(out=base + out, **{name: base + at})
            after = buf.cpu().numpy()
            assert np.array_equal(after[out:out + out_bytes].reshape(32, 16, 3), rule_overlay(img, mask, lut)), (name, out)
            assert np.array_equal(after[at:at + sizes[name]], before[at:at + sizes[name]])
    call(n=0, H=-5, C=9, factor=3, cols=0, out=None)     # an empty batch is a no-op before anything else


# ---- the Python layer --------------------------------------------------------------------------------------------------------
def test_overlay_is_the_sheet_of_one_column(torch_cuda):
    from gan_segmentation_amd import preview
    torch = torch_cuda
    img, mask, lut = _inputs(5, 3, 32, 48, 3)
    di, dm = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()
    over = preview.overlay(di, dm, lut)
    sheet = preview.contact_sheet(di, dm, 1, lut, factor=1)
    assert over.shape == (3, 32, 48, 3) and sheet.shape == (96, 48, 3) and torch.equal(over.reshape(96, 48, 3), sheet)
    assert torch.equal(sheet.cpu(), torch.from_numpy(rule_overlay(img, mask, lut)))
    # one sample without the batch dimension, a table on the device, the default table, the default factor of a sheet, out=
    one = preview.overlay(di[1], dm[1], torch.from_numpy(lut).cuda(), factor=2)
    assert one.shape == (16, 24, 3) and np.array_equal(one.cpu().numpy(), rule_overlay(img[1:2], mask[1:2], lut, 2))
    assert np.array_equal(preview.overlay(di, dm).cpu().numpy().reshape(96, 48, 3), rule_overlay(img, mask, preview.make_lut()))
    out = torch.full((16 * 24 * 3,), FILL, dtype=torch.uint8, device="cuda")
    got = preview.contact_sheet(di, dm, 2, lut, out=out)
    assert got.shape == (16, 24, 3) and got.data_ptr() == out.data_ptr() and np.array_equal(got.cpu().numpy(), rule_overlay(img, mask, lut, 4, 2))
    assert len([k for k in preview._device_luts if k[1] == lut.tobytes()]) == 1, "a numpy table is uploaded once per device"
    assert np.array_equal(di.cpu().numpy(), img) and np.array_equal(dm.cpu().numpy(), mask)
    for bad in (lambda: preview.overlay(di.cpu(), dm.cpu()), lambda: preview.overlay(di, dm[:, :, :-1].contiguous()), lambda: preview.overlay(di, dm, factor=3),
                lambda: preview.overlay(di, dm, factor=64), lambda: preview.contact_sheet(di, dm, 0), lambda: preview.overlay(di, dm, lut[:, :5]),
                lambda: preview.overlay(di, dm, out=di), lambda: preview.overlay(di, dm.to(torch.int32)), lambda: preview.overlay(di, dm, lut, out=out[:-1])):
        with pytest.raises(ValueError):
            bad()


def test_write_previews_on_a_generated_batch(torch_cuda, tmp_path, monkeypatch):
    """A batch of the reduced model from index 8: vis_ files for every index (k = 1), for the multiples of 3, for none (k = 0); what
    is handed to the encoder is the rule's overlay of the pair, DATASET_COLOURS at alpha 0.5 with a solid outline."""
    from PIL import Image
    from gan_segmentation_amd import preview
    from tests.test_gpu_augment import _build
    gen = _build("reduced", 4)
    img, mask = gen.generate_indexed(8, 4, seed=4)
    h_img, h_mask = img.cpu().numpy(), mask.cpu().numpy()
    assert len(np.unique(h_mask)) > 1
    saved, save = {}, preview.save_jpeg
    monkeypatch.setattr(preview, "save_jpeg", lambda path, array: (saved.__setitem__(os.path.basename(path), array.copy()), save(path, array)))
    for k, f, names in ((1, 1, [8, 9, 10, 11]), (3, 2, [9]), (0, 1, []), (5, 4, [10]), (7, 1, [])):
        d = tmp_path / ("k%d" % k)
        d.mkdir()
        saved.clear()
        paths = preview.write_previews(str(d), img, mask, 8, k, f)
        assert sorted(os.listdir(str(d))) == ["vis_%06d.jpg" % i for i in names] == [os.path.basename(p) for p in paths]
        for i in names:
            want = rule_overlay(h_img[i - 8:i - 7], h_mask[i - 8:i - 7], dataset_lut(), f)
            assert np.array_equal(saved["vis_%06d.jpg" % i], want)
            im = Image.open(str(d / ("vis_%06d.jpg" % i)))
            assert im.size == (want.shape[1], want.shape[0]) and im.mode == "RGB"
    assert np.array_equal(img.cpu().numpy(), h_img) and np.array_equal(mask.cpu().numpy(), h_mask)


def test_cli_preview_every_key(torch_cuda, tmp_path):
    """PREVIEW_EVERY: 2 on bedrooms (3 samples, batch 2): vis_000000.jpg and vis_000002.jpg at 256 / 4 px beside the six pair files,
    whose decoded images and masks are those of a run without the key."""
    from PIL import Image
    from tests.test_gpu_downscale import _cli_dirs
    runs = {}
    for name, keys in (("off", dict()), ("on", dict(PREVIEW_EVERY=2, PREVIEW_DOWNSCALE=4))):
        _gcfg, _gp, _dcfg, _dp, run = _cli_dirs(tmp_path, name)
        runs[name] = run(**keys) / "dataset" / "train_generated"
    assert len(list(runs["off"].iterdir())) == 6 and not list(runs["off"].glob("vis_*"))
    assert sorted(p.name for p in runs["on"].glob("vis_*")) == ["vis_000000.jpg", "vis_000002.jpg"] and len(list(runs["on"].iterdir())) == 8
    for p in runs["on"].glob("vis_*"):
        im = Image.open(p)
        assert im.size == (64, 64) and im.mode == "RGB"
    for i in range(3):
        for name in ("img_%06d.jpg" % i, "mask_%06d.png" % i):
            assert np.array_equal(np.asarray(Image.open(runs["on"] / name)), np.asarray(Image.open(runs["off"] / name))), name


def test_cli_annotation_writes_the_prediction_overlay_when_a_checkpoint_exists(torch_cuda, tmp_path):
    """`annotation --count 2` with a checkpoint: vis_img_%06d.jpg beside img_ and feat_, 256 px; without one: img_ and feat_ only."""
    from PIL import Image
    from tests.test_gpu_downscale import _cli_dirs
    _gcfg, _gp, _dcfg, _dp, run = _cli_dirs(tmp_path, "with")
    data = run("annotation", ["--count", "2"]) / "data"
    assert sorted(p.name for p in data.iterdir()) == sorted(n % i for i in range(2) for n in ("img_%06d.jpg", "feat_%06d.pickle", "vis_img_%06d.jpg"))
    vis, img = Image.open(data / "vis_img_000001.jpg"), Image.open(data / "img_000001.jpg")
    assert vis.size == img.size == (256, 256) and vis.mode == "RGB"
    _gcfg, _gp, _dcfg, _dp, run = _cli_dirs(tmp_path, "without")
    (tmp_path / "without" / "exp" / "checkpoints" / "checkpoint_last.params").unlink()
    data = run("annotation", ["--count", "2"]) / "data"
    assert sorted(p.name for p in data.iterdir()) == sorted(n % i for i in range(2) for n in ("img_%06d.jpg", "feat_%06d.pickle"))
