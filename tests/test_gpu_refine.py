"""The image-guided mask refinement on the GPU (csrc/gsa_refine.h gsa_mask_refine; mask_ops.refine; ImageGenerator(mask_refine=)):
bit for bit the rule of tests/test_refine_host.py, every byte of every mask, nothing excluded.  Every output is pre-filled with 0xAA,
so a byte the call does not write shows, and every input must come back unchanged.  Every case is held (``expected``) to change its
mask somewhere and, with the coarse weights, to hold a pixel that only the tie rule keeps."""
import os

import numpy as np
import pytest

from tests.test_boundary_host import rule_band
from tests.test_mask_morph_host import rule_morph
from tests.test_refine_host import (THIN, TILE_EDGES, TABLE_BYTES, case, coarse_tables, every_value, expected, region_image, rule_refine,
                                    salted_blobs)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xAA


def _behind(torch, array, offset):
    """``array`` on the device, ``offset`` bytes into a larger buffer (a fresh allocation is aligned far beyond 4 bytes)."""
    buf = torch.full((array.size + 8,), FILL, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + array.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(array).reshape(-1)))
    assert view.data_ptr() % 4 == offset % 4
    return buf, view


def _call(torch, img, mask, tables, classes, radius, offsets=(0, 0, 0, 0)):
    """The C entry on raw addresses -> the refined masks as a host array; asserts the inputs and the bytes around the output unchanged."""
    from gan_segmentation_amd import _runtime
    n, H, W, C = img.shape
    _bi, di = _behind(torch, img, offsets[0])
    _bm, dm = _behind(torch, mask, offsets[1])
    _bt, dt = _behind(torch, tables, offsets[2])
    bo = torch.full((mask.size + 8,), FILL, dtype=torch.uint8, device="cuda")
    do = bo[offsets[3]:offsets[3] + mask.size]
    _runtime.launch("gsa_mask_refine", do.device, n, H, W, C, classes, radius, di.data_ptr(), dm.data_ptr(), dt.data_ptr(), do.data_ptr())
    host = bo.cpu().numpy()
    assert (host[:offsets[3]] == FILL).all() and (host[offsets[3] + mask.size:] == FILL).all(), "bytes around the output were written"
    assert np.array_equal(di.cpu().numpy(), img.reshape(-1)) and np.array_equal(dm.cpu().numpy(), mask.reshape(-1)), "an input was written to"
    assert np.array_equal(dt.cpu().numpy(), tables)
    return host[offsets[3]:offsets[3] + mask.size].reshape(mask.shape)


def _check(torch, img, mask, tables, classes, radius, offsets=(0, 0, 0, 0), want_change=True, want_tie=True):
    want = expected(img, mask, tables, classes, radius, want_change, want_tie)
    got = _call(torch, img, mask, tables, classes, radius, offsets)
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(want)), "refine %s K %d R %d offsets %s: %d of %d bytes differ, first at %s" % (
        img.shape, classes, radius, offsets, int((got != want).sum()), want.size, tuple(np.argwhere(got != want)[0]))
    return want


# ---- shapes ------------------------------------------------------------------------------------------------------------------
def test_the_tile_constants_are_what_the_shapes_assume():
    src = open(os.path.join(ROOT, "gan-segmentation_amd", "csrc", "gsa_refine.hip")).read()
    assert "kTileW = 64;" in src and "kTileH = 32;" in src and "kPad = 8;" in src and "kThreads = 256;" in src


@pytest.mark.parametrize("shape", THIN)
def test_thin_planes(torch_cuda, shape):
    H, W = shape
    _check(torch_cuda, *case(H + W, 2, H, W), coarse_tables(), 3, 3, want_change=H * W > 1, want_tie=H * W > 1)


@pytest.mark.parametrize("shape", TILE_EDGES)
def test_tile_edges(torch_cuda, shape):
    """One pixel short of the 64 x 32 tile, exactly it and one beyond, each way, and three tiles across with W % 4 != 0."""
    H, W = shape
    _check(torch_cuda, *case(H + W, 2, H, W), coarse_tables(), 3, 3)


# ---- parameters --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2, 3, 4, 5])
def test_every_radius(torch_cuda, radius):
    """A tile-edge shape in the byte form and one of several tiles in the dword form, with the coarse and the default weights."""
    from gan_segmentation_amd import mask_ops
    for H, W in ((33, 65), (40, 72)):
        img, mask = case(radius + W, 1, H, W)
        _check(torch_cuda, img, mask, coarse_tables(), 3, radius)
        _check(torch_cuda, img, mask, mask_ops.refine_tables(radius), 3, radius, want_tie=False)


@pytest.mark.parametrize("classes", [2, 3, 8])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_classes_and_channels(torch_cuda, classes, C):
    for (H, W), R in (((33, 66), 2), ((20, 68), 4)):
        _check(torch_cuda, *case(classes + C, 2, H, W, C, classes), coarse_tables(), classes, R)


def test_batches_and_facing_rows(torch_cuda):
    for n in (1, 2, 5):
        _check(torch_cuda, *case(n, n, 18, 21, 3, 2), coarse_tables(), 2, 2)
    mask = np.zeros((2, 8, 12), np.uint8)
    mask[1] = 1                                                         # all 0 above all 1: the facing rows are not neighbours
    img = np.full((2, 8, 12, 3), 70, np.uint8)
    assert np.array_equal(_check(torch_cuda, img, mask, coarse_tables(), 2, 5, want_change=False, want_tie=False), mask)


def test_masks(torch_cuda):
    """All 256 values (most of them frozen), a constant plane, and all-zero tables."""
    H, W = 72, 136
    img = region_image(3, 1, H, W, 3)
    for K in (2, 5, 8):
        every = every_value(K, H, W, K)
        want = _check(torch_cuda, img, every, coarse_tables(), K, 3)
        assert np.array_equal(want[every >= K], every[every >= K])
    constant = np.full((1, H, W), 1, np.uint8)
    assert np.array_equal(_check(torch_cuda, img, constant, coarse_tables(), 3, 3, want_change=False, want_tie=False), constant)
    mask = case(5, 1, H, W)[1]
    assert np.array_equal(_check(torch_cuda, img, mask, np.zeros(TABLE_BYTES, np.uint8), 3, 5, want_change=False, want_tie=False), mask)


@pytest.mark.parametrize("offsets", [(1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1), (3, 1, 2, 2), (2, 3, 1, 3)], ids=lambda o: "-".join(map(str, o)))
def test_behind_unaligned_addresses(torch_cuda, offsets):
    """(2, 32, 64): W is a multiple of 4; img, mask, tables and out 1 to 3 bytes into a larger buffer.  img, mask and out each force the
    byte form; the tables are read byte by byte in either form."""
    img, mask = case(11, 2, 32, 64)
    _check(torch_cuda, img, mask, coarse_tables(), 3, 3, offsets)
    _check(torch_cuda, region_image(12, 2, 32, 64, 4), mask, coarse_tables(), 3, 1, offsets)


@pytest.mark.parametrize("n,H,W,radius,classes", [(1, 1024, 1024, 2, 8), (2, 256, 320, 5, 2)])
def test_larger_cases(torch_cuda, n, H, W, radius, classes):
    """Thousands of tiles, and two planes at the widest window: blobs scaled up by 4, with salt."""
    from gan_segmentation_amd import mask_ops
    rng = np.random.default_rng(H)
    img = region_image(H, n, H // 4, W // 4, 3, sd=0.0).repeat(4, axis=1).repeat(4, axis=2)
    img = np.clip(img.astype(np.int16) + np.rint(6.0 * rng.standard_normal(img.shape)).astype(np.int16), 0, 255).astype(np.uint8)
    mask = salted_blobs(H, n, H // 4, W // 4, classes, salt=0.0).repeat(4, axis=1).repeat(4, axis=2)
    hit = rng.random(mask.shape) < 0.08
    mask[hit] = rng.integers(0, classes, int(hit.sum()))
    mask[rng.random(mask.shape) < 0.01] = 255
    _check(torch_cuda, img, mask, mask_ops.refine_tables(radius), classes, radius, want_tie=False)


# ---- the Python layer --------------------------------------------------------------------------------------------------------
def test_refine_passes_land_in_out(torch_cuda):
    """iterations 1 and 3 (and 2): the result is in ``out``, the inputs are unchanged, three passes are three applications of the rule;
    the default tables are those of the parameters, uploaded once."""
    from gan_segmentation_amd import mask_ops
    torch = torch_cuda
    img, mask = case(7, 2, 40, 72, 3, 4)
    di, dm = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()
    tables = mask_ops.refine_tables(2, 1.5, 40.0)
    for k in (1, 2, 3):
        out = torch.full_like(dm, FILL)
        got = mask_ops.refine(di, dm, iterations=k, radius=2, classes=4, sigma_space=1.5, sigma_colour=40.0, out=out)
        assert got is out
        want = rule_refine(img, mask, tables, 4, 2, iterations=k)
        assert np.array_equal(out.cpu().numpy(), want)
        assert (want != rule_refine(img, mask, tables, 4, 2, iterations=k - 1)).any(), "pass %d changes nothing" % k
    assert np.array_equal(di.cpu().numpy(), img) and np.array_equal(dm.cpu().numpy(), mask)
    assert len([key for key in mask_ops._device_tables if key[1:] == (2, 1.5, 40.0)]) == 1, "one upload per device and parameters"
    # explicit tables (numpy and device), the caller's scratch, one sample without the batch dimension, the defaults
    scratch = torch.full_like(dm, FILL)
    got = mask_ops.refine(di, dm, 3, 3, 4, tables=coarse_tables(), scratch=scratch)
    assert np.array_equal(got.cpu().numpy(), rule_refine(img, mask, coarse_tables(), 4, 3, iterations=3))
    assert np.array_equal(scratch.cpu().numpy(), rule_refine(img, mask, coarse_tables(), 4, 3, iterations=2)), "the pass before the last is in scratch"
    one = mask_ops.refine(di[1], dm[1], tables=torch.from_numpy(coarse_tables()).cuda(), classes=4)
    assert one.shape == (40, 72) and np.array_equal(one.cpu().numpy(), rule_refine(img[1:], mask[1:], coarse_tables(), 4, 3)[0])
    assert np.array_equal(mask_ops.refine(di, dm).cpu().numpy(), rule_refine(img, mask, mask_ops.refine_tables(), 8, 3))
    empty = mask_ops.refine(di[:0], dm[:0], 2)
    assert empty.shape == (0, 40, 72)
    for bad in (lambda: mask_ops.refine(di.cpu(), dm.cpu()), lambda: mask_ops.refine(di[:, :, :-1].contiguous(), dm), lambda: mask_ops.refine(dm, dm),
                lambda: mask_ops.refine(di, dm, 0), lambda: mask_ops.refine(di, dm, 9), lambda: mask_ops.refine(di, dm, radius=6),
                lambda: mask_ops.refine(di, dm, classes=1), lambda: mask_ops.refine(di, dm, out=dm), lambda: mask_ops.refine(di, dm, 2, out=out, scratch=out),
                lambda: mask_ops.refine(di, dm, 2, scratch=dm), lambda: mask_ops.refine(di, dm, tables=coarse_tables()[:-1]),
                lambda: mask_ops.refine(di, dm, sigma_space=0.0), lambda: mask_ops.refine(di.to(torch.int32), dm)):
        with pytest.raises(ValueError):
            bad()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_raise_and_write_nothing(torch_cuda):
    from gan_segmentation_amd import _lib, _runtime
    torch = torch_cuda
    img, mask = case(2, 2, 16, 16)
    tables = coarse_tables()
    buf = torch.full((8192,), FILL, dtype=torch.uint8, device="cuda")
    di, dm, dt = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(tables).cuda()
    good = dict(n=2, H=16, W=16, C=3, K=3, R=3, img=di.data_ptr(), mask=dm.data_ptr(), tables=dt.data_ptr(), out=buf.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        _runtime.launch("gsa_mask_refine", buf.device, a["n"], a["H"], a["W"], a["C"], a["K"], a["R"], a["img"], a["mask"], a["tables"], a["out"])

    bad = [dict(n=-1), dict(img=None), dict(mask=None), dict(tables=None), dict(out=None), dict(C=0), dict(C=5), dict(K=1), dict(K=9), dict(K=0),
           dict(R=0), dict(R=6), dict(R=-1), dict(H=0), dict(W=0), dict(W=65536), dict(H=65536), dict(H=65535, W=32769, C=1),
           dict(n=1 << 24, H=1, W=1, C=1)]
    for kw in bad:
        with pytest.raises(_lib.GsaError, match=r"gsa_mask_refine failed \(-1\)"):
            call(**kw)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == FILL).all(), "a refused call wrote something"
    # out over an input: each of the three in turn at byte 2000 of the buffer, out with its last byte on the input's first and with
    # its first byte on the input's last -- refused; one byte further either way there is no overlap
    sizes, at = dict(img=img.size, mask=mask.size, tables=tables.size), 2000
    base, out_bytes = buf.data_ptr(), mask.size
    want = rule_refine(img, mask, tables, 3, 3)
    for name, t in (("img", di), ("mask", dm), ("tables", dt)):
        buf.fill_(FILL)
        buf[at:at + sizes[name]].copy_(t.reshape(-1))
        before = buf.cpu().numpy().copy()
        for out in (at - out_bytes + 1, at + sizes[name] - 1, at):
            with pytest.raises(_lib.GsaError, match=r"gsa_mask_refine failed \(-1\)"):
                call(out=base + out, **{name: base + at})
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), before), "a call refused for overlapping %s wrote something" % name
        for out in (at - out_bytes, at + sizes[name]):
            call(out=base + out, **{name: base + at})
            after = buf.cpu().numpy()
            assert np.array_equal(after[out:out + out_bytes].reshape(mask.shape), want), (name, out)
            assert np.array_equal(after[at:at + sizes[name]], before[at:at + sizes[name]])
    call(n=0, H=-5, C=9, K=1, R=9, out=None)      # an empty batch is a no-op before anything else


# ---- the generator -----------------------------------------------------------------------------------------------------------
def _pair(t):
    return t[0].cpu().numpy(), t[1].cpu().numpy()


def test_generate_indexed_returns_the_refined_mask(torch_cuda):
    """mask_refine=2: the rule applied twice to the raw mask with the returned image, the same bytes for batches 1 + 3 and 4; with
    mask_morph and mask_ignore_band on as well the order is refine, morph, band; with the option off the parent's bytes and no scratch."""
    from gan_segmentation_amd import mask_ops
    from tests.test_gpu_augment import _build
    plain, refined = _build("reduced", 4), _build("reduced", 4, mask_refine=2)
    K = int(plain._decoder.cfg["features"][-1])
    assert 2 <= K <= 8
    tables = mask_ops.refine_tables()
    img, raw = _pair(plain.generate_indexed(10, 4, seed=4))
    want = rule_refine(img, raw, tables, K, 3, iterations=2)
    assert (want != raw).any(), "the rule changed no raw mask"
    got = _pair(refined.generate_indexed(10, 4, seed=4))
    assert np.array_equal(got[0], img) and np.array_equal(got[1], want)
    parts = [_pair(refined.generate_indexed(10, 1, seed=4)), _pair(refined.generate_indexed(11, 3, seed=4))]
    assert np.array_equal(np.concatenate([p[1] for p in parts]), want) and np.array_equal(np.concatenate([p[0] for p in parts]), img)
    assert sorted({k[0] for k in refined.__dict__["_raw_masks"]}) == ["raw", "refining"]
    full = _build("reduced", 4, mask_refine=1, mask_refine_radius=2, mask_refine_sigma_space=1.0, mask_refine_sigma_colour=24.0, mask_morph=True,
                  mask_ignore_band=2)
    got = _pair(full.generate_indexed(10, 4, seed=4))
    step = rule_refine(img, raw, mask_ops.refine_tables(2, 1.0, 24.0), K, 2)
    assert np.array_equal(got[0], img) and np.array_equal(got[1], rule_band(rule_morph(step), 2))
    assert not np.array_equal(got[1], rule_band(rule_morph(raw), 2)), "the refinement made no difference to the finished mask"
    off = _build("reduced", 4, mask_refine=0, mask_refine_radius=5)
    got = _pair(off.generate_indexed(10, 4, seed=4))
    assert np.array_equal(got[0], img) and np.array_equal(got[1], raw) and "_raw_masks" not in off.__dict__
