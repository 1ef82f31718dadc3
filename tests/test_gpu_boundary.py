"""The mask boundary distance and the ignore band on the GPU (include/gsa_boundary.h gsa_mask_boundary; mask_ops.boundary_distance /
ignore_band; ImageGenerator(mask_ignore_band=...); the MASK_IGNORE_BAND key): every pixel of dist2 AND of out against the rule of
tests/test_boundary_host.py -- nothing is excluded.  Except on the constant and checkerboard planes every case asserts that its
expected result holds both FAR and non-FAR pixels."""
import os
import re

import numpy as np
import pytest

from tests.test_boundary_host import FAR, class_blobs, has_both, rule_band, rule_boundary
from tests.test_gpu_augment import _build, _host, _same_bits
from tests.test_mask_morph_host import rule_morph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TILE = 64                                       # the tile of csrc/gsa_boundary.hip (asserted against the source text)
RADII = (1, 2, 5, 31, 32)                       # 1, 2: the 4-px apron; 5: the 8-px one; 31, 32: the 32-px one, partly and fully used


def _differences(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s vs %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    bad = got != want
    assert not bad.any(), "%s: %d of %d values differ from the rule, first at %s: %s instead of %s" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def _check(torch, m, R, label=255, what="", both=True, device_mask=None):
    """ignore_band with the distance on ``m``: dist2 and out against the rule, the input unchanged.  -> the expected dist2."""
    from gan_segmentation_amd import mask_ops
    d = torch.from_numpy(m).cuda() if device_mask is None else device_mask
    want = rule_boundary(m, R)
    if both:
        assert has_both(want), "%s: the expected result is all FAR or all band, the case proves nothing" % what
    out, dist2 = mask_ops.ignore_band(d, R, label, return_distance=True)
    assert out.shape == d.shape and out.dtype == torch.uint8 and out.is_contiguous() and out.data_ptr() != d.data_ptr()
    assert dist2.shape == d.shape and dist2.dtype == torch.int16 and dist2.is_contiguous()
    what = "%s %s R %d label %d" % (what, m.shape, R, label)
    _differences(dist2.cpu().numpy(), want, what + " dist2")
    _differences(out.cpu().numpy(), rule_band(m, R, label, want), what + " out")
    assert np.array_equal(d.cpu().numpy(), m), what + ": the input was written to"
    return want


def test_the_tile_is_the_one_these_tests_assume():
    src = open(os.path.join(ROOT, "gan-segmentation_amd", "csrc", "gsa_boundary.hip")).read()
    assert int(re.search(r"constexpr int kTile = (\d+);", src).group(1)) == TILE
    assert "radius <= 4" in src and "radius <= 8" in src and "radius <= 16" in src     # the apron steps that RADII straddle


# ---- shapes ------------------------------------------------------------------------------------------------------------------
def _pattern(shape, period=5):
    """Two values in blocks of ``period`` pixels: boundaries everywhere, also in planes too small or too thin for blobs."""
    H, W = shape[-2:]
    m = ((np.arange(H)[:, None] // period + np.arange(W)[None, :] // period) & 1).astype(np.uint8) * 3
    return np.broadcast_to(m, shape).copy()


@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (70, 1), (16, 16)])
def test_small_and_thin_planes(torch_cuda, shape):
    for R in (1, 2, 5, 32):
        if shape == (1, 1):
            want = _check(torch_cuda, _pattern(shape, 7), R, what="1x1", both=False)
            assert want.tolist() == [[FAR]]
        elif R < 7:
            _check(torch_cuda, _pattern(shape, 7), R, what="blocks")
        else:                                   # one boundary near the origin: the far end of a 70-px plane is beyond R = 32
            m = np.zeros(shape, np.uint8)
            m[:3, :3] = 3
            want = _check(torch_cuda, m, R, what="corner", both=max(shape) > 3 + R)
            assert max(shape) > 3 + R or (want != FAR).all(), "a 16 x 16 plane with two values is all band at R = 32"


@pytest.mark.parametrize("shape", [(63, 65), (64, 64), (65, 63), (130, 67), (131, 66)])
def test_tile_edges(torch_cuda, shape):
    """One pixel short of, exactly and one pixel beyond a tile; three tiles down a partial edge (130 x 67: byte path, 131 x 66 too);
    64 x 64 takes the dword path."""
    for R in RADII:
        if R <= 5:                              # wider bands leave no FAR pixel in blobs of this size
            _check(torch_cuda, class_blobs(sum(shape) + R, shape, 3, sigma=4.0), R, what="blobs")
        m = np.zeros(shape, np.uint8)
        m[shape[0] // 2, shape[1] // 2] = 1
        m[2, 3] = 2
        _check(torch_cuda, m, R, what="two odd pixels")


def test_a_mask_that_starts_at_an_odd_byte(torch_cuda):
    """Planes of 40 x 64 bytes behind a 1-byte offset: W is a multiple of 4 but the mask is not aligned -- the byte path."""
    from gan_segmentation_amd import mask_ops
    torch = torch_cuda
    m = class_blobs(3, (2, 40, 64), 3)
    buf = torch.zeros(1 + m.size, dtype=torch.uint8, device="cuda")
    d = buf[1:].view(2, 40, 64)
    d.copy_(torch.from_numpy(m))
    assert d.data_ptr() % 4 == 1
    for R in (2, 5):
        _check(torch, m, R, what="odd start", device_mask=d)
    obuf = torch.full((3 + m.size,), 77, dtype=torch.uint8, device="cuda")
    out = obuf[3:].view(2, 40, 64)
    assert mask_ops.ignore_band(d, 2, out=out) is out
    _differences(out.cpu().numpy(), rule_band(m, 2), "out behind 3 bytes")
    assert (obuf[:3] == 77).all()
    dbuf = torch.full((1 + m.size,), -3, dtype=torch.int16, device="cuda")      # dist2 2-byte but not 8-byte aligned
    dist2 = dbuf[1:].view(2, 40, 64)
    aligned = torch.from_numpy(m).cuda()
    assert mask_ops.boundary_distance(aligned, 5, out=dist2) is dist2 and dist2.data_ptr() % 8 == 2
    _differences(dist2.cpu().numpy(), rule_boundary(m, 5), "dist2 behind 2 bytes")
    assert dbuf[0] == -3


def test_planes_of_a_batch_do_not_leak_into_each_other(torch_cuda):
    """(3, 96, 160): constant 1, blobs, constant 2 -- a read across planes would put a band along the constant planes' edges."""
    blobs = class_blobs(8, (96, 160), 3, sigma=4.0)
    batch = np.stack([np.ones((96, 160), np.uint8), blobs, np.full((96, 160), 2, np.uint8)])
    assert (blobs[0] != 1).any() and (blobs[-1] != 2).any()     # the rows next to the constant planes do differ from them
    for R in (2, 32):
        want = rule_boundary(batch, R)
        assert (want[0] == FAR).all() and (want[2] == FAR).all() and (want[1] != FAR).any()
        _check(torch_cuda, batch, R, what="batch")


# ---- radii and classes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [2, 3, 8])
def test_radii_and_classes(torch_cuda, classes):
    """150 x 200: three tiles by four with partial edges, the dword path.  At 3 classes the last one is stored as 255.  For the wide
    bands the blobs fill a box around the plane's centre, across the seams at row 64 and column 128, in a constant plane: its rim is
    more than 32 pixels from every boundary."""
    for R in RADII:
        m = class_blobs(10 * classes + R, (150, 200), classes, sigma=8.0 if classes < 8 else 6.0, with255=classes == 3)
        if R > 5:
            box = class_blobs(10 * classes + R, (44, 70), classes, sigma=2.0, with255=classes == 3)
            m = np.full((150, 200), box[0, 0], np.uint8)
            m[53:97, 65:135] = box
        assert len(np.unique(m)) == classes and (classes != 3 or 255 in m)
        _check(torch_cuda, m, R, what="%d classes" % classes)


def test_constant_and_checkerboard(torch_cuda):
    for R in (1, 5, 32):
        want = _check(torch_cuda, np.full((2, 70, 90), 255, np.uint8), R, 7, what="constant", both=False)
        assert (want == FAR).all()
        checker = ((np.arange(70)[:, None] + np.arange(90)[None, :]) & 1).astype(np.uint8)
        want = _check(torch_cuda, checker, R, what="checkerboard", both=False)
        assert (want == 1).all()


# ---- boundaries on the seams ---------------------------------------------------------------------------------------------------
def test_edges_along_the_tile_seams(torch_cuda):
    """A vertical edge between columns 63 | 64 and a horizontal one between rows 63 | 64 of a 129 x 129 plane."""
    m = np.zeros((129, 129), np.uint8)
    m[:, 64:] = 1
    m[64:, :] += 2
    for R in RADII:
        want = _check(torch_cuda, m, R, what="cross")
        assert want[10, 63] == want[10, 64] == want[63, 10] == want[64, 10] == 1 and want[63, 63] == 1
    for R in (3, 32):
        v = np.zeros((129, 129), np.uint8)
        v[:, 64:] = 1
        want = _check(torch_cuda, v, R, what="vertical")
        assert want[5, 64 - R] == R * R and want[5, 63 + R] == R * R and want[5, 63 - R] == FAR
        _check(torch_cuda, v.T.copy(), R, what="horizontal")


def test_odd_pixels_in_the_corners_and_on_the_seam(torch_cuda):
    m = np.zeros((129, 129), np.uint8)
    for y, x in ((0, 0), (0, 128), (128, 0), (128, 128), (64, 64)):
        m[y, x] = 9
    for R in RADII:
        want = _check(torch_cuda, m, R, what="corners")
        assert want[0, 0] == want[128, 128] == want[64, 64] == 1 and want[64 - R, 64] == R * R


def test_the_far_end_of_the_apron(torch_cuda):
    """R = 32: pixels exactly 32 columns (rows) from their only boundary, on either side of it, in the first and the last column
    (row) of a tile."""
    m = np.zeros((70, 200), np.uint8)
    m[:, 96:] = 1                               # column 64 is 32 from 96; column 127 is 32 from 95
    want = _check(torch_cuda, m, 32, what="columns")
    assert want[5, 64] == 1024 and want[5, 63] == FAR and want[5, 127] == 1024 and want[5, 128] == FAR
    want = _check(torch_cuda, m.T.copy(), 32, what="rows")
    assert want[64, 5] == 1024 and want[127, 5] == 1024 and want[128, 5] == FAR
    m = np.zeros((70, 200), np.uint8)
    m[:, 0] = 1                                 # the boundary in the image's first column
    want = _check(torch_cuda, m, 32, what="first column")
    assert want[5, 32] == 1024 and want[5, 33] == FAR


# ---- full size -----------------------------------------------------------------------------------------------------------------
def test_full_size(torch_cuda):
    m = class_blobs(5, (1, 1024, 1024), 2, sigma=12.0)
    _check(torch_cuda, m, 32, what="ffhq")
    m = np.stack([class_blobs(20 + i, (512, 512), 2 + i % 3, sigma=8.0) for i in range(8)])
    _check(torch_cuda, m, 3, what="cars batch 8")


# ---- output forms --------------------------------------------------------------------------------------------------------------
def test_output_forms(torch_cuda):
    from gan_segmentation_amd import mask_ops
    torch = torch_cuda
    m = class_blobs(4, (2, 70, 92), 3, sigma=4.0)
    d = torch.from_numpy(m).cuda()
    want = rule_boundary(m, 4)
    assert has_both(want)
    dist2 = mask_ops.boundary_distance(d, 4)                            # dist2 only
    assert dist2.dtype == torch.int16 and dist2.shape == d.shape
    _differences(dist2.cpu().numpy(), want, "dist2 only")
    _differences(mask_ops.boundary_distance(d).cpu().numpy(), rule_boundary(m, 32), "the default radius")
    out = mask_ops.ignore_band(d, 4)                                    # out only
    assert out.dtype == torch.uint8 and out.data_ptr() != d.data_ptr()
    _differences(out.cpu().numpy(), rule_band(m, 4, 255, want), "out only")
    given = torch.full_like(d, 77)                                      # out=: the same tensor back, the input unchanged
    got, dist2 = mask_ops.ignore_band(d, 4, out=given, return_distance=True)
    assert got is given
    _differences(given.cpu().numpy(), rule_band(m, 4, 255, want), "out=")
    _differences(dist2.cpu().numpy(), want, "dist2 beside out=")
    assert np.array_equal(d.cpu().numpy(), m), "the input was written to"
    for label in (0, 1, 2):                                             # label 0, and labels equal to class values
        _differences(mask_ops.ignore_band(d, 4, label).cpu().numpy(), rule_band(m, 4, label, want), "label %d" % label)
    plane = mask_ops.ignore_band(d[1], 4)                               # a 2-D mask
    assert plane.shape == (70, 92)
    _differences(plane.cpu().numpy(), rule_band(m[1], 4), "plane")
    assert mask_ops.boundary_distance(d[1], 4).shape == (70, 92)
    empty, dist2 = mask_ops.ignore_band(d[:0], 4, return_distance=True)
    assert empty.shape == (0, 70, 92) and empty.dtype == torch.uint8 and dist2.shape == (0, 70, 92) and dist2.dtype == torch.int16


def test_value_errors(torch_cuda):
    from gan_segmentation_amd import mask_ops
    torch = torch_cuda
    d = torch.zeros((2, 16, 16), dtype=torch.uint8, device="cuda")
    flat = torch.zeros(3 * 16 * 16, dtype=torch.uint8, device="cuda")
    a, b = flat[:2 * 256].view(2, 16, 16), flat[256:].view(2, 16, 16)       # two overlapping views of one buffer
    for bad in (dict(mask=d.float()), dict(mask=d[:, :, ::2]), dict(mask=d.cpu()), dict(mask=d, out=d), dict(mask=a, out=b),
                dict(mask=b, out=a), dict(mask=d, out=torch.empty_like(d)[:1]), dict(mask=d, out=torch.empty_like(d).float()),
                dict(mask=d, out=torch.empty_like(d).cpu()), dict(mask=d.view(1, 2, 16, 16)), dict(mask=d, radius=0),
                dict(mask=d, radius=33), dict(mask=d, radius=2.0), dict(mask=d, radius=True), dict(mask=d, label=256),
                dict(mask=d, label=-1), dict(mask=d, label="255")):
        with pytest.raises(ValueError):
            mask_ops.ignore_band(**dict(dict(radius=2), **bad))
    wide = torch.zeros(2 * 512, dtype=torch.uint8, device="cuda")
    a, i16 = wide[256:768].view(2, 16, 16), wide.view(torch.int16).view(2, 16, 16)      # a distance map that overlaps its mask
    for bad in (dict(mask=d.float()), dict(mask=d.cpu()), dict(mask=d, max_radius=0), dict(mask=d, max_radius=33),
                dict(mask=d.view(1, 2, 16, 16)), dict(mask=d, out=torch.empty_like(d)), dict(mask=a, out=i16),
                dict(mask=d, out=torch.empty((2, 16, 16), dtype=torch.int16)), dict(mask=d, out=torch.empty((1, 16, 16), dtype=torch.int16, device="cuda"))):
        with pytest.raises(ValueError):
            mask_ops.boundary_distance(**bad)


# ---- the generator -----------------------------------------------------------------------------------------------------------
# The reduced synthetic generator of the augment tests (128 px pairs).  These tests prove the plumbing -- that the rule runs, on the
# right tensor, at the right place and last; the kernel's correctness rests on the direct cases above.  Every test asserts that the
# band changes the mask it is applied to.
BAND = 2
MIN_AREA = 64


def _pair(t):
    return t[0].cpu().numpy(), t[1].cpu().numpy()


def _check_plumbing(raw, banded, what, before=None, radius=BAND, label=255):
    """``banded`` = (the plain generator's image, the band on ``before(plain mask)``)."""
    (img0, mask0), (img1, mask1) = raw, banded
    assert np.array_equal(img1, img0), "%s: the band changed the image" % what
    base = mask0 if before is None else before(mask0)
    want = rule_band(base, radius, label)
    assert not np.array_equal(want, base), "%s: the rule leaves the mask as it is, the case proves nothing" % what
    assert (want != label).any(), "%s: the band covers everything" % what
    assert np.array_equal(mask1, want), "%s: %d mask bytes differ from the rule" % (what, int((mask1 != want).sum()))


def _despeckled(mask):
    from tests.test_components_host import rule_despeckle
    return rule_despeckle(mask, MIN_AREA)


@pytest.mark.parametrize("kw,before", [(dict(), None), (dict(output_downscale=2), None), (dict(style_mix_prob=1.0), None),
                                       (dict(mask_morph=True), rule_morph), (dict(mask_min_area=MIN_AREA), _despeckled),
                                       (dict(mask_morph=True, mask_min_area=MIN_AREA), lambda m: _despeckled(rule_morph(m)))],
                         ids=["plain", "downscale2", "mixed", "after-morph", "after-min-area", "all-three"])
def test_generate_indexed_returns_the_band_on_the_finished_mask(torch_cuda, kw, before):
    """The band runs LAST: with mask_morph and mask_min_area the mask is the band on rule_despeckle(rule_morph(raw))."""
    base = {k: v for k, v in kw.items() if not k.startswith("mask_")}
    plain, banded = _build("reduced", 3, **base), _build("reduced", 3, mask_ignore_band=BAND, **kw)
    for first, n in ((10, 3), (13, 2)):
        raw = _pair(plain.generate_indexed(first, n, seed=4))
        assert raw[1].shape[-1] == 128 // kw.get("output_downscale", 1)
        _check_plumbing(raw, _pair(banded.generate_indexed(first, n, seed=4)), "samples %d..%d" % (first, first + n - 1), before)


def test_the_label_keyword_and_a_wide_band(torch_cuda):
    plain, banded = _build("reduced", 3), _build("reduced", 3, mask_ignore_band=9, mask_ignore_label=6)
    _check_plumbing(_pair(plain.generate_indexed(10, 3, seed=4)), _pair(banded.generate_indexed(10, 3, seed=4)), "label 6", radius=9,
                    label=6)


def test_band_zero_is_off_and_allocates_nothing(torch_cuda):
    plain = _build("reduced", 3)
    raw = _pair(plain.generate_indexed(10, 3, seed=4))
    gen = _build("reduced", 3, mask_ignore_band=0, mask_ignore_label=7)
    got = _pair(gen.generate_indexed(10, 3, seed=4))
    assert np.array_equal(got[0], raw[0]) and np.array_equal(got[1], raw[1])
    assert "_raw_masks" not in gen.__dict__, "no scratch without the band"


def test_out_batch_and_batch_w_get_it_too(torch_cuda):
    torch = torch_cuda
    plain, banded = _build("reduced", 3), _build("reduced", 3, mask_ignore_band=BAND)
    img = torch.empty((3, 128, 128, 3), dtype=torch.uint8, device="cuda")
    mask = torch.full((3, 128, 128), 9, dtype=torch.uint8, device="cuda")
    got = banded.generate_indexed(20, 3, seed=4, out=(img, mask))
    assert got[0] is img and got[1] is mask
    _check_plumbing(_pair(plain.generate_indexed(20, 3, seed=4)), _pair((img, mask)), "out=")
    z, noise = plain.netG.draw_indexed(30, 3, 4)
    _check_plumbing(_pair(plain.generate_batch(z, noise)), _pair(banded.generate_batch(z, noise)), "generate_batch")
    dl = plain.netG.mapping(z)[:, None, :].repeat(1, plain.netG.num_style_layers, 1).contiguous()
    _check_plumbing(_pair(plain.generate_batch_w(dl, noise)), _pair(banded.generate_batch_w(dl, noise)), "generate_batch_w")
    shapes = sorted((k[0], tuple(t.shape), str(t.dtype)) for k, t in banded.__dict__["_raw_masks"].items())
    assert shapes == [("raw", (3, 128, 128), "torch.uint8")], "the band alone needs the raw mask and nothing else"
    full = _build("reduced", 3, mask_ignore_band=BAND, mask_morph=True, mask_min_area=MIN_AREA)
    full.generate_indexed(20, 3, seed=4)
    assert sorted(k[0] for k in full.__dict__["_raw_masks"]) == ["areas", "filtered", "labels", "morphed", "raw"]


def test_replayed_graph_keeps_working(torch_cuda):
    """graph_mode "1", captured at the second call: four identical calls into preallocated outputs, every one the band on the raw
    mask -- the eager band behind a replayed graph reads what the graph wrote."""
    torch = torch_cuda
    plain, banded = _build("reduced", 3), _build("reduced", 3, mask_ignore_band=BAND)
    banded.graph_mode, banded.graph_after = "1", 2
    z, noise = plain.netG.draw_indexed(40, 3, 4)
    raw = _pair(plain.generate_batch(z, noise))
    img = torch.empty((3, 128, 128, 3), dtype=torch.uint8, device="cuda")
    mask = torch.empty((3, 128, 128), dtype=torch.uint8, device="cuda")
    for call in range(4):
        img.fill_(3)
        mask.fill_(9)
        banded.generate_batch(z, noise, out=(img, mask))
        _check_plumbing(raw, _pair((img, mask)), "call %d" % call)
    assert banded.graphs_captured() >= 1


def test_training_batches_warp_the_banded_mask(torch_cuda):
    """The labels are the warp of the banded mask, bit for bit; labels="int64" shows -1 in the band (and at the warp's border)."""
    from gan_segmentation_amd import augment
    torch = torch_cuda
    plain, banded = _build("reduced", 3), _build("reduced", 3, mask_ignore_band=BAND)
    kw = dict(crop=96, seed=4, first_index=10, num_samples=5)
    a = [(_host(image, label), first) for image, label, first in plain.training_batches(3, **kw)]
    b = [(_host(image, label), first) for image, label, first in banded.training_batches(3, **kw)]
    c = [(_host(image, label), first) for image, label, first in banded.training_batches(3, labels="int64", **kw)]
    assert [f for _, f in a] == [f for _, f in b] == [f for _, f in c] == [10, 13]
    changed = 0
    for ((image0, label0), first), ((image1, label1), _f), ((_image2, label2), _g) in zip(a, b, c):
        n = min(3, 15 - first)
        _same_bits(image1, image0, "image of batch %d" % first)
        img, mask = plain.generate_indexed(first, n, seed=4)
        want = rule_band(mask.cpu().numpy(), BAND)
        changed += int((want != mask.cpu().numpy()).sum())
        matrices = augment.plan_matrices(4, first, n, 128, 128, 96, "train")
        _image, label = augment.augment_pairs(img, torch.from_numpy(want).cuda(), matrices, augment.output_size(128, 128, 96))
        label = label.cpu().numpy()
        _same_bits(label1, label, "label of batch %d" % first)
        assert label2.dtype == np.int64 and np.array_equal(label2, np.where(label == 255, -1, label.astype(np.int64)))
        assert int((label2 == -1).sum()) > int((label0 == 255).sum()), "the band adds ignored pixels to the border's"
        assert label2.max() < 255
    assert changed > 0, "the rule changed no raw mask"


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("png_on_gpu", [True, False], ids=["device-png", "host-png"])
def test_cli_mask_ignore_band_key(torch_cuda, tmp_path, png_on_gpu):
    """MASK_IGNORE_BAND: 2 with PAIR_STATS on bedrooms (3 samples): every mask_*.png decodes to the band on the mask of a run
    without the key -- 255 unchanged through the device and the host PNG encoder --, every img_*.jpg holds the same bytes, and the
    pair statistics count the band in slot 8."""
    from PIL import Image
    from gan_segmentation_amd import pair_stats
    from tests.test_gpu_downscale import _cli_dirs
    runs = {}
    for name, keys in (("off", dict()), ("on", dict(MASK_IGNORE_BAND=2, PAIR_STATS=True))):
        _gcfg, _gp, _dcfg, _dp, run = _cli_dirs(tmp_path, name)
        runs[name] = run(PNG_ON_GPU=png_on_gpu, **keys) / "dataset" / "train_generated"
    assert len(list(runs["off"].iterdir())) == 6 and len(list(runs["on"].iterdir())) == 7
    band = []
    for i in range(3):
        assert (runs["on"] / ("img_%06d.jpg" % i)).read_bytes() == (runs["off"] / ("img_%06d.jpg" % i)).read_bytes()
        raw = np.asarray(Image.open(runs["off"] / ("mask_%06d.png" % i)))
        got = np.asarray(Image.open(runs["on"] / ("mask_%06d.png" % i)))
        assert raw.shape == (256, 256) and 255 not in raw and np.array_equal(got, rule_band(raw, 2)), "mask %d" % i
        band.append(int((got == 255).sum()))
    assert min(band) > 0 and max(band) < 256 * 256, "the band is empty or everything: the run proves nothing"
    index, rows, H, W, C = pair_stats.merge_shards(str(runs["on"]))
    assert (H, W, C) == (256, 256, 3) and np.array_equal(index, np.arange(3))
    assert [int(v) for v in rows[:, 8]] == band, "slot 8 holds the band's pixels"
