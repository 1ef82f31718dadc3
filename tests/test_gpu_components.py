"""The mask components on the GPU (include/gsa_components.h gsa_mask_components; mask_ops.components / despeckle;
ImageGenerator(mask_min_area=...); the MASK_MIN_AREA key): every pixel of labels, areas and out and every word of the rows against
the rule of tests/test_components_host.py -- nothing is excluded.  The oracle is the scipy form where scipy is importable and the
raster union-find otherwise; the host tests pin the two equal."""
import os
import re

import numpy as np
import pytest

from tests.test_components_host import (ALL_INPUTS, LARGEST, NCOMP, ROW, SLOTS, SMALL, make_input, oracle_components, rule_despeckle,
                                        rule_rows)
from tests.test_gpu_augment import _build, _host, _same_bits
from tests.test_mask_morph_host import blobs, make, rule_morph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The tile of csrc/gsa_components.hip: the shapes below are derived from it (asserted against the source text).
TILE_W = TILE_H = 64

SMALL_SHAPES = [(1, 1, 1), (1, 1, 7), (1, 9, 3), (1, 17, 23), (1, 40, 57)]      # smaller than a tile, odd widths
TWO_TILES_AND_A_PART = (1, 2 * TILE_H + 8, 2 * TILE_W + 8)
REMAINDERS = (1, 2 * TILE_H + 2, TILE_W + 6)    # a 2-row and a 6-column remainder, W % 4 != 0
WHOLE_TILES = (2, TILE_H, 2 * TILE_W)
ONE_WIDE = (1, 3 * TILE_H + 8, TILE_W)
ONE_HIGH = (1, TILE_H, 3 * TILE_W + 8)
SEAM_SHAPES = [TWO_TILES_AND_A_PART, REMAINDERS, WHOLE_TILES, ONE_WIDE, ONE_HIGH]

MIN_AREAS = (0, 2, 16, 64)
FILLS = (-1, 0, 255)


def _fill_arg(fill):
    return "neighbour" if fill == -1 else fill


def _run(torch, m, min_area, connectivity, fill, **kw):
    """despeckle with rows and scratch -> (labels, areas, out, rows) on the host; the input must stay as it was."""
    from gan_segmentation_amd import mask_ops
    d = torch.from_numpy(m).cuda()
    scratch = (torch.full(m.shape, -7, dtype=torch.int32, device="cuda"), torch.full(m.shape, 1 << 30, dtype=torch.int32, device="cuda"))
    out, rows = mask_ops.despeckle(d, min_area, connectivity, _fill_arg(fill), return_stats=True, scratch=scratch, **kw)
    assert out.shape == d.shape and out.dtype == torch.uint8 and out.is_contiguous() and out.data_ptr() != d.data_ptr()
    assert rows.dtype == torch.int64 and tuple(rows.shape) == ((m.shape[0], ROW) if m.ndim == 3 else (ROW,))
    assert np.array_equal(d.cpu().numpy(), m), "the input was written to"
    return scratch[0].cpu().numpy(), scratch[1].cpu().numpy(), out.cpu().numpy(), rows.cpu().numpy()


def _differences(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s vs %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    bad = got != want
    assert not bad.any(), "%s: %d of %d values differ from the rule, first at %s: %s instead of %s" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def _check_input(torch, name, m):
    """One input under both connectivities, every min_area and every fill: labels, areas, out and rows, all of them."""
    for connectivity in (4, 8):
        comps = oracle_components(m, connectivity)
        for min_area in MIN_AREAS:
            want_rows = rule_rows(m, min_area, connectivity, components=comps)
            for fill in FILLS:
                what = "%s %s connectivity %d min_area %d fill %d" % (name, m.shape, connectivity, min_area, fill)
                labels, areas, out, rows = _run(torch, m, min_area, connectivity, fill)
                _differences(labels, comps[0], what + " labels")
                _differences(areas, comps[1], what + " areas")
                _differences(out, rule_despeckle(m, min_area, connectivity, fill, components=comps), what + " out")
                _differences(rows, want_rows, what + " rows")
                if min_area <= 1:
                    assert np.array_equal(out, m) and not rows[..., SMALL:].any(), what + ": min_area <= 1 changes nothing"


def _check_all_inputs(torch, shape):
    for name in ALL_INPUTS:
        _check_input(torch, name, make_input(name, sum(shape), shape))


def test_the_tile_is_the_one_these_tests_assume():
    src = open(os.path.join(ROOT, "gan-segmentation_amd", "csrc", "gsa_components.hip")).read()
    assert int(re.search(r"constexpr int kTileW = (\d+);", src).group(1)) == TILE_W
    assert int(re.search(r"constexpr int kTileH = (\d+);", src).group(1)) == TILE_H
    for _n, H, W in SMALL_SHAPES:
        assert H < TILE_H and W < TILE_W and W % 2 == 1
    _n, H, W = TWO_TILES_AND_A_PART
    assert H // TILE_H == 2 and H % TILE_H and W // TILE_W == 2 and W % TILE_W
    _n, H, W = REMAINDERS
    assert H % TILE_H == 2 and W % TILE_W == 6 and W % 4
    n, H, W = WHOLE_TILES
    assert n == 2 and H % TILE_H == 0 and W % TILE_W == 0 and H * W > TILE_H * TILE_W
    assert ONE_WIDE[2] == TILE_W and ONE_WIDE[1] > 2 * TILE_H and ONE_HIGH[1] == TILE_H and ONE_HIGH[2] > 2 * TILE_W
    assert any(W % 4 for _n, _H, W in SEAM_SHAPES) and any(W % 4 == 0 for _n, _H, W in SEAM_SHAPES)      # both load paths


@pytest.mark.parametrize("shape", SMALL_SHAPES)
def test_shapes_smaller_than_a_tile(torch_cuda, shape):
    _check_all_inputs(torch_cuda, shape)


@pytest.mark.parametrize("shape", SEAM_SHAPES)
def test_tile_seams(torch_cuda, shape):
    """Two full tiles and a partial one each way; a 2-row and 6-column remainder with W % 4 != 0; whole tiles only with n = 2; one
    tile wide and several high, and the transpose.  The serpentine, spiral, comb and checker cross every seam."""
    _check_all_inputs(torch_cuda, shape)


def test_a_copy_kernel_cannot_pass(torch_cuda):
    """The guards of the issue, asserted for the case: blobs(5, (128, 128)) has 286 components at connectivity 8 and min_area 16
    changes 394 of its pixels."""
    m = blobs(5, (128, 128))
    comps = oracle_components(m, 8)
    want = rule_despeckle(m, 16, 8, -1, components=comps)
    assert len(np.unique(comps[0])) == 286 and int((want != m).sum()) == 394
    labels, areas, out, rows = _run(torch_cuda, m, 16, 8, -1)
    assert len(np.unique(labels)) == 286 and int((out != m).sum()) == 394
    _differences(labels, comps[0], "labels")
    _differences(areas, comps[1], "areas")
    _differences(out, want, "out")
    _differences(rows, rule_rows(m, 16, 8, components=comps), "rows")
    assert rows[NCOMP:NCOMP + SLOTS].sum() == 286 and rows[SMALL] > 0 and rows[LARGEST] > 1000
    comps4 = oracle_components(m, 4)
    assert len(np.unique(comps4[0])) > 286
    _differences(_run(torch_cuda, m, 16, 4, -1)[0], comps4[0], "labels under 4")


def test_components_returns_labels_and_areas(torch_cuda):
    from gan_segmentation_amd import mask_ops
    torch = torch_cuda
    m = make("classes", 9, (2, 70, 90))
    d = torch.from_numpy(m).cuda()
    for connectivity in (4, 8):
        labels, areas = mask_ops.components(d, connectivity)
        assert labels.dtype == areas.dtype == torch.int32 and labels.shape == areas.shape == d.shape
        want = oracle_components(m, connectivity)
        _differences(labels.cpu().numpy(), want[0], "labels")
        _differences(areas.cpu().numpy(), want[1], "areas")
    labels, areas = mask_ops.components(d[1])
    assert labels.shape == (70, 90)
    _differences(labels.cpu().numpy(), oracle_components(m[1])[0], "labels of a plane")
    assert mask_ops.components(d[:0])[0].shape == (0, 70, 90)


def test_images_of_a_batch_do_not_leak_into_each_other(torch_cuda):
    """n = 3 planes smaller than a tile: each equal to itself alone; a constant plane between two busy ones stays one component."""
    batch = np.stack([blobs(5, (32, 40)), np.ones((32, 40), np.uint8), make("classes", 4, (32, 40))])
    comps = oracle_components(batch, 8)
    labels, areas, out, rows = _run(torch_cuda, batch, 16, 8, -1)
    _differences(labels, comps[0], "labels")
    _differences(areas, comps[1], "areas")
    _differences(out, rule_despeckle(batch, 16, 8, -1, components=comps), "out")
    _differences(rows, rule_rows(batch, 16, 8, components=comps), "rows")
    for k in range(3):
        alone = _run(torch_cuda, batch[k:k + 1], 16, 8, -1)
        for got, one, name in zip((labels, areas, out, rows), alone, ("labels", "areas", "out", "rows")):
            assert np.array_equal(got[k], one[0]), "%s of image %d differ from image %d alone" % (name, k, k)
    assert (labels[1] == 0).all() and (areas[1] == 32 * 40).all() and (out[1] == 1).all()
    assert rows[1].tolist() == [0, 1] + [0] * 8 + [32 * 40] + [0] * 9
    assert not np.array_equal(out[0], batch[0]) and not np.array_equal(out[2], batch[2])


def test_a_view_that_is_not_dword_aligned(torch_cuda):
    """Planes of 15 x 20 bytes behind a 1-byte offset: W is a multiple of 4 but the mask is not aligned; so for out."""
    from gan_segmentation_amd import mask_ops
    torch = torch_cuda
    m = make("blobs", 7, (3, 15, 20))
    buf = torch.zeros(1 + m.size, dtype=torch.uint8, device="cuda")
    d = buf[1:].view(3, 15, 20)
    d.copy_(torch.from_numpy(m))
    assert d.data_ptr() % 4 == 1
    want = rule_despeckle(m, 6, 8, -1)
    assert not np.array_equal(want, m)
    obuf = torch.full((3 + m.size,), 77, dtype=torch.uint8, device="cuda")
    out = obuf[3:].view(3, 15, 20)
    assert mask_ops.despeckle(d, 6, out=out) is out
    _differences(out.cpu().numpy(), want, "out")
    assert (obuf[:3] == 77).all()
    _differences(mask_ops.components(d)[0].cpu().numpy(), oracle_components(m)[0], "labels")


def test_two_dimensional_input_out_argument_and_the_empty_batch(torch_cuda):
    from gan_segmentation_amd import mask_ops
    torch = torch_cuda
    m = make("blobs", 11, (2, 40, 56))
    d = torch.from_numpy(m).cuda()
    out = torch.empty_like(d)
    assert mask_ops.despeckle(d, 9, out=out) is out
    _differences(out.cpu().numpy(), rule_despeckle(m, 9), "out")
    plane, rows = mask_ops.despeckle(d[1], 9, 4, 3, return_stats=True)
    assert plane.shape == (40, 56) and rows.shape == (ROW,)
    _differences(plane.cpu().numpy(), rule_despeckle(m[1], 9, 4, 3), "plane")
    _differences(rows.cpu().numpy(), rule_rows(m[1], 9, 4), "rows of a plane")
    empty, rows = mask_ops.despeckle(d[:0], 9, return_stats=True)
    assert empty.shape == (0, 40, 56) and empty.dtype == torch.uint8 and rows.shape == (0, ROW)
    assert np.array_equal(mask_ops.despeckle(d, 0).cpu().numpy(), m) and np.array_equal(mask_ops.despeckle(d, 1).cpu().numpy(), m)


def test_the_entry_zeroes_what_it_must(torch_cuda):
    """Twice into the same labels / areas buffers, which hold garbage the first time and the results of ANOTHER input the second."""
    from gan_segmentation_amd import mask_ops
    torch = torch_cuda
    shape = (2, TILE_H + 8, TILE_W + 8)
    a, b = make("blobs", 21, shape), make("classes", 22, shape)
    scratch = (torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device="cuda"),
               torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device="cuda"))
    for m in (a, b, a, a):
        out, rows = mask_ops.despeckle(torch.from_numpy(m).cuda(), 16, return_stats=True, scratch=scratch)
        comps = oracle_components(m, 8)
        _differences(scratch[0].cpu().numpy(), comps[0], "labels")
        _differences(scratch[1].cpu().numpy(), comps[1], "areas")
        _differences(out.cpu().numpy(), rule_despeckle(m, 16, components=comps), "out")
        _differences(rows.cpu().numpy(), rule_rows(m, 16, components=comps), "rows")


def test_value_errors(torch_cuda):
    from gan_segmentation_amd import mask_ops
    torch = torch_cuda
    d = torch.from_numpy(make("half", 1, (2, 16, 16))).cuda()
    flat = torch.zeros(3 * 16 * 16, dtype=torch.uint8, device="cuda")
    a, b = flat[:2 * 256].view(2, 16, 16), flat[256:].view(2, 16, 16)       # two overlapping views of one buffer
    i32 = torch.empty((2, 16, 16), dtype=torch.int32, device="cuda")
    for bad in (dict(mask=d.float()), dict(mask=d[:, :, ::2]), dict(mask=d.cpu()), dict(mask=d, out=d), dict(mask=a, out=b),
                dict(mask=b, out=a), dict(mask=d, out=torch.empty_like(d)[:1]), dict(mask=d, out=torch.empty_like(d).float()),
                dict(mask=d, out=torch.empty_like(d).cpu()), dict(mask=d.view(1, 2, 16, 16)), dict(mask=d, min_area=-1),
                dict(mask=d, min_area=2.0), dict(mask=d, connectivity=6), dict(mask=d, fill="nearest"), dict(mask=d, fill=256),
                dict(mask=d, fill=-1), dict(mask=d, scratch=(i32, i32)), dict(mask=d, scratch=(i32, i32.clone()[:1])),
                dict(mask=d, scratch=(i32, i32.clone().float()))):
        with pytest.raises(ValueError):
            mask_ops.despeckle(**dict(dict(min_area=4), **bad))
    for bad in (dict(mask=d.float()), dict(mask=d.cpu()), dict(mask=d, connectivity=5), dict(mask=d.view(1, 2, 16, 16))):
        with pytest.raises(ValueError):
            mask_ops.components(**bad)


# ---- the generator -----------------------------------------------------------------------------------------------------------
# The reduced synthetic generator of the augment tests (128 px pairs).  These tests prove the plumbing -- that the rule runs, on the
# right tensor, at the right place; the kernels' correctness rests on the direct cases above.  MIN_AREA was chosen on the masks of
# this decoder so that the rule changes the raw mask AND the morphology's result of every sample set below (each test asserts it):
# at 64 it changes 687 and 283 pixels of the raw masks of samples 10..12 and 13..14 (8-connectivity) and 146 and 63 pixels of their
# morphology results, whose smallest components have 25..71 pixels; 16 and 32 leave the second morphology result as it is.
MIN_AREA = 64


def _pair(t):
    return t[0].cpu().numpy(), t[1].cpu().numpy()


def _check_plumbing(raw, cleaned, what, morph=False, **rule):
    (img0, mask0), (img1, mask1) = raw, cleaned
    assert np.array_equal(img1, img0), "%s: the filter changed the image" % what
    before = rule_morph(mask0) if morph else mask0
    want = rule_despeckle(before, MIN_AREA, **rule)
    assert not np.array_equal(want, before), "%s: the rule leaves the mask as it is, the case proves nothing" % what
    assert np.array_equal(mask1, want), "%s: %d mask bytes differ from the rule" % (what, int((mask1 != want).sum()))


@pytest.mark.parametrize("kw,rule", [(dict(), dict()), (dict(output_downscale=2), dict()), (dict(style_mix_prob=1.0), dict()),
                                     (dict(mask_connectivity=4, mask_fill=0), dict(connectivity=4, fill=0)),
                                     (dict(mask_morph=True), dict())],
                         ids=["plain", "downscale2", "mixed", "four-zero", "after-morph"])
def test_generate_indexed_returns_the_rule_on_the_raw_mask(torch_cuda, kw, rule):
    """With mask_morph=True too the mask is the rule on rule_morph(raw): the filter runs after the morphology."""
    base = {k: v for k, v in kw.items() if not k.startswith("mask_")}
    plain, filtered = _build("reduced", 3, **base), _build("reduced", 3, mask_min_area=MIN_AREA, **kw)
    for first, n in ((10, 3), (13, 2)):
        _check_plumbing(_pair(plain.generate_indexed(first, n, seed=4)), _pair(filtered.generate_indexed(first, n, seed=4)),
                        "samples %d..%d" % (first, first + n - 1), morph=kw.get("mask_morph", False), **rule)


def test_min_area_of_one_or_less_is_off(torch_cuda):
    plain = _build("reduced", 3)
    raw = _pair(plain.generate_indexed(10, 3, seed=4))
    for k in (0, 1):
        gen = _build("reduced", 3, mask_min_area=k)
        got = _pair(gen.generate_indexed(10, 3, seed=4))
        assert np.array_equal(got[0], raw[0]) and np.array_equal(got[1], raw[1])
        assert "_raw_masks" not in gen.__dict__, "no scratch without the filter"


def test_out_batch_and_batch_w_get_it_too(torch_cuda):
    torch = torch_cuda
    plain, filtered = _build("reduced", 3), _build("reduced", 3, mask_min_area=MIN_AREA)
    img = torch.empty((3, 128, 128, 3), dtype=torch.uint8, device="cuda")
    mask = torch.full((3, 128, 128), 9, dtype=torch.uint8, device="cuda")
    got = filtered.generate_indexed(20, 3, seed=4, out=(img, mask))
    assert got[0] is img and got[1] is mask
    _check_plumbing(_pair(plain.generate_indexed(20, 3, seed=4)), _pair((img, mask)), "out=")
    z, noise = plain.netG.draw_indexed(30, 3, 4)
    _check_plumbing(_pair(plain.generate_batch(z, noise)), _pair(filtered.generate_batch(z, noise)), "generate_batch")
    dl = plain.netG.mapping(z)[:, None, :].repeat(1, plain.netG.num_style_layers, 1).contiguous()
    _check_plumbing(_pair(plain.generate_batch_w(dl, noise)), _pair(filtered.generate_batch_w(dl, noise)), "generate_batch_w")
    shapes = sorted((k[0], tuple(t.shape), str(t.dtype)) for k, t in filtered.__dict__["_raw_masks"].items())
    assert shapes == [("areas", (3, 128, 128), "torch.int32"), ("labels", (3, 128, 128), "torch.int32"), ("raw", (3, 128, 128), "torch.uint8")]


def test_replayed_graph_keeps_working(torch_cuda):
    """graph_mode "1", captured at the second call: four identical calls into preallocated outputs, every one the rule on the raw
    mask -- the eager filter behind a replayed graph reads what the graph wrote."""
    torch = torch_cuda
    plain, filtered = _build("reduced", 3), _build("reduced", 3, mask_min_area=MIN_AREA)
    filtered.graph_mode, filtered.graph_after = "1", 2
    z, noise = plain.netG.draw_indexed(40, 3, 4)
    raw = _pair(plain.generate_batch(z, noise))
    img = torch.empty((3, 128, 128, 3), dtype=torch.uint8, device="cuda")
    mask = torch.empty((3, 128, 128), dtype=torch.uint8, device="cuda")
    for call in range(4):
        img.fill_(3)
        mask.fill_(9)
        filtered.generate_batch(z, noise, out=(img, mask))
        _check_plumbing(raw, _pair((img, mask)), "call %d" % call)
    assert filtered.graphs_captured() >= 1


def test_training_batches_warp_the_filtered_mask(torch_cuda):
    from gan_segmentation_amd import augment
    plain, filtered = _build("reduced", 3), _build("reduced", 3, mask_min_area=MIN_AREA)
    kw = dict(crop=96, seed=4, first_index=10, num_samples=5)
    a = [(_host(image, label), first) for image, label, first in plain.training_batches(3, **kw)]
    b = [(_host(image, label), first) for image, label, first in filtered.training_batches(3, **kw)]
    assert [f for _, f in a] == [f for _, f in b] == [10, 13]
    changed = 0
    for ((image0, _label0), first), ((image1, label1), _f) in zip(a, b):
        n = min(3, 15 - first)
        _same_bits(image1, image0, "image of batch %d" % first)
        img, mask = plain.generate_indexed(first, n, seed=4)
        want = rule_despeckle(mask.cpu().numpy(), MIN_AREA)
        changed += int((want != mask.cpu().numpy()).sum())
        matrices = augment.plan_matrices(4, first, n, 128, 128, 96, "train")
        _image, label = augment.augment_pairs(img, torch_cuda.from_numpy(want).cuda(), matrices, augment.output_size(128, 128, 96))
        _same_bits(label1, label.cpu().numpy(), "label of batch %d" % first)
    assert changed > 0, "the rule changed no raw mask"


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_mask_min_area_key(torch_cuda, tmp_path):
    """MASK_MIN_AREA on bedrooms (3 samples): every mask_*.png is the rule on the mask of a run without the key, every img_*.jpg
    the same bytes."""
    from PIL import Image
    from tests.test_gpu_downscale import _cli_dirs
    runs = {}
    for name, keys in (("off", dict()), ("on", dict(MASK_MIN_AREA=MIN_AREA, MASK_CONNECTIVITY=4, MASK_FILL="neighbour"))):
        _gcfg, _gp, _dcfg, _dp, run = _cli_dirs(tmp_path, name)
        runs[name] = run(**keys) / "dataset" / "train_generated"
        assert len(list(runs[name].iterdir())) == 6
    changed = 0
    for i in range(3):
        assert (runs["on"] / ("img_%06d.jpg" % i)).read_bytes() == (runs["off"] / ("img_%06d.jpg" % i)).read_bytes()
        raw = np.asarray(Image.open(runs["off"] / ("mask_%06d.png" % i)))
        got = np.asarray(Image.open(runs["on"] / ("mask_%06d.png" % i)))
        assert raw.shape == (256, 256) and np.array_equal(got, rule_despeckle(raw, MIN_AREA, 4)), "mask %d" % i
        changed += int((got != raw).sum())
    assert changed > 0, "the rule changed no mask: the run proves nothing"
