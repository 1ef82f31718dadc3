"""The pair statistics on the GPU (include/gsa_stats.h gsa_pair_stats; pair_stats.pair_stats; DatasetWriter(stats=True); the
PAIR_STATS key): bit for bit the rule of tests/test_pair_stats_host.py, every word of every row."""
import os

import numpy as np
import pytest

from tests.test_gpu_augment import _build
from tests.test_pair_stats_host import ROW, blob_mask, random_image, rule_stats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The tile of csrc/gsa_stats.hip: the seam shapes below are chosen for it (asserted against the source text).
TILE_W, TILE_H, PIX, WAVE_ROWS = 256, 32, 4, 8


def _field(word):
    for name, first in (("reserved", 87), ("edge_v", 86), ("edge_h", 85), ("sqsum", 81), ("csum", 45), ("box", 9), ("count", 0)):
        if word >= first:
            return "%s[%d]" % (name, word - first)


def _stats(torch, img, mask, **kw):
    from gan_segmentation_amd import pair_stats
    di = None if img is None else torch.from_numpy(img).cuda()
    dm = torch.from_numpy(mask).cuda()
    out = pair_stats.pair_stats(di, dm, **kw)
    n = mask.shape[0] if mask.ndim == 3 else 1
    assert out.shape == (n, ROW) and out.dtype == torch.int64 and out.is_contiguous() and out.device == dm.device
    got = out.cpu().numpy()
    assert np.array_equal(dm.cpu().numpy(), mask) and (img is None or np.array_equal(di.cpu().numpy(), img)), "an input was written to"
    return got


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d of %d words differ from the rule, first in sample %d at %s: got %d, rule %d" % (
        what, len(bad), want.size, bad[0][0], _field(bad[0][1]), got[tuple(bad[0])], want[tuple(bad[0])])


def _check(torch, img, mask, what):
    got = _stats(torch, img, mask)
    _same(got, rule_stats(img, mask), "%s %s" % (what, mask.shape))
    return got


# ---- tiny shapes, channel counts, class counts -------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [0, 1, 2, 3, 4])
def test_tiny_shapes_and_every_channel_count(torch_cuda, C):
    """1 x 1 up to sizes that are no multiple of the four pixels of a lane, and (2, 16, 24): the dword path at its smallest."""
    for H, W in ((1, 1), (1, 7), (7, 1), (3, 5), (5, 6), (9, 13), (2, 4), (16, 24), (11, 258)):
        mask = blob_mask(H * 31 + W + C, (2, H, W), classes=3, cell=3, specks=0.05)
        img = random_image(H + W, (2, H, W), C) if C else None
        _check(torch_cuda, img, mask, "C=%d" % C)


@pytest.mark.parametrize("classes", [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_class_count(torch_cuda, classes):
    for shape in ((2, 40, 52), (2, 37, 50)):            # dword and byte path
        mask = blob_mask(classes, shape, classes=classes, cell=6, specks=0.03)
        assert len(np.unique(mask)) == classes
        got = _check(torch_cuda, random_image(classes, shape, 3), mask, "%d classes" % classes)
        assert ((got[:, :9] > 0).sum(axis=1) <= classes).all() and (got[:, classes:9] == 0).all()


def test_values_from_8_up_share_slot_8_but_not_their_edges(torch_cuda):
    for shape in ((2, 40, 52), (1, 37, 50)):
        mask = blob_mask(9, shape, classes=6, cell=5, specks=0.03, values=[0, 3, 7, 8, 200, 255])
        got = _check(torch_cuda, random_image(9, shape, 3), mask, "values 8, 200, 255")
        assert (got[:, 8] == (mask >= 8).reshape(shape[0], -1).sum(axis=1)).all() and (got[:, 8] > 0).all()
    only = np.array([[8, 200, 255, 8] * 3] * 5, np.uint8)
    got = _check(torch_cuda, None, only, "slot 8 only")[0]
    assert got[8] == 60 and got[85] == 5 * 9 and got[86] == 0       # 8|200, 200|255, 255|8 in each group of four; 8|8 between groups is none


# ---- tile seams --------------------------------------------------------------------------------------------------------------
def test_the_tile_is_the_one_these_tests_assume():
    src = open(os.path.join(ROOT, "gan-segmentation_amd", "csrc", "gsa_stats.hip")).read()
    for line in ("constexpr int kTileW = %d;" % TILE_W, "constexpr int kTileH = %d;" % TILE_H, "constexpr int kPix = %d;" % PIX,
                 "constexpr int kWaveRows = %d;" % WAVE_ROWS, "constexpr int kThreads = 256;"):
        assert line in src, line
    assert "const unsigned blocks = (unsigned)(planes * tiles_per_plane);" in src       # one workgroup per tile: no grid cap to cross


SEAM_SHAPES = [(TILE_H - 1, TILE_W - 1), (TILE_H + 1, TILE_W + 1), (2 * TILE_H + 1, 2 * TILE_W + 1), (TILE_H, TILE_W),
               (2 * TILE_H, 2 * TILE_W), (TILE_H + 1, TILE_W - 4), (WAVE_ROWS + 1, TILE_W + 4), (WAVE_ROWS - 1, 2 * TILE_W - 1)]


@pytest.mark.parametrize("H,W", SEAM_SHAPES)
def test_tile_seams(torch_cuda, H, W):
    """Tile - 1, tile + 1 and 2 x tile + 1 each way, whole tiles, a wave's rows +- 1; widths that are and are not multiples of 4."""
    mask = blob_mask(H + W, (2, H, W), classes=4, cell=11, specks=0.02)
    _check(torch_cuda, random_image(H, (2, H, W), 3), mask, "seam")
    _check(torch_cuda, None, mask, "seam, labels only")


@pytest.mark.parametrize("W", [2 * TILE_W + 1, 2 * TILE_W + 4])
def test_class_boundaries_on_the_seams(torch_cuda, W):
    """Two classes that meet exactly on a tile seam, a wave seam and a lane seam, along x and along y: every edge is counted once and
    both boxes end on the seam."""
    H = 2 * TILE_H + 1
    cuts = [(None, TILE_W), (None, 2 * TILE_W), (None, TILE_W - PIX), (None, TILE_W + 1), (TILE_H, None), (2 * TILE_H, None),
            (WAVE_ROWS, None), (TILE_H + WAVE_ROWS, None), (TILE_H, TILE_W)]
    mask = np.zeros((len(cuts), H, W), np.uint8)
    for k, (y, x) in enumerate(cuts):
        mask[k, y if y is not None else 0:, x if x is not None else 0:] = 2
    got = _check(torch_cuda, random_image(W, mask.shape, 3), mask, "boundary on a seam")
    for k, (y, x) in enumerate(cuts):
        y, x = y or 0, x or 0
        assert tuple(got[k, 9 + 8:9 + 12]) == (x, y, W - 1, H - 1) and got[k, 2] == (H - y) * (W - x)
        assert got[k, 85] == (H - y if x else 0) and got[k, 86] == (W - x if y else 0)


@pytest.mark.parametrize("W", [2 * TILE_W + 1, 2 * TILE_W + 4])
def test_a_single_foreground_pixel(torch_cuda, W):
    """One pixel of class 1 in every corner and on both sides of every seam: the box is that pixel."""
    H = 2 * TILE_H + 1
    ys = [0, WAVE_ROWS - 1, WAVE_ROWS, TILE_H - 1, TILE_H, 2 * TILE_H - 1, 2 * TILE_H]
    xs = [0, PIX - 1, PIX, TILE_W - 1, TILE_W, 2 * TILE_W - 1, 2 * TILE_W, W - 1]
    spots = [(y, x) for y in (0, H - 1) for x in xs] + [(y, x) for y in ys for x in (0, TILE_W - 1, TILE_W, W - 1)]
    mask = np.zeros((len(spots), H, W), np.uint8)
    for k, (y, x) in enumerate(spots):
        mask[k, y, x] = 1
    got = _check(torch_cuda, random_image(7, mask.shape, 1), mask, "single pixel")
    for k, (y, x) in enumerate(spots):
        assert tuple(got[k, 13:17]) == (x, y, x, y) and got[k, 1] == 1 and tuple(got[k, 9:13]) == (0, 0, W - 1, H - 1)


# ---- row wrap and batch leak ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(5, 8), (6, 7), (TILE_H + 2, TILE_W), (3, TILE_W + 1)])
def test_the_end_of_a_row_is_no_neighbour_of_the_next_row(torch_cuda, H, W):
    mask = np.zeros((1, H, W), np.uint8)
    mask[:, :, -1] = 1          # every row ends in 1 and begins in 0
    got = _check(torch_cuda, None, mask, "row wrap")[0]
    assert got[85] == (H if W > 1 else 0) and got[86] == 0


def test_images_of_a_batch_do_not_leak_into_each_other(torch_cuda):
    """Planes smaller than a tile, so a workgroup's loads would reach into the next image; the last row of one image and the first
    of the next differ everywhere."""
    shape = (1, 20, 36)
    a, b = np.full(shape, 1, np.uint8), blob_mask(3, shape, classes=3, cell=4)
    ia, ib = random_image(1, shape, 3), random_image(2, shape, 3)
    both = _check(torch_cuda, np.concatenate([ia, ib, ia]), np.concatenate([a, b, a]), "batch")
    alone = [_stats(torch_cuda, ia, a)[0], _stats(torch_cuda, ib, b)[0]]
    assert np.array_equal(both[0], alone[0]) and np.array_equal(both[1], alone[1]) and np.array_equal(both[2], alone[0])
    assert both[0][86] == 0 and not np.array_equal(both[0], both[1])


def test_sources_that_are_slices(torch_cuda):
    """n = 3 out of a larger batch (a contiguous view at an offset), and a strided view made contiguous; the strided view itself is
    refused."""
    from gan_segmentation_amd import pair_stats
    torch = torch_cuda
    mask, img = blob_mask(4, (5, 33, 44), classes=4, cell=7), random_image(4, (5, 33, 88), 3)
    dm, di = torch.from_numpy(mask).cuda(), torch.from_numpy(img).cuda()
    view = di[1:4, :, ::2]
    assert not view.is_contiguous() and dm[1:4].is_contiguous()
    got = pair_stats.pair_stats(view.contiguous(), dm[1:4]).cpu().numpy()
    _same(got, rule_stats(np.ascontiguousarray(img[1:4, :, ::2]), mask[1:4]), "slices")
    with pytest.raises(ValueError):
        pair_stats.pair_stats(view, dm[1:4])


@pytest.mark.parametrize("offset", [1, 3])
def test_a_view_that_is_not_dword_aligned(torch_cuda, offset):
    """W is a multiple of 4 but the pointers are not 4-byte aligned: the mask, the image, and both."""
    from gan_segmentation_amd import pair_stats
    torch = torch_cuda
    shape = (3, 15, 20)
    mask, img = blob_mask(offset, shape, classes=3, cell=4), random_image(offset, shape, 3)
    want = rule_stats(img, mask)

    def shifted(a, off):
        buf = torch.zeros(off + a.size, dtype=torch.uint8, device="cuda")
        v = buf[off:].view(a.shape)
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 4 == off % 4
        return v

    for moff, ioff in ((offset, 0), (0, offset), (offset, offset)):
        got = pair_stats.pair_stats(shifted(img, ioff), shifted(mask, moff)).cpu().numpy()
        _same(got, want, "offsets %d / %d" % (moff, ioff))


# ---- width of the accumulators -------------------------------------------------------------------------------------------------
def test_sum_of_squares_past_32_bits(torch_cuda):
    H, W = 264, 256
    img = np.full((1, H, W, 3), 255, np.uint8)
    mask = np.ones((1, H, W), np.uint8)
    got = _check(torch_cuda, img, mask, "all 255")[0]
    assert got[81] == H * W * 65025 > 2 ** 32 and got[45 + 4] == H * W * 255


def test_channel_sum_past_32_bits(torch_cuda):
    H = W = 4104
    img = np.full((1, H, W, 1), 255, np.uint8)
    mask = np.ones((1, H, W), np.uint8)
    got = _check(torch_cuda, img, mask, "all 255, one channel")[0]
    assert got[45 + 4] == H * W * 255 > 2 ** 32 - 2 ** 16 and got[81] == H * W * 65025     # 4 294 918 080: past a signed 32-bit sum


# ---- the contract ----------------------------------------------------------------------------------------------------------------
def test_rows_are_fully_overwritten_and_out_is_returned(torch_cuda):
    from gan_segmentation_amd import pair_stats
    torch = torch_cuda
    mask, img = blob_mask(6, (3, 40, 56), classes=2), random_image(6, (3, 40, 56), 3)
    dm, di = torch.from_numpy(mask).cuda(), torch.from_numpy(img).cuda()
    want = rule_stats(img, mask)
    for fill in (-1, 0x7F7F7F7F7F7F7F7F, -2 ** 63):
        out = torch.full((3, ROW), fill, dtype=torch.int64, device="cuda")
        assert pair_stats.pair_stats(di, dm, out=out) is out
        _same(out.cpu().numpy(), want, "out filled with %d" % fill)
    buf = torch.full((5, ROW), 77, dtype=torch.int64, device="cuda")      # a contiguous slice: its neighbours stay
    pair_stats.pair_stats(di, dm, out=buf[1:4])
    _same(buf[1:4].cpu().numpy(), want, "out slice")
    assert (buf[0] == 77).all() and (buf[4] == 77).all()
    u = pair_stats.unpack(out)
    assert u["count"].shape == (3, 9) and int(u["count"].sum()) == 3 * 40 * 56 and u["box"].shape == (3, 9, 4)


def test_two_and_three_dimensional_inputs_and_the_empty_batch(torch_cuda):
    from gan_segmentation_amd import pair_stats
    torch = torch_cuda
    mask, img = blob_mask(8, (2, 40, 56)), random_image(8, (2, 40, 56), 3)
    dm, di = torch.from_numpy(mask).cuda(), torch.from_numpy(img).cuda()
    want = rule_stats(img, mask)
    plane = pair_stats.pair_stats(di[1], dm[1])
    assert plane.shape == (1, ROW)
    _same(plane.cpu().numpy(), want[1:], "2-D mask")
    _same(pair_stats.pair_stats(None, dm[0]).cpu().numpy(), rule_stats(None, mask[0]), "2-D mask, no image")
    empty = pair_stats.pair_stats(di[:0], dm[:0])
    assert empty.shape == (0, ROW) and empty.dtype == torch.int64
    assert pair_stats.pair_stats(None, dm[:0], out=empty) is empty


def test_value_errors(torch_cuda):
    from gan_segmentation_amd import pair_stats
    torch = torch_cuda
    dm = torch.zeros((2, 16, 16), dtype=torch.uint8, device="cuda")
    di = torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device="cuda")
    ok = torch.empty((2, ROW), dtype=torch.int64, device="cuda")
    for bad in (dict(img=di, mask=dm.float()), dict(img=di.float(), mask=dm), dict(img=di, mask=dm[:, :, ::2]), dict(img=di, mask=dm.cpu()),
                dict(img=di.cpu(), mask=dm), dict(img=di[:1], mask=dm), dict(img=di[0], mask=dm), dict(img=di, mask=dm[0]),
                dict(img=torch.zeros((2, 16, 16, 5), dtype=torch.uint8, device="cuda"), mask=dm), dict(img=di[..., :0], mask=dm),
                dict(img=di.cpu().numpy(), mask=dm), dict(img=di, mask=dm.view(1, 2, 16, 16)), dict(img=di, mask=dm, out=ok[:1]),
                dict(img=di, mask=dm, out=ok.int()), dict(img=di, mask=dm, out=ok.cpu()), dict(img=di, mask=dm, out=ok.t())):
        with pytest.raises(ValueError):
            pair_stats.pair_stats(**bad)


def test_the_result_is_on_the_callers_stream(torch_cuda):
    """On a side stream the inputs are produced by that stream's own work (a long chain of fills, then the copies): the pass must
    run behind it, and an event recorded on that stream covers the rows."""
    from gan_segmentation_amd import pair_stats
    torch = torch_cuda
    mask, img = blob_mask(12, (4, 256, 256), classes=3), random_image(12, (4, 256, 256), 3)
    want = rule_stats(img, mask)
    src_m, src_i = torch.from_numpy(mask).cuda(), torch.from_numpy(img).cuda()
    dm, di = torch.zeros_like(src_m), torch.zeros_like(src_i)
    ballast = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for k in range(20):
            ballast.fill_(k)
        dm.copy_(src_m)
        di.copy_(src_i)
        rows = pair_stats.pair_stats(di, dm)
        done = torch.cuda.Event()
        done.record(side)
    done.synchronize()
    host = torch.empty(rows.shape, dtype=rows.dtype).pin_memory()
    with torch.cuda.stream(side):
        host.copy_(rows, non_blocking=True)
        side.synchronize()
    _same(host.numpy(), want, "side stream")


# ---- the writer ------------------------------------------------------------------------------------------------------------------
def _pairs(gen, first, n, seed=4):
    img, mask = gen.generate_indexed(first, n, seed=seed)
    return img.cpu().numpy(), mask.cpu().numpy()


def _run_writer(gen, dst, batches, seed=4, **kw):
    """One writer over (first, n) batches -> its shard file."""
    from gan_segmentation_amd.dataset_writer import DatasetWriter
    with DatasetWriter(str(dst), workers=2, stats=True, **kw) as w:
        for first, n in batches:
            img, mask = gen.generate_indexed(first, n, seed=seed)
            w.submit(img, mask, first, status=gen.snapshot_status())
    return w.stats_path


@pytest.mark.parametrize("kw", [dict(), dict(gpu_jpeg=True, gpu_png=True)], ids=["raw", "encoded"])
def test_writer_rows_are_the_rule_on_what_generate_indexed_returned(torch_cuda, tmp_path, kw):
    """10 samples as batches of 4 + 4 + 2 in one writer, and as two shards (world 2, batch 3) through main.shard_batches: the shard
    files hold the rule's rows, and both runs merge to the same bytes."""
    from gan_segmentation_amd import main as cli
    from gan_segmentation_amd import pair_stats
    gen = _build("reduced", 4)
    img, mask = [np.concatenate(t) for t in zip(*[_pairs(gen, f, n) for f, n in ((20, 4), (24, 4), (28, 2))])]
    want = rule_stats(img, mask)
    assert len(np.unique(mask)) > 1 and (want[:, 85] > 0).any()

    path = _run_writer(gen, tmp_path / "one", [(20, 4), (24, 4), (28, 2)], **kw)
    assert os.path.basename(path) == "pair_stats_000020_000030.npz"
    with np.load(path) as z:
        assert z["index"].dtype == np.int64 and np.array_equal(z["index"], np.arange(20, 30))
        assert (int(z["H"]), int(z["W"]), int(z["C"])) == (128, 128, 3)
        _same(z["rows"], want, "the writer's rows")
    assert len(os.listdir(str(tmp_path / "one"))) == 21

    # world 2, batch 3, the slices of main.shard_batches shifted to the same 10 indices
    for rank in range(2):
        batches = [(20 + first, n) for first, n in cli.shard_batches(10, 3, 2, rank)]
        assert max(n for _f, n in batches) == 3
        _run_writer(gen, tmp_path / "two", batches, **kw)
    names = sorted(p for p in os.listdir(str(tmp_path / "two")) if p.endswith(".npz"))
    assert names == ["pair_stats_000020_000025.npz", "pair_stats_000025_000030.npz"]
    one, two = pair_stats.merge_shards(str(tmp_path / "one")), pair_stats.merge_shards(str(tmp_path / "two"))
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes() == want.tobytes() and one[2:] == two[2:]


def test_a_withheld_batch_contributes_no_rows(torch_cuda, tmp_path):
    """The statistics-range word forced from the third pass on (gsa_debug_inject kind 3): the files and the rows of the first two
    batches exist, nothing of the later ones."""
    from gan_segmentation_amd.dataset_writer import DatasetWriter, DeviceCheckFailed
    gen = _build("reduced", 2)
    want = rule_stats(*[np.concatenate(t) for t in zip(*[_pairs(gen, f, 2) for f in (0, 2)])])
    gen.netG._model.ctx.debug_inject(3, 2)
    w = DatasetWriter(str(tmp_path), workers=2, stats=True, gpu_jpeg=True, gpu_png=True)
    with pytest.raises(DeviceCheckFailed) as e:
        for first in (0, 2, 4, 6):
            img, mask = gen.generate_indexed(first, 2, seed=4)
            w.submit(img, mask, first, status=gen.snapshot_status())
        w.close()
    assert e.value.first_failure.first_index == 4
    try:
        w.close()
    except DeviceCheckFailed:
        pass
    names = sorted(os.listdir(str(tmp_path)))
    assert names == sorted(["img_%06d.jpg" % i for i in range(4)] + ["mask_%06d.png" % i for i in range(4)] + ["pair_stats_000000_000004.npz"])
    with np.load(w.stats_path) as z:
        assert np.array_equal(z["index"], np.arange(4))
        _same(z["rows"], want, "the released batches")


def test_mask_morph_statistics_are_those_of_the_cleaned_mask(torch_cuda, tmp_path):
    from tests.test_mask_morph_host import rule_morph
    plain, morph = _build("reduced", 3), _build("reduced", 3, mask_morph=True)
    img, raw = _pairs(plain, 10, 3)
    cleaned = rule_morph(raw)
    assert not np.array_equal(cleaned, raw)
    with np.load(_run_writer(morph, tmp_path, [(10, 3)])) as z:
        _same(z["rows"], rule_stats(img, cleaned), "rows of the cleaned mask")
        assert not np.array_equal(z["rows"], rule_stats(img, raw))


def test_labels_of_the_training_stream_count_their_border_in_slot_8(torch_cuda):
    from gan_segmentation_amd import pair_stats
    gen = _build("reduced", 3)
    seen = 0
    for _image, label, _first in gen.training_batches(3, crop=160, seed=4, first_index=10, num_samples=3):
        host = label.cpu().numpy()
        got = pair_stats.pair_stats(None, label).cpu().numpy()
        _same(got, rule_stats(None, host), "labels")
        border = (host == 255).reshape(host.shape[0], -1).sum(axis=1)
        assert (border > 0).all() and np.array_equal(got[:, 8], border) and (got[:, 45:85] == 0).all()
        seen += host.shape[0]
    assert seen == 3


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_pair_stats_key(torch_cuda, tmp_path, capsys):
    """PAIR_STATS: true on bedrooms (3 samples, batch 2): one shard file with the rule's rows of the written masks, the merge tool's
    summary beside it; without the key the directory holds the six pair files only."""
    import json
    from PIL import Image
    from gan_segmentation_amd import pair_stats
    from tests.test_gpu_downscale import _cli_dirs
    runs = {}
    for name, keys in (("off", dict()), ("on", dict(PAIR_STATS=True))):
        _gcfg, _gp, _dcfg, _dp, run = _cli_dirs(tmp_path, name)
        runs[name] = run(**keys) / "dataset" / "train_generated"
    assert len(list(runs["off"].iterdir())) == 6 and not list(runs["off"].glob("pair_stats*"))
    assert sorted(p.name for p in runs["on"].glob("pair_stats*")) == ["pair_stats_000000_000003.npz"]
    assert len(list(runs["on"].iterdir())) == 7
    masks = np.stack([np.asarray(Image.open(runs["on"] / ("mask_%06d.png" % i))) for i in range(3)])
    for i in range(3):
        assert (runs["on"] / ("img_%06d.jpg" % i)).read_bytes() == (runs["off"] / ("img_%06d.jpg" % i)).read_bytes()
        assert (runs["on"] / ("mask_%06d.png" % i)).read_bytes() == (runs["off"] / ("mask_%06d.png" % i)).read_bytes()
    index, rows, H, W, C = pair_stats.merge_shards(str(runs["on"]))
    assert (H, W, C) == (256, 256, 3) and np.array_equal(index, np.arange(3))
    _same(rows[:, :45], rule_stats(None, masks)[:, :45], "counts and boxes of the written masks")
    _same(rows[:, 85:], rule_stats(None, masks)[:, 85:], "edges of the written masks")
    assert pair_stats.main([str(runs["on"])]) == 0
    assert "class frequency" in capsys.readouterr().out
    summary = json.loads((runs["on"] / "pair_stats_summary.json").read_text())
    assert summary["samples"] == 3 and summary["pixels"] == [int(v) for v in rows[:, :9].sum(axis=0)]
    assert pair_stats.main([str(runs["off"])]) == 1
