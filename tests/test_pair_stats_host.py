"""The pair statistics without a GPU (include/gsa_stats.h; pair_stats.summarise, the shard files and the merge tool; the PAIR_STATS
key; DatasetWriter(stats=...)).

``rule_stats(img, mask)`` is the canonical rule in numpy, written the slow obvious way: a boolean mask per slot, np.nonzero for the
boxes, int64 sums.  It is held here against rows computed by hand and against invariants; the GPU tests
(tests/test_gpu_pair_stats.py) hold the kernel to it bit for bit."""
import json
import os
import re

import numpy as np
import pytest

from tests.test_downscale_host import _ModelLoaded, _config, no_models  # noqa: F401  (no_models is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW = 88


# -- the rule ------------------------------------------------------------------------------------------------------------------
def rule_stats(img, mask):
    """img (n, H, W, C) / (H, W, C) u8 or None, mask (n, H, W) / (H, W) u8 -> (n, 88) int64: section 1 of the rule, word for word."""
    mask = np.asarray(mask)
    assert mask.dtype == np.uint8 and mask.ndim in (2, 3)
    if mask.ndim == 2:
        mask, img = mask[None], None if img is None else np.asarray(img)[None]
    n, H, W = mask.shape
    C = 0
    if img is not None:
        img = np.asarray(img)
        assert img.dtype == np.uint8 and img.shape[:3] == mask.shape and img.ndim == 4
        C = img.shape[3]
    rows = np.zeros((n, ROW), np.int64)
    for k in range(n):
        m = mask[k]
        slot = np.minimum(m, 8)
        for s in range(9):
            sel = slot == s
            ys, xs = np.nonzero(sel)
            rows[k, s] = ys.size
            rows[k, 9 + 4 * s:13 + 4 * s] = (xs.min(), ys.min(), xs.max(), ys.max()) if ys.size else (W, H, -1, -1)
            for c in range(C):
                rows[k, 45 + 4 * s + c] = img[k, :, :, c][sel].astype(np.int64).sum()
        for c in range(C):
            rows[k, 81 + c] = (img[k, :, :, c].astype(np.int64) ** 2).sum()
        rows[k, 85] = int((m[:, :-1] != m[:, 1:]).sum())
        rows[k, 86] = int((m[:-1, :] != m[1:, :]).sum())
    return rows


def blob_mask(seed, shape, classes=3, cell=12, specks=0.01, values=None):
    """(n, H, W) u8: a coarse random class grid blown up to `cell`-px blocks (coherent regions, as a decoder's masks) with a share
    `specks` of single flipped pixels (ragged edges).  ``values`` maps the class index to the byte that is stored."""
    rng = np.random.RandomState(seed)
    n, H, W = shape
    coarse = rng.randint(0, classes, size=(n, H // cell + 2, W // cell + 2))
    oy, ox = rng.randint(0, cell, size=2)
    m = np.kron(coarse, np.ones((cell, cell), np.int64))[:, oy:oy + H, ox:ox + W]
    flip = rng.rand(n, H, W) < specks
    m = np.where(flip, rng.randint(0, classes, size=(n, H, W)), m)
    if values is not None:
        m = np.asarray(values)[m]
    return np.ascontiguousarray(m.astype(np.uint8))


def random_image(seed, shape, C):
    return np.random.RandomState(seed).randint(0, 256, size=tuple(shape) + (C,)).astype(np.uint8)


def _row(count=(), box=(), csum=(), sqsum=(), edge_h=0, edge_v=0, H=0, W=0):
    r = np.zeros(ROW, np.int64)
    for s in range(9):
        r[9 + 4 * s:13 + 4 * s] = (W, H, -1, -1)
    for s, v in count:
        r[s] = v
    for s, v in box:
        r[9 + 4 * s:13 + 4 * s] = v
    for s, v in csum:
        r[45 + 4 * s:45 + 4 * s + len(v)] = v
    r[81:81 + len(sqsum)] = sqsum
    r[85], r[86] = edge_h, edge_v
    return r


def test_rule_on_pairs_computed_by_hand():
    # 2 x 3, two channels: slot 0 = {(0,0), (1,0), (1,1)}, slot 1 = {(0,1), (0,2)}, slot 8 = {(1,2)} (value 9)
    mask = np.array([[0, 1, 1], [0, 0, 9]], np.uint8)
    img = np.stack([np.array([[1, 2, 3], [4, 5, 6]]), np.array([[10, 20, 30], [40, 50, 60]])], axis=-1).astype(np.uint8)
    want = _row(count=[(0, 3), (1, 2), (8, 1)], box=[(0, (0, 0, 1, 1)), (1, (1, 0, 2, 0)), (8, (2, 1, 2, 1))],
                csum=[(0, (10, 100)), (1, (5, 50)), (8, (6, 60))], sqsum=(91, 9100), edge_h=2, edge_v=2, H=2, W=3)
    assert np.array_equal(rule_stats(img, mask)[0], want)
    # one pixel, the ignore label, no image
    want = _row(count=[(8, 1)], box=[(8, (0, 0, 0, 0))], H=1, W=1)
    assert np.array_equal(rule_stats(None, np.array([[255]], np.uint8))[0], want)
    # 8 and 200 share slot 8, but the edge is counted on the raw values; 7 is a slot of its own
    mask = np.array([[8, 200, 7]], np.uint8)
    img = np.array([[[255], [255], [2]]], np.uint8)
    want = _row(count=[(7, 1), (8, 2)], box=[(7, (2, 0, 2, 0)), (8, (0, 0, 1, 0))], csum=[(7, (2,)), (8, (510,))],
                sqsum=(2 * 65025 + 4,), edge_h=2, edge_v=0, H=1, W=3)
    assert np.array_equal(rule_stats(img, mask)[0], want)
    # a column: only vertical neighbours; rows that end in one value and begin in another are no neighbours
    mask = np.array([[1, 2], [1, 2], [1, 2]], np.uint8)
    got = rule_stats(None, mask)[0]
    assert got[85] == 3 and got[86] == 0 and tuple(got[13:17]) == (0, 0, 0, 2) and tuple(got[17:21]) == (1, 0, 1, 2)
    # a batch is its samples one by one
    a, b = blob_mask(1, (1, 9, 11)), blob_mask(2, (1, 9, 11))
    ia, ib = random_image(3, (1, 9, 11), 3), random_image(4, (1, 9, 11), 3)
    both = rule_stats(np.concatenate([ia, ib]), np.concatenate([a, b]))
    assert np.array_equal(both[0], rule_stats(ia, a)[0]) and np.array_equal(both[1], rule_stats(ib, b)[0])


@pytest.mark.parametrize("H,W,C", [(1, 1, 1), (5, 7, 3), (16, 16, 4), (33, 20, 0), (40, 41, 2)])
def test_rule_invariants(H, W, C):
    mask = blob_mask(H + W, (2, H, W), classes=4, cell=5, values=[0, 1, 5, 255])
    img = random_image(H * W, (2, H, W), C) if C else None
    rows = rule_stats(img, mask)
    assert rows.shape == (2, ROW) and rows.dtype == np.int64 and (rows[:, 87] == 0).all()
    assert (rows[:, :9].sum(axis=1) == H * W).all()
    for c in range(4):
        want = img[..., c].astype(np.int64).sum(axis=(1, 2)) if c < C else 0
        assert np.array_equal(rows[:, 45 + c:81:4].sum(axis=1), np.broadcast_to(want, (2,)))
    const = rule_stats(None, np.full((H, W), 3, np.uint8))[0]
    assert const[85] == 0 and const[86] == 0 and const[3] == H * W and tuple(const[21:25]) == (0, 0, W - 1, H - 1)
    yy, xx = np.mgrid[:H, :W]
    board = rule_stats(None, ((yy + xx) & 1).astype(np.uint8))[0]
    assert board[85] == H * (W - 1) and board[86] == (H - 1) * W


def test_fields_are_the_header_offsets():
    from gan_segmentation_amd import pair_stats
    header = open(os.path.join(ROOT, "include", "gsa_stats.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"#define GSA_STATS_([A-Z_]+) (\d+)", header)}
    assert defines["ROW"] == pair_stats.ROW == ROW and defines["SLOTS"] == pair_stats.SLOTS and defines["CHANNELS"] == pair_stats.CHANNELS
    for name, (first, _shape) in pair_stats.FIELDS.items():
        assert defines[name.upper()] == first, name
    assert defines["RESERVED"] == 87
    rows = np.arange(2 * ROW, dtype=np.int64).reshape(2, ROW)
    u = pair_stats.unpack(rows)
    assert set(u) == {"count", "box", "csum", "sqsum", "edge_h", "edge_v"}
    assert u["count"].shape == (2, 9) and u["box"].shape == (2, 9, 4) and u["csum"].shape == (2, 9, 4) and u["sqsum"].shape == (2, 4)
    assert u["box"][1, 2, 3] == ROW + 9 + 4 * 2 + 3 and u["csum"][0, 8, 1] == 45 + 33 and u["edge_v"][1] == ROW + 86 and u["edge_h"][0] == 85
    with pytest.raises(ValueError):
        pair_stats.unpack(rows[:, :80])


# -- summarise -----------------------------------------------------------------------------------------------------------------
def _dataset(seed=5, m=7, H=24, W=36, C=3):
    mask = blob_mask(seed, (m, H, W), classes=4, cell=9, values=[0, 1, 3, 255])
    mask[2] = 0                 # no foreground
    mask[5] = 255               # nothing but the ignore label: no foreground either
    img = random_image(seed + 1, (m, H, W), C)
    return img, mask, np.arange(100, 100 + m)


def test_summarise_against_numpy():
    from gan_segmentation_amd import pair_stats
    img, mask, index = _dataset()
    m, H, W, C = img.shape
    s = pair_stats.summarise(index, rule_stats(img, mask), H, W, C)
    flat = img.reshape(-1, C).astype(np.float64)
    assert np.allclose(s["mean"], flat.mean(axis=0), rtol=1e-12, atol=0) and np.allclose(s["std"], flat.std(axis=0), rtol=1e-12, atol=0)
    assert np.allclose(s["mean_unit"], flat.mean(axis=0) / 255, rtol=1e-12, atol=0)
    assert np.allclose(s["std_unit"], flat.std(axis=0) / 255, rtol=1e-12, atol=0)
    assert abs(sum(s["frequency"]) - 1.0) < 1e-12 and sum(s["pixels"]) == m * H * W and s["samples"] == m
    slot = np.minimum(mask, 8)
    assert s["pixels"] == [int((slot == k).sum()) for k in range(9)]
    assert s["presence"] == [int((slot == k).any(axis=(1, 2)).sum()) for k in range(9)]
    assert s["empty_masks"] == [102, 105]
    assert s["num_classes"] == 4 and s["pixels"][2] == 0
    # classes 0, 1 and 3 are present: 2 (absent), 4..7 and the ignore slot get no weight
    for key in ("weights_inverse_frequency", "weights_median_frequency"):
        assert [w is not None for w in s[key]] == [True, True, False, True, False, False, False, False, False], key
    inv = [s["weights_inverse_frequency"][k] for k in (0, 1, 3)]
    assert abs(sum(inv) / 3 - 1.0) < 1e-12
    assert np.allclose([inv[0] * s["frequency"][0], inv[1] * s["frequency"][1]], inv[2] * s["frequency"][3], rtol=1e-12)
    among = [s["pixels"][k] / (s["presence"][k] * H * W) for k in (0, 1, 3)]
    assert np.allclose([s["weights_median_frequency"][k] for k in (0, 1, 3)], np.median(among) / np.array(among), rtol=1e-12)
    share = ((slot >= 1) & (slot <= 7)).reshape(m, -1).mean(axis=1)
    fg = s["foreground_fraction"]
    assert np.isclose(fg["min"], share.min(), rtol=1e-12) and np.isclose(fg["max"], share.max(), rtol=1e-12)
    assert np.isclose(fg["median"], np.median(share), rtol=1e-12, atol=1e-15)
    assert np.allclose(fg["deciles"], np.percentile(share, np.arange(0, 101, 10)), rtol=1e-12, atol=1e-15)
    edges = (mask[:, :, :-1] != mask[:, :, 1:]).sum() + (mask[:, :-1] != mask[:, 1:]).sum()
    assert np.isclose(s["mean_edges"], edges / m, rtol=1e-12)
    json.dumps(s)               # a plain dict
    # fewer classes asked for than present: class 3 loses its weight
    assert pair_stats.summarise(index, rule_stats(img, mask), H, W, C, num_classes=2)["weights_inverse_frequency"][3] is None
    with pytest.raises(ValueError):
        pair_stats.summarise(index, rule_stats(img, mask), H, W + 1, C)


# -- shard files and the merge tool ----------------------------------------------------------------------------------------------
def _write_shards(dst, cuts, rows, index, size):
    from gan_segmentation_amd import pair_stats
    os.makedirs(dst, exist_ok=True)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        path = pair_stats.save_shard(dst, index[lo:hi], rows[lo:hi], *size)
        assert os.path.basename(path) == "pair_stats_%06d_%06d.npz" % (index[lo], index[hi - 1] + 1)


def test_merge_is_the_same_for_any_cut(tmp_path, capsys):
    from gan_segmentation_amd import pair_stats
    img, mask, index = _dataset(m=10)
    _m, H, W, C = img.shape
    rows = rule_stats(img, mask)
    out = {}
    for name, cuts in (("whole", [0, 10]), ("batches", [0, 4, 8, 10]), ("ranks", [0, 5, 10]), ("ragged", [0, 1, 2, 9, 10])):
        _write_shards(str(tmp_path / name), cuts, rows, index, (H, W, C))
        assert pair_stats.main([str(tmp_path / name)]) == 0
        i, r, h, w, c = pair_stats.merge_shards(str(tmp_path / name))
        assert (h, w, c) == (H, W, C) and i.dtype == np.int64 and r.dtype == np.int64
        out[name] = (i.tobytes(), r.tobytes(), (tmp_path / name / "pair_stats_summary.json").read_bytes())
    assert all(v == out["whole"] for v in out.values())
    assert out["whole"][1] == rows.tobytes() and out["whole"][0] == index.astype(np.int64).tobytes()
    printed = capsys.readouterr().out
    assert "class frequency" in printed and "mean / 255" in printed and "empty masks: 2" in printed
    assert json.loads(out["whole"][2])["empty_masks"] == [102, 105]


def test_merge_refuses_duplicates_gaps_and_mixed_sizes(tmp_path, capsys):
    from gan_segmentation_amd import pair_stats
    img, mask, index = _dataset(m=6)
    _m, H, W, C = img.shape
    rows = rule_stats(img, mask)
    size = (H, W, C)
    cases = {
        "duplicate": ([(0, 4), (3, 6)], size, "duplicate index 103"),
        "gap": ([(0, 2), (4, 6)], size, "gap: no rows for the indices 102..103"),
        "mixed": ([(0, 3)], size, "differing sizes"),
    }
    for name, (parts, sz, message) in cases.items():
        d = str(tmp_path / name)
        os.makedirs(d)
        for lo, hi in parts:
            pair_stats.save_shard(d, index[lo:hi], rows[lo:hi], *sz)
        if name == "mixed":
            pair_stats.save_shard(d, index[3:6], rows[3:6], H, W + 2, C)
        with pytest.raises(ValueError, match=message):
            pair_stats.merge_shards(d)
        assert pair_stats.main([d]) == 1 and message in capsys.readouterr().err
        assert not os.path.exists(os.path.join(d, "pair_stats_summary.json"))
    os.makedirs(str(tmp_path / "none"))
    with pytest.raises(ValueError, match="no pair_stats"):
        pair_stats.merge_shards(str(tmp_path / "none"))


# -- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_symbols_are_exported(hip_library):
    """include/gsa_stats.h declares the one entry; include/gsa.h does not know it."""
    from tests.common import header_declarations
    assert set(header_declarations("gsa_stats.h")[1]) == {"gsa_pair_stats"}
    assert "gsa_pair_stats" not in open(os.path.join(ROOT, "include", "gsa.h")).read()


def test_entry_rejects_bad_arguments_before_touching_the_gpu(hip_library):
    """Argument validation happens on the host (no HIP call precedes it); an empty batch is a successful no-op."""
    from gan_segmentation_amd._lib import load_library
    fn = load_library().fn("gsa_pair_stats")
    good = dict(n=2, H=32, W=48, C=3, img=1 << 20, mask=2 << 20, rows=3 << 20)

    def call(**kw):
        a = dict(good, **kw)
        return fn(None, a["n"], a["H"], a["W"], a["C"], a["img"], a["mask"], a["rows"])

    for bad in (dict(n=-1), dict(H=0), dict(W=0), dict(H=65536), dict(W=65536), dict(W=-3), dict(H=65535, W=65535), dict(H=32769, W=65535),
                dict(C=-1), dict(C=5), dict(mask=None), dict(rows=None), dict(img=None), dict(img=None, C=1)):
        assert call(**bad) == -1, bad
    assert call(n=0) == 0 and call(n=0, img=None, mask=None, rows=None) == 0 and call(n=0, C=0, img=None) == 0


def test_pair_stats_checks_its_tensors_before_any_gpu_work():
    import torch
    from gan_segmentation_amd import pair_stats
    for bad in (torch.zeros((4, 4), dtype=torch.uint8), torch.zeros((1, 4, 4), dtype=torch.float32), np.zeros((4, 4), np.uint8), None):
        with pytest.raises(ValueError, match="mask"):
            pair_stats.pair_stats(None, bad)


# -- the key and the writer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [1, 0, "yes", "true", None, 1.0])
def test_pair_stats_key_rejects_what_is_not_a_bool(value):
    from gan_segmentation_amd import pair_stats
    with pytest.raises(ValueError, match="PAIR_STATS"):
        pair_stats.check_pair_stats(value)
    assert pair_stats.check_pair_stats(True) is True and pair_stats.check_pair_stats(False) is False


@pytest.mark.parametrize("value", [2, "yes"])
def test_cli_rejects_a_bad_key_before_loading_a_model(tmp_path, no_models, value):
    from gan_segmentation_amd import main as cli
    with pytest.raises(ValueError, match="PAIR_STATS"):
        cli.main(["generate", "--config", _config(tmp_path, PAIR_STATS=value)])


def test_cli_accepts_the_key_and_its_default(tmp_path, no_models):
    from gan_segmentation_amd import main as cli
    for keys in ({}, {"PAIR_STATS": True}, {"PAIR_STATS": False}):
        with pytest.raises(_ModelLoaded):
            cli.main(["generate", "--config", _config(tmp_path, **keys)])
    assert "PAIR_STATS" in cli.__doc__


def test_writer_with_stats_refuses_a_numpy_batch(tmp_path):
    import inspect
    from gan_segmentation_amd.dataset_writer import DatasetWriter
    assert inspect.signature(DatasetWriter.__init__).parameters["stats"].default is False
    img, mask = np.zeros((1, 8, 8, 3), np.uint8), np.zeros((1, 8, 8), np.uint8)
    w = DatasetWriter(str(tmp_path / "on"), workers=1, stats=True)
    with pytest.raises(ValueError, match="no CPU path"):
        w.submit(img, mask, 0)
    assert w.close() == 0 and w.stats_path is None and os.listdir(str(tmp_path / "on")) == []
    # without the option a numpy batch is written as before, and no shard file appears
    with DatasetWriter(str(tmp_path / "off"), workers=1) as w:
        w.submit(img, mask, 0)
    assert sorted(os.listdir(str(tmp_path / "off"))) == ["img_000000.jpg", "mask_000000.png"]
