"""The image-guided mask refinement without a GPU (csrc/gsa_refine.h; mask_ops.refine_tables / refine / check_refine_*;
ImageGenerator(mask_refine=...); the MASK_REFINE* keys).

``rule_refine`` is the rule of the header restated in numpy -- one shifted-array step per tap, votes as int32 -- and what
tests/test_host_emu_refine.py and tests/test_gpu_refine.py hold every output byte to.  The hand cases below pin the rule itself,
the quality condition says what the default weights are good for."""
import numpy as np
import pytest

from tests.test_boundary_host import class_blobs
from tests.test_downscale_host import _ModelLoaded, _config, no_models  # noqa: F401  (no_models is a fixture)

MAX_RADIUS = 5
SIDE = 2 * MAX_RADIUS + 1
TABLE_BYTES = 256 + SIDE * SIDE


# -- the rule ------------------------------------------------------------------------------------------------------------------
def rule_refine(img, mask, tables, classes, radius, iterations=1, return_ties=False):
    """img (n, H, W, C) u8, mask (n, H, W) u8, tables (377,) u8 -> (n, H, W) u8 after ``iterations`` passes of the vote.
    ``return_ties``: also the pixels (of the last pass) that kept their value only by the tie rule -- a smaller class had as many votes."""
    img, mask, tables = np.asarray(img), np.asarray(mask), np.asarray(tables)
    assert img.dtype == mask.dtype == tables.dtype == np.uint8 and tables.shape == (TABLE_BYTES,)
    assert img.ndim == 4 and img.shape[:3] == mask.shape and 1 <= img.shape[3] <= 4 and 2 <= classes <= 8 and 1 <= radius <= MAX_RADIUS
    wr, ws = tables[:256].astype(np.int32), tables[256:].astype(np.int32).reshape(SIDE, SIDE)
    n, H, W = mask.shape
    colour = img.astype(np.int32)
    for _ in range(iterations):
        votes = np.zeros((classes, n, H, W), np.int32)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                if abs(dy) >= H or abs(dx) >= W:
                    continue                                            # no pixel has this neighbour inside its plane
                p = (slice(None), slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx)))
                q = (slice(None), slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx)))
                d = np.minimum(255, np.abs(colour[p] - colour[q]).sum(axis=-1))
                w = ws[dy + MAX_RADIUS, dx + MAX_RADIUS] * wr[d]
                u = mask[q]
                for c in range(classes):
                    votes[c][p] += np.where(u == c, w, 0)
        assert votes.max(initial=0) < 1 << 23
        best, first = votes.max(axis=0), votes.argmax(axis=0).astype(np.uint8)        # argmax: the smallest class among equals
        mine = np.take_along_axis(votes, np.minimum(mask, classes - 1)[None].astype(np.intp), axis=0)[0]
        frozen = mask >= classes
        ties = ~frozen & (mine == best) & (first != mask)
        mask = np.where(frozen | (mine == best), mask, first).astype(np.uint8)
    return (mask, ties) if return_ties else mask


def make_tables(wr, ws):
    """wr (256) and ws (11, 11) as the 377 bytes of the entry."""
    return np.concatenate([np.asarray(wr, np.uint8).reshape(256), np.asarray(ws, np.uint8).reshape(SIDE * SIDE)])


def flat_tables(radius=MAX_RADIUS, value=1):
    """Every colour distance and every offset inside the radius weighs the same: the plain window majority."""
    ws = np.zeros((SIDE, SIDE), np.uint8)
    ws[MAX_RADIUS - radius:MAX_RADIUS + radius + 1, MAX_RADIUS - radius:MAX_RADIUS + radius + 1] = value
    return make_tables(np.full(256, 1, np.uint8), ws)


def coarse_tables(seed=0):
    """Weights in a few steps -- wr 3 up to a distance of 24, 1 up to 96, 0 beyond; ws 2 within one pixel and 1 elsewhere, in ALL 121
    entries -- so that equal vote sums, and therefore the tie rule, come up often.  Entries outside a radius hold values too: a
    kernel that read them would differ from the rule."""
    d = np.arange(256)
    ws = np.ones((SIDE, SIDE), np.uint8)
    ws[MAX_RADIUS - 1:MAX_RADIUS + 2, MAX_RADIUS - 1:MAX_RADIUS + 2] = 2
    return make_tables(np.where(d <= 24, 3, np.where(d <= 96, 1, 0)), ws)


# -- the inputs of the kernel tests ------------------------------------------------------------------------------------------------
def region_image(seed, n, H, W, C, sd=6.0):
    """A few flat regions of random colours per sample plus Gaussian noise, rounded and clipped."""
    rng = np.random.default_rng([seed, 77])
    out = np.empty((n, H, W, C), np.uint8)
    for i in range(n):
        regions = class_blobs(seed + 31 * i + 5, (H, W), 4, sigma=3.0)
        palette = rng.integers(0, 256, (4, C))
        out[i] = np.clip(np.rint(palette[regions] + sd * rng.standard_normal((H, W, C))), 0, 255).astype(np.uint8)
    return out


def salted_blobs(seed, n, H, W, classes, salt=0.08, frozen=0.0):
    """Class blobs per sample with ``salt`` of the pixels replaced by a random class and ``frozen`` of them by 255 or ``classes``."""
    rng = np.random.default_rng([seed, 78])
    m = np.stack([class_blobs(seed + 17 * i, (H, W), classes, sigma=2.5) for i in range(n)]) if n else np.zeros((0, H, W), np.uint8)
    hit = rng.random(m.shape) < salt
    m[hit] = rng.integers(0, classes, int(hit.sum()))
    hit = rng.random(m.shape) < frozen
    m[hit] = rng.choice(np.array([255, classes], np.uint8), int(hit.sum()))
    return m


def every_value(seed, H, W, classes):
    """(1, H, W): salted class blobs in which a third of the pixels hold all 256 values in turn."""
    rng = np.random.default_rng([seed, 79])
    m = salted_blobs(seed, 1, H, W, classes)
    at = rng.permutation(H * W)[:max(256, H * W // 3)]
    m.reshape(-1)[at] = np.arange(len(at)) % 256
    assert len(np.unique(m)) == 256
    return m


def case(seed, n, H, W, C=3, classes=3, frozen=0.02):
    return region_image(seed, n, H, W, C), salted_blobs(seed, n, H, W, classes, frozen=frozen)


# -- hand cases ----------------------------------------------------------------------------------------------------------------
def _uniform(n, H, W, C=3, value=90):
    return np.full((n, H, W, C), value, np.uint8)


def test_a_tie_keeps_the_current_value():
    """1 x 2, [0, 1] on a uniform image: either pixel sees one vote for each class of the same weight and keeps its own."""
    mask = np.array([[[0, 1]]], np.uint8)
    for tables in (flat_tables(), coarse_tables()):
        out, ties = rule_refine(_uniform(1, 1, 2), mask, tables, 2, 1, return_ties=True)
        assert np.array_equal(out, mask)
        assert ties.tolist() == [[[False, True]]], "pixel 1 would have gone to class 0 without the tie rule"
    assert np.array_equal(rule_refine(_uniform(1, 1, 2), mask, _defaults(), 2, 1), mask), "the default centre weight outvotes one neighbour"


def test_the_smallest_class_takes_a_tie_the_current_value_is_not_part_of():
    """Flat weights on a uniform image.  The centre 3 of [1, 2, 3, 2, 1] (4 classes, radius 2) sees two votes each for 1 and 2 and one
    for itself: it takes 1, the smaller, whichever side each stands on.  The centre 0 of [2, 0, 1] ties with both and stays."""
    out = rule_refine(_uniform(1, 1, 5), np.array([[[1, 2, 3, 2, 1]]], np.uint8), flat_tables(), 4, 2)
    assert out[0, 0, 2] == 1
    out = rule_refine(_uniform(1, 1, 5), np.array([[[2, 1, 3, 1, 2]]], np.uint8), flat_tables(), 4, 2)
    assert out[0, 0, 2] == 1
    out = rule_refine(_uniform(1, 1, 3), np.array([[[2, 0, 1]]], np.uint8), flat_tables(), 3, 1)
    assert out[0, 0, 1] == 0


def test_all_zero_tables_are_the_identity():
    img, mask = case(1, 2, 20, 23, 3, 4)
    assert np.array_equal(rule_refine(img, mask, np.zeros(TABLE_BYTES, np.uint8), 4, 3), mask)


def test_a_constant_mask_stays_constant():
    img = region_image(2, 1, 24, 24, 3)
    for v in (0, 2, 7, 9, 255):
        mask = np.full((1, 24, 24), v, np.uint8)
        assert np.array_equal(rule_refine(img, mask, _defaults(), 8, 3), mask)


def test_labels_never_cross_an_edge_no_weight_crosses():
    """wr = [255, 0, 0, ...]: only pixels of exactly the same colour vote.  Two flat colours, a mask whose boundary lies 3 px off the
    colour edge: no pixel of the left colour ever takes a label that only the right colour holds."""
    img = np.zeros((1, 16, 20, 3), np.uint8)
    img[:, :, 10:] = (200, 10, 10)
    mask = np.zeros((1, 16, 20), np.uint8)
    mask[:, :, 10:] = 1
    mask[:, :, 7:10] = 2                                    # class 2 lives left of the edge only, class 1 right of it only
    tables = make_tables([255] + [0] * 255, flat_tables()[256:])
    out = mask
    for _ in range(4):
        out = rule_refine(img, out, tables, 3, 3)
        assert not (out[:, :, :10] == 1).any() and not (out[:, :, 10:] != 1).any()
    assert (out[:, :, :7] == 0).all(), "the majority of the left colour wins there"


def test_a_region_of_255_stays_and_casts_no_vote():
    img = _uniform(1, 9, 9)
    mask = np.full((1, 9, 9), 255, np.uint8)
    mask[0, 4, 4] = 1                                       # one class pixel in a sea of 255: its own vote is the only one
    mask[0, 4, 5] = 0
    out = rule_refine(img, mask, flat_tables(), 2, 4)
    assert (out[mask == 255] == 255).all()
    assert out[0, 4, 4] == 1 and out[0, 4, 5] == 0, "1 vote each: a tie, both keep their value; 255 would have outvoted them"
    mask[0, 3, 3:6] = 0
    out = rule_refine(img, mask, flat_tables(), 2, 4)
    assert out[0, 4, 4] == 0 and (out[mask == 255] == 255).all()
    # values K .. 254 are frozen as well, and K counts: with K = 3 the same 2s vote
    mask = np.array([[[2, 2, 0, 2, 2]]], np.uint8)
    assert rule_refine(_uniform(1, 1, 5), mask, flat_tables(), 2, 2).tolist() == mask.tolist()
    assert rule_refine(_uniform(1, 1, 5), mask, flat_tables(), 3, 2).tolist() == [[[2, 2, 2, 2, 2]]]


def test_two_samples_do_not_see_each_other():
    """All 0 above all 1 on a uniform image: the facing rows are not neighbours, nothing changes."""
    mask = np.zeros((2, 6, 7), np.uint8)
    mask[1] = 1
    for R in range(1, MAX_RADIUS + 1):
        assert np.array_equal(rule_refine(_uniform(2, 6, 7), mask, flat_tables(), 2, R), mask)
    # the same rows as ONE plane with a ragged lower half: there the upper rows do change
    one = mask.reshape(1, 12, 7).copy()
    one[0, 6:, ::2] = 0
    assert not np.array_equal(rule_refine(_uniform(1, 12, 7), one, flat_tables(), 2, 2)[0, 6:], one[0, 6:])


def test_flat_tables_on_a_uniform_image_give_the_window_majority():
    rng = np.random.default_rng(5)
    mask = rng.integers(0, 3, (1, 17, 19)).astype(np.uint8)
    R = 2
    out = rule_refine(_uniform(1, 17, 19, 1), mask, flat_tables(), 3, R)
    for y in range(17):
        for x in range(19):
            window = mask[0, max(0, y - R):y + R + 1, max(0, x - R):x + R + 1]
            counts = np.bincount(window.reshape(-1), minlength=3)
            v = mask[0, y, x]
            assert out[0, y, x] == (v if counts[v] == counts.max() else counts.argmax()), (y, x)


def test_entries_outside_the_radius_are_not_part_of_the_rule():
    img, mask = case(3, 1, 20, 21, 3, 3)
    inside = coarse_tables()
    for R in (1, 2, 4):
        trimmed = inside.copy()
        ws = trimmed[256:].reshape(SIDE, SIDE)
        keep = ws[MAX_RADIUS - R:MAX_RADIUS + R + 1, MAX_RADIUS - R:MAX_RADIUS + R + 1].copy()
        ws[:] = 0
        ws[MAX_RADIUS - R:MAX_RADIUS + R + 1, MAX_RADIUS - R:MAX_RADIUS + R + 1] = keep
        assert np.array_equal(rule_refine(img, mask, inside, 3, R), rule_refine(img, mask, trimmed, 3, R))


def test_the_distance_is_a_sum_over_channels_clamped_to_255():
    """Two pixels 100 apart in each of three channels are 255 apart (300 clamped), not 100: with wr[255] = 0 and wr[100] = 1 they do
    not vote for each other."""
    img = np.zeros((1, 1, 2, 3), np.uint8)
    img[0, 0, 1] = 100
    wr = np.zeros(256, np.uint8)
    wr[0], wr[100] = 1, 9
    tables = make_tables(wr, flat_tables()[256:])
    mask = np.array([[[0, 1]]], np.uint8)
    assert np.array_equal(rule_refine(img, mask, tables, 2, 1), mask)
    assert rule_refine(img[..., :1], mask, tables, 2, 1).tolist() == [[[1, 0]]], "one channel: d = 100, the neighbour outweighs the pixel"


# -- the tables ----------------------------------------------------------------------------------------------------------------
def _defaults(radius=3):
    from gan_segmentation_amd import mask_ops
    return mask_ops.refine_tables(radius)


@pytest.mark.parametrize("radius,sigma_space,sigma_colour", [(3, 2.0, 32.0), (1, 0.5, 4.0), (5, 10.0, 500.0), (2, 1.0, 0.1), (5, 0.3, 32.0)])
def test_refine_tables(radius, sigma_space, sigma_colour):
    from gan_segmentation_amd import mask_ops
    t = mask_ops.refine_tables(radius, sigma_space, sigma_colour)
    assert t.shape == (TABLE_BYTES,) and t.dtype == np.uint8 and TABLE_BYTES == mask_ops.REFINE_TABLE_BYTES == 377
    wr, ws = t[:256].astype(int), t[256:].astype(int).reshape(SIDE, SIDE)
    assert wr[0] == 255 and (np.diff(wr) <= 0).all()
    assert ws[MAX_RADIUS, MAX_RADIUS] == 255 and np.array_equal(ws, ws.T) and np.array_equal(ws, ws[::-1]) and np.array_equal(ws, ws[:, ::-1])
    o = np.abs(np.arange(-MAX_RADIUS, MAX_RADIUS + 1))
    inside = (o[:, None] <= radius) & (o[None, :] <= radius)
    assert (ws[inside] >= 1).all() and (ws[~inside] == 0).all()
    d = np.arange(256, dtype=np.float64)
    assert np.array_equal(wr, np.rint(255 * np.exp(-d * d / (2 * sigma_colour ** 2))).astype(int))
    assert ws[MAX_RADIUS + 1, MAX_RADIUS - 1] == max(1, int(np.rint(255 * np.exp(-2 / (2 * sigma_space ** 2)))))
    assert "SUM" in mask_ops.refine_tables.__doc__


def test_refine_tables_defaults():
    from gan_segmentation_amd import mask_ops
    assert np.array_equal(mask_ops.refine_tables(), mask_ops.refine_tables(3, 2.0, 32.0))
    assert 121 * 255 * 255 < 1 << 23


# -- the checks ----------------------------------------------------------------------------------------------------------------
def test_check_helpers_accept_and_reject():
    from gan_segmentation_amd import mask_ops
    assert mask_ops.check_refine_iterations(0) == 0 and mask_ops.check_refine_iterations(np.int64(8)) == 8
    assert mask_ops.check_refine_radius(1) == 1 and mask_ops.check_refine_radius(np.int32(5)) == 5
    assert mask_ops.check_refine_classes(2) == 2 and mask_ops.check_refine_classes(8) == 8
    assert mask_ops.check_refine_sigma(2) == 2.0 and mask_ops.check_refine_sigma(np.float32(0.5)) == 0.5
    assert all(type(f(np.int64(2))) is int for f in (mask_ops.check_refine_iterations, mask_ops.check_refine_radius, mask_ops.check_refine_classes))
    assert type(mask_ops.check_refine_sigma(3)) is float
    bad = {mask_ops.check_refine_iterations: (-1, 9, 1.0, "1", None, True), mask_ops.check_refine_radius: (0, 6, -1, 3.0, "3", None, True),
           mask_ops.check_refine_classes: (1, 9, 0, 2.0, "2", None, False), mask_ops.check_refine_sigma: (0, 0.0, -1.0, float("nan"), float("inf"), "2", None, True)}
    for fn, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match="named"):
                fn(v, "named")
    for kw in (dict(radius=0), dict(radius=6), dict(sigma_space=0), dict(sigma_colour=-2.0), dict(radius=True)):
        with pytest.raises(ValueError):
            mask_ops.refine_tables(**kw)


def test_refine_checks_its_tensors_before_any_gpu_work():
    import torch
    from gan_segmentation_amd import mask_ops
    for bad in (torch.zeros((4, 4), dtype=torch.uint8), np.zeros((4, 4), np.uint8), None):
        with pytest.raises(ValueError, match="mask"):
            mask_ops.refine(torch.zeros((4, 4, 3), dtype=torch.uint8), bad)


BAD_KEYWORDS = [("mask_refine", -1), ("mask_refine", 9), ("mask_refine", 1.0), ("mask_refine", "1"), ("mask_refine", True), ("mask_refine", None),
                ("mask_refine_radius", 0), ("mask_refine_radius", 6), ("mask_refine_radius", 3.0), ("mask_refine_radius", None),
                ("mask_refine_sigma_space", 0), ("mask_refine_sigma_space", "2"), ("mask_refine_sigma_space", None),
                ("mask_refine_sigma_colour", -1.0), ("mask_refine_sigma_colour", float("nan")), ("mask_refine_sigma_colour", True)]


@pytest.mark.parametrize("name,value", BAD_KEYWORDS)
def test_keywords_reject_bad_values_before_any_device_work(name, value):
    from gan_segmentation_amd import weights as W
    from gan_segmentation_amd.image_generator import ImageGenerator
    with pytest.raises(ValueError, match=name):
        getattr(ImageGenerator, "check_" + name)(value)
    with pytest.raises(ValueError, match=name):
        ImageGenerator.from_params(W.reduced_generator_config(7), {}, gpu_ids=[0], **{name: value})


def test_keywords_default_to_off():
    import inspect
    from gan_segmentation_amd.image_generator import ImageGenerator
    names = ("mask_refine", "mask_refine_radius", "mask_refine_sigma_space", "mask_refine_sigma_colour")
    assert tuple(getattr(ImageGenerator, k) for k in names) == (0, 3, 2.0, 32.0)
    for fn in (ImageGenerator.__init__, ImageGenerator.from_params, ImageGenerator._setup):
        p = inspect.signature(fn).parameters
        assert tuple(p[k].default for k in names) == (0, 3, 2.0, 32.0)


@pytest.mark.parametrize("key,value,name", [("MASK_REFINE", -1, "mask_refine"), ("MASK_REFINE", 9, "mask_refine"), ("MASK_REFINE", True, "mask_refine"),
                                            ("MASK_REFINE", "two", "mask_refine"), ("MASK_REFINE_RADIUS", 0, "mask_refine_radius"),
                                            ("MASK_REFINE_RADIUS", 6, "mask_refine_radius"), ("MASK_REFINE_SIGMA_SPACE", 0, "mask_refine_sigma_space"),
                                            ("MASK_REFINE_SIGMA_COLOUR", "wide", "mask_refine_sigma_colour")])
def test_cli_rejects_a_bad_key_before_loading_a_model(tmp_path, no_models, key, value, name):
    from gan_segmentation_amd import main as cli
    with pytest.raises(ValueError, match=name):
        cli.main(["generate", "--config", _config(tmp_path, **{key: value})])


def test_cli_accepts_the_keys_and_their_defaults(tmp_path, no_models):
    from gan_segmentation_amd import main as cli
    for keys in ({}, {"MASK_REFINE": 0}, {"MASK_REFINE": 1}, {"MASK_REFINE": 8, "MASK_REFINE_RADIUS": 5, "MASK_REFINE_SIGMA_SPACE": 3, "MASK_REFINE_SIGMA_COLOUR": 48.5},
                 {"MASK_REFINE": 2, "MASK_MORPH": True, "MASK_IGNORE_BAND": 2}):
        with pytest.raises(_ModelLoaded):
            cli.main(["generate", "--config", _config(tmp_path, **keys)])
    for key in ("MASK_REFINE", "MASK_REFINE_RADIUS", "MASK_REFINE_SIGMA_SPACE", "MASK_REFINE_SIGMA_COLOUR"):
        assert key in cli.__doc__


# -- what the default weights are good for ---------------------------------------------------------------------------------------
def _disc(cy, cx, r, side=96):
    yy, xx = np.mgrid[:side, :side]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_vote_moves_a_misplaced_noisy_boundary_onto_the_image_edge(seed):
    """96 x 96: the truth is a disc of radius 30 at (48, 40), (200, 60, 40) inside and (40, 90, 160) outside plus Gaussian noise of
    sd 12; the mask is the disc of radius 28 at (50, 43) with 5 % of the pixels flipped.  With the default tables one pass leaves at
    most 0.6 of the wrong pixels (measured with this restatement: 0.48 to 0.50 for the three seeds), the count never rises over
    four passes, and no wrong pixel remains farther than R + 4 px from both circles."""
    R = 3
    rng = np.random.default_rng(seed)
    truth = _disc(48, 40, 30)
    img = np.where(truth[..., None], (200, 60, 40), (40, 90, 160)) + 12.0 * rng.standard_normal((96, 96, 3))
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)[None]
    mask = _disc(50, 43, 28) ^ (rng.random((96, 96)) < 0.05)
    mask = mask.astype(np.uint8)[None]
    wrong = [int((mask[0] != truth).sum())]
    for _ in range(4):
        mask = rule_refine(img, mask, _defaults(R), 2, R)
        wrong.append(int((mask[0] != truth).sum()))
    print("seed %d: wrong pixels %s, ratio after one pass %.3f" % (seed, wrong, wrong[1] / wrong[0]))
    assert wrong[1] <= 0.6 * wrong[0]
    assert all(b <= a for a, b in zip(wrong, wrong[1:]))
    yy, xx = np.mgrid[:96, :96]
    near = np.zeros((96, 96), bool)
    for cy, cx, r in ((48, 40, 30), (50, 43, 28)):
        near |= np.abs(np.hypot(yy - cy, xx - cx) - r) <= R + 4
    assert not ((mask[0] != truth) & ~near).any()


# -- the shapes of the kernel tests (tests/test_host_emu_refine.py, tests/test_gpu_refine.py) ---------------------------------------------
THIN = [(1, 1), (1, 70), (70, 1)]
# the kernel's tile is 64 wide and 32 high: one pixel short of it, exactly it and one beyond, each way; three tiles across with W % 4 != 0
TILE_EDGES = [(31, 63), (32, 64), (33, 65), (31, 65), (33, 63), (34, 130)]


def expected(img, mask, tables, classes, radius, want_change=True, want_tie=True):
    """rule_refine of a kernel-test case, held to what makes it a test: the result differs from the input mask, and (with tables
    coarse enough for equal sums) at least one pixel kept its value by the tie rule alone."""
    want, ties = rule_refine(img, mask, tables, classes, radius, return_ties=True)
    if want_change:
        assert (want != mask).any(), "the case changes nothing"
    if want_tie:
        assert ties.any(), "no pixel of the case is kept by the tie rule"
    return want
