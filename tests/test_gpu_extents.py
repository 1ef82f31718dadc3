"""The stateless device ops at the limits they document (csrc/gsa_plane.h and the entries' headers): sides of 65535, batches that
take a second launch, the largest grid an entry accepts, and offsets past 2^31 and 2^32 -- the counterpart of
tests/test_gpu_large_batch.py for the ops without a context.

Family A runs two different planes of each long thin shape against the CPU rule the op's own GPU test uses, byte for byte.
Families B and C are too large for a CPU rule and use batch-position invariance (tests/extent_cases.py): D distinct base planes are
held to the CPU rule, the large batch is ``base[pattern]`` gathered on the device, and output i must be the bits of the base
batch's output ``pattern[i]`` -- every index, compared on the device in chunks; the inputs must come back unchanged.  The loss and
the score rows are bit-equal here by the library's own promise that a sample's result does not depend on its batch (loss_ops.py).
tests/test_extents_host.py asserts, without a GPU, that every pattern below keeps equal values apart at the splits and at the
planes an offset wraps to, that every split case splits and every case passes the thresholds it names, and that the method
rejects a wrapped offset, a launch that is not re-based and a row pointer that is not re-based.

entry                 A: 2 planes of (1,65535) (65535,1) (65535,4) (3,65535)     B                                        C: planes 256 x 256
morph_mask            all four                                                   grid: 2^24-1 planes of 3x4, 3x5          n 65539
boundary_distance,    all four, R 5 and 32                                       grid: 2^24-1 of 3x4, 3x5 (R 2)           n 65539, R 5 (+ dist2)
  ignore_band
components, despeckle all four, connectivity 4 and 8, rows, fill "neighbour"     split: 16386 of 65535x1 (c4), 65535x4 (c8)  n 65539, c8, rows
pair_stats            all four, C 0 and 3                                        split: 8194 of 65535x1 (C0), 65535x4 (C3)   n 65539, C 3
refine                all four, C 3, R 5, 2 passes                               grid: 2^24-1 of 3x4, 3x5 (C 3, R 5)      n 65539, C 3, R 5, 2 passes
compare               all four, band 0 and 3                                     split: 8194 of 65535x1, 65535x4, band 0, 3  n 65539, band 3;
                                                                                                                          rows: n 6628192 of 3x4
overlay               all four, factor 1 (65535 is odd: no other divides)        grid: 2^24-1 of 3x4, 3x5 (C 3, f 1)      n 65539, C 3, f 4 and 16
photometric           (4,65535) (65535,4), C 1 and 3                             --                                       n 21849, C 3, no noise
softmax_loss          --                                                         grid-y: n 65537, HW 1 4 7, K 2 3         n 32771, K 2, HW 65536
score_histogram       --                                                         grid-y: n 65537, HW 1 4 7, K 2 3         n 32771, K 2, HW 65536;
                                                                                                                          rows: n 1048579, K 2, HW 4

The photometric op draws its noise from the sample's index in the run, so a sample's output DOES depend on its position: family C
runs it with blur and colour on and the noise off (family A has the noise on).  The overlay's sheet holds fewer than 2^31 bytes by
its own rule, so in family C only its inputs pass 2^32.  The scores cannot pass 2^32 in logits and in row words at once within the
memory limit below (17 GB + 34 GB), so they get two batches.  The row tensors of components and pair_stats (20 and 88 words a plane)
stay far below 2^31 words in every case here: their entries re-base the rows per launch of fewer than 2^24 planes, so no product
inside a kernel gets there.  Compare's can (324 words a plane), and one more batch, 6628192 planes of 3 x 4, takes them past 2^31.

What each large case holds on the device at once (bytes, from the shapes; the base batch and chunk copies are below 0.2 GB):
  C morph 2 x 4.3 GB; C boundary 4.3 + 8.6 + 4.3 = 17 GB; C components 4.3 + 2 x 17.2 + 4.3 = 43 GB, the largest; C pair_stats
  12.9 + 4.3 = 17 GB; C refine 12.9 + 3 x 4.3 = 26 GB; C compare 2 x 4.3 + 2 x 8.6 = 26 GB and, rows, 17.2 GB; C overlay 12.9 + 4.3 + 0.8 = 18 GB;
  C photometric 2 x 4.3 GB; C loss 2 x 17.2 + 2.1 + 4.3 = 41 GB; C scores 17.2 + 2.1 + 1.1 = 20 GB and, rows, 34.4 GB;
  B components 65535x4: 4.3 + 2 x 17.2 + 4.3 = 43 GB, 65535x1 a quarter of it; B pair_stats 6.4 + 2.1 GB; B compare 2 x 2.1 + 2 x 4.3
  = 13 GB; B grids 0.2 to 1.4 GB; B grid-y 3.2 GB of score rows.
No case holds more than 48 GB, a sixth of the card; each frees what it held before the next (del, empty_cache).  A case that cannot
allocate fails.

Measured on an MI355X: the module's 88 cases take 27 to 28 s.  The slowest three: test_offsets_past_2_to_the_32[C-refine] 2.4 s
(most of it the CPU rule on its 7 base planes), test_scores_offsets_past_2_to_the_32 1.9 s (C-scores-K2; C-scores-rows-K2 took 3.4 s
in another run) and test_compare_rows_past_2_to_the_31 1.8 s.  DESIGN.md section 26 has the three edits that were tried against these tests and which test caught each."""
import collections
import functools
import gc

import numpy as np
import pytest

from tests import extent_cases as X
from tests import loss_ref
from tests.test_boundary_host import class_blobs, has_both, rule_band, rule_boundary
from tests.test_compare_host import rule_compare
from tests.test_components_host import oracle_components, rule_despeckle, rule_rows
from tests.test_mask_morph_host import rule_morph
from tests.test_pair_stats_host import rule_stats
from tests.test_photometric_host import random_images, rule_photometric
from tests.test_preview_host import random_lut, rule_overlay
from tests.test_refine_host import coarse_tables, region_image, rule_refine
from tests.test_scores_host import rule_scores

pytestmark = pytest.mark.gpu

C_LOSS = 2.0                                    # tests/test_gpu_loss.py's constant: rho = C_LOSS * 2**-24 against tests/loss_ref.bounds
MIN_AREA = 16
SIDE = 256                                      # family C's planes: 2^16 pixels, 16 tiles of 64 x 64, W % 4 == 0
TINY = [(3, 4), (3, 5)]                         # one-tile planes of the largest grids: the dword form and the byte form


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def masks(seed, n, H, W, classes=3):
    """(n, H, W) u8 with structure for the shape: thin planes by ``thin_masks``; planes of a few pixels random; larger planes class
    blobs (255 among them) with a few single pixels flipped."""
    if H * W <= 64:
        rng = np.random.default_rng([seed, H, W])
        return rng.integers(0, classes, (n, H, W)).astype(np.uint8)
    if min(H, W) <= 4:
        return X.thin_masks(seed, n, H, W, classes)
    rng = np.random.default_rng([seed, H, W, 1])
    m = np.stack([class_blobs(seed + 13 * i, (H, W), classes + 1, sigma=3.0, with255=True) for i in range(n)])
    hit = rng.random(m.shape) < 0.004
    m[hit] = rng.integers(0, classes, int(hit.sum()))
    return m


def images(seed, n, H, W, C):
    if min(H, W) <= 4 and H * W > 64:
        return X.thin_images(seed, n, H, W, C)
    if H * W <= 64:
        return np.random.default_rng([seed, H, W, C]).integers(0, 256, (n, H, W, C)).astype(np.uint8)
    return region_image(seed, n, H, W, C)


# ---- the ops: base inputs on the host, the call on the device, the CPU rule ----------------------------------------------------------
class Op:
    """batch: the names of the tensors that have a plane (or sample) per index; fixed: those every plane shares (tables)."""
    fixed = ()

    def __init__(self, **kw):
        self.kw = kw


class Morph(Op):
    unit, batch = "gsa_mask.hip", ("mask",)

    def inputs(self, seed, n, H, W):
        m = masks(seed, n, H, W)
        if H * W <= 64:
            m = (m * 16 + 1 + np.arange(n)[:, None, None]).astype(np.uint8)       # the closing leaves little of 15 pixels but their values
        return {"mask": m}

    def run(self, torch, t):
        from gan_segmentation_amd import mask_ops
        return {"out": mask_ops.morph_mask(t["mask"])}

    def rule(self, a):
        return {"out": rule_morph(a["mask"])}

    def elems(self, H, W):
        return (H * W,)


class Boundary(Op):
    unit, batch = "gsa_boundary.hip", ("mask",)

    def inputs(self, seed, n, H, W):
        if H * W > 64:
            return {"mask": masks(seed, n, H, W)}
        m = np.empty((n, H, W), np.uint8)       # a plane of a few pixels: one value and one pixel of another, at a place of its own
        for k in range(n):
            m[k] = k % 3
            m[k].reshape(-1)[(7 * k + 1) % (H * W)] = (k + 1) % 3
        return {"mask": m}

    def run(self, torch, t):
        from gan_segmentation_amd import mask_ops
        R = self.kw["R"]
        out, dist2 = mask_ops.ignore_band(t["mask"], R, 255, return_distance=True)
        res = {"out": out, "dist2": dist2}
        if self.kw.get("distance", True):
            res["distance"] = mask_ops.boundary_distance(t["mask"], R)
        return res

    def rule(self, a):
        R = self.kw["R"]
        d = rule_boundary(a["mask"], R)
        res = {"out": rule_band(a["mask"], R, 255, d), "dist2": d}
        if self.kw.get("distance", True):
            res["distance"] = d
        return res

    def elems(self, H, W):
        return (H * W,)


class Components(Op):
    unit, batch = "gsa_components.hip", ("mask",)

    def inputs(self, seed, n, H, W):
        return {"mask": masks(seed, n, H, W)}

    def run(self, torch, t):
        from gan_segmentation_amd import mask_ops
        m = t["mask"]
        scratch = (torch.full(m.shape, -7, dtype=torch.int32, device=m.device), torch.full(m.shape, 1 << 30, dtype=torch.int32, device=m.device))
        out, rows = mask_ops.despeckle(m, MIN_AREA, self.kw["connectivity"], "neighbour", return_stats=True, scratch=scratch)
        res = {"labels": scratch[0], "areas": scratch[1], "out": out, "rows": rows}
        if self.kw.get("components", False):                               # the other wrapper of the entry: no out, no rows
            res["labels2"], res["areas2"] = mask_ops.components(m, self.kw["connectivity"])
        return res

    def rule(self, a):
        c = self.kw["connectivity"]
        comps = oracle_components(a["mask"], c)
        res = {"labels": comps[0], "areas": comps[1], "out": rule_despeckle(a["mask"], MIN_AREA, c, -1, components=comps),
               "rows": rule_rows(a["mask"], MIN_AREA, c, components=comps)}
        if self.kw.get("components", False):
            res["labels2"], res["areas2"] = comps
        return res

    def elems(self, H, W):
        return (H * W, 20)


class PairStats(Op):
    unit = "gsa_stats.hip"

    @property
    def batch(self):
        return ("img", "mask") if self.kw["C"] else ("mask",)

    def inputs(self, seed, n, H, W):
        res = {"mask": masks(seed, n, H, W)}
        if self.kw["C"]:
            res["img"] = images(seed, n, H, W, self.kw["C"])
        return res

    def run(self, torch, t):
        from gan_segmentation_amd import pair_stats
        return {"rows": pair_stats.pair_stats(t.get("img"), t["mask"])}

    def rule(self, a):
        return {"rows": rule_stats(a.get("img"), a["mask"])}

    def elems(self, H, W):
        return (H * W, 88) + ((H * W * self.kw["C"],) if self.kw["C"] else ())


class Refine(Op):
    unit, batch, fixed = "gsa_refine.hip", ("img", "mask"), ("tables",)
    K, R, PASSES, C = 3, 5, 2, 3

    def inputs(self, seed, n, H, W):
        m = masks(seed, n, H, W, self.K)
        return {"img": images(seed, n, H, W, self.C), "mask": m, "tables": coarse_tables()}

    def run(self, torch, t):
        from gan_segmentation_amd import mask_ops
        return {"out": mask_ops.refine(t["img"], t["mask"], iterations=self.PASSES, radius=self.R, classes=self.K, tables=t["tables"])}

    def rule(self, a):
        return {"out": rule_refine(a["img"], a["mask"], a["tables"], self.K, self.R, iterations=self.PASSES)}

    def elems(self, H, W):
        return (H * W, H * W * self.C)


class Compare(Op):
    unit, batch = "gsa_compare.hip", ("pred", "target")

    def inputs(self, seed, n, H, W):
        return {"pred": masks(seed + 1000, n, H, W), "target": masks(seed, n, H, W)}

    def run(self, torch, t):
        from gan_segmentation_amd import mask_ops
        return {"rows": mask_ops.compare(t["pred"], t["target"], self.kw["band"])}

    def rule(self, a):
        return {"rows": rule_compare(a["target"], a["pred"], self.kw["band"])}

    def elems(self, H, W):
        return (H * W, 324)


class Overlay(Op):
    unit, batch, fixed = "gsa_overlay.hip", ("img", "mask"), ("lut",)
    C = 3

    def inputs(self, seed, n, H, W):
        return {"img": images(seed, n, H, W, self.C), "mask": masks(seed, n, H, W), "lut": random_lut(seed)}

    def run(self, torch, t):
        from gan_segmentation_amd import preview
        return {"out%d" % f: preview.overlay(t["img"], t["mask"], t["lut"], f) for f in self.kw["factors"]}

    def rule(self, a):
        n, H, W, C = a["img"].shape
        return {"out%d" % f: rule_overlay(a["img"], a["mask"], a["lut"], f).reshape(n, H // f, W // f, C) for f in self.kw["factors"]}

    def elems(self, H, W):
        return (H * W, H * W * self.C) + tuple(H // f * (W // f) * self.C for f in self.kw["factors"])


class Photometric(Op):
    unit, batch = None, ("img", "params")
    SEED, FIRST = 7, 1000

    def inputs(self, seed, n, H, W):
        from tests.test_gpu_photometric import _rows
        rows = _rows(n, self.SEED, self.FIRST)
        if not self.kw["noise"]:
            rows[:, 5] = 0.0
        return {"img": random_images(seed, n, H, W, self.kw["C"]), "params": rows}

    def run(self, torch, t):
        from gan_segmentation_amd import photometric
        return {"out": photometric.photometric(t["img"], t["params"], self.SEED, self.FIRST)}

    def rule(self, a):
        return {"out": rule_photometric(a["img"], a["params"], self.SEED, self.FIRST)}

    def elems(self, H, W):
        return (H * W * self.kw["C"], 16)


OPS_A = [("morph", Morph()), ("boundary-R5", Boundary(R=5)), ("boundary-R32", Boundary(R=32)),
         ("components-c4", Components(connectivity=4, components=True)), ("components-c8", Components(connectivity=8, components=True)),
         ("pair_stats-C0", PairStats(C=0)), ("pair_stats-C3", PairStats(C=3)), ("refine", Refine()), ("compare-band0", Compare(band=0)),
         ("compare-band3", Compare(band=3)), ("overlay", Overlay(factors=(1,)))]


# ---- the steps ---------------------------------------------------------------------------------------------------------------------
def _device(torch, arrays):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in arrays.items()}


def _free(torch):
    gc.collect()
    torch.cuda.empty_cache()


def _hold_to_rule(torch, op, host, what):
    """The op on ``host``'s arrays against the CPU rule, every element; the inputs unchanged.  -> (device inputs, device outputs)."""
    dev = _device(torch, host)
    got, want = op.run(torch, dev), op.rule(host)
    torch.cuda.synchronize()
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        g, w = got[k].cpu().numpy(), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, "%s %s: %s %s vs %s %s" % (what, k, g.shape, g.dtype, w.shape, w.dtype)
        bad = g != w
        assert not bad.any(), "%s %s: %d of %d values differ from the rule, first at %s: %s instead of %s" % (
            what, k, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), g[bad][0], w[bad][0])
    for k, v in host.items():
        assert np.array_equal(dev[k].cpu().numpy(), v), "%s: the input %s was written to" % (what, k)
    return dev, got


Case = collections.namedtuple("Case", "name op shape n D seed per_launch launches split_at elems passes device_bytes unit")


def _case(name, op, shape, n, D, per_launch=None, passes=(), device_bytes=0, seed=11):
    per_launch = per_launch or n
    return Case(name, op, shape, n, D, seed, per_launch, len(X.launches(n, per_launch)), X.splits(n, per_launch), op.elems(*shape), tuple(passes),
                device_bytes, op.unit)


def _large(torch, case):
    """The method of the module docstring for one case."""
    op, (H, W) = case.op, case.shape
    host = op.inputs(case.seed, case.D, H, W)
    base_in, base_out = _hold_to_rule(torch, op, host, case.name + " base")
    for k in op.batch:
        X.assert_distinct(torch, base_in[k], case.name + " input " + k)
    for k, v in base_out.items():
        X.assert_distinct(torch, v, case.name + " output " + k)
    p = X.make_pattern(case.n, case.D, case.seed, case.split_at, case.elems)
    pattern = torch.from_numpy(np.array(p)).cuda()
    big = {k: (base_in[k].index_select(0, pattern) if k in op.batch else base_in[k]) for k in base_in}
    out = op.run(torch, big)
    torch.cuda.synchronize()
    for k in sorted(out):
        X.assert_gathered(torch, out[k], base_out[k], pattern, "%s %s" % (case.name, k))
    for k in op.batch:
        X.assert_gathered(torch, big[k], base_in[k], pattern, "%s: the input %s" % (case.name, k))
    for k in op.fixed:
        assert np.array_equal(big[k].cpu().numpy(), host[k]), "%s: %s was written to" % (case.name, k)
    return big


@pytest.fixture(autouse=True)
def _release(torch_cuda):
    yield
    _free(torch_cuda)


# ---- family A: long thin planes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", X.LONG_THIN, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name,op", OPS_A, ids=[name for name, _op in OPS_A])
def test_long_thin_planes(torch_cuda, name, op, shape):
    """Two different planes a shape: one tile column of 1024 or 2048 tile rows and its transpose, in the byte form and (65535 x 4)
    the dword form.  The expected band holds FAR and band pixels; the components cross the seams (more pixels than a tile holds)."""
    H, W = shape
    host = op.inputs(5 + H % 7, 2, H, W)
    _dev, got = _hold_to_rule(torch_cuda, op, host, "%s %s" % (name, shape))
    if isinstance(op, Boundary):
        assert has_both(got["dist2"].cpu().numpy())
    if isinstance(op, Components):
        areas = got["areas"].cpu().numpy()
        assert areas.max() > 64 * min(H, W, 64) and (areas < MIN_AREA).any(), "components beyond a tile, and specks to remove"
    if isinstance(op, Refine):
        assert not np.array_equal(got["out"].cpu().numpy(), host["mask"]), "the vote changed nothing"


@pytest.mark.parametrize("shape", X.PHOTOMETRIC_THIN, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("C", [1, 3])
def test_long_thin_planes_photometric(torch_cuda, C, shape):
    """The photometric op at its smallest short side, 4: every vertical (or horizontal) tap but the centre's is a reflection."""
    op = Photometric(C=C, noise=True)
    host = op.inputs(3, 2, *shape)
    _dev, got = _hold_to_rule(torch_cuda, op, host, "photometric C %d %s" % (C, shape))
    assert not np.array_equal(got["out"].cpu().numpy(), host["img"])


# ---- family B: every split -----------------------------------------------------------------------------------------------------------
def _split_case(name, op, shape, blocks, D):
    per = X.planes_per_launch(blocks(*shape))
    return _case("B-%s-%dx%d" % ((name,) + shape), op, shape, per + 3, D, per_launch=per)


SPLIT_CASES = [
    _split_case("components-c4", Components(connectivity=4), (65535, 1), X.components_blocks, 5),
    _split_case("components-c8", Components(connectivity=8), (65535, 4), X.components_blocks, 5),
    _split_case("pair_stats-C0", PairStats(C=0), (65535, 1), X.stats_blocks, 5),
    _split_case("pair_stats-C3", PairStats(C=3), (65535, 4), X.stats_blocks, 9),
    _split_case("compare-band0", Compare(band=0), (65535, 1), X.compare_blocks, 5),
    _split_case("compare-band3", Compare(band=3), (65535, 1), X.compare_blocks, 5),
    _split_case("compare-band0", Compare(band=0), (65535, 4), X.compare_blocks, 5),
    _split_case("compare-band3", Compare(band=3), (65535, 4), X.compare_blocks, 5),
]


@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: c.name)
def test_a_batch_of_several_launches(torch_cuda, case):
    """for_each_launch's second iteration: the entry's own rule gives two launches, the second of three planes."""
    assert case.launches == 2 and case.n - case.split_at[0] == 3
    _large(torch_cuda, case)


# ---- family B: the largest accepted grid ---------------------------------------------------------------------------------------------
GRID_CASES = [_case("B-grid-%s-%dx%d" % ((name,) + shape), op, shape, X.MAX_WORKGROUPS - 1, 5)
              for shape in TINY
              for name, op in (("morph", Morph()), ("ignore_band", Boundary(R=2, distance=False)), ("refine", Refine()), ("overlay", Overlay(factors=(1,))))]


@pytest.mark.parametrize("case", GRID_CASES, ids=lambda c: c.name)
def test_the_largest_grid_and_one_plane_more(torch_cuda, case):
    """2^24 - 1 one-tile planes run; the same call with one plane more raises."""
    from gan_segmentation_amd import _lib
    torch = torch_cuda
    assert X.tiles_per_plane(case.unit, *case.shape) == 1 and case.n == X.largest_grid(case.unit, *case.shape)
    big = _large(torch, case)
    more = {k: (torch.cat([v, v[:1]]) if k in case.op.batch else v) for k, v in big.items()}
    del big
    with pytest.raises(_lib.GsaError):
        case.op.run(torch, more)


# ---- the loss and the scores -----------------------------------------------------------------------------------------------------------
NORMS = ("mean", "valid", "focal")


@functools.lru_cache(maxsize=None)
def _samples(D, K, HW, seed=0):
    """(logits (D, K, HW) fp32, labels (D, HW) int8, dist2 (D, HW) int16, cw (K,), table) on the host, as tests/test_gpu_loss.py draws
    them, but logits of a spread that leaves the softmax unsaturated in places; a fifth of the labels ignored.  No sample is all
    ignored: every sample has a result of its own."""
    import torch
    from gan_segmentation_amd import loss_ops
    g = torch.Generator().manual_seed(100000 * seed + 1000 * K + HW)
    logits = torch.randn(D, K, HW, generator=g) * 4
    labels = torch.randint(0, K, (D, HW), generator=g)
    ignored = torch.rand(D, HW, generator=g) < 0.2
    ignored[:, 0] = False
    labels[ignored] = torch.tensor([-1, -128, 127, K])[torch.randint(0, 4, (int(ignored.sum()),), generator=g)]
    d2 = torch.randint(1, 1026, (D, HW), generator=g)
    d2[d2 == 1025] = 32767
    cw = torch.rand(K, generator=g) * 3.75 + 0.25
    table = torch.from_numpy(loss_ops.boundary_weight_table(32, 4.0, 12.0))
    return logits, labels.to(torch.int8), d2.to(torch.int16), cw, table


def _loss(torch, logits, labels, d2, cw, table, norm, weighted, grad):
    from gan_segmentation_amd import loss_ops
    extra = dict(class_weights=cw, dist2=d2, table=table) if weighted else {}
    loss, sums, dl = loss_ops.softmax_loss(logits, labels, gamma=2.0, normalise=norm, grad=grad, grad_scale=0.5, **extra)
    res = {"loss": loss, "sums": sums}
    if grad:
        res["dlogits"] = dl
    return res


def _loss_case(torch, D, K, HW, n, split_at, modes, what):
    """The base samples against tests/loss_ref.py within test_gpu_loss's bounds, then the batch of n against the base, bit for bit."""
    from tests import f64_ref as R
    host = _samples(D, K, HW)
    logits, labels, d2, cw, table = (t.cuda() for t in host)
    elems = (K * HW, HW, 4, 1)
    pattern = torch.from_numpy(np.array(X.make_pattern(n, D, 11, split_at, elems))).cuda()
    big_z, big_y, big_d = logits.index_select(0, pattern), labels.index_select(0, pattern), d2.index_select(0, pattern)
    X.assert_distinct(torch, logits, what + " logits")
    rho = C_LOSS * R.U
    for norm, weighted, grad in modes:
        mode = "%s %s %s %s" % (what, norm, "weighted" if weighted else "plain", "grad" if grad else "forward")
        base = _loss(torch, logits, labels, d2, cw, table, norm, weighted, grad)
        kw = dict(cw=host[3] if weighted else None, d2=host[2] if weighted else None, tab=host[4] if weighted else None, gamma=2.0,
                  normalise=NORMS.index(norm), grad_scale=0.5)
        lref, sref, dref = loss_ref.loss_f64(host[0], host[1], **kw)
        bnd = loss_ref.bounds(host[0], host[1], rho=rho, **kw)
        R.assert_bounded(base["sums"].cpu(), sref, bnd["sums"], rho, mode + ": sums")
        R.assert_bounded(base["loss"].cpu(), lref, bnd["loss"], rho, mode + ": loss")
        if grad:
            R.assert_bounded(base["dlogits"].cpu(), dref, bnd["dlogits"], rho, mode + ": dlogits")
        X.assert_distinct(torch, base["sums"], mode + " sums")
        got = _loss(torch, big_z, big_y, big_d, cw, table, norm, weighted, grad)
        torch.cuda.synchronize()
        for k in sorted(got):
            X.assert_gathered(torch, got[k], base[k], pattern, "%s %s" % (mode, k))
        del got, base
    for big, small, k in ((big_z, logits, "logits"), (big_y, labels, "labels"), (big_d, d2, "dist2")):
        X.assert_gathered(torch, big, small, pattern, "%s: the input %s" % (what, k))
    for t, h, k in ((cw, host[3], "class_weights"), (table, host[4], "table")):
        assert torch.equal(t.cpu(), h), "%s: %s was written to" % (what, k)


def _scores_case(torch, D, K, HW, n, split_at, shift, what):
    from gan_segmentation_amd import score_ops
    z, y = _samples(D, K, HW, seed=1)[:2]
    want = rule_scores(z.numpy(), y.numpy(), shift)
    logits, labels = z.cuda(), y.cuda()
    base = score_ops.score_histogram(logits, labels, shift)
    bad = np.argwhere(base.cpu().numpy() != want)
    assert not len(bad), "%s base: %d words differ from the rule, the first at %s" % (what, len(bad), bad[0])
    X.assert_distinct(torch, base, what + " rows")
    elems = (K * HW, HW, K * 2048)
    pattern = torch.from_numpy(np.array(X.make_pattern(n, D, 11, split_at, elems))).cuda()
    big_z, big_y = logits.index_select(0, pattern), labels.index_select(0, pattern)
    out = torch.full((n, K, 2, 1024), -7, dtype=torch.int64, device="cuda")
    assert score_ops.score_histogram(big_z, big_y, shift, out=out) is out
    torch.cuda.synchronize()
    X.assert_gathered(torch, out, base, pattern, what + " rows")
    X.assert_gathered(torch, big_z, logits, pattern, what + ": the input logits")
    X.assert_gathered(torch, big_y, labels, pattern, what + ": the input labels")


LossCase = collections.namedtuple("LossCase", "name n D seed K HW per_launch launches split_at elems passes device_bytes")


def _sample_case(name, kind, n, K, HW, passes=(), device_bytes=0, D=5):
    elems = (K * HW, HW, 4, 1) if kind == "loss" else (K * HW, HW, K * 2048)
    return LossCase(name, n, D, 11, K, HW, X.MAX_GRID_Y, len(X.launches(n, X.MAX_GRID_Y)), X.splits(n, X.MAX_GRID_Y), elems, tuple(passes),
                    device_bytes)


GRID_Y_SHAPES = [(HW, K) for HW in (1, 4, 7) for K in (2, 3)]
GRID_Y_CASES = ([_sample_case("B-gridy-loss-HW%d-K%d" % s, "loss", X.MAX_GRID_Y + 2, s[1], s[0]) for s in GRID_Y_SHAPES] +
                [_sample_case("B-gridy-scores-HW%d-K%d" % s, "scores", X.MAX_GRID_Y + 2, s[1], s[0]) for s in GRID_Y_SHAPES])
LOSS_MODES = [(norm, weighted, grad) for norm in NORMS for weighted in (False, True) for grad in (False, True)]


@pytest.mark.parametrize("case", GRID_Y_CASES[:len(GRID_Y_SHAPES)], ids=lambda c: c.name)
def test_loss_past_the_grid_y_split(torch_cuda, case):
    """n = 65535 + 2: the second launch re-bases logits, labels, dist2, workspace, sums, loss and dlogits by 65535 samples of HW = 1
    (any alignment), 4 (aligned) and 7 (odd); with and without dist2 and dlogits, in all three normalisers."""
    assert case.launches == 2 and case.split_at == (X.MAX_GRID_Y,)
    _loss_case(torch_cuda, case.D, case.K, case.HW, case.n, case.split_at, LOSS_MODES, case.name)


@pytest.mark.parametrize("case", GRID_Y_CASES[len(GRID_Y_SHAPES):], ids=lambda c: c.name)
def test_scores_past_the_grid_y_split(torch_cuda, case):
    """The same split of gsa_score_histogram; the aligned form (HW = 4) is chosen once, before the loop.  2 to 3 GiB of rows."""
    assert case.launches == 2 and case.split_at == (X.MAX_GRID_Y,)
    _scores_case(torch_cuda, case.D, case.K, case.HW, case.n, case.split_at, 5, case.name)


# ---- family C: offsets past 2^31 and 2^32 ----------------------------------------------------------------------------------------------
PX = SIDE * SIDE
N_U8 = (1 << 32) // PX + 3                      # 65539 planes: 3 planes past 2^32 bytes of mask
N_RGB = (1 << 32) // (3 * PX) + 4               # 21849 samples: past 2^32 bytes of a 3-channel image
N_LOGITS = (1 << 32) // (2 * PX) + 3            # 32771 samples of 2 classes: past 2^32 logits, past 2^31 labels
N_ROWS = (1 << 32) // (2 * 2048) + 3            # 1048579 samples of 2 classes: past 2^32 row words
P31, P32 = 1 << 31, 1 << 32
GB = N_U8 * PX


def _c(name, op, D, n=N_U8, passes=(), device_bytes=0):
    return _case("C-" + name, op, (SIDE, SIDE), n, D, passes=passes, device_bytes=device_bytes)


C_CASES = [
    _c("morph", Morph(), 5, passes=[(PX, P32)], device_bytes=2 * GB),
    _c("boundary-R5", Boundary(R=5, distance=False), 5, passes=[(PX, P32)], device_bytes=4 * GB),
    _c("components-c8", Components(connectivity=8), 5, passes=[(PX, P32)], device_bytes=10 * GB + N_U8 * 160),
    _c("pair_stats-C3", PairStats(C=3), 7, passes=[(PX, P32), (3 * PX, P32)], device_bytes=4 * GB),
    _c("refine", Refine(), 7, passes=[(PX, P32), (3 * PX, P32)], device_bytes=6 * GB),
    _c("compare-band3", Compare(band=3), 5, passes=[(PX, P32)], device_bytes=6 * GB),
    _c("overlay-f4-f16", Overlay(factors=(4, 16)), 7, passes=[(PX, P32), (3 * PX, P32)], device_bytes=4 * GB + N_U8 * 3 * (64 * 64 + 16 * 16)),
    _c("photometric-C3", Photometric(C=3, noise=False), 5, n=N_RGB, passes=[(3 * PX, P32)], device_bytes=2 * N_RGB * 3 * PX),
]
C_SAMPLE_CASES = [
    _sample_case("C-loss-K2", "loss", N_LOGITS, 2, PX, passes=[(2 * PX, P32), (PX, P31)], device_bytes=N_LOGITS * PX * (8 + 8 + 1 + 2)),
    _sample_case("C-scores-K2", "scores", N_LOGITS, 2, PX, passes=[(2 * PX, P32), (PX, P31)], device_bytes=N_LOGITS * (PX * 9 + 4096 * 8)),
    _sample_case("C-scores-rows-K2", "scores", N_ROWS, 2, 4, passes=[(4096, P32)], device_bytes=N_ROWS * (4 * 9 + 4096 * 8)),
]
N_COMPARE_ROWS = P31 // 324 + 3                 # 6628192 planes: past 2^31 words of compare rows inside ONE launch
COMPARE_ROWS_CASE = _case("C-compare-rows-band3", Compare(band=3), TINY[0], N_COMPARE_ROWS, 5, passes=[(324, P31)],
                          device_bytes=N_COMPARE_ROWS * (324 * 8 + 12 * 6))
ALL_LARGE_CASES = SPLIT_CASES + GRID_CASES + GRID_Y_CASES + C_CASES + [COMPARE_ROWS_CASE] + C_SAMPLE_CASES


@pytest.mark.parametrize("case", C_CASES, ids=lambda c: c.name)
def test_offsets_past_2_to_the_32(torch_cuda, case):
    """More than 2^32 bytes of mask (and of image): every (size_t)plane * H * W, in bytes and in int16 and int32 elements."""
    assert case.n * case.elems[0] > P32
    _large(torch_cuda, case)


def test_compare_rows_past_2_to_the_31(torch_cuda):
    """6.6 million one-tile planes in one launch: the workgroup of plane p adds into rows + p * 324, a product past 2^31 for the
    last 3 planes -- the one row index of the plane units that leaves 31 bits inside a kernel (pair_stats and components re-base
    their rows per launch of fewer than 2^24 planes of 88 and 20 words)."""
    case = COMPARE_ROWS_CASE
    assert case.launches == 1 and (case.n - 1) * 324 > P31 and X.planes_per_launch(X.compare_blocks(*case.shape)) >= case.n
    _large(torch_cuda, case)


def test_loss_offsets_past_2_to_the_32(torch_cuda):
    """More than 2^32 logits and gradients, more than 2^31 labels and distances: n * a.K * HW and n * HW in the loss kernels."""
    case = C_SAMPLE_CASES[0]
    assert case.n * case.K * case.HW > P32 and case.n * case.HW > P31 and case.launches == 1
    _loss_case(torch_cuda, case.D, case.K, case.HW, case.n, case.split_at, [("focal", True, True)], case.name)


@pytest.mark.parametrize("case", C_SAMPLE_CASES[1:], ids=lambda c: c.name)
def test_scores_offsets_past_2_to_the_32(torch_cuda, case):
    """More than 2^32 logits in one batch; more than 2^32 row words (17 launches, every row pointer re-based) in the other."""
    assert max(case.n * e for e in case.elems) > P32
    _scores_case(torch_cuda, case.D, case.K, case.HW, case.n, case.split_at, 5, case.name)
