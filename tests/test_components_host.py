"""The mask components without a GPU (include/gsa_components.h; mask_ops.components / despeckle; ImageGenerator(mask_min_area=...);
the MASK_MIN_AREA, MASK_CONNECTIVITY and MASK_FILL keys).

``rule_components(m, connectivity)`` is the canonical rule: a plain raster union-find over pixels of equal raw value.  It is the
definition.  ``rule_despeckle`` and ``rule_rows`` are written from the header's text.  The rule is PINNED here, with zero differences
allowed, against
* a scipy.ndimage.label form (per value; ndimage.minimum of the raster index per label; bincount areas),
* a committed fixture (tests/golden/mask_components.npz), which holds without scipy.
The GPU tests (tests/test_gpu_components.py) hold the kernels to this rule over every pixel and every row word.  Also here: hand
cases, the header's one entry and its macros, the entry's argument checks and the validation of the keywords and the keys."""
import os

import numpy as np
import pytest

from tests.test_downscale_host import _ModelLoaded, _config, no_models  # noqa: F401  (no_models is a fixture)
from tests.test_mask_morph_host import KINDS, blobs, make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SLOTS, NCOMP, LARGEST, SMALL, SMALL_PIXELS, ROW = 9, 0, 9, 18, 19, 20


# -- the rule ------------------------------------------------------------------------------------------------------------------
def _plane_components(m, connectivity):
    H, W = m.shape
    flat = m.reshape(-1).tolist()
    parent = list(range(H * W))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    steps = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if connectivity == 8 else [])
    for y in range(H):
        for x in range(W):
            p = y * W + x
            for dy, dx in steps:
                yy, xx = y + dy, x + dx
                if yy >= 0 and 0 <= xx < W and flat[yy * W + xx] == flat[p]:
                    a, b = find(p), find(yy * W + xx)
                    if a != b:
                        parent[max(a, b)] = min(a, b)       # the smaller raster index stays the root
    labels = np.array([find(p) for p in range(H * W)], np.int64)
    areas = np.bincount(labels, minlength=H * W)[labels]
    return labels.reshape(H, W).astype(np.int32), areas.reshape(H, W).astype(np.int32)


def _per_plane(fn, m, *args):
    m = np.asarray(m)
    assert m.dtype == np.uint8 and m.ndim in (2, 3)
    if m.ndim == 2:
        return fn(m, *args)
    parts = [fn(plane, *args) for plane in m]
    if not parts:
        return None
    return tuple(np.stack(c) for c in zip(*parts)) if isinstance(parts[0], tuple) else np.stack(parts)


def rule_components(m, connectivity=8):
    """(H, W) or (n, H, W) u8 -> (labels, areas) int32 of the same shape: the smallest raster index y * W + x of every pixel's
    component of equal raw value, and that component's pixel count; every image of a batch on its own."""
    assert connectivity in (4, 8)
    m = np.asarray(m)
    if m.ndim == 3 and m.shape[0] == 0:
        return np.zeros(m.shape, np.int32), np.zeros(m.shape, np.int32)
    return _per_plane(_plane_components, m, connectivity)


def scipy_components(m, connectivity=8):
    """The same by scipy.ndimage.label, value by value."""
    from scipy import ndimage as ndi

    def plane(a):
        H, W = a.shape
        idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
        structure = np.ones((3, 3), int) if connectivity == 8 else ndi.generate_binary_structure(2, 1)
        labels = np.zeros((H, W), np.int64)
        areas = np.zeros((H, W), np.int64)
        for v in np.unique(a):
            lab, k = ndi.label(a == v, structure=structure)
            first = np.asarray(ndi.minimum(idx, lab, index=np.arange(1, k + 1)), np.int64)
            count = np.bincount(lab.reshape(-1), minlength=k + 1)
            on = lab > 0
            labels[on] = first[lab[on] - 1]
            areas[on] = count[lab[on]]
        return labels.astype(np.int32), areas.astype(np.int32)
    return _per_plane(plane, m)


def oracle_components(m, connectivity=8):
    """The scipy form when scipy is importable, the loop otherwise: pinned equal below."""
    try:
        import scipy.ndimage  # noqa: F401
    except ImportError:
        return rule_components(m, connectivity)
    m = np.asarray(m)
    if m.ndim == 3 and m.shape[0] == 0:
        return rule_components(m, connectivity)
    return scipy_components(m, connectivity)


def rule_despeckle(m, min_area, connectivity=8, fill=-1, components=None):
    """out of the header's text: mask[p] where areas[p] >= min_area; else fill (0..255); else (fill = -1, "neighbour") the input
    value left of the component's first pixel, above it if that is in column 0, and mask[p] for the component that holds (0, 0)."""
    def plane(a, labels, areas):
        H, W = a.shape
        flat = a.reshape(-1)
        r = labels.reshape(-1).astype(np.int64)
        small = areas.reshape(-1) < min_area
        if fill >= 0:
            repl = np.full(H * W, fill, np.uint8)
        else:
            repl = np.where(r % W != 0, flat[np.maximum(r - 1, 0)], np.where(r >= W, flat[np.maximum(r - W, 0)], flat))
        return np.where(small, repl, flat).astype(np.uint8).reshape(H, W)
    m = np.asarray(m)
    labels, areas = components if components is not None else oracle_components(m, connectivity)
    if m.ndim == 2:
        return plane(m, labels, areas)
    return np.stack([plane(a, lab, ar) for a, lab, ar in zip(m, labels, areas)]) if len(m) else m.copy()


def rule_rows(m, min_area, connectivity=8, components=None):
    """(n, 20) int64 ((20,) for a plane): component counts and largest areas per slot, then the small components and their pixels."""
    def plane(a, labels, areas):
        H, W = a.shape
        row = np.zeros(ROW, np.int64)
        roots = np.flatnonzero(labels.reshape(-1) == np.arange(H * W))
        for p in roots:
            s, area = min(int(a.reshape(-1)[p]), 8), int(areas.reshape(-1)[p])
            row[NCOMP + s] += 1
            row[LARGEST + s] = max(row[LARGEST + s], area)
            if area < min_area:
                row[SMALL] += 1
                row[SMALL_PIXELS] += area
        return row
    m = np.asarray(m)
    labels, areas = components if components is not None else oracle_components(m, connectivity)
    if m.ndim == 2:
        return plane(m, labels, areas)
    return np.stack([plane(a, lab, ar) for a, lab, ar in zip(m, labels, areas)]) if len(m) else np.zeros((0, ROW), np.int64)


# -- the inputs: beside the KINDS of the morphology tests, patterns that are hard on a tiled union-find --------------------------
def serpentine(shape):
    """A one-pixel snake of ones over the whole image: full even rows, joined at alternating ends through the odd rows.  One
    component that crosses every tile seam many times, with the longest label chains; the zeros are one run per odd row."""
    m = np.zeros(shape, np.uint8)
    m[..., 0::2, :] = 1
    m[..., 1::4, -1] = 1
    m[..., 3::4, 0] = 1
    return m


def spiral(shape):
    """Rings of ones at insets 0, 2, 4, ..., each opened one pixel below its top-left corner and bridged to the next ring there:
    one spiral of ones around one spiral corridor of zeros."""
    H, W = shape[-2:]
    m = np.zeros((H, W), np.uint8)
    i = 0
    while 2 * i < min(H, W) - 2 * i:
        a, by, bx = 2 * i, H - 1 - 2 * i, W - 1 - 2 * i
        m[a, a:bx + 1] = m[by, a:bx + 1] = 1
        m[a:by + 1, a] = m[a:by + 1, bx] = 1
        if by - a >= 3 and bx - a >= 3:
            m[a + 1, a] = 0
            m[a + 2, a + 1] = 1
        i += 1
    return np.broadcast_to(m, shape).copy()


def comb(shape):
    """Teeth of ones in the even columns, joined only along the last row: the raster-first roots of the teeth merge last."""
    m = np.zeros(shape, np.uint8)
    m[..., :, 0::2] = 1
    m[..., -1, :] = 1
    return m


def checker(shape):
    """H * W components under 4-connectivity, two image-spanning ones under 8."""
    H, W = shape[-2:]
    m = ((np.arange(H)[:, None] + np.arange(W)[None, :]) & 1).astype(np.uint8)
    return np.broadcast_to(m, shape).copy()


def diag(shape):
    """Diagonal stripes of three values, three pixels wide."""
    H, W = shape[-2:]
    m = (((np.arange(H)[:, None] + np.arange(W)[None, :]) // 3) % 3).astype(np.uint8)
    return np.broadcast_to(m, shape).copy()


PATTERNS = {"serpentine": serpentine, "spiral": spiral, "comb": comb, "checker": checker, "diag": diag}
ALL_INPUTS = KINDS + tuple(PATTERNS)


def make_input(name, seed, shape):
    """One input by name: a kind of tests/test_mask_morph_host.make or a pattern above."""
    return PATTERNS[name](shape) if name in PATTERNS else make(name, seed, shape)


def test_the_patterns_are_what_they_are_for():
    for shape in ((136, 136), (130, 70), (33, 9)):
        H, W = shape
        for connectivity in (4, 8):
            m = serpentine(shape)
            lab, ar = oracle_components(m, connectivity)
            assert (lab[m == 1] == 0).all() and (ar[m == 1] == int(m.sum())).all(), "the snake is one component"
            assert len(np.unique(lab)) == 1 + H // 2, "and every odd row holds one run of zeros"
            m = comb(shape)
            lab, ar = oracle_components(m, connectivity)
            assert (lab[m == 1] == 0).all() and len(np.unique(lab)) == 1 + W // 2
            m = spiral(shape)
            lab, ar = oracle_components(m, connectivity)
            assert (lab[m == 1] == 0).all() and ar[0, 0] == int(m.sum()) and m[1, 0] == 0 and m[2, 1] == 1
            c = np.full(shape, 5, np.uint8)
            lab, ar = oracle_components(c, connectivity)
            assert (lab == 0).all() and (ar == H * W).all()
        m = checker(shape)
        assert len(np.unique(oracle_components(m, 4)[0])) == H * W
        lab, ar = oracle_components(m, 8)
        assert len(np.unique(lab)) == 2 and (ar[0, 0], ar[0, 1]) == (H * W - H * W // 2, H * W // 2)
        assert len(np.unique(oracle_components(diag(shape), 8)[0])) == (H + W - 2) // 3 + 1
    m = spiral((40, 40))
    assert len(np.unique(oracle_components(m, 4)[0])) == 2, "one spiral of ones, one corridor of zeros"


# -- the pins ------------------------------------------------------------------------------------------------------------------
PIN_SHAPES = [(1, 1), (1, 7), (5, 1), (17, 23), (40, 56), (70, 130)]


def _same(got, want, what):
    for g, w, name in zip(got, want, ("labels", "areas")):
        assert g.shape == w.shape and g.dtype == w.dtype == np.int32, (what, name)
        assert int((g != w).sum()) == 0, (what, name)


def test_rule_equals_the_scipy_label_form():
    pytest.importorskip("scipy.ndimage")
    for shape in PIN_SHAPES:
        for kind in KINDS:
            m = make(kind, sum(shape), shape)
            for connectivity in (4, 8):
                _same(rule_components(m, connectivity), scipy_components(m, connectivity), (shape, kind, connectivity))
    batch = np.stack([blobs(5, (32, 32)), np.ones((32, 32), np.uint8), make("classes", 3, (32, 32))])
    _same(rule_components(batch), scipy_components(batch), "batch")


def test_rule_reproduces_the_committed_results():
    """The same pin without scipy: what the scipy form computed (tests/golden/make_mask_components_golden.py)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "mask_components.npz"))
    keys = sorted(k[:-5] for k in g.files if k.endswith("_mask"))
    assert len(keys) >= 4
    many = 0
    for k in keys:
        m = g[k + "_mask"]
        assert m.dtype == np.uint8 and m.shape[-2] <= 64 and m.shape[-1] <= 64
        for connectivity in (4, 8):
            want = g["%s_labels%d" % (k, connectivity)], g["%s_areas%d" % (k, connectivity)]
            _same(rule_components(m, connectivity), want, (k, connectivity))
            many += len(np.unique(want[0])) > 2
    assert many >= 6, "the fixture holds next to no components: it pins nothing"


def test_labels_and_areas_are_what_they_say():
    """Independent of any labeller: a label is a pixel of the same value that labels itself and precedes every pixel it labels; the
    areas are the label counts; 4-components refine 8-components."""
    m = blobs(5, (48, 40))
    l4, a4 = rule_components(m, 4)
    l8, a8 = rule_components(m, 8)
    idx = np.arange(m.size).reshape(m.shape)
    for lab, ar in ((l4, a4), (l8, a8)):
        assert (lab <= idx).all() and (lab.reshape(-1)[lab.reshape(-1)] == lab.reshape(-1)).all()
        assert (m.reshape(-1)[lab.reshape(-1)] == m.reshape(-1)).all()
        assert (np.bincount(lab.reshape(-1), minlength=m.size)[lab] == ar).all()
    assert (l8 <= l4).all() and (a8 >= a4).all() and len(np.unique(l4)) > len(np.unique(l8))


def test_the_guards_of_the_gpu_tests():
    """blobs(5, (128, 128)) at connectivity 8: 286 components, and min_area 16 changes 394 pixels -- a copy kernel cannot pass."""
    m = blobs(5, (128, 128))
    labels, areas = oracle_components(m, 8)
    assert len(np.unique(labels)) == 286
    out = rule_despeckle(m, 16, 8, -1, components=(labels, areas))
    assert int((out != m).sum()) == 394
    rows = rule_rows(m, 16, 8, components=(labels, areas))
    assert rows[NCOMP:NCOMP + SLOTS].sum() == 286 and rows[NCOMP + 2:NCOMP + SLOTS].sum() == 0
    assert rows[SMALL] > 0 and rows[SMALL_PIXELS] >= 394 and rows[LARGEST:LARGEST + 2].min() > 1000


# -- hand cases ----------------------------------------------------------------------------------------------------------------
def _u8(rows):
    return np.array(rows, np.uint8)


def test_hand_cases_of_the_labels():
    for connectivity in (4, 8):
        lab, ar = rule_components(_u8([[7]]), connectivity)
        assert lab.tolist() == [[0]] and ar.tolist() == [[1]]
        lab, ar = rule_components(_u8([[1, 1, 0, 1, 1, 1, 0]]), connectivity)          # one row
        assert lab.tolist() == [[0, 0, 2, 3, 3, 3, 6]] and ar.tolist() == [[2, 2, 1, 3, 3, 3, 1]]
        lab, ar = rule_components(_u8([[0], [0], [5], [0], [0]]), connectivity)        # one column: the two zero runs do not meet
        assert lab.tolist() == [[0], [0], [2], [3], [3]] and ar.tolist() == [[2], [2], [1], [2], [2]]
    checker = _u8([[0, 1], [1, 0]])
    lab, ar = rule_components(checker, 4)
    assert lab.tolist() == [[0, 1], [2, 3]] and (ar == 1).all()
    lab, ar = rule_components(checker, 8)
    assert lab.tolist() == [[0, 1], [1, 0]] and (ar == 2).all()
    diag = np.eye(5, dtype=np.uint8)
    lab4, ar4 = rule_components(diag, 4)
    assert [lab4[i, i] for i in range(5)] == [0, 6, 12, 18, 24] and all(ar4[i, i] == 1 for i in range(5))
    lab8, ar8 = rule_components(diag, 8)
    assert all(lab8[i, i] == 0 and ar8[i, i] == 5 for i in range(5))
    # under 4: 5 pixels + the two triangles; under 8 the line and ONE background, whose triangles meet diagonally across the line
    assert len(np.unique(lab4)) == 7 and len(np.unique(lab8)) == 2 and lab8[1, 0] == lab8[0, 1] == 1 and ar8[4, 0] == 20
    anti = diag[:, ::-1].copy()                 # the other diagonal: joined through up-right steps
    lab8, ar8 = rule_components(anti, 8)
    assert all(lab8[i, 4 - i] == 4 and ar8[i, 4 - i] == 5 for i in range(5))
    # every value is a component of its own, 0 included, and values are compared raw (8 and 9 share a slot, not a component)
    lab, ar = rule_components(_u8([[8, 9, 9, 0, 0, 255]]), 8)
    assert lab.tolist() == [[0, 1, 1, 3, 3, 5]] and ar.tolist() == [[1, 2, 2, 2, 2, 1]]


def test_hand_cases_of_the_filter():
    m = np.zeros((6, 6), np.uint8)
    m[2:4, 2:4] = 1                             # an enclosed island of 4 px: takes the region around it
    assert not rule_despeckle(m, 5).any() and np.array_equal(rule_despeckle(m, 4), m)
    assert (rule_despeckle(m, 5, fill=9)[2:4, 2:4] == 9).all() and rule_despeckle(m, 5, fill=9)[0, 0] == 0
    for k in (0, 1):
        assert np.array_equal(rule_despeckle(make("bytes", 1, (9, 9)), k), make("bytes", 1, (9, 9))), "min_area <= 1 changes nothing"
    # an island whose first pixel is in column 0 takes the pixel ABOVE it
    m = _u8([[3, 3, 3], [1, 1, 3], [3, 3, 3]])
    assert rule_despeckle(m, 3).tolist() == [[3, 3, 3], [3, 3, 3], [3, 3, 3]]
    m = _u8([[2, 2, 4], [1, 4, 4], [4, 4, 4]])          # above, not right or below
    assert rule_despeckle(m, 2).tolist() == [[2, 2, 4], [2, 4, 4], [4, 4, 4]]
    # the component that holds (0, 0) is kept under "neighbour" and replaced under a constant fill
    m = _u8([[1, 0, 0], [0, 0, 0], [0, 0, 0]])
    assert np.array_equal(rule_despeckle(m, 5), m)
    assert rule_despeckle(m, 5, fill=0).tolist() == [[0, 0, 0]] * 3 and rule_despeckle(m, 5, fill=7)[0, 0] == 7
    # the first pixel's left neighbour, not the majority around the component
    m = _u8([[5, 5, 5, 5], [6, 1, 1, 5], [5, 5, 5, 5]])
    for connectivity in (4, 8):                 # the ones take the INPUT 6 left of their first pixel; that 6, a speck itself, the 5 above
        assert rule_despeckle(m, 3, connectivity)[1].tolist() == [5, 6, 6, 5]
    assert rule_despeckle(m, 2)[1].tolist() == [5, 1, 1, 5]
    # a speck nested in a speck: ONE pass on the input's values
    m = np.zeros((7, 7), np.uint8)
    m[1:6, 1:6] = 1
    m[3, 3] = 2
    once = rule_despeckle(m, 30)
    assert (once[1:6, 1:6] == 0).sum() == 24 and once[3, 3] == 1, "the inner speck takes the outer speck's INPUT value"
    twice = rule_despeckle(once, 30)
    assert not twice.any() and not np.array_equal(once, twice), "not idempotent on nested specks: the second pass finishes"


def test_hand_cases_of_the_rows():
    m = _u8([[0, 0, 1, 9], [0, 2, 1, 200], [0, 0, 0, 9]])
    rows = rule_rows(m, 2)
    assert rows.shape == (ROW,) and rows.dtype == np.int64
    assert rows[NCOMP:NCOMP + SLOTS].tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 3]
    assert rows[LARGEST:LARGEST + SLOTS].tolist() == [6, 2, 1, 0, 0, 0, 0, 0, 1]
    assert rows[SMALL] == 4 and rows[SMALL_PIXELS] == 4
    assert rule_rows(m, 0)[SMALL] == 0 and rule_rows(m, 7)[SMALL] == 6 and rule_rows(m, 7)[SMALL_PIXELS] == 12
    batch = np.stack([m, np.zeros((3, 4), np.uint8)])
    rows = rule_rows(batch, 2)
    assert rows.shape == (2, ROW) and rows[1, NCOMP] == 1 and rows[1, LARGEST] == 12 and rows[1].sum() == 13


def test_every_image_of_a_batch_is_a_plane_of_its_own():
    batch = np.stack([np.ones((16, 16), np.uint8), blobs(5, (16, 16)), np.ones((16, 16), np.uint8)])
    lab, ar = rule_components(batch)
    for i in range(3):
        _same((lab[i], ar[i]), rule_components(batch[i]), i)
    assert (lab[0] == 0).all() and (ar[2] == 256).all()
    assert rule_components(batch[:0])[0].shape == (0, 16, 16) and rule_rows(batch[:0], 3).shape == (0, ROW)


# -- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_components_header_symbols_and_macros():
    """include/gsa_components.h declares the one entry (tests/test_abi_and_host.py checks its export and its ctypes row), and its
    macros are the Python constants."""
    from gan_segmentation_amd import mask_ops
    from tests.common import header_declarations
    text, declared = header_declarations("gsa_components.h")
    assert set(declared) == {"gsa_mask_components"}
    for macro, value in (("SLOTS", mask_ops.COMP_SLOTS), ("NCOMP", mask_ops.COMP_NCOMP), ("LARGEST", mask_ops.COMP_LARGEST),
                         ("SMALL", mask_ops.COMP_SMALL), ("SMALL_PIXELS", mask_ops.COMP_SMALL_PIXELS), ("ROW", mask_ops.COMP_ROW)):
        assert "#define GSA_COMP_%s %d " % (macro, value) in text.replace("\n", " \n"), macro
    assert (mask_ops.COMP_SLOTS, mask_ops.COMP_NCOMP, mask_ops.COMP_LARGEST, mask_ops.COMP_SMALL, mask_ops.COMP_SMALL_PIXELS,
            mask_ops.COMP_ROW) == (SLOTS, NCOMP, LARGEST, SMALL, SMALL_PIXELS, ROW)


def test_entry_rejects_bad_arguments_before_touching_the_gpu(hip_library):
    """Argument validation of gsa_mask_components happens on the host (no HIP call precedes it)."""
    from gan_segmentation_amd._lib import load_library
    fn = load_library().fn("gsa_mask_components")
    good = dict(n=2, H=32, W=48, connectivity=8, min_area=4, fill=-1, mask=1 << 20, labels=2 << 20, areas=3 << 20, out=4 << 20, rows=5 << 20)

    def call(**kw):
        a = dict(good, **kw)
        return fn(None, a["n"], a["H"], a["W"], a["connectivity"], a["min_area"], a["fill"], a["mask"], a["labels"], a["areas"],
                  a["out"], a["rows"])

    for bad in (dict(n=-1), dict(H=0), dict(W=0), dict(H=65536), dict(W=65536), dict(H=65535, W=65535), dict(connectivity=6),
                dict(connectivity=0), dict(fill=-2), dict(fill=256), dict(min_area=-1), dict(mask=None), dict(labels=None),
                dict(areas=None), dict(out=1 << 20), dict(out=(1 << 20) + 2 * 32 * 48 - 1), dict(mask=(4 << 20) + 1)):
        assert call(**bad) == -1, bad
    assert call(n=0) == 0 and call(n=0, mask=None, labels=None, areas=None, out=None, rows=None) == 0


def test_wrappers_check_their_arguments_before_any_gpu_work():
    import torch
    from gan_segmentation_amd import mask_ops
    for bad in (torch.zeros((4, 4), dtype=torch.uint8), torch.zeros((1, 4, 4), dtype=torch.float32), np.zeros((4, 4), np.uint8), None):
        with pytest.raises(ValueError, match="mask"):
            mask_ops.components(bad)
        with pytest.raises(ValueError, match="mask"):
            mask_ops.despeckle(bad, 4)
    assert mask_ops.check_fill("neighbour") == -1 and mask_ops.check_fill(0) == 0 and mask_ops.check_fill(np.int64(255)) == 255
    assert mask_ops.check_connectivity(4) == 4 and mask_ops.check_min_area(0) == 0 and mask_ops.check_min_area(2 ** 31 - 1) == 2 ** 31 - 1
    for fn, values in ((mask_ops.check_fill, (-1, 256, "nearest", None, 1.0, True)), (mask_ops.check_connectivity, (6, 0, "8", 8.0, True, None)),
                       (mask_ops.check_min_area, (-1, 2 ** 31, 2.0, "4", None, True))):
        for v in values:
            with pytest.raises(ValueError):
                fn(v)


# -- the keywords and the keys -------------------------------------------------------------------------------------------------
BAD_KEYWORDS = [("mask_min_area", -1), ("mask_min_area", 2.5), ("mask_min_area", "16"), ("mask_min_area", True), ("mask_min_area", None),
                ("mask_min_area", 2 ** 31), ("mask_connectivity", 6), ("mask_connectivity", "8"), ("mask_connectivity", True),
                ("mask_fill", -1), ("mask_fill", 256), ("mask_fill", "nearest"), ("mask_fill", None), ("mask_fill", 0.0)]


@pytest.mark.parametrize("name,value", BAD_KEYWORDS)
def test_keywords_reject_bad_values_before_any_device_work(name, value):
    from gan_segmentation_amd import weights as W
    from gan_segmentation_amd.image_generator import ImageGenerator
    with pytest.raises(ValueError, match=name):
        getattr(ImageGenerator, "check_" + name)(value)
    with pytest.raises(ValueError, match=name):
        ImageGenerator.from_params(W.reduced_generator_config(7), {}, gpu_ids=[0], **{name: value})


def test_keywords_accept_and_default_to_off():
    import inspect
    from gan_segmentation_amd.image_generator import ImageGenerator
    assert ImageGenerator.check_mask_min_area(0) == 0 and ImageGenerator.check_mask_min_area(np.int64(64)) == 64
    assert type(ImageGenerator.check_mask_min_area(np.int64(64))) is int
    assert ImageGenerator.check_mask_connectivity(4) == 4 and ImageGenerator.check_mask_connectivity(8) == 8
    assert ImageGenerator.check_mask_fill("neighbour") == "neighbour" and ImageGenerator.check_mask_fill(0) == 0
    assert ImageGenerator.check_mask_fill(255) == 255
    assert (ImageGenerator.mask_min_area, ImageGenerator.mask_connectivity, ImageGenerator.mask_fill) == (0, 8, "neighbour")
    for fn in (ImageGenerator.__init__, ImageGenerator.from_params):
        p = inspect.signature(fn).parameters
        assert (p["mask_min_area"].default, p["mask_connectivity"].default, p["mask_fill"].default) == (0, 8, "neighbour")


@pytest.mark.parametrize("key,value,name", [("MASK_MIN_AREA", -4, "mask_min_area"), ("MASK_MIN_AREA", "many", "mask_min_area"),
                                            ("MASK_MIN_AREA", 1.5, "mask_min_area"), ("MASK_CONNECTIVITY", 6, "mask_connectivity"),
                                            ("MASK_FILL", 300, "mask_fill"), ("MASK_FILL", "zero", "mask_fill")])
def test_cli_rejects_a_bad_key_before_loading_a_model(tmp_path, no_models, key, value, name):
    from gan_segmentation_amd import main as cli
    with pytest.raises(ValueError, match=name):
        cli.main(["generate", "--config", _config(tmp_path, **{key: value})])


def test_cli_accepts_the_keys_and_their_defaults(tmp_path, no_models):
    from gan_segmentation_amd import main as cli
    for keys in ({}, {"MASK_MIN_AREA": 0}, {"MASK_MIN_AREA": 64, "MASK_CONNECTIVITY": 4, "MASK_FILL": 0},
                 {"MASK_MIN_AREA": 16, "MASK_FILL": "neighbour", "MASK_MORPH": True}):
        with pytest.raises(_ModelLoaded):
            cli.main(["generate", "--config", _config(tmp_path, **keys)])
    for key in ("MASK_MIN_AREA", "MASK_CONNECTIVITY", "MASK_FILL"):
        assert key in cli.__doc__
