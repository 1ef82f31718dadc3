"""What tests/test_extents_host.py and tests/test_gpu_extents.py share (no test in here): the launch rules of the stateless entries
restated from their tile constants, the shapes at the documented limits, inputs with structure for planes that are one tile wide,
and the batch-position method for batches too large for a CPU rule.

The method.  D distinct base planes (or samples) go through the op and are held to the CPU rule.  The large batch is
``base[pattern]``, a gather on the device with a fixed seeded ``pattern`` of length n; its output at index i must be the bits of the
base batch's output at ``pattern[i]`` (``assert_gathered``, chunked, on the device).  A kernel that reads or writes plane i at a
wrong offset -- a product that wrapped at 2^31 or 2^32, a pointer that a second launch did not re-base -- lands in another plane j
of the batch, or across two, and is seen iff ``pattern[j] != pattern[i]``.  ``make_pattern`` therefore builds the pattern so that

  * around every split (the first plane of a launch after the first) neighbours differ: pattern[b-2] != pattern[b-1] != pattern[b]
    != pattern[b+1];
  * every plane i whose offset i * e is at or past a wrap point M differs from the plane, or the two planes, that hold the elements
    (i * e) mod M .. (i * e) mod M + e - 1 -- for every e in ``elems``, the elements a plane has in one of the op's tensors (counted
    in that tensor's own unit: bytes for u8, elements for int16, int32, float and int64), and every M in ``wraps``;

and ``check_pattern`` asserts exactly that of a finished pattern, with numpy alone.  No index is excluded from the comparison."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gan-segmentation_amd", "csrc")

MAX_EXTENT = 65535                              # csrc/gsa_plane.h kMaxExtent
MAX_WORKGROUPS = 1 << 24                        # csrc/gsa_plane.h kMaxWorkgroups: a launch takes FEWER
MAX_GRID_Y = 65535                              # gsa_loss.hip, gsa_scores.hip kMaxGridY: samples of one launch
WRAPS = (1 << 31, 1 << 32)

# (tile width, tile height) of each plane unit, asserted against the source text by tests/test_extents_host.py
TILES = {"gsa_mask.hip": (64, 64), "gsa_boundary.hip": (64, 64), "gsa_components.hip": (64, 64), "gsa_stats.hip": (256, 32),
         "gsa_compare.hip": (256, 32), "gsa_refine.hip": (64, 32), "gsa_overlay.hip": (128, 32)}
COMPONENTS_BLOCK_PIX = 16 * 256                 # gsa_components.hip kBlockPix: pixels of a workgroup in phases 3 and 4
THREADS = 256

# Family A: one tile column of 1024 (64-row tiles) or 2048 (32-row tiles) tile rows, and the transpose; byte form and dword form
LONG_THIN = [(1, 65535), (65535, 1), (65535, 4), (3, 65535)]
PHOTOMETRIC_THIN = [(4, 65535), (65535, 4)]     # the photometric op takes sides from 4 up (reflect-101 at radius 3)


def source_tile(unit):
    """(tile width, tile height) as csrc/<unit> states them."""
    with open(os.path.join(CSRC, unit)) as f:
        src = f.read()
    one = re.search(r"constexpr int kTile = (\d+);", src)
    if one:
        return int(one.group(1)), int(one.group(1))
    return int(re.search(r"constexpr int kTileW = (\d+);", src).group(1)), int(re.search(r"constexpr int kTileH = (\d+);", src).group(1))


def tiles_per_plane(unit, H, W):
    tw, th = TILES[unit]
    return -(-W // tw) * -(-H // th)


# ---- the entries' launch rules -------------------------------------------------------------------------------------------------
def components_blocks(H, W):
    """gsa_mask_components: the most workgroups a plane takes in any of its four launches."""
    tw, th = TILES["gsa_components.hip"]
    tiles_x, tiles_y = -(-W // tw), -(-H // th)
    seam_px = (tiles_y - 1) * W + (tiles_x - 1) * H
    return max(tiles_x * tiles_y, -(-seam_px // THREADS), -(-(H * W) // COMPONENTS_BLOCK_PIX))


def stats_blocks(H, W):
    """gsa_pair_stats: a workgroup a tile."""
    return tiles_per_plane("gsa_stats.hip", H, W)


def compare_blocks(H, W):
    """gsa_mask_compare: a workgroup a tile, counted as at least two so that the init launch fits as well."""
    return max(tiles_per_plane("gsa_compare.hip", H, W), 2)


def planes_per_launch(blocks_per_plane):
    """csrc/gsa_plane.h for_each_launch."""
    assert 1 <= blocks_per_plane < MAX_WORKGROUPS
    return (MAX_WORKGROUPS - 1) // blocks_per_plane


def launches(n, per_launch):
    """[(first, count)] of consecutive groups of at most ``per_launch`` of n planes or samples."""
    return [(first, min(per_launch, n - first)) for first in range(0, n, per_launch)]


def splits(n, per_launch):
    """The first plane of every launch after the first."""
    return tuple(first for first, _count in launches(n, per_launch)[1:])


def largest_grid(unit, H, W):
    """The largest n a "refused, not split" entry accepts at (H, W)."""
    return (MAX_WORKGROUPS - 1) // tiles_per_plane(unit, H, W)


# ---- the pattern -----------------------------------------------------------------------------------------------------------------
def alias_planes(n, elems, modulus):
    """-> (i, lo, hi): the planes i of n whose offset i * elems is at or past ``modulus``, and the first and last plane that the
    ``elems`` elements from (i * elems) mod modulus on lie in (lo == hi where elems divides the modulus)."""
    i = np.arange(n, dtype=np.int64)
    off = i * int(elems)
    i = i[off >= modulus]
    w = (i * int(elems)) % int(modulus)
    return i, w // int(elems), (w + int(elems) - 1) // int(elems)


@functools.lru_cache(maxsize=2)
def make_pattern(n, D, seed, split_at=(), elems=(), wraps=WRAPS):
    """int64 (n,) of values in [0, D): seeded, with the conditions of the module docstring.  Asserts that D values suffice."""
    rng = np.random.default_rng([seed, n, D])
    p = rng.integers(0, D, n)
    p[:D] = rng.permutation(D)[:n]              # every base plane occurs
    differ = {}                                 # index -> the EARLIER indices it must differ from
    for b in split_at:
        for k in (b - 1, b, b + 1):
            if 1 <= k < n:
                differ.setdefault(k, set()).add(k - 1)
    for e in elems:
        for M in wraps:
            i, lo, hi = alias_planes(n, e, M)
            for a, b, c in zip(i.tolist(), lo.tolist(), hi.tolist()):
                differ.setdefault(a, set()).update((b, c))
    for i in sorted(differ):
        taken = {int(p[j]) for j in differ[i]}
        assert all(j < i for j in differ[i])
        if int(p[i]) in taken:
            free = [v for v in range(D) if v not in taken]
            assert free, "D = %d values do not suffice at index %d (%d planes to differ from)" % (D, i, len(differ[i]))
            p[i] = free[int(rng.integers(len(free)))]
    p.setflags(write=False)
    return p


def check_pattern(p, D, split_at=(), elems=(), wraps=WRAPS):
    """The conditions, asserted of a finished pattern.  -> {(elems, modulus): number of planes past that wrap point}."""
    p = np.asarray(p)
    n = len(p)
    assert p.dtype == np.int64 and p.min() >= 0 and p.max() < D and len(np.unique(p)) == min(D, n), "values 0..D-1, every one used"
    for b in split_at:
        assert 2 <= b <= n - 2, "a split needs two planes on either side"
        assert p[b - 2] != p[b - 1] and p[b - 1] != p[b] and p[b] != p[b + 1], "equal neighbours at the split %d" % b
    past = {}
    for e in elems:
        for M in wraps:
            i, lo, hi = alias_planes(n, e, M)
            past[(e, M)] = len(i)
            bad = (p[i] == p[lo]) | (p[i] == p[hi])
            assert not bad.any(), "plane %d has the value of the plane its offset wraps to (%d elements a plane, modulus 2^%d)" % (
                i[bad][0], e, int(M).bit_length() - 1)
    return past


# ---- the comparison ----------------------------------------------------------------------------------------------------------------
def _bits(torch, t):
    """t as integers of its element size: NaNs and signed zeros compare as what they are."""
    return t.view({4: torch.int32, 8: torch.int64, 2: torch.int16, 1: torch.uint8}[t.element_size()]) if t.is_floating_point() else t


def assert_gathered(torch, got, base, pattern, what, chunk_bytes=1 << 27):
    """got (n, ...) is base (D, ...)[pattern] bit for bit -- every index, on the tensors' own device, ``chunk_bytes`` at a time."""
    n = got.shape[0]
    assert pattern.shape == (n,) and pattern.dtype == torch.int64 and pattern.device == got.device == base.device, what
    assert got.shape[1:] == base.shape[1:] and got.dtype == base.dtype and got.is_contiguous() and base.is_contiguous(), "%s: %s %s vs %s %s" % (
        what, tuple(got.shape), got.dtype, tuple(base.shape), base.dtype)
    g, b = _bits(torch, got.reshape(n, -1)), _bits(torch, base.reshape(base.shape[0], -1))
    per = max(1, chunk_bytes // max(1, g.shape[1] * g.element_size()))
    for s in range(0, n, per):
        part, want = g[s:s + per], b.index_select(0, pattern[s:s + per])
        if not torch.equal(part, want):
            rows = (part != want).any(dim=1).nonzero().reshape(-1)
            i = s + int(rows[0])
            at = int((g[i] != b[int(pattern[i])]).nonzero()[0])
            raise AssertionError("%s: index %d (base plane %d) differs from the base batch's output, first at element %d: %s instead of %s; "
                                 "%d of the %d indices from %d on differ" % (what, i, int(pattern[i]), at, g[i, at].item(),
                                                                            b[int(pattern[i]), at].item(), len(rows), len(part), s))


def assert_distinct(torch, base, what):
    """No two base planes (inputs or outputs) are equal: a plane read in place of another then shows."""
    flat = _bits(torch, base.reshape(base.shape[0], -1))
    for a in range(len(flat)):
        for b in range(a + 1, len(flat)):
            assert not torch.equal(flat[a], flat[b]), "%s: base planes %d and %d are equal" % (what, a, b)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def thin_masks(seed, n, H, W, classes=3, with255=True):
    """(n, H, W) u8 for planes a few pixels across: along the long side runs of 1..40 px of ``classes`` values (a few of them 255),
    every line of the short side shifted against the last by a few pixels -- so regions of a few hundred pixels cross every tile seam,
    boundaries lie closer together than any band radius and further apart, and single pixels of another value are sprinkled in."""
    rng = np.random.default_rng([seed, H, W])
    long_side, short = max(H, W), min(H, W)
    out = np.empty((n, short, long_side), np.uint8)
    for i in range(n):
        runs = rng.integers(1, 41, long_side // 8 + 2)
        runs[rng.random(len(runs)) < 0.1] += 150                 # some regions wider than two 64-px tiles and any band
        values = rng.integers(0, classes, len(runs))
        values[1:][values[1:] == values[:-1]] += 1
        values %= classes
        line = np.repeat(values, runs)[:long_side].astype(np.uint8)
        assert len(line) == long_side
        for s in range(short):
            out[i, s] = np.roll(line, int(rng.integers(-3, 4)) * s)
        hit = rng.random(out[i].shape) < 0.01
        out[i][hit] = rng.integers(0, classes, int(hit.sum()))
        if with255:
            out[i][rng.random(out[i].shape) < 0.005] = 255
    return np.ascontiguousarray(out if W >= H else out.transpose(0, 2, 1))


def thin_images(seed, n, H, W, C):
    """(n, H, W, C) u8: a colour per region of ``thin_masks(seed + 1, ...)`` plus noise -- flat regions with edges, as images have."""
    rng = np.random.default_rng([seed, H, W, C])
    regions = thin_masks(seed + 1, n, H, W, classes=4, with255=False)
    palette = rng.integers(0, 256, (n, 4, C))
    img = np.stack([palette[i][regions[i]] for i in range(n)]) + 6.0 * rng.standard_normal((n, H, W, C))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
