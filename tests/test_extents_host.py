"""The method of tests/test_gpu_extents.py can fail, and its cases are what they claim to be -- no GPU needed.

  * the tile constants and launch rules restated in tests/extent_cases.py are those of the sources, and every split case of the GPU
    module takes the number of launches it names;
  * the pattern of every large case of the GPU module meets the conditions of tests/extent_cases.py (no equal neighbours at a
    split, no alias under wrapping at 2^31 and 2^32 in any tensor's own unit), and the case does pass the wrap points it is there for;
  * in the manner of tests/test_train_checks.py, a model op on the CPU -- the same split into launches, the same pattern builder and
    the same ``assert_gathered`` -- is accepted as it is and rejected with each of three faults: a plane offset that wrapped, a second
    launch that re-bases one pointer too few, and a row pointer that is not re-based.  The model runs at 2^15 and 2^16 in place of
    2^31 and 2^32, so that its tensors are real arrays."""
import os
import re

import numpy as np
import pytest
import torch

from tests import extent_cases as X
from tests import test_gpu_extents as G


# ---- the restated rules --------------------------------------------------------------------------------------------------------------
def _source(unit):
    with open(os.path.join(X.CSRC, unit)) as f:
        return f.read()


@pytest.mark.parametrize("unit", sorted(X.TILES))
def test_the_tiles_are_those_of_the_sources(unit):
    assert X.source_tile(unit) == X.TILES[unit]


def test_the_limits_are_those_of_the_sources():
    plane = _source("gsa_plane.h")
    assert "constexpr int kMaxExtent = %d;" % X.MAX_EXTENT in plane
    assert "constexpr long long kMaxWorkgroups = 1ll << 24;" in plane and X.MAX_WORKGROUPS == 1 << 24
    assert "const long long planes_per_launch = (kMaxWorkgroups - 1) / blocks_per_plane;" in plane
    for unit in ("gsa_loss.hip", "gsa_scores.hip"):
        src = _source(unit)
        assert "constexpr int kMaxGridY = %d;" % X.MAX_GRID_Y in src and "first += kMaxGridY" in src
    comp = _source("gsa_components.hip")
    assert "constexpr int kBlockPix = 16 * kThreads;" in comp and X.COMPONENTS_BLOCK_PIX == 16 * X.THREADS
    assert "for_each_launch(n, most," in comp
    assert "for_each_launch(n, tiles_per_plane," in _source("gsa_stats.hip")
    assert "for_each_launch(n, tiles_per_plane > 2 ? tiles_per_plane : 2," in _source("gsa_compare.hip")
    for unit in ("gsa_mask.hip", "gsa_boundary.hip", "gsa_refine.hip", "gsa_overlay.hip"):
        assert re.search(r">= kMaxWorkgroups\) return GSA_ERR_INVALID;\s+// refused, not split", _source(unit)), unit


def test_the_launch_rules_by_hand():
    """65535 rows are 1024 tiles of 64 rows and 2048 of 32; one workgroup fewer than 2^24 a launch."""
    assert X.components_blocks(65535, 1) == 1024 and X.components_blocks(65535, 4) == 1024 and X.planes_per_launch(1024) == 16383
    assert X.components_blocks(1, 65535) == 1024 and X.components_blocks(64, 64) == 1 and X.components_blocks(1, 1) == 1
    assert X.components_blocks(128, 65535) == 2048 and X.components_blocks(256, 256) == 16      # tiles; the seams take 6, the pixels 16
    assert X.stats_blocks(65535, 4) == 2048 and X.compare_blocks(65535, 1) == 2048 and X.planes_per_launch(2048) == 8191
    assert X.compare_blocks(3, 4) == 2 and X.stats_blocks(3, 4) == 1 and X.planes_per_launch(2) == (1 << 23) - 1
    assert X.launches(5, 2) == [(0, 2), (2, 2), (4, 1)] and X.splits(5, 2) == (2, 4) and X.splits(4, 4) == ()
    assert X.largest_grid("gsa_mask.hip", 3, 5) == (1 << 24) - 1 and X.largest_grid("gsa_overlay.hip", 33, 4) == ((1 << 24) - 1) // 2


# ---- the cases of the GPU module -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.SPLIT_CASES + G.GRID_Y_CASES, ids=lambda c: c.name)
def test_every_split_case_takes_the_launches_it_names(case):
    assert case.launches >= 2 and len(case.split_at) == case.launches - 1
    assert len(X.launches(case.n, case.per_launch)) == case.launches
    for b in case.split_at:
        assert 2 <= b <= case.n - 2, "two planes on either side of every split"


@pytest.mark.parametrize("case", G.ALL_LARGE_CASES, ids=lambda c: c.name)
def test_every_pattern_meets_the_conditions(case):
    p = X.make_pattern(case.n, case.D, case.seed, case.split_at, case.elems)
    past = X.check_pattern(p, case.D, case.split_at, case.elems)
    assert len(p) == case.n
    for e, M in case.passes:
        assert past[(e, M)] >= 2, "%s: no plane past 2^%d at %d elements a plane" % (case.name, M.bit_length() - 1, e)
    if case.name.startswith("C-"):
        assert case.device_bytes <= 48e9, "%s holds %.1f GB" % (case.name, case.device_bytes / 1e9)


def test_the_largest_grids_are_one_plane_short_of_refusal():
    for case in G.GRID_CASES:
        unit, (H, W) = case.unit, case.shape
        assert X.tiles_per_plane(unit, H, W) == 1 and case.n == (1 << 24) - 1 == X.largest_grid(unit, H, W)


def test_check_pattern_rejects_what_would_hide_a_fault():
    n, e = 1500, 48
    good = X.make_pattern(n, 5, 1, (700,), (e,), (1 << 15, 1 << 16))
    X.check_pattern(good, 5, (700,), (e,), (1 << 15, 1 << 16))
    with pytest.raises(AssertionError):
        X.check_pattern(np.zeros(n, np.int64), 5, (700,), (e,), (1 << 15, 1 << 16))
    flat = np.array(good)
    flat[700] = flat[699]
    with pytest.raises(AssertionError, match="neighbours"):
        X.check_pattern(flat, 5, (700,), (e,), (1 << 15, 1 << 16))
    alias = np.array(good)
    i, lo, _hi = X.alias_planes(n, e, 1 << 16)
    alias[i[-1]] = alias[lo[-1]]
    with pytest.raises(AssertionError, match="wraps to"):
        X.check_pattern(alias, 5, (700,), (e,), (1 << 15, 1 << 16))


# ---- the model op and its three faults -------------------------------------------------------------------------------------------------
ROW = 3                                         # words of the model's row: the plane's sum, its zeros, its first byte
SMALL_WRAPS = (1 << 15, 1 << 16)
FAULTS = ("a 32-bit-wrapped plane offset", "a launch that re-bases one pointer too few", "a row pointer that is not re-based")


def _model(x, per_launch, fault=None, wrap=SMALL_WRAPS[1]):
    """x (n, e) u8 -> (out (n, e) u8 = 255 - x, rows (n, ROW) int64), computed the way an entry does: launch by launch from flat
    buffers, the pointers re-based per launch, the plane's offset formed inside the launch -- with one of FAULTS built in."""
    n, e = x.shape
    flat = x.reshape(-1)
    out, rows = np.full(n * e, 0xA5, np.uint8), np.full(n * ROW, -1, np.int64)
    lane = np.arange(e)
    for first, count in X.launches(n, per_launch):
        in_base, out_base, row_base = first * e, first * e, first * ROW
        if fault == FAULTS[1]:
            in_base = 0                         # the output was re-based, the input not: the launch reads the first launch's planes
        if fault == FAULTS[2]:
            row_base = 0
        plane = np.arange(count, dtype=np.int64)
        off = plane * e
        src = flat[(in_base + (off % wrap if fault == FAULTS[0] else off))[:, None] + lane]
        out[(out_base + off)[:, None] + lane] = 255 - src
        r = np.stack([src.sum(axis=1, dtype=np.int64), (src == 0).sum(axis=1), src[:, 0].astype(np.int64)], axis=1)
        rows[(row_base + plane * ROW)[:, None] + np.arange(ROW)] = r
    return out.reshape(n, e), rows.reshape(n, ROW)


def _run_model(e, n, per_launch, fault):
    """The GPU module's steps on the model: base batch, pattern, gather, run, compare outputs and inputs."""
    D = 5
    rng = np.random.default_rng(e)
    base = rng.integers(0, 256, (D, e)).astype(np.uint8)
    base_out, base_rows = _model(base, D)
    assert np.array_equal(base_out, 255 - base) and np.array_equal(base_rows[:, 0], base.sum(axis=1))       # "the CPU rule"
    split_at = X.splits(n, per_launch)
    p = X.make_pattern(n, D, 7, split_at, (e, ROW), SMALL_WRAPS)
    X.check_pattern(p, D, split_at, (e, ROW), SMALL_WRAPS)
    big = base[p]
    out, rows = _model(big, per_launch, fault)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    pattern = t(np.array(p))
    X.assert_distinct(torch, t(base_out), "out")
    X.assert_distinct(torch, t(base_rows), "rows")
    X.assert_gathered(torch, t(out), t(base_out), pattern, "out", chunk_bytes=4096)
    X.assert_gathered(torch, t(rows), t(base_rows), pattern, "rows", chunk_bytes=4096)
    X.assert_gathered(torch, t(big), t(base), pattern, "the input", chunk_bytes=4096)


# e = 48 divides no power of two: a wrapped offset lands across two planes; e = 64 lands on one
WRAP_RUNS = [(48, (1 << 16) // 48 + 4), (64, (1 << 16) // 64 + 3)]
SPLIT_RUNS = [(48, 503, 500), (64, 1003, 500), (1, 203, 100)]


@pytest.mark.parametrize("e,n", WRAP_RUNS)
def test_the_model_passes_and_a_wrapped_offset_is_rejected(e, n):
    assert n * e > SMALL_WRAPS[1]
    _run_model(e, n, n, None)
    with pytest.raises(AssertionError, match="out: index"):
        _run_model(e, n, n, FAULTS[0])


@pytest.mark.parametrize("e,n,per_launch", SPLIT_RUNS)
def test_a_launch_that_is_not_re_based_is_rejected(e, n, per_launch):
    _run_model(e, n, per_launch, None)
    with pytest.raises(AssertionError, match="out: index %d " % per_launch):
        _run_model(e, n, per_launch, FAULTS[1])
    with pytest.raises(AssertionError, match="rows: index"):
        _run_model(e, n, per_launch, FAULTS[2])


def test_assert_gathered_compares_bits_and_every_index():
    base = torch.tensor([[0.0, 1.0], [-0.0, float("nan")], [2.0, 3.0]])
    pattern = torch.tensor([2, 1, 0, 1, 2], dtype=torch.int64)
    got = base[pattern].contiguous()
    X.assert_gathered(torch, got, base, pattern, "floats")             # a NaN equals itself, bit for bit
    for i in range(len(pattern)):
        bad = got.clone()
        bad[i, 0] = 0.0 if i != 2 else -0.0                             # +0 for -0 and the reverse are differences too
        if not torch.equal(bad.view(torch.int32), got.view(torch.int32)):
            with pytest.raises(AssertionError, match="index %d " % i):
                X.assert_gathered(torch, bad, base, pattern, "floats", chunk_bytes=8)
    with pytest.raises(AssertionError):
        X.assert_distinct(torch, torch.tensor([[1, 2], [3, 4], [1, 2]]), "equal planes")
