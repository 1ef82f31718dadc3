"""csrc/gsa_overlay.hip on the HOST under AddressSanitizer + UBSan and under ThreadSanitizer, as tests/test_host_emu.py runs the
other four tile kernels (DESIGN.md sections 19 and 21): the unit is compiled unedited with g++ against tools/host_emu/hip/
hip_runtime.h and linked, with those four, into two stand-alone programs of this module's own -- tools/host_emu/emu_run.cpp with
-DGSA_EMU_OVERLAY, which adds the gsa_overlay entry to the driver.  ``run_case`` and the build flags are test_host_emu's.

Every case is held to exit status 0 with the expected entry status, no sanitizer report, inputs unchanged, and every output byte
equal to ``rule_overlay`` -- the shapes of tests/test_gpu_overlay.py, the full-size one reduced.  Overlapping ranges cannot be
written as a case (every tensor is a heap block of its own); the GPU tests refuse them through views of one buffer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import test_host_emu as emu
from tests.extent_cases import LONG_THIN, thin_images, thin_masks
from tests.test_host_emu import COMMON, SANITIZERS, run_case
from tests.test_preview_host import blob_masks, dataset_lut, random_image, random_lut, rule_overlay

FILL = emu.FILL
UNITS = emu.UNITS + ["gsa_overlay.hip"]

THIN = [(1, 1), (1, 70), (70, 1)]
TILE_EDGES = [(16, 16), (63, 65), (65, 63), (64, 64), (66, 131), (32, 128), (33, 129)]      # the issue's, and the 128 x 32 tile's own
FACTOR_SHAPES = [(32, 48), (96, 80)]
FACTORS = (1, 2, 4, 8, 16)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """test_host_emu.build_programs with the fifth unit and the driver's guarded branch."""
    out = tmp_path_factory.mktemp("host_emu_overlay")
    gxx = shutil.which("g++")
    assert gxx, "g++ is not on the PATH: the host emulation needs g++ with its static sanitizer runtimes"
    jobs = {}
    for name, flags in SANITIZERS.items():
        exe = os.path.join(str(out), "emu_overlay_" + name)
        cmd = ([gxx] + COMMON + flags + ["-DGSA_EMU_OVERLAY", "-I", emu.EMU, "-x", "c++"] + [os.path.join(emu.CSRC, u) for u in UNITS]
               + [os.path.join(emu.EMU, "emu_run.cpp"), "-o", exe])
        jobs[name] = (exe, cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    built = {}
    for name, (exe, cmd, proc) in jobs.items():
        log = proc.communicate()[0]
        assert proc.returncode == 0 and os.path.exists(exe), "building the %s program failed:\n%s\n%s" % (name, " ".join(cmd), log[-4000:])
        built[name] = exe
    return built


def _overlay(programs, tmp_path, img, mask, lut, factor=1, cols=1, offsets=(0, 0, 0, 0)):
    n, H, W, C = img.shape
    want = rule_overlay(img, mask, lut, factor, cols)
    tensors = [("img", "in", img, offsets[0]), ("mask", "in", mask, offsets[1]), ("lut", "in", lut, offsets[2]), ("out", "out", want.size, offsets[3])]
    got = run_case(programs, tmp_path, "gsa_overlay", (n, H, W, C, factor, cols), tensors)["out"].reshape(want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), "overlay %s f %d cols %d offsets %s: %d of %d bytes differ from the rule, first at %s: %d instead of %d" % (
        img.shape, factor, cols, offsets, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    return want


def _inputs(seed, n, H, W, C):
    return random_image(seed, n, H, W, C), blob_masks(seed, n, H, W), random_lut(seed)


@pytest.mark.parametrize("shape", THIN + TILE_EDGES)
def test_thin_planes_and_tile_edges(programs, tmp_path, shape):
    """f = 1, two samples: of these only (16, 16), (64, 64) and (32, 128) take the dword form."""
    want = _overlay(programs, tmp_path, *_inputs(sum(shape), 2, *shape, 3))
    assert want.shape == (2 * shape[0], shape[1], 3)


@pytest.mark.parametrize("shape", LONG_THIN, ids=lambda s: "%dx%d" % s)
def test_long_thin_planes(programs, tmp_path, shape):
    """The sides of 65535 that tests/test_gpu_extents.py runs on the GPU, here first; f = 1 is the one factor that divides them."""
    H, W = shape
    _overlay(programs, tmp_path, thin_images(5 + H % 7, 1, H, W, 3), thin_masks(5 + H % 7, 1, H, W), random_lut(5 + H % 7))


@pytest.mark.parametrize("factor", FACTORS)
def test_every_factor(programs, tmp_path, factor):
    for H, W in FACTOR_SHAPES + [(16, 16), (64, 256)]:
        for C in (3, 4) if (H, W) == (32, 48) else (3,):
            _overlay(programs, tmp_path, *_inputs(factor + H, 2, H, W, C), factor=factor, cols=2)
    if factor <= 2:                                     # W % 4 == 2: the byte form, and at f = 2 a thread whose second block is outside
        _overlay(programs, tmp_path, *_inputs(factor, 1, 6, 134, 3), factor=factor)


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_channels_and_batch(programs, tmp_path, C):
    """n = 5 with cols 1, 2 and 5, with 3 (one empty cell, as with 2) and 7 (more columns than samples), in both access forms."""
    for cols in (1, 2, 3, 5, 7):
        for (H, W), f in (((32, 48), 2), ((18, 21), 1), ((16, 32), 1)):
            want = _overlay(programs, tmp_path, *_inputs(C + cols, 5, H, W, C), factor=f, cols=cols)
            if cols == 2:
                assert not want[2 * (H // f):, W // f:].any() and want[2 * (H // f):, : W // f].any(), "the sixth cell is empty, the fifth is not"


def test_masks(programs, tmp_path):
    H, W = 40, 136
    img, lut = random_image(3, 1, H, W, 3), random_lut(3)
    yy, xx = np.mgrid[:H, :W]
    checker = ((yy + xx) & 1).astype(np.uint8)[None]                     # every pixel is an edge
    constant = np.full((1, H, W), 2, np.uint8)                          # none is
    every = (np.arange(H * W) % 256).astype(np.uint8).reshape(1, H, W)  # all 256 values
    for mask in (checker, constant, every, blob_masks(9, 1, H, W, 6)):
        _overlay(programs, tmp_path, img, mask, lut)
        _overlay(programs, tmp_path, img, mask, dataset_lut(), factor=4)
    facing = np.zeros((2, 8, 12), np.uint8)
    facing[1] = 1                                                       # the facing rows of two samples differ: no edge
    lut = np.zeros((256, 6), np.uint8)
    lut[:2] = ((1, 2, 3, 4, 0, 128), (5, 6, 7, 8, 0, 128))
    img = random_image(4, 2, 8, 12, 3)
    assert np.array_equal(_overlay(programs, tmp_path, img, facing, lut), img.reshape(16, 12, 3))


@pytest.mark.parametrize("which", [0, 1, 2, 3, None], ids=["img", "mask", "lut", "out", "all"])
def test_behind_unaligned_addresses(programs, tmp_path, which):
    """(2, 32, 64): W is a multiple of 4; every tensor 1, 2 and 3 bytes into its block, one at a time and all at once (by
    different amounts).  img, mask and -- at f = 1 -- out force the byte form; the table is read byte by byte in either form."""
    img, mask, lut = _inputs(11, 2, 32, 64, 3)
    for off in (1, 2, 3):
        offsets = tuple((off + k) % 4 for k in range(4)) if which is None else tuple(off if k == which else 0 for k in range(4))
        for f in (1, 2, 8):
            _overlay(programs, tmp_path, img, mask, lut, factor=f, cols=1 if f == 1 else 3, offsets=offsets)


def test_full_size_reduced(programs, tmp_path):
    """The 2 x 1024 x 1024 x 3 case of the GPU tests at 128 x 256: f = 1, and f = 8 with cols = 2."""
    img, mask, lut = _inputs(12, 2, 128, 256, 3)
    _overlay(programs, tmp_path, img, mask, lut)
    _overlay(programs, tmp_path, img, mask, lut, factor=8, cols=2)


# ---- status ------------------------------------------------------------------------------------------------------------------
def _status(programs, tmp_path, scalars, expect, null=None, nbytes=(8, 8, 1536, 8)):
    """One call that must end before any launch: the output stays FILL."""
    tensors = []
    for name, size in zip(("img", "mask", "lut", "out"), nbytes):
        if name == null:
            tensors.append((name, "null", None, 0))
        elif name == "out":
            tensors.append((name, "out", size, 0))
        else:
            tensors.append((name, "in", np.zeros(size, np.uint8), 0))
    got = run_case(programs, tmp_path, "gsa_overlay", scalars, tensors, expect=expect)
    for name, part in got.items():
        assert (part == FILL).all(), "%s: %s was written to" % (scalars, name)


def test_an_empty_batch_is_ok_whatever_else_is_passed(programs, tmp_path):
    """n = 0 is decided before anything else: sizes, channels, factor and cols out of range, and null pointers."""
    _status(programs, tmp_path, (0, 16, 16, 3, 1, 1), 0)
    _status(programs, tmp_path, (0, 70000, 0, 9, 3, 0), 0)
    _status(programs, tmp_path, (0, 16, 16, 3, 1, 1), 0, null="out")


@pytest.mark.parametrize("scalars", [(-1, 16, 16, 3, 1, 1), (1, 16, 16, 0, 1, 1), (1, 16, 16, 5, 1, 1), (1, 16, 16, 3, 0, 1), (1, 16, 16, 3, 3, 1),
                                     (1, 32, 32, 3, 32, 1), (1, 16, 16, 3, -2, 1), (1, 6, 8, 3, 4, 1), (1, 8, 6, 3, 4, 1), (1, 16, 16, 3, 1, 0),
                                     (1, 16, 16, 3, 1, -1), (1, 0, 16, 3, 1, 1), (1, 16, 0, 3, 1, 1), (1, 65536, 1, 1, 1, 1), (1, 1, 65536, 1, 1, 1),
                                     (1, 65535, 32769, 1, 1, 1), (1 << 21, 16, 16, 4, 1, 1), (1 << 19, 16, 16, 4, 1, 1 << 25),
                                     (3, 16, 16, 4, 1, 1 << 26)], ids=lambda s: "-".join(map(str, s)))
def test_refusals(programs, tmp_path, scalars):
    """n < 0; channels, factor, cols and sizes outside their ranges; sides the factor does not divide; a plane of 2^31 pixels; and
    sheets of 2^31 bytes and more: 2^21 samples of 1 KiB in one column, 2^19 of them in a row of 2^25 cells, and 3 in a row of 2^26."""
    _status(programs, tmp_path, scalars, -1)


@pytest.mark.parametrize("null", ["img", "mask", "lut", "out"])
def test_a_null_pointer_is_refused(programs, tmp_path, null):
    _status(programs, tmp_path, (1, 16, 16, 3, 1, 1), -1, null=null, nbytes=(768, 256, 1536, 768))


def test_a_grid_of_2_to_the_24_tiles_is_refused(programs, tmp_path):
    """2^24 planes of 1 x 1, one tile each: a sheet of 16 MiB, within its limit, but exactly the workgroup ceiling -- refused, not
    split, before a byte is written."""
    _status(programs, tmp_path, (1 << 24, 1, 1, 1, 1, 1), -1, nbytes=(1 << 24, 1 << 24, 1536, 1 << 24))
