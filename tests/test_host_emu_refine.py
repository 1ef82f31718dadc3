"""csrc/gsa_refine.hip on the HOST under AddressSanitizer + UBSan and under ThreadSanitizer, as tests/test_host_emu.py runs the
other tile kernels (DESIGN.md sections 19 and 22): the unit is compiled unedited with g++ against tools/host_emu/hip/hip_runtime.h
and linked, with those four, into two stand-alone programs of this module's own -- tools/host_emu/emu_run.cpp with
-DGSA_EMU_REFINE, which adds the gsa_mask_refine entry to the driver (independent of -DGSA_EMU_OVERLAY).  ``run_case`` and the build
flags are test_host_emu's.

Every case is held to exit status 0 with the expected entry status, no sanitizer report, inputs unchanged, and every output byte
equal to ``rule_refine`` -- the shapes of tests/test_gpu_refine.py, the large ones reduced to at most 130 px a side.  Overlapping
ranges cannot be written as a case (every tensor is a heap block of its own); the GPU tests refuse them through views of one buffer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import test_host_emu as emu
from tests.extent_cases import LONG_THIN, thin_images, thin_masks
from tests.test_host_emu import COMMON, SANITIZERS, run_case
from tests.test_refine_host import THIN, TILE_EDGES, TABLE_BYTES, case, coarse_tables, every_value, expected, region_image

FILL = emu.FILL
UNITS = emu.UNITS + ["gsa_refine.hip"]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """test_host_emu.build_programs with the refinement's unit and the driver's guarded branch."""
    out = tmp_path_factory.mktemp("host_emu_refine")
    gxx = shutil.which("g++")
    assert gxx, "g++ is not on the PATH: the host emulation needs g++ with its static sanitizer runtimes"
    jobs = {}
    for name, flags in SANITIZERS.items():
        exe = os.path.join(str(out), "emu_refine_" + name)
        cmd = ([gxx] + COMMON + flags + ["-DGSA_EMU_REFINE", "-I", emu.EMU, "-x", "c++"] + [os.path.join(emu.CSRC, u) for u in UNITS]
               + [os.path.join(emu.EMU, "emu_run.cpp"), "-o", exe])
        jobs[name] = (exe, cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    built = {}
    for name, (exe, cmd, proc) in jobs.items():
        log = proc.communicate()[0]
        assert proc.returncode == 0 and os.path.exists(exe), "building the %s program failed:\n%s\n%s" % (name, " ".join(cmd), log[-4000:])
        built[name] = exe
    return built


def _refine(programs, tmp_path, img, mask, tables, classes, radius, offsets=(0, 0, 0, 0), want_change=True, want_tie=True):
    n, H, W, C = img.shape
    want = expected(img, mask, tables, classes, radius, want_change, want_tie)
    tensors = [("img", "in", img, offsets[0]), ("mask", "in", mask, offsets[1]), ("tables", "in", tables, offsets[2]), ("out", "out", want.size, offsets[3])]
    got = run_case(programs, tmp_path, "gsa_mask_refine", (n, H, W, C, classes, radius), tensors)["out"].reshape(want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), "refine %s K %d R %d offsets %s: %d of %d bytes differ from the rule, first at %s: %d instead of %d" % (
        img.shape, classes, radius, offsets, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    return want


@pytest.mark.parametrize("shape", THIN + TILE_EDGES)
def test_thin_planes_and_tile_edges(programs, tmp_path, shape):
    """Two samples, three channels, three classes, radius 3; of these only (32, 64) takes the dword form."""
    H, W = shape
    _refine(programs, tmp_path, *case(H + W, 2, H, W), coarse_tables(), 3, 3, want_change=H * W > 1, want_tie=H * W > 1)


@pytest.mark.parametrize("shape", LONG_THIN, ids=lambda s: "%dx%d" % s)
def test_long_thin_planes(programs, tmp_path, shape):
    """The sides of 65535 that tests/test_gpu_extents.py runs on the GPU, here first, with its radius 5: one tile column of 2048 tile
    rows, and 1024 tiles in a row."""
    H, W = shape
    _refine(programs, tmp_path, thin_images(5 + H % 7, 1, H, W, 3), thin_masks(5 + H % 7, 1, H, W), coarse_tables(), 3, 5)


@pytest.mark.parametrize("radius", [1, 2, 3, 4, 5])
def test_every_radius(programs, tmp_path, radius):
    """One tile-edge shape in the byte form and one of two tiles in the dword form, with the coarse and with the default weights."""
    from gan_segmentation_amd import mask_ops
    for H, W in ((33, 65), (40, 72)):
        img, mask = case(radius + W, 1, H, W)
        _refine(programs, tmp_path, img, mask, coarse_tables(), 3, radius)
        _refine(programs, tmp_path, img, mask, mask_ops.refine_tables(radius), 3, radius, want_tie=False)


@pytest.mark.parametrize("classes", [2, 3, 8])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_classes_and_channels(programs, tmp_path, classes, C):
    """n = 2; with 8 classes the masks hold 8 classes and values the call freezes."""
    for (H, W), R in (((33, 66), 2), ((20, 68), 4)):
        _refine(programs, tmp_path, *case(classes + C, 2, H, W, C, classes), coarse_tables(), classes, R)


def test_batches_and_facing_rows(programs, tmp_path):
    for n in (1, 2, 5):
        _refine(programs, tmp_path, *case(n, n, 18, 21, 3, 2), coarse_tables(), 2, 2)
    mask = np.zeros((2, 8, 12), np.uint8)
    mask[1] = 1                                                         # the facing rows of two samples differ: not neighbours
    img = np.full((2, 8, 12, 3), 70, np.uint8)
    assert np.array_equal(_refine(programs, tmp_path, img, mask, coarse_tables(), 2, 5, want_change=False, want_tie=False), mask)


def test_masks(programs, tmp_path):
    """All 256 values (most of them frozen), a constant plane, and all-zero tables."""
    H, W = 40, 72
    img = region_image(3, 1, H, W, 3)
    for K in (2, 5, 8):
        every = every_value(K, H, W, K)
        want = _refine(programs, tmp_path, img, every, coarse_tables(), K, 3)
        assert np.array_equal(want[every >= K], every[every >= K])
    constant = np.full((1, H, W), 1, np.uint8)
    assert np.array_equal(_refine(programs, tmp_path, img, constant, coarse_tables(), 3, 3, want_change=False, want_tie=False), constant)
    mask = case(5, 1, H, W)[1]
    assert np.array_equal(_refine(programs, tmp_path, img, mask, np.zeros(TABLE_BYTES, np.uint8), 3, 5, want_change=False, want_tie=False), mask)


@pytest.mark.parametrize("which", [0, 1, 2, 3, None], ids=["img", "mask", "tables", "out", "all"])
def test_behind_unaligned_addresses(programs, tmp_path, which):
    """(2, 32, 64): W is a multiple of 4; every tensor 1, 2 and 3 bytes into its block, one at a time and all at once (by different
    amounts).  img, mask and out force the byte form; the tables are read byte by byte in either form."""
    img, mask = case(11, 2, 32, 64)
    for off in (1, 2, 3):
        offsets = tuple((off + k) % 4 for k in range(4)) if which is None else tuple(off if k == which else 0 for k in range(4))
        for C, R in ((3, 3), (4, 1)):
            _refine(programs, tmp_path, img if C == 3 else region_image(12, 2, 32, 64, 4), mask, coarse_tables(), 3, R, offsets=offsets)


def test_larger_cases_reduced(programs, tmp_path):
    """1 x 1024 x 1024 x 3 at R = 2 and 2 x 256 x 320 x 3 at R = 5 of the GPU tests, at 128 x 128 and 2 x 64 x 80."""
    from gan_segmentation_amd import mask_ops
    _refine(programs, tmp_path, *case(21, 1, 128, 128, 3, 8), mask_ops.refine_tables(2), 8, 2, want_tie=False)
    _refine(programs, tmp_path, *case(22, 2, 64, 80, 3, 2), mask_ops.refine_tables(5, 3.0, 40.0), 2, 5, want_tie=False)


# ---- status ------------------------------------------------------------------------------------------------------------------
def _status(programs, tmp_path, scalars, expect, null=None, nbytes=(8, 8, TABLE_BYTES, 8)):
    """One call that must end before any launch: the output stays FILL."""
    tensors = []
    for name, size in zip(("img", "mask", "tables", "out"), nbytes):
        if name == null:
            tensors.append((name, "null", None, 0))
        elif name == "out":
            tensors.append((name, "out", size, 0))
        else:
            tensors.append((name, "in", np.zeros(size, np.uint8), 0))
    got = run_case(programs, tmp_path, "gsa_mask_refine", scalars, tensors, expect=expect)
    for name, part in got.items():
        assert (part == FILL).all(), "%s: %s was written to" % (scalars, name)


def test_an_empty_batch_is_ok_whatever_else_is_passed(programs, tmp_path):
    """n = 0 is decided before anything else: sizes, channels, classes and radius out of range, and null pointers."""
    _status(programs, tmp_path, (0, 16, 16, 3, 2, 3), 0)
    _status(programs, tmp_path, (0, 70000, 0, 9, 1, 6), 0)
    _status(programs, tmp_path, (0, 16, 16, 3, 2, 3), 0, null="out")


@pytest.mark.parametrize("scalars", [(-1, 16, 16, 3, 2, 3), (1, 16, 16, 0, 2, 3), (1, 16, 16, 5, 2, 3), (1, 16, 16, 3, 1, 3), (1, 16, 16, 3, 9, 3),
                                     (1, 16, 16, 3, 0, 3), (1, 16, 16, 3, 2, 0), (1, 16, 16, 3, 2, 6), (1, 16, 16, 3, 2, -1), (1, 0, 16, 3, 2, 3),
                                     (1, 16, 0, 3, 2, 3), (1, 65536, 1, 1, 2, 3), (1, 1, 65536, 1, 2, 3), (1, 65535, 32769, 1, 2, 3)],
                         ids=lambda s: "-".join(map(str, s)))
def test_refusals(programs, tmp_path, scalars):
    """n < 0; channels, classes, radius and sizes outside their ranges; a plane of 2^31 pixels."""
    _status(programs, tmp_path, scalars, -1)


@pytest.mark.parametrize("null", ["img", "mask", "tables", "out"])
def test_a_null_pointer_is_refused(programs, tmp_path, null):
    _status(programs, tmp_path, (1, 16, 16, 3, 2, 3), -1, null=null, nbytes=(768, 256, TABLE_BYTES, 256))


def test_a_grid_of_2_to_the_24_tiles_is_refused(programs, tmp_path):
    """2^24 planes of 1 x 1, one tile each: exactly the workgroup ceiling -- refused, not split, before a byte is written."""
    _status(programs, tmp_path, (1 << 24, 1, 1, 1, 2, 1), -1, nbytes=(1 << 24, 1 << 24, TABLE_BYTES, 1 << 24))
