"""The stateless tile kernels on the HOST under AddressSanitizer + UBSan and under ThreadSanitizer.

csrc/gsa_mask.hip, gsa_boundary.hip, gsa_augment.hip and gsa_photometric.hip are compiled unedited with g++ against the stand-in
runtime of tools/host_emu/hip/hip_runtime.h (a workgroup as 256 threads and a barrier) and linked with tools/host_emu/emu_run.cpp
into two stand-alone programs with static sanitizer runtimes, built once per run of this module into pytest's temporary directory.
Every case is written to a file, run by both programs in child processes of their own, and held to three things: exit status 0,
no sanitizer report on stderr, and every output byte equal to the rule the GPU tests use -- rule_morph, rule_boundary / rule_band,
rule_augment (fp32 and bf16 bit for bit), rule_photometric.  The GPU tests catch a wrong output; these catch what is right by luck:
an access past a buffer or an LDS array, a vector access at an address not aligned for it, a barrier that is missing, signed
overflow or a bad shift in the tile arithmetic.

Every tensor is a heap block of exactly the size the header asks for (plus the case's address offset), outputs are filled with
0xA5 before the call, and inputs must come back unchanged.

No host libm function stands in for a device function whose result could differ: the kernels call floorf, fminf and fmaxf only,
which are exact in both places, and the build uses -ffp-contract=off as the library's does.  Nothing is compared more loosely than
in the GPU tests.  No kernel is excluded from the ThreadSanitizer run.

The shapes are those of the GPU tests (imported where they are module constants or parametrisations), the large ones reduced."""
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

from tests import test_gpu_augment as gpu_augment, test_gpu_boundary as gpu_boundary, test_gpu_photometric as gpu_photometric
from tests.extent_cases import LONG_THIN, PHOTOMETRIC_THIN, thin_masks
from tests.test_augment_host import random_pair, rule_augment
from tests.test_boundary_host import class_blobs, has_both, rule_band, rule_boundary
from tests.test_mask_morph_host import SEAM_SHAPES, SMALL_SHAPES, make, rule_morph
from tests.test_photometric_host import random_images, row, rule_photometric

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gan-segmentation_amd", "csrc")
EMU = os.path.join(ROOT, "tools", "host_emu")
UNITS = ["gsa_boundary.hip", "gsa_mask.hip", "gsa_augment.hip", "gsa_photometric.hip"]
COMMON = ["-std=c++20", "-O1", "-g", "-ffp-contract=off", "-pthread"]
SANITIZERS = {
    "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"],
    "tsan": ["-fsanitize=thread", "-static-libtsan"],
}
FILL = 0xA5
TIME_LIMIT = 120                                # seconds for one child; a case takes well under one
LONG_TIME_LIMIT = 600                           # ... but for the planes with a side of 65535: thousands of workgroups, about a minute
REPORT = re.compile(r"Sanitizer|runtime error")


def _parametrised(fn):
    """The argument values of a test's one ``pytest.mark.parametrize``."""
    (mark,) = [m for m in fn.pytestmark if m.name == "parametrize"]
    return list(mark.args[1])


def build_programs(out, csrc=CSRC):
    """{"asan": path, "tsan": path}: the two programs, compiled side by side into the directory ``out``."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is not on the PATH: the host emulation needs g++ with its static sanitizer runtimes (libasan.a, libubsan.a, libtsan.a)"
    start = time.time()
    jobs = {}
    for name, flags in SANITIZERS.items():
        exe = os.path.join(str(out), "emu_" + name)
        cmd = [gxx] + COMMON + flags + ["-I", EMU, "-x", "c++"] + [os.path.join(csrc, u) for u in UNITS] + [os.path.join(EMU, "emu_run.cpp"), "-o", exe]
        jobs[name] = (exe, cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    built = {}
    for name, (exe, cmd, proc) in jobs.items():
        log = proc.communicate()[0]
        assert proc.returncode == 0 and os.path.exists(exe), (
            "building the %s program failed (a missing static sanitizer runtime shows as a linker error):\n%s\n%s" % (name, " ".join(cmd), log[-4000:]))
        built[name] = exe
    print("host_emu: both programs built in %.1f s" % (time.time() - start))
    return built


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return build_programs(tmp_path_factory.mktemp("host_emu"))


def _write_case(path, entry, scalars, tensors, expect):
    """tensors: (name, kind, array | byte count | None, offset) in the entry's pointer order."""
    lines = ["gsa-emu-case 1", "entry " + entry, "expect %d" % expect, "scalars %d %s" % (len(scalars), " ".join(str(int(v)) for v in scalars)),
             "tensors %d" % len(tensors)]
    data = []
    for name, kind, what, offset in tensors:
        assert kind in ("in", "out", "null")
        size = 0 if kind == "null" else what.nbytes if kind == "in" else int(what)
        lines.append("%s %s %d %d" % (name, kind, size, offset))
        if kind == "in":
            data.append(np.ascontiguousarray(what).tobytes())
    with open(path, "wb") as f:
        f.write(("\n".join(lines) + "\ndata\n").encode() + b"".join(data))


_serial = [0]


def run_case(programs, tmp_path, entry, scalars, tensors, expect=0):
    """Run one case under both programs at once.  Asserts a clean run, inputs unchanged and both programs' outputs identical;
    -> {name: uint8 array} of the output tensors."""
    _serial[0] += 1
    case = str(tmp_path / ("case%d.bin" % _serial[0]))
    _write_case(case, entry, scalars, tensors, expect)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    limit = LONG_TIME_LIMIT if any(int(s) >= 65535 for s in scalars[1:3]) else TIME_LIMIT
    procs = {}
    for name, exe in programs.items():
        out = "%s.%s.out" % (case, name)
        procs[name] = (out, subprocess.Popen([exe, case, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env))
    results = {}
    for name, (out, proc) in procs.items():
        what = "%s %s under %s" % (entry, list(scalars), name)
        try:
            _stdout, stderr = proc.communicate(timeout=limit)
        except subprocess.TimeoutExpired:       # a barrier that not every thread reaches: the emulation hangs where a GPU would not
            for _name, (_out, other) in procs.items():
                other.kill()
                other.communicate()
            raise AssertionError("%s: no end after %d s" % (what, limit))
        assert proc.returncode == 0 and not REPORT.search(stderr), "%s: exit status %d\n%s" % (what, proc.returncode, stderr[-6000:])
        blob = np.fromfile(out, np.uint8)
        got, at = {}, 0
        for tname, kind, arg, _offset in tensors:
            if kind == "null":
                continue
            size = arg.nbytes if kind == "in" else int(arg)
            part = blob[at:at + size]
            at += size
            if kind == "in":
                assert np.array_equal(part, np.ascontiguousarray(arg).reshape(-1).view(np.uint8)), "%s: the input %s was written to" % (what, tname)
            else:
                got[tname] = part
        assert at == blob.size, "%s: %d bytes of output for %d expected" % (what, blob.size, at)
        results[name] = got
        os.remove(out)
    os.remove(case)
    first = results["asan"]
    for tname, part in results["tsan"].items():
        assert np.array_equal(part, first[tname]), "%s: the two programs disagree on %s" % (entry, tname)
    return first


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s vs %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    bad = got != want
    assert not bad.any(), "%s: %d of %d values differ from the rule, first at %s: %s instead of %s" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


# ---- mask_morph ----------------------------------------------------------------------------------------------------------------
MORPH_KINDS = ("blobs", "bytes", "frame0")      # one smooth, one of all byte values, and the one a zero-padded erosion fails


def _morph(programs, tmp_path, m, mask_offset=0, out_offset=0):
    n, H, W = m.shape
    got = run_case(programs, tmp_path, "gsa_mask_morph", (n, H, W), [("mask", "in", m, mask_offset), ("out", "out", m.size, out_offset)])
    _same(got["out"].reshape(m.shape), rule_morph(m), "morph %s offsets %d / %d" % (m.shape, mask_offset, out_offset))


@pytest.mark.parametrize("shape", SMALL_SHAPES + SEAM_SHAPES + [(2, 20, 70)])
def test_mask_morph(programs, tmp_path, shape):
    """The GPU tests' shapes, with three input kinds stacked into one batch (every plane is on its own under the rule, so the batch
    also shows a leak between planes).  (2, 20, 70): W % 4 != 0, so the second plane of each kind starts at an unaligned byte."""
    m = np.concatenate([make(kind, sum(shape), shape) for kind in MORPH_KINDS])
    _morph(programs, tmp_path, m)


@pytest.mark.parametrize("mask_offset,out_offset", [(1, 0), (0, 1), (1, 1)])
def test_mask_morph_behind_an_odd_byte(programs, tmp_path, mask_offset, out_offset):
    """Planes of 15 x 20 bytes: W is a multiple of 4, one pointer or both are not aligned, so the byte form must be the one chosen."""
    _morph(programs, tmp_path, make("blobs", 7, (3, 15, 20)), mask_offset, out_offset)


@pytest.mark.parametrize("shape", LONG_THIN, ids=lambda s: "%dx%d" % s)
def test_mask_morph_long_thin_planes(programs, tmp_path, shape):
    """The sides of 65535 that tests/test_gpu_extents.py runs on the GPU, here first: one tile column of 1024 tile rows and its
    transpose, one plane each (a workgroup is 256 host threads here: a thousand of them take half a minute); (65535, 4) takes
    the dword form."""
    _morph(programs, tmp_path, thin_masks(5 + shape[0] % 7, 1, *shape))


# ---- boundary ------------------------------------------------------------------------------------------------------------------
SMALL_PLANES = _parametrised(gpu_boundary.test_small_and_thin_planes)      # (1, 1), (1, 70), (70, 1), (16, 16)
TILE_EDGES = _parametrised(gpu_boundary.test_tile_edges)                    # (63, 65) .. (131, 66)
ALL_RADII = (1, 2, 4, 5, 8, 9, 16, 17, 31, 32)                                   # both ends of each of the four apron sizes
FORMS = {"both": (True, True), "dist2": (True, False), "out": (False, True)}


def _boundary(programs, tmp_path, m, R, label=255, form="both", offsets=(0, 0, 0)):
    """One call in one output form against the rule; -> the expected dist2."""
    n, H, W = m.shape
    with_dist2, with_out = FORMS[form]
    tensors = [("mask", "in", m, offsets[0]),
               ("dist2", "out", 2 * m.size, offsets[1]) if with_dist2 else ("dist2", "null", None, 0),
               ("out", "out", m.size, offsets[2]) if with_out else ("out", "null", None, 0)]
    got = run_case(programs, tmp_path, "gsa_mask_boundary", (n, H, W, R, label), tensors)
    want = rule_boundary(m, R)
    what = "boundary %s R %d %s offsets %s" % (m.shape, R, form, offsets)
    if with_dist2:
        _same(got["dist2"].view(np.int16).reshape(m.shape), want, what + " dist2")
    if with_out:
        _same(got["out"].reshape(m.shape), rule_band(m, R, label, want), what + " out")
    return want


def _boundary_input(shape, R):
    """What the GPU tests feed these shapes.  Small and thin planes: blocks of 7 px up to R = 5, one corner of another value beyond;
    tile-edge planes: two odd pixels, and blobs as a second plane of the batch."""
    if tuple(shape) in SMALL_PLANES:
        if R < 7:
            return gpu_boundary._pattern(shape, 7)[None]
        m = np.zeros(shape, np.uint8)
        m[:3, :3] = 3
        return m[None]
    m = np.zeros(shape, np.uint8)
    m[shape[0] // 2, shape[1] // 2] = 1
    m[2, 3] = 2
    return np.stack([m, class_blobs(sum(shape) + R, shape, 3, sigma=4.0)])


@pytest.mark.parametrize("shape", SMALL_PLANES + TILE_EDGES)
def test_boundary_shapes_at_every_radius(programs, tmp_path, shape):
    """Every shape of test_small_and_thin_planes and test_tile_edges at each radius of ALL_RADII, dist2 and out written together.
    Of these only (16, 16) and (64, 64) take the aligned form."""
    proves = False
    for R in ALL_RADII:
        want = _boundary(programs, tmp_path, _boundary_input(shape, R), R)
        proves = proves or has_both(want)
    assert proves or shape == (1, 1), "every expected result is all FAR or all band"


@pytest.mark.parametrize("form", ["dist2", "out"])
@pytest.mark.parametrize("shape", [(2, 70, 92), (1, 65, 63)])
def test_boundary_output_forms(programs, tmp_path, shape, form):
    """The two forms with a null output ("both" is every other case), in the aligned form (W = 92) and the byte form (W = 63), at
    one radius of each apron size."""
    m = class_blobs(4, shape, 3, sigma=4.0)
    for R, label in ((4, 255), (5, 0), (16, 1), (32, 255)):
        _boundary(programs, tmp_path, m, R, label, form)


@pytest.mark.parametrize("offsets", [(1, 0, 0), (0, 0, 3), (0, 2, 0), (0, 4, 0), (1, 2, 3)], ids=lambda o: "-".join(map(str, o)))
def test_boundary_behind_unaligned_addresses(programs, tmp_path, offsets):
    """(2, 40, 64): W is a multiple of 4; the mask at an odd byte, out behind 3 bytes, dist2 2-byte (and 4-byte) but not 8-byte
    aligned, and all three at once -- each must take the byte form, whose widest access is an int16."""
    m = class_blobs(3, (2, 40, 64), 3)
    for R in (2, 5):
        assert has_both(_boundary(programs, tmp_path, m, R, offsets=offsets))


@pytest.mark.parametrize("shape", LONG_THIN, ids=lambda s: "%dx%d" % s)
def test_boundary_long_thin_planes(programs, tmp_path, shape):
    """The sides of 65535 of tests/test_gpu_extents.py at its two radii: the 8-px and the 32-px apron."""
    for R in (5, 32):
        assert has_both(_boundary(programs, tmp_path, thin_masks(5 + shape[0] % 7, 1, *shape), R))


# ---- augment -------------------------------------------------------------------------------------------------------------------
# tests/test_gpu_augment.py::test_kernel_matches_the_rule, every side reduced to at most 130 px: 512 -> 128 with crop 480 -> 120,
# 1024 -> 130 with crop 480 -> 60 (or -> 128 uncropped), 256 -> 64 with crop 480 -> 120 (padding), 300 x 500 -> 78 x 130 with crop
# 480 -> 124; the last two are small enough as they are.
AUGMENT_SHAPES = [(128, 128, 3, 8, 120, "train"), (128, 128, 3, 3, 120, "center"), (128, 128, 1, 1, 120, "train"),
                  (130, 130, 3, 3, 60, "train"), (128, 128, 3, 1, None, "train"), (130, 130, 1, 1, 60, "center"),
                  (64, 64, 3, 8, 120, "train"), (64, 64, 1, 3, 120, "center"), (64, 64, 3, 1, 120, "center"),
                  (78, 130, 3, 3, 124, "train"), (130, 78, 1, 8, 124, "train"), (37, 91, 4, 3, 64, "train"), (64, 64, 2, 1, None, "train")]


def _augment(programs, tmp_path, img, mask, matrices, out_size, ignore=255):
    """fp32 and bf16 output against the rule, bit for bit; -> the expected label."""
    n, H, W, C = img.shape
    oh, ow = out_size
    scale, bias = gpu_augment._norm(C)
    want, want_label = rule_augment(img, mask, matrices, out_size, scale, bias, ignore=ignore)
    want_bf, _ = rule_augment(img, mask, matrices, out_size, scale, bias, ignore=ignore, bf16=True)
    for bf in (0, 1):
        tensors = [("img", "in", img, 0), ("mask", "in", mask, 0), ("matrices", "in", matrices, 0), ("scale", "in", scale, 0),
                   ("bias", "in", bias, 0), ("image_out", "out", n * C * oh * ow * (2 if bf else 4), 0), ("label_out", "out", n * oh * ow, 0)]
        got = run_case(programs, tmp_path, "gsa_augment_pairs", (n, H, W, C, oh, ow, bf, ignore), tensors)
        what = "augment %s -> %s %s" % (img.shape, out_size, "bf16" if bf else "fp32")
        if bf:
            assert not (want_bf.view(np.uint32) & 0xFFFF).any()
            _same(got["image_out"].view(np.uint16).reshape(want.shape), (want_bf.view(np.uint32) >> 16).astype(np.uint16), what)
        else:
            _same(got["image_out"].view(np.uint32).reshape(want.shape), want.view(np.uint32), what)
        _same(got["label_out"].reshape(want_label.shape), want_label, what + " label")
    return want_label


@pytest.mark.parametrize("H,W,C,n,crop,mode", AUGMENT_SHAPES)
def test_augment(programs, tmp_path, H, W, C, n, crop, mode):
    """Planned matrices in both modes, 1 to 4 channels, cropped, padded and uncropped, output sizes that are no multiple of the
    64 x 16 tile (120, 124, 60), fp32 and bf16."""
    from gan_segmentation_amd import augment
    assert max(H, W, crop or 0) <= 130
    img, mask = random_pair(100 + H + C + n, n, H, W, C, classes=5)
    matrices = augment.plan_matrices(7, 1000, n, H, W, crop, mode)
    label = _augment(programs, tmp_path, img, mask, matrices, augment.output_size(H, W, crop))
    if crop is not None and (H < crop or W < crop):
        assert np.any(label == 255) and np.any(label != 255), "a padded canvas must hold both source and border pixels"


def test_augment_on_hand_made_matrices(programs, tmp_path):
    """The matrices of test_kernel_on_hand_made_matrices: identity, mirror, half-pixel shifts, a zoom, a quarter turn, and
    coordinates far outside the source, whose clamped addresses must stay inside it."""
    H, W = 64, 96
    rows = np.array([[1, 0, 0, 0, 1, 0], [-1, 0, W - 1, 0, 1, 0], [1, 0, 0.5, 0, 1, 0.5], [1, 0, -0.5, 0, 1, 2.5],
                     [0.37, 0, 3.25, 0, 0.41, -7.75], [0, -1, 80.5, 1, 0, -10.25], [1, 0, 3e9, 0, 1, 0], [1, 0, 0, 0, 1, -3e38],
                     [1, 0, 2.0 ** 32, 0, 1, 2.0 ** 31], [4.0e7, 0, -1.0e7, 0, 1, 0]], np.float32)
    img, mask = random_pair(5, len(rows), H, W, 3)
    label = _augment(programs, tmp_path, img, mask, rows, (64, 96), ignore=7)
    assert np.array_equal(label[0], mask[0]) and np.array_equal(label[1], mask[1][:, ::-1]) and np.all(label[6:9] == 7)


def test_augment_smallest_source_and_an_output_size_that_is_no_multiple_of_4(programs, tmp_path):
    """A 1 x 1 x 1 source (a batch smaller than one 8-byte window) through a half-pixel shift; and an output of 8 x 10, which the
    entry refuses with GSA_ERR_INVALID before it writes a byte."""
    img, mask = random_pair(3, 1, 1, 1, 1)
    _augment(programs, tmp_path, img, mask, np.array([[1, 0, -1.5, 0, 1, -1.5]], np.float32), (4, 4))
    img, mask = random_pair(4, 1, 8, 8, 3)
    scale, bias = gpu_augment._norm(3)
    tensors = [("img", "in", img, 0), ("mask", "in", mask, 0), ("matrices", "in", np.array([[1, 0, 0, 0, 1, 0]], np.float32), 0),
               ("scale", "in", scale, 0), ("bias", "in", bias, 0), ("image_out", "out", 3 * 8 * 10 * 4, 0), ("label_out", "out", 8 * 10, 0)]
    got = run_case(programs, tmp_path, "gsa_augment_pairs", (1, 8, 8, 3, 8, 10, 0, 255), tensors, expect=-1)
    assert (got["image_out"] == FILL).all() and (got["label_out"] == FILL).all()


# ---- photometric ---------------------------------------------------------------------------------------------------------------
PHOTOMETRIC_SHAPES = [(4, 4, 1, 1), (5, 7, 3, 2), (37, 91, 4, 3), (64, 64, 2, 1)]


def _photometric(programs, tmp_path, img, rows, seed, first, offsets=(0, 0)):
    n, H, W, C = img.shape
    tensors = [("img", "in", img, offsets[0]), ("params", "in", rows, 0), ("out", "out", img.size, offsets[1])]
    got = run_case(programs, tmp_path, "gsa_photometric", (n, H, W, C, seed, first), tensors)["out"].reshape(img.shape)
    _same(got, rule_photometric(img, rows, seed, first), "photometric %s offsets %s" % (img.shape, offsets))
    return got


@pytest.mark.parametrize("H,W,C,n", PHOTOMETRIC_SHAPES)
def test_photometric(programs, tmp_path, H, W, C, n):
    """Blur, colour and noise all on (from three samples on, one without blur and one without noise, as in the GPU tests)."""
    img = random_images(H + W + C, n, H, W, C)
    got = _photometric(programs, tmp_path, img, gpu_photometric._rows(n, 7, 1000), 7, 1000)
    assert not np.array_equal(got, img)


@pytest.mark.parametrize("H,W,C,n", gpu_photometric._seam_shapes())
def test_photometric_tile_seams(programs, tmp_path, H, W, C, n):
    img = random_images(H * W + C, n, H, W, C)
    _photometric(programs, tmp_path, img, gpu_photometric._rows(n, 3, 50), 3, 50)


@pytest.mark.parametrize("H,W", PHOTOMETRIC_THIN, ids=lambda v: str(v))
def test_photometric_long_thin_planes(programs, tmp_path, H, W, C=3):
    """A side of 65535 beside the smallest side the op takes, as tests/test_gpu_extents.py runs it, one sample of three channels."""
    img = random_images(3, 1, H, W, C)
    _photometric(programs, tmp_path, img, gpu_photometric._rows(1, 7, 1000), 7, 1000)


def test_photometric_saturation(programs, tmp_path):
    rng = np.random.default_rng(2)
    img = (rng.integers(0, 2, (2, 20, 33, 4)) * 255).astype(np.uint8)
    rows = np.stack([row(alpha=1.2, offset=(60, -60, 60, -60)), row(alpha=1.2, offset=(-60, 60, -60, 60))])
    got = _photometric(programs, tmp_path, img, rows, 0, 0)
    assert np.array_equal(got[0, ..., 0], np.where(img[0, ..., 0] == 0, 60, 255)) and np.array_equal(got[0, ..., 1], np.where(img[0, ..., 1] == 0, 0, 246))


def test_photometric_zero_limits_return_the_input_bytes(programs, tmp_path):
    """The path that skips the LDS stages and reads its source dwords directly."""
    from gan_segmentation_amd import photometric as ph
    for shape in ((2, 37, 91, 3), (1, 64, 64, 4), (3, 4, 5, 1)):
        img = random_images(5, *shape)
        rows = ph.photometric_plan(8, 70, shape[0], **ph.ZERO_LIMITS)
        assert np.array_equal(_photometric(programs, tmp_path, img, rows, 8, 70), img)


@pytest.mark.parametrize("offsets", [(1, 0), (0, 1), (3, 3), (1, 3)], ids=lambda o: "-".join(map(str, o)))
def test_photometric_behind_unaligned_addresses(programs, tmp_path, offsets):
    """img and out behind 1 and 3 bytes, with and without blur: the kernel's dword accesses are unaligned by design (memcpy) and
    must stay inside the batch at both of its ends."""
    img = random_images(12, 3, 21, 30, 3)
    _photometric(programs, tmp_path, img, gpu_photometric._rows(3, 7, 1000), 7, 1000, offsets)


# ---- the entry checks these units share (csrc/gsa_plane.h) -----------------------------------------------------------------------
def _entry(programs, tmp_path, entry, n, H, W, nbytes, expect):
    """One call that must end before the launch: `nbytes` of mask, outputs of the sizes that go with them, every output byte
    still FILL afterwards."""
    mask = np.zeros(nbytes, np.uint8)
    if entry == "gsa_mask_morph":
        scalars, tensors = (n, H, W), [("mask", "in", mask, 0), ("out", "out", nbytes, 0)]
    else:
        scalars, tensors = (n, H, W, 2, 255), [("mask", "in", mask, 0), ("dist2", "out", 2 * nbytes, 0), ("out", "out", nbytes, 0)]
    got = run_case(programs, tmp_path, entry, scalars, tensors, expect=expect)
    for name, part in got.items():
        assert (part == FILL).all(), "%s n %d H %d W %d: %s was written to" % (entry, n, H, W, name)


@pytest.mark.parametrize("entry", ["gsa_mask_morph", "gsa_mask_boundary"])
def test_extents_past_65535_are_refused(programs, tmp_path, entry):
    _entry(programs, tmp_path, entry, 1, 65536, 1, 65536, -1)
    _entry(programs, tmp_path, entry, 1, 1, 65536, 65536, -1)


def test_an_empty_batch_of_the_largest_planes_is_ok_and_writes_nothing(programs, tmp_path):
    """n = 0 at the largest extents each entry takes.  gsa_mask_morph takes 65535 x 65535; gsa_mask_boundary keeps plane-local
    indices in 32 bits and refuses H * W >= 2^31 whatever n is, so its largest plane here is 65535 x 32768 = 2^31 - 32768 pixels."""
    _entry(programs, tmp_path, "gsa_mask_morph", 0, 65535, 65535, 8, 0)
    _entry(programs, tmp_path, "gsa_mask_boundary", 0, 65535, 32768, 8, 0)
    _entry(programs, tmp_path, "gsa_mask_boundary", 0, 65535, 65535, 8, -1)
    _entry(programs, tmp_path, "gsa_mask_boundary", 0, 65535, 32769, 8, -1)


def test_mask_morph_refuses_a_grid_of_2_to_the_24_tiles(programs, tmp_path):
    """n = 2^24 planes of 1 x 1: one tile each, exactly the ceiling, 16 MiB per tensor -- refused (not split) before a byte is
    written.  One plane fewer would be launched."""
    _entry(programs, tmp_path, "gsa_mask_morph", 1 << 24, 1, 1, 1 << 24, -1)


def test_photometric_refuses_a_plane_no_larger_than_its_blur_radius(programs, tmp_path):
    """H = 3 = the blur radius: refused on shape grounds, as W = 3 is."""
    for H, W in ((3, 8), (8, 3)):
        img = random_images(1, 1, H, W, 3)
        tensors = [("img", "in", img, 0), ("params", "in", gpu_photometric._rows(1, 7, 1000), 0), ("out", "out", img.size, 0)]
        got = run_case(programs, tmp_path, "gsa_photometric", (1, H, W, 3, 7, 1000), tensors, expect=-1)
        assert (got["out"] == FILL).all()
