"""csrc/gsa_resize.hip on the HOST under AddressSanitizer + UBSan and under ThreadSanitizer, as tests/test_host_emu_refine.py runs the
refinement (DESIGN.md sections 19 and 27): the unit is compiled unedited with g++ against tools/host_emu/hip/hip_runtime.h and linked,
with test_host_emu's four, into two stand-alone programs of this module's own -- tools/host_emu/emu_run.cpp with -DGSA_EMU_RESIZE,
which adds the gsa_pair_resize entry to the driver (independent of the other two guards).  ``run_case`` and the build flags are
test_host_emu's.

Every case is held to exit status 0 with the expected entry status, no sanitizer report, inputs unchanged, and every output byte
equal to tests/resize_ref.py -- the small shapes of tests/test_gpu_resize.py.  Overlapping ranges cannot be written as a case (every
tensor is a heap block of its own); the GPU tests refuse them through views of one buffer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import resize_ref as ref
from tests import test_host_emu as emu
from tests.test_host_emu import COMMON, SANITIZERS, run_case

FILL = emu.FILL
UNITS = emu.UNITS + ["gsa_resize.hip"]
MODES = {"vote": 0, "nearest": 1}


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """test_host_emu.build_programs with the resize's unit and the driver's guarded branch."""
    out = tmp_path_factory.mktemp("host_emu_resize")
    gxx = shutil.which("g++")
    assert gxx, "g++ is not on the PATH: the host emulation needs g++ with its static sanitizer runtimes"
    jobs = {}
    for name, flags in SANITIZERS.items():
        exe = os.path.join(str(out), "emu_resize_" + name)
        cmd = ([gxx] + COMMON + flags + ["-DGSA_EMU_RESIZE", "-I", emu.EMU, "-x", "c++"] + [os.path.join(emu.CSRC, u) for u in UNITS]
               + [os.path.join(emu.EMU, "emu_run.cpp"), "-o", exe])
        jobs[name] = (exe, cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    built = {}
    for name, (exe, cmd, proc) in jobs.items():
        log = proc.communicate()[0]
        assert proc.returncode == 0 and os.path.exists(exe), "building the %s program failed:\n%s\n%s" % (name, " ".join(cmd), log[-4000:])
        built[name] = exe
    return built


def _resize(programs, tmp_path, img, mask, size, mode="vote", offsets=(0, 0, 0, 0)):
    """One call; img or mask may be None (a null pair).  Every output byte against the rule."""
    first = img if img is not None else mask
    n, H, W = first.shape[:3]
    C = img.shape[3] if img is not None else 1
    h, w = size
    want_img, want_mask = ref.resize_pair(img, mask, size, mode)
    tensors = [("img", "in", img, offsets[0]) if img is not None else ("img", "null", None, 0),
               ("mask", "in", mask, offsets[1]) if mask is not None else ("mask", "null", None, 0),
               ("img_out", "out", want_img.size, offsets[2]) if img is not None else ("img_out", "null", None, 0),
               ("mask_out", "out", want_mask.size, offsets[3]) if mask is not None else ("mask_out", "null", None, 0)]
    got = run_case(programs, tmp_path, "gsa_pair_resize", (n, H, W, C, h, w, MODES[mode]), tensors)
    for name, want in (("img_out", want_img), ("mask_out", want_mask)):
        if want is None:
            assert name not in got
            continue
        out = got[name].reshape(want.shape)
        bad = np.argwhere(out != want)
        assert not len(bad), "resize %s -> %s C %d %s offsets %s: %d of %d bytes of %s differ from the rule, first at %s: %d instead of %d" % (
            (H, W), size, C, mode, offsets, len(bad), want.size, name, tuple(bad[0]), out[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("shape,size", ref.SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes(programs, tmp_path, shape, size):
    """Two samples, three channels, both mask modes."""
    H, W = shape
    img, mask = ref.random_pair(H + W, 2, H, W, 3)
    _resize(programs, tmp_path, img, mask, size)
    _resize(programs, tmp_path, img, mask, size, "nearest")


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_channels_and_every_mask_value(programs, tmp_path, C):
    """(33, 47) takes the byte form for every C but 4; (32, 48) the dword form for all."""
    for (H, W), size in (((33, 47), (16, 16)), ((32, 48), (10, 13))):
        img = ref.random_pair(C, 2, H, W, C)[0]
        mask = ref.every_value_mask(C, 2, H, W)
        _resize(programs, tmp_path, img, mask, size)
        _resize(programs, tmp_path, img, mask, size, "nearest")


def test_ties_by_hand(programs, tmp_path):
    for mask, size, want in ref.hand_cases():
        assert np.array_equal(ref.resize_mask(mask, size), want)
        _resize(programs, tmp_path, None, mask, size)


def test_image_only_and_mask_only(programs, tmp_path):
    img, mask = ref.random_pair(5, 2, 40, 72, 3)
    _resize(programs, tmp_path, img, None, (17, 30))
    _resize(programs, tmp_path, None, mask, (17, 30))
    _resize(programs, tmp_path, None, mask, (17, 30), "nearest")


@pytest.mark.parametrize("which", [0, 1, 2, 3, None], ids=["img", "mask", "img_out", "mask_out", "all"])
def test_behind_unaligned_addresses(programs, tmp_path, which):
    """(2, 32, 64): both row pitches are multiples of 4; every tensor 1, 2 and 3 bytes into its block, one at a time and all at once
    (by different amounts).  An input off its dword takes the byte form, the other keeps the dword form."""
    for C in (3, 4):
        img, mask = ref.random_pair(11 + C, 2, 32, 64, C)
        for off in (1, 2, 3):
            offsets = tuple((off + k) % 4 for k in range(4)) if which is None else tuple(off if k == which else 0 for k in range(4))
            _resize(programs, tmp_path, img, mask, (12, 20), offsets=offsets)


def test_batches(programs, tmp_path):
    """n = 3 at (64, 80) -> (24, 28): several tiles a plane, several planes."""
    img, mask = ref.random_pair(9, 3, 64, 80, 3)
    _resize(programs, tmp_path, img, mask, (24, 28))


def test_a_window_of_several_chunks(programs, tmp_path):
    """Ratio 16 on both axes with four channels: 2052 bytes a staged image row, 11 rows a chunk, 129 rows under a tile."""
    img, mask = ref.random_pair(4, 1, 144, 528, 4)
    _resize(programs, tmp_path, img, mask, (9, 33))


# ---- status ------------------------------------------------------------------------------------------------------------------
def _status(programs, tmp_path, scalars, expect, null=(), nbytes=(8, 8, 8, 8)):
    """One call that must end before any launch: the outputs stay FILL."""
    tensors = []
    for name, size in zip(("img", "mask", "img_out", "mask_out"), nbytes):
        if name in null:
            tensors.append((name, "null", None, 0))
        elif name.endswith("_out"):
            tensors.append((name, "out", size, 0))
        else:
            tensors.append((name, "in", np.zeros(size, np.uint8), 0))
    got = run_case(programs, tmp_path, "gsa_pair_resize", scalars, tensors, expect=expect)
    for name, part in got.items():
        assert (part == FILL).all(), "%s: %s was written to" % (scalars, name)


def test_an_empty_batch_is_ok_whatever_else_is_passed(programs, tmp_path):
    _status(programs, tmp_path, (0, 16, 16, 3, 8, 8, 0), 0)
    _status(programs, tmp_path, (0, 70000, 0, 9, -1, 0, 7), 0)
    _status(programs, tmp_path, (0, 16, 16, 3, 8, 8, 0), 0, null=("img_out", "mask"))


@pytest.mark.parametrize("scalars", [(-1, 16, 16, 3, 8, 8, 0), (1, 16, 16, 0, 8, 8, 0), (1, 16, 16, 5, 8, 8, 0), (1, 16, 16, 3, 8, 8, 2), (1, 16, 16, 3, 8, 8, -1),
                                     (1, 0, 16, 3, 1, 8, 0), (1, 16, 0, 3, 8, 1, 0), (1, 16, 16, 3, 0, 8, 0), (1, 16, 16, 3, 8, 0, 0), (1, 16, 16, 3, 17, 8, 0),
                                     (1, 16, 16, 3, 8, 17, 0), (1, 65, 64, 3, 4, 4, 0), (1, 64, 65, 3, 4, 4, 0), (1, 65536, 16, 1, 65536, 16, 0),
                                     (1, 16, 65536, 1, 16, 65536, 0), (1, 4097, 4096, 1, 4097, 4096, 0)],
                         ids=lambda s: "-".join(map(str, s)))
def test_refusals(programs, tmp_path, scalars):
    """n < 0; C, mode and sizes outside their ranges; a ratio above 16; a plane of more than 2^24 pixels."""
    _status(programs, tmp_path, scalars, -1, nbytes=(768, 256, 768, 256))


@pytest.mark.parametrize("null", [("img",), ("img_out",), ("mask",), ("mask_out",), ("img", "mask_out"), ("img", "mask", "img_out", "mask_out")])
def test_a_half_null_pair_and_no_pair_are_refused(programs, tmp_path, null):
    _status(programs, tmp_path, (1, 16, 16, 3, 8, 8, 0), -1, null=null, nbytes=(768, 256, 192, 64))
