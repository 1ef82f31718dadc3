"""csrc/gsa_resize.h <-> the library's exports <-> its row of _lib.UNIT_SIGNATURES, as tests/test_scores_abi.py does for the header
before it, and the entry's argument checks, which need no device."""
import ctypes
import os

from gan_segmentation_amd import _lib
from tests.common import ctypes_kind, header_declarations

HEADER = "csrc/gsa_resize.h"
ENTRY = "gsa_pair_resize"


def _declared(header):
    """tests.common.header_declarations of a header below the package directory (it joins its argument to include/)."""
    return header_declarations(os.path.join("..", "gan-segmentation_amd", header))


def test_header_exports_and_unit_table_agree(hip_library):
    """The same names, every one exported, and bound with a result and arguments of the declared kinds, position by position."""
    assert HEADER in _lib.UNIT_SIGNATURES
    text, declared = _declared(HEADER)
    assert set(declared) == set(_lib.UNIT_SIGNATURES[HEADER]) == {ENTRY}
    assert 'extern "C"' in text and "GSA_RESIZE_H" in text
    lib, api = ctypes.CDLL(hip_library), _lib.Api(hip_library, "gsa_")
    for name, kinds in declared.items():
        assert hasattr(lib, name), "%s declared in %s but not exported" % (name, HEADER)
        fn = api.fn(name)
        assert (ctypes_kind(fn.restype), [ctypes_kind(t) for t in fn.argtypes]) == kinds, name
        assert _lib.load_library().fn(name) is not None
        assert not hasattr(api, name[len("gsa_"):]), "only the entries of include/gsa.h are attributes"
    assert declared[ENTRY] == ("i32", ["pointer"] + ["i32"] * 7 + ["pointer"] * 4)


def test_every_library_variant_exports_the_entry(hip_library):
    """The unit is in the Makefile's one UNITS line, so the experiments build exports it as well, and its header is a dependency of
    every .hip rule; the header is not under include/."""
    assert hasattr(ctypes.CDLL(hip_library), ENTRY)
    if os.path.exists(_lib.EXPERIMENTS_LIBRARY):
        assert _lib.Api(_lib.EXPERIMENTS_LIBRARY, "gsa_").fn(ENTRY) is not None
    csrc = os.path.dirname(_lib.HIP_LIBRARY)
    makefile = open(os.path.join(csrc, "Makefile")).read()
    (units,) = [line for line in makefile.splitlines() if line.startswith("UNITS =")]
    assert "gsa_resize" in units.split()
    assert makefile.count("gsa_scores.h gsa_resize.h") == 3, "the header is a dependency of every .hip rule"
    assert not os.path.exists(os.path.join(csrc, "..", "..", "include", "gsa_resize.h"))


def test_no_name_of_the_row_is_in_another_table():
    names = set(_lib.UNIT_SIGNATURES[HEADER])
    assert not names & {n for g in _lib.SIGNATURES.values() for n in g}
    assert not names & {n for g in _lib.EXTRA_SIGNATURES.values() for n in g}
    assert not names & {n for h, g in _lib.UNIT_SIGNATURES.items() if h != HEADER for n in g}
    assert HEADER not in _lib.SIGNATURES and HEADER not in _lib.EXTRA_SIGNATURES
    everything = [n for t in (_lib.SIGNATURES, _lib.EXTRA_SIGNATURES, _lib.UNIT_SIGNATURES) for g in t.values() for n in g]
    assert len(everything) == len(set(everything)), "a name is bound twice"


def test_entry_rejects_bad_arguments_before_touching_the_gpu(hip_library):
    """Argument validation of gsa_pair_resize happens on the host (no HIP call precedes it): fake pointers, no device.  No call with
    valid arguments and n > 0 is made here."""
    fn = _lib.load_library().fn(ENTRY)
    # img: 2 * 64 * 48 * 3 = 18432 bytes; mask: 6144; img_out: 2 * 16 * 24 * 3 = 2304; mask_out: 768
    good = dict(n=2, H=64, W=48, C=3, h=16, w=24, mode=0, img=1 << 20, mask=2 << 20, img_out=3 << 20, mask_out=4 << 20)

    def call(**kw):
        a = dict(good, **kw)
        return fn(None, a["n"], a["H"], a["W"], a["C"], a["h"], a["w"], a["mode"], a["img"], a["mask"], a["img_out"], a["mask_out"])

    i, m, io, mo = good["img"], good["mask"], good["img_out"], good["mask_out"]
    bad_cases = [dict(n=-1), dict(n=-2 ** 31), dict(H=0), dict(W=0), dict(H=-64), dict(h=0), dict(w=0), dict(h=-1), dict(w=-24),
                 dict(h=65), dict(w=49), dict(h=3), dict(w=2), dict(H=65, h=4), dict(W=49, w=3),
                 dict(H=65536, h=65536), dict(W=65536, w=65536), dict(H=4097, W=4096, h=4097, w=4096), dict(H=65535, W=257, h=65535, w=257),
                 dict(C=0), dict(C=5), dict(C=-1), dict(mode=2), dict(mode=-1),
                 dict(C=0, img=None, img_out=None), dict(mode=2, mask=None, mask_out=None),
                 dict(img=None), dict(img_out=None), dict(mask=None), dict(mask_out=None), dict(img=None, mask_out=None),
                 dict(img=None, img_out=None, mask=None, mask_out=None),
                 # an output over an input: its first byte, its last, and around them; an output over the other output
                 dict(img_out=i), dict(img_out=i + 18431), dict(img_out=i - 2303), dict(img_out=m), dict(img_out=m + 6143), dict(img_out=m - 2303),
                 dict(mask_out=m), dict(mask_out=m + 6143), dict(mask_out=m - 767), dict(mask_out=i), dict(mask_out=i + 18431), dict(mask_out=i - 767),
                 dict(mask_out=io), dict(mask_out=io + 2303), dict(mask_out=io - 767), dict(img_out=mo + 767)]
    for bad in bad_cases:
        assert call(**bad) == -1, bad
    assert call(n=0) == 0
    assert call(n=0, img=None, mask=None, img_out=None, mask_out=None) == 0
    assert call(n=0, H=0, W=-3, C=9, h=70000, w=0, mode=5, img_out=None) == 0
