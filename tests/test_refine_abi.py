"""csrc/gsa_refine.h <-> the library's exports <-> its row of _lib.UNIT_SIGNATURES: what tests/test_overlay_abi.py does for the
overlay's header and EXTRA_SIGNATURES, for the first header of the table that later features add rows to.
The table's list of keys is deliberately NOT pinned here: a later header brings a test of its own."""
import ctypes
import os

from gan_segmentation_amd import _lib
from tests.common import ctypes_kind, header_declarations

HEADER = "csrc/gsa_refine.h"
ENTRY = "gsa_mask_refine"


def _declared(header):
    """tests.common.header_declarations of a header below the package directory (it joins its argument to include/)."""
    return header_declarations(os.path.join("..", "gan-segmentation_amd", header))


def test_header_exports_and_unit_table_agree(hip_library):
    """The same names, every one exported, and bound with a result and arguments of the declared kinds, position by position; the
    cached ``load_library()`` resolves every one too."""
    assert HEADER in _lib.UNIT_SIGNATURES
    text, declared = _declared(HEADER)
    assert set(declared) == set(_lib.UNIT_SIGNATURES[HEADER]) == {ENTRY}
    assert 'extern "C"' in text and "GSA_REFINE_H" in text
    lib, api = ctypes.CDLL(hip_library), _lib.Api(hip_library, "gsa_")
    for name, kinds in declared.items():
        assert hasattr(lib, name), "%s declared in %s but not exported" % (name, HEADER)
        fn = api.fn(name)
        assert (ctypes_kind(fn.restype), [ctypes_kind(t) for t in fn.argtypes]) == kinds, name
        assert _lib.load_library().fn(name) is not None
        assert not hasattr(api, name[len("gsa_"):]), "only the entries of include/gsa.h are attributes"
    assert declared[ENTRY] == ("i32", ["pointer"] + ["i32"] * 6 + ["pointer"] * 4)


def test_every_library_variant_exports_the_entry(hip_library):
    """The unit is in the Makefile's one UNITS line, so the experiments build exports it as well."""
    assert hasattr(ctypes.CDLL(hip_library), ENTRY)
    if os.path.exists(_lib.EXPERIMENTS_LIBRARY):
        assert _lib.Api(_lib.EXPERIMENTS_LIBRARY, "gsa_").fn(ENTRY) is not None
    makefile = open(os.path.join(os.path.dirname(_lib.HIP_LIBRARY), "Makefile")).read()
    (units,) = [line for line in makefile.splitlines() if line.startswith("UNITS =")]
    assert "gsa_refine" in units.split()
    assert makefile.count("gsa_overlay.h gsa_refine.h") == 3, "the header is a dependency of every .hip rule"


def test_no_name_of_the_row_is_in_another_table():
    names = set(_lib.UNIT_SIGNATURES[HEADER])
    assert not names & {n for g in _lib.SIGNATURES.values() for n in g}
    assert not names & {n for g in _lib.EXTRA_SIGNATURES.values() for n in g}
    assert HEADER not in _lib.SIGNATURES and HEADER not in _lib.EXTRA_SIGNATURES
    everything = [n for t in (_lib.SIGNATURES, _lib.EXTRA_SIGNATURES, _lib.UNIT_SIGNATURES) for g in t.values() for n in g]
    assert len(everything) == len(set(everything)), "a name is bound twice"


def test_entry_rejects_bad_arguments_before_touching_the_gpu(hip_library):
    """Argument validation of gsa_mask_refine happens on the host (no HIP call precedes it): fake pointers, no device."""
    fn = _lib.load_library().fn(ENTRY)
    good = dict(n=2, H=32, W=48, C=3, K=3, R=3, img=1 << 20, mask=2 << 20, tables=3 << 20, out=4 << 20)
    size = 2 * 32 * 48

    def call(**kw):
        a = dict(good, **kw)
        return fn(None, a["n"], a["H"], a["W"], a["C"], a["K"], a["R"], a["img"], a["mask"], a["tables"], a["out"])

    for bad in (dict(n=-1), dict(H=0), dict(W=0), dict(H=65536), dict(W=65536), dict(H=65535, W=65535), dict(H=32768, W=65535),
                dict(C=0), dict(C=5), dict(K=1), dict(K=9), dict(R=0), dict(R=6), dict(img=None), dict(mask=None), dict(tables=None), dict(out=None),
                dict(out=1 << 20), dict(out=(1 << 20) + 3 * size - 1), dict(out=(1 << 20) - size + 1), dict(out=2 << 20), dict(out=(2 << 20) + size - 1),
                dict(out=(3 << 20) + 376), dict(out=(3 << 20) - size + 1), dict(n=1 << 14, H=2048, W=2048, img=1 << 40, mask=1 << 45, out=1 << 50)):
        assert call(**bad) == -1, bad
    assert call(n=0) == 0 and call(n=0, img=None, mask=None, tables=None, out=None) == 0 and call(n=0, H=0, C=9, K=0, R=77) == 0
