"""csrc/gsa_compare.h <-> the library's exports <-> its row of _lib.UNIT_SIGNATURES, as tests/test_refine_abi.py does for the first
header of that table, and the entry's argument checks, which need no device."""
import ctypes
import os

from gan_segmentation_amd import _lib, mask_ops
from tests.common import ctypes_kind, header_declarations

HEADER = "csrc/gsa_compare.h"
ENTRY = "gsa_mask_compare"


def _declared(header):
    """tests.common.header_declarations of a header below the package directory (it joins its argument to include/)."""
    return header_declarations(os.path.join("..", "gan-segmentation_amd", header))


def test_header_exports_and_unit_table_agree(hip_library):
    """The same names, every one exported, and bound with a result and arguments of the declared kinds, position by position; the
    cached ``load_library()`` resolves every one too."""
    assert HEADER in _lib.UNIT_SIGNATURES
    text, declared = _declared(HEADER)
    assert set(declared) == set(_lib.UNIT_SIGNATURES[HEADER]) == {ENTRY}
    assert 'extern "C"' in text and "GSA_COMPARE_H" in text
    lib, api = ctypes.CDLL(hip_library), _lib.Api(hip_library, "gsa_")
    for name, kinds in declared.items():
        assert hasattr(lib, name), "%s declared in %s but not exported" % (name, HEADER)
        fn = api.fn(name)
        assert (ctypes_kind(fn.restype), [ctypes_kind(t) for t in fn.argtypes]) == kinds, name
        assert _lib.load_library().fn(name) is not None
        assert not hasattr(api, name[len("gsa_"):]), "only the entries of include/gsa.h are attributes"
    assert declared[ENTRY] == ("i32", ["pointer"] + ["i32"] * 4 + ["pointer"] * 5)


def test_header_macros_are_the_python_constants():
    import re
    text, _declared_names = _declared(HEADER)
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(GSA_COMPARE_[A-Z_]+)\s+(\d+)", text)}
    assert macros == {"GSA_COMPARE_SLOTS": mask_ops.COMPARE_SLOTS, "GSA_COMPARE_BANDS": mask_ops.COMPARE_BANDS,
                      "GSA_COMPARE_ROW": mask_ops.COMPARE_ROW, "GSA_COMPARE_MAX_RADIUS": mask_ops.BOUNDARY_MAX_RADIUS}
    assert macros["GSA_COMPARE_ROW"] == 324 == macros["GSA_COMPARE_BANDS"] * macros["GSA_COMPARE_SLOTS"] ** 2


def test_every_library_variant_exports_the_entry(hip_library):
    """The unit is in the Makefile's one UNITS line, so the experiments build exports it as well; its header follows gsa_refine.h in
    the dependency list of every .hip rule."""
    assert hasattr(ctypes.CDLL(hip_library), ENTRY)
    if os.path.exists(_lib.EXPERIMENTS_LIBRARY):
        assert _lib.Api(_lib.EXPERIMENTS_LIBRARY, "gsa_").fn(ENTRY) is not None
    makefile = open(os.path.join(os.path.dirname(_lib.HIP_LIBRARY), "Makefile")).read()
    (units,) = [line for line in makefile.splitlines() if line.startswith("UNITS =")]
    assert "gsa_compare" in units.split()
    assert makefile.count("gsa_refine.h gsa_compare.h") == 3, "the header is a dependency of every .hip rule"


def test_no_name_of_the_row_is_in_another_table():
    names = set(_lib.UNIT_SIGNATURES[HEADER])
    assert not names & {n for g in _lib.SIGNATURES.values() for n in g}
    assert not names & {n for g in _lib.EXTRA_SIGNATURES.values() for n in g}
    assert not names & {n for h, g in _lib.UNIT_SIGNATURES.items() if h != HEADER for n in g}
    assert HEADER not in _lib.SIGNATURES and HEADER not in _lib.EXTRA_SIGNATURES
    everything = [n for t in (_lib.SIGNATURES, _lib.EXTRA_SIGNATURES, _lib.UNIT_SIGNATURES) for g in t.values() for n in g]
    assert len(everything) == len(set(everything)), "a name is bound twice"


def test_entry_rejects_bad_arguments_before_touching_the_gpu(hip_library):
    """Argument validation of gsa_mask_compare happens on the host (no HIP call precedes it): fake pointers, no device."""
    fn = _lib.load_library().fn(ENTRY)
    good = dict(n=2, H=32, W=48, R=2, target=1 << 20, pred=2 << 20, td=3 << 20, pd=4 << 20, rows=5 << 20)
    size, row_bytes = 2 * 32 * 48, 2 * 324 * 8

    def call(**kw):
        a = dict(good, **kw)
        return fn(None, a["n"], a["H"], a["W"], a["R"], a["target"], a["pred"], a["td"], a["pd"], a["rows"])

    for bad in (dict(n=-1), dict(H=0), dict(W=0), dict(H=65536), dict(W=65536), dict(H=65535, W=65535), dict(H=32768, W=65535),
                dict(R=-1), dict(R=33), dict(R=0), dict(R=0, td=None), dict(R=0, pd=None), dict(td=None), dict(pd=None), dict(td=None, pd=None),
                dict(target=None), dict(pred=None), dict(rows=None),
                dict(td=(3 << 20) + 1), dict(pd=(4 << 20) + 1), dict(td=(3 << 20) + 3, pd=(4 << 20) + 1),
                dict(rows=(5 << 20) + 4), dict(rows=(5 << 20) + 1), dict(rows=(5 << 20) + 2),
                dict(rows=1 << 20), dict(rows=(1 << 20) + size - 8), dict(rows=(1 << 20) - row_bytes + 8),
                dict(rows=2 << 20), dict(rows=(2 << 20) + size - 8), dict(rows=(2 << 20) - row_bytes + 8),
                dict(rows=3 << 20), dict(rows=(3 << 20) + 2 * size - 8), dict(rows=(3 << 20) - row_bytes + 8),
                dict(rows=4 << 20), dict(rows=(4 << 20) + 2 * size - 8), dict(rows=(4 << 20) - row_bytes + 8),
                dict(R=0, td=None, pd=None, rows=(2 << 20) + size - 8)):
        assert call(**bad) == -1, bad
    assert call(n=0) == 0 and call(n=0, target=None, pred=None, td=None, pd=None, rows=None) == 0 and call(n=0, H=0, W=-3, R=77, rows=3) == 0
