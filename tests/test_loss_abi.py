"""csrc/gsa_loss.h <-> the library's exports <-> its row of _lib.UNIT_SIGNATURES, as tests/test_compare_abi.py does for the header
before it, and the entries' argument checks, which need no device."""
import ctypes
import os
import re

from gan_segmentation_amd import _lib, loss_ops
from tests.common import ctypes_kind, header_declarations

HEADER = "csrc/gsa_loss.h"
ENTRY = "gsa_loss_softmax"
SIZE = "gsa_loss_workspace_bytes"


def _declared(header):
    """tests.common.header_declarations of a header below the package directory (it joins its argument to include/)."""
    return header_declarations(os.path.join("..", "gan-segmentation_amd", header))


def test_header_exports_and_unit_table_agree(hip_library):
    """The same names, every one exported, and bound with a result and arguments of the declared kinds, position by position."""
    assert HEADER in _lib.UNIT_SIGNATURES
    text, declared = _declared(HEADER)
    assert set(declared) == set(_lib.UNIT_SIGNATURES[HEADER]) == {ENTRY, SIZE}
    assert 'extern "C"' in text and "GSA_LOSS_H" in text
    lib, api = ctypes.CDLL(hip_library), _lib.Api(hip_library, "gsa_")
    for name, kinds in declared.items():
        assert hasattr(lib, name), "%s declared in %s but not exported" % (name, HEADER)
        fn = api.fn(name)
        assert (ctypes_kind(fn.restype), [ctypes_kind(t) for t in fn.argtypes]) == kinds, name
        assert _lib.load_library().fn(name) is not None
        assert not hasattr(api, name[len("gsa_"):]), "only the entries of include/gsa.h are attributes"
    assert declared[SIZE] == ("i64", ["i32", "i32"])
    assert declared[ENTRY] == ("i32", ["pointer"] + ["i32"] * 3 + ["pointer"] * 5 + ["float", "i32", "float"] + ["pointer"] * 4)


def test_header_macros_are_the_python_constants():
    text, _names = _declared(HEADER)
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(GSA_LOSS_[A-Z_]+)\s+(\d+)", text)}
    assert macros == {"GSA_LOSS_TABLE": loss_ops.LOSS_TABLE, "GSA_LOSS_MAX_BLOCKS": loss_ops.LOSS_MAX_BLOCKS,
                      "GSA_LOSS_SUMS": loss_ops.LOSS_SUMS}
    assert macros["GSA_LOSS_TABLE"] == 1026 and macros["GSA_LOSS_SUMS"] == 4
    cap = macros["GSA_LOSS_MAX_BLOCKS"]
    assert cap > 0 and cap & (cap - 1) == 0, "the block cap is a power of two"


def test_every_library_variant_exports_the_entries(hip_library):
    """The unit is in the Makefile's one UNITS line, so the experiments build exports it as well; its header follows gsa_compare.h
    in the dependency list of every .hip rule, and the strings the other ABI tests count are still there three times each."""
    lib = ctypes.CDLL(hip_library)
    assert hasattr(lib, ENTRY) and hasattr(lib, SIZE)
    if os.path.exists(_lib.EXPERIMENTS_LIBRARY):
        exp = _lib.Api(_lib.EXPERIMENTS_LIBRARY, "gsa_")
        assert exp.fn(ENTRY) is not None and exp.fn(SIZE) is not None
    makefile = open(os.path.join(os.path.dirname(_lib.HIP_LIBRARY), "Makefile")).read()
    (units,) = [line for line in makefile.splitlines() if line.startswith("UNITS =")]
    assert "gsa_loss" in units.split()
    assert makefile.count("gsa_compare.h gsa_loss.h") == 3, "the header is a dependency of every .hip rule"
    assert makefile.count("gsa_overlay.h gsa_refine.h") == 3 and makefile.count("gsa_refine.h gsa_compare.h") == 3


def test_no_name_of_the_row_is_in_another_table():
    names = set(_lib.UNIT_SIGNATURES[HEADER])
    assert not names & {n for g in _lib.SIGNATURES.values() for n in g}
    assert not names & {n for g in _lib.EXTRA_SIGNATURES.values() for n in g}
    assert not names & {n for h, g in _lib.UNIT_SIGNATURES.items() if h != HEADER for n in g}
    assert HEADER not in _lib.SIGNATURES and HEADER not in _lib.EXTRA_SIGNATURES
    everything = [n for t in (_lib.SIGNATURES, _lib.EXTRA_SIGNATURES, _lib.UNIT_SIGNATURES) for g in t.values() for n in g]
    assert len(everything) == len(set(everything)), "a name is bound twice"


def test_workspace_bytes(hip_library):
    fn = _lib.load_library().fn(SIZE)
    cap = loss_ops.LOSS_MAX_BLOCKS
    for n in (0, 1, 3, 65536):
        for HW in (1, 255, 256, 257, 1000, 256 * cap - 1, 256 * cap, 256 * cap + 1, 2 * 256 * cap + 3, 2 ** 31 - 1):
            assert fn(n, HW) == n * min(-(-HW // 256), cap) * 32, (n, HW)
    for n, HW in ((-1, 10), (1, 0), (1, -5), (-2, -2), (0, 0)):
        assert fn(n, HW) < 0, (n, HW)
    assert loss_ops.workspace_bytes(3, 1000) == 3 * 4 * 32


def test_entry_rejects_bad_arguments_before_touching_the_gpu(hip_library):
    """Argument validation of gsa_loss_softmax happens on the host (no HIP call precedes it): fake pointers, no device.  No call
    with valid arguments and n > 0 is made here."""
    fn = _lib.load_library().fn(ENTRY)
    inf, nan = float("inf"), float("nan")
    good = dict(n=2, K=3, HW=1000, logits=1 << 20, labels=2 << 20, cw=3 << 20, d2=4 << 20, tab=5 << 20, gamma=2.0, norm=2, gs=1.0,
                ws=6 << 20, sums=7 << 20, loss=8 << 20, dl=9 << 20)

    def call(**kw):
        a = dict(good, **kw)
        return fn(None, a["n"], a["K"], a["HW"], a["logits"], a["labels"], a["cw"], a["d2"], a["tab"], a["gamma"], a["norm"], a["gs"],
                  a["ws"], a["sums"], a["loss"], a["dl"])

    bad_cases = [dict(n=-1), dict(K=1), dict(K=0), dict(K=-3), dict(K=65), dict(HW=0), dict(HW=-1),
                 dict(logits=None), dict(labels=None), dict(ws=None), dict(sums=None), dict(loss=None),
                 dict(d2=None), dict(tab=None),
                 dict(gamma=0.5), dict(gamma=0.999), dict(gamma=-1.0), dict(gamma=8.5), dict(gamma=1e-30), dict(gamma=inf),
                 dict(gamma=-inf), dict(gamma=nan),
                 dict(norm=-1), dict(norm=3), dict(gs=inf), dict(gs=-inf), dict(gs=nan),
                 dict(ws=(6 << 20) + 4), dict(ws=(6 << 20) + 1), dict(sums=(7 << 20) + 4), dict(sums=(7 << 20) + 2),
                 dict(logits=(1 << 20) + 2), dict(logits=(1 << 20) + 1), dict(cw=(3 << 20) + 2), dict(tab=(5 << 20) + 1),
                 dict(loss=(8 << 20) + 2), dict(dl=(9 << 20) + 2), dict(dl=(9 << 20) + 3),
                 dict(d2=(4 << 20) + 1),
                 dict(n=2 ** 10, K=2, HW=2 ** 29), dict(n=2 ** 4, K=64, HW=2 ** 30), dict(n=2 ** 31 - 1, K=64, HW=2 ** 31 - 1),
                 # every one also without the optional pointers
                 dict(cw=None, d2=None, tab=None, dl=None, n=-1), dict(cw=None, d2=None, tab=None, dl=None, gamma=0.25),
                 dict(cw=None, d2=None, tab=None, dl=None, HW=0)]
    for bad in bad_cases:
        assert call(**bad) == -1, bad
    assert call(n=0) == 0
    assert call(n=0, logits=None, labels=None, cw=None, d2=None, tab=None, ws=None, sums=None, loss=None, dl=None) == 0
    assert call(n=0, K=0, HW=-3, gamma=nan, norm=9, ws=3) == 0
