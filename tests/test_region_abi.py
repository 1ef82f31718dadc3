"""csrc/gsa_region.h <-> the library's exports <-> its row of _lib.UNIT_SIGNATURES, as tests/test_loss_abi.py does for the header
before it, and the entries' argument checks, which need no device."""
import ctypes
import os
import re

from gan_segmentation_amd import _lib, loss_ops
from tests.common import ctypes_kind, header_declarations

HEADER = "csrc/gsa_region.h"
ENTRY = "gsa_region_tversky"
SIZE = "gsa_region_workspace_bytes"


def _declared(header):
    """tests.common.header_declarations of a header below the package directory (it joins its argument to include/)."""
    return header_declarations(os.path.join("..", "gan-segmentation_amd", header))


def test_header_exports_and_unit_table_agree(hip_library):
    """The same names, every one exported, and bound with a result and arguments of the declared kinds, position by position."""
    assert HEADER in _lib.UNIT_SIGNATURES
    text, declared = _declared(HEADER)
    assert set(declared) == set(_lib.UNIT_SIGNATURES[HEADER]) == {ENTRY, SIZE}
    assert 'extern "C"' in text and "GSA_REGION_H" in text
    lib, api = ctypes.CDLL(hip_library), _lib.Api(hip_library, "gsa_")
    for name, kinds in declared.items():
        assert hasattr(lib, name), "%s declared in %s but not exported" % (name, HEADER)
        fn = api.fn(name)
        assert (ctypes_kind(fn.restype), [ctypes_kind(t) for t in fn.argtypes]) == kinds, name
        assert _lib.load_library().fn(name) is not None
        assert not hasattr(api, name[len("gsa_"):]), "only the entries of include/gsa.h are attributes"
    assert declared[SIZE] == ("i64", ["i32", "i32", "i32"])
    assert declared[ENTRY] == ("i32", ["pointer"] + ["i32"] * 3 + ["pointer"] * 3 + ["float"] * 3 + ["i32", "float", "i32"] + ["pointer"] * 5)


def test_header_macros_are_the_python_constants():
    text, _names = _declared(HEADER)
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(GSA_REGION_[A-Z_]+)\s+(\d+)", text)}
    assert macros == {"GSA_REGION_MAX_CLASSES": loss_ops.REGION_MAX_CLASSES, "GSA_REGION_MAX_BLOCKS": loss_ops.REGION_MAX_BLOCKS,
                      "GSA_REGION_SUMS": loss_ops.REGION_SUMS}
    assert macros["GSA_REGION_MAX_CLASSES"] == 16 and macros["GSA_REGION_MAX_BLOCKS"] == 512 and macros["GSA_REGION_SUMS"] == 3
    cap = macros["GSA_REGION_MAX_BLOCKS"]
    assert cap > 0 and cap & (cap - 1) == 0, "the block cap is a power of two"
    assert (loss_ops.SUM_I, loss_ops.SUM_P, loss_ops.SUM_G) == (0, 1, 2) and loss_ops.REGION_CLASSES == {"present": 0, "all": 1}


def test_every_library_variant_exports_the_entries(hip_library):
    """The unit is in the Makefile's one UNITS line, so the experiments build exports it as well; its header follows gsa_resize.h
    in the dependency list of every .hip rule, and the strings the other ABI tests count are still there three times each."""
    lib = ctypes.CDLL(hip_library)
    assert hasattr(lib, ENTRY) and hasattr(lib, SIZE)
    if os.path.exists(_lib.EXPERIMENTS_LIBRARY):
        exp = _lib.Api(_lib.EXPERIMENTS_LIBRARY, "gsa_")
        assert exp.fn(ENTRY) is not None and exp.fn(SIZE) is not None
    makefile = open(os.path.join(os.path.dirname(_lib.HIP_LIBRARY), "Makefile")).read()
    (units,) = [line for line in makefile.splitlines() if line.startswith("UNITS =")]
    assert "gsa_region" in units.split() and units.split()[-1] == "gsa_region"
    assert makefile.count("gsa_resize.h gsa_region.h") == 3, "the header is a dependency of every .hip rule"
    assert makefile.count("gsa_compare.h gsa_loss.h") == 3 and makefile.count("gsa_loss.h gsa_scores.h") == 3


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
    cap = loss_ops.REGION_MAX_BLOCKS
    for n in (0, 1, 3, 65536):
        for K in (2, 3, 8, 16):
            for HW in (1, 255, 256, 257, 1000, 256 * cap - 1, 256 * cap, 256 * cap + 1, 2 * 256 * cap + 3, 2 ** 31 - 1):
                assert fn(n, K, HW) == n * min(-(-HW // 256), cap) * 3 * K * 8, (n, K, HW)
    for n, K, HW in ((-1, 2, 10), (1, 2, 0), (1, 2, -5), (-2, 2, -2), (0, 2, 0), (1, 1, 10), (1, 0, 10), (1, -4, 10), (1, 17, 10), (0, 64, 10)):
        assert fn(n, K, HW) < 0, (n, K, HW)
    assert loss_ops.region_workspace_bytes(3, 8, 1000) == 3 * 4 * 3 * 8 * 8


def test_entry_rejects_bad_arguments_before_touching_the_gpu(hip_library):
    """Argument validation of gsa_region_tversky happens on the host (no HIP call precedes it): fake pointers, no device.  No call
    with valid arguments and n > 0 is made here."""
    fn = _lib.load_library().fn(ENTRY)
    inf, nan = float("inf"), float("nan")
    good = dict(n=2, K=3, HW=1000, logits=1 << 20, labels=2 << 20, cw=3 << 20, alpha=0.3, beta=0.7, smooth=1.0, mode=0, gs=1.0, acc=0,
                ws=6 << 20, sums=7 << 20, index=10 << 20, loss=8 << 20, dl=9 << 20)

    def call(**kw):
        a = dict(good, **kw)
        return fn(None, a["n"], a["K"], a["HW"], a["logits"], a["labels"], a["cw"], a["alpha"], a["beta"], a["smooth"], a["mode"],
                  a["gs"], a["acc"], a["ws"], a["sums"], a["index"], a["loss"], a["dl"])

    bad_cases = [dict(n=-1), dict(K=1), dict(K=0), dict(K=-3), dict(K=17), dict(K=64), dict(HW=0), dict(HW=-1),
                 dict(logits=None), dict(labels=None), dict(ws=None), dict(sums=None), dict(index=None), dict(loss=None),
                 dict(alpha=-0.1), dict(alpha=inf), dict(alpha=nan), dict(beta=-1.0), dict(beta=inf), dict(beta=nan),
                 dict(smooth=-1e-3), dict(smooth=inf), dict(smooth=nan), dict(alpha=0.0, beta=0.0),
                 dict(mode=-1), dict(mode=2), dict(gs=inf), dict(gs=-inf), dict(gs=nan),
                 dict(ws=(6 << 20) + 4), dict(ws=(6 << 20) + 1), dict(sums=(7 << 20) + 4), dict(sums=(7 << 20) + 2),
                 dict(logits=(1 << 20) + 2), dict(logits=(1 << 20) + 1), dict(cw=(3 << 20) + 2), dict(index=(10 << 20) + 1),
                 dict(loss=(8 << 20) + 2), dict(dl=(9 << 20) + 2), dict(dl=(9 << 20) + 3),
                 dict(n=2 ** 10, K=2, HW=2 ** 29), dict(n=2 ** 6, K=16, HW=2 ** 30), dict(n=2 ** 31 - 1, K=16, HW=2 ** 31 - 1),
                 # every one also without the optional pointers, and with accumulate set
                 dict(cw=None, dl=None, n=-1), dict(cw=None, dl=None, alpha=-1.0), dict(cw=None, dl=None, HW=0), dict(acc=1, mode=5)]
    for bad in bad_cases:
        assert call(**bad) == -1, bad
    assert call(n=0) == 0
    assert call(n=0, logits=None, labels=None, cw=None, ws=None, sums=None, index=None, loss=None, dl=None) == 0
    assert call(n=0, K=0, HW=-3, alpha=nan, mode=9, ws=3) == 0
