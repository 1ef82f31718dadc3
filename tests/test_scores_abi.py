"""csrc/gsa_scores.h <-> the library's exports <-> its row of _lib.UNIT_SIGNATURES, as tests/test_loss_abi.py does for the header
before it, and the entry's argument checks, which need no device."""
import ctypes
import os
import re

from gan_segmentation_amd import _lib, score_ops
from tests.common import ctypes_kind, header_declarations

HEADER = "csrc/gsa_scores.h"
ENTRY = "gsa_score_histogram"


def _declared(header):
    """tests.common.header_declarations of a header below the package directory (it joins its argument to include/)."""
    return header_declarations(os.path.join("..", "gan-segmentation_amd", header))


def test_header_exports_and_unit_table_agree(hip_library):
    """The same names, every one exported, and bound with a result and arguments of the declared kinds, position by position."""
    assert HEADER in _lib.UNIT_SIGNATURES
    text, declared = _declared(HEADER)
    assert set(declared) == set(_lib.UNIT_SIGNATURES[HEADER]) == {ENTRY}
    assert 'extern "C"' in text and "GSA_SCORES_H" in text
    lib, api = ctypes.CDLL(hip_library), _lib.Api(hip_library, "gsa_")
    for name, kinds in declared.items():
        assert hasattr(lib, name), "%s declared in %s but not exported" % (name, HEADER)
        fn = api.fn(name)
        assert (ctypes_kind(fn.restype), [ctypes_kind(t) for t in fn.argtypes]) == kinds, name
        assert _lib.load_library().fn(name) is not None
        assert not hasattr(api, name[len("gsa_"):]), "only the entries of include/gsa.h are attributes"
    assert declared[ENTRY] == ("i32", ["pointer"] + ["i32"] * 4 + ["pointer"] * 3)


def test_header_macros_are_the_python_constants():
    text, _names = _declared(HEADER)
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(GSA_SCORE_[A-Z_]+)\s+(\d+)", text)}
    assert macros == {"GSA_SCORE_BINS": score_ops.SCORE_BINS, "GSA_SCORE_MAX_SHIFT": score_ops.SCORE_MAX_SHIFT,
                      "GSA_SCORE_MAX_CLASSES": score_ops.SCORE_MAX_CLASSES, "GSA_SCORE_STRETCH": score_ops.SCORE_STRETCH,
                      "GSA_SCORE_MAX_BLOCKS": score_ops.SCORE_MAX_BLOCKS}
    assert macros["GSA_SCORE_BINS"] == 1024 and macros["GSA_SCORE_MAX_SHIFT"] == 8 and macros["GSA_SCORE_MAX_CLASSES"] == 8
    assert macros["GSA_SCORE_STRETCH"] % 1024 == 0, "whole trips of 256 lanes x 4 pixels"
    assert (score_ops.MIN_CLASSES, score_ops.MAX_CLASSES) == (2, 8)
    # the header's comment says what the score is not, and the denormal mode the bins rest on
    flat = " ".join(open(os.path.join(os.path.dirname(_lib.HIP_LIBRARY), "gsa_scores.h")).read().replace(" * ", " ").split())
    assert "different score from the softmax probability" in flat and "FLOAT_DENORM_MODE_32 = 3" in flat


def test_every_library_variant_exports_the_entry(hip_library):
    """The unit is in the Makefile's one UNITS line, so the experiments build exports it as well; its header follows gsa_loss.h in
    the dependency list of every .hip rule, and the strings the other ABI tests count are still there three times each."""
    lib = ctypes.CDLL(hip_library)
    assert hasattr(lib, ENTRY)
    if os.path.exists(_lib.EXPERIMENTS_LIBRARY):
        assert _lib.Api(_lib.EXPERIMENTS_LIBRARY, "gsa_").fn(ENTRY) is not None
    makefile = open(os.path.join(os.path.dirname(_lib.HIP_LIBRARY), "Makefile")).read()
    (units,) = [line for line in makefile.splitlines() if line.startswith("UNITS =")]
    assert "gsa_scores" in units.split()
    assert makefile.count("gsa_loss.h gsa_scores.h") == 3, "the header is a dependency of every .hip rule"
    assert makefile.count("gsa_compare.h gsa_loss.h") == 3
    assert makefile.count("gsa_overlay.h gsa_refine.h") == 3 and makefile.count("gsa_refine.h gsa_compare.h") == 3


def test_no_name_of_the_row_is_in_another_table():
    names = set(_lib.UNIT_SIGNATURES[HEADER])
    assert not names & {n for g in _lib.SIGNATURES.values() for n in g}
    assert not names & {n for g in _lib.EXTRA_SIGNATURES.values() for n in g}
    assert not names & {n for h, g in _lib.UNIT_SIGNATURES.items() if h != HEADER for n in g}
    assert HEADER not in _lib.SIGNATURES and HEADER not in _lib.EXTRA_SIGNATURES
    everything = [n for t in (_lib.SIGNATURES, _lib.EXTRA_SIGNATURES, _lib.UNIT_SIGNATURES) for g in t.values() for n in g]
    assert len(everything) == len(set(everything)), "a name is bound twice"


def test_entry_rejects_bad_arguments_before_touching_the_gpu(hip_library):
    """Argument validation of gsa_score_histogram happens on the host (no HIP call precedes it): fake pointers, no device.  No call
    with valid arguments and n > 0 is made here."""
    fn = _lib.load_library().fn(ENTRY)
    # logits: 2 * 3 * 1000 floats = 24000 bytes from 1 << 20; labels: 2000 bytes from 2 << 20; rows: 2 * 3 * 2048 * 8 = 98304 bytes
    good = dict(n=2, K=3, HW=1000, shift=5, logits=1 << 20, labels=2 << 20, rows=8 << 20)

    def call(**kw):
        a = dict(good, **kw)
        return fn(None, a["n"], a["K"], a["HW"], a["shift"], a["logits"], a["labels"], a["rows"])

    z, y, r = good["logits"], good["labels"], good["rows"]
    bad_cases = [dict(n=-1), dict(n=-2 ** 31), dict(K=1), dict(K=0), dict(K=-3), dict(K=9), dict(K=64), dict(HW=0), dict(HW=-1),
                 dict(shift=-1), dict(shift=9), dict(shift=32),
                 dict(logits=None), dict(labels=None), dict(rows=None),
                 dict(logits=z + 2), dict(logits=z + 1), dict(logits=z + 3), dict(rows=r + 4), dict(rows=r + 1), dict(rows=r + 2),
                 # rows over the logits: their first word, their last, and around them; rows over the labels alike
                 dict(rows=z), dict(rows=z + 24000 - 8), dict(rows=z - 98304 + 8), dict(rows=z - 8, HW=1002),
                 dict(rows=y), dict(rows=y + 1992), dict(rows=y - 98304 + 8), dict(logits=r + 98304 - 4), dict(labels=r + 98303),
                 dict(n=2 ** 10, K=2, HW=2 ** 29), dict(n=2 ** 7, K=8, HW=2 ** 30), dict(n=2 ** 31 - 1, K=8, HW=2 ** 31 - 1),
                 dict(n=1, K=2, HW=2 ** 31 - 1, shift=9)]
    for bad in bad_cases:
        assert call(**bad) == -1, bad
    assert call(n=0) == 0
    assert call(n=0, logits=None, labels=None, rows=None) == 0
    assert call(n=0, K=0, HW=-3, shift=99, rows=3) == 0
