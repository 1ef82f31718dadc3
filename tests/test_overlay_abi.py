"""csrc/gsa_overlay.h <-> the library's exports <-> _lib.EXTRA_SIGNATURES: what tests/test_abi_and_host.py
test_header_exports_and_table_agree does for the headers under include/ and _lib.SIGNATURES, for the one header and table that
live beside them (DESIGN.md section 21 says why), and the facts that placement leaves as they were."""
import ctypes
import os

from gan_segmentation_amd import _lib
from tests.common import ctypes_kind, header_declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "csrc/gsa_overlay.h"


def _declared(header):
    """tests.common.header_declarations of a header below the package directory (it joins its argument to include/)."""
    return header_declarations(os.path.join("..", "gan-segmentation_amd", header))


def test_header_exports_and_extra_table_agree(hip_library):
    """The same names, every one exported, and bound with a result and arguments of the declared kinds, position by position; the
    cached ``load_library()`` resolves every one too."""
    assert list(_lib.EXTRA_SIGNATURES) == [HEADER]
    text, declared = _declared(HEADER)
    assert set(declared) == set(_lib.EXTRA_SIGNATURES[HEADER]) == {"gsa_overlay"}
    assert 'extern "C"' in text and "GSA_OVERLAY_H" in text
    lib, api = ctypes.CDLL(hip_library), _lib.Api(hip_library, "gsa_")
    for name, kinds in declared.items():
        assert hasattr(lib, name), "%s declared in %s but not exported" % (name, HEADER)
        fn = api.fn(name)
        assert (ctypes_kind(fn.restype), [ctypes_kind(t) for t in fn.argtypes]) == kinds, name
        assert _lib.load_library().fn(name) is not None
        assert not hasattr(api, name[len("gsa_"):]), "only the entries of include/gsa.h are attributes"
    assert declared["gsa_overlay"] == ("i32", ["pointer"] + ["i32"] * 4 + ["pointer"] * 3 + ["i32"] * 2 + ["pointer"])


def test_every_library_variant_exports_the_entry(hip_library):
    """The unit is in the Makefile's one UNITS line, so the experiments build exports it as well."""
    assert hasattr(ctypes.CDLL(hip_library), "gsa_overlay")
    if os.path.exists(_lib.EXPERIMENTS_LIBRARY):
        assert _lib.Api(_lib.EXPERIMENTS_LIBRARY, "gsa_").fn("gsa_overlay") is not None


def test_the_public_directory_and_table_are_what_they_were():
    """Eleven headers under include/, the same eleven keys in SIGNATURES, 57 entries; no name is in both tables."""
    headers = sorted(os.listdir(os.path.join(ROOT, "include")))
    assert len(headers) == 11 and headers == sorted(_lib.SIGNATURES) and "gsa_overlay.h" not in headers
    names = [n for g in _lib.SIGNATURES.values() for n in g]
    assert len(names) == len(set(names)) == 57 == sum(len(header_declarations(h)[1]) for h in headers)
    assert not set(names) & {n for g in _lib.EXTRA_SIGNATURES.values() for n in g}
