"""The vector-memory waits of the lean kernels' item loops, read from the ISA hipcc emits (tools/isa_count.py --waits; DESIGN.md
section 4.1, round 7).  No device: the four lean units are compiled to gfx950 assembly with the Makefile's own FLAGS.

(a) No item loop of an instantiation the FFHQ step launches makes an item wait for the previous item's output: between a barrier and
    the first MFMA behind it there is no `s_waitcnt vmcnt(N)` whose N -- less what the iteration itself has issued since that
    barrier -- is below the stores and atomics an iteration can leave in flight.  The counter counts loads, LDS-DMA pieces, stores
    and atomics alike, so such a wait is a wait for the epilogue's stores to be acknowledged.  (A wait with N below what was issued
    since the barrier waits for one of those operations: the AdaIN coefficients on a sample change, read where they are used, once
    per sample and workgroup.  It is what the source asks for and is not counted.)  Instead every item loop retires its prefetched
    loads -- and its LDS-DMA pieces -- by a vmcnt(0) behind the MFMA phase, in front of the epilogue.
(b) The vector-memory operations per iteration that the loops are built around: 4 LDS-DMA pieces and NCH activation loads (+ 2 noise
    loads with the synthesis epilogue, + the coefficient loop's load with an AdaIN source) in the streamed Winograd kernels; 2 KB
    loads and 4 NT (+ NT with the shortcut) stores in subpixel_lean, 2 NT (+ 1) pieces where it streams its weights; post_dma's
    5 pieces + 4 stores per row behind counted waits of 20 and 40.  The streamed kernels no longer rest a counted wait on theirs
    (their pieces are retired by the vmcnt(0) of (a)); post_dma still does."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gan-segmentation_amd", "csrc")
UNITS = ("gsa_wino_lean", "gsa_sub_lean", "gsa_post_lean", "gsa_bf16_lean")      # not gsa_kernels: it takes two minutes

# what the FFHQ step (1024^2, fp32) launches from these units: profiles/r06_kernel_stats.csv
FFHQ_WINO = ["conv3x3_wino_lean<2, false, true, 1, 1, true, 1, false>", "conv3x3_wino_lean<2, true, false, 1, 1, true, 1, true>",
             "conv3x3_wino_lean<1, true, false, 1, 1, true, 1, false>", "conv3x3_wino_lean<2, false, true, 2, 2, true, 1, false>",
             "conv3x3_wino_lean<2, true, false, 2, 2, true, 1, false>", "conv3x3_wino_lean<1, true, false, 2, 2, true, 1, false>"]
# name -> (activation loads, noise loads, coefficient loads) per iteration
FFHQ_STREAM = {"conv3x3_wino_stream_pair<1, true>": (3, 2, 1), "conv3x3_wino_stream_pair<2, true>": (3, 0, 1),
               "conv3x3_wino_stream<1, true, 1, 0>": (6, 2, 1), "conv3x3_wino_stream<2, true, 1, 0>": (6, 0, 1)}
# name -> (NT, SC, AFF, KB, WST)
FFHQ_SUB = {"subpixel_lean<2, 0, false, true, 1, true, false>": (2, False, True, 1, True),
            "subpixel_lean<1, 2, true, false, 2, false, false>": (1, True, False, 2, False),
            "subpixel_lean<2, 2, true, false, 1, true, false>": (2, True, False, 1, True),
            "subpixel_lean<1, 0, false, true, 2, false, false>": (1, False, True, 2, False),
            "subpixel_lean<2, 0, false, true, 1, false, false>": (2, False, True, 1, False)}
FFHQ_POST = ["post_dma<16, true>", "post_dma<32, true>"]


def _tool():
    spec = importlib.util.spec_from_file_location("isa_count", os.path.join(ROOT, "tools", "isa_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _makefile_vars():
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*=\s*(.+)$", text, re.M).group(1).split()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", text, re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    return hipcc, arch, flags


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    """{unit: waits report} of the four units, compiled side by side."""
    hipcc, arch, flags = _makefile_vars()
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa")
    procs = {u: subprocess.Popen([hipcc, "--offload-arch=" + arch] + flags + ["--cuda-device-only", "-S", os.path.join(CSRC, u + ".hip"),
                                  "-o", str(out / (u + ".s"))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for u in UNITS}
    for u, pr in procs.items():
        log = pr.communicate()[0]
        assert pr.returncode == 0, "%s: %s" % (u, log[-3000:])
    tool = _tool()
    rep = {}
    for u in UNITS:
        src = (out / (u + ".s")).read_text()
        rep[u] = {k["name"].replace("lean::", ""): k for k in tool.waits_report(src)}
        if u == "gsa_post_lean":
            rep[u] = {k["name"].replace("lean::", ""): k for k in tool.waits_report(src, dma_loops=True)}
    rep["tool"] = tool
    return rep


def _loops(reports, unit, name):
    assert name in reports[unit], "%s: no item loop found in %s (kernels: %s)" % (unit, name, sorted(reports[unit])[:40])
    loops = reports[unit][name]["loops"]
    assert loops, name
    return loops


@pytest.mark.parametrize("unit,name", [("gsa_wino_lean", n) for n in FFHQ_WINO + sorted(FFHQ_STREAM)] + [("gsa_sub_lean", n) for n in sorted(FFHQ_SUB)])
def test_no_item_waits_for_the_previous_items_stores(reports, unit, name):
    tool = reports["tool"]
    for lp in _loops(reports, unit, name):
        in_flight = lp["per_iter"]["stores"] + lp["per_iter"]["atomics"]
        for w in lp["waits"]:
            print(name, lp["head"], "vmcnt(%d)" % w["n"], "top" if w["top"] else "", {k: w[k] for k in ("loads", "dma", "stores", "atomics")}, "in flight", in_flight)
        bad = tool.false_store_waits(lp)
        assert not bad, "%s, loop %s: vmcnt(%s) in front of the item's staging with %d stores and atomics of the previous item in flight" % (
            name, lp["head"], ", ".join(str(w["n"]) for w in bad), in_flight)
        behind = [w for w in lp["waits"] if not w["top"] and w["n"] == 0 and w["stores"] + w["atomics"] == 0]
        assert behind, "%s, loop %s: no vmcnt(0) behind the MFMA phase and in front of the epilogue's stores" % (name, lp["head"])


@pytest.mark.parametrize("name", sorted(FFHQ_STREAM))
def test_streamed_winograd_loop_operations(reports, name):
    nch, noise, coef = FFHQ_STREAM[name]
    synth = noise != 0
    for lp in _loops(reports, "gsa_wino_lean", name):
        s = lp["static"]
        print(name, lp["head"], s, [w["n"] for w in lp["waits"]])
        assert s["dma"] == 4, (name, lp["head"], s)
        assert s["loads"] == nch + noise + coef, (name, lp["head"], s)
        assert s["stores"] == 4 and s["atomics"] in ((0, 8) if synth else (0,)), (name, lp["head"], s)
        assert all(w["n"] == 0 for w in lp["waits"]), "%s, loop %s: a counted wait is back: %s" % (name, lp["head"], [w["n"] for w in lp["waits"]])


@pytest.mark.parametrize("name", sorted(FFHQ_SUB))
def test_subpixel_loop_operations(reports, name):
    nt, sc, aff, kb, wst = FFHQ_SUB[name]
    for lp in _loops(reports, "gsa_sub_lean", name):
        s = lp["static"]
        print(name, lp["head"], s, [w["n"] for w in lp["waits"]])
        assert s["loads"] == 2 * kb + (1 if aff else 0), (name, lp["head"], s)
        assert s["stores"] == 4 * nt + (nt if sc else 0), (name, lp["head"], s)
        assert s["dma"] == ((2 * nt + (1 if sc else 0)) if wst else 0), (name, lp["head"], s)
        assert all(w["n"] == 0 for w in lp["waits"]), "%s, loop %s: a counted wait is back: %s" % (name, lp["head"], [w["n"] for w in lp["waits"]])


@pytest.mark.parametrize("name", FFHQ_POST)
def test_post_dma_row_operations(reports, name):
    """Four rows per trip of the row loop: 5 LDS-DMA pieces and 4 stores each, behind the counted waits vmcnt(20) (the band's first five
    rows) and vmcnt(40) -- the 5 + 4 operations of each of the four rows between a row's pieces and its use, and 4 stores more."""
    loops = _loops(reports, "gsa_post_lean", name)
    rows = [lp for lp in loops if lp["static"]["stores"]]
    assert len(rows) == 1, [lp["static"] for lp in loops]
    s = rows[0]["static"]
    print(name, s, [w["n"] for w in rows[0]["waits"]])
    assert (s["dma"], s["stores"], s["loads"], s["atomics"]) == (4 * 5, 4 * 4, 0, 0), s
    assert sorted({w["n"] for w in rows[0]["waits"]}) == [20, 40], [w["n"] for w in rows[0]["waits"]]
