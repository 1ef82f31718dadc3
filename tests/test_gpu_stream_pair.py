"""The paired streamed-weight Winograd kernel (gsa_wino_lean.hip conv3x3_wino_stream_pair: one 8-wave workgroup stages each tile once for
two 16-channel output groups) at the smallest shapes at which it can go wrong, bit for bit against the C oracle.

GSA_WINO_PAIR is read once per process, so every case runs in a child process of its own, one child at a time: 2 = the paired kernel
wherever Cout % 32 == 0 (the default rule asks for a workgroup per CU, which no small shape gives), 0 = never, unset = the rule.  A child
builds the model, checks rgb, image, every feature, logits and mask of the two-call path against the oracle and generate_batch against
the two-call path (tests/test_gpu_output_forms.py's helpers), and reports the digests and the (layer, kernel) pairs of one profiled step
of each path; the parent asserts which streamed kernel ran where.

 S16c     512 channels at 16 px, batch 3: one tile per sample with all four borders, 32 blocks per tile, a coefficient reload and a
          statistics flush at every tile, 16 workgroup columns (g.16.conv_2).
 S32c     512 channels at 32 px, batch 3: four two-border tiles per sample, tile ranges that cross sample boundaries inside a workgroup,
          an odd number of items per workgroup (g.16 / g.32.conv_2).
 M64      64 channels at every level up to 64 px (M64 with fmap_base 2048), batch 2: interior tiles (the border-free staging path),
          nblk = 4, Cout = 64 (two columns: g.32 / g.64.conv_2), and the decoder's d.cvt_4 (EPI_DEC, 64 -> 32: exactly one pair) with an
          AdaIN source (generate_batch) and without one (the two-call path).
 fallback M128 with 64 channels up to 64 px (fmap_base 2048) and the decoder's 64 px level 48 wide: d.cvt_4 has Cout % 32 == 16 and keeps
          the four-wave kernel while every other streamed layer runs the paired one.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_WORKER = r'''
import hashlib
import json
import sys
sys.path.insert(0, ROOT_DIR)
import numpy as np
from oracle import binding
binding.build()
from gan_segmentation_amd import weights as W
from tests import test_gpu_output_forms as F
from tests.common import form_setup, unsaturated_colours, w_spread
from tests.dispatch_map import path_map

spec = json.loads(sys.argv[1])
batch = spec["batch"]
gcfg, gp, dcfg, dp, z, noise = form_setup(spec["form"], batch, 3, 2, **spec["overrides"])
for level, width in spec["widths"]:           # decoder widths, as tests.common.odd_setup sets them
    dcfg["features"][level] = width
if spec["widths"]:
    dp = W.synthetic_decoder_params(dcfg, seed=3)
setup = (gcfg, gp, dcfg, dp, z, noise)
o = binding.Oracle(gcfg, gp, dcfg, dp)
assert w_spread(o.mapping(np.random.default_rng(1).standard_normal((4, 512)).astype(np.float32))) > 0.0, "precondition: w must depend on z"
rgb, img, feats = o.generator(z, noise)
logits, mask = o.decoder(feats)
assert unsaturated_colours(img) == [0, 1, 2], "precondition: every colour needs bytes strictly between 0 and 255"
assert sorted(np.unique(mask).tolist()) == [0, 1], "precondition: both classes must occur in the oracle's mask"
case = {"setup": setup, "rgb": rgb, "img": img, "feats": feats, "logits": logits, "mask": mask}
gen = F._build(setup, batch)
got = F._check_against_oracle(gen, case, batch, spec["form"])
digest = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
out = {"digests": {k: digest(got[k]) for k in ("rgb", "img", "logits", "mask")},
       "pairs": {path: sorted(path_map(gen, path, z, noise, batch)) for path in ("two_call", "generate")}}
out["digests"].update({"feature_%d" % i: digest(f) for i, f in enumerate(got["feats"])})
print("PAIR_RESULT " + json.dumps(out))
'''

_M64 = dict(form="M64", overrides={"fmap_base": 2048}, widths=[], batch=2)
_SPECS = {
    "S16c": dict(form="S16c", overrides={}, widths=[], batch=3),
    "S32c": dict(form="S32c", overrides={}, widths=[], batch=3),
    "M64": _M64,
    "fallback": dict(form="M128", overrides={"fmap_base": 2048}, widths=[[4, 48]], batch=2),
}
_RESULTS = {}      # (case, GSA_WINO_PAIR or None) -> the child's report: a setting shared by two tests runs once


def _child(tmp_path, script_text, env_pair, args=(), timeout=600):
    script = tmp_path / "stream_pair_worker.py"
    script.write_text(script_text.replace("ROOT_DIR", repr(ROOT)))
    env = {k: v for k, v in os.environ.items() if k != "GSA_WINO_PAIR"}
    if env_pair is not None:
        env["GSA_WINO_PAIR"] = env_pair
    return subprocess.run([sys.executable, str(script)] + list(args), env=env, capture_output=True, text=True, timeout=timeout)


def _run(tmp_path, name, env_pair):
    key = (name, env_pair)
    if key not in _RESULTS:
        out = _child(tmp_path, _WORKER, env_pair, [json.dumps(_SPECS[name])])
        lines = [l for l in out.stdout.splitlines() if l.startswith("PAIR_RESULT ")]
        assert out.returncode == 0 and lines, "%s GSA_WINO_PAIR=%s: %s" % (name, env_pair, out.stdout[-800:] + out.stderr[-2500:])
        _RESULTS[key] = json.loads(lines[-1][len("PAIR_RESULT "):])
    return _RESULTS[key]


def _streamed(result, path):
    """{layer: "pair" | "four"} of the layers of one path that ran a streamed-weight lean kernel."""
    kinds = {}
    for layer, kernel in result["pairs"][path]:
        if "conv3x3_wino_stream_pair<" in kernel:
            kinds[layer] = "pair"
        elif "conv3x3_wino_stream<" in kernel:
            kinds[layer] = "four"
    return kinds


# what GSA_WINO_PAIR=2 must run: every streamed layer of these models has Cout % 32 == 0
_EXPECT = {
    "S16c": {"g.16.conv_2"},
    "S32c": {"g.16.conv_2", "g.32.conv_2"},
    "M64": {"g.32.conv_2", "g.64.conv_2", "d.cvt_4"},
}


@pytest.mark.parametrize("name", ["S16c", "S32c", "M64"])
def test_paired_kernel_matches_the_oracle(torch_cuda, tmp_path, name):
    """GSA_WINO_PAIR=2: the child's oracle comparison passed, and the paired kernel is what ran every streamed layer, on both paths."""
    r = _run(tmp_path, name, "2")
    for path in ("two_call", "generate"):
        kinds = _streamed(r, path)
        assert kinds == {layer: "pair" for layer in _EXPECT[name]}, "%s %s: %r" % (name, path, kinds)
    if name == "M64":      # both AFF instances of the decoder epilogue: the fused step reads the AdaIN source, the two-call path the exported feature
        cvt = {k for p in ("two_call", "generate") for layer, k in r["pairs"][p] if layer == "d.cvt_4"}
        assert len(cvt) == 2 and all("stream_pair<" in k for k in cvt), sorted(cvt)


def test_odd_group_count_keeps_the_four_wave_kernel(torch_cuda, tmp_path):
    """Cout = 48 (three groups): d.cvt_4 runs conv3x3_wino_stream and matches the oracle; the other streamed layers (64 -> 64 at 32 and
    64 px; g.128.conv_2 is 32 -> 32, the resident-panel kernel) run the paired kernel."""
    r = _run(tmp_path, "fallback", "2")
    for path in ("two_call", "generate"):
        kinds = _streamed(r, path)
        assert kinds == {"g.32.conv_2": "pair", "g.64.conv_2": "pair", "d.cvt_4": "four"}, "%s: %r" % (path, kinds)


@pytest.mark.parametrize("env_pair", ["0", None])
def test_neighbouring_settings_give_the_same_bytes(torch_cuda, tmp_path, env_pair):
    """M64 with the paired kernel off and under the default rule (which keeps these small layers on the four-wave kernel: fewer
    workgroups than CUs): the oracle's outputs again, the digests of GSA_WINO_PAIR=2, and no paired launch."""
    want = _run(tmp_path, "M64", "2")
    r = _run(tmp_path, "M64", env_pair)
    assert r["digests"] == want["digests"]
    for path in ("two_call", "generate"):
        assert _streamed(r, path) == {layer: "four" for layer in _EXPECT["M64"]}, "%s GSA_WINO_PAIR=%s: %r" % (path, env_pair, _streamed(r, path))


# tests/test_gpu_parity.py's worker: ffhq 1024^2, batch 4, bench.py's inputs
_SWITCH_WORKER = r'''
import sys
sys.path.insert(0, ROOT_DIR)
from tests.common import bench_setup, golden_bench_outputs, pair_digest
from gan_segmentation_amd.image_generator import ImageGenerator
gcfg, gp, dcfg, dp, z, noise = bench_setup("ffhq", 4)
gen = ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=4)
img, mask = gen.generate_batch(z, noise)
img, mask = img.cpu().numpy(), mask.cpu().numpy()
assert pair_digest(img[0], mask[0]) == golden_bench_outputs()["ffhq_b4"]["samples"][0]
print("SWITCH_OK")
'''


def test_full_size_without_the_paired_kernel(torch_cuda, tmp_path):
    """ffhq 1024^2 batch 4 with GSA_WINO_PAIR=0 equals the oracle's digest: the four-wave kernel stays tested at the shapes the default
    rule hands to the paired one."""
    out = _child(tmp_path, _SWITCH_WORKER, "0")
    assert out.returncode == 0 and "SWITCH_OK" in out.stdout, out.stdout[-800:] + out.stderr[-2500:]
