"""Generates tests/golden/sweep_anchors.json: SHA-256 of what the CANONICAL C ORACLE (oracle/c/gsa_oracle.c, fp32) computes for
sample 0 of tests/test_gpu_batch_sweep.py's inputs (tests.common.sweep_setup), for ffhq, cars and bedrooms.

    python tests/golden/make_sweep_anchors.py

The batch-1 GPU run of that sample must reproduce every digest: the fused step's u8 image and mask, the two-call path's fp32 rgb
and logits, and its last two fp32 features.  tests/golden/bench_outputs.json (bench.py's digests) is a different file.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.binding import Oracle            # noqa: E402
from tests.common import sweep_setup         # noqa: E402

GANS = ["ffhq", "cars", "bedrooms"]


def h(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def anchors(gan):
    gcfg, gp, dcfg, dp, z, noise = sweep_setup(gan)
    o = Oracle(gcfg, gp, dcfg, dp)
    rgb, img, feats = o.generator(z[:1], [a[:1] for a in noise])
    logits, mask = o.decoder(feats)
    return {"image_u8": h(img), "mask_u8": h(mask), "rgb_f32": h(rgb), "logits_f32": h(logits),
            "feature_last_f32": h(feats[-1]), "feature_second_last_f32": h(feats[-2]),
            "shapes": {"image": list(img.shape), "mask": list(mask.shape), "rgb": list(rgb.shape), "logits": list(logits.shape),
                       "feature_last": list(feats[-1].shape), "feature_second_last": list(feats[-2].shape)}}


def main():
    out = {}
    for gan in GANS:
        out[gan] = anchors(gan)
        print(gan, out[gan]["image_u8"], flush=True)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sweep_anchors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
