"""Cost of the mask agreement (csrc/gsa_compare.hip, csrc/gsa_compare.h) beside the pair statistics, an FFHQ batch: 8 x 1024 x 1024.

Three pairs of masks, 4 classes each: "blobs" (tests' class_blobs at sigma 6: regions of 20 to 30 px, a few dozen boundaries a row),
"large" (128 px blobs enlarged 8 times: regions of a hundred pixels and more, as a face parsing has them) and "noise" (uniform, 3
classes).  The dist2 planes of the band cases are computed once, before the timed window: compare_launch_* is gsa_mask_compare's two
launches alone, compare_wrapper_* is mask_ops.compare(band=2), the two boundary passes included.  pair_stats_* is
pair_stats.pair_stats on the same target masks, with a random 3-channel image (C3) and without one (C0).  ROUNDS rounds; in each,
every case is timed once as ITERS back-to-back calls between two device events (launch gaps included), so the cases alternate.
Prints one JSON line per case: the median, minimum and maximum us per call over the rounds and, for the single entries, the
algorithmic bytes per second (2 or 6 bytes a pixel for compare, C + 1 for pair_stats).

    python tools/compare_bench.py [--iters 200] [--rounds 5]

GSA_HIP_LIBRARY selects another build of the library (how the kTurns and tile variants of DESIGN.md section 23 were timed).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W, R = 8, 1024, 1024, 2


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("compare_bench.py needs a HIP device: there is nothing to measure without one")
    from gan_segmentation_amd import mask_ops, pair_stats
    from gan_segmentation_amd._runtime import launch
    from tests.test_boundary_host import class_blobs

    def eightfold(a):           # two planes and their three mirror images
        return np.concatenate([a, a[:, ::-1], a[:, :, ::-1], a[:, ::-1, ::-1]]).copy()

    def enlarged(a):
        return np.repeat(np.repeat(a, 8, axis=1), 8, axis=2).copy()

    rng = np.random.default_rng(0)
    noise = rng.integers(0, 3, (2, N, H, W)).astype(np.uint8)
    masks = {"blobs": (eightfold(class_blobs(1, (2, H, W), 4, sigma=6.0)), eightfold(class_blobs(2, (2, H, W), 4, sigma=6.0))),
             "large": (enlarged(class_blobs(3, (N, H // 8, W // 8), 4, sigma=4.0)), enlarged(class_blobs(4, (N, H // 8, W // 8), 4, sigma=4.0))),
             "noise": (noise[0], noise[1])}
    img = torch.from_numpy(rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)).cuda()
    rows = torch.empty((N, mask_ops.COMPARE_ROW), dtype=torch.int64, device="cuda")
    srows = torch.empty((N, pair_stats.ROW), dtype=torch.int64, device="cuda")
    dev = rows.device
    pixels = N * H * W
    cases, alg_bytes = {}, {}

    def entry(t, p, r, a, b):
        launch("gsa_mask_compare", dev, N, H, W, r, t.data_ptr(), p.data_ptr(), a.data_ptr() if r else None, b.data_ptr() if r else None,
               rows.data_ptr())

    for name, (target, pred) in masks.items():
        t, p = torch.from_numpy(target).cuda(), torch.from_numpy(pred).cuda()
        bt, bp = mask_ops.boundary_distance(t, R), mask_ops.boundary_distance(p, R)
        cases["compare_launch_no_bands_" + name] = lambda t=t, p=p: entry(t, p, 0, None, None)
        cases["compare_launch_bands_" + name] = lambda t=t, p=p, bt=bt, bp=bp: entry(t, p, R, bt, bp)
        cases["compare_wrapper_band2_" + name] = lambda t=t, p=p: mask_ops.compare(p, t, band=R, out=rows)
        alg_bytes["compare_launch_no_bands_" + name], alg_bytes["compare_launch_bands_" + name] = 2 * pixels, 6 * pixels
        if name != "noise":
            cases["pair_stats_C3_" + name] = lambda t=t: pair_stats.pair_stats(img, t, out=srows)
            cases["pair_stats_C0_" + name] = lambda t=t: pair_stats.pair_stats(None, t, out=srows)
            alg_bytes["pair_stats_C3_" + name], alg_bytes["pair_stats_C0_" + name] = 4 * pixels, pixels

    times = {k: [] for k in cases}
    for fn in cases.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in cases.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1000.0 / args.iters)
    library = os.path.basename(os.environ.get("GSA_HIP_LIBRARY", "libgsa_hip.so"))
    for name, t in times.items():
        line = {"case": name, "library": library, "batch": [N, H, W], "iters": args.iters, "rounds": args.rounds,
                "call_us": round(float(np.median(t)), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2)}
        if name in alg_bytes:
            line["call_GBps"] = round(alg_bytes[name] / float(np.median(t)) / 1e3, 1)
        print(json.dumps(line))


if __name__ == "__main__":
    main()
