"""Cost of the mask components (csrc/gsa_components.hip, include/gsa_components.h) on generated masks, bench.py's synthetic weights.

Kernel mode (default): one mask batch -- the decoder's (--input decoder) or the serpentine, the union-find's worst case (--input
serpentine) -- then ROUNDS blocks of ITERS calls of mask_ops.despeckle with rows, each block timed with device events; prints the
median us per call, the algorithmic floor (1 B/px read, 8 B/px of labels and areas written), the component count and the share of
pixels the filter changes, as one JSON line; --scipy adds scipy.ndimage.label's time on the host for the same batch (one label call
per value and plane).  For the per-phase kernel times run it under the profiler and read the rows of label_tiles_kernel,
merge_seams_kernel, flatten_count_kernel and spread_filter_kernel:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/components_bench.py --gan ffhq --batch 8 [--input serpentine]

Step mode (--step): alternates, in one process, blocks of STEPS calls of generate_indexed on a generator without and one with
mask_min_area, ROUNDS times after a warm-up; prints the median ms per step of each, their difference and the blocks, as one JSON line.

    python tools/components_bench.py --step [--gan ffhq] [--batch 8] [--min-area 64] [--steps 10] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(args, **kw):
    from gan_segmentation_amd.image_generator import ImageGenerator
    from tests.common import bench_setup
    gcfg, gp, dcfg, dp, _z, _noise = bench_setup(args.gan, args.batch)
    return ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=args.batch, precision=args.precision, **kw)


def timed(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def serpentine(torch, n, R):
    m = torch.zeros((n, R, R), dtype=torch.uint8)
    m[:, 0::2, :] = 1
    m[:, 1::4, -1] = 1
    m[:, 3::4, 0] = 1
    return m.cuda()


def scipy_seconds(mask, connectivity):
    import numpy as np
    from scipy import ndimage as ndi
    structure = np.ones((3, 3), int) if connectivity == 8 else ndi.generate_binary_structure(2, 1)
    t0 = time.perf_counter()
    for plane in mask:
        for v in np.unique(plane):
            ndi.label(plane == v, structure=structure)
    return time.perf_counter() - t0


def kernel_mode(args):
    import torch
    from gan_segmentation_amd import mask_ops
    n = args.batch
    if args.input == "decoder":
        gen = build(args)
        _img, mask = gen.generate_indexed(0, n, seed=args.seed)
        gen.netG._model.ctx.check()
    else:
        from gan_segmentation_amd.weights import GAN_MAX_RES_LOG2
        mask = serpentine(torch, n, 2 ** GAN_MAX_RES_LOG2[args.gan])
    _, H, W = mask.shape
    out = torch.empty_like(mask)
    scratch = (torch.empty(mask.shape, dtype=torch.int32, device="cuda"), torch.empty(mask.shape, dtype=torch.int32, device="cuda"))

    def ours():
        return mask_ops.despeckle(mask, args.min_area, args.connectivity, out=out, return_stats=True, scratch=scratch)

    for _ in range(args.warmup):
        ours()
    torch.cuda.synchronize()
    t = [timed(torch, ours, args.iters) for _ in range(args.rounds)]
    _out, rows = ours()
    rows = rows.cpu()
    us = statistics.median(t)
    floor = n * H * W * 9
    line = {"mode": "kernel", "gan": args.gan, "batch": n, "input": args.input, "mask": [H, W], "connectivity": args.connectivity,
            "min_area": args.min_area, "iters": args.iters, "rounds": args.rounds, "call_us": round(us, 2),
            "rounds_us": [round(x, 2) for x in t], "floor_bytes": floor, "floor_GBps_reached": round(floor / us / 1e3, 1),
            "components_per_sample": [int(x) for x in rows[:, mask_ops.COMP_NCOMP:mask_ops.COMP_NCOMP + mask_ops.COMP_SLOTS].sum(1)],
            "small_components_per_sample": [int(x) for x in rows[:, mask_ops.COMP_SMALL]],
            "fraction_of_pixels_changed": round(float((out != mask).float().mean()), 6),
            "note": "call times are back-to-back calls of four launches timed with device events (launch gaps included); the kernels' "
                    "own times are their rows of a rocprofv3 --kernel-trace --stats run"}
    if args.scipy:
        line["scipy_label_host_ms"] = round(1000.0 * scipy_seconds(mask.cpu().numpy(), args.connectivity), 1)
        line["host_cpus"] = len(os.sched_getaffinity(0))
    print(json.dumps(line))


def step_mode(args):
    import torch
    gens = {"plain": build(args), "filtered": build(args, mask_min_area=args.min_area, mask_connectivity=args.connectivity)}
    n = args.batch
    R = 2 ** gens["plain"].max_res_log2
    outs = {name: (torch.empty((n, R, R, g.netG.nc), dtype=torch.uint8, device="cuda"),
                   torch.empty((n, R, R), dtype=torch.uint8, device="cuda")) for name, g in gens.items()}

    def stepper(name):
        return lambda: gens[name].generate_indexed(0, n, seed=args.seed, out=outs[name])

    for name in gens:
        for _ in range(args.warmup):
            stepper(name)()
    torch.cuda.synchronize()
    t = {name: [] for name in gens}
    for _ in range(args.rounds):
        for name in gens:
            t[name].append(timed(torch, stepper(name), args.steps) / 1000.0)
    for g in gens.values():
        g.netG._model.ctx.check()
    m0, m1 = statistics.median(t["plain"]), statistics.median(t["filtered"])
    print(json.dumps({"mode": "step", "gan": args.gan, "batch": n, "precision": args.precision, "min_area": args.min_area,
                      "connectivity": args.connectivity, "steps_per_block": args.steps, "rounds": args.rounds, "step_ms": round(m0, 4),
                      "step_with_filter_ms": round(m1, 4), "difference_us": round((m1 - m0) * 1000.0, 2),
                      "difference_percent": round(100.0 * (m1 - m0) / m0, 3), "step_rounds_ms": [round(x, 4) for x in t["plain"]],
                      "step_with_filter_rounds_ms": [round(x, 4) for x in t["filtered"]],
                      "pixels_changed": int((outs["plain"][1] != outs["filtered"][1]).sum())}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gan", default="ffhq")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--input", default="decoder", choices=["decoder", "serpentine"])
    ap.add_argument("--connectivity", type=int, default=8)
    ap.add_argument("--min-area", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--scipy", action="store_true", help="also time scipy.ndimage.label on the host for the same masks")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("components_bench.py needs a HIP device: there is nothing to measure without one")
    (step_mode if args.step else kernel_mode)(args)


if __name__ == "__main__":
    main()
