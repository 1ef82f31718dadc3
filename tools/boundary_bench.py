"""Cost of the mask boundary distance and the ignore band (csrc/gsa_boundary.hip, include/gsa_boundary.h) on generated masks,
bench.py's synthetic weights.

Kernel mode (default): one mask batch from the decoder, then for every radius of --radii ROUNDS blocks of ITERS calls of
mask_ops.ignore_band, once for the band only and once with the distance map, and the same blocks of mask_ops.morph_mask on the same
masks as the yardstick (the same 2 bytes per pixel of traffic), each block timed with device events; prints the median us per call,
the bytes each form moves, the share of pixels in the band and the masks' class count, as one JSON line.  For the kernels' own times
run it under the profiler and read the rows of mask_boundary_kernel<K, ALIGNED> (K = 1, 2, 4, 8 for radii up to 4, 8, 16, 32) and
mask_morph_kernel; every output form is the same kernel, so --forms picks the one a profiled run is to show:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/boundary_bench.py --gan ffhq --batch 8 --radii 2 32 --forms band

Step mode (--step): alternates, in one process, blocks of STEPS calls of generate_indexed on a generator without and one with
mask_ignore_band, ROUNDS times after a warm-up; prints the median ms per step of each, their difference and the blocks, as one JSON line.

    python tools/boundary_bench.py --step [--gan ffhq] [--batch 8] [--radius 2] [--steps 10] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

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


def kernel_mode(args):
    import torch
    from gan_segmentation_amd import mask_ops
    n = args.batch
    gen = build(args)
    _img, mask = gen.generate_indexed(0, n, seed=args.seed)
    gen.netG._model.ctx.check()
    _, H, W = mask.shape
    out = torch.empty_like(mask)
    dist2 = torch.empty(mask.shape, dtype=torch.int16, device="cuda")
    pixels = n * H * W

    def measure(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t = [timed(torch, fn, args.iters) for _ in range(args.rounds)]
        return {"call_us": round(statistics.median(t), 2), "rounds_us": [round(x, 2) for x in t]}

    cases = {"morph": dict(measure(lambda: mask_ops.morph_mask(mask, out=out)), bytes=2 * pixels)}
    for R in args.radii:
        if "band" in args.forms:
            band = measure(lambda: mask_ops.ignore_band(mask, R, args.label, out=out))
            share = float((out == args.label).float().mean()) if not bool((mask == args.label).any()) else None
            cases["band_r%d" % R] = dict(band, bytes=2 * pixels, fraction_of_pixels_in_band=None if share is None else round(share, 6))
        if "both" in args.forms:                # the distance map comes from torch's caching allocator
            cases["band_and_dist2_r%d" % R] = dict(measure(lambda: mask_ops.ignore_band(mask, R, args.label, out=out, return_distance=True)),
                                                    bytes=4 * pixels)
        if "dist2" in args.forms:
            cases["dist2_r%d" % R] = dict(measure(lambda: mask_ops.boundary_distance(mask, R, out=dist2)), bytes=3 * pixels)
    for c in cases.values():
        c["GBps"] = round(c["bytes"] / c["call_us"] / 1e3, 1)
    print(json.dumps({"mode": "kernel", "gan": args.gan, "batch": n, "mask": [H, W], "classes": int(mask.max()) + 1, "label": args.label,
                      "iters": args.iters, "rounds": args.rounds, "cases": cases,
                      "note": "call times are back-to-back calls timed with device events (launch gaps included); the kernels' own "
                              "times are their rows of a rocprofv3 --kernel-trace --stats run"}))


def step_mode(args):
    import torch
    gens = {"plain": build(args), "banded": build(args, mask_ignore_band=args.radius, mask_ignore_label=args.label)}
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
    m0, m1 = statistics.median(t["plain"]), statistics.median(t["banded"])
    print(json.dumps({"mode": "step", "gan": args.gan, "batch": n, "precision": args.precision, "radius": args.radius, "label": args.label,
                      "steps_per_block": args.steps, "rounds": args.rounds, "step_ms": round(m0, 4), "step_with_band_ms": round(m1, 4),
                      "difference_us": round((m1 - m0) * 1000.0, 2), "difference_percent": round(100.0 * (m1 - m0) / m0, 3),
                      "step_rounds_ms": [round(x, 4) for x in t["plain"]], "step_with_band_rounds_ms": [round(x, 4) for x in t["banded"]],
                      "pixels_in_band": int((outs["plain"][1] != outs["banded"][1]).sum())}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gan", default="ffhq")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--radii", type=int, nargs="+", default=[2, 32], help="kernel mode: the radii to time")
    ap.add_argument("--forms", nargs="+", default=["band", "both", "dist2"], choices=["band", "both", "dist2"],
                    help="kernel mode: the output forms to time (out only, out and dist2, dist2 only)")
    ap.add_argument("--radius", type=int, default=2, help="step mode: mask_ignore_band")
    ap.add_argument("--label", type=int, default=255)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("boundary_bench.py needs a HIP device: there is nothing to measure without one")
    (step_mode if args.step else kernel_mode)(args)


if __name__ == "__main__":
    main()
