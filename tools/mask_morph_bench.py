"""Cost and effect of the mask clean-up (csrc/gsa_mask.hip, include/gsa_mask.h) on generated masks, bench.py's synthetic weights.

Kernel mode (default): one generated batch, then ROUNDS blocks of ITERS calls of mask_ops.morph_mask on its masks, each block timed
with device events; prints the median us per call, the algorithmic bytes (1 B/px read, 1 B/px written) and the bytes/s reached, and
the share of mask pixels the rule changes (synthetic weights: an illustration of the tool, not of a trained decoder), as one JSON
line.  For the kernel's own time run it under the profiler and read the row of mask_morph_kernel:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/mask_morph_bench.py --gan ffhq --batch 8 [--downscale 2]

Step mode (--step): alternates, in one process, blocks of STEPS calls of generate_indexed on a generator without and one with
mask_morph, ROUNDS times after a warm-up; prints the median ms per step of each, their difference and the blocks, as one JSON line.

    python tools/mask_morph_bench.py --step [--gan ffhq] [--batch 8] [--precision fp32] [--steps 10] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(args, mask_morph=False):
    from gan_segmentation_amd.image_generator import ImageGenerator
    from tests.common import bench_setup
    gcfg, gp, dcfg, dp, _z, _noise = bench_setup(args.gan, args.batch)
    gen = ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=args.batch, precision=args.precision,
                                     output_downscale=args.downscale, mask_morph=mask_morph)
    if args.eager:
        gen.graph_mode = "0"
    return gen


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
    gen = build(args)
    n = args.batch
    _img, mask = gen.generate_indexed(0, n, seed=args.seed)
    _, H, W = mask.shape
    out = torch.empty_like(mask)

    def ours():
        return mask_ops.morph_mask(mask, out=out)

    for _ in range(args.warmup):
        ours()
    torch.cuda.synchronize()
    t = [timed(torch, ours, args.iters) for _ in range(args.rounds)]
    changed = float((out != mask).float().mean())
    gen.netG._model.ctx.check()
    alg_bytes = n * H * W * 2
    us = statistics.median(t)
    print(json.dumps({"mode": "kernel", "gan": args.gan, "batch": n, "precision": args.precision, "downscale": args.downscale,
                      "mask": [H, W], "iters": args.iters, "rounds": args.rounds, "morph_call_us": round(us, 2),
                      "algorithmic_bytes": alg_bytes, "morph_call_GBps": round(alg_bytes / us / 1e3, 1),
                      "morph_rounds_us": [round(x, 2) for x in t], "fraction_of_pixels_changed": round(changed, 5),
                      "foreground_share_raw": round(float((mask != 0).float().mean()), 5),
                      "note": "call times are back-to-back launches timed with device events (launch gaps included); the kernel's own "
                              "time is its row of a rocprofv3 --kernel-trace --stats run"}))


def step_mode(args):
    import torch
    gens = {"plain": build(args), "morph": build(args, mask_morph=True)}
    n = args.batch
    R = 2 ** gens["plain"].max_res_log2 // args.downscale
    outs = {name: (torch.empty((n, R, R, g.netG.nc), dtype=torch.uint8, device="cuda"),
                   torch.empty((n, R, R), dtype=torch.uint8, device="cuda")) for name, g in gens.items()}

    def stepper(name):
        return lambda: gens[name].generate_indexed(0, n, seed=args.seed, out=outs[name])

    for name in gens:
        for _ in range(args.warmup):
            stepper(name)()
    torch.cuda.synchronize()
    t = {"plain": [], "morph": []}
    for _ in range(args.rounds):
        for name in ("plain", "morph"):
            t[name].append(timed(torch, stepper(name), args.steps) / 1000.0)
    for g in gens.values():
        g.netG._model.ctx.check()
    m0, m1 = statistics.median(t["plain"]), statistics.median(t["morph"])
    print(json.dumps({"mode": "step", "gan": args.gan, "batch": n, "precision": args.precision, "downscale": args.downscale,
                      "eager": bool(args.eager), "steps_per_block": args.steps, "rounds": args.rounds,
                      "step_ms": round(m0, 4), "step_with_morph_ms": round(m1, 4), "difference_us": round((m1 - m0) * 1000.0, 2),
                      "difference_percent": round(100.0 * (m1 - m0) / m0, 3),
                      "step_rounds_ms": [round(x, 4) for x in t["plain"]],
                      "step_with_morph_rounds_ms": [round(x, 4) for x in t["morph"]],
                      "graphs_captured": {name: g.graphs_captured() for name, g in gens.items()}}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gan", default="ffhq")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--downscale", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--eager", action="store_true", help="never replay a hipGraph (GSA_GRAPH=0 for both generators)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("mask_morph_bench.py needs a HIP device: there is nothing to measure without one")
    (step_mode if args.step else kernel_mode)(args)


if __name__ == "__main__":
    main()
