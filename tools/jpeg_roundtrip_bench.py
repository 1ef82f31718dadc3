"""Cost of the training stream's JPEG round trip (csrc/gsa_jpeg.hip, include/gsa_jpeg_roundtrip.h) on generated images,
bench.py's synthetic weights.

Kernel mode (default): one generated batch, then ROUNDS blocks of ITERS calls of jpeg.roundtrip and of the encoder
(JpegEncoder.encode: jpeg_transform_kernel, the same forward work, + the entropy-coding kernels) on the same images, each block
timed with device events; prints the median us per call of both, the round trip's algorithmic bytes (3 B/px read, 3 B/px written,
1.5 B/px of workspace written and read once) and the bytes/s reached, as one JSON line.  For the kernels' own times run it under the
profiler and read the rows of jpeg_roundtrip_mcu_kernel, jpeg_roundtrip_merge_kernel and jpeg_transform_kernel:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/jpeg_roundtrip_bench.py --gan ffhq --batch 8 --downscale 2

Step mode (--step): alternates, in one process, blocks of STEPS batches of ImageGenerator.training_batches without and with
jpeg_quality, ROUNDS times after a warm-up; prints the median ms per step of each, their difference and the blocks, as one JSON line.

    python tools/jpeg_roundtrip_bench.py --step [--gan ffhq] [--batch 8] [--downscale 2] [--quality 95] [--steps 10] [--rounds 5]
"""
import argparse
import itertools
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(args):
    from gan_segmentation_amd.image_generator import ImageGenerator
    from tests.common import bench_setup
    gcfg, gp, dcfg, dp, _z, _noise = bench_setup(args.gan, args.batch)
    gen = ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=args.batch, precision=args.precision,
                                     output_downscale=args.downscale)
    gen.graph_mode = "0"        # eager: the comparison is of the kernels, not of graph replay
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
    from gan_segmentation_amd import jpeg
    gen = build(args)
    n = args.batch
    img, _mask = gen.generate_indexed(0, n, seed=args.seed)
    _, H, W, _C = img.shape
    out = torch.empty_like(img)
    enc = jpeg.JpegEncoder(n, H, W, img.device, quality=args.quality)

    def ours():
        return jpeg.roundtrip(img, args.quality, out=out)

    def encode():
        return enc.encode(img)

    for _ in range(args.warmup):
        ours()
        encode()
    torch.cuda.synchronize()
    t_ours, t_enc = [], []
    for _ in range(args.rounds):
        t_ours.append(timed(torch, ours, args.iters))
        t_enc.append(timed(torch, encode, args.iters))
    changed = float((out != img).float().mean())
    worst = int((out.int() - img.int()).abs().max())
    gen.netG._model.ctx.check()
    alg_bytes = n * H * W * 9
    us = statistics.median(t_ours)
    print(json.dumps({"mode": "kernel", "gan": args.gan, "batch": n, "precision": args.precision, "downscale": args.downscale,
                      "image": [H, W, 3], "quality": args.quality, "iters": args.iters, "rounds": args.rounds,
                      "roundtrip_call_us": round(us, 2), "encode_call_us": round(statistics.median(t_enc), 2),
                      "algorithmic_bytes": alg_bytes, "roundtrip_call_GBps": round(alg_bytes / us / 1e3, 1),
                      "roundtrip_rounds_us": [round(x, 2) for x in t_ours], "encode_rounds_us": [round(x, 2) for x in t_enc],
                      "fraction_of_bytes_changed": round(changed, 4), "largest_change_levels": worst,
                      "note": "call times are back-to-back launches timed with device events (launch gaps included); the kernels' own "
                              "times are their rows of a rocprofv3 --kernel-trace --stats run"}))


def step_mode(args):
    import torch
    gen = build(args)
    n = args.batch
    streams = {"plain": gen.training_batches(n, crop=args.crop, seed=args.seed),
               "jpeg": gen.training_batches(n, crop=args.crop, seed=args.seed, jpeg_quality=args.quality)}

    def stepper(name):
        return lambda: next(streams[name])

    for name in streams:
        for _ in itertools.repeat(None, args.warmup):
            next(streams[name])
    torch.cuda.synchronize()
    t = {"plain": [], "jpeg": []}
    for _ in range(args.rounds):
        for name in ("plain", "jpeg"):
            t[name].append(timed(torch, stepper(name), args.steps) / 1000.0)
    gen.netG._model.ctx.check()
    m0, m1 = statistics.median(t["plain"]), statistics.median(t["jpeg"])
    print(json.dumps({"mode": "step", "gan": args.gan, "batch": n, "precision": args.precision, "downscale": args.downscale,
                      "crop": args.crop, "quality": args.quality, "steps_per_block": args.steps, "rounds": args.rounds,
                      "stream_ms": round(m0, 4), "stream_with_jpeg_ms": round(m1, 4), "difference_ms": round(m1 - m0, 4),
                      "difference_percent": round(100.0 * (m1 - m0) / m0, 3),
                      "stream_rounds_ms": [round(x, 4) for x in t["plain"]],
                      "stream_with_jpeg_rounds_ms": [round(x, 4) for x in t["jpeg"]]}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gan", default="ffhq")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--downscale", type=int, default=2)
    ap.add_argument("--crop", type=int, default=480)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("jpeg_roundtrip_bench.py needs a HIP device: there is nothing to measure without one")
    (step_mode if args.step else kernel_mode)(args)


if __name__ == "__main__":
    main()
