"""Cost of the training stream's photometric kernel (csrc/gsa_photometric.hip) on generated images, bench.py's synthetic weights.

Kernel mode (default): one generated batch, then ROUNDS blocks of ITERS launches of gsa_photometric and (unless --only ours) of
torch's own composition of the same work on the same tensors (reflect pad + two grouped conv2d for the blur, the affine, randn for
the noise, clamp, round), each block timed with device events; prints the median us per call of both, the kernel's algorithmic
bytes (n*H*W*C read once + as many written) and the bytes/s reached, as one JSON line.  --variant picks the rows: "default" (the
default limits; of the samples --first-index 32.. of seed 0 half are blurred and half noisy, as the limits have it on average), "no-noise" (noise_prob = 0), "no-blur" (blur_prob = 0), "all" (every
sample blurred and noisy).  For the kernels' own times run it under the profiler and read photometric_kernel's row (and, with
--only torch, the sum of torch's rows):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/photometric_bench.py --gan ffhq --batch 8 --downscale 2 --only ours

Step mode (--step): alternates, in one process, blocks of STEPS batches of ImageGenerator.training_batches without and with
photometric=True, ROUNDS times after a warm-up; prints the median ms per batch of each and their difference as one JSON line.

    python tools/photometric_bench.py --step [--gan ffhq] [--batch 8] [--precision fp32] [--downscale 2] [--crop 480] [--steps 10] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {"default": {}, "no-noise": {"noise_prob": 0.0}, "no-blur": {"blur_prob": 0.0}, "all": {"blur_prob": 1.0, "noise_prob": 1.0}}


def build(args):
    from gan_segmentation_amd.image_generator import ImageGenerator
    from tests.common import bench_setup
    gcfg, gp, dcfg, dp, _z, _noise = bench_setup(args.gan, args.batch)
    gen = ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=args.batch, precision=args.precision,
                                     output_downscale=args.downscale)
    gen.graph_mode = "0"        # eager: the comparison is of the kernels, not of graph replay
    return gen


def torch_composition(torch, img, alpha, offset, sigma, wh, wv):
    """The same work in torch operators on the NHWC u8 batch: per-sample 7-tap weights as grouped convolutions over (n*C) planes,
    fresh normal noise instead of the counter-based one (the same amount of work, other values)."""
    import torch.nn.functional as F
    n, H, W, C = img.shape
    x = img.permute(0, 3, 1, 2).float().reshape(1, n * C, H, W)
    x = F.conv2d(F.pad(x, (3, 3, 0, 0), mode="reflect"), wh, groups=n * C)
    x = F.conv2d(F.pad(x, (0, 0, 3, 3), mode="reflect"), wv, groups=n * C)
    x = x.reshape(n, C, H, W) * alpha + offset
    x = x + sigma * torch.randn_like(x)
    return torch.floor(x.clamp(0.0, 255.0) + 0.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


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
    from gan_segmentation_amd import photometric as ph
    gen = build(args)
    dev = gen.netG._model.device
    n = args.batch
    img, _mask = gen.generate_indexed(args.first_index, n, seed=args.seed)
    _, H, W, C = img.shape
    rows_h = ph.photometric_plan(args.seed, args.first_index, n, **VARIANTS[args.variant])
    rows = torch.from_numpy(rows_h).to(dev)
    alpha = rows[:, 0].view(n, 1, 1, 1)
    offset = rows[:, 1:1 + C].reshape(n, C, 1, 1)
    sigma = rows[:, 5].view(n, 1, 1, 1)
    w = rows[:, 6:13].repeat_interleave(C, dim=0)                # (n*C, 7)
    wh, wv = w.view(n * C, 1, 1, 7).contiguous(), w.view(n * C, 1, 7, 1).contiguous()

    def ours():
        return ph.photometric(img, rows, args.seed, args.first_index)

    def theirs():
        return torch_composition(torch, img, alpha, offset, sigma, wh, wv)

    run_ours, run_theirs = args.only in ("both", "ours"), args.only in ("both", "torch")
    for _ in range(args.warmup):
        if run_ours:
            ours()
        if run_theirs:
            theirs()
    torch.cuda.synchronize()
    t_ours, t_theirs = [], []
    for _ in range(args.rounds):
        if run_ours:
            t_ours.append(timed(torch, ours, args.iters))
        if run_theirs:
            t_theirs.append(timed(torch, theirs, args.iters))
    out = {"mode": "kernel", "variant": args.variant, "gan": args.gan, "batch": n, "first_index": args.first_index, "precision": args.precision, "downscale": args.downscale,
           "image": [H, W, C], "iters": args.iters, "rounds": args.rounds, "blurred_samples": int((rows_h[:, 9] != 1).sum()),
           "noisy_samples": int((rows_h[:, 5] != 0).sum())}
    alg_bytes = 2 * n * H * W * C
    if run_ours:
        us = statistics.median(t_ours)
        out.update(photometric_call_us=round(us, 2), algorithmic_bytes=alg_bytes, photometric_call_GBps=round(alg_bytes / us / 1e3, 1),
                   photometric_rounds_us=[round(x, 2) for x in t_ours])
    if run_theirs:
        out.update(torch_composition_us=round(statistics.median(t_theirs), 2), torch_rounds_us=[round(x, 2) for x in t_theirs])
    if run_ours and run_theirs and args.variant == "no-noise":
        diff = (ours().int() - theirs().int()).abs()
        out.update(max_abs_diff_vs_torch=int(diff.max()), share_of_bytes_equal_to_torch=round(float((diff == 0).float().mean()), 6))
    gen.netG._model.ctx.check()
    out["note"] = ("call times are back-to-back launches timed with device events (launch gaps included); the kernel's own time is "
                   "photometric_kernel's row of a rocprofv3 --kernel-trace --stats run")
    print(json.dumps(out))


def step_mode(args):
    import torch
    gen = build(args)
    n = args.batch
    state = {"first": 0}

    def stepper(photometric):
        def run():
            for _ in gen.training_batches(n, crop=args.crop, seed=args.seed, first_index=state["first"], num_samples=n * args.steps,
                                          photometric=photometric):
                pass
            state["first"] += n * args.steps
        return run

    plain, changed = stepper(None), stepper(True)
    for _ in range(max(1, args.warmup // 2)):
        plain()
        changed()
    torch.cuda.synchronize()
    t = {"plain": [], "photometric": []}
    for _ in range(args.rounds):
        t["plain"].append(timed(torch, plain, 1) / 1000.0 / args.steps)
        t["photometric"].append(timed(torch, changed, 1) / 1000.0 / args.steps)
    gen.netG._model.ctx.check()
    m0, m1 = statistics.median(t["plain"]), statistics.median(t["photometric"])
    print(json.dumps({"mode": "step", "gan": args.gan, "batch": n, "precision": args.precision, "downscale": args.downscale,
                      "crop": args.crop, "steps_per_block": args.steps, "rounds": args.rounds,
                      "stream_ms": round(m0, 4), "stream_with_photometric_ms": round(m1, 4), "difference_us": round((m1 - m0) * 1000.0, 2),
                      "difference_percent": round(100.0 * (m1 - m0) / m0, 3),
                      "stream_rounds_ms": [round(x, 4) for x in t["plain"]],
                      "photometric_rounds_ms": [round(x, 4) for x in t["photometric"]]}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gan", default="ffhq")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--downscale", type=int, default=2)
    ap.add_argument("--crop", type=int, default=480)
    ap.add_argument("--variant", default="default", choices=sorted(VARIANTS))
    ap.add_argument("--only", default="both", choices=["both", "ours", "torch"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--first-index", type=int, default=32,
                    help="global index of the batch's first sample; with seed 0 the default plan of samples 32..39 blurs four and adds "
                         "noise to four (two and two of 32..35), the expectation of the default limits")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("photometric_bench.py needs a HIP device: there is nothing to measure without one")
    (step_mode if args.step else kernel_mode)(args)


if __name__ == "__main__":
    main()
