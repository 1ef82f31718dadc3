"""Cost of the training stream's kernel (csrc/gsa_augment.hip) on generated pairs, bench.py's synthetic weights.

Kernel mode (default): one generated batch, then ITERS launches of gsa_augment_pairs and ITERS rounds of torch's own composition of
the same work (affine_grid + grid_sample bilinear for the image, nearest for the mask, the ignore label outside, then the
normalisation) on the same tensors, each timed with device events; prints the mean us per call of both, the kernel's algorithmic
bytes (n*H*W*(C+1) read once + n*oh*ow*(bytes per value*C + 1) written) and the bytes/s reached, as one JSON line.  For the kernel's
own time run it under the profiler and read augment_pairs_kernel's row:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/augment_bench.py --gan ffhq --batch 8 --downscale 2

Step mode (--step): alternates, in one process, blocks of generate_indexed alone and of generate_indexed + plan + kernel (what one
batch of ImageGenerator.training_batches does), ROUNDS times after a warm-up; prints the median ms per step of each and their
difference as one JSON line.

    python tools/augment_bench.py --step [--gan ffhq] [--batch 8] [--precision fp32] [--downscale 2] [--crop 480] [--steps 10] [--rounds 5]
"""
import argparse
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


def torch_composition(torch, img, mask, theta, out_size, scale_t, bias_t, dtype):
    """The same work in torch operators: theta (n, 2, 3) maps normalised output to normalised source coordinates
    (align_corners=True, where the normalised corner is the centre of the corner pixel, as in the kernel's rule)."""
    import torch.nn.functional as F
    n = img.shape[0]
    grid = F.affine_grid(theta, (n, 1, out_size[0], out_size[1]), align_corners=True)
    x = img.permute(0, 3, 1, 2).float()
    image = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    image = (image * scale_t + bias_t).to(dtype)
    m = mask[:, None].float() - 255.0                         # zero padding then reads as the ignore label
    label = (F.grid_sample(m, grid, mode="nearest", padding_mode="zeros", align_corners=True) + 255.0).to(torch.uint8)[:, 0]
    return image, label


def normalised_theta(np, matrices, H, W, oh, ow):
    """Output-pixel -> source-pixel rows (n, 6) as affine_grid's theta (float64 arithmetic, fp32 result)."""
    m = matrices.astype(np.float64).reshape(-1, 2, 3)
    sx, sy = (ow - 1) / 2.0, (oh - 1) / 2.0
    t = np.empty_like(m)
    t[:, 0, 0], t[:, 0, 1] = m[:, 0, 0] * sx, m[:, 0, 1] * sy
    t[:, 1, 0], t[:, 1, 1] = m[:, 1, 0] * sx, m[:, 1, 1] * sy
    t[:, 0, 2] = m[:, 0, 0] * sx + m[:, 0, 1] * sy + m[:, 0, 2]
    t[:, 1, 2] = m[:, 1, 0] * sx + m[:, 1, 1] * sy + m[:, 1, 2]
    t[:, 0, :] = t[:, 0, :] * (2.0 / (W - 1))
    t[:, 1, :] = t[:, 1, :] * (2.0 / (H - 1))
    t[:, 0, 2] -= 1.0
    t[:, 1, 2] -= 1.0
    return t.astype(np.float32)


def timed(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def kernel_mode(args):
    import numpy as np
    import torch
    from gan_segmentation_amd import augment
    gen = build(args)
    dev = gen.netG._model.device
    n = args.batch
    img, mask = gen.generate_indexed(0, n, seed=args.seed)
    _, H, W, C = img.shape
    out_size = augment.output_size(H, W, args.crop)
    dtype = torch.bfloat16 if args.out_dtype == "bf16" else torch.float32
    scale, bias = augment.normalisation()
    matrices_h = augment.plan_matrices(args.seed, 0, n, H, W, args.crop, "train")
    matrices = torch.from_numpy(matrices_h).to(dev)
    theta = torch.from_numpy(normalised_theta(np, matrices_h, H, W, *out_size)).to(dev)
    scale_t = torch.from_numpy(scale).to(dev).view(1, C, 1, 1)
    bias_t = torch.from_numpy(bias).to(dev).view(1, C, 1, 1)

    def ours():
        return augment.augment_pairs(img, mask, matrices, out_size, scale=scale, bias=bias, dtype=dtype)

    def theirs():
        return torch_composition(torch, img, mask, theta, out_size, scale_t, bias_t, dtype)

    for _ in range(args.warmup):
        ours()
        theirs()
    torch.cuda.synchronize()
    t_ours, t_theirs = [], []
    for _ in range(args.rounds):
        t_ours.append(timed(torch, ours, args.iters))
        t_theirs.append(timed(torch, theirs, args.iters))
    a, b = ours(), theirs()
    diff = float((a[0].float() - b[0].float()).abs().max())
    labels_equal = float((a[1] == b[1]).float().mean())
    gen.netG._model.ctx.check()
    value_bytes = 2 if dtype == torch.bfloat16 else 4
    alg_bytes = n * H * W * (C + 1) + n * out_size[0] * out_size[1] * (value_bytes * C + 1)
    us = statistics.median(t_ours)
    print(json.dumps({"mode": "kernel", "gan": args.gan, "batch": n, "precision": args.precision, "downscale": args.downscale,
                      "source": [H, W, C], "out": list(out_size), "out_dtype": args.out_dtype, "iters": args.iters, "rounds": args.rounds,
                      "augment_call_us": round(us, 2), "torch_composition_us": round(statistics.median(t_theirs), 2),
                      "algorithmic_bytes": alg_bytes, "augment_call_GBps": round(alg_bytes / us / 1e3, 1),
                      "augment_rounds_us": [round(x, 2) for x in t_ours], "torch_rounds_us": [round(x, 2) for x in t_theirs],
                      "max_abs_diff_vs_torch": diff, "labels_equal_to_torch": labels_equal,
                      "note": "call times are back-to-back launches timed with device events (launch gaps included); the kernel's own "
                              "time is augment_pairs_kernel's row of a rocprofv3 --kernel-trace --stats run"}))


def step_mode(args):
    import torch
    from gan_segmentation_amd import augment
    gen = build(args)
    n = args.batch
    R = 2 ** gen.max_res_log2 // args.downscale
    out_size = augment.output_size(R, R, args.crop)
    dtype = torch.bfloat16 if args.out_dtype == "bf16" else torch.float32
    scale, bias = augment.normalisation()
    state = {"first": 0}

    def alone():
        gen.generate_indexed(state["first"], n, seed=args.seed)
        state["first"] += n

    def streamed():
        first = state["first"]
        img, mask = gen.generate_indexed(first, n, seed=args.seed)
        matrices = augment.plan_matrices(args.seed, first, n, R, R, args.crop, "train")
        augment.augment_pairs(img, mask, matrices, out_size, scale=scale, bias=bias, dtype=dtype)
        state["first"] += n

    for _ in range(args.warmup):
        alone()
        streamed()
    torch.cuda.synchronize()
    t = {"alone": [], "streamed": []}
    for _ in range(args.rounds):
        t["alone"].append(timed(torch, alone, args.steps) / 1000.0)
        t["streamed"].append(timed(torch, streamed, args.steps) / 1000.0)
    gen.netG._model.ctx.check()
    m0, m1 = statistics.median(t["alone"]), statistics.median(t["streamed"])
    print(json.dumps({"mode": "step", "gan": args.gan, "batch": n, "precision": args.precision, "downscale": args.downscale,
                      "crop": args.crop, "out_dtype": args.out_dtype, "steps_per_block": args.steps, "rounds": args.rounds,
                      "generate_ms": round(m0, 4), "generate_plus_augment_ms": round(m1, 4), "difference_ms": round(m1 - m0, 4),
                      "difference_percent": round(100.0 * (m1 - m0) / m0, 3),
                      "generate_rounds_ms": [round(x, 4) for x in t["alone"]],
                      "streamed_rounds_ms": [round(x, 4) for x in t["streamed"]]}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gan", default="ffhq")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--downscale", type=int, default=2)
    ap.add_argument("--crop", type=int, default=480)
    ap.add_argument("--out-dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("augment_bench.py needs a HIP device: there is nothing to measure without one")
    (step_mode if args.step else kernel_mode)(args)


if __name__ == "__main__":
    main()
