"""Cost of the pair statistics (csrc/gsa_stats.hip, include/gsa_stats.h) on generated pairs, bench.py's synthetic weights.

Kernel mode (default): one generated batch, then ROUNDS blocks of ITERS calls of pair_stats.pair_stats on it, each block timed with
device events; prints the median us per call, the algorithmic bytes (C + 1 bytes per pixel read) and the bytes/s reached, as one
JSON line.  With --torch the timed call is torch's own composition of the same quantities on the same tensors (bincount, masked
sums, amin / amax of index grids, shifted compares), checked once against the kernel's rows.  For the kernels' own time run either
form under the profiler and read the rows of pair_stats_kernel + stats_init_kernel, or the sum of every row of the --torch run
minus the generate step's kernels (--skip-generate feeds random pairs of the same size, so that the trace holds nothing else):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/pair_stats_bench.py --gan ffhq --batch 8 --skip-generate [--torch]

Step mode (--step): alternates, in one process, blocks of STEPS steps of generate_indexed + DatasetWriter.submit (GPU JPEG and PNG,
files into a temporary directory, each block ended by drain()) without and with stats=True, ROUNDS times after a warm-up; prints
the median ms per step of each, their difference and the blocks, as one JSON line.

    python tools/pair_stats_bench.py --step [--gan ffhq] [--batch 8] [--steps 10] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"ffhq": 1024, "celebahq": 1024, "cars": 512, "bedrooms": 256, "cats": 256}


def build(args):
    from gan_segmentation_amd.image_generator import ImageGenerator
    from tests.common import bench_setup
    gcfg, gp, dcfg, dp, _z, _noise = bench_setup(args.gan, args.batch)
    return ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=args.batch, precision=args.precision,
                                      output_downscale=args.downscale)


def timed(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def torch_rows(torch, img, mask):
    """The same 88 words per sample from torch's own operators (int64 throughout)."""
    n, H, W = mask.shape
    C = img.shape[-1]
    dev = mask.device
    rows = torch.zeros((n, 88), dtype=torch.int64, device=dev)
    slot = mask.clamp(max=8).long()
    keyed = slot.view(n, -1) + 9 * torch.arange(n, device=dev)[:, None]
    rows[:, 0:9] = torch.bincount(keyed.view(-1), minlength=9 * n).view(n, 9)
    ys = torch.arange(H, device=dev)[None, :, None].expand(n, H, W)
    xs = torch.arange(W, device=dev)[None, None, :].expand(n, H, W)
    wide = img.long()
    for s in range(9):
        sel = slot == s
        rows[:, 9 + 4 * s] = torch.where(sel, xs, W).amin(dim=(1, 2))
        rows[:, 10 + 4 * s] = torch.where(sel, ys, H).amin(dim=(1, 2))
        rows[:, 11 + 4 * s] = torch.where(sel, xs, -1).amax(dim=(1, 2))
        rows[:, 12 + 4 * s] = torch.where(sel, ys, -1).amax(dim=(1, 2))
        rows[:, 45 + 4 * s:45 + 4 * s + C] = (wide * sel[..., None]).sum(dim=(1, 2))
    rows[:, 81:81 + C] = (wide * wide).sum(dim=(1, 2))
    rows[:, 85] = (mask[:, :, :-1] != mask[:, :, 1:]).sum(dim=(1, 2))
    rows[:, 86] = (mask[:, :-1, :] != mask[:, 1:, :]).sum(dim=(1, 2))
    return rows


def kernel_mode(args):
    import torch
    from gan_segmentation_amd import pair_stats
    n = args.batch
    if args.skip_generate:
        R = SIZES[args.gan] // args.downscale
        g = torch.Generator(device="cuda").manual_seed(args.seed)
        img = torch.randint(0, 256, (n, R, R, 3), dtype=torch.uint8, device="cuda", generator=g)
        # coherent regions, as a decoder's masks: a coarse random class grid blown up 32-fold
        coarse = torch.randint(0, 3, (n, R // 32, R // 32), dtype=torch.uint8, device="cuda", generator=g)
        mask = coarse.repeat_interleave(32, dim=1).repeat_interleave(32, dim=2).contiguous()
        gen = None
    else:
        gen = build(args)
        img, mask = gen.generate_indexed(0, n, seed=args.seed)
    _, H, W, C = img.shape
    out = torch.empty((n, 88), dtype=torch.int64, device="cuda")

    calls = {"hip": 0, "torch": 0}   # every call the process makes, the check and the warm-up included: a trace's divisor

    def ours():
        calls["hip"] += 1
        return pair_stats.pair_stats(img, mask, out=out)

    def theirs():
        calls["torch"] += 1
        return torch_rows(torch, img, mask)

    if args.torch and not torch.equal(ours(), theirs()):
        sys.exit("pair_stats_bench.py: the torch composition and the kernel disagree")
    fn = theirs if args.torch else ours
    iters = max(1, args.iters // 20) if args.torch else args.iters
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    t = [timed(torch, fn, iters) for _ in range(args.rounds)]
    if gen is not None:
        gen.netG._model.ctx.check()
    alg_bytes = n * H * W * (C + 1)
    us = statistics.median(t)
    classes = int((pair_stats.unpack(ours())["count"].sum(dim=0) > 0).sum())
    print(json.dumps({"mode": "kernel", "form": "torch" if args.torch else "hip", "gan": args.gan, "batch": n, "pair": [H, W, C],
                      "generated": gen is not None, "slots_present": classes, "iters": iters, "rounds": args.rounds,
                      "calls_in_process": calls, "call_us": round(us, 2), "algorithmic_bytes": alg_bytes, "call_GBps": round(alg_bytes / us / 1e3, 1),
                      "rounds_us": [round(x, 2) for x in t],
                      "note": "call times are back-to-back calls timed with device events (launch gaps included); the kernels' own "
                              "time is their rows of a rocprofv3 --kernel-trace --stats run; calls_in_process counts every call "
                              "of either form that such a trace holds (check, warm-up and the slot count included)"}))


def step_mode(args):
    import torch
    from gan_segmentation_amd.dataset_writer import DatasetWriter
    gen = build(args)
    n = args.batch
    with tempfile.TemporaryDirectory() as tmp:
        writers = {name: DatasetWriter(os.path.join(tmp, name), gpu_jpeg=True, gpu_png=True, stats=(name == "stats"))
                   for name in ("plain", "stats")}

        def block(name, steps):
            w = writers[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(steps):
                img, mask = gen.generate_indexed(k * n, n, seed=args.seed)
                w.submit(img, mask, k * n, status=gen.snapshot_status())
            w.drain()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1000.0 / steps

        for name in writers:
            block(name, args.warmup)
        t = {"plain": [], "stats": []}
        for _ in range(args.rounds):
            for name in ("plain", "stats"):
                t[name].append(block(name, args.steps))
        for w in writers.values():
            w.close()
        gen.netG._model.ctx.check()
    m0, m1 = statistics.median(t["plain"]), statistics.median(t["stats"])
    print(json.dumps({"mode": "step", "gan": args.gan, "batch": n, "precision": args.precision, "steps_per_block": args.steps,
                      "rounds": args.rounds, "step_ms": round(m0, 4), "step_with_stats_ms": round(m1, 4),
                      "difference_us": round((m1 - m0) * 1000.0, 2), "difference_percent": round(100.0 * (m1 - m0) / m0, 3),
                      "step_rounds_ms": [round(x, 4) for x in t["plain"]], "step_with_stats_rounds_ms": [round(x, 4) for x in t["stats"]],
                      "note": "a step = generate_indexed + DatasetWriter.submit (GPU JPEG and PNG); a block ends with drain() and a "
                              "device synchronise, host clock"}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gan", default="ffhq", choices=sorted(SIZES))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--downscale", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--torch", action="store_true", help="kernel mode: time torch's composition of the same quantities instead")
    ap.add_argument("--skip-generate", action="store_true", help="kernel mode: random pairs of the same size, no generator")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("pair_stats_bench.py needs a HIP device: there is nothing to measure without one")
    (step_mode if args.step else kernel_mode)(args)


if __name__ == "__main__":
    main()
