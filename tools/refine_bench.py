"""Cost of the image-guided mask refinement's kernel (csrc/gsa_refine.hip) on generated pairs, bench.py's synthetic weights.

One generated batch, then for every radius ROUNDS rounds of ITERS launches of gsa_mask_refine (one pass, K classes, the default
weights of that radius) and of torch's own composition of the same rule on the same tensors (one shifted-view step per tap), each
timed with device events; prints one JSON line per radius: the median us per call of both, the taps of the batch (pixels x window)
and the kernel's instruction bound (VALU and LDS instructions per tap counted in the disassembly, times the
taps, over the chip's issue rate).  The two results are compared byte for byte before anything is timed.  Call times are
back-to-back launches (launch gaps included); for the kernel's own time run it under the profiler, in a run of its own without
counters, and read the rows of mask_refine_kernel<R, ...>:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/refine_bench.py --gan ffhq --batch 8 --no-torch

    python tools/refine_bench.py [--gan ffhq] [--batch 8] [--classes 2] [--radii 1 3 5] [--iters 20] [--rounds 5] [--no-torch]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# The yardstick: instructions per tap of the timed instantiations (K <= 2, three channels, dword form), counted in the disassembly of
# the row pass that serves both output rows (DESIGN.md section 22 has the count), and the issue rates they are held against: a wave64
# VALU instruction takes 2 cycles of one of a CU's four SIMDs; the CU's one LDS array takes 2 cycles for a conflict-free byte or dword
# read of a wave and 4 for a ds_read2_b32.
VALU_PER_TAP = {1: 4.58, 3: 4.11, 5: 3.98}
LDS_CYCLES_PER_TAP = {1: 3.0, 3: 2.86, 5: 2.82}
CUS, SIMDS_PER_CU, CLOCK_HZ = 256, 4, 2.4e9
VALU_CYCLES_PER_WAVE_INSTRUCTION = 2


def instruction_bound_us(taps, radius):
    """(VALU bound, LDS bound) in us of ``taps`` taps at ``radius``: wave-taps per CU times the cycles of a tap, at CLOCK_HZ."""
    wave_taps_per_cu = taps / 64.0 / CUS
    valu = wave_taps_per_cu / SIMDS_PER_CU * VALU_PER_TAP[radius] * VALU_CYCLES_PER_WAVE_INSTRUCTION / CLOCK_HZ * 1e6
    lds = wave_taps_per_cu * LDS_CYCLES_PER_TAP[radius] / CLOCK_HZ * 1e6
    return valu, lds


def torch_composition(torch, img, mask, tables, classes, radius):
    """The rule of csrc/gsa_refine.h in torch operators -> the refined mask, uint8."""
    n, H, W = mask.shape
    wr, ws = tables[:256].int(), tables[256:].int().view(11, 11)
    colour = img.int()
    votes = torch.zeros((classes, n, H, W), dtype=torch.int32, device=mask.device)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if abs(dy) >= H or abs(dx) >= W:
                continue
            p = (slice(None), slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx)))
            q = (slice(None), slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx)))
            d = (colour[p] - colour[q]).abs().sum(dim=-1).clamp(max=255)
            w = wr[d.long()] * ws[dy + 5, dx + 5]
            u = mask[q]
            for c in range(classes):
                votes[c][p] += torch.where(u == c, w, torch.zeros_like(w))
    best, first = votes.max(dim=0)
    # torch's max returns some index of the maximum: the smallest one is found by comparison instead
    first = torch.full_like(mask, classes)
    for c in range(classes - 1, -1, -1):
        first = torch.where(votes[c] == best, torch.full_like(mask, c), first)
    mine = torch.gather(votes, 0, mask.clamp(max=classes - 1).long()[None])[0]
    return torch.where((mask >= classes) | (mine == best), mask, first)


def timed(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gan", default="ffhq")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--radii", type=int, nargs="+", default=[1, 3, 5])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="time the kernel only (a profiler run then lists its kernels alone)")
    args = ap.parse_args(argv)

    import torch
    from gan_segmentation_amd import mask_ops
    from gan_segmentation_amd.image_generator import ImageGenerator
    from tests.common import bench_setup
    gcfg, gp, dcfg, dp, _z, _noise = bench_setup(args.gan, args.batch)
    gen = ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=args.batch)
    img, mask = gen.generate_indexed(0, args.batch, seed=0)
    img, mask = img.clone(), mask.clone()
    n, H, W, C = img.shape
    out = torch.empty_like(mask)
    for radius in args.radii:
        tables = torch.from_numpy(mask_ops.refine_tables(radius)).to(img.device)

        def kernel():
            return mask_ops.refine(img, mask, 1, radius, args.classes, tables=tables, out=out)

        def composition():
            return torch_composition(torch, img, mask, tables, args.classes, radius)

        kernel()
        torch.cuda.synchronize()
        same = None if args.no_torch else bool(torch.equal(kernel(), composition()))
        changed = float((out != mask).float().mean())
        timed(torch, kernel, 5)                                             # warm up
        k_rounds, t_rounds = [], []
        for _ in range(args.rounds):                                        # alternating
            k_rounds.append(timed(torch, kernel, args.iters))
            if not args.no_torch:
                t_rounds.append(timed(torch, composition, 1))
        k_us = statistics.median(k_rounds)
        taps = n * H * W * (2 * radius + 1) ** 2
        valu_us, lds_us = instruction_bound_us(taps, radius) if radius in VALU_PER_TAP and args.classes <= 2 else (None, None)
        bound_us = None if valu_us is None else max(valu_us, lds_us)
        print(json.dumps({"gan": args.gan, "batch": n, "pair": [H, W, C], "classes": args.classes, "radius": radius, "iters": args.iters,
                          "rounds": args.rounds, "refine_call_us": round(k_us, 2), "refine_rounds_us": [round(v, 2) for v in k_rounds],
                          "taps": taps, "valu_per_tap": VALU_PER_TAP.get(radius), "lds_cycles_per_tap": LDS_CYCLES_PER_TAP.get(radius),
                          "valu_bound_us": None if valu_us is None else round(valu_us, 2), "lds_bound_us": None if lds_us is None else round(lds_us, 2),
                          "call_over_bound": None if bound_us is None else round(k_us / bound_us, 2),
                          "torch_composition_us": round(statistics.median(t_rounds), 1) if t_rounds else None,
                          "torch_rounds_us": [round(v, 1) for v in t_rounds], "torch_result_equal": same,
                          "changed_pixel_share": round(changed, 5), "foreground_share": round(float((mask != 0).float().mean()), 5),
                          "note": "call times are back-to-back launches timed with device events (launch gaps included); the kernel's own "
                                  "time is its row of a rocprofv3 --kernel-trace --stats run"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
