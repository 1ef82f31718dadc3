"""Cost of the pair previews' kernel (csrc/gsa_overlay.hip) on generated pairs, bench.py's synthetic weights.

One generated batch, then ROUNDS rounds of ITERS launches of gsa_overlay and of torch's own composition of the same work on the same
tensors (table gather, edge test on shifted views, integer blend, f x f block sum, cells of the sheet), each timed with device events;
prints the median us per call of both, the kernel's algorithmic bytes (n*H*W*(C+1) read once + the sheet written once) and the
bytes/s reached beside the 4.5 TB/s of the project's one-pass halo kernels, as one JSON line.  The two results
are compared byte for byte first.  Call times are back-to-back launches (launch gaps included); for the kernel's own time run it
under the profiler, in a run of its own, and read overlay_kernel's row:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/overlay_bench.py --gan ffhq --batch 8 --factor 8 --cols 4

    python tools/overlay_bench.py [--gan ffhq] [--batch 8] [--factor 1] [--cols 1] [--iters 50] [--rounds 5] [--no-torch]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ONE_PASS_BYTES_PER_S = 4.5e12


def edges(torch, mask):
    """Whether a 4-neighbour inside the same plane holds another value, on shifted views."""
    edge = torch.zeros(mask.shape, dtype=torch.bool, device=mask.device)
    d = mask[:, 1:] != mask[:, :-1]
    edge[:, 1:] |= d
    edge[:, :-1] |= d
    d = mask[:, :, 1:] != mask[:, :, :-1]
    edge[:, :, 1:] |= d
    edge[:, :, :-1] |= d
    return edge


def torch_composition(torch, img, mask, lut, factor, cols):
    """The rule of csrc/gsa_overlay.h in torch operators -> the sheet, uint8."""
    n, H, W, C = img.shape
    rows = lut[mask.long()]                                             # (n, H, W, 6)
    w = torch.where(edges(torch, mask), rows[..., 5], rows[..., 4]).clamp(max=128).int()[..., None]
    b = (w * rows[..., :C].int() + (128 - w) * img.int()) >> 7
    h, wd = H // factor, W // factor
    if factor > 1:
        b = (b.view(n, h, factor, wd, factor, C).sum(dim=(2, 4)) + factor * factor // 2) >> (2 * (factor.bit_length() - 1))
    b = b.to(torch.uint8)
    cells = -(-n // cols) * cols
    if cells > n:
        b = torch.cat([b, torch.zeros((cells - n, h, wd, C), dtype=torch.uint8, device=b.device)])
    return b.view(cells // cols, cols, h, wd, C).permute(0, 2, 1, 3, 4).reshape(cells // cols * h, cols * wd, C)


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
    ap.add_argument("--factor", type=int, default=1)
    ap.add_argument("--cols", type=int, default=1)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="time the kernel only (a profiler run then lists its kernels alone)")
    args = ap.parse_args(argv)

    import torch
    from gan_segmentation_amd import preview
    from gan_segmentation_amd.image_generator import ImageGenerator
    from tests.common import bench_setup
    gcfg, gp, dcfg, dp, _z, _noise = bench_setup(args.gan, args.batch)
    gen = ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=args.batch)
    img, mask = gen.generate_indexed(0, args.batch, seed=0)
    img, mask = img.clone(), mask.clone()
    lut_host = preview.make_lut(preview.DATASET_COLOURS, alpha=0.5, outline=1.0)
    lut = torch.from_numpy(lut_host).to(img.device)
    n, H, W, C = img.shape
    out = torch.empty(preview.sheet_shape(n, H, W, C, args.cols, args.factor), dtype=torch.uint8, device=img.device)

    def kernel():
        return preview.contact_sheet(img, mask, args.cols, lut, args.factor, out=out)

    def composition():
        return torch_composition(torch, img, mask, lut, args.factor, args.cols)

    kernel()
    torch.cuda.synchronize()
    same = None
    if not args.no_torch:
        same = bool(torch.equal(kernel(), composition()))
    for fn in ([kernel] if args.no_torch else [kernel, composition]):      # warm up
        timed(torch, fn, 5)
    k_rounds, t_rounds = [], []
    for _ in range(args.rounds):                                            # alternating
        k_rounds.append(timed(torch, kernel, args.iters))
        if not args.no_torch:
            t_rounds.append(timed(torch, composition, max(1, args.iters // 5)))
    k_us = statistics.median(k_rounds)
    nbytes = n * H * W * (C + 1) + out.numel()
    edge_share = float(edges(torch, mask).float().mean())
    result = {"gan": args.gan, "batch": n, "pair": [H, W, C], "factor": args.factor, "cols": args.cols, "sheet": list(out.shape),
              "iters": args.iters, "rounds": args.rounds, "overlay_call_us": round(k_us, 2), "overlay_rounds_us": [round(v, 2) for v in k_rounds],
              "algorithmic_bytes": nbytes, "overlay_call_GBps": round(nbytes / k_us / 1e3, 1),
              "share_of_one_pass_rate": round(nbytes / (k_us * 1e-6) / ONE_PASS_BYTES_PER_S, 3),
              "least_us_at_one_pass_rate": round(nbytes / ONE_PASS_BYTES_PER_S * 1e6, 2),
              "torch_composition_us": round(statistics.median(t_rounds), 1) if t_rounds else None,
              "torch_rounds_us": [round(v, 1) for v in t_rounds], "torch_result_equal": same,
              "foreground_share": round(float((mask != 0).float().mean()), 5), "edge_pixel_share": round(edge_share, 5),
              "note": "call times are back-to-back launches timed with device events (launch gaps included); the kernel's own time is its "
                      "row of a rocprofv3 --kernel-trace --stats run"}
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
