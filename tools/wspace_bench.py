"""Cost of the style-mixed W-space step against the z step: FFHQ, batch 8, bench.py's synthetic weights and inputs.

Alternates, in one process, blocks of the eager fused z step (gsa_generate) and of the mixed step at prob 1.0 (the second
mapping launch, the torch mix into (8, 18, 512) dlatents and gsa_generate_w), ROUNDS times after a warm-up, and prints the
median ms per step of each with their ratio as one JSON line.

    python tools/wspace_bench.py [--steps 10] [--rounds 5] [--warmup 3] [--precision fp32]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="steps per timed block")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="fp32")
    args = ap.parse_args()

    import numpy as np
    import torch
    from gan_segmentation_amd import style_mix as M
    from gan_segmentation_amd.image_generator import ImageGenerator
    from tests.common import bench_setup

    gcfg, gp, dcfg, dp, z, noise = bench_setup("ffhq", args.batch)
    gen = ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=args.batch, precision=args.precision)
    gen.graph_mode = "0"            # both steps eager: the W path is never captured
    g = gen.netG
    dev = g._model.device
    L, n = g.num_style_layers, args.batch
    zd = torch.from_numpy(np.ascontiguousarray(z)).to(dev)
    zb = torch.from_numpy(np.random.default_rng(7).standard_normal(z.shape).astype(np.float32)).to(dev)
    nz = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in noise]
    _mix, cutoff = M.mix_plan(0, 0, n, 1.0, L)
    sel = torch.from_numpy(M.layer_select(np.ones(n, bool), cutoff, L)).to(dev)
    img = torch.empty((n, 1024, 1024, 3), device=dev, dtype=torch.uint8)
    mask = torch.empty((n, 1024, 1024), device=dev, dtype=torch.uint8)

    def z_step():
        gen.generate_batch(zd, nz, out=(img, mask))

    def w_step():
        w_a, w_b = g.mapping(zd), g.mapping(zb)
        dl = torch.where(sel[:, :, None], w_b[:, None, :], w_a[:, None, :]).contiguous()
        gen.generate_batch_w(dl, nz, out=(img, mask))

    def block(step):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            step()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.steps

    for _ in range(args.warmup):
        z_step()
        w_step()
    torch.cuda.synchronize()
    tz, tw = [], []
    for _ in range(args.rounds):
        tz.append(block(z_step))
        tw.append(block(w_step))
    g._model.ctx.check()
    mz, mw = statistics.median(tz), statistics.median(tw)
    print(json.dumps({"batch": n, "precision": args.precision, "steps_per_block": args.steps, "rounds": args.rounds,
                      "z_step_ms": round(mz, 4), "mixed_w_step_ms": round(mw, 4), "ratio": round(mw / mz, 4),
                      "z_rounds_ms": [round(t, 4) for t in tz], "w_rounds_ms": [round(t, 4) for t in tw]}))


if __name__ == "__main__":
    main()
