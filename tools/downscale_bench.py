"""Cost of the downscaled step against the full-resolution step, bench.py's synthetic weights and inputs.

Step mode (default): alternates, in one process, blocks of the eager fused step at full resolution (gsa_generate) and at 1/f
(gsa_generate_downscaled), ROUNDS times after a warm-up, and prints the median ms per step of each with their ratio as one JSON line.

    python tools/downscale_bench.py [--gan ffhq] [--batch 8] [--precision fp32] [--factor 2] [--steps 10] [--rounds 5]

To-disk mode (--to-disk N): `main.py generate --limit N` on synthetic .params files, writing the files, with OUTPUT_DOWNSCALE 1
and f alternating ROUNDS times each after one warm-up run of each; prints the wall time of every run as one JSON line.

    python tools/downscale_bench.py --to-disk 2000 --batch 32 --rounds 2
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step_mode(args):
    import numpy as np
    import torch
    from gan_segmentation_amd.image_generator import ImageGenerator
    from tests.common import bench_setup

    gcfg, gp, dcfg, dp, z, noise = bench_setup(args.gan, args.batch)
    gens = {f: ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=args.batch, precision=args.precision,
                                          output_downscale=f) for f in (1, args.factor)}
    dev = gens[1].netG._model.device
    zd = torch.from_numpy(np.ascontiguousarray(z)).to(dev)
    nz = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in noise]
    n, R, nc = args.batch, 2 ** gcfg["max_res_log2"], gcfg["channels"]
    outs = {f: (torch.empty((n, R // f, R // f, nc), device=dev, dtype=torch.uint8),
                torch.empty((n, R // f, R // f), device=dev, dtype=torch.uint8)) for f in gens}
    for g in gens.values():
        g.graph_mode = "0"          # both steps eager: the comparison is of the kernels, not of graph replay

    def block(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            gens[f].generate_batch(zd, nz, out=outs[f])
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.steps

    for _ in range(args.warmup):
        for f in gens:
            gens[f].generate_batch(zd, nz, out=outs[f])
    torch.cuda.synchronize()
    t = {f: [] for f in gens}
    for _ in range(args.rounds):
        for f in gens:
            t[f].append(block(f))
    for g in gens.values():
        g.netG._model.ctx.check()
    m1, mf = statistics.median(t[1]), statistics.median(t[args.factor])
    print(json.dumps({"gan": args.gan, "batch": n, "precision": args.precision, "factor": args.factor, "steps_per_block": args.steps,
                      "rounds": args.rounds, "full_step_ms": round(m1, 4), "down_step_ms": round(mf, 4), "ratio": round(mf / m1, 4),
                      "full_rounds_ms": [round(x, 4) for x in t[1]], "down_rounds_ms": [round(x, 4) for x in t[args.factor]]}))


def disk_mode(args):
    from gan_segmentation_amd import main as cli
    from gan_segmentation_amd import params as P
    from gan_segmentation_amd import weights as W

    mr = W.GAN_MAX_RES_LOG2[args.gan]
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "models"))
        os.makedirs(os.path.join(d, "exp", "checkpoints"))
        P.save_params(os.path.join(d, "models", "stylegan-%s.params" % args.gan), W.synthetic_generator_params(W.generator_config(mr)))
        P.save_params(os.path.join(d, "exp", "checkpoints", "checkpoint_last.params"), W.synthetic_decoder_params(W.decoder_config(mr)))
        out_dir = os.path.join(d, "exp", "dataset", "train_generated")

        def run(f, limit):
            shutil.rmtree(out_dir, ignore_errors=True)
            cfg = {"BASE_DIR": os.path.join(d, "exp"), "GAN": args.gan, "GAN_DIR": os.path.join(d, "models"), "GAN_GPU_IDS": [0],
                   "GAN_BATCH_SIZE_PER_GPU": args.batch, "SOLVER_GPU_IDS": [0], "ANNOTATION": "segmentation",
                   "PRECISION": args.precision, "OUTPUT_DOWNSCALE": f}
            t = time.perf_counter()
            assert cli.generate(cfg, limit=limit) == 0
            dt = time.perf_counter() - t
            assert len(os.listdir(out_dir)) == 2 * limit
            return dt

        for f in (1, args.factor):
            run(f, args.batch)          # warm-up: code objects, encoders
        runs = []
        for _ in range(args.rounds):
            for f in (1, args.factor):
                runs.append({"factor": f, "seconds": round(run(f, args.to_disk), 3)})
        print(json.dumps({"gan": args.gan, "batch": args.batch, "precision": args.precision, "pairs": args.to_disk,
                          "runs": runs, "note": "wall time of main.generate incl. model load and file writes"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gan", default="ffhq")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--factor", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed block")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--to-disk", type=int, default=0, help="pairs per main.py generate run (0: step mode)")
    args = ap.parse_args()
    if args.to_disk:
        disk_mode(args)
    else:
        step_mode(args)


if __name__ == "__main__":
    main()
