"""Cost of the decoder losses (csrc/gsa_loss.hip, csrc/gsa_loss.h) beside gsa_train_softmax_ce, at the FFHQ decoder's output: one
sample, 2 classes, 1024 x 1024 pixels; and of one DecoderTrainer.step at FFHQ size with and without a LossSpec.

Entry cases, each on preallocated buffers (logits uniform in [-8, 8], a quarter of the labels -1, dist2 the boundary distance of a
blob mask): softmax_ce is the parent entry (a memset and one kernel); loss_plain is gsa_loss_softmax with gamma 0, "mean" and no
weights, the same loss; loss_all is gamma 2, "focal", class weights and a boundary table; loss_all_forward is the same without
dlogits.  ROUNDS rounds; in each, every case is timed once as ITERS back-to-back calls between two device events (launch gaps
included), so the cases alternate.  Prints one JSON line per case: the median, minimum and maximum us per call over the rounds and
the algorithmic bytes per second (logits read once and the gradient written once: 4 K bytes a pixel each, 1 for the label, 2 for
dist2 -- the second read of the inputs by the gradient pass is not counted).

Step cases: DecoderTrainer.step on the FFHQ decoder, batch 1, host clock around STEPS steps that end in a device synchronise, the
two trainers alternating over the rounds: step_default (softmax_ce) and step_spec (every option on: the boundary distance of the
labels, then the loss).

    python tools/loss_bench.py [--iters 200] [--rounds 5] [--steps 10] [--no-steps]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, K, H, W = 1, 2, 1024, 1024


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-steps", action="store_true", help="the entry cases only")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("loss_bench.py needs a HIP device: there is nothing to measure without one")
    from gan_segmentation_amd import loss_ops, mask_ops, weights as Wt
    from gan_segmentation_amd._runtime import launch
    from gan_segmentation_amd.trainer import DecoderTrainer
    from tests.test_boundary_host import class_blobs

    HW = H * W
    g = torch.Generator().manual_seed(0)
    logits = ((torch.rand(N, K, H, W, generator=g) * 2 - 1) * 8).cuda()
    blobs = torch.from_numpy(class_blobs(1, (N, H, W), K, sigma=6.0).astype(np.int8))
    blobs[torch.rand(N, H, W, generator=g) < 0.25] = -1
    labels = blobs.cuda()
    dist2 = mask_ops.boundary_distance(labels.view(torch.uint8), 5)
    cw = torch.tensor([0.5, 3.0]).cuda()
    table = torch.from_numpy(loss_ops.boundary_weight_table(5, 4.0, 2.0)).cuda()
    dev = logits.device
    ws = torch.empty(loss_ops.workspace_bytes(N, HW), dtype=torch.uint8, device=dev)
    sums = torch.empty((N, loss_ops.LOSS_SUMS), dtype=torch.float64, device=dev)
    loss = torch.empty(N, device=dev)
    dl = torch.empty_like(logits)

    def entry(gamma, norm, weighted, grad):
        launch("gsa_loss_softmax", dev, N, K, HW, logits.data_ptr(), labels.data_ptr(), cw.data_ptr() if weighted else None,
               dist2.data_ptr() if weighted else None, table.data_ptr() if weighted else None, gamma, norm, 1.0, ws.data_ptr(),
               sums.data_ptr(), loss.data_ptr(), dl.data_ptr() if grad else None)

    cases = {
        "softmax_ce": lambda: launch("gsa_train_softmax_ce", dev, N, K, HW, logits.data_ptr(), labels.data_ptr(), loss.data_ptr(),
                                     dl.data_ptr(), 1.0),
        "loss_plain": lambda: entry(0.0, 0, False, True),
        "loss_all": lambda: entry(2.0, 2, True, True),
        "loss_all_forward": lambda: entry(2.0, 2, True, False),
    }
    pixels = N * HW
    alg_bytes = {"softmax_ce": pixels * (8 * K + 1), "loss_plain": pixels * (8 * K + 1), "loss_all": pixels * (8 * K + 3),
                 "loss_all_forward": pixels * (4 * K + 3)}
    times = {k: [] for k in cases}
    for fn in cases.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in cases.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1000.0 / args.iters)
    for name, t in times.items():
        print(json.dumps({"case": name, "shape": [N, K, H, W], "iters": args.iters, "rounds": args.rounds,
                          "call_us": round(float(np.median(t)), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2),
                          "call_GBps": round(alg_bytes[name] / float(np.median(t)) / 1e3, 1)}), flush=True)
    if args.no_steps:
        return

    dcfg = Wt.decoder_config(Wt.GAN_MAX_RES_LOG2["ffhq"])
    chans = dcfg["in_channels"]
    rng = np.random.default_rng(0)
    feats = [torch.from_numpy(rng.standard_normal((1, c, 4 << i, 4 << i)).astype(np.float32)).cuda() for i, c in enumerate(chans)]
    spec = loss_ops.LossSpec(gamma=2.0, normalise="focal", class_weights=[0.5, 3.0], boundary={"weight": 4.0, "sigma": 2.0, "radius": 5})
    trainers = {"step_default": DecoderTrainer(dcfg, Wt.initial_decoder_params(dcfg, 1), lr=1e-4, seed=1),
                "step_spec": DecoderTrainer(dcfg, Wt.initial_decoder_params(dcfg, 1), lr=1e-4, seed=1, loss=spec)}
    step_ms = {k: [] for k in trainers}
    for tr in trainers.values():
        tr.step(feats, labels)
        tr.step(feats, labels)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, tr in trainers.items():
            t0 = time.perf_counter()
            for _ in range(args.steps):
                tr.step(feats, labels)
            torch.cuda.synchronize()
            step_ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    for name, t in step_ms.items():
        print(json.dumps({"case": name, "gan": "ffhq", "steps": args.steps, "rounds": args.rounds, "step_ms": round(float(np.median(t)), 3),
                          "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}), flush=True)


if __name__ == "__main__":
    main()
