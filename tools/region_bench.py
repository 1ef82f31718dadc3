"""Cost of the region term (csrc/gsa_region.hip, csrc/gsa_region.h) beside the decoder losses it is added to, at the FFHQ decoder's
output: one sample, 2 classes, 1024 x 1024 pixels; and of one DecoderTrainer.step at FFHQ size with and without it.

Entry cases, each on preallocated buffers (logits uniform in [-8, 8], blob labels, a quarter of them -1): copy is a device copy of
the logits (4 K bytes a pixel read and written: the rate the floor of the pass is taken from); loss_all is gsa_loss_softmax with
gamma 2, "focal" and class weights, the cross-entropy term of the same step; region_forward is gsa_region_tversky without dlogits
(the first launch and a one-workgroup second launch); region_write writes the gradient; region_accumulate adds it into an
existing one.  ROUNDS rounds; in each, every case is timed once as ITERS back-to-back calls between two device events (launch gaps
included), so the cases alternate.  Prints one JSON line per case: the median, minimum and maximum us per call over the rounds, the
bytes the pass moves (per pixel 4 K + 1 read by the first launch; the second reads them again and writes 4 K, or reads and writes
4 K) and that count over the time.

Step cases: DecoderTrainer.step on the FFHQ decoder, batch 1, host clock around STEPS steps that end in a device synchronise, the
trainers alternating over the rounds: step_default (softmax_ce), step_spec (gamma 2, "focal", class weights) and step_region (the
same with region = {weight 1, alpha 0.3, beta 0.7}).

    python tools/region_bench.py [--iters 200] [--rounds 5] [--steps 10] [--no-steps]
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
        sys.exit("region_bench.py needs a HIP device: there is nothing to measure without one")
    from gan_segmentation_amd import loss_ops, weights as Wt
    from gan_segmentation_amd._runtime import launch
    from gan_segmentation_amd.trainer import DecoderTrainer
    from tests.test_boundary_host import class_blobs

    HW = H * W
    g = torch.Generator().manual_seed(0)
    logits = ((torch.rand(N, K, H, W, generator=g) * 2 - 1) * 8).cuda()
    blobs = torch.from_numpy(class_blobs(1, (N, H, W), K, sigma=6.0).astype(np.int8))
    blobs[torch.rand(N, H, W, generator=g) < 0.25] = -1
    labels = blobs.cuda()
    cw = torch.tensor([0.5, 3.0]).cuda()
    dev = logits.device
    ws = torch.empty(loss_ops.workspace_bytes(N, HW), dtype=torch.uint8, device=dev)
    sums = torch.empty((N, loss_ops.LOSS_SUMS), dtype=torch.float64, device=dev)
    rws = torch.empty(loss_ops.region_workspace_bytes(N, K, HW), dtype=torch.uint8, device=dev)
    rsums = torch.empty((N, loss_ops.REGION_SUMS, K), dtype=torch.float64, device=dev)
    index = torch.empty((N, K), device=dev)
    loss = torch.empty(N, device=dev)
    dl = torch.zeros_like(logits)

    def region(grad, accumulate):
        launch("gsa_region_tversky", dev, N, K, HW, logits.data_ptr(), labels.data_ptr(), cw.data_ptr(), 0.3, 0.7, 1.0, 0, 1e-3,
               accumulate, rws.data_ptr(), rsums.data_ptr(), index.data_ptr(), loss.data_ptr(), dl.data_ptr() if grad else None)

    cases = {
        "copy": lambda: dl.copy_(logits),
        "loss_all": lambda: launch("gsa_loss_softmax", dev, N, K, HW, logits.data_ptr(), labels.data_ptr(), cw.data_ptr(), None, None,
                                   2.0, 2, 1.0, ws.data_ptr(), sums.data_ptr(), loss.data_ptr(), dl.data_ptr()),
        "region_forward": lambda: region(False, 0),
        "region_write": lambda: region(True, 0),
        "region_accumulate": lambda: region(True, 1),
    }
    pixels = N * HW
    read = 4 * K + 1
    moved = {"copy": pixels * 8 * K, "loss_all": pixels * (2 * read + 4 * K), "region_forward": pixels * read,
             "region_write": pixels * (2 * read + 4 * K), "region_accumulate": pixels * (2 * read + 8 * K)}
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
                          "moved_MB": round(moved[name] / 1e6, 2), "moved_GBps": round(moved[name] / float(np.median(t)) / 1e3, 1)}),
              flush=True)
    if args.no_steps:
        return

    dcfg = Wt.decoder_config(Wt.GAN_MAX_RES_LOG2["ffhq"])
    chans = dcfg["in_channels"]
    rng = np.random.default_rng(0)
    feats = [torch.from_numpy(rng.standard_normal((1, c, 4 << i, 4 << i)).astype(np.float32)).cuda() for i, c in enumerate(chans)]
    base = dict(gamma=2.0, normalise="focal", class_weights=[0.5, 3.0])
    specs = {"step_default": None, "step_spec": loss_ops.LossSpec(**base),
             "step_region": loss_ops.LossSpec(region={"weight": 1.0, "alpha": 0.3, "beta": 0.7}, **base)}
    trainers = {k: DecoderTrainer(dcfg, Wt.initial_decoder_params(dcfg, 1), lr=1e-4, seed=1, loss=s) for k, s in specs.items()}
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
