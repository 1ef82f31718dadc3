"""Cost of the score histograms (csrc/gsa_scores.hip, csrc/gsa_scores.h) beside gsa_segmentation_eval, the nearest existing kernel:
both read the same 4 K + 1 bytes a pixel.

Two batches: an FFHQ evaluation batch, 8 x 2 x 1024^2, and 8 x 8 x 256^2.  Two kinds of logits each: "confident" (the label's class
at +12 and the others at -12, plus unit noise, with half a percent of the pixels undecided: more than 99 % of the pixels in the
clamp bins, what a trained decoder gives) and "noise" (uniform in [-8, 8]: every lane another bin).  scores_* is
gsa_score_histogram's two launches at shift 5, eval_* is gsa_segmentation_eval on the same tensors.  ROUNDS rounds; in each, every
case is timed once as ITERS back-to-back calls between two device events (launch gaps included), so the cases alternate.  Prints one
JSON line per case: the median, minimum and maximum us per call over the rounds, the algorithmic bytes per second, the time as a
multiple of those bytes at HBM_RATE (the 4.5 TB/s the project's one-pass kernels reach) and, for scores_*, as
a multiple of eval_* on the same tensors.  With --out the lines also go to that file.  With --logits FILE.npz (arrays ``logits``
(n, 2, R, R) float32 and ``labels`` (n, R, R) int8, R a divisor of 1024: what a decoder gave on annotated samples) a third kind,
"recorded", joins the FFHQ batch: those planes tiled to 1024^2 and repeated to 8 samples.

    python tools/scores_bench.py [--iters 200] [--rounds 5] [--logits FILE.npz] [--out profiles/scores_bench.txt]

GSA_HIP_LIBRARY selects another build of the library (how the kernel forms of DESIGN.md section 25 were timed).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_RATE = 4.5e12
BATCHES = {"ffhq_8x2x1024": (8, 2, 1024), "k8_8x8x256": (8, 8, 256)}


def make_logits(kind, n, K, R, seed):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, K, (n, R, R)).astype(np.int8)
    if kind == "confident":
        z = np.where(np.arange(K)[None, :, None, None] == y[:, None], 12.0, -12.0) + rng.standard_normal((n, K, R, R))
        few = rng.random((n, R, R)) < 0.005
        z = np.where(few[:, None], rng.standard_normal((n, K, R, R)), z)
    else:
        z = rng.uniform(-8, 8, (n, K, R, R))
    y[rng.random((n, R, R)) < 0.05] = -1
    return z.astype(np.float32), y


def recorded_logits(path, n, K, R):
    """The arrays of ``path`` tiled to (n, K, R, R) and (n, R, R)."""
    with np.load(path) as f:
        z, y = f["logits"].astype(np.float32), f["labels"].astype(np.int8)
    if z.ndim != 4 or z.shape[1] != K or y.shape != (z.shape[0],) + z.shape[2:] or z.shape[2] != z.shape[3] or R % z.shape[2]:
        sys.exit("%s: logits must be (n, %d, r, r) with r a divisor of %d and labels (n, r, r), got %s and %s" % (path, K, R, z.shape, y.shape))
    t = R // z.shape[2]
    pick = np.arange(n) % z.shape[0]
    return np.ascontiguousarray(np.tile(z[pick], (1, 1, t, t))), np.ascontiguousarray(np.tile(y[pick], (1, t, t)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--logits", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("scores_bench.py needs a HIP device: there is nothing to measure without one")
    from gan_segmentation_amd import score_ops
    from gan_segmentation_amd._runtime import DeviceModel, current_stream_ptr
    from gan_segmentation_amd.metrics import ScoreCurves

    model = DeviceModel(0)
    dev = model.device
    cases, alg_bytes, clamped, keep = {}, {}, {}, []
    for batch, (n, K, R) in BATCHES.items():
        rows = torch.empty((n, K, 2, score_ops.SCORE_BINS), dtype=torch.int64, device=dev)
        conf = torch.zeros((K, K), dtype=torch.int64, device=dev)
        lossf = torch.zeros((n,), dtype=torch.int64, device=dev)
        for kind in ("confident", "noise") + (("recorded",) if args.logits and batch.startswith("ffhq") else ()):
            z, y = recorded_logits(args.logits, n, K, R) if kind == "recorded" else make_logits(kind, n, K, R, seed=K)
            zt, yt = torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev)
            keep.append((zt, yt, rows, conf, lossf))
            name = "%s_%s" % (batch, kind)
            cases["scores_" + name] = lambda zt=zt, yt=yt, rows=rows: score_ops.score_histogram(zt, yt, shift=5, out=rows)
            cases["eval_" + name] = lambda zt=zt, yt=yt, n=n, K=K, R=R, conf=conf, lossf=lossf: model.ctx.segmentation_eval(
                current_stream_ptr(dev), n, K, R, R, zt.data_ptr(), yt.data_ptr(), conf.data_ptr(), lossf.data_ptr())
            alg_bytes["scores_" + name] = alg_bytes["eval_" + name] = n * R * R * (4 * K + 1)
            curves = ScoreCurves(K, shift=5, skip_bg=False)
            curves.update_rows(score_ops.score_histogram(zt, yt, shift=5).cpu().numpy())
            clamped["scores_" + name] = round(max(curves.clamped(c) for c in range(K)), 4)

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
    library = os.path.basename(os.environ.get("GSA_HIP_LIBRARY", "libgsa_hip.so"))
    lines = []
    for name, t in times.items():
        med = float(np.median(t))
        line = {"case": name, "library": library, "iters": args.iters, "rounds": args.rounds, "call_us": round(med, 2),
                "min_us": round(min(t), 2), "max_us": round(max(t), 2), "bytes": alg_bytes[name],
                "call_GBps": round(alg_bytes[name] / med / 1e3, 1), "x_hbm": round(med * 1e-6 / (alg_bytes[name] / HBM_RATE), 2)}
        if name.startswith("scores_"):
            line["x_eval"] = round(med / float(np.median(times["eval_" + name[len("scores_"):]])), 2)
            line["clamped"] = clamped[name]
        lines.append(json.dumps(line))
        print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
