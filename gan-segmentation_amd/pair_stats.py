"""On-device statistics of generated pairs and the dataset report made of them (include/gsa_stats.h, csrc/gsa_stats.hip,
DESIGN.md section 16).  The reference has no counterpart: at 0.8 pairs/s a person can watch the samples go by.

``pair_stats(img, mask)`` enqueues one pass over an (image, mask) batch on the current stream and returns one int64 row of
``ROW`` = 88 words per sample: per mask slot (values 0..7, then "8 and above") the pixel count, bounding box and channel sums,
per channel the sum of squares, and the two edge counts -- all integers, so the rows are the same for any batch size, launch shape
and number of ranks.  ``unpack`` names the fields, ``summarise`` turns the rows of a dataset into the report a consumer needs
(class frequencies and weights, Normalize constants, empty masks), ``DatasetWriter(stats=True)`` collects them while `generate`
writes, and ``python -m gan_segmentation_amd.pair_stats DIR`` merges the shard files of a run.  No CPU fallback for the pass."""
import glob
import json
import os
import statistics
import sys

import numpy as np

SLOTS, CHANNELS, ROW = 9, 4, 88
MAX_EXTENT = 65535
# name -> (first word, shape of the field inside a row): the offsets of include/gsa_stats.h
FIELDS = {
    "count": (0, (SLOTS,)),
    "box": (9, (SLOTS, 4)),             # x0, y0, x1, y1; an empty slot: W, H, -1, -1
    "csum": (45, (SLOTS, CHANNELS)),
    "sqsum": (81, (CHANNELS,)),
    "edge_h": (85, ()),
    "edge_v": (86, ()),
}
SHARD_FORMAT = "pair_stats_%06d_%06d.npz"
SUMMARY_NAME = "pair_stats_summary.json"

def check_pair_stats(v):
    """The PAIR_STATS switch: a real bool (ValueError otherwise -- 1, "yes" or None are not an answer)."""
    if not isinstance(v, bool):
        raise ValueError("PAIR_STATS must be true or false, got %r" % (v,))
    return v


def pair_stats(img, mask, out=None):
    """img (n, H, W, C) or (H, W, C) contiguous uint8 CUDA tensor with C in 1..4, or None (labels only: C = 0); mask (n, H, W) or
    (H, W) contiguous uint8 CUDA tensor on the same device, H and W in 1..65535 with H * W < 2^31 -> int64 (n, 88) on that device
    (new, or ``out``, every word of which is overwritten): the rows of include/gsa_stats.h.  Enqueued on the current stream of the
    mask's device, no synchronisation; the inputs are not written.  ValueError on anything else; no CPU fallback."""
    import torch
    from ._runtime import is_device_tensor, launch

    def u8(t, dims, what):
        if not is_device_tensor(t, torch.uint8, dims=dims):
            raise ValueError("%s must be a contiguous uint8 CUDA tensor with %s dimensions" % (what, " or ".join(map(str, dims))))

    u8(mask, (2, 3), "mask")
    H, W = mask.shape[-2:]
    n = mask.shape[0] if mask.dim() == 3 else 1
    C = 0
    if img is not None:
        u8(img, (mask.dim() + 1,), "img")
        C = img.shape[-1]
        if tuple(img.shape[:-1]) != tuple(mask.shape) or img.device != mask.device or not 1 <= C <= CHANNELS:
            raise ValueError("img must be %s + (C,) with C in 1..%d on %s, got %s on %s"
                             % (tuple(mask.shape), CHANNELS, mask.device, tuple(img.shape), img.device))
    if not 1 <= H <= MAX_EXTENT or not 1 <= W <= MAX_EXTENT or H * W >= 2 ** 31:
        raise ValueError("pair_stats takes planes whose sides are 1..%d px with fewer than 2^31 pixels, got %dx%d" % (MAX_EXTENT, H, W))
    dev = mask.device
    if out is not None and not is_device_tensor(out, torch.int64, shape=(n, ROW), device=dev):
        raise ValueError("out must be a contiguous int64 tensor (%d, %d) on %s" % (n, ROW, dev))
    if out is None:
        out = torch.empty((n, ROW), dtype=torch.int64, device=dev)
    if n:
        launch("gsa_pair_stats", dev, n, H, W, C, img.data_ptr() if C else None, mask.data_ptr(), out.data_ptr())
    return out


def unpack(rows):
    """rows (..., 88), a tensor or an array -> {"count": (..., 9), "box": (..., 9, 4), "csum": (..., 9, 4), "sqsum": (..., 4),
    "edge_h": (...), "edge_v": (...)}: views of ``rows``, nothing is copied."""
    if rows.shape[-1] != ROW:
        raise ValueError("rows must end in %d words, got %s" % (ROW, tuple(rows.shape)))
    lead = tuple(rows.shape[:-1])
    out = {}
    for name, (first, shape) in FIELDS.items():
        size = int(np.prod(shape, dtype=np.int64))
        out[name] = rows[..., first:first + size].reshape(lead + shape) if shape else rows[..., first]
    return out


def _quantile(sorted_values, q):
    """Linear interpolation between order statistics (numpy's default), on a sorted list of floats."""
    pos = q * (len(sorted_values) - 1)
    lo = int(pos)
    hi = min(lo + 1, len(sorted_values) - 1)
    return sorted_values[lo] + (sorted_values[hi] - sorted_values[lo]) * (pos - lo)


def summarise(index, rows, H, W, C, num_classes=None):
    """The report of a dataset from its rows: ``index`` (m,) global sample indices, ``rows`` (m, 88) int64, both host arrays; H, W, C
    the size of every pair.  Pure host code on Python integers (exact) and float64.  -> a plain dict (JSON-serialisable):

    samples, H, W, C, num_classes
                    m and the sizes; num_classes = the argument, or 1 + the highest slot below 8 that holds a pixel.
    pixels          per slot (9 integers): the sum of count[s] over the samples.  Their sum is m * H * W.
    frequency       per slot: pixels[s] / (m * H * W).  They sum to 1.
    presence        per slot: the number of samples with count[s] > 0.
    weights_inverse_frequency
                    per slot, for the classes present (pixels[s] > 0, s < num_classes): (1 / frequency[s]) scaled so that the
                    weights of the present classes have mean 1; null for every other slot.
    weights_median_frequency
                    per slot, for the classes present: median(f) / f[s] with f[s] = pixels[s] / (presence[s] * H * W), the
                    frequency of s among the samples that hold it (median-frequency balancing); null for every other slot.
    mean, std       per channel c < C in 0..255 units: N = m * H * W, mean = sum_s csum[s][c] / N, var = sqsum[c] / N - mean^2 (the
                    population variance, clamped at 0), std = sqrt(var) -- from the exact integer sums, in float64.
    mean_unit, std_unit
                    mean / 255 and std / 255: a consumer's Normalize constants.
    foreground_fraction
                    of the per-sample share of pixels in slots 1..7: min, median, max and deciles (11 values, the 0th..100th
                    percentile in steps of 10, linear interpolation).
    empty_masks     the sorted global indices of the samples with no pixel in slots 1..7.
    mean_edges      the mean over the samples of edge_h + edge_v."""
    index = [int(i) for i in np.asarray(index).reshape(-1)]
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] != ROW or rows.shape[0] != len(index):
        raise ValueError("rows must be (%d, %d), got %s" % (len(index), ROW, rows.shape))
    if not index:
        raise ValueError("no samples to summarise")
    H, W, C = int(H), int(W), int(C)
    table = [[int(v) for v in row] for row in rows.tolist()]
    m, plane = len(table), H * W
    total = m * plane
    f_count, f_csum, f_sq = FIELDS["count"][0], FIELDS["csum"][0], FIELDS["sqsum"][0]
    f_eh, f_ev = FIELDS["edge_h"][0], FIELDS["edge_v"][0]
    pixels = [sum(r[f_count + s] for r in table) for s in range(SLOTS)]
    if sum(pixels) != total:
        raise ValueError("the counts hold %d pixels, %d samples of %dx%d hold %d" % (sum(pixels), m, H, W, total))
    presence = [sum(1 for r in table if r[f_count + s] > 0) for s in range(SLOTS)]
    if num_classes is None:
        num_classes = 1 + max([s for s in range(SLOTS - 1) if pixels[s] > 0], default=0)
    num_classes = int(num_classes)
    frequency = [p / total for p in pixels]
    inverse, median_f = frequency_weights(pixels, presence, plane, total, min(num_classes, SLOTS - 1))
    mean, std = [], []
    for c in range(C):
        mu = sum(r[f_csum + 4 * s + c] for r in table for s in range(SLOTS)) / total
        var = sum(r[f_sq + c] for r in table) / total - mu * mu
        mean.append(mu)
        std.append(max(var, 0.0) ** 0.5)
    fg = [sum(r[f_count + s] for s in range(1, SLOTS - 1)) for r in table]
    share = sorted(v / plane for v in fg)
    return {
        "samples": m, "H": H, "W": W, "C": C, "num_classes": num_classes,
        "pixels": pixels, "frequency": frequency, "presence": presence,
        "weights_inverse_frequency": inverse, "weights_median_frequency": median_f,
        "mean": mean, "std": std, "mean_unit": [v / 255.0 for v in mean], "std_unit": [v / 255.0 for v in std],
        "foreground_fraction": {"min": share[0], "median": _quantile(share, 0.5), "max": share[-1],
                                "deciles": [_quantile(share, k / 10.0) for k in range(11)]},
        "empty_masks": sorted(i for i, v in zip(index, fg) if v == 0),
        "mean_edges": sum(r[f_eh] + r[f_ev] for r in table) / m,
    }


def frequency_weights(pixels, presence, plane, total, classes):
    """The two class-weight vectors "for the loss" from per-class counts: ``pixels[s]`` pixels of class s among ``total`` pixels (ignored
    ones included) in samples of ``plane`` pixels, ``presence[s]`` samples that hold the class; the classes are 0 .. ``classes`` - 1.
    -> (inverse, median), lists as long as ``pixels``, as ``summarise`` documents them: (1 / frequency[s]) scaled so that the weights of
    the present classes have mean 1, and median(f) / f[s] with f[s] = pixels[s] / (presence[s] * plane).  None for a class without a
    pixel and for every entry from ``classes`` up.  What ``summarise`` reports and ``loss_ops.class_weights_from_masks`` computes."""
    inverse, median_f = [None] * len(pixels), [None] * len(pixels)
    present = [s for s in range(classes) if pixels[s] > 0]
    if present:
        raw = {s: 1.0 / (pixels[s] / total) for s in present}
        scale = len(present) / sum(raw.values())
        among = {s: pixels[s] / (presence[s] * plane) for s in present}
        med = statistics.median(among.values())
        for s in present:
            inverse[s] = raw[s] * scale
            median_f[s] = med / among[s]
    return inverse, median_f


# ---- shard files -----------------------------------------------------------------------------------------------------------
def save_shard(dst_dir, index, rows, H, W, C):
    """One ``pair_stats_<first>_<last + 1>.npz`` with index (int64), rows, H, W, C, sorted by index -> its path."""
    index = np.asarray(index, np.int64).reshape(-1)
    rows = np.asarray(rows, np.int64).reshape(-1, ROW)
    if index.size == 0 or index.size != rows.shape[0]:
        raise ValueError("a shard holds one row per index and at least one")
    order = np.argsort(index, kind="stable")
    index, rows = index[order], np.ascontiguousarray(rows[order])
    path = os.path.join(dst_dir, SHARD_FORMAT % (int(index[0]), int(index[-1]) + 1))
    with open(path, "wb") as f:
        np.savez(f, index=index, rows=rows, H=np.int64(H), W=np.int64(W), C=np.int64(C))
    return path


def merge_shards(src_dir):
    """Every pair_stats_*.npz of ``src_dir`` -> (index, rows, H, W, C), sorted by index: index (m,) int64 = first .. first + m - 1,
    rows (m, 88) int64.  ValueError, naming the files, on no shard, differing H/W/C, a duplicate index or a gap."""
    paths = sorted(p for p in glob.glob(os.path.join(src_dir, "pair_stats_*.npz")))
    if not paths:
        raise ValueError("no pair_stats_*.npz in %s" % src_dir)
    size, index, rows, owner = None, [], [], []
    for p in paths:
        with np.load(p) as z:
            this = (int(z["H"]), int(z["W"]), int(z["C"]))
            i, r = z["index"].astype(np.int64).reshape(-1), z["rows"].astype(np.int64)
        if r.shape != (i.size, ROW):
            raise ValueError("%s: rows %s do not fit %d indices" % (os.path.basename(p), r.shape, i.size))
        if size is None:
            size, first = this, p
        elif this != size:
            raise ValueError("differing sizes: %s holds H, W, C = %s, %s holds %s"
                             % (os.path.basename(first), size, os.path.basename(p), this))
        index.append(i)
        rows.append(r)
        owner += [os.path.basename(p)] * i.size
    index, rows = np.concatenate(index), np.concatenate(rows)
    order = np.argsort(index, kind="stable")
    index, rows = index[order], np.ascontiguousarray(rows[order])
    step = np.diff(index)
    if (step == 0).any():
        k = int(np.argmax(step == 0))
        raise ValueError("duplicate index %d (in %s and %s)" % (int(index[k]), owner[order[k]], owner[order[k + 1]]))
    if (step > 1).any():
        k = int(np.argmax(step > 1))
        raise ValueError("gap: no rows for the indices %d..%d" % (int(index[k]) + 1, int(index[k + 1]) - 1))
    return (index, rows) + size


def report(src_dir, num_classes=None, out=None):
    """Merge the shards of ``src_dir``, write pair_stats_summary.json there and print the short form -> the summary."""
    index, rows, H, W, C = merge_shards(src_dir)
    summary = summarise(index, rows, H, W, C, num_classes=num_classes)
    summary["first_index"], summary["last_index"] = int(index[0]), int(index[-1])
    with open(os.path.join(src_dir, SUMMARY_NAME), "w") as f:
        json.dump(summary, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d samples %dx%dx%d, indices %d..%d" % (summary["samples"], H, W, C, index[0], index[-1]), file=out)
    print("class frequency: " + ", ".join("%d: %.6f" % (s, v) for s, v in enumerate(summary["frequency"]) if summary["pixels"][s]),
          file=out)
    print("mean / 255: [%s]  std / 255: [%s]" % (", ".join("%.6f" % v for v in summary["mean_unit"]),
                                               ", ".join("%.6f" % v for v in summary["std_unit"])), file=out)
    print("empty masks: %d" % len(summary["empty_masks"]), file=out)
    return summary


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Merge the pair_stats_*.npz shard files of a generated dataset into one report.")
    ap.add_argument("dir", help="the dataset directory (BASE_DIR/dataset/train_generated)")
    ap.add_argument("--num-classes", type=int, default=None)
    args = ap.parse_args(argv)
    try:
        report(args.dir, num_classes=args.num_classes)
    except ValueError as e:
        print("pair_stats: %s" % e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
