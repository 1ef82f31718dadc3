"""ctypes binding of the on-device decoder score histograms (csrc/gsa_scores.h, csrc/gsa_scores.hip): per
sample and class two 1024-bin histograms of the quantised logit margin ``z_c - max_{j != c} z_j``, one over the pixels labelled with
the class and one over the others -- what ``metrics.ScoreCurves`` reads ROC-AUC, average precision and threshold sweeps from, and
what ``SegSolver.evaluate_scores`` and the config key ``EVAL_SCORES`` report.

``score_histogram`` enqueues the two kernels on the current stream of the logits' device.  Every word is specified by the rule in the
header; a sample's row does not depend on the batch it is in.  No CPU fallback."""
import numpy as np

# csrc/gsa_scores.h
SCORE_BINS = 1024           # bins of one histogram; bin b holds the margins in ((b - 512) / 2^shift, (b - 511) / 2^shift]
SCORE_MAX_SHIFT = 8         # 2^shift bins per logit unit
SCORE_MAX_CLASSES = 8
SCORE_STRETCH = 2048        # pixels a workgroup takes at least
SCORE_MAX_BLOCKS = 128      # workgroups that walk one sample
MIN_CLASSES, MAX_CLASSES = 2, SCORE_MAX_CLASSES
DEFAULT_SHIFT = 5           # 32 bins per logit unit: margins in (-16, 16] between the clamp bins


def check_shift(v, what="shift"):
    """The bin density as an int: 0 .. 8, 2^shift bins per logit unit.  ValueError otherwise."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= SCORE_MAX_SHIFT:
        raise ValueError("%s must be an int in 0..%d, got %r" % (what, SCORE_MAX_SHIFT, v))
    return int(v)


def score_histogram(logits, labels, shift=DEFAULT_SHIFT, out=None):
    """logits (n, K, H, W) or (n, K, HW) contiguous float32 CUDA tensor, K in 2..8; labels: a contiguous int8 tensor of n * HW
    elements on the same device, a pixel being valid iff its label is in 0 .. K - 1; ``shift``: 0..8, 2^shift bins per logit unit;
    ``out``: a contiguous int64 tensor (n, K, 2, SCORE_BINS) on the same device to write into, else one is allocated.
    -> rows (n, K, 2, SCORE_BINS) int64: rows[i, c, 0] the histogram of class c's margin over the valid pixels of sample i NOT
    labelled c, rows[i, c, 1] over those labelled c.  Every word is written.  Two kernels on the current stream of the logits' device;
    ValueError on anything else; no CPU fallback."""
    import torch
    from ._runtime import is_device_tensor, launch
    if not is_device_tensor(logits, torch.float32, dims=(3, 4)):
        raise ValueError("logits must be a contiguous float32 CUDA tensor (n, K, H, W) or (n, K, HW)")
    n, K = int(logits.shape[0]), int(logits.shape[1])
    HW = int(np.prod(logits.shape[2:]))
    dev = logits.device
    if not MIN_CLASSES <= K <= MAX_CLASSES or HW <= 0:
        raise ValueError("logits must hold %d..%d classes and at least one pixel, got shape %s" % (MIN_CLASSES, MAX_CLASSES, tuple(logits.shape)))
    if n * K * HW >= 2 ** 40:
        raise ValueError("logits of %d elements: at most 2^40 - 1" % (n * K * HW))
    if not is_device_tensor(labels, torch.int8, device=dev) or labels.numel() != n * HW:
        raise ValueError("labels must be a contiguous int8 tensor of %d elements on %s" % (n * HW, dev))
    shift = check_shift(shift)
    shape = (n, K, 2, SCORE_BINS)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.int64)
    elif not is_device_tensor(out, torch.int64, shape=shape, device=dev):
        raise ValueError("out must be a contiguous int64 tensor %s on %s" % (shape, dev))
    if n:
        launch("gsa_score_histogram", dev, n, K, HW, shift, logits.data_ptr(), labels.data_ptr(), out.data_ptr())
    return out
