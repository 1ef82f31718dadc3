"""pixAcc / mIoU bookkeeping of the reference's ``SegmentationMetric`` (metrics.py:497-606) on top of a
confusion matrix (``gsa_segmentation_eval`` produces it on the device).

confusion[l, p] = number of pixels with label l >= 0 (ignored pixels never counted) and predicted class p.
The reference's quantities follow exactly: ``batch_pix_accuracy`` -> correct = trace, labelled = sum;
``batch_intersection_union`` -> inter = diagonal, area_pred = column sums (its ``predict`` is zeroed where the
target is ignored), area_lab = row sums, union = pred + lab - inter.
"""
import numpy as np


class SegmentationMetric:
    def __init__(self, nclass, skip_bg=True):
        self.nclass = nclass
        self._skip_bg = skip_bg
        self.reset()

    def reset(self):
        self.total_inter = np.zeros(self.nclass, np.int64)
        self.total_union = np.zeros(self.nclass, np.int64)
        self.total_correct = 0
        self.total_label = 0

    def update_confusion(self, confusion):
        c = np.asarray(confusion).astype(np.int64).reshape(self.nclass, self.nclass)
        inter = np.diag(c)
        self.total_inter += inter
        self.total_union += c.sum(axis=0) + c.sum(axis=1) - inter
        self.total_correct += int(inter.sum())
        self.total_label += int(c.sum())

    def get(self):
        """-> (['accuracy', 'mean-iou'], [pixAcc, mIoU]), the reference's formulas (metrics.py:541-561)."""
        pixAcc = 1.0 * self.total_correct / (np.spacing(1) + self.total_label)
        IoU = 1.0 * self.total_inter / (np.spacing(1) + self.total_union)
        IoU = IoU[self.total_union > 0]
        if self._skip_bg:
            IoU = IoU[1:]      # reference: skip background class (after dropping empty classes, as it does)
        mIoU = IoU.mean() if IoU.size else float("nan")
        return ["accuracy", "mean-iou"], [pixAcc, mIoU]

    def get_name_value(self):
        names, values = self.get()
        return list(zip(names, values))


class MaskAgreement:
    """How two masks agree, from the banded confusion rows of ``mask_ops.compare(pred, target, band)`` (csrc/gsa_compare.h; DESIGN.md
    section 23): ``rows.reshape(-1, 4, 9, 9)`` is [band code f, target slot, prediction slot], f = (in the target's band) + 2 * (in the
    prediction's band).  Target values >= ``nclass`` are ignored pixels, predictions >= ``nclass`` are abstained -- what an ignore band
    writes.  With T[f] the ``nclass x nclass`` corner of table f:

      accuracy, mean-iou   ``SegmentationMetric`` on T[0] + T[1] + T[2] + T[3], its formulas to the letter -- the ``np.spacing(1)``,
                           the empty-class drop, the background skip -- so a chain without an ignore band gives ``evaluate``'s numbers
                           to the bit.  Abstained pixels are in neither numerator nor denominator.
      band-accuracy        trace / sum of T[1] + T[3]: the accuracy among the pixels within ``band`` px of a class boundary of the
                           target -- the trimap accuracy.  NaN when that band holds no counted pixel (``band = 0``).
      boundary-iou         per class k: inter = T[3][k][k]; gt = sum over p of (T[1] + T[3])[k][p]; pred = sum over t of
                           (T[2] + T[3])[t][k]; union = gt + pred - inter; the mean of inter / union over the classes with union > 0,
                           the first of them skipped with ``skip_bg`` as mean-iou does.  NaN when no class is left.  It differs
                           from the Boundary IoU of Cheng et al. (CVPR 2021) in two ways: the band is Euclidean, class k's pixels
                           within ``band`` px of a pixel of another value (theirs comes from repeated 3x3 erosions, a chessboard
                           distance, with d a share of the image diagonal), and an image edge makes no boundary (theirs pads the mask
                           with background first, so the image border is contour).
      abstained            labelled pixels (target < nclass) whose prediction is >= nclass, over the labelled pixels; NaN without any.
    """
    NAMES = ["accuracy", "mean-iou", "band-accuracy", "boundary-iou", "abstained"]
    ROW, BANDS, SLOTS = 324, 4, 9

    def __init__(self, nclass, skip_bg=True):
        if isinstance(nclass, bool) or not isinstance(nclass, (int, np.integer)) or not 1 <= int(nclass) <= self.SLOTS - 1:
            raise ValueError("nclass must be an int in 1..8 (the values from 8 up share a slot), got %r" % (nclass,))
        self.nclass = int(nclass)
        self._skip_bg = skip_bg
        self.reset()

    def reset(self):
        self.tables = np.zeros((self.BANDS, self.SLOTS, self.SLOTS), np.int64)

    def update_rows(self, rows):
        """Add rows of ``mask_ops.compare``: any array whose last axis has 324 words; the leading axes are summed."""
        r = np.asarray(rows)
        if r.ndim < 1 or r.shape[-1] != self.ROW or r.dtype.kind not in "iu":
            raise ValueError("rows must be an integer array (..., %d), got %s %s" % (self.ROW, r.dtype, r.shape))
        self.tables += r.astype(np.int64).reshape(-1, self.BANDS, self.SLOTS, self.SLOTS).sum(axis=0)

    def get(self):
        """-> (NAMES, [accuracy, mIoU, band accuracy, boundary IoU, abstained share])."""
        k = self.nclass
        T = self.tables[:, :k, :k]
        whole = SegmentationMetric(k, skip_bg=self._skip_bg)
        whole.update_confusion(T.sum(axis=0))
        _names, (pixAcc, mIoU) = whole.get()
        band = T[1] + T[3]
        band_acc = float(np.trace(band)) / float(band.sum()) if band.sum() else float("nan")
        inter = np.diag(T[3])
        union = band.sum(axis=1) + (T[2] + T[3]).sum(axis=0) - inter
        keep = union > 0
        biou = inter[keep] / union[keep]
        if self._skip_bg:
            biou = biou[1:]
        labelled = self.tables[:, :k, :].sum()
        abstained = float(self.tables[:, :k, k:].sum()) / float(labelled) if labelled else float("nan")
        return list(self.NAMES), [pixAcc, mIoU, band_acc, biou.mean() if biou.size else float("nan"), abstained]

    def get_name_value(self):
        names, values = self.get()
        return list(zip(names, values))


class ScoreCurves:
    """How well the decoder's logits separate each class, from the score histograms of ``score_ops.score_histogram`` (csrc/gsa_scores.h;
    DESIGN.md section 25): ``rows.reshape(-1, nclass, 2, 1024)`` is [class c, pixel labelled c or not, bin of the margin
    ``z_c - max_{j != c} z_j``].  With ``P[b]`` and ``N[b]`` the pixels of class c and the other valid pixels in bin b, and "positive at
    threshold t" meaning bin >= t, that is margin > ``(t - 512) / 2^shift``:

      roc_auc(c)            sum_b P[b] (N_below[b] + N[b] / 2) / (P N): Mann-Whitney with a tie inside a bin counted half, sklearn's
                            ``roc_auc_score`` on the quantised scores (what the reference's ``compute_auc`` calls on every pixel's
                            score).  The numerator is a Python integer; the one division is the only float.
      average_precision(c)  sum_t (R_t - R_{t-1}) Prec_t over the occupied bins in descending order, sklearn's
                            ``average_precision_score`` on the quantised scores: every term P[b] TP_t / (TP_t + FP_t) is one
                            correctly rounded quotient of integers, the terms are added by ``math.fsum`` and divided by P.
      sweep(c)              TP, FP and FN (int64, 1025 entries) at every threshold t = 0 .. 1024.
      at(c, margin)         precision, recall, iou and dice at the bin edge nearest to ``margin``; ``at(c, 0)`` is the strict winner,
                            for two classes the argmax mask of class 1.
      best(c, metric)       the threshold with the best iou or dice, the lowest on ties (compared as integer fractions).
      clamped(c)            the share of valid pixels in the clamp bins 0 and 1023: where it is large, ``shift`` is too fine for
                            the decoder's margins and the curves are coarse.

    A class without positives or without negatives has NaN for AUC and AP and is left out of the means.  For ``nclass > 2`` the margin
    is a different score from the softmax probability; for two classes ``sigmoid(margin)`` is class 1's probability."""
    BINS = 1024
    ZERO = 512          # the first bin of the positive margins
    METRICS = ("iou", "dice")

    def __init__(self, nclass, shift=5, skip_bg=True):
        if isinstance(nclass, bool) or not isinstance(nclass, (int, np.integer)) or not 2 <= int(nclass) <= 8:
            raise ValueError("nclass must be an int in 2..8, got %r" % (nclass,))
        if isinstance(shift, bool) or not isinstance(shift, (int, np.integer)) or not 0 <= int(shift) <= 8:
            raise ValueError("shift must be an int in 0..8, got %r" % (shift,))
        self.nclass = int(nclass)
        self.shift = int(shift)
        self._skip_bg = skip_bg
        self.reset()

    def reset(self):
        self.hist = np.zeros((self.nclass, 2, self.BINS), np.int64)

    def update_rows(self, rows):
        """Add rows of ``score_ops.score_histogram``: any integer array (..., nclass, 2, 1024); the leading axes are summed."""
        r = np.asarray(rows)
        if r.ndim < 3 or tuple(r.shape[-3:]) != self.hist.shape or r.dtype.kind not in "iu":
            raise ValueError("rows must be an integer array (..., %d, 2, %d), got %s %s" % (self.nclass, self.BINS, r.dtype, r.shape))
        self.hist += r.astype(np.int64).reshape((-1,) + self.hist.shape).sum(axis=0)

    def _class(self, c):
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) < self.nclass:
            raise ValueError("class must be an int in 0..%d, got %r" % (self.nclass - 1, c))
        return [int(v) for v in self.hist[int(c), 0]], [int(v) for v in self.hist[int(c), 1]]     # Python integers: no overflow

    def margin_of(self, t):
        """The margin a threshold t = 0 .. 1024 stands for: positive iff margin > (t - 512) / 2^shift."""
        return (int(t) - self.ZERO) / 2.0 ** self.shift

    def roc_auc(self, c):
        N, P = self._class(c)
        p, n = sum(P), sum(N)
        if not p or not n:
            return float("nan")
        twice, below = 0, 0
        for b in range(self.BINS):
            twice += P[b] * (2 * below + N[b])
            below += N[b]
        return twice / (2 * p * n)

    def average_precision(self, c):
        import math
        N, P = self._class(c)
        p, n = sum(P), sum(N)
        if not p or not n:
            return float("nan")
        tp = fp = 0
        terms = []
        for b in range(self.BINS - 1, -1, -1):
            if not P[b] and not N[b]:
                continue
            tp += P[b]
            fp += N[b]
            terms.append(P[b] * tp / (tp + fp))
        return math.fsum(terms) / p

    def sweep(self, c):
        """-> (TP, FP, FN), int64 arrays of 1025 entries: entry t counts with "positive iff bin >= t" (t = 1024: nothing is)."""
        self._class(c)
        N, P = self.hist[int(c), 0], self.hist[int(c), 1]
        zero = np.zeros(1, np.int64)
        tp = np.concatenate([np.cumsum(P[::-1])[::-1], zero])
        fp = np.concatenate([np.cumsum(N[::-1])[::-1], zero])
        return tp, fp, tp[0] - tp

    @staticmethod
    def _ratio(a, b):
        return a / b if b else float("nan")

    def _at(self, c, t):
        tp, fp, fn = (int(v[t]) for v in self.sweep(c))
        return {"threshold": t, "margin": self.margin_of(t), "tp": tp, "fp": fp, "fn": fn,
                "precision": self._ratio(tp, tp + fp), "recall": self._ratio(tp, tp + fn),
                "iou": self._ratio(tp, tp + fp + fn), "dice": self._ratio(2 * tp, 2 * tp + fp + fn)}

    def at(self, c, margin):
        """Counts and precision, recall, iou, dice of class c with "positive iff margin > m", m the bin edge nearest to ``margin``
        (the upper one half way, clamped to the histogram); the edge taken is returned as ``margin``.  NaN where a denominator is 0."""
        x = float(margin) * 2.0 ** self.shift
        if x != x:
            raise ValueError("margin must be a number, got %r" % (margin,))
        t = int(min(max(np.floor(x + 0.5), -self.ZERO), self.BINS - self.ZERO)) + self.ZERO
        return self._at(c, t)

    def best(self, c, metric="iou"):
        """The threshold t = 0 .. 1024 at which ``metric`` ("iou" or "dice") of class c is largest, the lowest on ties, as ``_at`` gives
        it; for two classes also ``probability`` = sigmoid(margin).  ``threshold`` None and NaN values for a class without positives."""
        if metric not in self.METRICS:
            raise ValueError("metric must be one of %s, got %r" % (", ".join(self.METRICS), metric))
        tp, fp, fn = self.sweep(c)
        best_t, num, den = None, 0, 1
        for t in range(self.BINS + 1 if int(tp[0]) else 0):         # with a positive pixel every denominator is at least tp + fn > 0
            a, f = int(tp[t]), int(fp[t]) + int(fn[t])
            a, d = (a, a + f) if metric == "iou" else (2 * a, 2 * a + f)
            if best_t is None or a * den > num * d:
                best_t, num, den = t, a, d
        if best_t is None:
            nan = float("nan")
            return {"threshold": None, "margin": nan, metric: nan, "probability": nan} if self.nclass == 2 else \
                {"threshold": None, "margin": nan, metric: nan}
        out = self._at(c, best_t)
        if self.nclass == 2:
            out["probability"] = 1.0 / (1.0 + float(np.exp(-out["margin"])))
        return out

    def clamped(self, c):
        N, P = self._class(c)
        return self._ratio(N[0] + P[0] + N[-1] + P[-1], sum(N) + sum(P))

    def get(self):
        """-> (names, values): mean-auc and mean-ap over the classes that have both (the first class skipped with ``skip_bg``, NaN when
        none is left), the reference's 100*(1-mean-auc) and 100*(1-mean-ap), then per class k (background skipped alike)
        ``k-best-margin``, ``k-iou@best`` and ``k-iou@0``, and ``clamped``, the largest clamped share among those classes."""
        classes = list(range(1 if self._skip_bg else 0, self.nclass))
        auc = [v for v in (self.roc_auc(c) for c in classes) if v == v]
        ap = [v for v in (self.average_precision(c) for c in classes) if v == v]
        mean_auc = float(np.mean(auc)) if auc else float("nan")
        mean_ap = float(np.mean(ap)) if ap else float("nan")
        names = ["mean-auc", "mean-ap", "100*(1-mean-auc)", "100*(1-mean-ap)"]
        values = [mean_auc, mean_ap, 100 * (1 - mean_auc), 100 * (1 - mean_ap)]
        for c in classes:
            b = self.best(c, "iou")
            names += ["%d-best-margin" % c, "%d-iou@best" % c, "%d-iou@0" % c]
            values += [b["margin"], b["iou"], self.at(c, 0.0)["iou"]]
        share = [v for v in (self.clamped(c) for c in classes) if v == v]
        names.append("clamped")
        values.append(max(share) if share else float("nan"))
        return names, values

    def get_name_value(self):
        names, values = self.get()
        return list(zip(names, values))
