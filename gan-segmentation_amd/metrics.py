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
