/*
 * gsa_scores.h -- C ABI of the on-device decoder score histograms: per sample and class, two fixed-size
 * histograms of the quantised logit margin, one over the pixels labelled with the class and one over the rest, made in one pass
 * over the logits.  ROC-AUC, average precision and every threshold sweep of metrics.ScoreCurves are read from them -- what the
 * reference's SegmentationMetricDetailed.compute_auc reads from every pixel's score kept on the host.
 *
 * The rule.  Per sample i, pixel p in [0, HW), logits z[i][k][p] (fp32, NCHW as gsa_loss.h), label y_p (int8):
 *
 *   valid    a pixel is valid iff 0 <= y_p < classes, as in gsa_loss.h: -1, every other negative label and every label >= classes
 *            are ignored, NOT clamped.  An ignored pixel is counted nowhere.
 *   margin   for every class c of a valid pixel, m_c = z_c - max_{j != c} z_j: one fp32 subtraction, round to nearest, never
 *            contracted.  The maximum is the largest of the other logits and is NaN when one of them is NaN, so ONE NaN logit makes
 *            every margin of its pixel NaN.  Two equal maxima give both classes the margin 0; every margin is <= 0 but the strict
 *            winner's.
 *   bin      b = clamp(ceil(m_c * 2^shift) + 511, 0, GSA_SCORE_BINS - 1), shift in 0..GSA_SCORE_MAX_SHIFT.  The scaling by a power
 *            of two is exact, so bin b holds the margins in the half-open interval ((b - 512) / 2^shift, (b - 511) / 2^shift] and
 *            b >= 512 <=> m_c > 0: the strict winner.  +inf and a product that overflows go to bin 1023, -inf to bin 0, and a NaN
 *            margin (a NaN logit, inf - inf) to bin 0.  A subnormal positive margin is NOT flushed: it lands in bin 512 (the
 *            library is built with fp32 denormals on, hipcc's default for gfx950: FLOAT_DENORM_MODE_32 = 3 in the kernel
 *            descriptors).
 *   count    rows[i][c][y_p == c][b] += 1.  For every c the 2 * GSA_SCORE_BINS words of a sample sum to its number of valid pixels.
 *
 * The score is the margin, not the softmax probability: it needs no expf, so every word is specified to the bit.  For two classes
 * p_1 = sigmoid(m_1) is monotone in the margin: ROC, AP and every threshold on the probability are those on the margin, up to the
 * binning (<= 1/128 in probability at shift 5).  For MORE than two classes the one-vs-rest margin z_c - max_{j != c} z_j is a
 * different score from the softmax probability p_c -- it orders pixels differently -- and curves read from these rows are curves
 * of the margin.
 *
 * Every word of rows is overwritten: nothing accumulates across calls.  Two launches on the stream (zero, count); integer sums,
 * so no order of arrival changes a bit, and a sample's row does not depend on the batch it is in.
 *
 * Conventions as gsa_loss.h: `stream` is a hipStream_t as void*, calls are stream-ordered and never synchronise, device pointers,
 * 0 on success / negative gsa_status on error.  No context, no workspace, no CPU fallback.
 *
 * This header lives in csrc/ and its entry in _lib.UNIT_SIGNATURES, not in include/ and _lib.SIGNATURES: see DESIGN.md section 22.
 */
#ifndef GSA_SCORES_H
#define GSA_SCORES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSA_SCORE_BINS 1024         /* bins of one histogram; bin 512 is the first of the positive margins */
#define GSA_SCORE_MAX_SHIFT 8       /* 2^shift bins per logit unit, shift 0..8 */
#define GSA_SCORE_MAX_CLASSES 8     /* the decoder's range, 2..8 */
#define GSA_SCORE_STRETCH 2048      /* pixels a workgroup takes at least (fewer only when the sample has fewer) */
#define GSA_SCORE_MAX_BLOCKS 128    /* workgroups that walk one sample; beyond STRETCH * MAX_BLOCKS pixels they stride */

/* logits (n, classes, HW) fp32; labels (n, HW) int8; rows (n, classes, 2, GSA_SCORE_BINS) int64, every word written.
 * n = 0 is a successful no-op, decided before anything else.  GSA_ERR_INVALID, decided on the host before any HIP call: n < 0;
 * classes outside 2..GSA_SCORE_MAX_CLASSES; HW <= 0; shift outside 0..GSA_SCORE_MAX_SHIFT; a null logits, labels or rows; logits not
 * 4-byte aligned; rows not 8-byte aligned; rows overlapping logits or labels; n * classes * HW >= 2^40. */
int gsa_score_histogram(void* stream, int32_t n, int32_t classes, int32_t HW, int32_t shift, const float* logits,
                        const int8_t* labels, int64_t* rows);

#ifdef __cplusplus
}
#endif
#endif /* GSA_SCORES_H */
