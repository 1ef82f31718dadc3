/*
 * gsa_region.h -- C ABI of the on-device region-overlap loss: the soft Tversky index of the decoder's softmax
 * against the labels, per sample and class, with its gradient -- soft Dice and soft Jaccard are two settings of it.  It is the
 * region term that csrc/gsa_loss.h's pixel-wise losses lack: a pixel's gradient depends on per-class sums over the whole sample.
 *
 * The rule.  Per sample n, pixel i in [0, HW), logits z[n][k][i] (fp32, NCHW as include/gsa_train.h), label y_i (int8):
 *
 *   valid    a pixel is valid iff 0 <= y_i < classes; everything else is ignored, NOT clamped (as csrc/gsa_loss.h).
 *   softmax  m = max_k z_k, se = sum_k exp(z_k - m), p_k = exp(z_k - m) / se, all fp32, the sum in class order.
 *   sums     per class k over the valid pixels, in double: I_k = sum [y_i == k] p_k,i;  P_k = sum p_k,i;  G_k = sum [y_i == k], a
 *            count and exact.
 *   index    N_k = I_k + smooth;  D_k = (1 - alpha - beta) I_k + alpha P_k + beta G_k + smooth;  TI_k = N_k / D_k.
 *            alpha = beta = 0.5 is soft Dice, alpha = beta = 1 soft Jaccard; alpha weighs false positives, beta false negatives.
 *   classes  a_k: mode 0 ("present") a_k = 1 iff G_k > 0; mode 1 ("all") a_k = 1 iff D_k > 0; a_k = 0 whenever D_k == 0, and for
 *            every class of a sample without a valid pixel (there `smooth` alone would score every class 1): its A is 0.
 *            D_k > 0 is meant in exact arithmetic, where a softmax is positive: with a valid pixel it holds iff G_k > 0, or, in
 *            mode 1, smooth > 0 or alpha > 0.  The kernel decides it so, from the counts and the parameters; a class whose fp32
 *            p_k underflows to 0 at every pixel stays in the set and scores TI_k = 0.
 *   loss     A = sum_k a_k c_k with c_k = class_weight[k], 1 for a null pointer;  L_n = sum_k a_k c_k (1 - TI_k) / A, and 0 when
 *            A == 0.  In double, rounded once to fp32.
 *   gradient g_k,i = -(a_k c_k / A) (D_k - (1 - beta) N_k) / D_k^2 where y_i == k, and +(a_k c_k / A) alpha N_k / D_k^2 where not;
 *            dL_n / dz_j,i = valid_i p_j,i (g_j,i - sum_k g_k,i p_k,i).  The kernel writes grad_scale * dL_n / dz, formed in double
 *            from the fp32 p and rounded once; with accumulate != 0 it performs one fp32 add instead, dlogits = dlogits + that
 *            value, so that the term rides on the gradient the cross-entropy kernels just wrote.  Exactly 0 for an ignored pixel
 *            and for a sample with A == 0; with accumulate such a pixel keeps its bits.
 *
 * Two launches on the stream, no atomics, no memset: every workgroup of the first walks its strides of 256 pixels and stores its
 * partial I_k, P_k (double) and G_k (int64) in `workspace`; every workgroup of the second adds its sample's partials in index order,
 * forms the 2 * classes coefficients, recomputes the softmax of its pixels and writes or accumulates the gradient, and workgroup 0
 * of a sample stores loss, sums and index.  They are therefore the same bits from run to run, for every n and at every position
 * in the batch, and so is dlogits.
 *
 * Conventions as include/gsa_train.h: `stream` is a hipStream_t as void*, calls are stream-ordered and never synchronise, device
 * pointers, 0 on success / negative gsa_status on error.  No CPU fallback.
 *
 * This header lives in csrc/ and its entries in _lib.UNIT_SIGNATURES, not in include/ and _lib.SIGNATURES: see DESIGN.md section 22.
 */
#ifndef GSA_REGION_H
#define GSA_REGION_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSA_REGION_MAX_CLASSES 16   /* a thread keeps its 3 * classes accumulators in registers */
#define GSA_REGION_MAX_BLOCKS 512   /* workgroups (of 256 pixels a stride) that walk one sample; a power of two */
#define GSA_REGION_SUMS 3           /* I, P, G */

/* Bytes of `workspace` for n samples of `classes` classes and HW pixels:
 * n * min(ceil(HW / 256), GSA_REGION_MAX_BLOCKS) * GSA_REGION_SUMS * classes * 8.  n < 0, classes outside
 * 2..GSA_REGION_MAX_CLASSES or HW <= 0: -1. */
int64_t gsa_region_workspace_bytes(int32_t n, int32_t classes, int32_t HW);

/* logits (n, classes, HW) fp32; labels (n, HW) int8; class_weight `classes` floats or null; workspace
 * gsa_region_workspace_bytes(n, classes, HW) bytes, written by the call; sums (n, GSA_REGION_SUMS, classes) doubles: I, P, G;
 * index (n, classes) floats: TI_k, 0 where a_k == 0; loss (n) floats; dlogits as logits, or null: forward only, loss, sums and
 * index are the same bits and nothing else is written.  mode 0..1 as above.  n = 0 is a successful no-op, decided before anything
 * else.  GSA_ERR_INVALID, decided on the host before any HIP call: n < 0; classes outside 2..GSA_REGION_MAX_CLASSES; HW <= 0; a null
 * logits, labels, workspace, sums, index or loss; alpha, beta or smooth negative or not finite; alpha + beta == 0; mode outside
 * 0..1; grad_scale not finite; workspace or sums not 8-byte aligned; logits, class_weight, index, loss or dlogits not 4-byte
 * aligned; n * classes * HW >= 2^40. */
int gsa_region_tversky(void* stream, int32_t n, int32_t classes, int32_t HW, const float* logits, const int8_t* labels,
                       const float* class_weight, float alpha, float beta, float smooth, int32_t mode, float grad_scale,
                       int32_t accumulate, void* workspace, double* sums, float* index, float* loss, float* dlogits);

#ifdef __cplusplus
}
#endif
#endif /* GSA_REGION_H */
