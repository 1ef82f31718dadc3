/*
 * gsa_loss.h -- C ABI of the on-device decoder losses: the softmax cross-entropy of include/gsa_train.h's
 * gsa_train_softmax_ce with per-class and per-pixel (boundary) weights, a focal factor and a choice of normaliser, with its
 * gradient.  The reference's fit carries a per-pixel weight that it never fills (seg_solver.py:402-405); its downstream losses
 * (deeplabv3plus/lib/model/loss.py) normalise by the valid count or by the focal mass.
 *
 * The rule.  Per sample n, pixel i in [0, HW), logits z[n][k][i] (fp32, NCHW as include/gsa_train.h), label y_i (int8):
 *
 *   valid    a pixel is valid iff 0 <= y_i < classes; -1, every other negative label and every label >= classes are ignored (NOT
 *            clamped, as gsa_train_softmax_ce clamps them).
 *   softmax  m = max_k z_k, se = sum_k exp(z_k - m), p_k = exp(z_k - m) / se, CE_i = (m + log se) - z_y.
 *   q_i      = 1 - p_y, formed as sum_{k != y} exp(z_k - m) / se: it keeps its digits where the pixel is confidently right.
 *   weight   w_i = valid_i * class_weight[y_i] * dist_table[idx(dist2_i)]; a null class_weight is all ones, null dist2 and
 *            dist_table are a factor 1.  idx(d) = d for 0 <= d <= 1024 and 1025 otherwise (GSA_BOUNDARY_FAR, negative values).
 *   focal    beta_i = q_i^gamma, gamma = 0 or 1 <= gamma <= 8; gamma = 0 is beta_i = 1 exactly, also at q_i = 0.  b_i = w_i beta_i.
 *   sums     in double, sums[n] = { W = sum w_i, B = sum b_i, S = sum b_i CE_i, T = sum valid_i }.
 *   loss     normalise 0 ("mean"): L_n = S / HW; 1 ("valid"): S / W, 0 when W == 0; 2 ("focal"): S / B, 0 when B == 0.
 *   gradient dlogits[n][k][i] = grad_scale * dL_n / dz[n][k][i].  With e_k = p_k - [k == y] (e_y = -q_i),
 *            h_i = gamma q_i^(gamma - 1) p_y (0 for gamma = 0) and g_i = beta_i + h_i CE_i:
 *            normalise 0, 1: w_i g_i e_k / D, D = HW or W;  normalise 2: w_i (g_i - L_n h_i) e_k / B (the normaliser depends on
 *            the logits and is differentiated through).  Exactly 0 for an ignored pixel and for a sample whose D is 0.
 *
 * Two launches on the stream, no atomics, no memset: every block of the first stores its four partial sums in `workspace`, every
 * block of the second adds its sample's partials in index order.  loss, sums and dlogits of a sample are therefore the same bits
 * from run to run, for every n and at every position in the batch.
 *
 * Conventions as include/gsa_train.h: `stream` is a hipStream_t as void*, calls are stream-ordered and never synchronise, device
 * pointers, 0 on success / negative gsa_status on error.  No CPU fallback.
 *
 * This header lives in csrc/ and its entries in _lib.UNIT_SIGNATURES, not in include/ and _lib.SIGNATURES: see DESIGN.md section 22.
 */
#ifndef GSA_LOSS_H
#define GSA_LOSS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSA_LOSS_TABLE 1026         /* floats of dist_table: dist2 0..1024, then the entry of everything else */
#define GSA_LOSS_MAX_BLOCKS 512     /* workgroups (of 256 pixels a stride) that walk one sample; a power of two */
#define GSA_LOSS_SUMS 4             /* W, B, S, T */

/* Bytes of `workspace` for n samples of HW pixels: n * min(ceil(HW / 256), GSA_LOSS_MAX_BLOCKS) * GSA_LOSS_SUMS doubles.
 * n < 0 or HW <= 0: -1. */
int64_t gsa_loss_workspace_bytes(int32_t n, int32_t HW);

/* logits (n, classes, HW) fp32; labels (n, HW) int8; class_weight `classes` floats or null; dist2 (n, HW) int16 with dist_table
 * GSA_LOSS_TABLE floats, or both null; workspace gsa_loss_workspace_bytes(n, HW) bytes, written by the call; sums (n, GSA_LOSS_SUMS)
 * doubles; loss (n) floats; dlogits as logits, or null: forward only, loss and sums are the same bits and nothing else is written.
 * normalise 0..2 as above.  n = 0 is a successful no-op, decided before anything else.  GSA_ERR_INVALID, decided on the host before
 * any HIP call: n < 0; classes outside 2..64; HW <= 0; a null logits, labels, workspace, sums or loss; dist2 without dist_table or
 * the reverse; gamma not 0 and not in [1, 8], or not finite; normalise outside 0..2; grad_scale not finite; workspace or sums not
 * 8-byte aligned; logits, class_weight, dist_table, loss or dlogits not 4-byte aligned; dist2 not 2-byte aligned;
 * n * classes * HW >= 2^40. */
int gsa_loss_softmax(void* stream, int32_t n, int32_t classes, int32_t HW, const float* logits, const int8_t* labels,
                     const float* class_weight, const int16_t* dist2, const float* dist_table, float gamma, int32_t normalise,
                     float grad_scale, void* workspace, double* sums, float* loss, float* dlogits);

#ifdef __cplusplus
}
#endif
#endif /* GSA_LOSS_H */
