/*
 * gsa_compare.h -- C ABI of the on-device mask agreement: how two uint8 masks of one shape agree, as a banded confusion table per
 * sample.  What boundary IoU, trimap accuracy and a plain confusion matrix of two masks are read from.  The
 * reference scores only the decoder's argmax against an annotation (its SegmentationMetric); it has nothing for two masks.
 *
 * The rule (canonical, all integers).  Inputs: target and pred (n, H, W) u8; radius R; with R > 0 the planes target_dist2 and
 * pred_dist2 (n, H, W) int16, as gsa_mask_boundary (include/gsa_boundary.h) writes them for target and for pred -- the entry reads
 * them as numbers and nothing else.  Every image is a plane of its own.  For the pixel p of sample i:
 *
 *   slot       slot(v) = min(v, 8): the nine slots of include/gsa_stats.h, the values 0..7 each and everything from 8 up
 *              together, 255 included.
 *   band code  f = (target_dist2[p] <= R*R) + 2 * (pred_dist2[p] <= R*R); without dist2 planes (R = 0) f = 0.
 *   row        rows[i][f * 81 + slot(target[p]) * 9 + slot(pred[p])] counts the pixel.
 *
 * The GSA_COMPARE_ROW = 324 bins of a row are disjoint and sum to H * W.  Every word of every row is overwritten; nothing
 * accumulates across calls.  Integer sums: the order in which the kernel's workgroups arrive cannot change a bit.
 *
 * Conventions as include/gsa_boundary.h: `stream` is a hipStream_t as void*, calls are stream-ordered and never synchronise, device
 * pointers, 0 on success / negative gsa_status on error.  Stateless: no context, no workspace.
 *
 * This header lives in csrc/ and its entry in _lib.UNIT_SIGNATURES, not in include/ and _lib.SIGNATURES: see DESIGN.md section 23.
 */
#ifndef GSA_COMPARE_H
#define GSA_COMPARE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSA_COMPARE_SLOTS 9
#define GSA_COMPARE_BANDS 4
#define GSA_COMPARE_ROW 324         /* GSA_COMPARE_BANDS * GSA_COMPARE_SLOTS * GSA_COMPARE_SLOTS int64 words per sample */
#define GSA_COMPARE_MAX_RADIUS 32

/* target, pred: (n, H, W) u8, any alignment; target_dist2, pred_dist2: (n, H, W) int16, 2-byte aligned, or both null; rows:
 * (n, GSA_COMPARE_ROW) int64, 8-byte aligned, overlapping no input; all on the device.  radius 0 goes with both dist2 pointers null,
 * radius 1..32 with both non-null.  H and W each 1..65535 with H * W < 2^31; a batch too large for one launch is split, not refused.
 * n = 0 is a successful no-op, decided before anything else.  n < 0, a size or radius outside its range, a radius that does not go
 * with the dist2 pointers, a null target, pred or rows, an odd dist2 address, a rows address that is no multiple of 8, or rows
 * overlapping an input: GSA_ERR_INVALID, decided on the host before any HIP call. */
int gsa_mask_compare(void* stream, int32_t n, int32_t H, int32_t W, int32_t radius, const uint8_t* target, const uint8_t* pred,
                     const int16_t* target_dist2, const int16_t* pred_dist2, int64_t* rows);

#ifdef __cplusplus
}
#endif
#endif /* GSA_COMPARE_H */
