/*
 * gsa_resize.h -- C ABI of the on-device pair resize: a uint8 image batch and / or a uint8 mask batch shrunk to any smaller-or-equal
 * size, the image by the exact area mean, the mask by an area vote or by nearest sampling.  The counterpart of
 * the cv2.resize calls in the reference's dataset loaders, which resize every sample on the host.
 *
 * The rule (canonical, all integers).  Every sample is a plane of its own.
 *
 *   axis weights  One axis has source length L and target length l, 1 <= l <= L.  In a scale where source pixel y covers
 *                 [y * l, (y + 1) * l) and output pixel i covers [i * L, (i + 1) * L), the weight of y in i is the overlap
 *                     a(i, y) = max(0, min((i + 1) * L, (y + 1) * l) - max(i * L, y * l)).
 *                 It is non-zero only for floor(i * L / l) <= y <= floor(((i + 1) * L - 1) / l): at most ceil(L / l) + 1 taps.
 *                 sum over y of a(i, y) = L; sum over i of a(i, y) = l.  Rows use (H, h), columns (W, w), independently: the aspect
 *                 may change, and l == L is the identity on that axis.
 *   image         img (n, H, W, C) u8, C in 1..4.  For every channel c of the output pixel (i, j)
 *                     S   = sum over y, x of a_r(i, y) * a_c(j, x) * img[y][x][c]
 *                     out = (S + (H * W >> 1)) / (H * W)          an integer division: the area mean, rounded half up
 *                 With H * W <= 2^24 the numerator stays below 2^32.
 *   mask, mode 0  "vote".  slot(v) = min(v, 8), the nine slots of include/gsa_stats.h and gsa_compare.h.
 *                     A_s = sum over y, x of a_r(i, y) * a_c(j, x) * [slot(mask[y][x]) == s]
 *                 The output is the slot with the largest A_s, the LOWEST such slot on a tie, and slot 8 is written as 255: every
 *                 input value 8..254 comes out as 255, the ignore label.
 *   mask, mode 1  "nearest".  out[i][j] = mask[floor(i * H / h)][floor(j * W / w)], every value passed through: the index rule of
 *                 cv2.INTER_NEAREST.
 *
 * All sums are integer sums: the order of accumulation cannot change a bit, and a sample does not depend on the batch it is in.
 *
 * Conventions as include/gsa_boundary.h: `stream` is a hipStream_t as void*, calls are stream-ordered and never synchronise, device
 * pointers, 0 on success / negative gsa_status on error.  Stateless: no context, no workspace, no atomics.
 *
 * This header lives in csrc/ and its entry in _lib.UNIT_SIGNATURES, not in include/ and _lib.SIGNATURES: see DESIGN.md section 27.
 */
#ifndef GSA_RESIZE_H
#define GSA_RESIZE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSA_RESIZE_VOTE 0
#define GSA_RESIZE_NEAREST 1
#define GSA_RESIZE_MAX_RATIO 16             /* H <= 16 * h and W <= 16 * w */
#define GSA_RESIZE_MAX_PIXELS 16777216      /* 2^24: H * W of one source plane */

/* img: (n, H, W, C) u8 and img_out: (n, h, w, C) u8, or both null; mask: (n, H, W) u8 and mask_out: (n, h, w) u8, or both null; at
 * least one of the two pairs; all on the device, any alignment; no output may overlap an input or the other output.
 * 1 <= h <= H <= 16 * h and 1 <= w <= W <= 16 * w; H and W each at most 65535 with H * W <= 2^24; C 1..4, also when there is no
 * image; mask_mode GSA_RESIZE_VOTE or GSA_RESIZE_NEAREST, also when there is no mask.  A batch too large for one launch is split,
 * not refused.
 * n = 0 is a successful no-op, decided before anything else.  n < 0, a size, C or mask_mode outside its range, a pair of which one
 * pointer is null, both pairs null, or overlapping ranges: GSA_ERR_INVALID, decided on the host before any HIP call. */
int gsa_pair_resize(void* stream, int32_t n, int32_t H, int32_t W, int32_t C, int32_t h, int32_t w, int32_t mask_mode,
                    const uint8_t* img, const uint8_t* mask, uint8_t* img_out, uint8_t* mask_out);

#ifdef __cplusplus
}
#endif
#endif /* GSA_RESIZE_H */
