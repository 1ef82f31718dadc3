/*
 * gsa_mask.h -- C ABI of the on-device mask clean-up: the per-pixel argmax mask that the generate entries of include/gsa.h
 * leave in HBM loses its isolated flipped pixels and pinholes without leaving the GPU.
 *
 * The reference has this as utils.morph_mask (utils.py:105-109): a 5x5 cv2.MORPH_CLOSE followed by a 5x5 cv2.MORPH_OPEN with
 * cv2's defaults -- all-ones element, centre anchor, one iteration, default border.
 *
 * The rule (canonical, on u8 values):
 *
 *     D(m)[y,x] = max of m[y+dy, x+dx] over |dy| <= 2, |dx| <= 2, taps outside the image skipped
 *     E(m)[y,x] = min of the same taps, taps outside the image skipped
 *     morph(m)  = D(E(E(D(m))))             close = E after D, then open = D after E
 *
 * "Skipped": the outside of the image acts as 0 for a dilation and as 255 for an erosion, at every stage, on that stage's own
 * input; a constant mask stays what it is.  Every image of a batch is a plane of its own: no tap reads a neighbouring image.
 * On more than two classes this is grey-level morphology on the class index, as the reference's function would do.
 *
 * Conventions as include/gsa.h: `stream` is a hipStream_t as void*, calls are stream-ordered and never synchronise,
 * device pointers, 0 on success / negative gsa_status on error.  Stateless: no context, no workspace.
 */
#ifndef GSA_MASK_H
#define GSA_MASK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mask and out: (n, H, W) u8 on the device, any alignment; out must not overlap mask.  H and W each 1..65535 (any size, not only
 * the generate entries' multiples of 16), n * ceil(H/64) * ceil(W/64) < 2^24 (one launch).  n = 0 is a successful no-op.
 * A null pointer with n > 0, a size outside the range or overlapping ranges: GSA_ERR_INVALID. */
int gsa_mask_morph(void* stream, int32_t n, int32_t H, int32_t W, const uint8_t* mask, uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif /* GSA_MASK_H */
