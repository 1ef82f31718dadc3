/*
 * gsa_refine.h -- C ABI of the on-device image-guided mask refinement: a joint bilateral vote that pulls the class boundaries of a
 * generated mask onto the edges visible in the image it belongs to.  The reference has nothing like it: its
 * only clean-up is utils.morph_mask, which looks at the mask alone.
 *
 * The rule (canonical, all integers).  Inputs: img (n, H, W, C) u8 with C in 1..4; mask (n, H, W) u8; tables, 377 u8: wr[256], the
 * weight of a colour distance, then ws[11][11] row-major, the weight of an offset, the entry for (dy, dx) at (dy + 5) * 11 + (dx + 5);
 * K = classes in 2..8; R = radius in 1..5.  Every image is a plane of its own.  For the pixel p = (y, x) with v = mask[p]:
 *
 *   frozen     v >= K: out[p] = v.  The ignore label 255 survives a refinement this way.
 *   votes      otherwise, for every q = (y + dy, x + dx) with |dy| <= R and |dx| <= R that lies inside the same plane and has
 *              u = mask[q] < K -- the centre q = p included --
 *                  d = min(255, sum over ch < C of |img[p][ch] - img[q][ch]|)         a SUM over the channels, not a norm
 *                  votes[u] += ws[dy][dx] * wr[d]
 *              A neighbour outside the plane casts no vote, nor does a frozen one, nor the facing row of the next sample.
 *   result     best = max over c < K of votes[c]; out[p] = v if votes[v] == best, else the smallest c with votes[c] == best.
 *
 * Votes stay below 121 * 255 * 255 < 2^23.  All-zero tables give out == mask.  ws entries outside the radius are never read.
 * It is ONE pass: every value is read from the inputs and every output byte has one writer, so no result depends on the order in
 * which the kernel's workgroups arrive.  Several passes are the caller's loop, ping-ponging between two buffers.
 *
 * Conventions as include/gsa_boundary.h: `stream` is a hipStream_t as void*, calls are stream-ordered and never synchronise, device
 * pointers, 0 on success / negative gsa_status on error.  Stateless: no context, no workspace, no atomics.
 *
 * This header lives in csrc/ and its entry in _lib.UNIT_SIGNATURES, not in include/ and _lib.SIGNATURES: see DESIGN.md section 22.
 */
#ifndef GSA_REFINE_H
#define GSA_REFINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* img: (n, H, W, channels) u8; mask, out: (n, H, W) u8; tables: 377 u8; all on the device, any alignment; out must not overlap img,
 * mask or tables.  channels 1..4; classes 2..8; radius 1..5.  H and W each 1..65535 with H * W < 2^31;
 * n * ceil(H/32) * ceil(W/64) < 2^24 (one launch: a larger call is refused, not split).
 * n = 0 is a successful no-op, decided before anything else.  n < 0, a null pointer with n > 0, channels, classes, radius or a size
 * outside its range, or overlapping ranges: GSA_ERR_INVALID, decided on the host before any HIP call. */
int gsa_mask_refine(void* stream, int32_t n, int32_t H, int32_t W, int32_t channels, int32_t classes, int32_t radius,
                    const uint8_t* img, const uint8_t* mask, const uint8_t* tables, uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif /* GSA_REFINE_H */
