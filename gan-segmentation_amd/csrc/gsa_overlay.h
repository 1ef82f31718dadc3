/*
 * gsa_overlay.h -- C ABI of the on-device pair previews: the class-index mask of a generated pair laid over its image in the class
 * colours, the class outlines, a thumbnail of it and a contact sheet of a batch, without leaving the GPU.
 *
 * The reference has the overlay as utils.get_draw_mask (utils.py:69-102): a float blend of the image with one colour per class,
 * background skipped, which its annotator shows after every epoch and saves as vis_img_%06d.jpg beside every sample.  For
 * alpha = k/128 the blend below is that function bit for bit.  Outlines, thumbnails and sheets are ours.
 *
 * The rule (canonical, all integers).  Inputs: img (n, H, W, C) u8 with C in 1..4; mask (n, H, W) u8; lut (256, 6) u8, row v =
 * c0 c1 c2 c3 w_in w_edge.  Every image is a plane of its own.
 *
 *   edge(p)    p is an edge pixel iff one of its 4-neighbours q inside the same plane has mask[q] != mask[p] (raw u8 values):
 *              D(p) == 1 of include/gsa_boundary.h.  The image border makes no edge, and the last row of one sample and the first
 *              row of the next are not neighbours.
 *   w(p)       min(w_edge, 128) of row mask[p] if edge(p), else min(w_in, 128) of that row
 *   b[p][ch]   (w * c_ch + (128 - w) * img[p][ch]) >> 7 for ch < C, c_ch of row mask[p]
 *              w = 0 leaves the pixel untouched, w = 128 gives the solid colour, w = 64 gives (c + p) >> 1
 *   t[Y][X][ch] = (sum of b over the f x f block at (f*Y, f*X) + f*f/2) >> (2 * log2 f)       f = factor, h = H/f, w = W/f
 *   out        (rows*h, cols*w, C) u8 with rows = ceil(n / cols): sample i fills the cell at row i / cols, column i % cols; cells
 *              with no sample are 0.  The call writes every byte of out.
 *
 * With cols = 1 the sheet is exactly the (n, h, w, C) batch of thumbnails; with factor = 1 as well, the batch of overlays.  It is
 * ONE pass: every value is read from the inputs, and every output byte has one writer, so no result depends on the order in which
 * the kernel's workgroups arrive.
 *
 * Conventions as include/gsa_mask.h: `stream` is a hipStream_t as void*, calls are stream-ordered and never synchronise, device
 * pointers, 0 on success / negative gsa_status on error.  Stateless: no context, no workspace.
 *
 * This header lives in csrc/ and its entry in _lib.EXTRA_SIGNATURES, not in include/ and _lib.SIGNATURES: see DESIGN.md section 21.
 */
#ifndef GSA_OVERLAY_H
#define GSA_OVERLAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* img: (n, H, W, channels) u8; mask: (n, H, W) u8; lut: (256, 6) u8; out: (ceil(n/cols) * H/factor, cols * W/factor, channels) u8;
 * all on the device, any alignment; out must not overlap img, mask or lut.  channels 1..4; factor 1, 2, 4, 8 or 16, H and W
 * multiples of it; cols >= 1.  H and W each 1..65535 with H * W < 2^31; out holds fewer than 2^31 bytes;
 * n * ceil(H/32) * ceil(W/128) < 2^24 (one launch; the cells without a sample are cleared by a second one under the same limit).
 * n = 0 is a successful no-op, decided before anything else.  n < 0, a null pointer with n > 0, channels, factor, cols or a size
 * outside its range, or overlapping ranges: GSA_ERR_INVALID, decided on the host before any HIP call. */
int gsa_overlay(void* stream, int32_t n, int32_t H, int32_t W, int32_t channels, const uint8_t* img, const uint8_t* mask,
                const uint8_t* lut, int32_t factor, int32_t cols, uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif /* GSA_OVERLAY_H */
