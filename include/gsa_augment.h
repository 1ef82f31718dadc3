/*
 * gsa_augment.h -- C ABI of the on-device training stream: the (image, mask) pair that the generate entries of
 * include/gsa.h leave in HBM becomes a ready training batch -- warped, cropped, padded, normalised, NCHW -- without
 * leaving the GPU.
 *
 * The reference's consumer does this on host threads for every pair it reads back from disk (its segmentation
 * experiment: HorizontalFlip, ShiftScaleRotate with a constant border, PadIfNeeded, RandomCrop, ToTensor, Normalize;
 * the mask border becomes the ignore label).  Flip, shift, scale, rotation, padding and crop compose into ONE affine
 * map per sample, which the host plans (gan-segmentation_amd/augment.py) and this kernel applies in one pass.
 *
 * The rule (canonical, fp32; every multiply and every add is rounded on its own, nothing is fused):
 *
 *     m = [a b c; d e f] maps the OUTPUT pixel index (X, Y) to continuous SOURCE pixel-index coordinates
 *     (integer k = the centre of source pixel k):
 *
 *     xs = (a*X + b*Y) + c              ys = (d*X + e*Y) + f
 *     x0 = floor(xs), fx = xs - x0      y0 = floor(ys), fy = ys - y0
 *     p_ij = source value at (y0+i, x0+j) as fp32, or 0 where that tap lies outside the image (constant border)
 *     top = p00 + fx*(p01 - p00)        bot = p10 + fx*(p11 - p10)        v = top + fy*(bot - top)
 *     image[n, ch, Y, X] = v*scale[ch] + bias[ch]        (fp32; or bf16 = that fp32 value rounded to nearest even)
 *     label[n, Y, X]     = mask at (floor(ys + 0.5), floor(xs + 0.5)), or `ignore_label` outside the image
 *
 * Inside / outside is decided on the floor values as floats, before any integer conversion: a far-off coordinate
 * cannot wrap.
 *
 * Conventions as include/gsa.h: `stream` is a hipStream_t as void*, calls are stream-ordered and never synchronise,
 * device pointers unless stated, 0 on success / negative gsa_status on error.  Stateless: no context.
 */
#ifndef GSA_AUGMENT_H
#define GSA_AUGMENT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* img (n, H, W, channels) u8 and mask (n, H, W) u8 as the generate entries write them; matrices (n, 6) fp32 on the
 * DEVICE, row = a b c d e f; scale and bias: `channels` floats each on the HOST (read before the call returns).
 * image_out (n, channels, out_h, out_w) fp32, or bf16 when out_bf16 = 1; label_out (n, out_h, out_w) u8.
 * channels 1..4; H, W in [1, 2^24] with H*W*channels < 2^31 (one sample); out_h, out_w multiples of 4 with
 * out_h*out_w < 2^31; ignore_label 0..255; image_out 16-byte aligned (8 in bf16), label_out 4-byte aligned.
 * n = 0 is a successful no-op.  Anything else: GSA_ERR_INVALID. */
int gsa_augment_pairs(void* stream, int32_t n, int32_t H, int32_t W, int32_t channels,
                      const uint8_t* img, const uint8_t* mask, const float* matrices,
                      const float* scale, const float* bias,
                      int32_t out_h, int32_t out_w, int32_t out_bf16, int32_t ignore_label,
                      void* image_out, uint8_t* label_out);

#ifdef __cplusplus
}
#endif
#endif /* GSA_AUGMENT_H */
