/*
 * gsa_jpeg_roundtrip.h -- C ABI of the on-device JPEG round trip of the training stream.
 *
 * `main.py generate` stores every image as a quality-95 4:2:0 baseline JPEG (include/gsa_jpeg.h), so a consumer of the files
 * only ever sees pixels that went through that codec.  This entry turns an image in HBM into exactly the pixels a reader of
 * its file would decode -- without writing the file: the encoder's arithmetic up to the quantised coefficients (the very
 * code of gsa_jpeg_encode), then libjpeg's decoder arithmetic, integer for integer: dequantisation, the "islow" inverse DCT
 * (jidctint: column pass first, CONST_BITS 13, PASS1_BITS 2), h2v2 "fancy" (triangle) chroma upsampling with the rows and
 * columns replicated at the edges of each image, YCbCr -> RGB in 16-bit fixed point.  Entropy coding is lossless and restart
 * markers do not change the pixels, so neither takes part.  tests/test_jpeg_roundtrip_host.py states the rule in numpy and
 * pins it, with zero differing bytes, against libjpeg-turbo (through Pillow) at quality 85, 95 and 100.
 *
 * Range limiting: both places libjpeg range-limits (the IDCT's output + 128, and R, G, B) are clamps to 0..255 here.
 * libjpeg's C code uses a masked table that equals a clamp for IDCT outputs in -384..639 and wraps outside.  A pixel's
 * quantisation error is at most (sum of the table's 64 steps) / 8, which keeps every value inside that band for quality >= 82:
 * there the clamp provably equals libjpeg.  Below 82 it equals the saturating SIMD decoders (libjpeg-turbo on x86-64 matched at
 * quality 50 and 10 on every input tried); a scalar C libjpeg could differ there on extreme inputs.
 *
 * Conventions as include/gsa.h: `stream` is a hipStream_t as void*, calls are stream-ordered and never synchronise,
 * device pointers, 0 on success / negative gsa_status on error (checked on the host before any launch).  Stateless: no context.
 */
#ifndef GSA_JPEG_ROUNDTRIP_H
#define GSA_JPEG_ROUNDTRIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device workspace gsa_jpeg_roundtrip needs for n images: the decoded Y plane at full size and the decoded Cb and Cr
 * planes at half size, 1.5 bytes per pixel.  n >= 0 (0 for n = 0); H and W multiples of 16 in 16..65535.  Negative otherwise. */
int64_t gsa_jpeg_roundtrip_workspace_bytes(int32_t n, int32_t H, int32_t W);

/* out (n,H,W,3) u8 = the pixels a libjpeg decoder returns for the quality-`quality` 4:2:0 file of rgb (n,H,W,3) u8, every
 * image on its own.  H and W multiples of 16 in 16..65535; quality 1..100 (the encoder's range); rgb, workspace and out 16-byte
 * aligned; out must not be rgb.  n = 0 returns 0 without a launch. */
int gsa_jpeg_roundtrip(void* stream, int32_t n, int32_t H, int32_t W, const uint8_t* rgb, int32_t quality, void* workspace,
                       int64_t workspace_bytes, uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif /* GSA_JPEG_ROUNDTRIP_H */
