/*
 * gsa_boundary.h -- C ABI of the on-device mask boundary distance and ignore band: for a class-index mask that already lies in
 * HBM, every pixel's squared Euclidean distance to the nearest pixel of another value, up to a radius, and the mask with a band
 * of an ignore label around every class boundary.  The reference has no kernel for it; its dataset readers
 * map a stored 255 to -1, as VOC's void border asks, and that is the value the band is meant to write.
 *
 * The rule (canonical, all integers).  Input: mask (n, H, W) u8; every image is a plane of its own.  R = radius, 1..32.
 *
 *   D(p)     = min over pixels q of the SAME plane with mask[q] != mask[p] (raw u8 values) of (qy-py)^2 + (qx-px)^2;
 *              no such q: infinite.  The outside of the image is not "another value": an image edge makes no boundary.
 *   dist2[p] = (int16) D(p) if D(p) <= R*R, else GSA_BOUNDARY_FAR = 32767
 *   out[p]   = (u8) label if D(p) <= R*R, else mask[p]              label in 0..255
 *
 * The rule is symmetric: both sides of a boundary get the band, and R*R is inclusive.  It is ONE pass: values are read from the
 * input, out never feeds back, and a pixel whose input value already equals label is a value like any other.  Every u8 value is a
 * legal mask value, 255 included.
 *
 * The rule separates exactly, for any number of classes.  With h[y,x] the vertical distance from (y,x) to the nearest pixel of
 * column x whose value differs from mask[y,x] (anything beyond R counts as infinite):
 *
 *   D(y,x) = min over |dx| <= R, x+dx inside the image, of  dx^2 + ( mask[y,x+dx] != mask[y,x] ? 0 : h[y,x+dx]^2 )
 *
 * (if mask[y,x+dx] equals mask[y,x], the nearest other value of that column is h away; if it differs, it is the other value.)
 * Every quantity is an integer minimum: no result depends on the order in which the kernel's workgroups arrive.
 *
 * Conventions as include/gsa_mask.h: `stream` is a hipStream_t as void*, calls are stream-ordered and never synchronise, device
 * pointers, 0 on success / negative gsa_status on error.  Stateless: no context, no workspace, one launch.
 */
#ifndef GSA_BOUNDARY_H
#define GSA_BOUNDARY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSA_BOUNDARY_FAR 32767
#define GSA_BOUNDARY_MAX_RADIUS 32

/* mask: (n, H, W) u8, any alignment.  dist2: (n, H, W) int16, 2-byte aligned, or null.  out: (n, H, W) u8 or null.  At least one of
 * the two; neither may overlap mask, nor each other.  When dist2 is null nothing is written for it, and so for out.  radius 1..32;
 * label 0..255 (checked even when out is null).  H and W each 1..65535 with H * W < 2^31, n * ceil(H/64) * ceil(W/64) < 2^24 (one
 * launch).  n = 0 is a successful no-op.  n < 0, a size, radius or label outside its range, a null mask or two null outputs with
 * n > 0, an odd dist2 address or overlapping ranges: GSA_ERR_INVALID, decided on the host before any HIP call. */
int gsa_mask_boundary(void* stream, int32_t n, int32_t H, int32_t W, int32_t radius, int32_t label,
                      const uint8_t* mask, int16_t* dist2, uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif /* GSA_BOUNDARY_H */
