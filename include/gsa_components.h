/*
 * gsa_components.h -- C ABI of the on-device mask components: connected-component labels and areas of a class-index mask that
 * already lies in HBM, a clean-up that removes components below an area threshold, and per-sample component counts (DESIGN.md
 * section 17).  The reference has no counterpart: its utils.morph_mask (include/gsa_mask.h) removes what fits inside a 5x5 window
 * and nothing larger.
 *
 * The rule (canonical, all integers).  Input: mask (n, H, W) u8; every image is a plane of its own.
 *
 *   connectivity  4 or 8.  Two pixels are neighbours if they differ by one step horizontally or vertically; with 8 a diagonal step
 *                 counts too.
 *   component     a maximal set of pixels of EQUAL RAW u8 VALUE that is connected through neighbours.  Every value forms components,
 *                 0 included.
 *   p = y*W + x   the raster index of a pixel inside its plane.
 *
 *   labels[p]     (int32) the smallest raster index of p's component: its first pixel in raster order.
 *   areas[p]      (int32) the number of pixels of p's component.
 *   out[p]        (u8, optional) = mask[p] if areas[p] >= min_area;
 *                 otherwise, with fill in 0..255: fill;
 *                 otherwise, with fill = -1 ("neighbour"), with r = labels[p] the component's first pixel:
 *                     mask[r-1]  if r is not in column 0                (the pixel left of the first pixel)
 *                     mask[r-W]  else if r is not in row 0              (the pixel above it)
 *                     mask[p]    else: the component that holds pixel (0, 0) has no such neighbour and is kept.
 *                 That neighbour necessarily has another value than the component (it precedes the component's first pixel in raster
 *                 order and touches it), and for an enclosed island or hole it belongs to the enclosing region.
 *                 min_area <= 1 changes nothing.
 *
 * Values are read from the INPUT: this is ONE pass.  A small speck nested inside a small speck takes the outer speck's input
 * value, not what the outer speck becomes, so the filter is not idempotent on nested specks; applying it again finishes the job.
 *
 * Summary rows (optional): rows (n, GSA_COMP_ROW) int64; the call writes EVERY word of every row.  Slots as in include/gsa_stats.h:
 * slot k < 8 is mask value k, slot 8 takes every value >= 8.
 *
 *     words    field              definition
 *     0..8     ncomp[s]           number of components whose value falls in slot s
 *     9..17    largest[s]         largest area among those components, 0 if there is none
 *     18       small components   number of components with area < min_area
 *     19       small pixels       sum of the areas of those components
 *
 * The rows depend neither on fill nor on whether out is given.  Every quantity is an integer sum, minimum or maximum: no result
 * depends on the order in which the kernels' workgroups arrive.
 *
 * Conventions as include/gsa_mask.h: `stream` is a hipStream_t as void*, calls are stream-ordered and never synchronise, device
 * pointers, 0 on success / negative gsa_status on error.  Stateless: no context; labels and areas are the only working storage.
 */
#ifndef GSA_COMPONENTS_H
#define GSA_COMPONENTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSA_COMP_SLOTS 9            /* mask values 0..7, then "8 and above" */
#define GSA_COMP_NCOMP 0            /* + s */
#define GSA_COMP_LARGEST 9          /* + s */
#define GSA_COMP_SMALL 18
#define GSA_COMP_SMALL_PIXELS 19
#define GSA_COMP_ROW 20             /* int64 words of a row */
#define GSA_COMP_FILL_NEIGHBOUR (-1)

/* mask: (n, H, W) u8, any alignment.  labels, areas: (n, H, W) int32, required: they are the results AND the kernels' working storage
 * (8 bytes per pixel), owned by the caller; whatever they hold before the call is overwritten.  out: (n, H, W) u8 or null, must not
 * overlap mask.  rows: (n, GSA_COMP_ROW) int64, 8-byte aligned, or null.  connectivity 4 or 8; min_area >= 0; fill in -1..255.
 * H and W each 1..65535 with H * W < 2^31.  n = 0 is a successful no-op.  n < 0, a size outside the range, another connectivity,
 * fill outside -1..255, min_area < 0, a null mask, labels or areas with n > 0, or out overlapping mask: GSA_ERR_INVALID. */
int gsa_mask_components(void* stream, int32_t n, int32_t H, int32_t W, int32_t connectivity, int32_t min_area, int32_t fill,
                        const uint8_t* mask, int32_t* labels, int32_t* areas, uint8_t* out, int64_t* rows);

#ifdef __cplusplus
}
#endif
#endif /* GSA_COMPONENTS_H */
