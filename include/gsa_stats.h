/*
 * gsa_stats.h -- C ABI of the on-device pair statistics: one pass over a generated (image, mask) batch that already lies in HBM
 * leaves, per sample, the integer sums, minima and maxima a dataset report is made of.  The reference has
 * no counterpart: it writes 0.8 pairs/s and a person can watch them go by.
 *
 * The rule (canonical, all integers).  Inputs: img (n, H, W, C) u8 with C in 0..4 (C = 0: no image, a null pointer -- a caller that
 * has only labels), mask (n, H, W) u8.  Output: rows (n, GSA_STATS_ROW) int64; the call writes EVERY word of every row, whatever
 * the buffer held before.
 *
 * Nine slots s: slot k < 8 is mask value k, slot 8 takes every value >= 8 (the training stream's ignore label 255 among them).
 * One row, in this order:
 *
 *     words    field                        definition
 *     0..8     count[s]                     pixels of the sample whose mask value falls in slot s
 *     9..44    box[s] = x0, y0, x1, y1      smallest and largest column and row index of those pixels; an empty slot: W, H, -1, -1
 *     45..80   csum[s][c], c < 4            sum of channel c over the pixels of slot s; 0 for c >= C
 *     81..84   sqsum[c]                     sum of the squared u8 value of channel c over the whole sample; 0 for c >= C
 *     85       edge_h                       number of (y, x), x < W-1, with mask[y,x] != mask[y,x+1] -- raw u8 values, not slots
 *     86       edge_v                       the same for y < H-1 against mask[y+1,x]
 *     87       reserved                     written as 0
 *
 * Every sample is a plane of its own: no neighbour pair crosses from one image into the next, and the last pixel of one row and
 * the first pixel of the next row are not neighbours.
 *
 * Every quantity is an integer sum, minimum or maximum, so the order in which the kernel's workgroups add their partial results
 * into a row cannot change a bit of it: the rows are the same for any launch shape, batch size and number of ranks.
 *
 * Conventions as include/gsa_mask.h: `stream` is a hipStream_t as void*, calls are stream-ordered and never synchronise, device
 * pointers, 0 on success / negative gsa_status on error.  Stateless: no context, no workspace supplied by the caller.
 */
#ifndef GSA_STATS_H
#define GSA_STATS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSA_STATS_SLOTS 9       /* mask values 0..7, then "8 and above" */
#define GSA_STATS_CHANNELS 4    /* channel columns of a row; those >= C hold 0 */
#define GSA_STATS_COUNT 0       /* + s */
#define GSA_STATS_BOX 9         /* + 4 * s + {0: x0, 1: y0, 2: x1, 3: y1} */
#define GSA_STATS_CSUM 45       /* + 4 * s + c */
#define GSA_STATS_SQSUM 81      /* + c */
#define GSA_STATS_EDGE_H 85
#define GSA_STATS_EDGE_V 86
#define GSA_STATS_RESERVED 87
#define GSA_STATS_ROW 88        /* int64 words of a row */

/* img: (n, H, W, C) u8 or null with C = 0; mask: (n, H, W) u8; rows: (n, GSA_STATS_ROW) int64, 8-byte aligned; img and mask at any
 * alignment.  H and W each 1..65535 with H * W < 2^31; C in 0..4.  n = 0 is a successful no-op.  A null mask or rows with n > 0,
 * a null img with C > 0, n < 0 or a size or C outside the range: GSA_ERR_INVALID. */
int gsa_pair_stats(void* stream, int32_t n, int32_t H, int32_t W, int32_t C, const uint8_t* img, const uint8_t* mask, int64_t* rows);

#ifdef __cplusplus
}
#endif
#endif /* GSA_STATS_H */
