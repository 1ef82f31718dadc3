// gsa_boundary.hip -- the mask boundary distance's one kernel (include/gsa_boundary.h): for every pixel
// of every (H, W) u8 plane the squared Euclidean distance to the nearest pixel of another value, up to a radius R <= 32, and the
// mask with `label` wherever that distance is at most R*R.
//
// One launch, no workspace.  A workgroup owns a kTile x kTile tile of output pixels and stages it with an apron of A = 4K pixels
// (K = ceil(R / 4) rounded up to 1, 2, 4 or 8: a template argument) in LDS, one byte per pixel.  Two passes follow the separable
// form of the rule:
//
//   column pass   h[y][c] for the tile's 64 rows and all 64 + 2A staged columns: the vertical distance to the nearest pixel of the
//                 column with another value, capped at R + 1, as two run-length sweeps (down, then up) -- a work item is one
//                 column and 16 tile rows and starts each sweep R rows outside them, so every distance <= R is exact.  Rows outside
//                 the image restart the run at the cap: an image edge makes no boundary.  A column outside the image gets
//                 kOutside in every row.
//   row pass      a work item is 4 pixels of a tile row (one dword).  It walks the 2K + 1 dwords of mask and h around its own and
//                 takes, for each of its pixels p and each byte q, dx^2 + hh^2 with hh = h[q] where mask[q] == mask[p] and
//                 h[q] & kOutside where it differs: 0 for a pixel of the image, 128 for a position outside it, which (as
//                 128^2 > 32^2) can never come into the band.  Inside / outside is decided on coordinates in the column pass;
//                 no mask value serves as filler.  Taps with |dx| > R need no test of their own: dx^2 > R*R fails the band's
//                 threshold.  Both results are written from registers.
//
// The kernel is bound by the row pass's VALU work, 4 operations per (pixel, tap) and 4K + 1 .. 8K + 7 taps per pixel, not by its
// 2 .. 4 bytes per pixel of HBM traffic; K keeps a band of a few pixels from paying for the 65 taps of R = 32.
//
// Global access: dword loads and stores (8-byte stores of dist2) when W is a multiple of 4 and the pointers are aligned to
// that (every generated mask); byte and int16 access with per-pixel bounds otherwise (any H, W in 1..65535 is accepted).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gsa.h"
#include "../../include/gsa_boundary.h"
#include "gsa_plane.h"

namespace {

using namespace gsa::plane;

constexpr int kThreads = 256;
constexpr int kTile = 64;                       // output pixels of a workgroup: 64 x 64
constexpr int kTileD = kTile / 4;               // 16 dwords of a tile row
constexpr int kSegment = 16;                    // tile rows of a column-pass work item
constexpr unsigned kOutside = 0x80u;            // h of a column outside the image; its square exceeds every R*R

static_assert(kOutside * kOutside > GSA_BOUNDARY_MAX_RADIUS * GSA_BOUNDARY_MAX_RADIUS && GSA_BOUNDARY_MAX_RADIUS + 1 < (int)kOutside,
              "a position outside the image never comes into the band, and the cap R + 1 never looks like it");
static_assert(GSA_BOUNDARY_MAX_RADIUS * GSA_BOUNDARY_MAX_RADIUS < GSA_BOUNDARY_FAR, "every distance in a band fits below FAR");
static_assert(kTile % kSegment == 0 && kTile % 4 == 0, "whole segments, dword columns");

// K: dwords of apron on each side (apron A = 4K pixels >= R).  LDS: (64 + 8K) x (64 + 8K) bytes of mask and 64 x (64 + 8K) bytes
// of h -- 9.8 KB at K = 1, 24 KB at K = 8.
template <int K, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void mask_boundary_kernel(const uint8_t* __restrict__ mask, int16_t* __restrict__ dist2,
                                                                 uint8_t* __restrict__ out, int H, int W, int R, unsigned label,
                                                                 int tiles_x, int tiles_per_plane) {
    constexpr int A = 4 * K;                    // apron in pixels
    constexpr int kRows = kTile + 2 * A;        // staged rows
    constexpr int kColsD = kTileD + 2 * K;      // staged dword columns
    constexpr int kCols = 4 * kColsD;           // staged byte columns
    __shared__ unsigned lds_m[kRows * kColsD];
    __shared__ unsigned lds_h[kTile * kColsD];
    const Tile tl = tile_of(tiles_x, tiles_per_plane);                  // uniform over the workgroup
    const int y0 = tl.tile_y * kTile, x0 = tl.tile_x * kTile;
    const size_t plane_at = (size_t)tl.plane * H * W;
    const uint8_t* __restrict__ plane_in = mask + plane_at;             // every image is a plane of its own: no tap leaves it

    // stage the tile and its apron; what lies outside the image is never read as a value (0 keeps the LDS defined)
    for (int i = threadIdx.x; i < kRows * kColsD; i += kThreads) {
        const int j = i / kColsD, d = i % kColsD;
        const int gy = y0 - A + j, gx = x0 - A + 4 * d;
        unsigned v = 0;
        if ((unsigned)gy < (unsigned)H) {
            const uint8_t* p = plane_in + (size_t)gy * W;
            if (ALIGNED) {                      // W % 4 == 0 and gx % 4 == 0: the dword is inside or outside as a whole
                if ((unsigned)gx < (unsigned)W) v = *reinterpret_cast<const unsigned*>(p + gx);
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if ((unsigned)(gx + b) < (unsigned)W) v |= (unsigned)p[gx + b] << (8 * b);
            }
        }
        lds_m[i] = v;
    }
    __syncthreads();

    // column pass: h for the tile's rows over every staged column
    {
        const uint8_t* m8 = reinterpret_cast<const uint8_t*>(lds_m);
        uint8_t* h8 = reinterpret_cast<uint8_t*>(lds_h);
        const unsigned cap = (unsigned)R + 1u;
        for (int i = threadIdx.x; i < (kTile / kSegment) * kCols; i += kThreads) {
            const int c = i % kCols, t0 = (i / kCols) * kSegment;       // staged column, first tile row
            const int gx = x0 - A + c;
            if ((unsigned)gx >= (unsigned)W) {
                for (int t = t0; t < t0 + kSegment; ++t) h8[t * kCols + c] = (uint8_t)kOutside;
                continue;
            }
            // down: distance to the nearest other value above.  Staged row j is image row y0 - A + j; A >= R keeps j >= 0.
            unsigned run = cap, prev = 0;
            bool prev_inside = false;
            for (int j = t0 + A - R; j < t0 + A + kSegment; ++j) {
                const bool inside = (unsigned)(y0 - A + j) < (unsigned)H;
                const unsigned v = m8[j * kCols + c];
                run = !inside ? cap : (prev_inside && v != prev) ? 1u : min(run + 1u, cap);
                prev = v;
                prev_inside = inside;
                if (j >= t0 + A) h8[(j - A) * kCols + c] = (uint8_t)run;
            }
            // up: the same from below, j <= 63 + A + R < kRows; the smaller of the two stays
            run = cap;
            prev_inside = false;
            for (int j = t0 + A + kSegment - 1 + R; j >= t0 + A; --j) {
                const bool inside = (unsigned)(y0 - A + j) < (unsigned)H;
                const unsigned v = m8[j * kCols + c];
                run = !inside ? cap : (prev_inside && v != prev) ? 1u : min(run + 1u, cap);
                prev = v;
                prev_inside = inside;
                if (j < t0 + A + kSegment) {
                    uint8_t* q = h8 + (j - A) * kCols + c;
                    *q = (uint8_t)min((unsigned)*q, run);
                }
            }
        }
    }
    __syncthreads();

    // row pass: 4 pixels of a tile row per work item
    const unsigned R2 = (unsigned)(R * R);
    for (int i = threadIdx.x; i < kTile * kTileD; i += kThreads) {
        const int t = i / kTileD, d = i % kTileD;
        const int gy = y0 + t, gx = x0 + 4 * d;
        if (gy >= H || gx >= W) continue;       // no barrier follows
        const unsigned* mrow = lds_m + (t + A) * kColsD + K + d;
        const unsigned* hrow = lds_h + t * kColsD + K + d;
        const unsigned own = mrow[0];
        unsigned mp[4], best[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            mp[p] = byte_of(own, p);
            best[p] = GSA_BOUNDARY_FAR;
        }
#pragma unroll
        for (int k = -K; k <= K; ++k) {
            const unsigned mw = mrow[k], hw = hrow[k];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const unsigned mq = byte_of(mw, b), hq = byte_of(hw, b), hf = hq & kOutside;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int dx = 4 * k + b - p;                       // a constant once unrolled
                    if (dx * dx > A * A) continue;                      // beyond every R of this K
                    const unsigned hh = mq != mp[p] ? hf : hq;
                    best[p] = min(best[p], __umul24(hh, hh) + (unsigned)(dx * dx));
                }
            }
        }
        unsigned o = 0;
        unsigned dd[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const bool in = best[p] <= R2;
            dd[p] = in ? best[p] : (unsigned)GSA_BOUNDARY_FAR;
            o |= (in ? label : mp[p]) << (8 * p);
        }
        const size_t at = plane_at + (size_t)gy * W + gx;
        if (ALIGNED) {                          // W % 4 == 0: the four pixels are inside as a whole
            if (out) *reinterpret_cast<unsigned*>(out + at) = o;
            if (dist2) *reinterpret_cast<uint2*>(dist2 + at) = make_uint2(dd[0] | (dd[1] << 16), dd[2] | (dd[3] << 16));
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (gx + p < W) {
                    if (out) out[at + p] = (uint8_t)byte_of(o, p);
                    if (dist2) dist2[at + p] = (int16_t)dd[p];
                }
            }
        }
    }
}

}  // namespace

extern "C" {

int gsa_mask_boundary(void* stream, int32_t n, int32_t H, int32_t W, int32_t radius, int32_t label, const uint8_t* mask, int16_t* dist2,
                      uint8_t* out) {
    if (n < 0 || !extent_ok_31(H, W)) return GSA_ERR_INVALID;
    if (radius < 1 || radius > GSA_BOUNDARY_MAX_RADIUS || label < 0 || label > 255) return GSA_ERR_INVALID;
    if (n == 0) return GSA_OK;
    if (!mask || (!dist2 && !out)) return GSA_ERR_INVALID;
    const uint64_t pixels = (uint64_t)n * (uint64_t)H * (uint64_t)W;
    const uintptr_t a = reinterpret_cast<uintptr_t>(mask), b = reinterpret_cast<uintptr_t>(out), c = reinterpret_cast<uintptr_t>(dist2);
    if (c & 1) return GSA_ERR_INVALID;
    if (out && ranges_overlap(mask, pixels, out, pixels)) return GSA_ERR_INVALID;
    if (dist2 && ranges_overlap(mask, pixels, dist2, 2 * pixels)) return GSA_ERR_INVALID;
    if (out && dist2 && ranges_overlap(out, pixels, dist2, 2 * pixels)) return GSA_ERR_INVALID;
    const TileGrid g = tile_grid(H, W, kTile, kTile);
    if (g.per_plane * n >= kMaxWorkgroups) return GSA_ERR_INVALID;     // refused, not split
    const bool aligned = W % 4 == 0 && ((a | b) & 3) == 0 && (c & 7) == 0;     // a null pointer is aligned
    const auto kernel = radius <= 4    ? (aligned ? mask_boundary_kernel<1, true> : mask_boundary_kernel<1, false>)
                        : radius <= 8  ? (aligned ? mask_boundary_kernel<2, true> : mask_boundary_kernel<2, false>)
                        : radius <= 16 ? (aligned ? mask_boundary_kernel<4, true> : mask_boundary_kernel<4, false>)
                                       : (aligned ? mask_boundary_kernel<8, true> : mask_boundary_kernel<8, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(g.per_plane * n)), dim3(kThreads), 0, (hipStream_t)stream, mask, dist2, out, H, W, (int)radius,
                       (unsigned)label, (int)g.tiles_x, (int)g.per_plane);
    return hipGetLastError() == hipSuccess ? GSA_OK : GSA_ERR_HIP;
}

}  // extern "C"
