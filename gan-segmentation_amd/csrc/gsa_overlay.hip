// gsa_overlay.hip -- the pair previews' kernel (gsa_overlay.h): the class colours of a mask blended over its
// image, another weight on the class outlines, the f x f box thumbnail of that and the cell of a contact sheet it goes to.
//
// One launch for the samples, no workspace, and a second small launch that clears the cells of the sheet's last row that hold no
// sample.  A workgroup owns a kTileW x kTileH tile of input pixels -- both multiples of 16, the largest factor, so no thumbnail
// block straddles two workgroups, no atomics are needed and every output byte has exactly one writer.  It stages
//
//   the mask tile   with a 1-px apron (one dword column on each side, one row above and below) in LDS, one byte per pixel; what lies
//                   outside the image is staged as 0 and never read as a value: whether a neighbour counts is decided on coordinates
//   the table       once, as 256 x (colour dword, w_in | w_edge << 8) with both weights already clamped to 128: the per-pixel look-up
//                   is then one 8-byte LDS gather with per-lane indices
//
// and then a thread owns 4 consecutive pixels of 4 consecutive rows.  For each row it takes the mask dword and its four neighbour
// dwords from LDS, forms "differs from a neighbour" for its four pixels with dword operations (xor against the dword shifted by a
// pixel, the row above and the row below; a neighbour outside the image is replaced by the pixel itself), reads its 4 * C image
// bytes as C dwords, blends, and
//
//   f = 1        packs the 4 * C result bytes into C dwords and stores them
//   f = 2, 4     sums the f x f blocks in its own registers and stores the rounded bytes
//   f = 8, 16    leaves the sum of its 4 x 4 pixels per channel in LDS; after a barrier one thread per thumbnail pixel adds the 4 or
//                16 partial sums of its block and stores the bytes
//
// The kernel reads C + 1 bytes per pixel and writes C / f^2; it is templated on C (the byte positions of a pixel's channels in the
// loaded dwords are then constants), on f and on the access form.
//
// Global access: dword loads, and dword stores at f = 1, when W is a multiple of 4 and the pointers are aligned to that (every
// generated pair); the byte form of load_px4 / store_px4 with per-byte bounds otherwise.  Thumbnails are stored as bytes in either form.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gsa.h"
#include "gsa_overlay.h"
#include "gsa_plane.h"

namespace {

using namespace gsa::plane;

constexpr int kThreads = 256;
constexpr int kTileW = 128;                     // input pixels of a workgroup: 128 x 32 -- rows of 128 C bytes of image, 128 of mask
constexpr int kTileH = 32;
constexpr int kTileD = kTileW / 4;              // 32 dwords of a tile row of the mask
constexpr int kGroups = kTileH / 4;             // 8 groups of 4 rows
constexpr int kRows = kTileH + 2;               // staged rows: one above, one below
constexpr int kColsD = kTileD + 2;              // staged dword columns: one left, one right
constexpr int kMaxFactor = 16;
constexpr unsigned kFullWeight = 128;

static_assert(kTileD * kGroups == kThreads, "a thread owns 4 pixels of 4 rows");
static_assert(kTileW % kMaxFactor == 0 && kTileH % kMaxFactor == 0, "no thumbnail block straddles two tiles");

constexpr int shift_of(int f) { return f == 1 ? 0 : f == 2 ? 2 : f == 4 ? 4 : f == 8 ? 6 : 8; }    // 2 * log2 f

template <int C, int F, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void overlay_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask,
                                                           const uint8_t* __restrict__ lut, uint8_t* __restrict__ out, int H, int W,
                                                           int cols, int tiles_x, int tiles_per_plane) {
    __shared__ unsigned lds_m[kRows * kColsD];
    __shared__ uint2 lds_lut[256];
    __shared__ unsigned lds_part[F >= 8 ? kThreads * C : 1];
    constexpr int kShift = shift_of(F);
    constexpr unsigned kHalf = (unsigned)(F * F / 2);
    const Tile tl = tile_of(tiles_x, tiles_per_plane);                  // uniform over the workgroup
    const int y0 = tl.tile_y * kTileH, x0 = tl.tile_x * kTileW;
    const uint8_t* __restrict__ plane_m = mask + (size_t)tl.plane * H * W;      // every image is a plane of its own: no neighbour leaves it
    const uint8_t* __restrict__ plane_i = img + (size_t)tl.plane * H * W * C;
    const int h = H / F, w = W / F;                                     // the thumbnail, and its cell of the sheet
    const int cell_y = tl.plane / cols, cell_x = tl.plane - cell_y * cols;
    const size_t out_row = (size_t)cols * w * C;                        // bytes of a row of the sheet
    uint8_t* __restrict__ cell = out + (size_t)cell_y * h * out_row + (size_t)cell_x * w * C;

    {
        const uint8_t* r = lut + 6 * threadIdx.x;                       // 256 threads, 256 rows
        lds_lut[threadIdx.x] = make_uint2(r[0] | ((unsigned)r[1] << 8) | ((unsigned)r[2] << 16) | ((unsigned)r[3] << 24),
                                          min((unsigned)r[4], kFullWeight) | (min((unsigned)r[5], kFullWeight) << 8));
    }
    for (int i = threadIdx.x; i < kRows * kColsD; i += kThreads) {
        const int j = i / kColsD, k = i % kColsD;
        const int gy = y0 - 1 + j, gx = x0 - 4 + 4 * k;
        lds_m[i] = (unsigned)gy < (unsigned)H ? load_px4<ALIGNED>(plane_m + (size_t)gy * W, gx, W) : 0u;
    }
    __syncthreads();

    const int d = threadIdx.x % kTileD, g = threadIdx.x / kTileD;
    const int gx = x0 + 4 * d, gy0 = y0 + 4 * g;
    if (gx < W && gy0 < H) {                                            // no return: at F >= 8 a barrier follows
        const int row_bytes = W * C, at = gx * C;                       // an image row as bytes; <= 4 * 65535
        unsigned px[4][C];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int k = 0; k < C; ++k)
                px[r][k] = gy0 + r < H ? load_px4<ALIGNED>(plane_i + (size_t)(gy0 + r) * row_bytes, at + 4 * k, row_bytes) : 0u;
        }
        unsigned rmask = 0;                                             // 0xff where the pixel has a right neighbour inside the image
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (gx + b + 1 < W) rmask |= 0xffu << (8 * b);
        const unsigned* m = lds_m + (4 * g + 1) * kColsD + d + 1;       // the mask dword of (gy0, gx)
        unsigned acc[F == 2 ? 2 : 1][C] = {};                           // block sums in progress (F >= 2)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gy = gy0 + r;
            if (gy >= H) break;
            const unsigned own = m[r * kColsD];
            const unsigned up = gy > 0 ? m[(r - 1) * kColsD] : own, dn = gy + 1 < H ? m[(r + 1) * kColsD] : own;
            const unsigned lf = gx > 0 ? m[r * kColsD - 1] : own << 24, rt = m[r * kColsD + 1];
            const unsigned left = (own << 8) | (lf >> 24), right = (own >> 8) | (rt << 24);       // byte b: the pixel's neighbour
            const unsigned diff = (own ^ up) | (own ^ dn) | (own ^ left) | ((own ^ right) & rmask);
            unsigned bl[4][C];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint2 row = lds_lut[byte_of(own, b)];
                const unsigned wt = byte_of(diff, b) ? row.y >> 8 : row.y & 255u;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    const int at_b = C * b + ch;                        // a constant once unrolled
                    bl[b][ch] = (wt * byte_of(row.x, ch) + (kFullWeight - wt) * byte_of(px[r][at_b / 4], at_b % 4)) >> 7;
                }
            }
            if constexpr (F == 1) {
                uint8_t* o = cell + (size_t)gy * out_row;
#pragma unroll
                for (int k = 0; k < C; ++k) {
                    unsigned v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = bl[(4 * k + j) / C][(4 * k + j) % C];
                    store_px4<ALIGNED>(o, at + 4 * k, row_bytes, pack4(v));
                }
            } else if constexpr (F == 2) {
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    acc[0][ch] += bl[0][ch] + bl[1][ch];
                    acc[1][ch] += bl[2][ch] + bl[3][ch];
                }
                if (r & 1) {
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int X = gx / 2 + s;
                        if (X < w) {                                    // W % 4 == 2: the second block of the last thread is outside
                            uint8_t* o = cell + (size_t)(gy / 2) * out_row + (size_t)X * C;
#pragma unroll
                            for (int ch = 0; ch < C; ++ch) o[ch] = (uint8_t)((acc[s][ch] + kHalf) >> kShift);
                        }
#pragma unroll
                        for (int ch = 0; ch < C; ++ch) acc[s][ch] = 0;
                    }
                }
            } else {
#pragma unroll
                for (int ch = 0; ch < C; ++ch) acc[0][ch] += bl[0][ch] + bl[1][ch] + bl[2][ch] + bl[3][ch];
            }
        }
        if constexpr (F == 4) {                                         // H % 4 == 0: the four rows were all inside
            uint8_t* o = cell + (size_t)(gy0 / 4) * out_row + (size_t)(gx / 4) * C;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) o[ch] = (uint8_t)((acc[0][ch] + kHalf) >> kShift);
        } else if constexpr (F >= 8) {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) lds_part[threadIdx.x * C + ch] = acc[0][ch];
        }
    }
    if constexpr (F >= 8) {
        constexpr int kOutX = kTileW / F, kOutY = kTileH / F, kSide = F / 4;       // thumbnail pixels of a tile; partial sums along a block's side
        __syncthreads();
        const int ox = threadIdx.x % kOutX, oy = threadIdx.x / kOutX;
        // W and H are multiples of F: a block whose first pixel is inside is inside as a whole, and its partial sums were all written
        if (oy < kOutY && x0 + ox * F < W && y0 + oy * F < H) {
            uint8_t* o = cell + (size_t)(y0 / F + oy) * out_row + (size_t)(x0 / F + ox) * C;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                unsigned s = kHalf;
                for (int i = 0; i < kSide; ++i)
                    for (int j = 0; j < kSide; ++j) s += lds_part[((oy * kSide + i) * kTileD + ox * kSide + j) * C + ch];
                o[ch] = (uint8_t)(s >> kShift);
            }
        }
    }
}

// Zeroes the rectangle of `rows` x `seg_bytes` bytes at `first` in rows of `row_bytes`: the cells of the sheet's last row that hold
// no sample.  A thread clears 4 bytes.
template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void overlay_clear_kernel(uint8_t* __restrict__ first, int row_bytes, int seg_bytes, int seg_d,
                                                                 unsigned items) {
    const unsigned i = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    if (i >= items) return;
    const unsigned y = i / (unsigned)seg_d, k = i - y * (unsigned)seg_d;
    store_px4<ALIGNED>(first + (size_t)y * row_bytes, (int)(4 * k), seg_bytes, 0u);
}

using Kernel = void (*)(const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*, int, int, int, int, int);

template <int C, int F>
Kernel kernel_of(bool aligned) {
    return aligned ? overlay_kernel<C, F, true> : overlay_kernel<C, F, false>;
}
template <int C>
Kernel kernel_of(int factor, bool aligned) {
    return factor == 1 ? kernel_of<C, 1>(aligned) : factor == 2 ? kernel_of<C, 2>(aligned) : factor == 4 ? kernel_of<C, 4>(aligned)
           : factor == 8 ? kernel_of<C, 8>(aligned) : kernel_of<C, 16>(aligned);
}

}  // namespace

extern "C" {

int gsa_overlay(void* stream, int32_t n, int32_t H, int32_t W, int32_t channels, const uint8_t* img, const uint8_t* mask, const uint8_t* lut,
                int32_t factor, int32_t cols, uint8_t* out) {
    if (n == 0) return GSA_OK;
    if (n < 0 || !extent_ok_31(H, W) || channels < 1 || channels > 4 || cols < 1) return GSA_ERR_INVALID;
    if (factor != 1 && factor != 2 && factor != 4 && factor != 8 && factor != 16) return GSA_ERR_INVALID;
    if (H % factor || W % factor || !img || !mask || !lut || !out) return GSA_ERR_INVALID;
    const long long h = H / factor, w = W / factor, rows = ((long long)n + cols - 1) / cols;
    const long long sheet_rows = rows * h, row_bytes = (long long)cols * w * channels;         // < 2^47 and < 2^50
    if (sheet_rows >= (1ll << 31) || row_bytes >= (1ll << 31) || sheet_rows * row_bytes >= (1ll << 31)) return GSA_ERR_INVALID;
    const uint64_t pixels = (uint64_t)n * (uint64_t)H * (uint64_t)W, out_bytes = (uint64_t)(sheet_rows * row_bytes);
    if (ranges_overlap(out, out_bytes, img, pixels * (uint64_t)channels) || ranges_overlap(out, out_bytes, mask, pixels) ||
        ranges_overlap(out, out_bytes, lut, 256 * 6))
        return GSA_ERR_INVALID;
    const TileGrid g = tile_grid(H, W, kTileW, kTileH);
    if (g.per_plane * n >= kMaxWorkgroups) return GSA_ERR_INVALID;     // refused, not split
    // the cells of the last row without a sample: one rectangle, `empty` cells wide
    const long long empty = rows * cols - n, seg_bytes = empty * w * channels, seg_d = (seg_bytes + 3) / 4, items = h * seg_d;
    const long long clear_groups = (items + kThreads - 1) / kThreads;
    if (clear_groups >= kMaxWorkgroups) return GSA_ERR_INVALID;
    const uintptr_t a = reinterpret_cast<uintptr_t>(img), b = reinterpret_cast<uintptr_t>(mask), c = reinterpret_cast<uintptr_t>(out);
    const bool aligned = W % 4 == 0 && ((a | b) & 3) == 0 && (factor > 1 || (c & 3) == 0);
    const Kernel kernel = channels == 1   ? kernel_of<1>(factor, aligned)
                          : channels == 2 ? kernel_of<2>(factor, aligned)
                          : channels == 3 ? kernel_of<3>(factor, aligned)
                                          : kernel_of<4>(factor, aligned);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(g.per_plane * n)), dim3(kThreads), 0, (hipStream_t)stream, img, mask, lut, out, (int)H, (int)W,
                       (int)cols, (int)g.tiles_x, (int)g.per_plane);
    if (empty > 0) {
        uint8_t* first = out + (uint64_t)((rows - 1) * h * row_bytes + (cols - empty) * w * channels);
        const bool whole = ((c | (uintptr_t)row_bytes | (uintptr_t)((cols - empty) * w * channels) | (uintptr_t)seg_bytes) & 3) == 0;
        hipLaunchKernelGGL(whole ? overlay_clear_kernel<true> : overlay_clear_kernel<false>, dim3((unsigned)clear_groups), dim3(kThreads), 0,
                           (hipStream_t)stream, first, (int)row_bytes, (int)seg_bytes, (int)seg_d, (unsigned)items);
    }
    return hipGetLastError() == hipSuccess ? GSA_OK : GSA_ERR_HIP;
}

}  // extern "C"
