// gsa_refine.hip -- the kernel of the image-guided mask refinement (gsa_refine.h): every pixel takes the class
// that its neighbours of similar colour agree on, a joint bilateral vote over a (2R + 1)^2 window, in integers.
//
// One launch, no workspace, no atomics.  A workgroup of 256 threads owns a kTileW x kTileH tile and stages, once,
//
//   the tile        with an apron of R rows above and below and kPad columns on each side, ONE dword per pixel: for C <= 3 the colour
//                   in the low bytes and the label in the top byte; for C = 4 the colour dword in one array and the label in a second.
//                   What lies outside the plane is staged with label 255, which is >= K and so votes nothing: a tap needs no
//                   coordinate test.  kPad = 8 >= R keeps a thread's row segment 16-byte aligned for ds_read_b128.
//   wr              as 1024 bytes, wr[min(s, 255)] for every byte sum s <= 4 * 255: the per-tap clamp is in the table
//   ws              as 121 dwords, the entries outside the radius as 0 (they are never read from `tables`)
//
// and then a thread owns 4 consecutive pixels of 2 consecutive rows.  It walks the 2R + 2 staged rows its block needs, ROLLED (one
// pass per staged row; the first serves the upper output row only, the last the lower one only, the rest both: three inlined forms),
// because a fully unrolled R = 5 body is 8 * 121 taps of 6 to 12 instructions, several times the instruction cache.  A pass reads its
// row segment wide (3 or 5 uint4), splits every dword into colour and label once, forms the K one-hot flags of the label once per
// dword, and then for each of its up to 4 x 2 centre pixels the dword serves
//
//   s = v_sad_u8(centre colour, colour)        the byte-wise distance of two packed pixels, one instruction
//   t = lds_wr[s] * ws[dy][dx]                 one LDS byte gather with per-lane indices, one 24-bit multiply
//   votes[c] += t * flag[c]   for c < KMAX     one v_mad_i32_i24 per class: selected by a flag, never by an index
//
// With KMAX = 2 there is ONE accumulator, votes[0] - votes[1], and the flag is +1, -1 or 0: the decision between two classes needs
// the sign of the difference only (0 is the tie, which keeps the pixel's value).
//
// The accumulators are arrays with constant indices after unrolling, i.e. registers; no instantiation uses scratch.  The weights of
// an offset are uniform reads of the LDS copy (the table may start at any address, so scalar dword loads are not to be had); they
// cost 2R + 1 dwords per pass and output row beside 4 * (2R + 1) gathers.
//
// Templated on R (the segment width and the dx loop), on KMAX in {2, 4, 8} (classes <= KMAX: accumulators of the classes K .. KMAX - 1
// collect frozen neighbours' votes and are left out of the decision), on C and on the access form.  No wave intrinsics and no
// cross-lane moves: the unit runs on the host stand-in as well.
//
// Global access: dword loads and stores when W is a multiple of 4 and img, mask and out are aligned to that (every generated pair);
// the byte form of load_px4 / store_px4 with per-byte bounds otherwise.  `tables` is read byte by byte in either form.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gsa.h"
#include "gsa_plane.h"
#include "gsa_refine.h"

namespace {

using namespace gsa::plane;

constexpr int kThreads = 256;
constexpr int kTileW = 64;                      // pixels of a workgroup: 64 x 32, a thread 4 x 2 of them
constexpr int kTileH = 32;
constexpr int kPxW = 4, kPxH = 2;
constexpr int kTileD = kTileW / kPxW;           // 16 threads along a tile row
constexpr int kGroups = kTileH / kPxH;          // 16 along a column
constexpr int kPad = 8;                         // staged columns on each side of the tile: >= kMaxRadius and a multiple of 4
constexpr int kStageW = kTileW + 2 * kPad;      // 80 staged columns
constexpr int kStageD = kStageW / 4;            // 20 uint4 of a staged row
constexpr int kMaxRadius = 5;
constexpr int kMaxClasses = 8;
constexpr int kWsSide = 2 * kMaxRadius + 1;     // 11
constexpr int kWrBytes = 256;
constexpr int kTableBytes = kWrBytes + kWsSide * kWsSide;       // 377
constexpr int kWrStaged = 1024;                 // > 4 * 255, the largest byte sum
constexpr unsigned kOutside = 255;              // the label of a staged position outside the plane

static_assert(kTileD * kGroups == kThreads, "a thread owns 4 pixels of 2 rows");
static_assert(kPad >= kMaxRadius && kPad % 4 == 0, "the apron holds every tap and keeps the segments aligned");
static_assert(kMaxClasses <= kOutside, "an outside position is frozen for every K");

// The staged columns a thread's segment covers, relative to its first quad column d: quads kSegFirst .. kSegFirst + kSegQuads - 1 of
// the staged row hold every column from 4d + kPad - R to 4d + kPad + 3 + R.
constexpr int seg_first(int R) { return (kPad - R) / 4; }
constexpr int seg_quads(int R) { return (kPad + 3 + R) / 4 - seg_first(R) + 1; }

// The sum of the four absolute byte differences of a and b: the distance of two packed pixels.
__device__ __forceinline__ unsigned sad4(unsigned a, unsigned b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(a, b, 0u);
#else
    unsigned s = 0;
    for (int k = 0; k < 4; ++k) {
        const int x = (int)byte_of(a, k), y = (int)byte_of(b, k);
        s += (unsigned)(x > y ? x - y : y - x);
    }
    return s;
#endif
}

// The weight of an offset as the compiler should see it: 8 bits.  Both factors of a tap's weight are then known to fit 24 bits and
// their product is one full-rate v_mul_u32_u24 (__umul24 on the dword came out as a mask and v_mul_lo_u32, a quarter of the rate).
__device__ __forceinline__ int weight_of(unsigned w) { return (int)(w & 255u); }

// c + a * b for a and b within 24 bits, signed.  Written out for the device: with a flag of -1, 0 or 1 as one factor the compiler
// chose v_mul_lo_u32, a quarter of the rate, and an add.
__device__ __forceinline__ int mad24(int a, int b, int c) {
#if defined(__HIP_DEVICE_COMPILE__)
    int d;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
#else
    return a * b + c;
#endif
}

// The accumulators of a pixel.  KMAX > 2: one per class.  KMAX == 2: ONE, votes[0] - votes[1] -- all the decision between two classes
// needs -- fed by a flag of +1, -1 or 0.
constexpr int accumulators(int KMAX) { return KMAX == 2 ? 1 : KMAX; }

// The colour of pixel b of the four whose C * 4 bytes are w[0 .. C - 1], channel ch in byte ch.
template <int C>
__device__ __forceinline__ unsigned colour_of(const unsigned (&w)[C], int b) {
    unsigned v = 0;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const int at = C * b + ch;              // a constant once unrolled
        v |= byte_of(w[at / 4], at % 4) << (8 * ch);
    }
    return v;
}

// One staged row's votes for a thread's block: DO0 / DO1 say whether the row lies within R rows of the upper / lower output row.
// seg, lab_seg: the thread's first uint4 of the row; ws0, ws1: the weights of the row's dy for either output row, at dx = 0.
template <int R, int KMAX, bool C4, bool DO0, bool DO1>
__device__ __forceinline__ void row_pass(const uint4* seg, const uint4* lab_seg, const unsigned* ws0, const unsigned* ws1,
                                         const uint8_t* lds_wr, const unsigned (&centre)[kPxH][kPxW], int (&votes)[kPxH][kPxW][accumulators(KMAX)]) {
    constexpr int kAcc = accumulators(KMAX);
    constexpr int kQuads = seg_quads(R), kOwn = kPad - 4 * seg_first(R);       // kOwn: the segment position of the thread's first pixel
    unsigned col[4 * kQuads], lab[4 * kQuads];
#pragma unroll
    for (int q = 0; q < kQuads; ++q) {
        const uint4 v = seg[q];
        col[4 * q] = v.x, col[4 * q + 1] = v.y, col[4 * q + 2] = v.z, col[4 * q + 3] = v.w;
        if (C4) {
            const uint4 l = lab_seg[q];
            lab[4 * q] = l.x, lab[4 * q + 1] = l.y, lab[4 * q + 2] = l.z, lab[4 * q + 3] = l.w;
        }
    }
    int w[kPxH][2 * R + 1] = {};
#pragma unroll
    for (int k = 0; k <= 2 * R; ++k) {
        if (DO0) w[0][k] = weight_of(ws0[k - R]);
        if (DO1) w[1][k] = weight_of(ws1[k - R]);
    }
#pragma unroll
    for (int i = kOwn - R; i <= kOwn + kPxW - 1 + R; ++i) {
        unsigned c_i = col[i], u_i;
        if (C4) {
            u_i = lab[i];
        } else {
            u_i = c_i >> 24;
            c_i &= 0xffffffu;
        }
        int flag[kAcc];
        if (KMAX == 2) {
            flag[0] = (u_i == 0u ? 1 : 0) - (u_i == 1u ? 1 : 0);
        } else {
#pragma unroll
            for (int c = 0; c < kAcc; ++c) flag[c] = u_i == (unsigned)c ? 1 : 0;
        }
#pragma unroll
        for (int r = 0; r < kPxH; ++r) {
            if (r == 0 ? !DO0 : !DO1) continue;
#pragma unroll
            for (int b = 0; b < kPxW; ++b) {
                const int dx = i - kOwn - b;
                if (dx < -R || dx > R) continue;
                const int t = (int)lds_wr[sad4(centre[r][b], c_i)] * w[r][dx + R];     // < 2^16
#pragma unroll
                for (int c = 0; c < kAcc; ++c) votes[r][b][c] = mad24(t, flag[c], votes[r][b][c]);
            }
        }
    }
}

template <int R, int KMAX, int C, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void mask_refine_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask,
                                                               const uint8_t* __restrict__ tables, uint8_t* __restrict__ out, int H, int W,
                                                               int classes, int tiles_x, int tiles_per_plane) {
    constexpr bool C4 = C == 4;
    constexpr int kRows = kTileH + 2 * R;       // staged rows
    __shared__ uint4 lds_px[kRows * kStageD];
    __shared__ uint4 lds_lab[C4 ? kRows * kStageD : 1];
    __shared__ uint8_t lds_wr[kWrStaged];
    __shared__ unsigned lds_ws[kWsSide * kWsSide];
    const Tile tl = tile_of(tiles_x, tiles_per_plane);                  // uniform over the workgroup
    const int y0 = tl.tile_y * kTileH, x0 = tl.tile_x * kTileW;
    const uint8_t* __restrict__ plane_m = mask + (size_t)tl.plane * H * W;      // every image is a plane of its own: no neighbour leaves it
    const uint8_t* __restrict__ plane_i = img + (size_t)tl.plane * H * W * C;
    const int row_bytes = W * C;                                        // an image row as bytes; <= 4 * 65535

    {
        const uint8_t last = tables[kWrBytes - 1];                      // 256 threads, 256 weights; wr[255] for every sum beyond
        lds_wr[threadIdx.x] = tables[threadIdx.x];
#pragma unroll
        for (int k = 1; k < kWrStaged / kThreads; ++k) lds_wr[threadIdx.x + k * kThreads] = last;
    }
    if (threadIdx.x < kWsSide * kWsSide) {
        const int dy = (int)threadIdx.x / kWsSide - kMaxRadius, dx = (int)threadIdx.x % kWsSide - kMaxRadius;
        const bool inside = dy >= -R && dy <= R && dx >= -R && dx <= R;
        lds_ws[threadIdx.x] = inside ? (unsigned)tables[kWrBytes + threadIdx.x] : 0u;
    }
    for (int i = threadIdx.x; i < kRows * kStageD; i += kThreads) {
        const int t = i / kStageD, k = i % kStageD;
        const int gy = y0 - R + t, gx = x0 - kPad + 4 * k;
        const bool row_in = (unsigned)gy < (unsigned)H;
        unsigned m = 0, w[C] = {};
        if (row_in && gx + 3 >= 0 && gx < W) {
            m = load_px4<ALIGNED>(plane_m + (size_t)gy * W, gx, W);
#pragma unroll
            for (int c = 0; c < C; ++c) w[c] = load_px4<ALIGNED>(plane_i + (size_t)gy * row_bytes, gx * C + 4 * c, row_bytes);
        }
        unsigned px[4], lab[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            lab[b] = row_in && (unsigned)(gx + b) < (unsigned)W ? byte_of(m, b) : kOutside;
            px[b] = C4 ? colour_of<C>(w, b) : colour_of<C>(w, b) | (lab[b] << 24);
        }
        lds_px[i] = make_uint4(px[0], px[1], px[2], px[3]);
        if (C4) lds_lab[i] = make_uint4(lab[0], lab[1], lab[2], lab[3]);
    }
    __syncthreads();

    const int d = threadIdx.x % kTileD, g = threadIdx.x / kTileD;
    const int gx = x0 + kPxW * d, gy0 = y0 + kPxH * g;
    if (gx >= W || gy0 >= H) return;                                    // no barrier follows
    unsigned centre[kPxH][kPxW], own[kPxH][kPxW];
    int votes[kPxH][kPxW][accumulators(KMAX)] = {};
#pragma unroll
    for (int r = 0; r < kPxH; ++r) {
        const int at = (kPxH * g + R + r) * kStageD + d + kPad / 4;
        const uint4 c = lds_px[at];
        const unsigned px[4] = {c.x, c.y, c.z, c.w};
        uint4 l = c;
        if (C4) l = lds_lab[at];
        const unsigned lb[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
        for (int b = 0; b < kPxW; ++b) {
            centre[r][b] = C4 ? px[b] : px[b] & 0xffffffu;
            own[r][b] = C4 ? lb[b] : px[b] >> 24;
        }
    }
    // staged row kPxH * g + j holds dy = j - R for the upper output row and dy = j - R - 1 for the lower one
    const uint4* seg = lds_px + kPxH * g * kStageD + d + seg_first(R);
    const uint4* lab_seg = C4 ? lds_lab + kPxH * g * kStageD + d + seg_first(R) : lds_lab;
    const unsigned* ws = lds_ws + kMaxRadius * kWsSide + kMaxRadius;    // the entry of (0, 0)
    row_pass<R, KMAX, C4, true, false>(seg, lab_seg, ws - R * kWsSide, ws, lds_wr, centre, votes);
#pragma unroll 1
    for (int j = 1; j <= 2 * R; ++j)
        row_pass<R, KMAX, C4, true, true>(seg + j * kStageD, C4 ? lab_seg + j * kStageD : lab_seg, ws + (j - R) * kWsSide,
                                          ws + (j - R - 1) * kWsSide, lds_wr, centre, votes);
    row_pass<R, KMAX, C4, false, true>(seg + (2 * R + 1) * kStageD, C4 ? lab_seg + (2 * R + 1) * kStageD : lab_seg, ws, ws + R * kWsSide, lds_wr,
                                       centre, votes);

#pragma unroll
    for (int r = 0; r < kPxH; ++r) {
        const int gy = gy0 + r;
        if (gy >= H) break;
        unsigned o[4];
#pragma unroll
        for (int b = 0; b < kPxW; ++b) {
            const unsigned v = own[r][b];
            if constexpr (KMAX == 2) {                                  // classes == 2; the difference decides, 0 is the tie
                const int diff = votes[r][b][0];
                o[b] = v >= 2u ? v : v == 0u ? (diff >= 0 ? 0u : 1u) : (diff <= 0 ? 1u : 0u);
            } else {
                int best = 0, mine = 0;
                unsigned first = v;
#pragma unroll
                for (int c = 0; c < KMAX; ++c) {
                    if (c < classes && votes[r][b][c] > best) best = votes[r][b][c];
                    if (v == (unsigned)c) mine = votes[r][b][c];
                }
#pragma unroll
                for (int c = KMAX - 1; c >= 0; --c)
                    if (c < classes && votes[r][b][c] == best) first = (unsigned)c;
                o[b] = v >= (unsigned)classes || mine == best ? v : first;
            }
        }
        store_px4<ALIGNED>(out + ((size_t)tl.plane * H + gy) * W, gx, W, pack4(o));
    }
}

using Kernel = void (*)(const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*, int, int, int, int, int);

template <int R, int KMAX, int C>
Kernel kernel_of(bool aligned) {
    return aligned ? mask_refine_kernel<R, KMAX, C, true> : mask_refine_kernel<R, KMAX, C, false>;
}
template <int R, int KMAX>
Kernel kernel_of(int channels, bool aligned) {
    return channels == 1   ? kernel_of<R, KMAX, 1>(aligned)
           : channels == 2 ? kernel_of<R, KMAX, 2>(aligned)
           : channels == 3 ? kernel_of<R, KMAX, 3>(aligned)
                           : kernel_of<R, KMAX, 4>(aligned);
}
template <int R>
Kernel kernel_of(int classes, int channels, bool aligned) {
    return classes <= 2 ? kernel_of<R, 2>(channels, aligned) : classes <= 4 ? kernel_of<R, 4>(channels, aligned) : kernel_of<R, 8>(channels, aligned);
}

}  // namespace

extern "C" {

int gsa_mask_refine(void* stream, int32_t n, int32_t H, int32_t W, int32_t channels, int32_t classes, int32_t radius, const uint8_t* img,
                    const uint8_t* mask, const uint8_t* tables, uint8_t* out) {
    if (n == 0) return GSA_OK;
    if (n < 0 || !extent_ok_31(H, W) || channels < 1 || channels > 4 || classes < 2 || classes > kMaxClasses || radius < 1 || radius > kMaxRadius)
        return GSA_ERR_INVALID;
    if (!img || !mask || !tables || !out) return GSA_ERR_INVALID;
    const uint64_t pixels = (uint64_t)n * (uint64_t)H * (uint64_t)W;
    if (ranges_overlap(out, pixels, img, pixels * (uint64_t)channels) || ranges_overlap(out, pixels, mask, pixels) ||
        ranges_overlap(out, pixels, tables, kTableBytes))
        return GSA_ERR_INVALID;
    const TileGrid g = tile_grid(H, W, kTileW, kTileH);
    if (g.per_plane * n >= kMaxWorkgroups) return GSA_ERR_INVALID;     // refused, not split
    const uintptr_t a = reinterpret_cast<uintptr_t>(img), b = reinterpret_cast<uintptr_t>(mask), c = reinterpret_cast<uintptr_t>(out);
    const bool aligned = W % 4 == 0 && ((a | b | c) & 3) == 0;
    const Kernel kernel = radius == 1   ? kernel_of<1>(classes, channels, aligned)
                          : radius == 2 ? kernel_of<2>(classes, channels, aligned)
                          : radius == 3 ? kernel_of<3>(classes, channels, aligned)
                          : radius == 4 ? kernel_of<4>(classes, channels, aligned)
                                        : kernel_of<5>(classes, channels, aligned);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(g.per_plane * n)), dim3(kThreads), 0, (hipStream_t)stream, img, mask, tables, out, (int)H, (int)W,
                       (int)classes, (int)g.tiles_x, (int)g.per_plane);
    return hipGetLastError() == hipSuccess ? GSA_OK : GSA_ERR_HIP;
}

}  // extern "C"
