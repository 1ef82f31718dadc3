// gsa_mask.hip -- the mask clean-up's one kernel (include/gsa_mask.h): a 5x5 close followed by a 5x5 open of
// every (H, W) u8 plane, morph = D(E(E(D(m)))), taps outside the image skipped at every stage.
//
// One launch, no workspace.  A workgroup owns a kTileW x kTileH tile of output pixels, stages it with an 8-px apron (2 + 4 + 2) in
// LDS and runs THREE separable stages on it -- D5, E9, D5: two skipped-border 5x5 erosions are one skipped-border 9x9 erosion, the
// union of the clipped windows -- each as a row pass and a column pass between two LDS images.  Every stage is valid on a region
// that shrinks by its radius; what lies outside that region is computed from filler and never read by a pixel that counts.
//
// "Skipped" = the outside of the image is the stage's identity (0 for a dilation, 255 for an erosion) on that stage's own input:
// the load writes 0 there, and the column pass that ends a stage writes the NEXT stage's identity at every position outside the
// image, so a pixel next to the border never sees a value that an earlier stage grew or shrank into the outside.
//
// Data layout: one byte per pixel, a thread works on dwords (4 pixels of a row).  A row pass reads the three dwords around its own
// (12 bytes: exactly the reach of radius 4) and writes one; a column pass owns 4 rows of one dword column, reads the 4 + 2r dwords
// above and below once and writes four.  Both reduce "4 + 2r values in, 4 out" with shared partial results (7 max/min for r = 2,
// 9 for r = 4, three-operand instructions) instead of 4 * (2r + 1).  The kernel is bound by these byte-wise VALU operations and
// the LDS passes, not by its 2 bytes per pixel of HBM traffic (DESIGN.md section 14 has the numbers).
//
// Global access: dword loads and stores when W is a multiple of 4 and both pointers are 4-byte aligned (every generated mask);
// byte access with per-pixel bounds otherwise (any H, W in 1..65535 is accepted).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gsa.h"
#include "../../include/gsa_mask.h"
#include "gsa_plane.h"

namespace {

using namespace gsa::plane;

constexpr int kThreads = 256;
constexpr int kTileW = 64;                      // output pixels of a workgroup: 64 x 64.  With the 8-px apron it stages 80 x 80 (1.56 x
constexpr int kTileH = 64;                      // the tile; 32 x 32 would stage 2.25 x) in 2 x 7 KB of LDS: 8+ workgroups per CU
constexpr int kApron = 8;                       // 2 (D5) + 4 (E9) + 2 (D5)
constexpr int kRows = kTileH + 2 * kApron;      // 80 staged rows
constexpr int kTileD = kTileW / 4;              // 16 dwords of a tile row
constexpr int kFirstD = 1 + kApron / 4;         // 3: dword column of the tile's first pixel -- one filler column, two of apron
constexpr int kCols = kTileD + 2 * kFirstD;     // 22 dword columns: filler, apron, tile, apron, filler

static_assert(kTileW % 4 == 0 && kTileH % 4 == 0 && kApron % 4 == 0, "dword columns, 4-row blocks");

template <bool MX>
__device__ __forceinline__ unsigned op2(unsigned a, unsigned b) { return MX ? (a > b ? a : b) : (a < b ? a : b); }
template <bool MX>
__device__ __forceinline__ unsigned op3(unsigned a, unsigned b, unsigned c) { return op2<MX>(op2<MX>(a, b), c); }     // v_max3_u32 / v_min3_u32

// o[i] = max (MX) or min of v[i .. i + 2R], i = 0..3: four windows of 2R + 1 over 4 + 2R consecutive values.
template <int R, bool MX>
__device__ __forceinline__ void window4(const unsigned (&v)[4 + 2 * R], unsigned (&o)[4]) {
    static_assert(R == 2 || R == 4, "5- and 9-tap windows");
    if constexpr (R == 2) {
        const unsigned c = op2<MX>(v[3], v[4]), lo = op2<MX>(v[1], v[2]), hi = op2<MX>(v[5], v[6]);
        o[0] = op3<MX>(v[0], lo, c);
        o[1] = op3<MX>(lo, c, v[5]);
        o[2] = op3<MX>(v[2], c, hi);
        o[3] = op3<MX>(c, hi, v[7]);
    } else {
        const unsigned c = op2<MX>(op3<MX>(v[3], v[4], v[5]), op3<MX>(v[6], v[7], v[8]));
        const unsigned lo = op2<MX>(v[1], v[2]), hi = op2<MX>(v[9], v[10]);
        o[0] = op3<MX>(v[0], lo, c);
        o[1] = op3<MX>(lo, c, v[9]);
        o[2] = op3<MX>(v[2], c, hi);
        o[3] = op3<MX>(c, hi, v[11]);
    }
}

// 0xff in every byte of the dword at (gy, gx .. gx+3) that lies outside the H x W image.
__device__ __forceinline__ unsigned outside_mask(int gy, int gx, int H, int W) {
    if ((unsigned)gy >= (unsigned)H) return 0xffffffffu;
    unsigned m = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if ((unsigned)(gx + b) >= (unsigned)W) m |= 0xffu << (8 * b);
    return m;
}

// Row pass of radius R over rows [row_lo, row_hi) and dword columns [d_lo, d_hi) of the LDS image: dst = max / min along x of src.
// Reads the columns d_lo - 1 .. d_hi of src.
template <int R, bool MX>
__device__ __forceinline__ void row_pass(const unsigned* __restrict__ src, unsigned* __restrict__ dst, int row_lo, int row_hi,
                                         int d_lo, int d_hi) {
    const int nd = d_hi - d_lo, items = (row_hi - row_lo) * nd;
    for (int i = threadIdx.x; i < items; i += kThreads) {
        const int j = row_lo + i / nd, d = d_lo + i % nd;
        const unsigned* p = src + j * kCols + d;
        const unsigned w[3] = {p[-1], p[0], p[1]};
        unsigned v[4 + 2 * R], o[4];
#pragma unroll
        for (int k = 0; k < 4 + 2 * R; ++k) {
            const int at = k + (4 - R);         // byte k of the window row = byte `at` of the 12 loaded (pixel 0 of the dword = byte 4)
            v[k] = byte_of(w[at / 4], at % 4);
        }
        window4<R, MX>(v, o);
        dst[j * kCols + d] = pack4(o);
    }
}

// Column pass of radius R over rows [row_lo, row_hi) (a multiple of 4 rows) and dword columns [d_lo, d_hi): max / min along y of
// src, reading its rows row_lo - R .. row_hi + R - 1.  The result goes to the LDS image `dst` with the NEXT stage's identity
// (`next_identity`: 0 or 255) at every position outside the image, or -- LAST -- to the output plane, inside the image only.
template <int R, bool MX, bool LAST, bool ALIGNED>
__device__ __forceinline__ void col_pass(const unsigned* __restrict__ src, unsigned* __restrict__ dst, int row_lo, int row_hi,
                                         int d_lo, int d_hi, int y0, int x0, int H, int W, unsigned next_identity,
                                         uint8_t* __restrict__ plane_out) {
    const int nd = d_hi - d_lo, items = ((row_hi - row_lo) / 4) * nd;
    for (int i = threadIdx.x; i < items; i += kThreads) {
        const int j0 = row_lo + 4 * (i / nd), d = d_lo + i % nd;
        unsigned w[4 + 2 * R];
#pragma unroll
        for (int k = 0; k < 4 + 2 * R; ++k) w[k] = src[(j0 - R + k) * kCols + d];
        unsigned res[4] = {0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            unsigned v[4 + 2 * R], o[4];
#pragma unroll
            for (int k = 0; k < 4 + 2 * R; ++k) v[k] = byte_of(w[k], b);
            window4<R, MX>(v, o);
#pragma unroll
            for (int r = 0; r < 4; ++r) res[r] |= o[r] << (8 * b);
        }
        const int gx = x0 + 4 * (d - kFirstD);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gy = y0 - kApron + j0 + r;
            if (!LAST) {
                const unsigned m = outside_mask(gy, gx, H, W);
                dst[(j0 + r) * kCols + d] = next_identity ? (res[r] | m) : (res[r] & ~m);
            } else if (gy < H && gx < W) {      // the tile's own pixels: gy, gx >= 0
                store_px4<ALIGNED>(plane_out + (size_t)gy * W, gx, W, res[r]);
            }
        }
    }
}

template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void mask_morph_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ out, int H, int W,
                                                              int tiles_x, int tiles_per_plane) {
    __shared__ unsigned lds_a[kRows * kCols], lds_b[kRows * kCols];
    const Tile t = tile_of(tiles_x, tiles_per_plane);                   // uniform over the workgroup
    const int y0 = t.tile_y * kTileH, x0 = t.tile_x * kTileW;
    const uint8_t* __restrict__ plane_in = mask + (size_t)t.plane * H * W;  // every image is a plane of its own: no tap leaves it
    uint8_t* __restrict__ plane_out = out + (size_t)t.plane * H * W;

    // stage the tile and its apron; 0 (the first dilation's identity) outside the image and in the two filler columns
    for (int i = threadIdx.x; i < kRows * kCols; i += kThreads) {
        const int j = i / kCols, d = i % kCols;
        const int gy = y0 - kApron + j, gx = x0 + 4 * (d - kFirstD);
        unsigned v = 0;
        if (d != 0 && d != kCols - 1 && (unsigned)gy < (unsigned)H) v = load_px4<ALIGNED>(plane_in + (size_t)gy * W, gx, W);
        lds_a[i] = v;
    }
    __syncthreads();
    // D5: valid 2 px inside the staged region
    row_pass<2, true>(lds_a, lds_b, 0, kRows, 1, kCols - 1);
    __syncthreads();
    col_pass<2, true, false, ALIGNED>(lds_b, lds_a, 2, kRows - 2, 1, kCols - 1, y0, x0, H, W, 255u, nullptr);
    __syncthreads();
    // E9 = E5 of E5: valid 6 px inside
    row_pass<4, false>(lds_a, lds_b, 2, kRows - 2, 1, kCols - 1);
    __syncthreads();
    col_pass<4, false, false, ALIGNED>(lds_b, lds_a, 6, kRows - 6, 1, kCols - 1, y0, x0, H, W, 0u, nullptr);
    __syncthreads();
    // D5: valid on the tile
    row_pass<2, true>(lds_a, lds_b, 6, kRows - 6, kFirstD, kFirstD + kTileD);
    __syncthreads();
    col_pass<2, true, true, ALIGNED>(lds_b, nullptr, kApron, kRows - kApron, kFirstD, kFirstD + kTileD, y0, x0, H, W, 0u, plane_out);
}

}  // namespace

extern "C" {

int gsa_mask_morph(void* stream, int32_t n, int32_t H, int32_t W, const uint8_t* mask, uint8_t* out) {
    if (n < 0 || !extent_ok(H, W)) return GSA_ERR_INVALID;              // alone among the plane entries: H * W may reach 2^31
    if (n == 0) return GSA_OK;
    if (!mask || !out) return GSA_ERR_INVALID;
    const uint64_t bytes = (uint64_t)n * (uint64_t)H * (uint64_t)W;
    if (ranges_overlap(mask, bytes, out, bytes)) return GSA_ERR_INVALID;
    const TileGrid g = tile_grid(H, W, kTileW, kTileH);
    const long long tiles_per_plane = g.per_plane;
    if (tiles_per_plane * n >= kMaxWorkgroups) return GSA_ERR_INVALID;  // refused, not split
    const bool aligned = W % 4 == 0 && ((reinterpret_cast<uintptr_t>(mask) | reinterpret_cast<uintptr_t>(out)) & 3) == 0;
    const dim3 grid((unsigned)(tiles_per_plane * n)), block(kThreads);
    const auto kernel = aligned ? mask_morph_kernel<true> : mask_morph_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, mask, out, H, W, (int)g.tiles_x, (int)tiles_per_plane);
    return hipGetLastError() == hipSuccess ? GSA_OK : GSA_ERR_HIP;
}

}  // extern "C"
