// gsa_compare.hip -- the mask agreement's kernel (gsa_compare.h): per sample a 324-bin histogram of
// (band code, target slot, prediction slot) over two u8 masks and, with a radius, their two int16 boundary-distance planes: 6 bytes
// a pixel, one pass over HBM.
//
// Two launches, no workspace.  compare_init_kernel zeroes every word of every row.  mask_compare_kernel gives a workgroup one
// kTileW x kTileH tile of one plane, as pair_stats_kernel does: a wave owns kWaveRows consecutive rows of it, a lane kPix = 4
// consecutive pixels of each -- a dword of each mask, 8 bytes of each dist2 plane.  A wave loads its rows up front and then works on
// registers.
//
// 324 bins, counted per LANE and added to the workgroup's 324-word LDS row with LDS atomics.  A lane packs its pixels' keys
// byte-parallel -- code = 9 * slot(target) + slot(pred) <= 80 in one dword, the band code f in another -- and counts its pixels of
// one key together: one byte-parallel compare against the key of its first uncounted pixel and a popcount, at most four times a row
// and once where the four pixels agree.  Equal keys down the lane's rows add up in a register; the LDS atomic goes out when the key
// changes and at the end, so a lane inside a uniform region issues ONE for its 32 pixels.  At the end the 324 words go to the
// sample's row, those that are not zero, by 64-bit global atomic add.
// No wave-level step: the first version found the bins present in a wave's row by ballot and readlane and counted each by popcount,
// as pair_stats_kernel does, to keep 64 lanes off one LDS address.  Measured, every such turn cost more than
// the contention it saved -- a turn is a round trip through the scalar unit -- on smooth masks, ragged ones and noise alike, and
// what the contention does cost is met by the two merges above.
// Correctness rests on the rule, not on the masks being smooth: integer sums know no order.
//
// Global access: dword and 8-byte loads when W is a multiple of 4 and the pointers are aligned for it (4 bytes the masks, 8 the dist2
// planes); byte and int16 loads with per-pixel bounds otherwise.  A pixel outside the image is in no bin.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gsa.h"
#include "gsa_compare.h"
#include "gsa_plane.h"

namespace {

using namespace gsa::plane;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPix = 4;                         // pixels of a lane in a row: one dword of each mask
constexpr int kWaveRows = 8;                    // rows of a wave
constexpr int kTileW = 256;                     // 64 lanes x kPix
constexpr int kTileH = 32;                      // kWaves x kWaveRows
constexpr int kSlots = GSA_COMPARE_SLOTS;
constexpr int kCodes = kSlots * kSlots;         // 81 (target slot, prediction slot) pairs of one band code
constexpr int kRow = GSA_COMPARE_ROW;

static_assert(kTileW == 64 * kPix && kTileH == kWaves * kWaveRows, "a lane per mask dword, a wave per row group");
static_assert(kRow == GSA_COMPARE_BANDS * kCodes && kCodes <= 128, "a code fits the low seven bits of a byte");
static_assert(kRow <= 2 * kThreads, "compare_init_kernel takes at most two workgroups a plane (gsa_mask_compare's split)");

// 0x80 in every byte of x that is zero / that is not zero (exact per byte: no carry crosses a byte)
__device__ __forceinline__ unsigned zero_bytes(unsigned x) { return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu); }
__device__ __forceinline__ unsigned nonzero_bytes(unsigned x) { return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }

// slot(v) = min(v, 8) of every byte
__device__ __forceinline__ unsigned slot_bytes(unsigned w) {
    const unsigned hi = nonzero_bytes(w & 0xf8f8f8f8u);                 // 0x80 where v >= 8
    const unsigned full = (hi - (hi >> 7)) | hi;                        // 0xff there: 0x80 - 0x01 = 0x7f, no borrow
    return (w & ~full) | (0x08080808u & full);
}

// in[p] = 1 for every pixel p of the lane inside [0, W) whose dist2 is at most r2, one per byte
template <bool ALIGNED>
__device__ __forceinline__ unsigned band_bytes(const int16_t* row, int gx, int W, int r2) {
    unsigned v = 0;
    if (ALIGNED) {
        if (gx < W) {
            const uint2 d = *reinterpret_cast<const uint2*>(row + gx);
            v = (unsigned)((int)(int16_t)(d.x & 0xffffu) <= r2) | (unsigned)((int)(int16_t)(d.x >> 16) <= r2) << 8 |
                (unsigned)((int)(int16_t)(d.y & 0xffffu) <= r2) << 16 | (unsigned)((int)(int16_t)(d.y >> 16) <= r2) << 24;
        }
    } else {
#pragma unroll
        for (int b = 0; b < kPix; ++b)
            if (gx + b < W) v |= (unsigned)((int)row[gx + b] <= r2) << (8 * b);
    }
    return v;
}

__global__ __launch_bounds__(kThreads) void compare_init_kernel(long long* __restrict__ rows, long long words) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < words) rows[i] = 0;
}

template <bool BANDS, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void mask_compare_kernel(const uint8_t* __restrict__ target, const uint8_t* __restrict__ pred,
                                                                const int16_t* __restrict__ tdist, const int16_t* __restrict__ pdist,
                                                                long long* __restrict__ rows, int H, int W, int r2, int tiles_x,
                                                                int tiles_per_plane) {
    __shared__ unsigned part[kRow];             // the workgroup's row
    const Tile t = tile_of(tiles_x, tiles_per_plane);                   // uniform over the workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = t.tile_x * kTileW + lane * kPix;                      // x < 65536 + 256
    const int yb = t.tile_y * kTileH + wave * kWaveRows;
    const size_t plane = (size_t)t.plane * H * W;                       // every sample is a plane of its own
    const uint8_t* __restrict__ pt = target + plane;
    const uint8_t* __restrict__ pp = pred + plane;
    const int16_t* __restrict__ ptd = BANDS ? tdist + plane : nullptr;
    const int16_t* __restrict__ ppd = BANDS ? pdist + plane : nullptr;

    for (int f = threadIdx.x; f < kRow; f += kThreads) part[f] = 0;
    __syncthreads();

    unsigned vmask = 0;                         // 0x80 for every pixel of the lane that is inside the image
#pragma unroll
    for (int p = 0; p < kPix; ++p)
        if (x + p < W) vmask |= 0x80u << (8 * p);

    // ---- loads: kWaveRows rows of both masks and, with bands, of both dist2 planes; keys per byte
    unsigned code[kWaveRows], band[kWaveRows];
#pragma unroll
    for (int r = 0; r < kWaveRows; ++r) {
        const int y = yb + r;
        code[r] = band[r] = 0;
        if (y < H) {
            const size_t o = (size_t)y * W;
            const unsigned st = slot_bytes(load_px4<ALIGNED>(pt + o, x, W)), sp = slot_bytes(load_px4<ALIGNED>(pp + o, x, W));
            code[r] = (st << 3) + st + sp;      // 9 * st + sp <= 80 in every byte: no carry crosses a byte
            if (BANDS) band[r] = band_bytes<ALIGNED>(ptd + o, x, W, r2) + 2 * band_bytes<ALIGNED>(ppd + o, x, W, r2);
        }
    }

    // ---- the bins of each row: a lane's pixels of one key go together, and so do its runs of one key down the rows
    int run_bin = -1;                           // per lane
    unsigned run = 0;
#pragma unroll
    for (int r = 0; r < kWaveRows; ++r) {
        if (yb + r >= H) break;                 // uniform
        const unsigned c = code[r], b = band[r];
        unsigned left = vmask;                  // 0x80 for every pixel of the lane not yet counted
#pragma unroll
        for (int p = 0; p < kPix; ++p) {
            if (!(left & (0x80u << (8 * p)))) continue;
            const unsigned vc = byte_of(c, p), vb = BANDS ? byte_of(b, p) : 0u;
            const unsigned z = zero_bytes((c ^ (vc * 0x01010101u)) | (BANDS ? b ^ (vb * 0x01010101u) : 0u)) & left;    // 0x80 for every pixel of this key
            left &= ~z;
            const int bin = (int)(vb * kCodes + vc);
            if (bin != run_bin) {
                if (run) atomicAdd(&part[run_bin], run);
                run_bin = bin;
                run = 0;
            }
            run += (unsigned)__popc(z);
        }
    }
    if (run) atomicAdd(&part[run_bin], run);
    __syncthreads();

    // ---- the workgroup's row into the sample's: one 64-bit atomic per word that is not zero
    for (int f = threadIdx.x; f < kRow; f += kThreads) {
        const unsigned v = part[f];
        if (v) __hip_atomic_fetch_add(rows + (size_t)t.plane * kRow + f, (long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

extern "C" {

int gsa_mask_compare(void* stream, int32_t n, int32_t H, int32_t W, int32_t radius, const uint8_t* target, const uint8_t* pred,
                     const int16_t* target_dist2, const int16_t* pred_dist2, int64_t* rows) {
    if (n == 0) return GSA_OK;
    if (n < 0 || !extent_ok_31(H, W) || radius < 0 || radius > GSA_COMPARE_MAX_RADIUS) return GSA_ERR_INVALID;
    if (!target || !pred || !rows) return GSA_ERR_INVALID;
    const bool bands = radius > 0;
    if (bands ? (!target_dist2 || !pred_dist2) : (target_dist2 || pred_dist2)) return GSA_ERR_INVALID;
    const uintptr_t dist_bits = reinterpret_cast<uintptr_t>(target_dist2) | reinterpret_cast<uintptr_t>(pred_dist2);
    if ((dist_bits & 1) || (reinterpret_cast<uintptr_t>(rows) & 7)) return GSA_ERR_INVALID;
    const uint64_t pixels = (uint64_t)n * H * W, row_bytes = (uint64_t)n * kRow * sizeof(int64_t);
    if (ranges_overlap(rows, row_bytes, target, pixels) || ranges_overlap(rows, row_bytes, pred, pixels)) return GSA_ERR_INVALID;
    if (bands && (ranges_overlap(rows, row_bytes, target_dist2, 2 * pixels) || ranges_overlap(rows, row_bytes, pred_dist2, 2 * pixels)))
        return GSA_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    long long* out = reinterpret_cast<long long*>(rows);
    const TileGrid g = tile_grid(H, W, kTileW, kTileH);
    const int tiles_x = (int)g.tiles_x, tiles_per_plane = (int)g.per_plane;             // at most 2^18 + 2^11: H * W < 2^31
    const uintptr_t mask_bits = reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(pred);
    const bool aligned = W % 4 == 0 && (mask_bits & 3) == 0 && (dist_bits & 7) == 0;
    const auto kernel = bands ? (aligned ? mask_compare_kernel<true, true> : mask_compare_kernel<true, false>)
                              : (aligned ? mask_compare_kernel<false, true> : mask_compare_kernel<false, false>);
    // split, not refused; at least two workgroups a plane are counted, so that the init launch stays below 2^24 workgroups as well
    for_each_launch(n, tiles_per_plane > 2 ? tiles_per_plane : 2, [&](long long first, long long planes) {
        const size_t o = (size_t)first * H * W;
        long long* rw = out + first * kRow;
        const unsigned blocks = (unsigned)(planes * tiles_per_plane);
        const long long words = planes * kRow;
        hipLaunchKernelGGL(compare_init_kernel, dim3((unsigned)((words + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, rw, words);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kThreads), 0, s, target + o, pred + o, bands ? target_dist2 + o : nullptr,
                           bands ? pred_dist2 + o : nullptr, rw, H, W, radius * radius, tiles_x, tiles_per_plane);
    });
    return hipGetLastError() == hipSuccess ? GSA_OK : GSA_ERR_HIP;
}

}  // extern "C"
