// gsa_stats.hip -- the pair statistics' kernel (include/gsa_stats.h): per sample the pixel count, bounding
// box and channel sums of each of nine mask slots, the channel sums of squares and the two edge counts, all integers, in one pass
// over an (image, mask) batch in HBM.
//
// Two launches, no workspace.  stats_init_kernel writes every word of every row (0, and W, H, -1, -1 for the boxes: the identity
// of what follows).  pair_stats_kernel gives a workgroup one kTileW x kTileH tile of one plane: a wave owns kWaveRows consecutive
// rows of it, a lane kPix = 4 consecutive pixels of each -- the mask as one dword, the image as C dwords.  A wave loads its rows
// (and the row below them, for the vertical edges) up front and then works on registers.
//
// Nine slots of state without a per-pixel table: a row of a wave is 256 neighbouring pixels and holds one or two classes, so the
// wave first finds the slots PRESENT in the row -- it asks which value its first unaccounted pixel has (one ballot, two
// readlanes), strikes every pixel of that slot with one byte-parallel compare of the mask dword and repeats until none is left --
// and then, for those slots only (a uniform branch per slot), marks the slot's pixels with the same compare and adds them to the
// slot's registers: count by popcount, bytes of a channel by one sum-of-absolute-differences against 0, columns by an OR of the
// marks; the first and last row of a slot are wave-uniform.  At the end of the tile a wave reduces the slots it has seen (xor shuffles for the
// sums; the box columns from a ballot), one lane adds them into the workgroup's 88-word LDS row with LDS atomics, and 87 threads
// of the workgroup send what is not the identity on to the sample's row: 64-bit global atomic add, min and max, at most 87 per
// workgroup and typically about twenty.  Partials are 32-bit: a tile has 8192 pixels, so a count is at most 2^13, a channel sum
// 2^21 and a sum of squares 2^29.  The row is 64-bit.  Integer sums, minima and maxima: the order of the atomics cannot change a bit.
//
// Global access: dword loads when W is a multiple of 4 and the pointers are 4-byte aligned (every generated pair); byte loads with
// per-pixel bounds otherwise.  A pixel outside the image loads as 0 and is masked out of every count.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gsa.h"
#include "../../include/gsa_stats.h"
#include "gsa_plane.h"

namespace {

using namespace gsa::plane;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPix = 4;                         // pixels of a lane in a row: one mask dword
constexpr int kWaveRows = 8;                    // rows of a wave
constexpr int kTileW = 256;                     // 64 lanes x kPix
constexpr int kTileH = 32;                      // kWaves x kWaveRows
constexpr int kSlots = GSA_STATS_SLOTS;

static_assert(kTileW == 64 * kPix && kTileH == kWaves * kWaveRows, "a lane per mask dword, a wave per row group");
static_assert(kTileW * kTileH * 255ll * 255ll < (1ll << 31), "the 32-bit partials hold a tile");

// 0x80 in every byte of x that is zero / that is not zero (exact per byte: no carry crosses a byte)
__device__ __forceinline__ unsigned zero_bytes(unsigned x) { return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu); }
__device__ __forceinline__ unsigned nonzero_bytes(unsigned x) { return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the kPix values of channel c, one per byte, from the 4 * C interleaved bytes in d
template <int C>
__device__ __forceinline__ unsigned channel_bytes(const unsigned (&d)[C ? C : 1], int c) {
    unsigned r = 0;
#pragma unroll
    for (int p = 0; p < kPix; ++p) {
        const int i = p * C + c;
        r |= ((d[i >> 2] >> (8 * (i & 3))) & 255u) << (8 * p);
    }
    return r;
}

__global__ __launch_bounds__(kThreads) void stats_init_kernel(long long* __restrict__ rows, long long words, int H, int W) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= words) return;
    const int f = (int)(i % GSA_STATS_ROW);
    long long v = 0;
    if (f >= GSA_STATS_BOX && f < GSA_STATS_CSUM) {
        const int k = (f - GSA_STATS_BOX) & 3;
        v = k == 0 ? W : k == 1 ? H : -1;
    }
    rows[i] = v;
}

template <int C, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void pair_stats_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask,
                                                              long long* __restrict__ rows, int H, int W, int tiles_x, int tiles_per_plane) {
    constexpr int CD = C ? C : 1;
    __shared__ int part[GSA_STATS_ROW];          // the workgroup's row: sums as 32-bit words, boxes as signed ints
    const Tile t = tile_of(tiles_x, tiles_per_plane);                   // uniform over the workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int xw = t.tile_x * kTileW, x = xw + lane * kPix;             // x < 65536 + 256
    const int yb = t.tile_y * kTileH + wave * kWaveRows;
    const uint8_t* __restrict__ pm = mask + (size_t)t.plane * H * W;   // every sample is a plane of its own
    const uint8_t* __restrict__ pi = C ? img + (size_t)t.plane * H * W * C : nullptr;

    if (threadIdx.x < GSA_STATS_ROW) {
        const int f = threadIdx.x;
        int v = 0;
        if (f >= GSA_STATS_BOX && f < GSA_STATS_CSUM) {
            const int k = (f - GSA_STATS_BOX) & 3;
            v = k == 0 ? W : k == 1 ? H : -1;
        }
        part[f] = v;
    }
    __syncthreads();

    // 0x80 for every pixel of the lane that is inside the image / that has a right-hand neighbour inside the image
    unsigned vmask = 0, hmask = 0;
#pragma unroll
    for (int p = 0; p < kPix; ++p) {
        if (x + p < W) vmask |= 0x80u << (8 * p);
        if (x + p + 1 < W) hmask |= 0x80u << (8 * p);
    }

    // ---- loads: kWaveRows + 1 mask rows, the mask pixel right of the wave's last, kWaveRows image rows
    unsigned m[kWaveRows + 1], right[kWaveRows / 4] = {}, d[kWaveRows][CD];
#pragma unroll
    for (int r = 0; r <= kWaveRows; ++r) {
        const int y = yb + r;
        unsigned v = 0;
        if (y < H) {
            const uint8_t* p = pm + (size_t)y * W;
            if (ALIGNED) {
                if (x < W) v = *reinterpret_cast<const unsigned*>(p + x);
            } else {
#pragma unroll
                for (int b = 0; b < kPix; ++b)
                    if (x + b < W) v |= (unsigned)p[x + b] << (8 * b);
            }
            if (r < kWaveRows && lane == 63 && x + kPix < W) right[r >> 2] |= (unsigned)p[x + kPix] << (8 * (r & 3));
        }
        m[r] = v;
    }
#pragma unroll
    for (int r = 0; r < kWaveRows; ++r) {
        const int y = yb + r;
#pragma unroll
        for (int k = 0; k < CD; ++k) d[r][k] = 0;
        if (C && y < H) {
            const uint8_t* p = pi + ((size_t)y * W + x) * C;
            if (ALIGNED) {
                if (x < W) {
#pragma unroll
                    for (int k = 0; k < C; ++k) d[r][k] = reinterpret_cast<const unsigned*>(p)[k];
                }
            } else {
#pragma unroll
                for (int i = 0; i < kPix * C; ++i)
                    if (x + i / C < W) d[r][i >> 2] |= (unsigned)p[i] << (8 * (i & 3));
            }
        }
    }

    // ---- per-lane state of the nine slots (registers: every index below is a constant after unrolling)
    unsigned cnt[kSlots] = {}, col[kSlots] = {}, cs[kSlots][CD] = {}, sq[CD] = {}, eh = 0, ev = 0;
    int y0[kSlots], y1[kSlots];                 // wave-uniform: first and last row in which the wave met the slot
    unsigned present = 0;                       // wave-uniform: the slots the wave met
#pragma unroll
    for (int s = 0; s < kSlots; ++s) y0[s] = H, y1[s] = -1;

#pragma unroll
    for (int r = 0; r < kWaveRows; ++r) {
        const int y = yb + r;
        if (y >= H) break;                      // uniform
        const unsigned mw = m[r];
        unsigned ch[CD];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            ch[c] = channel_bytes<C>(d[r], c);
            sq[c] = __builtin_amdgcn_udot4(ch[c], ch[c], sq[c], false);
        }
        // edges on the raw values: the pixel to the right is the next byte, the next lane's first byte, or the extra load
        unsigned next = __shfl_down(mw, 1);
        if (lane == 63) next = (right[r >> 2] >> (8 * (r & 3))) & 255u;
        eh += __popc(nonzero_bytes(mw ^ ((mw >> 8) | (next << 24))) & hmask);
        if (y + 1 < H) ev += __popc(nonzero_bytes(mw ^ m[r + 1]) & vmask);

        // which slots does this row of the wave hold?  Ask for the value of the first pixel not yet accounted for, strike every
        // pixel of that slot, repeat: once per slot present, all of it wave-uniform
        unsigned left = vmask, here = 0;        // 0x80 for every pixel not yet struck; the slots met (uniform)
        while (true) {
            const unsigned long long live = __ballot(left != 0);
            if (!live) break;
            const int src = __ffsll((long long)live) - 1;
            const unsigned smw = __builtin_amdgcn_readlane(mw, src), sleft = __builtin_amdgcn_readlane(left, src);
            const unsigned v = (smw >> ((__ffs((int)sleft) - 1) & 24)) & 255u;         // the value of that pixel
            left &= ~(v < 8 ? zero_bytes(mw ^ (v * 0x01010101u)) : nonzero_bytes(mw & 0xf8f8f8f8u));
            here |= 1u << (v < 8 ? v : 8u);
        }
        present |= here;
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            if (!(here & (1u << s))) continue;  // uniform
            const unsigned z = (s < 8 ? zero_bytes(mw ^ (s * 0x01010101u)) : nonzero_bytes(mw & 0xf8f8f8f8u)) & vmask;
            const unsigned full = (z - (z >> 7)) | z;               // 0xff for every pixel of the slot: 0x80 - 0x01 = 0x7f, no borrow
            cnt[s] += __popc(z);
            col[s] |= z;
#pragma unroll
            for (int c = 0; c < C; ++c) cs[s][c] = __builtin_amdgcn_sad_u8(ch[c] & full, 0u, cs[s][c]);
            y0[s] = y0[s] < y ? y0[s] : y;
            y1[s] = y;
        }
    }

    // ---- the wave's sums into the workgroup's row
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        if (!(present & (1u << s))) continue;   // uniform
        const unsigned n = wave_sum(cnt[s]);
        unsigned sum[CD];
#pragma unroll
        for (int c = 0; c < C; ++c) sum[c] = wave_sum(cs[s][c]);
        const unsigned long long has = __ballot(col[s] != 0);           // not 0: the wave met the slot
        const int l0 = __ffsll((long long)has) - 1, l1 = 63 - __clzll((long long)has);
        const unsigned c0 = __builtin_amdgcn_readlane(col[s], l0), c1 = __builtin_amdgcn_readlane(col[s], l1);
        const int x0 = xw + l0 * kPix + ((__ffs((int)c0) - 1) >> 3), x1 = xw + l1 * kPix + ((31 - __clz((int)c1)) >> 3);
        if (lane == 0) {
            atomicAdd(&part[GSA_STATS_COUNT + s], (int)n);
            atomicMin(&part[GSA_STATS_BOX + 4 * s + 0], x0);
            atomicMin(&part[GSA_STATS_BOX + 4 * s + 1], y0[s]);
            atomicMax(&part[GSA_STATS_BOX + 4 * s + 2], x1);
            atomicMax(&part[GSA_STATS_BOX + 4 * s + 3], y1[s]);
#pragma unroll
            for (int c = 0; c < C; ++c) atomicAdd(&part[GSA_STATS_CSUM + 4 * s + c], (int)sum[c]);
        }
    }
    if (yb < H) {                               // uniform
        unsigned tot[CD];
#pragma unroll
        for (int c = 0; c < C; ++c) tot[c] = wave_sum(sq[c]);
        const unsigned th = wave_sum(eh), tv = wave_sum(ev);
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) atomicAdd(&part[GSA_STATS_SQSUM + c], (int)tot[c]);
            atomicAdd(&part[GSA_STATS_EDGE_H], (int)th);
            atomicAdd(&part[GSA_STATS_EDGE_V], (int)tv);
        }
    }
    __syncthreads();

    // ---- the workgroup's row into the sample's: one 64-bit atomic per word that is not the identity
    if (threadIdx.x < GSA_STATS_RESERVED) {
        const int f = threadIdx.x;
        long long* __restrict__ q = rows + (size_t)t.plane * GSA_STATS_ROW + f;
        const int v = part[f];
        if (f >= GSA_STATS_BOX && f < GSA_STATS_CSUM) {
            if (part[GSA_STATS_COUNT + ((f - GSA_STATS_BOX) >> 2)] != 0) {
                if (((f - GSA_STATS_BOX) & 3) < 2)
                    __hip_atomic_fetch_min(q, (long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else
                    __hip_atomic_fetch_max(q, (long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else if (v != 0) {
            __hip_atomic_fetch_add(q, (long long)(unsigned)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

extern "C" {

int gsa_pair_stats(void* stream, int32_t n, int32_t H, int32_t W, int32_t C, const uint8_t* img, const uint8_t* mask, int64_t* rows) {
    if (n < 0 || !extent_ok_31(H, W) || C < 0 || C > GSA_STATS_CHANNELS) return GSA_ERR_INVALID;
    if (n == 0) return GSA_OK;
    if (!mask || !rows || (C > 0 && !img)) return GSA_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    long long* out = reinterpret_cast<long long*>(rows);
    const TileGrid g = tile_grid(H, W, kTileW, kTileH);
    const int tiles_x = (int)g.tiles_x, tiles_per_plane = (int)g.per_plane;             // at most 2^18 + 2^11: H * W < 2^31
    const bool aligned = W % 4 == 0 && ((reinterpret_cast<uintptr_t>(mask) | (C ? reinterpret_cast<uintptr_t>(img) : 0)) & 3) == 0;
    const auto kernel = C == 0   ? (aligned ? pair_stats_kernel<0, true> : pair_stats_kernel<0, false>)
                        : C == 1 ? (aligned ? pair_stats_kernel<1, true> : pair_stats_kernel<1, false>)
                        : C == 2 ? (aligned ? pair_stats_kernel<2, true> : pair_stats_kernel<2, false>)
                        : C == 3 ? (aligned ? pair_stats_kernel<3, true> : pair_stats_kernel<3, false>)
                                 : (aligned ? pair_stats_kernel<4, true> : pair_stats_kernel<4, false>);
    for_each_launch(n, tiles_per_plane, [&](long long first, long long planes) {         // split, not refused
        const uint8_t* im = C ? img + (size_t)first * H * W * C : nullptr;
        const uint8_t* mk = mask + (size_t)first * H * W;
        long long* rw = out + first * GSA_STATS_ROW;
        const unsigned blocks = (unsigned)(planes * tiles_per_plane);
        const long long words = planes * GSA_STATS_ROW;                                 // fewer than 2^24 blocks as well
        hipLaunchKernelGGL(stats_init_kernel, dim3((unsigned)((words + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, rw, words, H, W);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kThreads), 0, s, im, mk, rw, H, W, tiles_x, tiles_per_plane);
    });
    return hipGetLastError() == hipSuccess ? GSA_OK : GSA_ERR_HIP;
}

}  // extern "C"
