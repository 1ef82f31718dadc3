// gsa_photometric.hip -- the photometric augmentation's one kernel (include/gsa_photometric.h): a separable
// 7-tap blur with a reflect-101 border, contrast / brightness / channel shift, counter-based noise and the quantisation back to u8,
// on the NHWC u8 image batch in front of the training stream's warp.
//
// One launch, no workspace.  A row of an NHWC image is W*C bytes in which channel ch of pixel x sits at byte x*C + ch, so a
// horizontal tap k pixels away is the byte k*C further on.  The kernel therefore tiles ROW BYTES, not pixels: a workgroup owns
// kTileB = 256 consecutive bytes of kTileH = 16 rows of one sample -- 64 dword columns, whatever C is -- and a thread owns one dword
// (4 consecutive values) of a row.  Every wave then works on 64 consecutive dwords of one row in every pass: global loads and stores
// are 256 contiguous bytes per wave, LDS reads and writes are consecutive dwords (or consecutive 16-byte slots) and free of bank
// conflicts.  A tile seam may split a pixel (C = 3); nothing depends on where it falls.
//
// Stages: (1) the tile plus a halo of 3 rows and 3*C bytes is staged into LDS as it lies in memory, one unaligned dword load per
// lane, the rows taken from their reflected source row; (2) tiles on the left or right image border mirror the up to 3 pixels
// outside the row inside LDS, so no later stage knows about borders; (3) the horizontal pass reads each thread's 4 + 6*C bytes as
// dwords and writes 4 fp32 sums; (4) the vertical pass reads 10 rows of them (float4) for 4 output rows of one dword column; (5)
// colour, noise and quantisation run in registers and a packed dword is stored.  A sample whose weights are the identity skips (1)
// to (4) and reads its source dwords directly; a sample without noise skips the generator: both switches are uniform over the
// workgroup (the parameter row is read with scalar loads).
//
// The arithmetic is the header's rule, one rounding per operation: this file is built with -ffp-contract=off and uses no fmaf.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gsa.h"
#include "../../include/gsa_photometric.h"
#include "gsa_plane.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileB = 256;                     // row bytes of a workgroup's tile: 64 dword columns = one wave per row
constexpr int kTileH = 16;                      // rows of a tile: 4 per wave
constexpr int kRadius = 3;
constexpr int kTaps = 2 * kRadius + 1;
constexpr int kRows = kTileH + 2 * kRadius;     // 22 staged rows
constexpr int kTileD = kTileB / 4;              // 64
constexpr int kRowsPerThread = kTileH / (kThreads / kTileD);    // 4
constexpr int kMaxChannels = 4;
constexpr unsigned kCounterTag = 0x50480000u;   // "PH" in the counter's second word, the channel in its low bits
constexpr float kInvStd = (float)(1.0 / 295.6010825419961);

static_assert(kThreads == kTileD * (kTileH / kRowsPerThread), "one thread per dword column and group of rows");

__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// acc + the sum of w's four bytes: v_sad_u8 against 0
__device__ __forceinline__ unsigned add_bytes(unsigned w, unsigned acc) { return __builtin_amdgcn_sad_u8(w, 0u, acc); }

struct Row {                // a sample's parameter row, uniform over the workgroup
    float alpha, offset[kMaxChannels], noise_sigma, w[kTaps];
};

// The 4 bytes at byte offset `off` of the image batch (`total` bytes): one unaligned dword load when they all lie inside the batch,
// single bytes (0 for what lies outside) at its two ends.
__device__ __forceinline__ unsigned load4(const uint8_t* __restrict__ img, size_t total, long long off) {
    unsigned v = 0;
    if (off >= 0 && (size_t)off + 4 <= total) {
        __builtin_memcpy(&v, img + off, 4);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (off + k >= 0 && (size_t)(off + k) < total) v |= (unsigned)img[off + k] << (8 * k);
    }
    return v;
}

// Tile-relative byte positions: u = 0 is row byte b0 of the tile's first column, LDS byte t = u + 3*C.  `rem` = the row's bytes from
// b0 on (capped: only "more than the tile and its halo" matters), so the image is u in [-b0, rem).
template <int C>
__global__ __launch_bounds__(kThreads) void photometric_kernel(const uint8_t* __restrict__ img, const float* __restrict__ params,
                                                               uint8_t* __restrict__ out, int H, int W, int tiles_x,
                                                               int tiles_per_sample, unsigned seed_lo, unsigned seed_hi,
                                                               unsigned long long first_index, size_t total) {
    constexpr int kHalo = kRadius * C;                          // bytes
    constexpr int kSrcD = (kTileB + 2 * kHalo + 3) / 4;         // dwords of a staged row
    constexpr int kReadD = (3 + 2 * kHalo) / 4 + 1;             // dwords that hold a thread's 4 + 6*C source bytes
    static_assert(kTileD - 1 + kReadD <= kSrcD, "the horizontal pass stays inside the staged row");
    __shared__ unsigned s_src[kRows * kSrcD];
    __shared__ __attribute__((aligned(16))) float s_h[kRows * kTileB];

    const int sample = blockIdx.x / tiles_per_sample;           // uniform over the workgroup
    const int tile = blockIdx.x - sample * tiles_per_sample;
    const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    const int y0 = tile_y * kTileH;
    const unsigned b0 = (unsigned)tile_x * kTileB;
    const unsigned row_bytes = (unsigned)W * C;
    const int rem = (int)min(row_bytes - b0, (unsigned)(2 * kTileB));
    const size_t sample_off = (size_t)sample * H * row_bytes;

    const float* pr = params + (size_t)sample * GSA_PHOTOMETRIC_ROW;
    Row p;
    p.alpha = pr[0];
#pragma unroll
    for (int k = 0; k < kMaxChannels; ++k) p.offset[k] = pr[1 + k];
    p.noise_sigma = pr[5];
#pragma unroll
    for (int k = 0; k < kTaps; ++k) p.w[k] = pr[6 + k];
    const bool blur = !(p.w[0] == 0.0f && p.w[1] == 0.0f && p.w[2] == 0.0f && p.w[3] == 1.0f && p.w[4] == 0.0f && p.w[5] == 0.0f &&
                        p.w[6] == 0.0f);
    const bool noise = p.noise_sigma != 0.0f;
    const unsigned long long index = first_index + (unsigned long long)sample;

    const int q = threadIdx.x % kTileD;                         // dword column: values u = 4q .. 4q+3
    const int r0 = (threadIdx.x / kTileD) * kRowsPerThread;     // first of this thread's rows in the tile
    float b[kRowsPerThread][4];

    if (blur) {
        // (1) stage
        for (int i = threadIdx.x; i < kRows * kSrcD; i += kThreads) {
            const int j = i / kSrcD, d = i - j * kSrcD;
            const int u = 4 * d - kHalo;
            if ((b0 == 0 && u + 4 <= 0) || u >= rem) continue;  // all 4 bytes outside the row
            int gy = y0 - kRadius + j;
            gy = gy < 0 ? -gy : gy;
            gy = gy > H - 1 ? 2 * (H - 1) - gy : gy;
            gy = gy < 0 ? 0 : gy;                               // rows more than 3 below the image: nobody's taps
            const long long off = (long long)(sample_off + (size_t)gy * row_bytes + b0) + u;
            s_src[i] = load4(img, total, off);                  // bytes outside the row are another row's: step (2) replaces them
        }
        // (2) reflect-101 along the row, where the tile touches a border
        const bool left = b0 == 0, right = rem < kTileB + kHalo;
        if (left || right) {
            __syncthreads();
            uint8_t* sb = reinterpret_cast<uint8_t*>(s_src);
            for (int i = threadIdx.x; i < kRows * 2 * kHalo; i += kThreads) {
                const int j = i / (2 * kHalo), e = i - j * (2 * kHalo);
                const bool rs = e >= kHalo;
                if (rs ? !right : !left) continue;
                const int f = rs ? e - kHalo : e, k = f / C + 1, ch = f - (k - 1) * C;  // pixel k outside the border, channel ch
                const int dst = rs ? rem + (k - 1) * C + ch : -k * C + ch;
                const int src = rs ? rem - (k + 1) * C + ch : k * C + ch;
                const int td = dst + kHalo, ts = src + kHalo;
                if (td < 0 || td >= 4 * kSrcD || ts < 0 || ts >= 4 * kSrcD) continue;      // not in this tile: not this tile's taps
                sb[j * 4 * kSrcD + td] = sb[j * 4 * kSrcD + ts];
            }
        }
        __syncthreads();
        // (3) horizontal: value u = 4q + v reads the LDS bytes 4q + v + k*C, k = 0..6
        for (int i = threadIdx.x; i < kRows * kTileD; i += kThreads) {
            const int j = i / kTileD, d = i - j * kTileD;
            const unsigned* s = s_src + j * kSrcD + d;
            unsigned w[kReadD];
#pragma unroll
            for (int m = 0; m < kReadD; ++m) w[m] = s[m];
            float acc[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
#pragma unroll
                for (int k = 0; k < kTaps; ++k) {
                    const int at = v + k * C;
                    const float px = (float)((w[at / 4] >> (8 * (at % 4))) & 255u);
                    acc[v] = k == 0 ? p.w[0] * px : acc[v] + p.w[k] * px;
                }
            }
            *reinterpret_cast<float4*>(s_h + j * kTileB + 4 * d) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        }
        __syncthreads();
        // (4) vertical: output row r of the tile reads the staged rows r .. r+6
        float4 h[kRowsPerThread + 2 * kRadius];
#pragma unroll
        for (int m = 0; m < kRowsPerThread + 2 * kRadius; ++m) h[m] = *reinterpret_cast<const float4*>(s_h + (r0 + m) * kTileB + 4 * q);
#pragma unroll
        for (int r = 0; r < kRowsPerThread; ++r) {
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
                const float4 t = h[r + k];
                b[r][0] = k == 0 ? p.w[0] * t.x : b[r][0] + p.w[k] * t.x;
                b[r][1] = k == 0 ? p.w[0] * t.y : b[r][1] + p.w[k] * t.y;
                b[r][2] = k == 0 ? p.w[0] * t.z : b[r][2] + p.w[k] * t.z;
                b[r][3] = k == 0 ? p.w[0] * t.w : b[r][3] + p.w[k] * t.w;
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < kRowsPerThread; ++r) {
            const int gy = y0 + r0 + r;
            unsigned w = 0;
            if (gy < H && 4 * q < rem) w = load4(img, total, (long long)(sample_off + (size_t)gy * row_bytes + b0) + 4 * q);
#pragma unroll
            for (int v = 0; v < 4; ++v) b[r][v] = (float)((w >> (8 * v)) & 255u);
        }
    }

    // (5) colour, noise, quantise, store
    if (4 * q >= rem) return;
#pragma unroll
    for (int r = 0; r < kRowsPerThread; ++r) {
        const int gy = y0 + r0 + r;
        if (gy >= H) break;
        unsigned packed = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const unsigned at = b0 + 4 * q + v;                 // row byte = x*C + ch
            const unsigned x = at / C, ch = at - x * C;
            const float o = ch == 0 ? p.offset[0] : ch == 1 ? p.offset[1] : ch == 2 ? p.offset[2] : p.offset[3];
            float val = b[r][v] * p.alpha + o;
            if (noise) {
                unsigned c[4] = {(unsigned)gy * (unsigned)W + x, kCounterTag | ch, (unsigned)index, (unsigned)(index >> 32)};
                philox4x32_10(c, seed_lo, seed_hi);
                const int s = (int)add_bytes(c[0], add_bytes(c[1], add_bytes(c[2], add_bytes(c[3], 0u)))) - 2040;
                const float g = (float)s * kInvStd;
                val = val + p.noise_sigma * g;
            }
            const float qv = floorf(fminf(fmaxf(val, 0.0f), 255.0f) + 0.5f);
            packed |= (unsigned)qv << (8 * v);
        }
        uint8_t* dst = out + sample_off + (size_t)gy * row_bytes + b0 + 4 * q;
        if (4 * q + 4 <= rem) {
            __builtin_memcpy(dst, &packed, 4);                  // one dword store, aligned or not
        } else {
#pragma unroll
            for (int v = 0; v < 3; ++v)
                if (4 * q + v < rem) dst[v] = (uint8_t)(packed >> (8 * v));
        }
    }
}

}  // namespace

extern "C" {

int gsa_photometric(void* stream, int32_t n, int32_t H, int32_t W, int32_t channels, const uint8_t* img, const float* params,
                    uint64_t seed, uint64_t first_index, uint8_t* out) {
    if (n < 0 || channels < 1 || channels > kMaxChannels || H <= kRadius || W <= kRadius) return GSA_ERR_INVALID;
    if ((int64_t)H * W > (1ll << 31) || (int64_t)W * channels > 0x7fffffffll) return GSA_ERR_INVALID;
    if (n == 0) return GSA_OK;
    if (!img || !params || !out || (reinterpret_cast<uintptr_t>(params) & 3)) return GSA_ERR_INVALID;
    const uint64_t row_bytes = (uint64_t)W * channels;
    const uint64_t total = (uint64_t)n * H * row_bytes;
    if (gsa::plane::ranges_overlap(img, total, out, total)) return GSA_ERR_INVALID;     // out is, or overlaps, img
    const int64_t tiles_x = (int64_t)((row_bytes + kTileB - 1) / kTileB);
    const int64_t tiles_per_sample = tiles_x * ((H + kTileH - 1) / kTileH);
    if (tiles_per_sample * n > 0x7fffffffll) return GSA_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(tiles_per_sample * n)), block(kThreads);
    const unsigned lo = (unsigned)seed, hi = (unsigned)(seed >> 32);
#define GSA_PHOTOMETRIC_LAUNCH(C)                                                                                                  \
    hipLaunchKernelGGL(photometric_kernel<C>, grid, block, 0, s, img, params, out, H, W, (int)tiles_x, (int)tiles_per_sample, lo, hi, \
                       (unsigned long long)first_index, (size_t)total)
    switch (channels) {
        case 1: GSA_PHOTOMETRIC_LAUNCH(1); break;
        case 2: GSA_PHOTOMETRIC_LAUNCH(2); break;
        case 3: GSA_PHOTOMETRIC_LAUNCH(3); break;
        default: GSA_PHOTOMETRIC_LAUNCH(4); break;
    }
#undef GSA_PHOTOMETRIC_LAUNCH
    return hipGetLastError() == hipSuccess ? GSA_OK : GSA_ERR_HIP;
}

}  // extern "C"
