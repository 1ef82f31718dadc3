// gsa_augment.hip -- the training stream's one kernel (include/gsa_augment.h): per sample one inverse affine
// map, bilinear taps with a constant border from the NHWC u8 image, the nearest mask value or the ignore label, per-channel scale
// and bias, NCHW fp32 / bf16 out.  Memory bound: one thread owns 4 consecutive output pixels of one row, so every channel plane is
// written with one 16-byte store per lane (8 bytes in bf16) and the labels with one packed dword; the sample's matrix is uniform
// over the workgroup (scalar loads); the 16 taps of a thread are gathered from the NHWC u8 source, which neighbouring lanes share
// in cache, as 8 unaligned 8-byte windows (two adjacent taps, all channels, each).
//
// The arithmetic is the header's rule, one rounding per operation: this file is built with -ffp-contract=off and uses no fmaf.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gsa.h"
#include "../../include/gsa_augment.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 4;              // output pixels per thread
constexpr int kMaxChannels = 4;
constexpr int kMaxExtent = 1 << 24;  // every pixel index is an exact float

struct ChannelAffine {
    float scale[kMaxChannels];
    float bias[kMaxChannels];
};

__device__ __forceinline__ unsigned short bf16_rne(float v) {
    unsigned u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);     // NaN stays a (quiet) NaN
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// Clamp a floor value to [0, hi] as a float, then convert: the address is in bounds whatever the coordinate (NaN included --
// fmaxf / fminf return the other operand).  Whether the tap counts is decided separately, on the unclamped float.
__device__ __forceinline__ int clamp_index(float v, float hi) { return (int)fminf(fmaxf(v, 0.0f), hi); }

// The 8 bytes that start at byte `off` of the image batch (`total` bytes in all): the two horizontally adjacent taps of a row,
// all channels (2 * C <= 8 bytes), in ONE load instead of 2 * C byte loads -- the kernel is bound by the number of cache lines its
// gathers touch per instruction, not by bytes.  The window is moved back where it would pass the end of the batch, and the bytes
// shifted down again, so nothing outside the buffer is read; bytes past the wanted ones are other pixels' and are ignored.
__device__ __forceinline__ unsigned long long load_window(const uint8_t* __restrict__ img, size_t total, size_t off) {
    unsigned long long v = 0;
    if (total >= 8) {
        const size_t base = off + 8 <= total ? off : total - 8;
        __builtin_memcpy(&v, img + base, 8);        // unaligned: one global_load_dwordx2
        return v >> (8 * (unsigned)(off - base));
    }
    for (unsigned k = 0; k < 8; ++k)                // a batch smaller than one window
        if (off + k < total) v |= (unsigned long long)img[off + k] << (8 * k);
    return v;
}

// Workgroup = a tile of kTileW x kTileH output pixels: 16 lanes x 4 pixels wide, 16 rows high (a wave covers 64 x 4 pixels, so a
// gather instruction of a rotated sample touches a few source rows instead of the ~66 a 256-pixel row segment crosses at 15
// degrees), and every lane still stores 16 contiguous bytes per channel plane, 256 per row of the wave.
constexpr int kLanesX = 16;
constexpr int kTileW = kLanesX * kPix;          // 64
constexpr int kTileH = kThreads / kLanesX;      // 16

template <bool BF>
__global__ __launch_bounds__(kThreads) void augment_pairs_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask,
                                                                 const float* __restrict__ matrices, ChannelAffine ca, int H, int W,
                                                                 int C, int oh, int ow, int tiles_x, int tiles_per_sample, size_t total,
                                                                 int ignore_label, void* __restrict__ image_out,
                                                                 uint8_t* __restrict__ label_out) {
    const int sample = blockIdx.x / tiles_per_sample;                   // uniform over the workgroup
    const int tile = blockIdx.x - sample * tiles_per_sample;
    const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    const int X0 = tile_x * kTileW + (threadIdx.x % kLanesX) * kPix;
    const int Y = tile_y * kTileH + threadIdx.x / kLanesX;
    if (X0 >= ow || Y >= oh) return;                                    // ow is a multiple of kPix: a thread's 4 pixels are in or out together

    const float* m = matrices + (size_t)sample * 6;
    const float a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5];
    const float wmax = (float)(W - 1), hmax = (float)(H - 1);
    const size_t src = (size_t)sample * H * W * C;                      // byte offset of the sample in the image batch
    const uint8_t* msk = mask + (size_t)sample * H * W;

    unsigned long long win[kPix][2];    // per source row (y0, y0+1): the taps x0 and x0+1, all channels
    unsigned shift1[kPix];              // bit position of tap x0+1 inside a window (0 where both clamp to one column)
    unsigned inside[kPix];              // bit k: tap k (00, 01, 10, 11) lies inside the image
    float fx[kPix], fy[kPix];
    unsigned labels = 0;
    const float Yf = (float)Y;
#pragma unroll
    for (int p = 0; p < kPix; ++p) {
        const float Xf = (float)(X0 + p);
        const float xs = (a * Xf + b * Yf) + c;
        const float ys = (d * Xf + e * Yf) + f;
        const float x0 = floorf(xs), y0 = floorf(ys);
        fx[p] = xs - x0;
        fy[p] = ys - y0;
        const float x1 = x0 + 1.0f, y1 = y0 + 1.0f;
        const bool ix0 = x0 >= 0.0f && x0 <= wmax, ix1 = x1 >= 0.0f && x1 <= wmax;
        const bool iy0 = y0 >= 0.0f && y0 <= hmax, iy1 = y1 >= 0.0f && y1 <= hmax;
        inside[p] = (unsigned)(iy0 && ix0) | ((unsigned)(iy0 && ix1) << 1) | ((unsigned)(iy1 && ix0) << 2) | ((unsigned)(iy1 && ix1) << 3);
        const int cx0 = clamp_index(x0, wmax), cx1 = clamp_index(x1, wmax);     // cx1 is cx0 or cx0 + 1
        const int cy0 = clamp_index(y0, hmax), cy1 = clamp_index(y1, hmax);
        shift1[p] = (unsigned)(cx1 - cx0) * C * 8;
        win[p][0] = load_window(img, total, src + (size_t)(cy0 * W + cx0) * C);
        win[p][1] = load_window(img, total, src + (size_t)(cy1 * W + cx0) * C);
        const float xn = floorf(xs + 0.5f), yn = floorf(ys + 0.5f);
        const bool in = xn >= 0.0f && xn <= wmax && yn >= 0.0f && yn <= hmax;
        const unsigned got = msk[clamp_index(yn, hmax) * W + clamp_index(xn, wmax)];
        labels |= (in ? got : (unsigned)ignore_label) << (8 * p);
    }
    const size_t plane = (size_t)oh * ow;
    const size_t at = (size_t)Y * ow + X0;
    *reinterpret_cast<unsigned*>(label_out + (size_t)sample * plane + at) = labels;

    for (int ch = 0; ch < C; ++ch) {
        const float sc = ca.scale[ch], bi = ca.bias[ch];
        float v[kPix];
#pragma unroll
        for (int p = 0; p < kPix; ++p) {
            const unsigned s0 = 8 * ch, s1 = shift1[p] + 8 * ch;
            const float p00 = (inside[p] & 1u) ? (float)(unsigned)((win[p][0] >> s0) & 255u) : 0.0f;
            const float p01 = (inside[p] & 2u) ? (float)(unsigned)((win[p][0] >> s1) & 255u) : 0.0f;
            const float p10 = (inside[p] & 4u) ? (float)(unsigned)((win[p][1] >> s0) & 255u) : 0.0f;
            const float p11 = (inside[p] & 8u) ? (float)(unsigned)((win[p][1] >> s1) & 255u) : 0.0f;
            const float top = p00 + fx[p] * (p01 - p00);
            const float bot = p10 + fx[p] * (p11 - p10);
            v[p] = (top + fy[p] * (bot - top)) * sc + bi;
        }
        const size_t o = ((size_t)sample * C + ch) * plane + at;
        if (BF) {
            ushort4 q;
            q.x = bf16_rne(v[0]);
            q.y = bf16_rne(v[1]);
            q.z = bf16_rne(v[2]);
            q.w = bf16_rne(v[3]);
            *reinterpret_cast<ushort4*>(static_cast<unsigned short*>(image_out) + o) = q;
        } else {
            *reinterpret_cast<float4*>(static_cast<float*>(image_out) + o) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

}  // namespace

extern "C" {

int gsa_augment_pairs(void* stream, int32_t n, int32_t H, int32_t W, int32_t channels, const uint8_t* img, const uint8_t* mask,
                      const float* matrices, const float* scale, const float* bias, int32_t out_h, int32_t out_w, int32_t out_bf16,
                      int32_t ignore_label, void* image_out, uint8_t* label_out) {
    if (n < 0 || H < 1 || W < 1 || H > kMaxExtent || W > kMaxExtent || channels < 1 || channels > kMaxChannels) return GSA_ERR_INVALID;
    if (out_h < kPix || out_w < kPix || out_h % kPix || out_w % kPix || (out_bf16 != 0 && out_bf16 != 1)) return GSA_ERR_INVALID;
    if (ignore_label < 0 || ignore_label > 255) return GSA_ERR_INVALID;
    if (!img || !mask || !matrices || !scale || !bias || !image_out || !label_out) return GSA_ERR_INVALID;
    // offsets inside one sample are 32-bit in the kernel
    if ((int64_t)H * W * channels > 0x7fffffffll || (int64_t)out_h * out_w > 0x7fffffffll) return GSA_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(image_out) & (out_bf16 ? 7 : 15)) || (reinterpret_cast<uintptr_t>(label_out) & 3)) return GSA_ERR_INVALID;
    if (n == 0) return GSA_OK;
    const int64_t tiles_x = (out_w + kTileW - 1) / kTileW;
    const int64_t tiles_per_sample = tiles_x * ((out_h + kTileH - 1) / kTileH);
    if (tiles_per_sample * n > 0x7fffffffll) return GSA_ERR_INVALID;
    const size_t total = (size_t)n * H * W * channels;
    ChannelAffine ca = {};
    for (int ch = 0; ch < channels; ++ch) {
        ca.scale[ch] = scale[ch];
        ca.bias[ch] = bias[ch];
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(tiles_per_sample * n)), block(kThreads);
    if (out_bf16)
        hipLaunchKernelGGL(augment_pairs_kernel<true>, grid, block, 0, s, img, mask, matrices, ca, H, W, channels, out_h, out_w,
                           (int)tiles_x, (int)tiles_per_sample, total, ignore_label, image_out, label_out);
    else
        hipLaunchKernelGGL(augment_pairs_kernel<false>, grid, block, 0, s, img, mask, matrices, ca, H, W, channels, out_h, out_w,
                           (int)tiles_x, (int)tiles_per_sample, total, ignore_label, image_out, label_out);
    return hipGetLastError() == hipSuccess ? GSA_OK : GSA_ERR_HIP;
}

}  // extern "C"
