// gsa_scores.hip -- the score histograms' kernels (gsa_scores.h): per sample and class two 1024-bin histograms
// of the quantised logit margin z_c - max_{j != c} z_j, over the pixels of the class and over the others: 4 * classes + 1 bytes a
// pixel, one pass over HBM.
//
// Two launches, no workspace.  scores_init_kernel zeroes every word of every row.  score_histogram_kernel<K, ALIGNED> has
// (min(ceil(HW / GSA_SCORE_STRETCH), GSA_SCORE_MAX_BLOCKS), n) workgroups of 256 threads; a workgroup strides over the pixels of
// ONE sample, a lane four consecutive pixels a trip in the aligned form -- a 16-byte load from each class plane and one label dword --
// and one pixel a trip, with its bounds checked, in the scalar form (HW no multiple of 4, logits not 16-byte or labels not 4-byte
// aligned).  The largest logit, the second largest and the argmax are found in registers; all K margins come from those.
//
// The workgroup counts into a K x 2 x 1024 histogram of 32-bit words in LDS (16 KB at 2 classes, 64 KB at 8: the whole static
// allowance, so the kernel has no other shared variable) and adds the words that are not zero to the sample's row with 64-bit
// global atomics.  Integer sums: no order of arrival changes a bit.
//
// A trained decoder is confident almost everywhere: nearly every pixel is in the clamp bin 1023 of its own class and in the clamp
// bin 0 of every other class, and 64 lanes of a wave would meet at one LDS address.  Those two words of every class are therefore
// counted per WAVE, not in LDS: a ballot and a popcount each, added to a wave-uniform register, and one lane adds the sums at the
// end.  Every other pixel is one LDS atomic a class.  Measured: the ballots take a third off the confident
// FFHQ batch and cost a tenth on uniform noise; runs of equal keys per lane, the merge that pays in gsa_compare.hip, gain the same
// on confident logits but nothing on top of the ballots, and two quads a lane in flight gain nothing either.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/gsa.h"
#include "gsa_plane.h"
#include "gsa_scores.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 4;                         // pixels of a lane in a trip of the aligned form
constexpr int kBins = GSA_SCORE_BINS;
constexpr int kMaxClasses = GSA_SCORE_MAX_CLASSES;
constexpr int kStretch = GSA_SCORE_STRETCH;
constexpr int kMaxBlocks = GSA_SCORE_MAX_BLOCKS;
constexpr int kMaxGridY = 65535;

static_assert(kBins == 1024, "the key of a word is (2 c + [y == c]) << 10 | bin");
static_assert(kMaxClasses * 2 * kBins * sizeof(unsigned) <= 65536, "the histogram of 8 classes is the static LDS allowance");
static_assert(kStretch % (kThreads * kPix) == 0, "a stretch is whole trips of the aligned form");

// What a wave carries through its pixels, per class, the same in every lane: its pixels in the two clamp words, (others, bin 0)
// and (own, bin 1023).
template <int K>
struct Counts {
    unsigned lo[K], hi[K];
};

__device__ __forceinline__ int bin_of(float m, float scale, bool nan) {
    const float t = ceilf(m * scale);           // exact scaling; +-inf stay, NaN stays
    return (nan || !(t > -511.0f)) ? 0 : (t >= 512.0f ? kBins - 1 : (int)t + 511);
}

// One pixel: z its K logits, y its label.  Called by every lane of the wave together (the ballots), `inside` false for a lane that
// has no pixel.
template <int K>
__device__ __forceinline__ void count_pixel(unsigned* hist, const float (&z)[K], int y, bool inside, float scale, Counts<K>& s) {
    const bool valid = inside && y >= 0 && y < K;
    float a = z[0], b = -INFINITY;              // the largest and the second largest; b = a on a tie
    int arg = 0;
    bool nan = z[0] != z[0];
#pragma unroll
    for (int k = 1; k < K; ++k) {
        const float v = z[k];
        nan |= v != v;
        if (v > a) {
            b = a;
            a = v;
            arg = k;
        } else if (v > b) {
            b = v;
        }
    }
#pragma unroll
    for (int c = 0; c < K; ++c) {
        const float m = c == arg ? a - b : z[c] - a;
        const int bin = bin_of(m, scale, nan);
        const bool own = y == c;
        const unsigned key = (unsigned)((2 * c + (own ? 1 : 0)) << 10) + (unsigned)bin;
        const bool l = valid && !own && bin == 0, h = valid && own && bin == kBins - 1;
        s.lo[c] += (unsigned)__popcll(__ballot(l));
        s.hi[c] += (unsigned)__popcll(__ballot(h));
        if (valid && !l && !h) atomicAdd(&hist[key], 1u);
    }
}

__global__ __launch_bounds__(kThreads) void scores_init_kernel(long long* __restrict__ rows, long long words) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < words) rows[i] = 0;
}

// logits, labels, rows: of the launch's first sample; the sample is blockIdx.y
template <int K, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void score_histogram_kernel(const float* __restrict__ logits, const int8_t* __restrict__ labels,
                                                                   long long* __restrict__ rows, int HW, float scale) {
    constexpr int kWords = K * 2 * kBins;
    __shared__ unsigned hist[kWords];
    const size_t n = blockIdx.y, HWs = (size_t)HW;
    const float* __restrict__ z = logits + n * K * HWs;
    const int8_t* __restrict__ lab = labels + n * HWs;
    for (int f = threadIdx.x; f < kWords; f += kThreads) hist[f] = 0;
    __syncthreads();

    Counts<K> s;
#pragma unroll
    for (int c = 0; c < K; ++c) s.lo[c] = s.hi[c] = 0;

    // every loop below is uniform over the workgroup: a lane without a pixel reads the trip's first one and counts nothing
    const size_t stride = (size_t)gridDim.x * kThreads;
    if (ALIGNED) {
        const size_t quads = HWs / kPix;
        for (size_t base = (size_t)blockIdx.x * kThreads; base < quads; base += stride) {
            const bool inside = base + threadIdx.x < quads;
            const size_t o = kPix * (inside ? base + threadIdx.x : base);
            float4 v[K];
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = *reinterpret_cast<const float4*>(z + k * HWs + o);
            const unsigned lw = *reinterpret_cast<const unsigned*>(lab + o);
#pragma unroll
            for (int p = 0; p < kPix; ++p) {
                float zp[K];
#pragma unroll
                for (int k = 0; k < K; ++k) zp[k] = p == 0 ? v[k].x : p == 1 ? v[k].y : p == 2 ? v[k].z : v[k].w;
                count_pixel<K>(hist, zp, (int)(int8_t)gsa::plane::byte_of(lw, p), inside, scale, s);
            }
        }
    } else {
        for (size_t base = (size_t)blockIdx.x * kThreads; base < HWs; base += stride) {
            const bool inside = base + threadIdx.x < HWs;
            const size_t o = inside ? base + threadIdx.x : base;
            float zp[K];
#pragma unroll
            for (int k = 0; k < K; ++k) zp[k] = z[k * HWs + o];
            count_pixel<K>(hist, zp, (int)lab[o], inside, scale, s);
        }
    }

#pragma unroll
    for (int c = 0; c < K; ++c) {
        if ((threadIdx.x & 63) == 0) {
            if (s.lo[c]) atomicAdd(&hist[(2 * c) << 10], s.lo[c]);
            if (s.hi[c]) atomicAdd(&hist[((2 * c + 1) << 10) + kBins - 1], s.hi[c]);
        }
    }
    __syncthreads();

    // ---- the workgroup's histogram into the sample's row: one 64-bit atomic per word that is not zero
    long long* __restrict__ row = rows + n * kWords;
    for (int f = threadIdx.x; f < kWords; f += kThreads) {
        const unsigned v = hist[f];
        if (v) __hip_atomic_fetch_add(row + f, (long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

int blocks_of(int32_t HW) {
    const int64_t b = ((int64_t)HW + kStretch - 1) / kStretch;
    return (int)(b < kMaxBlocks ? b : kMaxBlocks);
}

using Kernel = void (*)(const float*, const int8_t*, long long*, int, float);

template <int K>
Kernel kernel_of(int classes, bool aligned) {
    if (classes == K) return aligned ? score_histogram_kernel<K, true> : score_histogram_kernel<K, false>;
    if constexpr (K < kMaxClasses) return kernel_of<K + 1>(classes, aligned);
    return nullptr;
}

}  // namespace

extern "C" {

int gsa_score_histogram(void* stream, int32_t n, int32_t classes, int32_t HW, int32_t shift, const float* logits,
                        const int8_t* labels, int64_t* rows) {
    if (n == 0) return GSA_OK;
    if (n < 0 || classes < 2 || classes > kMaxClasses || HW <= 0 || shift < 0 || shift > GSA_SCORE_MAX_SHIFT) return GSA_ERR_INVALID;
    if (!logits || !labels || !rows) return GSA_ERR_INVALID;
    const uintptr_t zbits = reinterpret_cast<uintptr_t>(logits), lbits = reinterpret_cast<uintptr_t>(labels);
    if ((zbits & 3) || (reinterpret_cast<uintptr_t>(rows) & 7)) return GSA_ERR_INVALID;
    const uint64_t planes = (uint64_t)n * (uint64_t)classes;            // < 2^34
    if (planes > ((1ull << 40) - 1) / (uint64_t)HW) return GSA_ERR_INVALID;         // n * classes * HW >= 2^40
    const uint64_t row_bytes = planes * 2 * kBins * sizeof(int64_t);
    if (gsa::plane::ranges_overlap(rows, row_bytes, logits, planes * (uint64_t)HW * sizeof(float)) ||
        gsa::plane::ranges_overlap(rows, row_bytes, labels, (uint64_t)n * (uint64_t)HW))
        return GSA_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const bool aligned = HW % kPix == 0 && (zbits & 15) == 0 && (lbits & 3) == 0;
    const Kernel kernel = kernel_of<2>(classes, aligned);
    const int blocks = blocks_of(HW);
    const size_t HWs = (size_t)HW, row_words = (size_t)classes * 2 * kBins;
    long long* out = reinterpret_cast<long long*>(rows);
    // the sample is the grid's y: at most 65535 of them a launch
    for (int32_t first = 0; first < n; first += kMaxGridY) {
        const int count = n - first < kMaxGridY ? n - first : kMaxGridY;
        const size_t f = (size_t)first;
        long long* rw = out + f * row_words;
        const long long words = (long long)count * (long long)row_words;           // < 2^30
        hipLaunchKernelGGL(scores_init_kernel, dim3((unsigned)((words + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, rw, words);
        hipLaunchKernelGGL(kernel, dim3(blocks, count), dim3(kThreads), 0, s, logits + f * classes * HWs, labels + f * HWs, rw, HW,
                           (float)(1 << shift));
    }
    return hipGetLastError() == hipSuccess ? GSA_OK : GSA_ERR_HIP;
}

}  // extern "C"
