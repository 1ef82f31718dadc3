// gsa_loss.hip -- the decoder losses' kernels (gsa_loss.h): softmax cross-entropy with class and boundary
// weights, a focal factor q^gamma and three normalisers, and its gradient.
//
// Two launches, the same grid shape: (min(ceil(HW / 256), GSA_LOSS_MAX_BLOCKS), n) workgroups of 256 threads; a workgroup
// grid-strides over the pixels of ONE sample, a lane a pixel, so for a fixed class consecutive lanes read consecutive floats.  A
// thread takes four pixels a trip, each a grid stride from the last: the walk is latency-bound, a label and then K logits deep, and
// four independent chains in flight cost little more than one.
//
//   loss_sums_kernel    every thread adds W, B, S, T of its pixels in double; a wave reduces by shuffles (offsets 32 .. 1), the four
//                       waves through LDS, added in wave order; threads 0..3 store the four sums at workspace[n][block][0..3].
//   loss_finish_kernel  every workgroup copies the partials of its sample to LDS and four of its lanes add them in index order,
//                       one sum each -- every workgroup gets the same bits -- and workgroup 0 of the sample writes sums[n] and
//                       loss[n].  With dlogits the workgroup then walks its pixels again, recomputes their softmax and writes the
//                       gradient; without, the launch has one workgroup a sample and ends there.
//
// No atomics, no memset, no value that depends on n or on which workgroup ran first: loss, sums and dlogits of a sample are the
// same bits in every run, for every batch size and at every position in the batch.
//
// class_weight (up to 64 floats) and dist_table (1026 floats, 4 KB) are indexed per lane by label and by dist2, so they go to LDS
// once a workgroup.  Per pixel everything is fp32 (expf, logf, powf; -ffp-contract=off), as in softmax_ce_kernel of gsa_train.hip;
// q = 1 - p_y is the sum of the OTHER classes' exponentials over the sum of all; e_y = p_y - 1 is written as -q where q <= 1/2 and as
// p_y - 1 where p_y < 1/2, each time the form that loses no digits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/gsa.h"
#include "gsa_loss.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSums = GSA_LOSS_SUMS;
constexpr int kTable = GSA_LOSS_TABLE;
constexpr int kMaxClasses = 64;
constexpr int kMaxBlocks = GSA_LOSS_MAX_BLOCKS;
constexpr int kMaxGridY = 65535;
constexpr int kUnroll = 4;                        // pixels of a thread in flight together

static_assert((kMaxBlocks & (kMaxBlocks - 1)) == 0, "the block cap is a power of two");
static_assert(kSums == 4 && kTable == 1026, "W, B, S, T; dist2 0..1024 and one entry for the rest");

struct Args {
    const float* logits;
    const int8_t* labels;
    const float* class_weight;
    const int16_t* dist2;
    const float* dist_table;
    int K, HW;
    float gamma;
    int normalise;
};

// What one pixel contributes: its weight, the focal factor and the pieces of the gradient.
struct Pixel {
    float w, beta, h, ce, q, py, m, se;
};

// The pixels of one trip of a thread: kUnroll of them, a grid stride apart.  Their loads are independent of one another and of the
// labels, so they are in flight together; a pixel past the end of the plane or with an ignored label is computed on the address
// and the class of a pixel that exists and then dropped (valid = false), which keeps the trip free of branches around its loads.
struct Trip {
    size_t idx[kUnroll];            // offset in the plane, below HW
    int y[kUnroll];                 // class, in [0, K)
    bool inside[kUnroll], valid[kUnroll];
};

// class_weight and dist_table into LDS (ones where there is none); the caller synchronises
__device__ __forceinline__ void stage_tables(const Args& a, float* cw, float* tab) {
    for (int k = threadIdx.x; k < a.K; k += kThreads) cw[k] = a.class_weight ? a.class_weight[k] : 1.0f;
    if (a.dist_table)
        for (int d = threadIdx.x; d < kTable; d += kThreads) tab[d] = a.dist_table[d];
}

// first < HW: the trip's first pixel; stride: the pixels of all threads of the sample
__device__ __forceinline__ Trip trip_of(const Args& a, const int8_t* __restrict__ lab, size_t first, size_t stride) {
    Trip t;
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        const size_t i = first + u * stride;
        t.inside[u] = i < (size_t)a.HW;
        t.idx[u] = t.inside[u] ? i : first;
        const int y = lab[t.idx[u]];
        t.valid[u] = t.inside[u] && y >= 0 && y < a.K;
        t.y[u] = t.valid[u] ? y : 0;
    }
    return t;
}

// z, d2: the sample's planes (d2 or null).  The class loops run over the trip's pixels inside: kUnroll loads a class in flight.
__device__ __forceinline__ void eval_pixels(const Args& a, const float* __restrict__ z, const int16_t* __restrict__ d2, const Trip& t,
                                            const float* cw, const float* tab, Pixel (&p)[kUnroll]) {
    const size_t HW = (size_t)a.HW;
    float m[kUnroll], so[kUnroll], ey[kUnroll], zy[kUnroll];       // per pixel: the maximum; all classes but y, y alone; the logit of y
    int d[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        m[u] = z[t.idx[u]];
        d[u] = d2 ? (int)d2[t.idx[u]] : 0;
        so[u] = ey[u] = zy[u] = 0.0f;
    }
    for (int k = 1; k < a.K; ++k)
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) m[u] = fmaxf(m[u], z[k * HW + t.idx[u]]);
    for (int k = 0; k < a.K; ++k)
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const float v = z[k * HW + t.idx[u]];
            const float e = expf(v - m[u]);
            if (k == t.y[u]) {
                ey[u] = e;
                zy[u] = v;
            } else {
                so[u] += e;
            }
        }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        const float se = so[u] + ey[u];             // so that q = so / (so + ey) carries the roundings of so in both places
        p[u].m = m[u];
        p[u].se = se;
        p[u].ce = (m[u] + logf(se)) - zy[u];
        p[u].q = so[u] / se;
        p[u].py = ey[u] / se;
        float w = cw[t.y[u]];
        if (d2) w *= tab[(d[u] >= 0 && d[u] <= kTable - 2) ? d[u] : kTable - 1];
        p[u].w = w;
        if (a.gamma == 0.0f) {
            p[u].beta = 1.0f;
            p[u].h = 0.0f;
        } else {
            // q^(gamma - 1): 1 at gamma = 1, also for q = 0; the common exponents without powf, which is a hundred instructions
            const float q = p[u].q;
            const float qg1 = a.gamma == 1.0f ? 1.0f : a.gamma == 2.0f ? q : a.gamma == 3.0f ? q * q : powf(q, a.gamma - 1.0f);
            p[u].beta = qg1 * p[u].q;
            p[u].h = a.gamma * qg1 * p[u].py;
        }
    }
}

__global__ __launch_bounds__(kThreads) void loss_sums_kernel(Args a, double* __restrict__ workspace) {
    __shared__ float cw[kMaxClasses];
    __shared__ float tab[kTable];
    __shared__ double part[kWaves][kSums];
    stage_tables(a, cw, tab);
    __syncthreads();
    const size_t n = blockIdx.y, HW = (size_t)a.HW, stride = (size_t)gridDim.x * kThreads;
    const float* __restrict__ z = a.logits + n * a.K * HW;
    const int8_t* __restrict__ lab = a.labels + n * HW;
    const int16_t* __restrict__ d2 = a.dist2 ? a.dist2 + n * HW : nullptr;
    double s[kSums] = {0.0, 0.0, 0.0, 0.0};
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += kUnroll * stride) {
        const Trip t = trip_of(a, lab, i, stride);
        Pixel p[kUnroll];
        eval_pixels(a, z, d2, t, cw, tab, p);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {         // in the order of the pixels
            if (!t.valid[u]) continue;
            const double b = (double)p[u].w * (double)p[u].beta;
            s[0] += (double)p[u].w;
            s[1] += b;
            s[2] += b * (double)p[u].ce;
            s[3] += 1.0;
        }
    }
#pragma unroll
    for (int j = 0; j < kSums; ++j)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[j] += __shfl_down(s[j], off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < kSums; ++j) part[wave][j] = s[j];
    __syncthreads();
    if (threadIdx.x < kSums) {
        double t = part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) t += part[w][threadIdx.x];
        workspace[(n * gridDim.x + blockIdx.x) * kSums + threadIdx.x] = t;
    }
}

// blocks: the workgroups a sample had in loss_sums_kernel (gridDim.x there; here gridDim.x is 1 when dlogits is null)
__global__ __launch_bounds__(kThreads) void loss_finish_kernel(Args a, const double* __restrict__ workspace, int blocks,
                                                               float grad_scale, double* __restrict__ sums, float* __restrict__ loss,
                                                               float* __restrict__ dlogits) {
    __shared__ float cw[kMaxClasses];
    __shared__ float tab[kTable];
    __shared__ double total[kSums];
    __shared__ double parts[kMaxBlocks * kSums];        // 16 KB
    const size_t n = blockIdx.y, HW = (size_t)a.HW, stride = (size_t)gridDim.x * kThreads;
    // the sample's partials into LDS by all threads, then four lanes add them, one sum each: a chain of adds fed from LDS, not a
    // chain of loads from memory (measured: 19 us for 512 partials read one after the other)
    const double* __restrict__ src = workspace + n * blocks * kSums;
    for (int j = threadIdx.x; j < blocks * kSums; j += kThreads) parts[j] = src[j];
    if (dlogits) stage_tables(a, cw, tab);
    __syncthreads();
    if (threadIdx.x < kSums) {
        double t = 0.0;
#pragma unroll 8
        for (int b = 0; b < blocks; ++b) t += parts[b * kSums + threadIdx.x];        // index order: the same bits in every workgroup
        total[threadIdx.x] = t;
    }
    __syncthreads();
    const double S = total[2];
    const double D = a.normalise == 0 ? (double)a.HW : total[a.normalise == 1 ? 0 : 1];
    const double L = D != 0.0 ? S / D : 0.0;
    if (blockIdx.x == 0) {
        if (threadIdx.x < kSums) sums[n * kSums + threadIdx.x] = total[threadIdx.x];
        if (threadIdx.x == 0) loss[n] = (float)L;
    }
    if (!dlogits) return;

    const float* __restrict__ z = a.logits + n * a.K * HW;
    float* __restrict__ dz = dlogits + n * a.K * HW;
    const int8_t* __restrict__ lab = a.labels + n * HW;
    const int16_t* __restrict__ d2 = a.dist2 ? a.dist2 + n * HW : nullptr;
    const double scale = D != 0.0 ? (double)grad_scale / D : 0.0;
    const double Lh = a.normalise == 2 ? L : 0.0;         // the normaliser's own derivative: -L_n h_i
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < HW; i += kUnroll * stride) {
        const Trip t = trip_of(a, lab, i, stride);
        Pixel p[kUnroll];
        eval_pixels(a, z, d2, t, cw, tab, p);
        double c[kUnroll];
        float ey[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const float g = p[u].beta + p[u].h * p[u].ce;
            c[u] = (double)p[u].w * ((double)g - Lh * (double)p[u].h) * scale;
            // e_y = p_y - 1 = -q.  Where q <= 1/2, -q keeps the digits that p_y - 1 cancels; where p_y < 1/2 the subtraction is one
            // rounding of a value near -1 and q = so / se carries two.  The product with the coefficient is rounded once, from double.
            ey[u] = p[u].q > 0.5f ? p[u].py - 1.0f : -p[u].q;
        }
        const bool live = D != 0.0;
        for (int k = 0; k < a.K; ++k)
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                if (!t.inside[u]) continue;
                const float e = k == t.y[u] ? ey[u] : expf(z[k * HW + t.idx[u]] - p[u].m) / p[u].se;
                dz[k * HW + t.idx[u]] = t.valid[u] && live ? (float)(c[u] * (double)e) : 0.0f;       // exact zeros, never 0 * NaN
            }
    }
}

int blocks_of(int32_t HW) {
    const int64_t b = ((int64_t)HW + kThreads - 1) / kThreads;
    return (int)(b < kMaxBlocks ? b : kMaxBlocks);
}

bool misaligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0; }

}  // namespace

extern "C" {

int64_t gsa_loss_workspace_bytes(int32_t n, int32_t HW) {
    if (n < 0 || HW <= 0) return -1;
    return (int64_t)n * blocks_of(HW) * kSums * (int64_t)sizeof(double);
}

int gsa_loss_softmax(void* stream, int32_t n, int32_t classes, int32_t HW, const float* logits, const int8_t* labels,
                     const float* class_weight, const int16_t* dist2, const float* dist_table, float gamma, int32_t normalise,
                     float grad_scale, void* workspace, double* sums, float* loss, float* dlogits) {
    if (n == 0) return GSA_OK;
    if (n < 0 || classes < 2 || classes > kMaxClasses || HW <= 0) return GSA_ERR_INVALID;
    if (!logits || !labels || !workspace || !sums || !loss) return GSA_ERR_INVALID;
    if ((dist2 == nullptr) != (dist_table == nullptr)) return GSA_ERR_INVALID;
    if (!std::isfinite(gamma) || !(gamma == 0.0f || (gamma >= 1.0f && gamma <= 8.0f))) return GSA_ERR_INVALID;
    if (normalise < 0 || normalise > 2 || !std::isfinite(grad_scale)) return GSA_ERR_INVALID;
    if (misaligned(workspace, 8) || misaligned(sums, 8)) return GSA_ERR_INVALID;
    if (misaligned(logits, 4) || misaligned(class_weight, 4) || misaligned(dist_table, 4) || misaligned(loss, 4) || misaligned(dlogits, 4))
        return GSA_ERR_INVALID;
    if (misaligned(dist2, 2)) return GSA_ERR_INVALID;
    if ((uint64_t)n * (uint64_t)classes * (uint64_t)HW >= (1ull << 40)) return GSA_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int blocks = blocks_of(HW);
    const size_t HWs = (size_t)HW;
    // the sample is the grid's y: at most 65535 of them a launch
    for (int32_t first = 0; first < n; first += kMaxGridY) {
        const int count = n - first < kMaxGridY ? n - first : kMaxGridY;
        const size_t f = (size_t)first;
        Args a;
        a.logits = logits + f * classes * HWs;
        a.labels = labels + f * HWs;
        a.class_weight = class_weight;
        a.dist2 = dist2 ? dist2 + f * HWs : nullptr;
        a.dist_table = dist_table;
        a.K = classes;
        a.HW = HW;
        a.gamma = gamma;
        a.normalise = normalise;
        double* ws = reinterpret_cast<double*>(workspace) + f * blocks * kSums;
        hipLaunchKernelGGL(loss_sums_kernel, dim3(blocks, count), dim3(kThreads), 0, s, a, ws);
        hipLaunchKernelGGL(loss_finish_kernel, dim3(dlogits ? blocks : 1, count), dim3(kThreads), 0, s, a, ws, blocks, grad_scale,
                           sums + f * kSums, loss + f, dlogits ? dlogits + f * classes * HWs : nullptr);
    }
    return hipGetLastError() == hipSuccess ? GSA_OK : GSA_ERR_HIP;
}

}  // extern "C"
