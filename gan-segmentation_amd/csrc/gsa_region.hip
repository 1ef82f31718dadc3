// gsa_region.hip -- the region-overlap loss's kernels (gsa_region.h): per sample and class the soft Tversky
// index of the softmax against the labels, the loss over the chosen classes, and its gradient, written or accumulated.
//
// Two launches, the same grid shape: (blocks, n) workgroups of 256 threads, blocks = min(ceil(HW / 256), GSA_REGION_MAX_BLOCKS).
// The unit of the walk is a stride of 256 pixels, one wave's: a lane holds four consecutive pixels, so for a fixed class a wave
// reads 1 KB of consecutive floats, 16 bytes a lane, and the four labels are one dword.  Stride s of a sample belongs to workgroup
// s % blocks, and in it to wave (s / blocks) % 4.  Where HW is no multiple of four or a pointer is not 16-byte aligned the same
// lane takes the same four pixels with scalar loads and stores: the bits do not depend on the alignment.
//
//   region_sums_kernel    a thread keeps I_k, P_k (double) and G_k of its pixels in registers -- every loop over the classes is
//                         unrolled to a bound KM >= K (4, 8 or 16) and cut off at K by uniform branches, so no accumulator is ever
//                         indexed at run time; a wave reduces by shuffles (offsets 32 .. 1), the four waves through LDS, added
//                         in wave order; threads 0 .. 3K-1 store the partials at workspace[n][block][0 .. 3K-1] (G as int64).
//   region_finish_kernel  every workgroup stages the partials of its sample through LDS, 24 KB at a time, and 3K of its lanes add
//                         them in index order, one sum each -- every workgroup gets the same bits.  K lanes form N_k, D_k, TI_k
//                         and a_k c_k, every thread adds A and the loss in class order, K lanes form the two gradient
//                         coefficients of their class, grad_scale folded in.  Workgroup 0 of the sample writes sums, index and
//                         loss.  With dlogits the workgroup then walks its strides again, recomputes their softmax and writes
//                         the gradient; without, the launch has one workgroup a sample and ends there.
//
// No atomics, no memset, no value that depends on n or on which workgroup ran first.  Per pixel the softmax is fp32 (expf,
// -ffp-contract=off, correctly rounded division), as in gsa_loss.hip; everything that is summed or that cancels -- the sums, the
// index, sum_k g_k p_k and g_j - sum_k g_k p_k -- is double, and a gradient element is rounded once.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/gsa.h"
#include "gsa_region.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kQuad = 4;                          // pixels of a lane
constexpr int kStride = 64 * kQuad;               // pixels of a wave's trip
constexpr int kSums = GSA_REGION_SUMS;
constexpr int kMaxClasses = GSA_REGION_MAX_CLASSES;
constexpr int kMaxBlocks = GSA_REGION_MAX_BLOCKS;
constexpr int kMaxGridY = 65535;
constexpr int kStage = 64 * kSums * kMaxClasses;  // 8-byte partials staged in LDS at a time: 24 KB, at least 64 workgroups' worth

static_assert((kMaxBlocks & (kMaxBlocks - 1)) == 0, "the block cap is a power of two");
static_assert(kStride == 256 && kSums == 3, "a stride is 256 pixels; I, P, G");
static_assert(kSums * kMaxClasses <= 64, "the partials of a workgroup are added by one wave");

struct Args {
    const float* logits;
    const int8_t* labels;
    int K, HW;
    int vec;                        // HW % 4 == 0 and logits, labels, dlogits aligned for 16-byte accesses of four pixels
};

// The four pixels of a lane: their softmax, class by class, and their labels.
template <int KM>
struct Quad {
    float p[KM][kQuad];
    int y[kQuad];
    bool inside[kQuad], valid[kQuad];
};

// z, lab: the sample's planes; i0: the lane's first pixel.  The logits go to q.p as they are, softmax_quad turns them into the
// softmax; the two are apart so that the loads of a wave's next stride are in flight while it computes the one before.  A pixel
// past the end of the plane is computed on pixel 0 and dropped (inside = false), which keeps the loads free of branches.
template <int KM>
__device__ __forceinline__ void load_quad(const Args& a, const float* __restrict__ z, const int8_t* __restrict__ lab, size_t i0,
                                          Quad<KM>& q) {
    const size_t HW = (size_t)a.HW;
    if (a.vec) {                    // the four pixels are inside together
        const bool in = i0 < HW;
        const size_t i = in ? i0 : 0;
        const int packed = *reinterpret_cast<const int*>(lab + i);
#pragma unroll
        for (int u = 0; u < kQuad; ++u) {
            q.inside[u] = in;
            q.y[u] = (int)(int8_t)((unsigned)packed >> (8 * u));
        }
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            if (k >= a.K) continue;
            const float4 v = *reinterpret_cast<const float4*>(z + k * HW + i);
            q.p[k][0] = v.x;
            q.p[k][1] = v.y;
            q.p[k][2] = v.z;
            q.p[k][3] = v.w;
        }
    } else {
        size_t i[kQuad];
#pragma unroll
        for (int u = 0; u < kQuad; ++u) {
            q.inside[u] = i0 + u < HW;
            i[u] = q.inside[u] ? i0 + u : 0;
            q.y[u] = lab[i[u]];
        }
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            if (k >= a.K) continue;
#pragma unroll
            for (int u = 0; u < kQuad; ++u) q.p[k][u] = z[k * HW + i[u]];
        }
    }
}

template <int KM>
__device__ __forceinline__ void softmax_quad(const Args& a, Quad<KM>& q) {
    float m[kQuad], se[kQuad];
#pragma unroll
    for (int u = 0; u < kQuad; ++u) {
        q.valid[u] = q.inside[u] && q.y[u] >= 0 && q.y[u] < a.K;
        m[u] = q.p[0][u];
        se[u] = 0.0f;
    }
#pragma unroll
    for (int k = 1; k < KM; ++k) {
        if (k >= a.K) continue;
#pragma unroll
        for (int u = 0; u < kQuad; ++u) m[u] = fmaxf(m[u], q.p[k][u]);
    }
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        if (k >= a.K) continue;
#pragma unroll
        for (int u = 0; u < kQuad; ++u) {
            q.p[k][u] = expf(q.p[k][u] - m[u]);
            se[u] += q.p[k][u];
        }
    }
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        if (k >= a.K) continue;
#pragma unroll
        for (int u = 0; u < kQuad; ++u) q.p[k][u] = q.p[k][u] / se[u];
    }
}

template <int KM>
__global__ __launch_bounds__(kThreads) void region_sums_kernel(Args a, unsigned long long* __restrict__ workspace) {
    __shared__ unsigned long long part[kWaves][kSums * kMaxClasses];
    const int K = a.K, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t n = blockIdx.y, HW = (size_t)a.HW, blocks = gridDim.x, strides = (HW + kStride - 1) / kStride;
    const float* __restrict__ z = a.logits + n * K * HW;
    const int8_t* __restrict__ lab = a.labels + n * HW;
    double I[KM], P[KM];
    int G[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        I[k] = P[k] = 0.0;
        G[k] = 0;
    }
    const size_t first = blockIdx.x + blocks * wave, step = blocks * kWaves;
    Quad<KM> q, next;
    if (first < strides) load_quad(a, z, lab, first * kStride + (size_t)lane * kQuad, next);
    for (size_t s = first; s < strides; s += step) {
        q = next;
        if (s + step < strides) load_quad(a, z, lab, (s + step) * kStride + (size_t)lane * kQuad, next);
        softmax_quad(a, q);
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            if (k >= K) continue;
#pragma unroll
            for (int u = 0; u < kQuad; ++u) {       // in the order of the pixels
                const double p = q.valid[u] ? (double)q.p[k][u] : 0.0;
                const bool own = q.valid[u] && q.y[u] == k;
                P[k] += p;
                I[k] += own ? p : 0.0;
                G[k] += own ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        if (k >= K) continue;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            I[k] += __shfl_down(I[k], off, 64);
            P[k] += __shfl_down(P[k], off, 64);
            G[k] += __shfl_down(G[k], off, 64);     // a wave's count is below HW < 2^31
        }
        if (lane == 0) {
            part[wave][k] = (unsigned long long)__double_as_longlong(I[k]);
            part[wave][K + k] = (unsigned long long)__double_as_longlong(P[k]);
            part[wave][2 * K + k] = (unsigned long long)(long long)G[k];
        }
    }
    __syncthreads();
    const int j = threadIdx.x;
    if (j < kSums * K) {
        unsigned long long out;
        if (j < 2 * K) {
            double t = __longlong_as_double((long long)part[0][j]);
#pragma unroll
            for (int w = 1; w < kWaves; ++w) t += __longlong_as_double((long long)part[w][j]);
            out = (unsigned long long)__double_as_longlong(t);
        } else {
            long long t = (long long)part[0][j];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) t += (long long)part[w][j];
            out = (unsigned long long)t;
        }
        workspace[(n * blocks + blockIdx.x) * (size_t)(kSums * K) + j] = out;
    }
}

struct Rule {
    const float* class_weight;
    float alpha, beta, smooth, grad_scale;
    int mode, accumulate;
};

// blocks: the workgroups a sample had in region_sums_kernel (gridDim.x there; here gridDim.x is 1 when dlogits is null)
template <int KM>
__global__ __launch_bounds__(kThreads) void region_finish_kernel(Args a, Rule r, const unsigned long long* __restrict__ workspace,
                                                                 int blocks, double* __restrict__ sums, float* __restrict__ index,
                                                                 float* __restrict__ loss, float* __restrict__ dlogits) {
    __shared__ unsigned long long parts[kStage];
    __shared__ double total[kSums * kMaxClasses];                                   // I, P, G (as a double: below 2^31)
    __shared__ double Nk[kMaxClasses], Dk[kMaxClasses], TIk[kMaxClasses], ack[kMaxClasses];
    __shared__ double gown[kMaxClasses], gother[kMaxClasses];                       // grad_scale g_k,i where y_i == k, where not
    const int K = a.K, width = kSums * K, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t n = blockIdx.y, HW = (size_t)a.HW;
    const float* __restrict__ z = a.logits + n * K * HW;
    const int8_t* __restrict__ lab = a.labels + n * HW;
    const size_t strides = (HW + kStride - 1) / kStride, first = blockIdx.x + (size_t)gridDim.x * wave, step = (size_t)gridDim.x * kWaves;
    // the logits of the wave's first stride are asked for now and arrive behind the sums below
    Quad<KM> q, next;
    if (dlogits && first < strides) load_quad(a, z, lab, first * kStride + (size_t)lane * kQuad, next);

    // ---- the sample's partials, staged through LDS by all threads and added in index order by one lane a sum: a chain of adds
    // fed from LDS, not a chain of loads from memory (as loss_finish_kernel of gsa_loss.hip)
    const unsigned long long* __restrict__ src = workspace + n * blocks * (size_t)width;
    const int rows = kStage / width;
    double t = 0.0;
    long long g = 0;
    for (int b0 = 0; b0 < blocks; b0 += rows) {
        const int count = blocks - b0 < rows ? blocks - b0 : rows;
        for (int e = tid; e < count * width; e += kThreads) parts[e] = src[(size_t)b0 * width + e];
        __syncthreads();
        if (tid < 2 * K) {
#pragma unroll 8
            for (int b = 0; b < count; ++b) t += __longlong_as_double((long long)parts[b * width + tid]);
        } else if (tid < width) {
#pragma unroll 8
            for (int b = 0; b < count; ++b) g += (long long)parts[b * width + tid];
        }
        __syncthreads();
    }
    if (tid < width) total[tid] = tid < 2 * K ? t : (double)g;
    __syncthreads();

    // ---- the index of every class
    const double alpha = (double)r.alpha, beta = (double)r.beta, smooth = (double)r.smooth;
    if (tid < K) {
        const double I = total[tid], P = total[K + tid], G = total[2 * K + tid];
        const double N = I + smooth;
        const double D = ((1.0 - alpha - beta) * I + alpha * P) + beta * G + smooth;
        double T = 0.0;                     // the sample's valid pixels: without one no class is in the set
        for (int k = 0; k < K; ++k) T += total[2 * K + k];
        // D_k > 0 as the rule means it, in exact arithmetic: a softmax is positive, so with a valid pixel P_k > 0 and I_k > 0 where
        // G_k > 0.  It is decided from the counts and the parameters, which are exact -- an fp32 p_k that underflows to 0 at every
        // pixel must not move its class out of the set.  Such a class has N_k = smooth = 0 and scores 0.
        const bool on = T > 0.0 && (G > 0.0 || (r.mode == 1 && (smooth > 0.0 || alpha > 0.0)));
        const double c = r.class_weight ? (double)r.class_weight[tid] : 1.0;
        Nk[tid] = N;
        Dk[tid] = D;
        TIk[tid] = on && D > 0.0 ? N / D : 0.0;
        ack[tid] = on ? c : 0.0;
    }
    __syncthreads();
    double A = 0.0, L = 0.0;
    for (int k = 0; k < K; ++k) {           // class order: the same bits in every thread
        A += ack[k];
        L += ack[k] * (1.0 - TIk[k]);
    }
    const bool live = A != 0.0;
    L = live ? L / A : 0.0;
    if (tid < K) {
        const double N = Nk[tid], D = Dk[tid];
        const bool on = live && ack[tid] != 0.0 && D > 0.0;
        const double w = on ? (double)r.grad_scale * (ack[tid] / A) / (D * D) : 0.0;
        gown[tid] = on ? -(w * (D - (1.0 - beta) * N)) : 0.0;
        gother[tid] = on ? w * (alpha * N) : 0.0;
    }
    if (blockIdx.x == 0) {
        if (tid < width) sums[n * width + tid] = total[tid];
        if (tid < K) index[n * K + tid] = (float)TIk[tid];
        if (tid == 0) loss[n] = (float)L;
    }
    if (!dlogits) return;
    if (!live && r.accumulate) return;      // nothing to add: every pixel keeps its bits
    __syncthreads();

    // ---- the gradient of the workgroup's strides
    float* __restrict__ dz = dlogits + n * K * HW;
    for (size_t s = first; s < strides; s += step) {
        const size_t i0 = s * kStride + (size_t)lane * kQuad;
        q = next;
        if (s + step < strides) load_quad(a, z, lab, (s + step) * kStride + (size_t)lane * kQuad, next);
        softmax_quad(a, q);
        double dot[kQuad] = {0.0, 0.0, 0.0, 0.0};       // sum_k g_k,i p_k,i
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            if (k >= K) continue;
            const double go = gown[k], gn = gother[k];
#pragma unroll
            for (int u = 0; u < kQuad; ++u) dot[u] += (q.y[u] == k ? go : gn) * (double)q.p[k][u];
        }
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            if (k >= K) continue;
            const double go = gown[k], gn = gother[k];
            float d[kQuad];
#pragma unroll
            for (int u = 0; u < kQuad; ++u)             // exact zeros, never 0 * NaN
                d[u] = q.valid[u] && live ? (float)((double)q.p[k][u] * ((q.y[u] == k ? go : gn) - dot[u])) : 0.0f;
            float* __restrict__ out = dz + k * HW + i0;
            if (a.vec) {
                if (!q.inside[0]) continue;
                float4* __restrict__ out4 = reinterpret_cast<float4*>(out);
                if (r.accumulate) {
                    const float4 old = *out4;
                    float4 v;
                    v.x = q.valid[0] ? old.x + d[0] : old.x;
                    v.y = q.valid[1] ? old.y + d[1] : old.y;
                    v.z = q.valid[2] ? old.z + d[2] : old.z;
                    v.w = q.valid[3] ? old.w + d[3] : old.w;
                    *out4 = v;
                } else {
                    *out4 = make_float4(d[0], d[1], d[2], d[3]);
                }
            } else {
#pragma unroll
                for (int u = 0; u < kQuad; ++u) {
                    if (!q.inside[u]) continue;
                    if (!r.accumulate)
                        out[u] = d[u];
                    else if (q.valid[u])
                        out[u] = out[u] + d[u];
                }
            }
        }
    }
}

struct Out {
    double* sums;
    float *index, *loss, *dlogits;
};

// KM: the bound the class loops are unrolled to, the smallest of 4, 8 and GSA_REGION_MAX_CLASSES that holds the classes.  The
// kernels are the same text for each; a thread's registers grow with the bound (the softmax of two strides and the accumulators:
// 92, 136 and 241 VGPRs), so the decoder's 2 .. 8 classes keep five or three waves a SIMD resident where 16 keep two.
template <int KM>
void launch_pair(hipStream_t s, const Args& a, const Rule& r, unsigned long long* ws, int blocks, int count, const Out& o) {
    hipLaunchKernelGGL(region_sums_kernel<KM>, dim3(blocks, count), dim3(kThreads), 0, s, a, ws);
    hipLaunchKernelGGL(region_finish_kernel<KM>, dim3(o.dlogits ? blocks : 1, count), dim3(kThreads), 0, s, a, r, ws, blocks, o.sums,
                       o.index, o.loss, o.dlogits);
}

int blocks_of(int32_t HW) {
    const int64_t b = ((int64_t)HW + kStride - 1) / kStride;
    return (int)(b < kMaxBlocks ? b : kMaxBlocks);
}

bool misaligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0; }

bool weight_ok(float v) { return std::isfinite(v) && v >= 0.0f; }

}  // namespace

extern "C" {

int64_t gsa_region_workspace_bytes(int32_t n, int32_t classes, int32_t HW) {
    if (n < 0 || classes < 2 || classes > kMaxClasses || HW <= 0) return -1;
    return (int64_t)n * blocks_of(HW) * kSums * classes * (int64_t)sizeof(double);
}

int gsa_region_tversky(void* stream, int32_t n, int32_t classes, int32_t HW, const float* logits, const int8_t* labels,
                       const float* class_weight, float alpha, float beta, float smooth, int32_t mode, float grad_scale,
                       int32_t accumulate, void* workspace, double* sums, float* index, float* loss, float* dlogits) {
    if (n == 0) return GSA_OK;
    if (n < 0 || classes < 2 || classes > kMaxClasses || HW <= 0) return GSA_ERR_INVALID;
    if (!logits || !labels || !workspace || !sums || !index || !loss) return GSA_ERR_INVALID;
    if (!weight_ok(alpha) || !weight_ok(beta) || !weight_ok(smooth) || alpha + beta == 0.0f) return GSA_ERR_INVALID;
    if (mode < 0 || mode > 1 || !std::isfinite(grad_scale)) return GSA_ERR_INVALID;
    if (misaligned(workspace, 8) || misaligned(sums, 8)) return GSA_ERR_INVALID;
    if (misaligned(logits, 4) || misaligned(class_weight, 4) || misaligned(index, 4) || misaligned(loss, 4) || misaligned(dlogits, 4))
        return GSA_ERR_INVALID;
    if ((uint64_t)n * (uint64_t)classes * (uint64_t)HW >= (1ull << 40)) return GSA_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int blocks = blocks_of(HW), width = kSums * classes;
    const size_t HWs = (size_t)HW;
    // the sample is the grid's y: at most 65535 of them a launch
    for (int32_t first = 0; first < n; first += kMaxGridY) {
        const int count = n - first < kMaxGridY ? n - first : kMaxGridY;
        const size_t f = (size_t)first;
        Args a;
        a.logits = logits + f * classes * HWs;
        a.labels = labels + f * HWs;
        a.K = classes;
        a.HW = HW;
        a.vec = HW % kQuad == 0 && !misaligned(logits, 16) && !misaligned(labels, 4) && !misaligned(dlogits, 16);
        Rule r;
        r.class_weight = class_weight;
        r.alpha = alpha;
        r.beta = beta;
        r.smooth = smooth;
        r.grad_scale = grad_scale;
        r.mode = mode;
        r.accumulate = accumulate != 0;
        unsigned long long* ws = reinterpret_cast<unsigned long long*>(workspace) + f * blocks * width;
        const Out o = {sums + f * width, index + f * classes, loss + f, dlogits ? dlogits + f * classes * HWs : nullptr};
        if (classes <= 4)
            launch_pair<4>(s, a, r, ws, blocks, count, o);
        else if (classes <= 8)
            launch_pair<8>(s, a, r, ws, blocks, count, o);
        else
            launch_pair<kMaxClasses>(s, a, r, ws, blocks, count, o);
    }
    return hipGetLastError() == hipSuccess ? GSA_OK : GSA_ERR_HIP;
}

}  // extern "C"
