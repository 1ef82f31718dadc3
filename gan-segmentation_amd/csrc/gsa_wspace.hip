// Style affines of all 2*nlev layers from per-layer dlatents (N, NL, K) -- StyleGAN's W+ synthesis input.  The arithmetic per
// output is that of dense_lds_kernel<true, 64, 128> (gsa_kernels.hip): the truncated latent x' = avg[k]*(1-psi_l) + w[k]*psi_l
// (three roundings), one k-ordered fmaf chain from 0 over k, then + b[j].  So when every layer's row is the same w, the styles are
// bit-identical to launch_styles.  Each workgroup owns up to 64 columns of ONE layer (a tile table built at commit), so it stages
// one dlatent row per sample and always forms x' once per (sample, k) before the chains; a layer narrower than 64 columns or not a
// multiple of 16 simply leaves lanes idle.
#include "gsa_kernels.h"
#include "gsa_dev.h"

#include <algorithm>

namespace gsa {

template <int JB, int KC>      // JB output columns per workgroup, KC K rows per LDS pass
__global__ __launch_bounds__(256) void dlatent_styles_kernel(const float* dl, const float* WT, const float* b, float* y, int n, int K,
                                                             int J, int NL, const float* avg, const float* psi, const int4* tiles) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int G = 256 / JB, SPT = 16 / G, NW = KC * JB / 256;
    float* sW = smem;                               // [KC][JB]
    float* sX = sW + KC * JB;                       // [16][KC]
    float* sAvg = sX + 16 * KC;                     // [KC]
    const int4 t = tiles[blockIdx.x];               // {layer, first column, columns}
    const int layer = t.x, j0 = t.y, nc = t.z;
    const int tid = threadIdx.x, jl = tid % JB, ng = tid / JB;
    const int j = j0 + jl;
    const float ps = psi[layer], om = 1.0f - ps;
    for (int n0 = 16 * (int)blockIdx.y; n0 < n; n0 += 16 * (int)gridDim.y) {
        const int nn = min(16, n - n0);
        float acc[SPT];                             // samples n0 + ng + G*i
#pragma unroll
        for (int i = 0; i < SPT; ++i) acc[i] = 0.f;
        for (int k0 = 0; k0 < K; k0 += KC) {
            __syncthreads();
            // weight panel: KC x nc floats of this layer's columns (rows of 4*nc contiguous bytes; columns past nc are zero, never stored)
            float rw[NW];
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                const int idx = tid + i * 256, kr = idx / JB, c = idx % JB;
                rw[i] = c < nc ? WT[(size_t)(k0 + kr) * J + j0 + c] : 0.f;
            }
            for (int idx = tid; idx < nn * KC; idx += 256)
                sX[idx] = dl[((size_t)(n0 + idx / KC) * NL + layer) * K + k0 + idx % KC];
            for (int idx = tid; idx < KC; idx += 256) sAvg[idx] = avg[k0 + idx];
#pragma unroll
            for (int i = 0; i < NW; ++i) sW[tid + i * 256] = rw[i];
            __syncthreads();
            for (int idx = tid; idx < nn * KC; idx += 256) {
                const float t0 = sAvg[idx % KC] * om, t1 = sX[idx] * ps;
                sX[idx] = t0 + t1;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < SPT; ++i) {
                const int s = ng + G * i;
                if (s < nn) {
                    float a = acc[i];
                    const float* xs = sX + s * KC;
#pragma unroll 8
                    for (int k = 0; k < KC; ++k) a = fmaf(xs[k], sW[k * JB + jl], a);
                    acc[i] = a;
                }
            }
        }
        if (jl < nc) {
            const float bj = b[j];
#pragma unroll
            for (int i = 0; i < SPT; ++i) {
                const int s = ng + G * i;
                if (s < nn) y[(size_t)(n0 + s) * J + j] = acc[i] + bj;
            }
        }
    }
}

hipError_t launch_styles_dlatents(const float* dlatents, const float* avg, const float* psi, const float* WT, const float* b,
                                  const int4* tiles, int num_tiles, float* styles, int n, int K, int J, int NL, hipStream_t s) {
    if (K % 128 || num_tiles < 1) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * (128 * 64 + 16 * 128 + 128);
    return launch<dlatent_styles_kernel<64, 128>>(current_device(), dim3(num_tiles, std::min((n + 15) / 16, 8)), dim3(256), lds, s, dlatents,
                                                  WT, b, styles, n, K, J, NL, avg, psi, tiles);
}

}  // namespace gsa
