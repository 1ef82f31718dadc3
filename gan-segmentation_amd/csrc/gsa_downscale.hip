// Downscaled pairs (include/gsa.h gsa_generate_downscaled): the image and the mask at R/F, F in {2, 4, 8}, formed on the GPU from
// the fp32 values the full-size kernels stop at -- toRGB's u = 255 * clamp((v + 1) / 2, 0, 1) before the uint8 truncation, and the
// decoder's logits before the argmax.  Canonical rule: a block's sum S_F is a pairwise quad tree,
// S_2s(TL) = (S_s(TL) + S_s(TR)) + (S_s(BL) + S_s(BR)), every add rounded to fp32; pixel = (uint8_t)(S_F(u) * (1 / F^2)),
// mask = the first maximum over classes of S_F(logit).
//
// Both kernels own 16 x 16 pixel tiles with thread t on pixel (t / 16, t % 16), so a wave holds 4 rows of 16 pixels and F <= 8
// divides the tile: no block straddles a tile.  The tree is formed by xor exchanges -- lane distance 1 / 2 / 4 is the next pixel
// pair in x, 16 / 32 the next row pair in y -- and both partners of an exchange hold the same sum (fp32 add is commutative).  The
// 8-row level crosses waves and goes through LDS.  The per-pixel values are those of the full-size kernels bit for bit: toRGB's
// k-ordered fmaf chain + bias (torgb_direct_kernel / torgb_kernel) and final_conv_kernel's per-class chains (gsa_kernels.hip).
#include "gsa_kernels.h"
#include "gsa_dev.h"

namespace gsa {

// one level of the tree inside a wave: the x pair (lane distance DX) then the y pair (lane distance DY)
template <int DX, int DY>
__device__ __forceinline__ float quad_level(float s) {
    const float h = s + __shfl_xor(s, DX);
    return h + __shfl_xor(h, DY);
}

// S_F of every value of v[0..K) over the F x F block of this thread's pixel (16 x 16 tile, 256 threads); the result is valid in the
// block's top-left thread.  xch: >= 2 * 4 * K floats of LDS, used for F = 8 only (the caller's barrier protects its earlier use).
template <int F, int K>
__device__ __forceinline__ void block_tree(float (&v)[K], float* xch, int tid) {
    static_assert(F == 2 || F == 4 || F == 8, "F in {2, 4, 8}");
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = quad_level<1, 16>(v[k]);
    if constexpr (F >= 4) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = quad_level<2, 32>(v[k]);
    }
    if constexpr (F == 8) {
        // (S_4(TL) + S_4(TR)) in the upper wave of each wave pair, (S_4(BL) + S_4(BR)) in the lower one; the lower wave's left lanes
        // of each 8-pixel block hand theirs over
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += __shfl_xor(v[k], 4);
        const int wave = tid >> 6, lane = tid & 63, slot = ((wave >> 1) * 2 + ((lane >> 3) & 1)) * K;
        if ((wave & 1) && lane < 16 && (lane & 7) == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) xch[slot + k] = v[k];
        }
        __syncthreads();
        if (!(wave & 1)) {
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = v[k] + xch[slot + k];
        }
    }
}

// ------------------------------------------------------------------------------------------
// toRGB + _transform_gan_back at R/F.  Reads the generator's last activation (NHWC, AdaIN applied on read) once, with 16-byte
// loads: a thread reads its own pixel, 16 channels (four loads) in flight at a time, so the 64 lanes of a load cover 4 x 16 pixels
// of whole cache lines between them.
template <int F, bool BF>
__global__ __launch_bounds__(256) void torgb_down_kernel(const float* x, const Aff* aff, const float* w, const float* b, uint8_t* img,
                                                         int H, int W, int C, int nc, int tiles_x) {
    __shared__ float xch[2 * 4 * 4];
    const int tid = threadIdx.x, n = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const int y = ty * 16 + (tid >> 4), xx = tx * 16 + (tid & 15);
    const size_t px = ((size_t)(n * H + y) * W + xx) * C;
    const Aff* a = aff + (size_t)n * C;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < C; c0 += 16) {
        f32x4 ld[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (c0 + 4 * q < C) ld[q] = act_load4<BF>(x, px + c0 + 4 * q);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = c0 + 4 * q;
            if (c < C) {
                const float f[4] = {fmaf(ld[q][0], a[c].A, a[c].B), fmaf(ld[q][1], a[c + 1].A, a[c + 1].B),
                                    fmaf(ld[q][2], a[c + 2].A, a[c + 2].B), fmaf(ld[q][3], a[c + 3].A, a[c + 3].B)};
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int o = 0; o < 4; ++o)
                        if (o < nc) acc[o] = fmaf(f[j], w[o * C + c + j], acc[o]);
            }
        }
    }
    float u[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const float v = acc[o] + (o < nc ? b[o] : 0.0f);
        float t = (v + 1.0f) * 0.5f;
        t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
        u[o] = 255.0f * t;
    }
    block_tree<F, 4>(u, xch, tid);
    if ((y % F) == 0 && (xx % F) == 0) {
        const int Wo = W / F;
        uint8_t* dst = img + ((size_t)(n * (H / F) + y / F) * Wo + xx / F) * nc;
        for (int o = 0; o < nc; ++o) dst[o] = (uint8_t)(u[o] * (1.0f / (F * F)));
    }
}

// ------------------------------------------------------------------------------------------
// Final conv3x3 (in_c -> NCLS classes) + bias, then S_F per class and the argmax (first maximum wins), one byte per F x F block.
// The per-pixel logits are final_conv_kernel's bit for bit: the same 16 x 16 tiles and LDS-staged halo, the same register prefetch
// and per-class fmaf chains (in fp32 with an even class count, a class pair as ONE v_pk_fma_f32).  No logits are written.
template <int NCLS, int F, bool BF, bool PK>
__global__ __launch_bounds__(256) void final_conv_down_kernel(const float* src0, int C0, const float* src1, int C1,
                                                              const float* wpk, const float* bias, uint8_t* mask, int H, int W,
                                                              int tiles_x) {
    constexpr int LW = 18, CP = 20, RS = 384;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int bt = xcd_block(blockIdx.x, gridDim.x);
    const int ty = bt / tiles_x, tx = bt % tiles_x, n = blockIdx.y;
    const int y0 = ty * 16, x0 = tx * 16;
    const int ly = tid >> 4, lx = tid & 15;
    float acc[NCLS];
#pragma unroll
    for (int o = 0; o < NCLS; ++o) acc[o] = 0.0f;
    const int nblk0 = C0 >> 4, nblk = (C0 + C1) >> 4;
    float4 pre[2][4];
    auto load_block = [&](int cb) {
        const bool first = cb < nblk0;
        const float* src = first ? src0 : src1;
        const int Cs = first ? C0 : C1;
        const int coff = (first ? cb : cb - nblk0) * 16;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int idx = min(tid + it * 256, 18 * LW - 1);
            const int sy = idx / LW, sx = idx % LW;
            const int gy = y0 - 1 + sy, gx = x0 - 1 + sx;
            const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
            const int cy = min(max(gy, 0), H - 1), cx = min(max(gx, 0), W - 1);
            const size_t eidx = ((size_t)(n * H + cy) * W + cx) * Cs + coff;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const f32x4 ld = act_load4<BF>(src, eidx + 4 * k);
                pre[it][k] = make_float4(ld[0], ld[1], ld[2], ld[3]);
                if (!inside) pre[it][k] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };
    load_block(0);
    for (int cb = 0; cb < nblk; ++cb) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int idx = tid + it * 256;
            if (idx < 18 * LW) {
                float4* dst = reinterpret_cast<float4*>(smem + (idx / LW) * RS + (idx % LW) * CP);
#pragma unroll
                for (int k = 0; k < 4; ++k) dst[k] = pre[it][k];
            }
        }
        __syncthreads();
        if (cb + 1 < nblk) load_block(cb + 1);
        const float* wb = wpk + (size_t)cb * 9 * 16 * NCLS;   // [tap][c][NCLS]
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const float4* a4 = reinterpret_cast<const float4*>(smem + (ly + tap / 3) * RS + (lx + tap % 3) * CP);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 a = a4[k];
                const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (NCLS % 2 == 0 && PK) {
#pragma unroll
                        for (int o = 0; o < NCLS; o += 2) {
                            const f32x2 w2 = {wb[(tap * 16 + k * 4 + j) * NCLS + o], wb[(tap * 16 + k * 4 + j) * NCLS + o + 1]};
                            const f32x2 r = __builtin_elementwise_fma(f32x2{av[j], av[j]}, w2, f32x2{acc[o], acc[o + 1]});
                            acc[o] = r.x; acc[o + 1] = r.y;
                        }
                    } else {
#pragma unroll
                        for (int o = 0; o < NCLS; ++o) acc[o] = fmaf(av[j], wb[(tap * 16 + k * 4 + j) * NCLS + o], acc[o]);
                    }
                }
            }
        }
        __syncthreads();      // also ends every read of smem before block_tree reuses it
    }
    float v[NCLS];
#pragma unroll
    for (int o = 0; o < NCLS; ++o) v[o] = acc[o] + bias[o];
    block_tree<F, NCLS>(v, smem, tid);
    const int y = y0 + ly, x = x0 + lx;
    if ((y % F) == 0 && (x % F) == 0) {
        int best = 0;
        float bv = 0.0f;
#pragma unroll
        for (int o = 0; o < NCLS; ++o)
            if (o == 0 || v[o] > bv) { bv = v[o]; best = o; }
        if (mask) mask[(size_t)(n * (H / F) + y / F) * (W / F) + x / F] = (uint8_t)best;
    }
}

// ------------------------------------------------------------------------------------------ launchers

template <int F>
static hipError_t launch_torgb_down_t(const float* x, const Aff* aff, const float* w, const float* b, uint8_t* img, int n, int H, int W,
                                      int C, int nc, int bf16, hipStream_t s) {
    const dim3 grid((H / 16) * (W / 16), n);
    const int dev = current_device();
    if (bf16) return launch<torgb_down_kernel<F, true>>(dev, grid, dim3(256), 0, s, x, aff, w, b, img, H, W, C, nc, W / 16);
    return launch<torgb_down_kernel<F, false>>(dev, grid, dim3(256), 0, s, x, aff, w, b, img, H, W, C, nc, W / 16);
}

hipError_t launch_torgb_down(const float* x, const Aff* aff, const float* w, const float* b, uint8_t* img, int n, int H, int W, int C,
                             int nc, int f, int bf16, hipStream_t s) {
    if (nc < 1 || nc > 4 || C < 4 || C % 4 || H % 16 || W % 16 || H / f < 1 || W / f < 1) return hipErrorInvalidValue;
    switch (f) {
        case 2: return launch_torgb_down_t<2>(x, aff, w, b, img, n, H, W, C, nc, bf16, s);
        case 4: return launch_torgb_down_t<4>(x, aff, w, b, img, n, H, W, C, nc, bf16, s);
        case 8: return launch_torgb_down_t<8>(x, aff, w, b, img, n, H, W, C, nc, bf16, s);
    }
    return hipErrorInvalidValue;
}

template <int NCLS, int F>
static hipError_t launch_final_down_t(const float* src0, int C0, const float* src1, int C1, const float* wpk, const float* bias,
                                      uint8_t* mask, int n, int H, int W, int bf16, hipStream_t s) {
    const size_t lds = sizeof(float) * 18 * 384;
    const dim3 grid((H / 16) * (W / 16), n);
    const int dev = current_device();
    if (bf16)
        return launch<final_conv_down_kernel<NCLS, F, true, false>>(dev, grid, dim3(256), lds, s, src0, C0, src1, C1, wpk, bias, mask, H, W, W / 16);
    return launch<final_conv_down_kernel<NCLS, F, false, NCLS % 2 == 0>>(dev, grid, dim3(256), lds, s, src0, C0, src1, C1, wpk, bias, mask, H,
                                                                          W, W / 16);
}

template <int NCLS>
static hipError_t launch_final_down_c(const float* src0, int C0, const float* src1, int C1, const float* wpk, const float* bias,
                                      uint8_t* mask, int n, int H, int W, int f, int bf16, hipStream_t s) {
    switch (f) {
        case 2: return launch_final_down_t<NCLS, 2>(src0, C0, src1, C1, wpk, bias, mask, n, H, W, bf16, s);
        case 4: return launch_final_down_t<NCLS, 4>(src0, C0, src1, C1, wpk, bias, mask, n, H, W, bf16, s);
        case 8: return launch_final_down_t<NCLS, 8>(src0, C0, src1, C1, wpk, bias, mask, n, H, W, bf16, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_final_conv_down(const float* src0, int C0, const float* src1, int C1, const float* wpk, const float* bias, uint8_t* mask,
                                  int n, int H, int W, int ncls, int f, int bf16, hipStream_t s) {
    if (H % 16 || W % 16 || C0 % 16 || C1 % 16) return hipErrorInvalidValue;
    switch (ncls) {
        case 1: return launch_final_down_c<1>(src0, C0, src1, C1, wpk, bias, mask, n, H, W, f, bf16, s);
        case 2: return launch_final_down_c<2>(src0, C0, src1, C1, wpk, bias, mask, n, H, W, f, bf16, s);
        case 3: return launch_final_down_c<3>(src0, C0, src1, C1, wpk, bias, mask, n, H, W, f, bf16, s);
        case 4: return launch_final_down_c<4>(src0, C0, src1, C1, wpk, bias, mask, n, H, W, f, bf16, s);
        case 5: return launch_final_down_c<5>(src0, C0, src1, C1, wpk, bias, mask, n, H, W, f, bf16, s);
        case 6: return launch_final_down_c<6>(src0, C0, src1, C1, wpk, bias, mask, n, H, W, f, bf16, s);
        case 7: return launch_final_down_c<7>(src0, C0, src1, C1, wpk, bias, mask, n, H, W, f, bf16, s);
        case 8: return launch_final_down_c<8>(src0, C0, src1, C1, wpk, bias, mask, n, H, W, f, bf16, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace gsa
