// Host arithmetic of the weight commit (gsa_api.cpp): the packed layouts the MFMA kernels read and the oracle restates, and the
// parameter folds.  Plain C++17, no HIP, no context: tests/test_pack_host.py calls these entries without a GPU.  Internal -- not
// part of include/ -- but exported like every other symbol of the library.  `out` buffers are the caller's; sizes in floats.
#pragma once
#include <stddef.h>
#include <stdint.h>

// the effective weight (W*std)*lr_mult -- two fp32 roundings, reference networks_stylegan.py:407-412,513-518
inline float gsa_eff(float w, float std, bool use_std, float lr) {
    float v = use_std ? w * std : w;
    return v * lr;
}

extern "C" {

// Blocked MFMA packs [O/16][I/4J][tap][kq][16][J]: cout = 16g + n, channel = 4J*cb + J*kq + j (kq = k slot of the MFMA); J = 4 but
// for gsa_pack_wino43 (J = 2).  Weights are effective ones (gsa_eff).
void gsa_pack_conv3(const float* w, int O, int I, float std, int use_std, float lr, float* out);    // OIHW (O,I,3,3) -> 9 taps
void gsa_pack_deconv(const float* w, int I, int O, float std, int use_std, float lr, float* out);   // IOHW (I,O,4,4) -> 16 taps
void gsa_pack_upconv(const float* w, int O, int I, float std, int use_std, float lr, float* out);   // (O,I,3,3) -> 16 sub-pixel taps
void gsa_pack_conv1(const float* w, int O, int I, float* out);                                      // (O,I,1,1) -> 1 tap, raw weights
void gsa_pack_wino(const float* w, int O, int I, float std, int use_std, float lr, float* out);     // (O,I,3,3) -> 16 frequencies
void gsa_pack_wino43(const float* w, int O, int I, float std, int use_std, float lr, float* out);   // (O,I,3,3) -> 36 frequencies
void gsa_pack_final(const float* w, int K, int I, float* out);      // final conv (K,I,3,3) -> [I/16][tap][c16][K]

uint16_t gsa_pack_bf16_rne(float f);                                // fp32 -> bf16, round to nearest even; NaN stays NaN
void gsa_pack_bf16(const float* in, size_t count, uint16_t* out);   // an fp32 MFMA pack element by element: its k order is bf16's already
// conv bias + inference BatchNorm as one fma: s = gamma / sqrtf(var + 1e-5f), k = fmaf(bias - mean, s, beta)
void gsa_pack_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, const float* bias, int C, float* s,
                      float* k);
void gsa_pack_constant(const float* w, int C, float* out);                              // constant tensor (C,4,4) -> [p][ch]
void gsa_pack_mapping(const float* w, int L, float std, int use_std, float* out);       // dense (L,L) [j][k] -> [k][j], lr_mult 0.01

}  // extern "C"
