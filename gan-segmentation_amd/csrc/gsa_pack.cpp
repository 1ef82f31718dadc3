// The pure host arithmetic of the weight commit (gsa_pack.h).  Every evaluation order here is canonical: the kernels
// and the oracle (oracle/c/gsa_oracle.c restates these packers) reproduce it bit for bit; -ffp-contract=off is part of it.
#include "gsa_pack.h"

#include <cmath>
#include <cstring>
#include <type_traits>

namespace {

// The one blocked layout [g][cb][t][kq][n][j] with o = 16g + n, channel = 4J*cb + J*kq + j.  A rule is either tap(o, channel, t), the value
// of one tap, walked in output order, or taps(o, channel, dst), which writes all T taps of a pair, tap t to dst[t * 64 * J].
template <int T, int J, class F>
inline void pack_blocks(int O, int I, float* __restrict out, F rule) {
    for (int g = 0; g < O / 16; ++g)
        for (int cb = 0; cb < I / (4 * J); ++cb, out += T * 64 * J)
            if constexpr (std::is_invocable_v<F, int, int, int>) {
                for (int t = 0; t < T; ++t)
                    for (int kq = 0; kq < 4; ++kq)
                        for (int n = 0; n < 16; ++n)
                            for (int j = 0; j < J; ++j) out[((t * 4 + kq) * 16 + n) * J + j] = rule(g * 16 + n, cb * 4 * J + kq * J + j, t);
            } else {
                float blk[T * 64 * J];      // the block, gathered where nothing aliases it, then copied out whole
                for (int kq = 0; kq < 4; ++kq)
                    for (int n = 0; n < 16; ++n)
                        for (int j = 0; j < J; ++j) rule(g * 16 + n, cb * 4 * J + kq * J + j, blk + (kq * 16 + n) * J + j);
                memcpy(out, blk, sizeof blk);
            }
}

}  // namespace

extern "C" {

void gsa_pack_conv3(const float* w, int O, int I, float std, int us, float lr, float* out) {
    pack_blocks<9, 4>(O, I, out, [=](int o, int ch, int t) { return gsa_eff(w[((size_t)o * I + ch) * 9 + t], std, us, lr); });
}

void gsa_pack_deconv(const float* w, int I, int O, float std, int us, float lr, float* out) {
    pack_blocks<16, 4>(O, I, out, [=](int o, int ch, int t) { return gsa_eff(w[((size_t)ch * O + o) * 16 + t], std, us, lr); });
}

// nearest-x2 + conv3x3 in sub-pixel form: the equivalent stride-2 transposed 4x4 kernel Wd[a][b] = sum_{ky in S(a)} sum_{kx in S(b)}
// W[ky][kx], S(0)={2} S(1)={1,2} S(2)={0,1} S(3)={0}; fp32 sums, ky then kx ascending, left to right, the first term assigned
void gsa_pack_upconv(const float* w, int O, int I, float std, int us, float lr, float* out) {
    static const int S[4][2] = {{2, -1}, {1, 2}, {0, 1}, {0, -1}};
    pack_blocks<16, 4>(O, I, out, [=](int o, int ch, float* taps) {
        const float* wk = w + ((size_t)o * I + ch) * 9;
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) {
                float sum = 0.0f;
                bool first = true;
                for (int i = 0; i < 2; ++i)
                    for (int j = 0; j < 2; ++j) {
                        if (S[a][i] < 0 || S[b][j] < 0) continue;
                        const float e = gsa_eff(wk[S[a][i] * 3 + S[b][j]], std, us, lr);
                        sum = first ? e : sum + e;
                        first = false;
                    }
                taps[(a * 4 + b) * 256] = sum;
            }
    });
}

void gsa_pack_conv1(const float* w, int O, int I, float* out) {
    pack_blocks<1, 4>(O, I, out, [=](int o, int ch, int) { return w[(size_t)o * I + ch]; });
}

// Winograd F(2x2,3x3): U = G g G^T evaluated in double on the effective fp32 weights and rounded once; frequency f = 4i + j
void gsa_pack_wino(const float* w, int O, int I, float std, int us, float lr, float* out) {
    pack_blocks<16, 4>(O, I, out, [=](int o, int ch, float* taps) {
        const float* wk = w + ((size_t)o * I + ch) * 9;
        double k[3][3], r[4][3], u[4][4];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) k[a][b] = (double)gsa_eff(wk[a * 3 + b], std, us, lr);
        for (int b = 0; b < 3; ++b) {
            r[0][b] = k[0][b];
            r[1][b] = 0.5 * ((k[0][b] + k[1][b]) + k[2][b]);
            r[2][b] = 0.5 * ((k[0][b] - k[1][b]) + k[2][b]);
            r[3][b] = k[2][b];
        }
        for (int a = 0; a < 4; ++a) {
            u[a][0] = r[a][0];
            u[a][1] = 0.5 * ((r[a][0] + r[a][1]) + r[a][2]);
            u[a][2] = 0.5 * ((r[a][0] - r[a][1]) + r[a][2]);
            u[a][3] = r[a][2];
        }
        for (int f = 0; f < 16; ++f) taps[f * 256] = (float)u[f >> 2][f & 3];
    });
}

// Winograd F(4x4,3x3): U = G g G^T with Lavin & Gray's 6x3 G, in double, rounded once; frequency f = 6i + j; 8-channel blocks
// (channel = 8cb + 2kq + j, the K order of conv3x3_wino43: a lane's weight pair is one 8-byte LDS read)
void gsa_pack_wino43(const float* w, int O, int I, float std, int us, float lr, float* out) {
    static const double G[6][3] = {{0.25, 0, 0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                   {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
    pack_blocks<36, 2>(O, I, out, [=](int o, int ch, float* taps) {
        const float* wk = w + ((size_t)o * I + ch) * 9;
        double k[3][3], r[6][3];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) k[a][b] = (double)gsa_eff(wk[a * 3 + b], std, us, lr);
        for (int i = 0; i < 6; ++i)
            for (int b = 0; b < 3; ++b) r[i][b] = (G[i][0] * k[0][b] + G[i][1] * k[1][b]) + G[i][2] * k[2][b];
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) taps[(i * 6 + j) * 128] = (float)((r[i][0] * G[j][0] + r[i][1] * G[j][1]) + r[i][2] * G[j][2]);
    });
}

void gsa_pack_final(const float* w, int K, int I, float* out) {
    for (int cb = 0; cb < I / 16; ++cb)
        for (int t = 0; t < 9; ++t)
            for (int ci = 0; ci < 16; ++ci)
                for (int o = 0; o < K; ++o)
                    out[(((size_t)cb * 9 + t) * 16 + ci) * K + o] = w[((size_t)o * I + cb * 16 + ci) * 9 + t];
}

// what v_cvt_pk_bf16_f32 does to the activations
uint16_t gsa_pack_bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// each 256-float [kq][16][j] chunk becomes [kq][16][4] bf16 with channel = 4*kq+j, the k order of v_mfma_f32_16x16x16_bf16 --
// half the bytes, addressed in the same 4-byte slots
void gsa_pack_bf16(const float* in, size_t count, uint16_t* out) {
    for (size_t i = 0; i < count; ++i) out[i] = gsa_pack_bf16_rne(in[i]);
}

void gsa_pack_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, const float* bias, int C, float* s,
                      float* k) {
    for (int i = 0; i < C; ++i) {
        s[i] = gamma[i] / std::sqrt(var[i] + 1e-5f);   // fp32: sqrtf, then one division
        k[i] = std::fmaf(bias[i] - mean[i], s[i], beta[i]);
    }
}

void gsa_pack_constant(const float* w, int C, float* out) {
    for (int ch = 0; ch < C; ++ch)
        for (int p = 0; p < 16; ++p) out[(size_t)p * C + ch] = w[ch * 16 + p];
}

void gsa_pack_mapping(const float* w, int L, float std, int us, float* out) {
    for (int j = 0; j < L; ++j)
        for (int k = 0; k < L; ++k) out[(size_t)k * L + j] = gsa_eff(w[(size_t)j * L + k], std, us, 0.01f);  // lr_mult 0.01, reference :135
}

}  // extern "C"
