// Kernel launch interface between the host orchestration (gsa_api.cpp) and the HIP kernels
// (gsa_kernels.hip).  Internal; the public boundary is include/gsa.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <atomic>
#include <string>

namespace gsa {

// Per-(sample, channel) AdaIN coefficients: out = fmaf(x, A, B), B = fmaf(-mean, A, beta*(ys+1)+yb)
// (InstanceNorm + style of reference networks_stylegan.py:250-264, folded; `mean` is kept for reference only).
struct Aff { float mean, A, B, pad; };

// 64-bit fixed-point partial statistics of one (sample, tile-row, channel)
struct StatPart { unsigned long long s1, s2; };

constexpr double kStatScale1 = 268435456.0;  // 2^28: quad sums
// quad sums of squares: 2^S2 with S2 = clamp(40 - ceil(log2(H*W)), 20, 26), a static function of the plane size (round 4):
// 20 at 1024^2 -- where the 64-bit sum of a plane holds rms(x) < 2.9e3 -- 22 / 24 at 512^2 / 256^2, 26 from 128^2 down.
// Small planes have few quads to average the rounding of rint(q * 2^S2) over, and E[x^2] - mean^2 must survive the cancellation
// when a plane's values sit on a bias far above their spread (device function stat_scale2 in gsa_kernels.hip; oracle: stat_scale2)

enum Epilogue { EPI_RAW = 0, EPI_SYNTH = 1, EPI_DEC = 2 };

struct ConvParams {
    int device;      // HIP device of the launching context (the launch helper keeps its state per device)
    // input: up to two NHWC sources concatenated on channels (C0 then C1), both multiples of 16
    const float* src0; const Aff* aff0; int C0;   // aff0 may be null (identity)
    const float* src1; int C1;                    // src1 may be null
    int Hs, Ws;      // spatial size of the sources
    int up;          // 1: logical input is the nearest x2 upsample of the sources
    int H, W;        // output size
    const float* wpk;   // packed weights [Cout/16][Cin/16][tap][ci][16][cg]
    const float* wino;  // or null: the same conv in Winograd F(2x2,3x3) form, U packed [Cout/16][Cin/16][f16][ci][16][cg]
                        // (F(4x4,3x3) layers, ConvForm::Wino43: [Cout/16][Cin/8][f36][kq][16][2], channel 8b + 2kq + j)
    int Cout;           // total output channels
    float* out;         // NHWC
    // EPI_SYNTH: AddNoise -> Bias -> LeakyReLU -> statistics
    const float* noise; const float* nscale; const float* nbias;
    StatPart* partials; int prow;      // prow = partial rows per sample
    // EPI_DEC: conv bias -> BatchNorm(inference) -> LeakyReLU [-> + resid], folded on the host into ONE fma per element:
    // y = lrelu(fmaf(v, bn_s, bn_beta)) with bn_s = gamma / sqrt(running_var + eps), bn_beta = fmaf(bias - running_mean, bn_s, beta)
    const float* bn_s; const float* bn_beta;
    const float* resid; int resid_up;   // resid_up: residual lives at half resolution (identity shortcut)
    const float* resid1; int res_c0;    // residual = concat(resid [res_c0 channels], resid1 [Cout - res_c0]); resid1 null: one tensor
    // fused 1x1 shortcut of DecoderResBlock (second output)
    const float* wsc; const float* sc_bias; float* out_sc;
    int tiles_x, tiles_y, groups, total_tiles;   // filled by the launcher
    int stats_direct;                            // filled by the launcher: EPI_SYNTH sums go to acc with atomics (no partial rows)
    int* stat_rows_host;                         // host pointer or null: the launcher reports the partial rows it used (0 = direct).  A host pointer has
                                                 // no business in a kernel argument; it stays because moving a field changes the argument layout of every kernel
    int w_resident;                              // filled by the launcher: whole weight panel LDS-resident (conv3x3 DB form)
    int group_minor;                             // filled by the launcher (conv3x3_wino): 1-D grid, the channel groups of a tile consecutive on one XCD
    unsigned long long* stamps;   // diagnostic build (-DGSA_STAMP) only: per-phase cycle sums
    int dbg;                      // diagnostic build only: bit0 = stage pixel 0 everywhere (timing of a cache-resident input)
    int prio;                     // experiment (GSA_PRIO): 1 = the wave OUTSIDE its MFMA phase gets the higher issue priority
    int bf16;                     // 1: bf16 MFMA mode -- wpk/wsc hold bf16 packs [..][tap][kq][16][4], operands rounded at staging
    // EPI_SYNTH in a kernel whose workgroup holds a WHOLE plane (conv3x3_ksplit at 4 and 8 px: conv_fuses_finalize): the workgroup writes
    // the AdaIN coefficients itself instead of partial rows -- the finalize launch of the layer is skipped (fin_aff null: not fused)
    const float* fin_style; int fin_style_stride; const float* fin_gamma; const float* fin_beta; Aff* fin_aff; unsigned* fin_flags;
    const float* zeros;           // >= 64 bytes of zeros in device memory: what conv3x3_wino43's LDS-DMA reads for a pixel outside the image
    // toRGB fused into the convolution that stages the SAME tensor with the SAME AdaIN (round 5: the decoder's last cvt conv reads the generator's
    // last feature, as toRGB does): rgb_img non-null = also write the uint8 image (N, H, W, 3) from the staged, AdaIN-applied tile
    const float* rgb_w; const float* rgb_b; uint8_t* rgb_img;
};

struct PostParams {
    const float* src;      // raw conv_1 output NHWC, or the constant tensor [H][W][C]
    int src_per_sample;    // 1: src indexed by sample; 0: broadcast (constant tensor)
    const float* blur;     // [C][9] or null (no blur)
    const float* noise; const float* nscale; const float* nbias;
    float* out; StatPart* partials; int prow;
    int H, W, C;
    int bf16;              // 1: the per-sample source and the output are bf16 tensors (bf16 mode)
    int row_groups;        // filled by the launcher (post_rows_kernel<4>): groups of 4 rows a thread walks
};

struct FinalizeParams {
    const StatPart* partials; int prow; int HW; int C;
    StatPart* acc;     // [n][C] zero-initialised accumulators, cleared again by finalize
    unsigned* tickets; // [n][ceil(C/64)] zero-initialised arrival counters, cleared again by finalize
    const float* style; int style_stride;  // style[n*style_stride + c] = ys, [.. + C + c] = yb
    const float* gamma; const float* beta;
    Aff* aff;   // [n][C]
    unsigned* flags;   // sticky device word or null: set to 1 when a sum is within a factor 4 of its 64-bit wrap or the variance is negative
};

// One reader for the GSA_* switches: atoi of the variable, or dflt when it is unset (set but not a number reads as 0, as atoi does).
// Each site keeps the value in a static const of its own; INTEGRATION.md lists every name read through here.
inline int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

// Each family below -- 3x3 convolutions, stride-2 layers, the post pass -- is a PLAN and a LAUNCH.  The plan is a pure host function of the
// params struct, the epilogue, the shortcut flag and, where it matters, the batch size; it returns a plain stack value that names the kernel
// form and what the form fixes.  The launch executes it and chooses no form; what depends on the batch inside a form (tile geometry,
// persistence, grid shape) stays in that form's launcher.  Whoever asks what a launch will do reads the plan, never a copy of its rule.

// launches (all stream-ordered, no sync)
// The kernel form of a 3x3 convolution, in the order the rule tries them.  Static: layer shape, arithmetic mode and switches, never the batch.
enum class ConvForm { Wino43, WinoDma, WinoTwoTiles, WinoLean, Wino, KSplit, Bf16Lean, Direct };
ConvForm conv3x3_form(const ConvParams& p, int epi, bool shortcut);
hipError_t launch_conv3x3(const ConvParams& p, int epi, bool shortcut, int n, hipStream_t s);   // executes conv3x3_form(p, epi, shortcut)
inline bool conv_form_wino(ConvForm f) { return f <= ConvForm::Wino; }      // a Winograd form: p.wino is the panel the kernel reads
// products per output and (input, output) channel pair the form executes: F(4x4,3x3) 36 per 16 outputs, F(2x2,3x3) 16 per 4, direct 9
inline double conv_form_products(ConvForm f) { return f == ConvForm::Wino43 ? 2.25 : conv_form_wino(f) ? 4 : 9; }
// The static shape rule of the Winograd forms, stated once: the commit (gsa_api.cpp) packs U by it, conv3x3_form selects the kernel by it
// plus the clauses only a launch knows.  F(2x2,3x3): fp32 mode, outputs >= 64 px, or >= 32 px with >= 64 output
// channels, or >= 16 px with >= 256 (fewer tiles leave the chip idle: the direct small-tile kernels are faster there).  F(4x4,3x3): such
// a layer with >= 64 input channels and >= 32 px.  The oracle's copy (oracle/c/gsa_oracle.c use_wino, use_wino43) stays separate on purpose.
inline bool wino_shape(int H, int Cout, int bf16) { return !bf16 && (H >= 64 || (H >= 32 && Cout >= 64) || (H >= 16 && Cout >= 256)); }
inline bool wino43_shape(int H, int Cin) { return Cin >= 64 && H >= 32; }
bool wino43_enabled();                                              // GSA_WINO43 != 0 (experiments build)
// gsa_wino_lean.hip (round 5): the Winograd layers with one 16-channel input block and one 16-channel output group in a leaner
// instruction stream -- speed only, the same arithmetic and bits as conv3x3_wino (GSA_WINO_LEAN=0 keeps conv3x3_wino)
bool wino_lean_applies(const ConvParams& p, int epi);
// ... and, inside that form, which of its two streamed-weight kernels (>= 64 input channels) a launch of n samples runs: true = the paired
// one (conv3x3_wino_stream_pair: one 8-wave workgroup stages each tile once for two output groups), when Cout % 32 == 0 and
// tiles x n x (Cout / 32) >= CUs; GSA_WINO_PAIR = 0 never, 2 wherever Cout % 32 == 0.  The one statement of the rule: the launcher asks it
bool wino_stream_paired(const ConvParams& p, int n);
hipError_t launch_wino_lean(const ConvParams& p, int epi, int n, hipStream_t s);
bool wino_lean_fuses_torgb(const ConvParams& p, int epi, int nc);      // the lean kernel's own conditions
bool conv_fuses_torgb(const ConvParams& p, int epi, bool shortcut, int nc);      // true: launch_conv3x3 on p (rgb_* set) also produces toRGB's uint8 image
// gsa_bf16_lean.hip (round 5): the bf16 mode's 3x3 convolutions from 32 px on in the lean form (GSA_BF16_LEAN=0: conv3x3_mfma<..., true>)
bool bf16_lean_applies(const ConvParams& p, int epi, bool shortcut);
hipError_t launch_bf16_lean(const ConvParams& p, int epi, int n, hipStream_t s);
// gsa_sub_lean.hip (round 5): subpixel_res<..., WINO> (fp32) in a leaner instruction stream -- speed only, same bits (GSA_SUB_LEAN=0: subpixel_res)
bool subpixel_lean_applies(const ConvParams& p, int nt, int epi, bool sc, int kb, bool wst);
hipError_t launch_subpixel_lean(const ConvParams& q, int nt, int epi, bool sc, int kb, bool wst, dim3 grid, hipStream_t s);
// The plan of a stride-2 layer (deconv4x4s2 / sub-pixel up+conv): output channels per workgroup, the path, and what the path fixes
enum class SubPath { Resident, Streamed, Plain };
struct SubpixelPlan {
    int ct;             // channel tile: 16, 32 or 64 output channels per workgroup
    SubPath path;
    bool wino;          // subpixel_uses_wino
    int kb;             // Resident: channel blocks per item (1 or 2); Streamed: 1
    size_t lds;         // Resident, Streamed: bytes of dynamic LDS (Plain: its launcher computes them)
    int wgs_per_group;  // Streamed: workgroups per channel group
};
SubpixelPlan subpixel_plan(const ConvParams& p, bool shortcut, int n);
hipError_t launch_subpixel(const ConvParams& p, int epi, bool shortcut, int n, hipStream_t s);   // executes subpixel_plan(p, shortcut, n)
bool subpixel_uses_wino(const ConvParams& p);                      // true: Winograd F(2x2,2x2) form (static rule: fp32 mode): 9 products per 2x2 class outputs instead of 16
// The plan of the post pass: the kernel, rows per thread, row groups per thread (post_rows_kernel<4>), workgroups per sample, and the
// statistic partial rows per sample they write.  (The small planes of post_fuses_finalize go through launch_post_fin instead.)
enum class PostKind { Dma, Packed, Rows, OneRow };
struct PostPlan { PostKind kind; int rpt, row_groups, blocks, rows_used; };
PostPlan post_plan(const PostParams& p);
hipError_t launch_post(const PostParams& p, int n, hipStream_t s);      // executes post_plan(p)
// gsa_post_lean.hip (round 5): post_rows_kernel<4> in packed fp32 arithmetic (same bits).  GSA_POST_PK: 0 = off, 1 = packed (default), 2 = + non-temporal stores
int post_pk_mode();
bool post_dma_applies(const PostParams& p);      // GSA_POST_DMA: the LDS-DMA ring form (16 / 32 channels, fp32, blurred)
int post_dma_band(const PostParams& p);
int post_dma_blocks(const PostParams& p);
hipError_t launch_post_dma(const PostParams& p, int n, hipStream_t s);
hipError_t launch_post_pk(const PostParams& q, dim3 grid, size_t lds, hipStream_t s);
hipError_t launch_finalize(const FinalizeParams& p, int n, hipStream_t s);
bool conv_fuses_finalize(const ConvParams& p, int epi, bool shortcut);   // true: launch_conv3x3 writes the layer's AdaIN coefficients itself when p.fin_aff is set (whole-plane K-split tiles)
bool post_fuses_finalize(const PostParams& p);      // true: launch_post_fin does the post pass AND the finalize of this plane in one launch (planes <= 32 x 32)
hipError_t launch_post_fin(const PostParams& p, const FinalizeParams& f, int n, hipStream_t s);
hipError_t launch_pixelnorm(const float* z, float* out, int n, int L, hipStream_t s);
// PixelNorm + the eight mapping layers in one launch (result in lat[0]); mapping_fused: whether it applies to this latent size
constexpr int kMapSlices = 8;     // most sample slices of the fused mapping network (launch-number words ctl[2 .. 2 + kMapSlices))
bool mapping_fused(int L, int device);
hipError_t launch_mapping(const float* z, float* const* wt, float* const* b, unsigned long long* const* ll, float* out, unsigned* ctl,
                          int n, int L, int device, hipStream_t s, int drop_workgroups = 0);   // drop_workgroups: fault injection (tests)
hipError_t launch_dense(const float* x, const float* WT, const float* b, float* y, int n, int K, int J,
                        int lrelu, hipStream_t s);
hipError_t launch_styles(const float* w, const float* avg, const float* psi, const float* WT, const float* b,
                         const int* col_layer, float* styles, int n, int K, int J, hipStream_t s);
// gsa_wspace.hip: the same styles from per-layer dlatents (N, NL, K); tiles[i] = {layer, first column, columns <= 64, 0}
hipError_t launch_styles_dlatents(const float* dlatents, const float* avg, const float* psi, const float* WT, const float* b,
                                  const int4* tiles, int num_tiles, float* styles, int n, int K, int J, int NL, hipStream_t s);
hipError_t launch_torgb(const float* x, const Aff* aff, const float* w, const float* b, float* rgb,
                        uint8_t* img, int n, int H, int W, int C, int nc, int bf16, hipStream_t s);
// gsa_downscale.hip: the image and the mask at 1/f resolution (f in {2, 4, 8}): toRGB's u reduced over each
// f x f block in the quad-tree order (img: (N, H/f, W/f, nc) u8), and the final conv's per-class block sums -> argmax (mask: (N, H/f, W/f))
hipError_t launch_torgb_down(const float* x, const Aff* aff, const float* w, const float* b, uint8_t* img, int n, int H, int W, int C,
                             int nc, int f, int bf16, hipStream_t s);
hipError_t launch_final_conv_down(const float* src0, int C0, const float* src1, int C1, const float* wpk, const float* bias, uint8_t* mask,
                                  int n, int H, int W, int ncls, int f, int bf16, hipStream_t s);
hipError_t launch_export_nchw(const float* x, const Aff* aff, float* out, int n, int H, int W, int C, int bf16, hipStream_t s);
hipError_t launch_import_nhwc(const float* in, float* out, int n, int H, int W, int C, int bf16, hipStream_t s);
hipError_t launch_final_conv(const float* src0, int C0, const float* src1, int C1, const float* wpk,
                             const float* bias, float* logits, uint8_t* mask, int n, int H, int W, int ncls, int bf16,
                             hipStream_t s);

// geometry the launchers pick (weights are packed per 16 output channels, so it is free to vary)
int conv_stat_rows(int H, int W, int Cout, int n);   // statistic partial rows per sample written by conv3x3 EPI_SYNTH
int post_prow(int H, int W, int C);                  // ... written by the post kernel (upper bound: the one-row form)
int post_rows_used(const PostParams& p);             // ... by post_plan(p)
hipError_t launch_fill_normal(float* out, int per_sample, int n, unsigned long long first_index, unsigned plane,
                              unsigned long long seed, hipStream_t s);
hipError_t launch_seg_eval(const float* logits, const int8_t* labels, int n, int classes, int H, int W,
                           unsigned long long* confusion, unsigned long long* loss_fixed, hipStream_t s);

// ---- launch helper of the generate path (gsa_kernels.hip, gsa_*_lean.hip) --------------------------------------------------
// The first use of a kernel on a device allows it the whole 160 KB of LDS (less its static LDS); the CU count and the occupancy
// answers are kept per device.  A process may hold contexts on several GPUs (ImageGenerator(gpu_ids=[0, 1, ...]), reference
// image_generator.py:17): one mutex makes the first-use path safe for the "one context per (device, host thread)" contract of
// include/gsa.h.  A device outside [0, kMaxDevices) is hipErrorInvalidDevice.  After the first use a launch takes no lock.
constexpr int kMaxDevices = 64;
int device_cus(int device);       // CU count (256 when the runtime cannot say)
int current_device();             // the calling thread's device, for the launchers whose parameters carry none (-1: unknown)
hipError_t allow_max_lds(const void* kern);
hipError_t cached_occupancy(const void* kern, int device, int block, size_t lds, int* wgs_per_cu);
void note_launch(const void* kern);
// what the calling thread launched through launch() since the last call (the profiler's label): the last kernel and the count
struct LaunchRecord { const void* kern = nullptr; int count = 0; };
LaunchRecord take_launch_record();
std::string kernel_name(const void* kern);     // the demangled C++ signature, as rocprofv3 prints it

template <auto K>
hipError_t prepare_kernel(int device) {
    static std::atomic<uint64_t> ready{0};     // one bit per device
    if (device < 0 || device >= kMaxDevices) return hipErrorInvalidDevice;
    if (ready.load(std::memory_order_acquire) >> device & 1) return hipSuccess;
    if (hipError_t e = allow_max_lds(reinterpret_cast<const void*>(K))) return e;
    ready.fetch_or(1ull << device, std::memory_order_release);
    return hipSuccess;
}

// resident workgroups per CU of K with `block` threads and `lds` bytes of dynamic LDS, clamped to 1..8 (cached)
template <auto K>
hipError_t kernel_occupancy(int device, int block, size_t lds, int* wgs_per_cu) {
    if (hipError_t e = prepare_kernel<K>(device)) return e;
    return cached_occupancy(reinterpret_cast<const void*>(K), device, block, lds, wgs_per_cu);
}

template <auto K, class... Args>
hipError_t launch(int device, dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
    if (hipError_t e = prepare_kernel<K>(device)) return e;
    hipLaunchKernelGGL(K, grid, block, lds, s, args...);
    note_launch(reinterpret_cast<const void*>(K));
    return hipGetLastError();
}

}  // namespace gsa
