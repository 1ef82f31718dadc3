// gsa_resize.hip -- the kernel of the pair resize (gsa_resize.h): a u8 image batch and / or a u8 mask batch
// shrunk to any smaller-or-equal size; the image by the exact area mean, the mask by an area vote over the nine slots or by nearest
// sampling.  All integers.
//
// One launch, no workspace, no atomics.  A workgroup of 256 threads owns a tile of kTileW x kTileH = 32 x 8 output pixels, a thread
// one of them.  The tile's source window -- at most 32 * 16 + 1 columns and 8 * 16 + 1 rows -- is staged to LDS in chunks of source
// rows, each source byte read from memory once per tile that covers it (a source row or column on a tile seam twice); a chunk holds
// as many rows as fit 24 KiB of image and 6 KiB of mask, which is the whole window of a tile at FFHQ's ratios and 11 rows at the
// limits (ratio 16, four channels).  The chunk's dwords, image and mask, are ONE index space that the threads walk eight loads at a
// time, all in flight before the first goes to LDS: a tile is a few KiB, and what it waits for is the latency of its loads, not their
// number.  After the barrier a thread walks the taps of its output pixel that lie in the chunk: the row weight once per source row,
// the column weight once per tap, and per tap C multiply-adds into u32 channel sums.  The vote keeps ONE sum while every tap so far
// held the same slot -- most output pixels lie inside a region -- and nine selected adds into u32 slot sums from the first tap that
// differs; a wave none of whose pixels straddles a boundary never runs the nine.  Every product has factors below 2^24
// (v_mul_u32_u24, full rate; v_mul_lo_u32 runs at a quarter): a tap's weight wr * wc can BE 2^24, so it is never a factor -- the
// image forms (wr * pixel) * wc.  The sums are bounded by the rule's totals (255 * H * W < 2^32 and
// H * W <= 2^24), so no partial sum can overflow either.
//
// The taps are walked in two dimensions, not separably.  Shrinking by r, a separable form pays r * (r + 1) horizontal taps and r + 1
// vertical ones per output pixel -- every source row needs its own horizontal pass -- against (r + 1)^2 here: the same work, with
// a second LDS array and a second barrier per chunk on top.
//
// The division by H * W happens once per output value: a float estimate of the quotient (at most 255, so within one of the truth)
// and one exact integer correction step, which makes the result the rule's whatever the float rounding was.
//
// Global access: the staging reads whole dwords when the plane's address and its row pitch are multiples of 4 (every generated pair)
// -- the dwords that cover the window's bytes, which lie inside the row because the row's ends are aligned -- and bytes otherwise.
// Outputs are byte stores: an output row of a tile is 32 * C bytes at an address with no alignment to speak of.
// No wave intrinsics and no cross-lane moves: the unit runs on the host stand-in as well.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gsa.h"
#include "gsa_plane.h"
#include "gsa_resize.h"

namespace {

using namespace gsa::plane;

constexpr int kThreads = 256;
constexpr int kTileW = 32;                      // output pixels of a workgroup: 32 x 8, a thread one of them
constexpr int kTileH = 8;
constexpr int kSlots = 9;                       // slot(v) = min(v, 8)
constexpr unsigned kNoSlot = 255;               // no tap seen yet
constexpr int kMaxRatio = GSA_RESIZE_MAX_RATIO;
constexpr int kMaxChannels = 4;
constexpr unsigned kImgWords = 6144;            // staged image rows: 24 KiB
constexpr unsigned kMaskWords = 1536;           // staged mask rows: 6 KiB
constexpr unsigned kMaxWindowW = kTileW * kMaxRatio + 1;        // 513 source columns under a tile
// a staged row: the dwords that cover the window's bytes, which may start up to 3 bytes into the first one
constexpr unsigned kMaxImgRowWords = (3 + kMaxWindowW * kMaxChannels + 3) / 4;
constexpr unsigned kMaxMaskRowWords = (3 + kMaxWindowW + 3) / 4;

static_assert(kTileW * kTileH == kThreads, "a thread owns one output pixel");
static_assert(kImgWords >= kMaxImgRowWords && kMaskWords >= kMaxMaskRowWords, "a chunk holds at least one row of the widest window");
static_assert(255ull * GSA_RESIZE_MAX_PIXELS + (GSA_RESIZE_MAX_PIXELS >> 1) < (1ull << 32), "the image's numerator fits 32 bits");

enum { kNoMask = 0, kVote = 1, kNearest = 2 };

__device__ __forceinline__ unsigned umin(unsigned a, unsigned b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }

// num / d for num < 2^32, 1 <= d <= 2^24 and a quotient of at most 255; rcp = 1.0f / d.  The estimate's error is below 2^-14, so
// its floor is within one of the quotient and one step either way corrects it.
__device__ __forceinline__ unsigned div_small(unsigned num, unsigned d, float rcp) {
    unsigned q = (unsigned)((float)num * rcp);
    const unsigned qd = q * d;                  // q <= 255: no overflow
    if (qd > num) return q - 1;
    return num - qd >= d ? q + 1 : q;
}

// idx / d for idx < 2^16 and 1 <= d < 2^16, rcp = 1.0f / d: the half added keeps the estimate clear of both neighbours (its
// error is below idx * 2^-22, the margin is 1 / (2 d)).
__device__ __forceinline__ unsigned div_index(unsigned idx, float rcp) { return (unsigned)(((float)idx + 0.5f) * rcp); }

// How the rows of one input's window go to LDS.  In the dword form a unit is a dword, a staged row `per_row` = `words` of them, and
// unit idx of a chunk lands at lds[idx]; in the byte form a unit is a byte, a row `per_row` = the window's bytes, at the start of the
// row's `words` dwords.  `first` is the window's first byte in a source row, less the bytes that the dword form starts early.
struct Staging {
    const uint8_t* plane;
    unsigned* lds;
    size_t pitch;
    unsigned first, words, per_row;
    float rcp;                                  // 1.0f / per_row
    bool aligned;
};

struct Unit {
    unsigned r, k, v;
};

__device__ __forceinline__ Unit load_unit(const Staging& s, unsigned yc, unsigned idx) {
    Unit u;
    u.r = div_index(idx, s.rcp);
    u.k = idx - u.r * s.per_row;
    const uint8_t* row = s.plane + (size_t)(yc + u.r) * s.pitch + s.first;
    u.v = s.aligned ? reinterpret_cast<const unsigned*>(row)[u.k] : (unsigned)row[u.k];
    return u;
}

__device__ __forceinline__ void store_unit(const Staging& s, unsigned idx, const Unit& u) {
    if (s.aligned)
        s.lds[idx] = u.v;
    else
        reinterpret_cast<uint8_t*>(s.lds + u.r * s.words)[u.k] = (uint8_t)u.v;
}

// Rows yc .. yc + nr - 1 of both windows into LDS: the units of the image's rows and then of the mask's as ONE index space that the
// 256 threads walk kBatch units a thread at a time, every load of a batch issued before its first store -- the loads of a chunk are
// in flight together, not one row after the other.
template <bool IMG, bool VOTE>
__device__ __forceinline__ void stage_chunk(const Staging& si, const Staging& sm, unsigned yc, unsigned nr) {
    constexpr unsigned kBatch = 8;
    const unsigned n_img = IMG ? nr * si.per_row : 0u, total = n_img + (VOTE ? nr * sm.per_row : 0u);
    for (unsigned base = threadIdx.x; base < total; base += kBatch * kThreads) {
        Unit u[kBatch];
#pragma unroll
        for (unsigned b = 0; b < kBatch; ++b) {
            const unsigned idx = base + b * kThreads;
            if (idx >= total) break;
            if (IMG && (!VOTE || idx < n_img))
                u[b] = load_unit(si, yc, idx);
            else
                u[b] = load_unit(sm, yc, idx - n_img);
        }
#pragma unroll
        for (unsigned b = 0; b < kBatch; ++b) {
            const unsigned idx = base + b * kThreads;
            if (idx >= total) break;
            if (IMG && (!VOTE || idx < n_img))
                store_unit(si, idx, u[b]);
            else
                store_unit(sm, idx - n_img, u[b]);
        }
    }
}

template <int C, int MASK>
__global__ __launch_bounds__(kThreads) void pair_resize_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask,
                                                               uint8_t* __restrict__ img_out, uint8_t* __restrict__ mask_out, int H, int W, int h,
                                                               int w, int tiles_x, int tiles_per_plane, int img_aligned, int mask_aligned) {
    constexpr bool IMG = C > 0, VOTE = MASK == kVote, NEAREST = MASK == kNearest;
    constexpr unsigned CH = IMG ? C : 1;
    __shared__ unsigned lds_img[IMG ? kImgWords : 1];
    __shared__ unsigned lds_mask[VOTE ? kMaskWords : 1];
    const Tile tl = tile_of(tiles_x, tiles_per_plane);                  // uniform over the workgroup
    const unsigned uH = (unsigned)H, uW = (unsigned)W, uh = (unsigned)h, uw = (unsigned)w;      // products of two sides fit 32 bits: 65535^2 < 2^32
    const unsigned i0 = (unsigned)tl.tile_y * kTileH, j0 = (unsigned)tl.tile_x * kTileW;
    const unsigned i_end = umin(i0 + kTileH, uh), j_end = umin(j0 + kTileW, uw);
    // the source window of the tile
    const unsigned y_lo = i0 * uH / uh, y_hi = (i_end * uH - 1) / uh;  // y_hi <= H - 1
    const unsigned x_lo = j0 * uW / uw, x_hi = (j_end * uW - 1) / uw;
    const unsigned nx = x_hi - x_lo + 1, ny = y_hi - y_lo + 1;          // nx <= 513
    const uint8_t* __restrict__ plane_i = IMG ? img + (size_t)tl.plane * uH * uW * CH : nullptr;
    const uint8_t* __restrict__ plane_m = MASK != kNoMask ? mask + (size_t)tl.plane * uH * uW : nullptr;

    const unsigned img_first = x_lo * CH, img_bytes = nx * CH;
    const unsigned img_shift = img_aligned ? img_first & 3u : 0u, img_words = (img_shift + img_bytes + 3u) / 4u;
    const unsigned mask_shift = mask_aligned ? x_lo & 3u : 0u, mask_words = (mask_shift + nx + 3u) / 4u;
    const unsigned img_per_row = img_aligned ? img_words : img_bytes, mask_per_row = mask_aligned ? mask_words : nx;
    const Staging stage_i = {plane_i, lds_img, (size_t)uW * CH, img_first - img_shift, img_words, img_per_row, 1.0f / (float)img_per_row, img_aligned != 0};
    const Staging stage_m = {plane_m, lds_mask, (size_t)uW, x_lo - mask_shift, mask_words, mask_per_row, 1.0f / (float)mask_per_row, mask_aligned != 0};
    unsigned rows = ny;                         // source rows of a chunk
    if (IMG) rows = umin(rows, kImgWords / img_words);
    if (VOTE) rows = umin(rows, kMaskWords / mask_words);

    // the thread's output pixel and its taps
    const unsigned i = i0 + threadIdx.x / kTileW, j = j0 + threadIdx.x % kTileW;
    const bool active = i < uh && j < uw;
    unsigned ys = 1, ye = 0, xs = 0, xe = 0, iH = 0, jW = 0;
    if (active) {
        iH = i * uH, jW = j * uW;
        ys = iH / uh, ye = (iH + uH - 1) / uh;
        xs = jW / uw, xe = (jW + uW - 1) / uw;
    }
    unsigned S[CH] = {}, A[kSlots] = {};
    // the vote while every tap so far held one slot: that slot and its area.  Most output pixels lie inside a region and never leave
    // this state; the first tap of another slot moves the area to the slot's sum, and the nine sums take over.
    unsigned lone = kNoSlot, lone_area = 0;
    bool mixed = false;

    // the sampled mask reads its one pixel from memory: without an image and a vote nothing is staged and no barrier is met
    for (unsigned yc = y_lo; (IMG || VOTE) && yc <= y_hi; yc += rows) {  // uniform
        const unsigned nr = umin(rows, y_hi - yc + 1);
        if (yc != y_lo) __syncthreads();                                // the chunk before has been read
        stage_chunk<IMG, VOTE>(stage_i, stage_m, yc, nr);
        __syncthreads();
        if (!active) continue;
        const unsigned ya = umax(ys, yc), yb = umin(ye, yc + nr - 1);
        for (unsigned y = ya; y <= yb; ++y) {
            const unsigned yh = __umul24(y, uh), wr = umin(iH + uH, yh + uh) - umax(iH, yh);      // every factor here fits 24 bits
            const uint8_t* pi = IMG ? reinterpret_cast<const uint8_t*>(lds_img + (y - yc) * img_words) + img_shift + (xs - x_lo) * CH : nullptr;
            const uint8_t* pm = VOTE ? reinterpret_cast<const uint8_t*>(lds_mask + (y - yc) * mask_words) + mask_shift + (xs - x_lo) : nullptr;
            unsigned xw = __umul24(xs, uw);
            for (unsigned x = xs; x <= xe; ++x, xw += uw) {
                const unsigned wc = umin(jW + uW, xw + uw) - umax(jW, xw);
                // wr, wc < 2^16, so their product is exact -- but it REACHES 2^24 (an identity on both axes of a plane of 2^24 pixels)
                // and is then no 24-bit factor: the image multiplies the pixel in first, wr * pixel < 2^24, and the weight is only added
                const unsigned wgt = __umul24(wr, wc);                                  // <= h * w <= 2^24
                if (IMG) {
#pragma unroll
                    for (unsigned c = 0; c < CH; ++c) S[c] += __umul24(__umul24(wr, pi[c]), wc);
                    pi += CH;
                }
                if (VOTE) {
                    const unsigned slot = umin(*pm++, (unsigned)(kSlots - 1));
                    if (lone == kNoSlot) lone = slot;
                    if (!mixed && slot == lone) {
                        lone_area += wgt;
                    } else {
                        if (!mixed) {
                            mixed = true;
#pragma unroll
                            for (unsigned s = 0; s < (unsigned)kSlots; ++s) A[s] = lone == s ? lone_area : 0u;
                        }
#pragma unroll
                        for (unsigned s = 0; s < (unsigned)kSlots; ++s) A[s] += slot == s ? wgt : 0u;
                    }
                }
            }
        }
    }
    if (!active) return;                        // no barrier follows

    const size_t o = ((size_t)tl.plane * uh + i) * uw + j;
    if (IMG) {
        const unsigned hw = uH * uW;
        const float rcp = 1.0f / (float)hw;
#pragma unroll
        for (unsigned c = 0; c < CH; ++c) img_out[o * CH + c] = (uint8_t)div_small(S[c] + (hw >> 1), hw, rcp);
    }
    if (VOTE) {
        unsigned best = lone, area = A[0];
        if (mixed) {
            best = 0;
#pragma unroll
            for (unsigned s = 1; s < (unsigned)kSlots; ++s)
                if (A[s] > area) area = A[s], best = s;                 // strictly more: a tie stays with the lowest slot
        }
        mask_out[o] = (uint8_t)(best == (unsigned)(kSlots - 1) ? 255u : best);
    }
    if (NEAREST) mask_out[o] = plane_m[(size_t)ys * uW + xs];
}

using Kernel = void (*)(const uint8_t*, const uint8_t*, uint8_t*, uint8_t*, int, int, int, int, int, int, int, int);

template <int C>
Kernel kernel_of(int mask) {
    return mask == kVote ? pair_resize_kernel<C, kVote> : mask == kNearest ? pair_resize_kernel<C, kNearest> : pair_resize_kernel<C, kNoMask>;
}
Kernel kernel_of(int channels, int mask) {      // channels 0: no image, and then a mask
    return channels == 0   ? (mask == kVote ? pair_resize_kernel<0, kVote> : pair_resize_kernel<0, kNearest>)
           : channels == 1 ? kernel_of<1>(mask)
           : channels == 2 ? kernel_of<2>(mask)
           : channels == 3 ? kernel_of<3>(mask)
                           : kernel_of<4>(mask);
}

}  // namespace

extern "C" {

int gsa_pair_resize(void* stream, int32_t n, int32_t H, int32_t W, int32_t C, int32_t h, int32_t w, int32_t mask_mode, const uint8_t* img,
                    const uint8_t* mask, uint8_t* img_out, uint8_t* mask_out) {
    if (n == 0) return GSA_OK;
    if (n < 0 || !extent_ok(H, W) || h < 1 || w < 1 || h > H || w > W || (long long)H > (long long)kMaxRatio * h ||
        (long long)W > (long long)kMaxRatio * w || (long long)H * W > GSA_RESIZE_MAX_PIXELS || C < 1 || C > kMaxChannels ||
        (mask_mode != GSA_RESIZE_VOTE && mask_mode != GSA_RESIZE_NEAREST))
        return GSA_ERR_INVALID;
    const bool has_img = img && img_out, has_mask = mask && mask_out;
    if ((img != nullptr) != (img_out != nullptr) || (mask != nullptr) != (mask_out != nullptr) || (!has_img && !has_mask)) return GSA_ERR_INVALID;
    const uint64_t src = (uint64_t)n * H * W, dst = (uint64_t)n * h * w;
    if (has_img && (ranges_overlap(img_out, dst * C, img, src * C) || (has_mask && ranges_overlap(img_out, dst * C, mask, src)))) return GSA_ERR_INVALID;
    if (has_mask && (ranges_overlap(mask_out, dst, mask, src) || (has_img && ranges_overlap(mask_out, dst, img, src * C)))) return GSA_ERR_INVALID;
    if (has_img && has_mask && ranges_overlap(img_out, dst * C, mask_out, dst)) return GSA_ERR_INVALID;

    const TileGrid g = tile_grid(h, w, kTileW, kTileH);                 // fewer than 2^17 tiles a plane: h * w <= 2^24
    const Kernel kernel = kernel_of(has_img ? C : 0, !has_mask ? kNoMask : mask_mode == GSA_RESIZE_VOTE ? kVote : kNearest);
    // a dword form per input: the plane's address and its row pitch multiples of 4, and then every plane's and every row's
    const int img_aligned = has_img && (reinterpret_cast<uintptr_t>(img) & 3) == 0 && ((long long)W * C) % 4 == 0;
    const int mask_aligned = has_mask && (reinterpret_cast<uintptr_t>(mask) & 3) == 0 && W % 4 == 0;
    for_each_launch(n, g.per_plane, [&](long long first, long long planes) {    // split, not refused
        const size_t so = (size_t)first * H * W, to = (size_t)first * h * w;
        hipLaunchKernelGGL(kernel, dim3((unsigned)(planes * g.per_plane)), dim3(kThreads), 0, (hipStream_t)stream, has_img ? img + so * C : nullptr,
                           has_mask ? mask + so : nullptr, has_img ? img_out + to * C : nullptr, has_mask ? mask_out + to : nullptr, (int)H, (int)W,
                           (int)h, (int)w, (int)g.tiles_x, (int)g.per_plane, img_aligned, mask_aligned);
    });
    return hipGetLastError() == hipSuccess ? GSA_OK : GSA_ERR_HIP;
}

}  // extern "C"
