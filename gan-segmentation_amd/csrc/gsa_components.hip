// gsa_components.hip -- the mask components' kernels (include/gsa_components.h): labels (smallest raster
// index of the component), areas, the area-threshold filter and the per-sample summary rows of every (H, W) u8 plane.
//
// A data-dependent union-find, unlike the fixed-shape stencils and reductions beside it.  ONE invariant carries every phase:
// labels[x] <= x at all times (plane-local raster indices; a pixel's label is its parent, a root has labels[x] == x), and a word
// is only ever lowered (atomic minimum) -- the larger of two roots is linked under the smaller.  So every walk from a pixel to its
// root and every retry of a union visits strictly decreasing indices: all loops are bounded by the data, none waits for a value
// that another workgroup has yet to write, and the root a component ends with is its smallest raster index whatever the order of
// arrival.  The caller's labels and areas are the only working storage.
//
// Four launches on the caller's stream, no grid-wide barrier:
//   1 label_tiles    a workgroup labels one kTileW x kTileH tile in LDS (horizontal runs per thread, then lock-free unions with LDS
//                    atomic minima) and counts the pixels of every tile component in LDS.  It writes plane-global labels -- every
//                    pixel points straight at its TILE ROOT, the first pixel of its tile component --, areas = that count at a tile
//                    root and 0 everywhere else, and (the plane's first tile) zeroes the summary row.
//   2 merge_seams    a thread per pixel on a tile's top or left edge unions it with its equal-valued neighbours across the seam;
//                    a pair whose union follows from the seam pixel before it and the two tiles' own labelling is skipped.  Only
//                    words of tile roots are ever lowered.  Workgroups on different XCDs touch the same words in this launch and
//                    the XCDs' L2s are not coherent for plain accesses, so EVERY labels access of this phase is an agent-scope
//                    atomic (relaxed load / fetch_min).  A stale guess of a root costs an iteration; the value the atomic returns
//                    is the truth.
//   3 flatten_count  the tile roots (areas != 0) walk to their root, store it and add their tile's count into areas[root]: one
//                    atomic per tile component, not per pixel or wave -- a component that spans the image is hit once per tile.
//                    Roots count their component into the row.  A walker may pass through a word while its owner replaces the
//                    parent by the root: either value is an ancestor, so the walk ends at the same root.
//   4 spread_filter  a pixel reads its tile root's label, now the root r, keeps it, and areas[p] = areas[r].  Words of tile roots
//                    (labels) and of roots (areas) are final and only read; every other word is written by its own thread and read
//                    by nobody else -- no thread reads a word that another writes.  Then out, then the largest areas and the
//                    small-component words.
//
// Launch boundaries order the phases: what one launch wrote with atomics the next reads with plain loads.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gsa.h"
#include "../../include/gsa_components.h"
#include "gsa_plane.h"

namespace {

using namespace gsa::plane;

constexpr int kThreads = 256;
constexpr int kTileW = 64;                      // a tile row is one wave's worth of labels: 256 contiguous bytes
constexpr int kTileH = 64;                      // 4096 pixels: 16 KB of labels, 16 KB of counts, 4 KB of values in LDS; 16 px per thread
constexpr int kSeg = 16;                        // pixels of a thread's horizontal segment in the first pass
constexpr int kTilePix = kTileW * kTileH;
constexpr int kPerThread = kTilePix / kThreads;
constexpr int kSameRootRounds = 4;              // phase 1: shared roots a wave counts with one LDS atomic each before lanes add alone
constexpr int kBlockPix = 16 * kThreads;        // phases 3 and 4: consecutive pixels of a workgroup, 16 per thread.  A workgroup sends its
                                                // partial row words on with a few atomics, and atomics on one row's cache line run one
                                                // after the other chip-wide (measured: DESIGN.md section 17) -- few, fat workgroups

static_assert(kPerThread == kSeg && kTileW % kSeg == 0 && kThreads == kTileH * (kTileW / kSeg), "a thread per 16-px row segment");
static_assert(kTileW % 4 == 0, "dword loads of a segment");

__device__ __forceinline__ int slot_of(unsigned v) { return v < 8u ? (int)v : 8; }

// ---- union-find on an LDS tile (workgroup scope) --------------------------------------------------------------------------------
// Terminates: lab[x] <= x always, so x strictly decreases until lab[x] == x; at most x steps.
__device__ __forceinline__ int find_lds(const int* lab, int x) {
    int p;
    while ((p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != x) x = p;
    return x;
}

// Terminates: every pass either ends (the roots met, or the larger root was still a root and now hangs under the smaller) or
// replaces the larger index a by the value the atomic returned, old < a, while b only decreases: max(a, b) strictly decreases.
__device__ __forceinline__ void union_lds(int* lab, int a, int b) {
    while (true) {
        a = find_lds(lab, a);
        b = find_lds(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(lab + a, b);
        if (old == a) return;
        a = old;                                // a had a parent already (old < a): what is left to join is old with b
    }
}

// ---- union-find on a plane in global memory (agent scope) -------------------------------------------------------------------------
// Terminates: labels[x] <= x always and words are only lowered, so x strictly decreases until a word equals its index.
__device__ __forceinline__ int find_global(int* labels, int x) {
    int p;
    while ((p = __hip_atomic_load(labels + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != x) x = p;
    return x;
}

// Terminates: as union_lds -- max(a, b) strictly decreases with every pass that does not end; no pass waits for another thread.
__device__ __forceinline__ void union_global(int* labels, int a, int b) {
    while (true) {
        a = find_global(labels, a);
        b = find_global(labels, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(labels + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}

// ---- phase 1 ------------------------------------------------------------------------------------------------------------------
template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void label_tiles_kernel(const uint8_t* __restrict__ mask, int* __restrict__ labels,
                                                               int* __restrict__ areas, long long* __restrict__ rows, int H, int W,
                                                               int tiles_x, int tiles_per_plane, int conn8) {
    __shared__ int lab[kTilePix];
    __shared__ int cnt[kTilePix];               // pixels of the tile component whose local root is the index; 0 elsewhere
    __shared__ unsigned val4[kTilePix / 4];     // the tile's values, one byte per pixel; 0 outside the image (never compared)
    const uint8_t* val = reinterpret_cast<const uint8_t*>(val4);
    const Tile t = tile_of(tiles_x, tiles_per_plane);                   // uniform over the workgroup
    const int y0 = t.tile_y * kTileH, x0 = t.tile_x * kTileW;
    const size_t base = (size_t)t.plane * H * W;                        // every image is a plane of its own
    const uint8_t* __restrict__ pm = mask + base;
    int* __restrict__ pl = labels + base;
    int* __restrict__ pa = areas + base;

    if (rows && t.tile == 0 && threadIdx.x < GSA_COMP_ROW) rows[(size_t)t.plane * GSA_COMP_ROW + threadIdx.x] = 0;

    // pass 1: a thread loads its 16-px row segment and labels every pixel with the start of its horizontal run inside the segment
    {
        const int ly = threadIdx.x / (kTileW / kSeg), lx0 = (threadIdx.x % (kTileW / kSeg)) * kSeg;
        const int gy = y0 + ly, gx0 = x0 + lx0;
        unsigned w[kSeg / 4] = {};
        if (gy < H) {
            const uint8_t* p = pm + (size_t)gy * W;
#pragma unroll
            for (int d = 0; d < kSeg / 4; ++d) {
                const int gx = gx0 + 4 * d;
                if (ALIGNED) {                  // W % 4 == 0: a dword is inside as a whole or not at all
                    if (gx < W) w[d] = *reinterpret_cast<const unsigned*>(p + gx);
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (gx + b < W) w[d] |= (unsigned)p[gx + b] << (8 * b);
                }
            }
        }
        const int i0 = ly * kTileW + lx0;
        int run = i0;
        unsigned prev = 0;
#pragma unroll
        for (int k = 0; k < kSeg; ++k) {
            const unsigned v = byte_of(w[k >> 2], k & 3);
            if (k == 0 || v != prev) run = i0 + k;
            lab[i0 + k] = run;
            cnt[i0 + k] = 0;
            prev = v;
        }
#pragma unroll
        for (int d = 0; d < kSeg / 4; ++d) val4[(i0 >> 2) + d] = w[d];
    }
    __syncthreads();

    // pass 2: unions with the equal-valued neighbours that precede a pixel inside the tile -- the left one where a segment begins,
    // the one above, and with 8-connectivity the two diagonals above.  Lock-free: no barrier between the pixels of a thread.
    for (int k = 0; k < kPerThread; ++k) {
        const int i = k * kThreads + threadIdx.x;
        const int ly = i / kTileW, lx = i % kTileW;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        const unsigned v = val[i];
        if (lx > 0 && lx % kSeg == 0 && val[i - 1] == v) union_lds(lab, i, i - 1);
        if (ly > 0) {
            if (val[i - kTileW] == v) union_lds(lab, i, i - kTileW);
            if (conn8) {
                if (lx > 0 && val[i - kTileW - 1] == v) union_lds(lab, i, i - kTileW - 1);
                if (lx + 1 < kTileW && gx + 1 < W && val[i - kTileW + 1] == v) union_lds(lab, i, i - kTileW + 1);
            }
        }
    }
    __syncthreads();

    // pass 3: the tile's roots as plane-global raster indices (local raster order is global raster order, so the smallest local
    // index of a tile component is its smallest global one), and the tile components' pixel counts.  A wave is one tile row here:
    // the lanes that share a root count once, for the first kSameRootRounds roots of the row; the lanes left after that add alone.
    // A fixed number of rounds: no loop over the data.
    for (int k = 0; k < kPerThread; ++k) {
        const int i = k * kThreads + threadIdx.x;
        const int gy = y0 + i / kTileW, gx = x0 + i % kTileW;
        const bool live = gy < H && gx < W;
        int r = -1;
        if (live) {
            r = find_lds(lab, i);
            pl[(long long)gy * W + gx] = (int)((long long)(y0 + r / kTileW) * W + x0 + r % kTileW);      // < H * W < 2^31
        }
        bool pending = live;
#pragma unroll
        for (int round = 0; round < kSameRootRounds; ++round) {
            const unsigned long long todo = __ballot(pending);
            if (!todo) break;                   // uniform
            const int src = __ffsll((long long)todo) - 1;
            const int rr = __builtin_amdgcn_readlane(r, src);
            const bool mine = pending && r == rr;
            const unsigned long long same = __ballot(mine);
            if ((int)(threadIdx.x & 63) == src) atomicAdd(&cnt[rr], (int)__popcll(same));
            if (mine) pending = false;
        }
        if (pending) atomicAdd(&cnt[r], 1);
    }
    __syncthreads();
    for (int k = 0; k < kPerThread; ++k) {
        const int i = k * kThreads + threadIdx.x;
        const int gy = y0 + i / kTileW, gx = x0 + i % kTileW;
        if (gy < H && gx < W) pa[(long long)gy * W + gx] = cnt[i];
    }
}

// ---- phase 2 ------------------------------------------------------------------------------------------------------------------
// A thread per seam pixel of a plane: first the (tiles_y - 1) * W pixels of the rows y = k * kTileH, then the (tiles_x - 1) * H
// pixels of the columns x = k * kTileW.  A top-edge pixel joins up, up-left and up-right; a left-edge pixel joins left, up-left and
// down-left (the up-right pair of the pixel below-left, whose tile ends there): every neighbour pair that crosses a seam is covered.
// Skipped, because phase 1 has joined what lies inside one tile: a diagonal whose far end sits beside the straight neighbour in the
// same tile, both of the value; and the straight pair itself where the seam pixel before this one, in the same two tiles, holds the
// same pair of values -- it makes the union (or skips it for the same reason: the first pixel of such a run along the seam never skips).
__global__ __launch_bounds__(kThreads) void merge_seams_kernel(const uint8_t* __restrict__ mask, int* labels, int H, int W, int tiles_y,
                                                               int blocks_per_plane, int conn8) {
    const int plane = blockIdx.x / blocks_per_plane;
    const long long t = (long long)(blockIdx.x - plane * blocks_per_plane) * kThreads + threadIdx.x;
    const long long n_top = (long long)(tiles_y - 1) * W;
    const size_t base = (size_t)plane * H * W;
    const uint8_t* __restrict__ pm = mask + base;
    int* pl = labels + base;
    int y, x;
    bool top;
    if (t < n_top) {
        y = (int)(t / W + 1) * kTileH;
        x = (int)(t % W);
        top = true;
    } else {
        const long long u = t - n_top;
        x = (int)(u / H + 1) * kTileW;
        y = (int)(u % H);
        top = false;
        if (x >= W) return;                     // past the last seam pixel of the plane
    }
    const long long p = (long long)y * W + x;
    const unsigned v = pm[p];
    if (top) {                                  // y >= kTileH; the seam runs along x
        const uint8_t* up = pm + p - W;
        const bool tile_left = x % kTileW != 0, tile_right = x % kTileW != kTileW - 1;       // p +- 1 lies in p's tile
        const bool u0 = up[0] == v, ul = x > 0 && up[-1] == v, ur = x + 1 < W && up[1] == v;
        if (u0 && !(tile_left && ul && pm[p - 1] == v)) union_global(pl, (int)p, (int)(p - W));
        if (conn8) {
            if (ul && !(u0 && tile_left)) union_global(pl, (int)p, (int)(p - W - 1));
            if (ur && !(u0 && tile_right)) union_global(pl, (int)p, (int)(p - W + 1));
        }
    } else {                                    // x >= kTileW; the seam runs along y
        const bool tile_up = y % kTileH != 0, tile_down = y % kTileH != kTileH - 1;          // p -+ W lies in p's tile
        const bool l0 = pm[p - 1] == v, lu = y > 0 && pm[p - W - 1] == v, ld = y + 1 < H && pm[p + W - 1] == v;
        if (l0 && !(tile_up && lu && pm[p - W] == v)) union_global(pl, (int)p, (int)(p - 1));
        if (conn8) {
            if (lu && !(l0 && tile_up)) union_global(pl, (int)p, (int)(p - W - 1));
            if (ld && !(l0 && tile_down)) union_global(pl, (int)p, (int)(p + W - 1));
        }
    }
}

// ---- phase 3 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void flatten_count_kernel(const uint8_t* __restrict__ mask, int* labels, int* areas,
                                                                 long long* __restrict__ rows, int HW, int blocks_per_plane) {
    __shared__ int ncomp[GSA_COMP_SLOTS];
    const int plane = blockIdx.x / blocks_per_plane;
    const long long p0 = (long long)(blockIdx.x - plane * blocks_per_plane) * kBlockPix + threadIdx.x;
    const size_t base = (size_t)plane * HW;
    int* pl = labels + base;
    int* pa = areas + base;
    if (threadIdx.x < GSA_COMP_SLOTS) ncomp[threadIdx.x] = 0;
    __syncthreads();
    for (long long p = p0; p < p0 + kBlockPix && p < HW; p += kThreads) {
        // a tile root holds its tile component's count, every other pixel 0.  A root's word may be growing under other tile roots'
        // adds while it is read here: it only grows, so "not 0" holds, and a root does not use the value.
        const int c = __hip_atomic_load(pa + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c != 0) {
            const int r = find_global(pl, (int)p);
            if (r != (int)p) {
                // the owner's store: a walker that passes through this word reads the old parent or the root, both ancestors of p
                __hip_atomic_store(pl + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(pa + r, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else if (rows) {
                atomicAdd(&ncomp[slot_of(mask[base + p])], 1);
            }
        }
    }
    if (rows) {
        __syncthreads();
        if (threadIdx.x < GSA_COMP_SLOTS && ncomp[threadIdx.x] != 0)
            __hip_atomic_fetch_add(rows + (size_t)plane * GSA_COMP_ROW + GSA_COMP_NCOMP + threadIdx.x, (long long)ncomp[threadIdx.x],
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- phase 4 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void spread_filter_kernel(const uint8_t* __restrict__ mask, int* labels, int* areas, uint8_t* __restrict__ out, long long* __restrict__ rows,
                                                                 int W, int HW, int blocks_per_plane, int min_area, int fill) {
    __shared__ int largest[GSA_COMP_SLOTS];
    __shared__ int small_count;
    __shared__ unsigned long long small_pixels;
    const int plane = blockIdx.x / blocks_per_plane;
    const long long p0 = (long long)(blockIdx.x - plane * blocks_per_plane) * kBlockPix + threadIdx.x;
    const size_t base = (size_t)plane * HW;
    const uint8_t* __restrict__ pm = mask + base;
    if (threadIdx.x < GSA_COMP_SLOTS) largest[threadIdx.x] = 0;
    if (threadIdx.x == 0) small_count = 0, small_pixels = 0;
    __syncthreads();
    for (long long p = p0; p < p0 + kBlockPix && p < HW; p += kThreads) {
        const int t = labels[base + p];         // p's tile root, or already the root where p is a tile root itself
        const int r = labels[base + t];         // a tile root's word: flattened by phase 3, nobody writes it in this launch
        if (r != t) labels[base + p] = r;       // then p is no tile root: nobody else reads or writes its word
        const int a = areas[base + r];          // a root's word: nobody writes it in this launch
        const unsigned v = pm[p];
        if (r != (int)p) {
            areas[base + p] = a;                // a non-root's word: nobody else reads or writes it
        } else if (rows) {
            atomicMax(&largest[slot_of(v)], a);
            if (a < min_area) {
                atomicAdd(&small_count, 1);
                atomicAdd(&small_pixels, (unsigned long long)a);
            }
        }
        if (out) {
            unsigned o = v;
            if (a < min_area) {
                if (fill >= 0) o = (unsigned)fill;
                else if (r % W != 0) o = pm[r - 1];
                else if (r >= W) o = pm[r - W];
            }
            out[base + p] = (uint8_t)o;
        }
    }
    if (rows) {
        __syncthreads();
        long long* __restrict__ row = rows + (size_t)plane * GSA_COMP_ROW;
        // the word only grows: a value that does not exceed what it holds already need not be sent
        if (threadIdx.x < GSA_COMP_SLOTS && largest[threadIdx.x] != 0 &&
            __hip_atomic_load(row + GSA_COMP_LARGEST + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (long long)largest[threadIdx.x])
            __hip_atomic_fetch_max(row + GSA_COMP_LARGEST + threadIdx.x, (long long)largest[threadIdx.x], __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        if (threadIdx.x == 0 && small_count != 0) {
            __hip_atomic_fetch_add(row + GSA_COMP_SMALL, (long long)small_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(row + GSA_COMP_SMALL_PIXELS, (long long)small_pixels, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

extern "C" {

int gsa_mask_components(void* stream, int32_t n, int32_t H, int32_t W, int32_t connectivity, int32_t min_area, int32_t fill,
                        const uint8_t* mask, int32_t* labels, int32_t* areas, uint8_t* out, int64_t* rows) {
    if (n < 0 || !extent_ok_31(H, W)) return GSA_ERR_INVALID;
    if ((connectivity != 4 && connectivity != 8) || min_area < 0 || fill < GSA_COMP_FILL_NEIGHBOUR || fill > 255) return GSA_ERR_INVALID;
    if (n == 0) return GSA_OK;
    if (!mask || !labels || !areas) return GSA_ERR_INVALID;
    const uint64_t plane_px = (uint64_t)H * (uint64_t)W, bytes = (uint64_t)n * plane_px;        // n * H * W in 64 bits
    if (out && ranges_overlap(mask, bytes, out, bytes)) return GSA_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int HW = (int)plane_px, conn8 = connectivity == 8;
    const TileGrid g = tile_grid(H, W, kTileW, kTileH);
    const int tiles_x = (int)g.tiles_x, tiles_y = (int)g.tiles_y;
    const long long tiles = g.per_plane;                                                // workgroups of phase 1, per plane
    const long long seam_px = (long long)(tiles_y - 1) * W + (long long)(tiles_x - 1) * H;
    const long long seam_blocks = (seam_px + kThreads - 1) / kThreads;                   // phase 2; 0: one tile, nothing to merge
    const long long px_blocks = ((long long)HW + kBlockPix - 1) / kBlockPix;             // phases 3 and 4; at most 2^19
    long long most = tiles > px_blocks ? tiles : px_blocks;                             // tiles <= 2^10 * 2^10 + ... : far below 2^24
    if (seam_blocks > most) most = seam_blocks;
    if (most >= kMaxWorkgroups) return GSA_ERR_INVALID;
    const auto label_tiles = W % 4 == 0 && (reinterpret_cast<uintptr_t>(mask) & 3) == 0 ? label_tiles_kernel<true> : label_tiles_kernel<false>;
    const dim3 block(kThreads);
    for_each_launch(n, most, [&](long long first, long long planes) {      // split, not refused
        const size_t off = (size_t)first * plane_px;
        const uint8_t* mk = mask + off;
        int* lb = labels + off;
        int* ar = areas + off;
        uint8_t* ot = out ? out + off : nullptr;
        long long* rw = rows ? reinterpret_cast<long long*>(rows) + first * GSA_COMP_ROW : nullptr;
        hipLaunchKernelGGL(label_tiles, dim3((unsigned)(planes * tiles)), block, 0, s, mk, lb, ar, rw, H, W, tiles_x, (int)tiles, conn8);
        if (seam_blocks > 0)
            hipLaunchKernelGGL(merge_seams_kernel, dim3((unsigned)(planes * seam_blocks)), block, 0, s, mk, lb, H, W, tiles_y,
                               (int)seam_blocks, conn8);
        const dim3 grid_px((unsigned)(planes * px_blocks));
        hipLaunchKernelGGL(flatten_count_kernel, grid_px, block, 0, s, mk, lb, ar, rw, HW, (int)px_blocks);
        hipLaunchKernelGGL(spread_filter_kernel, grid_px, block, 0, s, mk, lb, ar, ot, rw, W, HW, (int)px_blocks,
                           (int)min_area, (int)fill);
    });
    return hipGetLastError() == hipSuccess ? GSA_OK : GSA_ERR_HIP;
}

}  // extern "C"
