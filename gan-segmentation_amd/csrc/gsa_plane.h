// gsa_plane.h -- what the stateless u8 plane operations share: the tile decomposition of gsa_mask.hip,
// gsa_boundary.hip, gsa_components.hip and gsa_stats.hip, the "four pixels of a row" load and store, and the entry checks of those
// four and gsa_photometric.hip.  Internal to csrc/; included after <hip/hip_runtime.h> (or its host stand-in), which supplies
// __device__, __forceinline__ and blockIdx.  No __shared__ memory, no launch.
//
// load_px4 / store_px4 are what a new plane kernel should use and what mask_morph_kernel uses.  mask_boundary_kernel,
// label_tiles_kernel and pair_stats_kernel keep the hand-written loads they had: through load_px4 their code differed from the
// measured one by a few instructions and came out 0.2 to 1.5 % slower on the MI355X (DESIGN.md section 20 has the runs).
//
// The tile constants (kTileW, kTileH, kThreads ...) are facts of each kernel and stay in its unit.  Two differences between the
// entries are deliberate and are NOT evened out here: gsa_mask_morph and gsa_mask_boundary refuse a call of kMaxWorkgroups tiles or
// more, gsa_mask_components and gsa_pair_stats split it (for_each_launch); and gsa_mask_morph alone takes planes of 2^31 pixels
// and more (extent_ok, not extent_ok_31).  load4 / load_window of gsa_photometric.hip and gsa_augment.hip clamp against the whole
// batch, not against a row: another rule, they stay where they are.
#pragma once
#include <cstdint>

namespace gsa {
namespace plane {

// ---- device side ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned byte_of(unsigned w, int b) { return (w >> (8 * b)) & 255u; }
__device__ __forceinline__ unsigned pack4(const unsigned (&o)[4]) { return o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24); }

// The workgroup's plane and its tile in it, for a 1-D grid of planes x tiles_per_plane workgroups.  Uniform over the workgroup.
struct Tile {
    int plane, tile, tile_y, tile_x;
};
__device__ __forceinline__ Tile tile_of(int tiles_x, int tiles_per_plane) {
    const int plane = blockIdx.x / tiles_per_plane;
    const int tile = blockIdx.x - plane * tiles_per_plane;
    const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    return {plane, tile, tile_y, tile_x};
}

// The pixels gx .. gx + 3 of a row of W, one per byte; 0 for every column outside [0, W) -- gx may be negative (an apron).
// ALIGNED (W % 4 == 0, gx % 4 == 0, a 4-byte aligned plane): one dword, inside or outside as a whole.  Whether the row itself
// lies inside the image is the caller's to decide.
template <bool ALIGNED>
__device__ __forceinline__ unsigned load_px4(const uint8_t* row, int gx, int W) {
    unsigned v = 0;
    if (ALIGNED) {
        if ((unsigned)gx < (unsigned)W) v = *reinterpret_cast<const unsigned*>(row + gx);
    } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if ((unsigned)(gx + b) < (unsigned)W) v |= (unsigned)row[gx + b] << (8 * b);
    }
    return v;
}

// The mirror image for 0 <= gx < W: the bytes of v to the pixels gx .. gx + 3 of a row, those inside [0, W) only.
template <bool ALIGNED>
__device__ __forceinline__ void store_px4(uint8_t* row, int gx, int W, unsigned v) {
    uint8_t* q = row + gx;
    if (ALIGNED) {
        *reinterpret_cast<unsigned*>(q) = v;
    } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (gx + b < W) q[b] = (uint8_t)byte_of(v, b);
    }
}

// ---- host side: the entry checks ----------------------------------------------------------------------------------------------------
constexpr int kMaxExtent = 65535;
constexpr long long kMaxWorkgroups = 1ll << 24;    // a launch takes FEWER than this many workgroups of 256: HIP takes fewer than 2^32 threads

inline bool extent_ok(int H, int W) { return H >= 1 && W >= 1 && H <= kMaxExtent && W <= kMaxExtent; }
inline bool extent_ok_31(int H, int W) { return extent_ok(H, W) && (long long)H * W < (1ll << 31); }     // plane-local indices are ints

inline bool ranges_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
    return p < q + b_bytes && q < p + a_bytes;
}

struct TileGrid {
    long long tiles_x, tiles_y, per_plane;
};
inline TileGrid tile_grid(int H, int W, int tile_w, int tile_h) {
    const long long tiles_x = (W + tile_w - 1) / tile_w, tiles_y = (H + tile_h - 1) / tile_h;
    return {tiles_x, tiles_y, tiles_x * tiles_y};
}

// fn(first_plane, planes) for consecutive groups of the n planes, each of as many planes as one launch of blocks_per_plane
// workgroups a plane can take (1 <= blocks_per_plane < kMaxWorkgroups).
template <class F>
void for_each_launch(long long n, long long blocks_per_plane, F fn) {
    const long long planes_per_launch = (kMaxWorkgroups - 1) / blocks_per_plane;
    for (long long first = 0; first < n; first += planes_per_launch) fn(first, n - first < planes_per_launch ? n - first : planes_per_launch);
}

}  // namespace plane
}  // namespace gsa
