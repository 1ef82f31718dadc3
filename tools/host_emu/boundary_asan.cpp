// gsa_mask_boundary on the host (tools/host_emu/hip/hip_runtime.h), for AddressSanitizer and UBSan: every shape of the GPU tests at
// radii across the four apron sizes, with an aligned and an odd mask address, all three output forms, on heap buffers of exactly the
// size the header asks for -- and every result compared with a brute-force search of the window.  A stand-alone program:
//
//   g++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -I tools/host_emu \
//       -x c++ gan-segmentation_amd/csrc/gsa_boundary.hip tools/host_emu/boundary_asan.cpp -o boundary_asan && ./boundary_asan
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/gsa_boundary.h"

static int brute(const uint8_t* m, int H, int W, int y, int x, int R) {
    int best = GSA_BOUNDARY_FAR;
    for (int yy = y - R < 0 ? 0 : y - R; yy <= y + R && yy < H; ++yy)
        for (int xx = x - R < 0 ? 0 : x - R; xx <= x + R && xx < W; ++xx)
            if (m[yy * W + xx] != m[y * W + x]) {
                const int d = (yy - y) * (yy - y) + (xx - x) * (xx - x);
                if (d <= R * R && d < best) best = d;
            }
    return best;
}

int main() {
    const int shapes[][3] = {{1, 1, 1},   {1, 1, 70},   {1, 70, 1},   {1, 16, 16},  {1, 63, 65},  {1, 64, 64},
                             {1, 65, 63}, {1, 130, 67}, {1, 131, 66}, {3, 40, 72}, {1, 129, 129}};
    const int radii[] = {1, 2, 4, 5, 8, 9, 16, 17, 31, 32};
    unsigned seed = 1;
    long checked = 0;
    for (auto& s : shapes)
        for (int R : radii)
            for (int off = 0; off < 2; ++off) {                         // off = 1: an odd mask address, the byte path
                const int n = s[0], H = s[1], W = s[2];
                const size_t px = (size_t)n * H * W;
                uint8_t* buf = (uint8_t*)malloc(px + off);
                uint8_t* m = buf + off;
                for (size_t i = 0; i < px; ++i) {                       // blocks of three values, 255 among them, and some noise
                    seed = seed * 1664525u + 1013904223u;
                    const size_t y = i / W % H, x = i % W;
                    m[i] = (seed >> 27) == 0 ? 7 : ((y / 11 + x / 13) % 3 == 0 ? 255 : (y / 11 + x / 13) % 3);
                }
                int16_t* d = (int16_t*)malloc(px * 2);
                int16_t* d2 = (int16_t*)malloc(px * 2);
                uint8_t* o = (uint8_t*)malloc(px);
                uint8_t* o2 = (uint8_t*)malloc(px);
                int rc = gsa_mask_boundary(nullptr, n, H, W, R, 9, m, d, o);
                rc |= gsa_mask_boundary(nullptr, n, H, W, R, 9, m, nullptr, o2);
                rc |= gsa_mask_boundary(nullptr, n, H, W, R, 9, m, d2, nullptr);
                if (rc) return printf("status %d at %d x %d x %d, R %d\n", rc, n, H, W, R), 1;
                for (int p = 0; p < n; ++p)
                    for (int y = 0; y < H; ++y)
                        for (int x = 0; x < W; ++x, ++checked) {
                            const size_t at = ((size_t)p * H + y) * W + x;
                            const int want = brute(m + (size_t)p * H * W, H, W, y, x, R);
                            const uint8_t band = want == GSA_BOUNDARY_FAR ? m[at] : 9;
                            if (d[at] != want || d2[at] != want || o[at] != band || o2[at] != band)
                                return printf("%d x %d x %d, R %d, offset %d: (%d, %d, %d) is %d / %d, rule %d\n", n, H, W, R, off, p, y, x,
                                              d[at], o[at], want), 1;
                        }
                free(buf), free(d), free(d2), free(o), free(o2);
            }
    printf("clean: %ld pixels equal to the brute-force rule\n", checked);
    return 0;
}
