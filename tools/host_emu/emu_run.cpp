// The stateless tile kernels on the host (tools/host_emu/hip/hip_runtime.h), one call per run, for the host sanitizers: a
// stand-alone program that reads a case from a file, calls the C entry with a null stream and writes every output to a file.  It
// holds no reference of its own: tests/test_host_emu.py builds it, writes the cases and compares the outputs with the Python rules.
//
//   g++ -std=c++20 -O1 -g -ffp-contract=off -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan \
//       -static-libubsan -I tools/host_emu -x c++ gan-segmentation_amd/csrc/gsa_boundary.hip gan-segmentation_amd/csrc/gsa_mask.hip \
//       gan-segmentation_amd/csrc/gsa_augment.hip gan-segmentation_amd/csrc/gsa_photometric.hip tools/host_emu/emu_run.cpp -o emu_asan
//   (or -fsanitize=thread -static-libtsan), then  emu_asan CASE OUTPUT
//
// A case is a text header and the input bytes:
//
//   gsa-emu-case 1
//   entry gsa_mask_morph            one of the four entries below (with -DGSA_EMU_OVERLAY and csrc/gsa_overlay.hip also gsa_overlay; with
//                                   -DGSA_EMU_REFINE and csrc/gsa_refine.hip also gsa_mask_refine; with -DGSA_EMU_RESIZE and
//                                   csrc/gsa_resize.hip also gsa_pair_resize; each without the others)
//   expect 0                        the status the entry must return
//   scalars 3 2 15 20               a count and the entry's integer arguments in order (decimal; 64-bit ones too)
//   tensors 2                       a count and one line per pointer argument, in order:
//   mask in 600 1                     name, in | out | null, bytes, address offset
//   out out 600 0
//   data
//   <the bytes of every `in` tensor, in order>
//
// Every tensor is a heap block of its own of exactly offset + bytes bytes, 64-byte aligned, and starts `offset` bytes into it, so
// one byte past its end is AddressSanitizer's to report and the offset decides the pointer's alignment.  Outputs, and the offset
// bytes in front of every tensor, are filled with kFill first; the output file holds the bytes of every tensor that is not null, in
// order, as they are after the call: the inputs too, which must come back unchanged.
// Exit status: 0 if the entry returned `expect` and no byte in front of a tensor changed, 1 otherwise, 2 for a malformed case.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gsa.h"
#include "../../include/gsa_augment.h"
#include "../../include/gsa_boundary.h"
#include "../../include/gsa_mask.h"
#include "../../include/gsa_photometric.h"
#ifdef GSA_EMU_OVERLAY      // tests/test_host_emu_overlay.py: a fifth unit, gsa_overlay.hip, linked in
#include "../../gan-segmentation_amd/csrc/gsa_overlay.h"
#endif
#ifdef GSA_EMU_REFINE       // tests/test_host_emu_refine.py: gsa_refine.hip linked in, with or without the overlay
#include "../../gan-segmentation_amd/csrc/gsa_refine.h"
#endif
#ifdef GSA_EMU_RESIZE       // tests/test_host_emu_resize.py: gsa_resize.hip linked in, with or without the other two
#include "../../gan-segmentation_amd/csrc/gsa_resize.h"
#endif

namespace {

constexpr unsigned char kFill = 0xA5;

struct Tensor {
    std::string name, kind;
    size_t bytes = 0, offset = 0;
    unsigned char* block = nullptr;
    unsigned char* at() const { return kind == "null" ? nullptr : block + offset; }
};

[[noreturn]] void malformed(const char* what) {
    fprintf(stderr, "emu_run: malformed case: %s\n", what);
    exit(2);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return fprintf(stderr, "usage: %s CASE OUTPUT\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) malformed("cannot open the case");
    char word[64], kind[8];
    int version = 0, expect = 0, count = 0;
    if (fscanf(f, "gsa-emu-case %d entry %63s expect %d scalars %d", &version, word, &expect, &count) != 4 || version != 1 || count < 0 ||
        count > 16)
        malformed("header");
    const std::string entry = word;
    std::vector<unsigned long long> s(count);
    for (auto& v : s) {
        if (fscanf(f, "%63s", word) != 1) malformed("scalar");
        v = word[0] == '-' ? (unsigned long long)strtoll(word, nullptr, 10) : strtoull(word, nullptr, 10);
    }
    if (fscanf(f, " tensors %d", &count) != 1 || count < 0 || count > 16) malformed("tensors");
    std::vector<Tensor> t(count);
    for (auto& x : t) {
        unsigned long long bytes, offset;
        if (fscanf(f, "%63s %7s %llu %llu", word, kind, &bytes, &offset) != 4) malformed("tensor line");
        x.name = word, x.kind = kind, x.bytes = bytes, x.offset = offset;
        if (x.kind != "in" && x.kind != "out" && x.kind != "null") malformed("tensor kind");
    }
    if (fscanf(f, "%63s", word) != 1 || strcmp(word, "data") || fgetc(f) != '\n') malformed("data");
    for (auto& x : t) {
        if (x.kind == "null") continue;
        void* p = nullptr;
        if (posix_memalign(&p, 64, x.offset + x.bytes ? x.offset + x.bytes : 1)) malformed("out of memory");
        x.block = (unsigned char*)p;
        memset(x.block, kFill, x.offset + x.bytes);
        if (x.kind == "in" && fread(x.at(), 1, x.bytes, f) != x.bytes) malformed("input bytes");
    }
    fclose(f);

    auto i32 = [&](size_t k) { return (int32_t)s[k]; };
    auto need = [&](size_t scalars, size_t tensors) {
        if (s.size() != scalars || t.size() != tensors) malformed("argument count");
    };
    int status;
    if (entry == "gsa_mask_morph") {
        need(3, 2);
        status = gsa_mask_morph(nullptr, i32(0), i32(1), i32(2), t[0].at(), t[1].at());
    } else if (entry == "gsa_mask_boundary") {
        need(5, 3);
        status = gsa_mask_boundary(nullptr, i32(0), i32(1), i32(2), i32(3), i32(4), t[0].at(), (int16_t*)t[1].at(), t[2].at());
    } else if (entry == "gsa_augment_pairs") {
        need(8, 7);
        status = gsa_augment_pairs(nullptr, i32(0), i32(1), i32(2), i32(3), t[0].at(), t[1].at(), (const float*)t[2].at(),
                                   (const float*)t[3].at(), (const float*)t[4].at(), i32(4), i32(5), i32(6), i32(7), t[5].at(), t[6].at());
    } else if (entry == "gsa_photometric") {
        need(6, 3);
        status = gsa_photometric(nullptr, i32(0), i32(1), i32(2), i32(3), t[0].at(), (const float*)t[1].at(), s[4], s[5], t[2].at());
#ifdef GSA_EMU_OVERLAY
    } else if (entry == "gsa_overlay") {
        need(6, 4);     // n H W channels factor cols; img mask lut out
        status = gsa_overlay(nullptr, i32(0), i32(1), i32(2), i32(3), t[0].at(), t[1].at(), t[2].at(), i32(4), i32(5), t[3].at());
#endif
#ifdef GSA_EMU_REFINE
    } else if (entry == "gsa_mask_refine") {
        need(6, 4);     // n H W channels classes radius; img mask tables out
        status = gsa_mask_refine(nullptr, i32(0), i32(1), i32(2), i32(3), i32(4), i32(5), t[0].at(), t[1].at(), t[2].at(), t[3].at());
#endif
#ifdef GSA_EMU_RESIZE
    } else if (entry == "gsa_pair_resize") {
        need(7, 4);     // n H W C h w mask_mode; img mask img_out mask_out
        status = gsa_pair_resize(nullptr, i32(0), i32(1), i32(2), i32(3), i32(4), i32(5), i32(6), t[0].at(), t[1].at(), t[2].at(), t[3].at());
#endif
    } else {
        malformed("unknown entry");
    }

    int rc = 0;
    if (status != expect) fprintf(stderr, "emu_run: %s returned %d, the case expects %d\n", entry.c_str(), status, expect), rc = 1;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return fprintf(stderr, "emu_run: cannot write %s\n", argv[2]), 2;
    for (auto& x : t) {
        for (size_t k = 0; k < x.offset && x.block; ++k)
            if (x.block[k] != kFill) {
                fprintf(stderr, "emu_run: byte %zu in front of %s was written\n", k, x.name.c_str());
                rc = 1;
                break;
            }
        if (x.block && fwrite(x.at(), 1, x.bytes, o) != x.bytes) rc = 2;
        free(x.block);
    }
    if (fclose(o)) rc = 2;
    return rc;
}
