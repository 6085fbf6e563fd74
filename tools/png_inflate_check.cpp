// png_inflate_check.cpp -- the inflate of the PNG file decoder (csrc/mm_inflate.h, the very text the kernel compiles, its lane-cooperative
// copies and table builder run serially: one lane) as a stand-alone host program, so that damaged streams can be run under the host sanitizers:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I 3d-magic-mirror_amd/csrc tools/png_inflate_check.cpp -o check
//     ./check corpus_dir > result.txt
//
// corpus_dir (tests/test_png_decode_host.py writes it) holds 000000.bin, 000001.bin, ... without a gap; each is 4 bytes S (little-endian)
// and the raw deflate stream.  Every stream gets heap buffers of exactly its bytes and exactly S zeroed bytes, so a read or a write outside
// them is the sanitizer's to report.  Per stream one line goes to stdout: the status, then a checksum of the S bytes (hex): the sum over i
// of (byte i + 1) * (i * 0x9E3779B97F4A7C15 + 1), modulo 2^64.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "mm_inflate.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s corpus_dir\n", argv[0]); return 2; }
    std::unique_ptr<mm::InfShared> sh(new mm::InfShared());
    for (int k = 0;; ++k) {
        char path[4096];
        snprintf(path, sizeof path, "%s/%06d.bin", argv[1], k);
        FILE* f = fopen(path, "rb");
        if (!f) return k ? 0 : 2;
        std::vector<unsigned char> all;
        unsigned char buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, f)) > 0) all.insert(all.end(), buf, buf + got);
        fclose(f);
        if (all.size() < 4) { fprintf(stderr, "%s: too short\n", path); return 2; }
        const uint32_t S = all[0] | all[1] << 8 | all[2] << 16 | (uint32_t)all[3] << 24;
        const size_t n = all.size() - 4;
        if (S > (1u << 30) || n > (1u << 30)) { fprintf(stderr, "%s: too large\n", path); return 2; }
        std::unique_ptr<unsigned char[]> in(new unsigned char[n ? n : 1]);
        memcpy(in.get(), all.data() + 4, n);
        std::unique_ptr<unsigned char[]> out(new unsigned char[S ? S : 1]());
        const int st = mm::inflate_stream(in.get(), 0, (int)n, out.get(), (int)S, sh.get());
        uint64_t h = 0;
        for (size_t i = 0; i < S; ++i) h += ((uint64_t)out[i] + 1) * ((uint64_t)i * 0x9E3779B97F4A7C15ull + 1);
        printf("%d %016llx\n", st, (unsigned long long)h);
    }
}
