// jpeg_entropy_check.cpp -- the segment decoder of the JPEG file decoder (csrc/mm_jpeg_entropy.h, the very text the kernel compiles) as a
// stand-alone host program, so that damaged streams can be run under the host sanitizers:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I 3d-magic-mirror_amd/csrc tools/jpeg_entropy_check.cpp -o check
//     ./check forms.bin > result.txt
//
// forms.bin (32-bit little-endian words; tests/test_jpeg_decode_host.py writes it): n_bytes, n_tables, n_blocks, n_forms; the base bytes
// (padded to a word); n_tables x MM_JPEG_TABLE_WORDS table words; then per form: length (the form is the first `length` base bytes),
// n_edits, n_segments; n_edits x {position, value}; n_segments x {first block, MCU count, byte begin, byte end, blocks per MCU, luma blocks,
// selector bits, table DC 0, DC 1, AC 0, AC 1}.  Every form gets heap buffers of exactly its bytes and exactly n_blocks blocks, so a read or
// a write outside them is the sanitizer's to report.  Per form one line goes to stdout: the segments' statuses, then a checksum of the coefficient buffer (hex): the sum
// over i of (coefficient i as uint16 + 1) * (i * 0x9E3779B97F4A7C15 + 1), modulo 2^64.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "mm_jpeg_entropy.h"

static std::vector<uint32_t> read_words(const char* path) {
    std::vector<uint32_t> w;
    FILE* f = fopen(path, "rb");
    if (!f) return w;
    uint32_t buf[4096];
    size_t got;
    while ((got = fread(buf, 4, 4096, f)) > 0) w.insert(w.end(), buf, buf + got);
    fclose(f);
    return w;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s forms.bin\n", argv[0]); return 2; }
    const std::vector<uint32_t> w = read_words(argv[1]);
    size_t at = 0;
    auto next = [&]() -> int64_t { if (at >= w.size()) { fprintf(stderr, "forms.bin is truncated\n"); exit(2); } return (int32_t)w[at++]; };
    const int64_t n_bytes = next(), n_tables = next(), n_blocks = next(), n_forms = next();
    if (n_bytes < 0 || n_tables < 1 || n_blocks < 1 || n_forms < 0 || at + (size_t)(n_bytes + 3) / 4 + (size_t)n_tables * MM_JPEG_TABLE_WORDS > w.size()) {
        fprintf(stderr, "forms.bin: a bad header\n");
        return 2;
    }
    const unsigned char* base = (const unsigned char*)&w[at];
    at += (size_t)(n_bytes + 3) / 4;
    const uint32_t* tables = &w[at];
    at += (size_t)n_tables * MM_JPEG_TABLE_WORDS;
    std::vector<unsigned> set(4 * MM_JPEG_TABLE_WORDS);
    for (int64_t f = 0; f < n_forms; ++f) {
        const int64_t length = next(), n_edits = next(), n_segments = next();
        if (length < 0 || length > n_bytes) { fprintf(stderr, "form %lld: a bad length\n", (long long)f); return 2; }
        std::unique_ptr<unsigned char[]> bytes(new unsigned char[length ? length : 1]);
        memcpy(bytes.get(), base, (size_t)length);
        for (int64_t e = 0; e < n_edits; ++e) {
            const int64_t pos = next(), val = next();
            if (pos < 0 || pos >= length) { fprintf(stderr, "form %lld: a bad edit\n", (long long)f); return 2; }
            bytes[pos] = (unsigned char)val;
        }
        std::unique_ptr<short[]> coef(new short[(size_t)n_blocks * 64]());
        for (int64_t s = 0; s < n_segments; ++s) {
            int64_t v[11];
            for (int k = 0; k < 11; ++k) v[k] = next();
            const int64_t first = v[0], count = v[1], begin = v[2], end = v[3], per = v[4], luma = v[5];
            // what the library's own checks hold a segment record to
            if (first < 0 || count < 0 || per < 1 || per > 6 || luma < 1 || luma > per || first + count * per > n_blocks || begin < 0 || end < begin || end > length) {
                fprintf(stderr, "form %lld: a bad segment\n", (long long)f);
                return 2;
            }
            for (int k = 0; k < 4; ++k) {
                if (v[7 + k] < 0 || v[7 + k] >= n_tables) { fprintf(stderr, "form %lld: a bad table\n", (long long)f); return 2; }
                memcpy(&set[(size_t)k * MM_JPEG_TABLE_WORDS], tables + (size_t)v[7 + k] * MM_JPEG_TABLE_WORDS, 4 * MM_JPEG_TABLE_WORDS);
            }
            const int st = mm::jpeg_decode_segment(bytes.get(), (int)begin, (int)end, set.data(), (unsigned)v[6], (int)per, (int)luma, (int)count,
                                                   coef.get() + (size_t)first * 64);
            printf("%d ", st);
        }
        uint64_t h = 0;
        for (size_t i = 0; i < (size_t)n_blocks * 64; ++i) h += ((uint64_t)(uint16_t)coef[i] + 1) * ((uint64_t)i * 0x9E3779B97F4A7C15ull + 1);
        printf("%016llx\n", (unsigned long long)h);
    }
    return 0;
}
