// mm_jpeg_entropy.h -- one segment of a baseline JPEG scan (a file, or one restart interval of it) from bytes to quantised coefficients:
// the bit reader, the Huffman code lookup and the block loop of mm_jpeg_decode.hip, as plain C++.  MM_HD is __host__ __device__ under
// hipcc and empty otherwise, so the same text compiles into the kernel and into tools/jpeg_entropy_check.cpp, the stand-alone host program
// the damaged-stream tests run.
//
// Total by construction: for ANY bytes, any tables and any segment record that passed the library's checks, nothing is read outside
// bytes[begin, end) or the tables, and nothing is written outside the count * per blocks of the segment's MCU range -- every index comes
// from a loop counter held below 64 or is masked, never from the stream alone.
//   reader   bytes[begin, end), most significant bit first.  FF 00 is a data FF; FF FF.. are fill bytes; FF followed by anything else, a
//            lone FF at the end, and the end itself stop the reader: from there it supplies zero bits.  A symbol that needed any of
//            those zero bits sets MM_JPEG_ST_OVERRUN; bits a segment leaves unused are ignored, as libjpeg ignores them.
//   codes    per table MM_JPEG_TABLE_WORDS 32-bit words: 512 look-ahead entries of 16 bits, length << 8 | symbol for the codes of up to 9
//            bits (0: longer), two to a word, entry i in the low half of word i / 2 when i is even; then libjpeg's maxcode[0..17]
//            (-1: no code of that length), valoffset[0..17] (index of the length's first symbol minus its first code) and the 256
//            symbols, four to a word, lowest byte first.  A code of more than 16 bits (none matches) is MM_JPEG_ST_BAD_CODE.
//   block    DC: category s <= 11 (else MM_JPEG_ST_BAD_SIZE), s more bits, EXTEND, added to the component's predictor (0 at the segment's
//            start; kept as an int16).  AC from k = 1: run << 4 | size; size 0 is ZRL for run 15 (k += 16; beyond coefficient 63:
//            MM_JPEG_ST_BAD_RUN) and EOB otherwise; size > 10: BAD_SIZE; k += run, beyond 63: BAD_RUN; the value goes to coefficient k
//            (zigzag order) as one 2-byte store.  Zeros are not stored: the buffer was zeroed.
// The first status that is not 0 ends the segment; what it had stored stays, the rest of its coefficients stay zero.
#ifndef MM_JPEG_ENTROPY_H
#define MM_JPEG_ENTROPY_H

#if defined(__HIPCC__)
#define MM_HD __host__ __device__
#else
#define MM_HD
#endif

#define MM_JPEG_ST_OVERRUN 1
#define MM_JPEG_ST_BAD_CODE 2
#define MM_JPEG_ST_BAD_RUN 4
#define MM_JPEG_ST_BAD_SIZE 8

#define MM_JPEG_TABLE_WORDS 356         /* 256 look-ahead + 18 maxcode + 18 valoffset + 64 symbols */
#define MM_JPEG_TABLE_MAXCODE 256
#define MM_JPEG_TABLE_VALOFF 274
#define MM_JPEG_TABLE_SYMBOLS 292

namespace mm {

struct JpegBits {
    const unsigned char* bytes;
    int pos, end;                       // the next byte and the segment's end
    unsigned long long acc;             // the low n bits are unread
    int n, pad;                         // pad: how many of them are zeros supplied past the stop (always the lowest)
    bool stop;
};

// at least 57 unread bits: a code (16) and its value bits (11) never refill in between
MM_HD inline void jpeg_bits_fill(JpegBits& b) {
    while (b.n <= 56) {
        unsigned c = 0;
        if (!b.stop && b.pos < b.end) {
            c = b.bytes[b.pos++];
            if (c == 0xFFu) {
                while (b.pos < b.end && b.bytes[b.pos] == 0xFFu) ++b.pos;       // fill bytes
                if (b.pos < b.end && b.bytes[b.pos] == 0u) ++b.pos;             // stuffed: a data FF
                else { b.stop = true; c = 0; }                                  // a marker, or the end after FF
            }
        } else {
            b.stop = true;
        }
        if (b.stop) b.pad += 8;
        b.acc = (b.acc << 8) | c;
        b.n += 8;
    }
}

MM_HD inline bool jpeg_bits_overrun(const JpegBits& b) { return b.n < b.pad; }

// s unread bits (1..11), after jpeg_decode_symbol's fill
MM_HD inline int jpeg_bits_get(JpegBits& b, int s) {
    b.n -= s;
    return (int)(b.acc >> b.n) & ((1 << s) - 1);
}

// T.81 F.2.2.1 EXTEND: s bits as a signed value
MM_HD inline int jpeg_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// the next symbol of table t, or -1: no code of up to 16 bits matches (or the look-ahead entry is not a length of 1..9)
MM_HD inline int jpeg_decode_symbol(JpegBits& b, const unsigned* t) {
    jpeg_bits_fill(b);
    const unsigned peek = (unsigned)(b.acc >> (b.n - 16)) & 0xFFFFu;
    const unsigned i = peek >> 7, e = (t[i >> 1] >> (16 * (i & 1u))) & 0xFFFFu, len = e >> 8;
    if (len >= 1 && len <= 9) { b.n -= (int)len; return (int)(e & 0xFFu); }
    if (len != 0) return -1;
    for (int l = 10; l <= 16; ++l) {
        const int code = (int)(peek >> (16 - l));
        if (code <= (int)t[MM_JPEG_TABLE_MAXCODE + l]) {
            const unsigned at = (unsigned)(code + (int)t[MM_JPEG_TABLE_VALOFF + l]) & 0xFFu;
            b.n -= l;
            return (int)((t[MM_JPEG_TABLE_SYMBOLS + (at >> 2)] >> (8 * (at & 3u))) & 0xFFu);
        }
    }
    return -1;
}

// one block into block[0..63] (zeroed before); pred: its component's DC predictor.  0, or the status that ends the segment
MM_HD inline int jpeg_decode_block(JpegBits& b, const unsigned* dc, const unsigned* ac, int& pred, short* block) {
    int s = jpeg_decode_symbol(b, dc);
    if (s < 0) return MM_JPEG_ST_BAD_CODE;
    if (s > 11) return MM_JPEG_ST_BAD_SIZE;
    int diff = 0;
    if (s) diff = jpeg_extend(jpeg_bits_get(b, s), s);
    if (jpeg_bits_overrun(b)) return MM_JPEG_ST_OVERRUN;
    pred = (int)(short)(pred + diff);
    if (pred != 0) block[0] = (short)pred;
    for (int k = 1; k < 64;) {
        const int rs = jpeg_decode_symbol(b, ac);
        if (rs < 0) return MM_JPEG_ST_BAD_CODE;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (jpeg_bits_overrun(b)) return MM_JPEG_ST_OVERRUN;
            if (r != 15) break;                                                 // EOB
            if (k + 16 > 64) return MM_JPEG_ST_BAD_RUN;
            k += 16;                                                            // ZRL
            continue;
        }
        if (s > 10) return MM_JPEG_ST_BAD_SIZE;
        k += r;
        if (k > 63) return MM_JPEG_ST_BAD_RUN;
        const int v = jpeg_extend(jpeg_bits_get(b, s), s);
        if (jpeg_bits_overrun(b)) return MM_JPEG_ST_OVERRUN;
        block[k++] = (short)v;
    }
    return 0;
}

// count MCUs of per blocks each (the first luma of them component 0, then one block each of components 1 and 2) from bytes[begin, end)
// into coef[count * per][64].  tables: four tables, DC 0, DC 1, AC 0, AC 1; sel: bit 2c picks component c's DC table, bit 2c + 1 its AC
// table.  Returns the segment's status.
MM_HD inline int jpeg_decode_segment(const unsigned char* bytes, int begin, int end, const unsigned* tables, unsigned sel, int per, int luma,
                                     int count, short* coef) {
    JpegBits b = {bytes, begin, end, 0ull, 0, 0, false};
    int p0 = 0, p1 = 0, p2 = 0;                                                 // (three names, not an array: a runtime index would put it in scratch)
    for (int m = 0; m < count; ++m) {
        for (int j = 0; j < per; ++j) {
            const int c = j < luma ? 0 : j - luma + 1;
            const unsigned* dc = tables + ((sel >> (2 * c)) & 1u) * MM_JPEG_TABLE_WORDS;
            const unsigned* ac = tables + (2u + ((sel >> (2 * c + 1)) & 1u)) * MM_JPEG_TABLE_WORDS;
            int pred = c == 0 ? p0 : (c == 1 ? p1 : p2);
            const int st = jpeg_decode_block(b, dc, ac, pred, coef + ((long long)m * per + j) * 64);
            if (st) return st;
            if (c == 0) p0 = pred; else if (c == 1) p1 = pred; else p2 = pred;
        }
    }
    return 0;
}

}  // namespace mm
#endif
