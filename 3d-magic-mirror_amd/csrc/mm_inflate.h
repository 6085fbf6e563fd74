// mm_inflate.h -- one raw deflate stream (RFC 1951: a PNG file's IDAT data behind its two zlib header bytes) to the S bytes it inflates to:
// the bit reader, the code-table builder, the per-symbol step and the block loop of mm_png_decode.hip, as plain C++.  MM_HD is
// __host__ __device__ under hipcc and empty otherwise, so the same text compiles into the kernel and into tools/png_inflate_check.cpp, the
// stand-alone host program the damaged-stream tests run under the host sanitizers.
//
// ONE WAVE decodes one stream.  Everything in an `Inflate` is the same in every lane: the chain of symbols is decoded uniformly.  The lanes
// work together (lane, lanes: threadIdx.x and 64 in the kernel, 0 and 1 on the host -- MM_INF_SERIAL) on what is not the chain: loading the
// input window, building the code tables, stored-block copies and match copies.
//
// THE INVARIANT, for ANY bytes and any record that passed check_png_decode:
//   reads    of the input only through inf_in(), which returns 0 for every position outside [begin, end);
//   writes   of the output only at out[o .. o + k) with k <= S - o, and o <= S always (inf_put, inf_copy_stored, inf_copy_match clamp to
//            S - o); a match reads out[o - dist ..) with 1 <= dist <= o, checked before the copy;
//   tables   every index into lens / look / syms / maxcode is a loop counter below the array's size, a masked peek (& 511), or a
//            checked sum (inf_symbol tests idx < MM_INF_MAX_SYMS);
//   loops    every iteration of the block loop, the symbol loop and the code-length loop either consumes at least one input bit or
//            produces at least one output byte.  Consumed bits are capped: the first symbol that needed a bit past `end` (the reader
//            supplied zeros) sets MM_PNG_ST_OVERRUN and ends the decode, so at most 8 * (end - begin) + 64 bits are ever consumed; produced
//            bytes are capped by S, where the decode ends whatever follows.  The copy loops advance by at least one byte a step.
// So no byte sequence makes the decode spin, or read or write outside its input range and its S bytes.
//
//   reader   least significant bit first (RFC 1951 3.1.1); 64-bit accumulator refilled four bytes at a time to more than 32 unread bits:
//            a literal/length code and its extra bits (15 + 5) or a distance code and its extra bits (15 + 13) never refill in between.
//   tables   per code (literal/length, distance, code-length): count[1..15]; the canonical maxcode[L] (-1: no code of length L) and
//            valoff[L] (index of the length's first symbol in syms, minus its first code); syms, the symbols sorted by (length, symbol);
//            and 512 look-ahead entries indexed by the next 9 stream bits: length << 12 | symbol for codes of up to 9 bits, 0 otherwise
//            (then the 15 peeked bits are reversed and lengths 10..15 tried in turn, as libjpeg's slow path does).
//   validity zlib's (inftrees.c): an over-subscribed set is refused; an incomplete one too, except a literal/length or distance set
//            whose only code has length 1, and a distance set with no code at all.
// The first status that is not 0 ends the stream; the bytes it had produced stay, the rest of S stays zero (the caller zeroed it).
#ifndef MM_INFLATE_H
#define MM_INFLATE_H

#if defined(__HIPCC__)
#define MM_HD __host__ __device__
#else
#define MM_HD
#endif

#if defined(__HIP_DEVICE_COMPILE__) && !defined(MM_INF_SERIAL)
#define MM_INF_LANE ((int)threadIdx.x)
#define MM_INF_LANES 64
#define MM_INF_SYNC() __syncthreads()          /* a workgroup is one wave: orders LDS and global memory between its lanes */
#else
#define MM_INF_LANE 0
#define MM_INF_LANES 1
#define MM_INF_SYNC() ((void)0)
#endif

#define MM_PNG_ST_OVERRUN 1
#define MM_PNG_ST_BAD_BLOCK 2
#define MM_PNG_ST_BAD_TABLE 4
#define MM_PNG_ST_BAD_CODE 8
#define MM_PNG_ST_BAD_DISTANCE 16
#define MM_PNG_ST_SHORT 32
#define MM_PNG_ST_BAD_FILTER 64

#define MM_INF_LOOK_BITS 9
#define MM_INF_LOOK (1 << MM_INF_LOOK_BITS)
#define MM_INF_MAX_SYMS 320                    /* 288 literal/length + 32 distance lengths of the fixed codes; a dynamic header has at most 286 + 30 */
#define MM_INF_WINDOW 1024                     /* bytes of input staged at a time (the kernel's LDS window) */

namespace mm {

struct InfTable {
    unsigned short look[MM_INF_LOOK];
    unsigned short syms[MM_INF_MAX_SYMS];
    short maxcode[16], valoff[16], off[16], count[16];
};

struct InfShared {                              // the kernel keeps one in LDS
    unsigned window[MM_INF_WINDOW / 4];
    unsigned char lens[MM_INF_MAX_SYMS];
    InfTable ll, dd, cl;
};

struct Inflate {
    const unsigned char* in;                    // the call's bytes; this stream is in[begin, end)
    int begin, end;
    unsigned char* out;                         // S bytes, zeroed
    int S, o;                                   // o: bytes produced
    unsigned long long acc;                     // the low n bits are unread
    int n, pos;                                 // pos: the next byte to fetch; it runs past `end` (zeros) when the stream is short
    int wbase;                                  // the window holds bytes [wbase, wbase + MM_INF_WINDOW)
    bool fixed_ready;                           // ll / dd hold the fixed codes
    InfShared* sh;
};

MM_HD inline unsigned inf_in(const Inflate& s, int at) { return at >= s.begin && at < s.end ? s.in[at] : 0u; }

// bytes pos .. pos + 3 as one little-endian word
MM_HD inline unsigned inf_word(Inflate& s) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(MM_INF_SERIAL)
    if (s.pos < s.wbase || s.pos + 4 > s.wbase + MM_INF_WINDOW) {       // (uniform: every lane takes it)
        MM_INF_SYNC();
        s.wbase = s.pos;
        for (int j = MM_INF_LANE; j < MM_INF_WINDOW / 4; j += MM_INF_LANES) {
            const int at = s.wbase + 4 * j;
            s.sh->window[j] = inf_in(s, at) | inf_in(s, at + 1) << 8 | inf_in(s, at + 2) << 16 | inf_in(s, at + 3) << 24;
        }
        MM_INF_SYNC();
    }
    return s.sh->window[(s.pos - s.wbase) >> 2];                        // (pos - wbase is a multiple of 4: both move by 4 after a load at pos)
#else
    return inf_in(s, s.pos) | inf_in(s, s.pos + 1) << 8 | inf_in(s, s.pos + 2) << 16 | inf_in(s, s.pos + 3) << 24;
#endif
}

MM_HD inline void inf_fill(Inflate& s) {                                // more than 32 unread bits
    if (s.n <= 32) {
        s.acc |= (unsigned long long)inf_word(s) << s.n;
        s.pos += 4;
        s.n += 32;
    }
}
MM_HD inline unsigned inf_bits(Inflate& s, int k) {                     // k <= 16 unread bits, after a fill
    const unsigned v = (unsigned)s.acc & ((1u << k) - 1u);
    s.acc >>= k;
    s.n -= k;
    return v;
}
// a bit past the stream's end has been consumed (peeked bits do not count)
MM_HD inline bool inf_overrun(const Inflate& s) { return 8LL * (s.pos - s.begin) - s.n > 8LL * (s.end - s.begin); }

MM_HD inline unsigned inf_rev15(unsigned x) {                           // the low 15 bits reversed
    x = ((x & 0x5555u) << 1) | ((x >> 1) & 0x5555u);
    x = ((x & 0x3333u) << 2) | ((x >> 2) & 0x3333u);
    x = ((x & 0x0F0Fu) << 4) | ((x >> 4) & 0x0F0Fu);
    x = ((x & 0x00FFu) << 8) | ((x >> 8) & 0x00FFu);
    return x >> 1;
}

// The table of n code lengths (each 0..15).  Returns max length | over-subscribed << 8 | incomplete << 9; an over-subscribed set builds nothing more.
MM_HD inline int inf_build(InfTable& t, const unsigned char* lens, int n) {
    const int lane = MM_INF_LANE;
    MM_INF_SYNC();                                                      // the lengths are written
    for (int L = lane; L < 16; L += MM_INF_LANES) {                     // lane L counts length L
        int c = 0;
        for (int i = 0; i < n; ++i) c += lens[i] == L;
        t.count[L] = (short)c;
    }
    MM_INF_SYNC();
    int code = 0, k = 0, left = 1, max = 0;
    for (int L = 1; L < 16; ++L) {                                      // every lane the same sums; lane 0 keeps them
        const int c = t.count[L];
        left = 2 * left - c;
        if (left < 0) return max | 1 << 8;
        if (c) max = L;
        if (lane == 0) {
            t.off[L] = (short)k;
            t.valoff[L] = (short)(k - code);
            t.maxcode[L] = (short)(c ? code + c - 1 : -1);
        }
        code = (code + c) << 1;
        k += c;
    }
    MM_INF_SYNC();
    for (int L = 1 + lane; L < 16; L += MM_INF_LANES) {                 // lane L - 1 places the symbols of length L, ascending
        int at = t.off[L];
        for (int i = 0; i < n; ++i) if (lens[i] == L) t.syms[at++] = (unsigned short)i;
    }
    MM_INF_SYNC();
    for (int e = lane; e < MM_INF_LOOK; e += MM_INF_LANES) {            // a look-ahead entry each: the canonical search over its own 9 bits
        const unsigned rev = inf_rev15((unsigned)e) >> (15 - MM_INF_LOOK_BITS);
        unsigned short v = 0;
        for (int L = 1; L <= MM_INF_LOOK_BITS; ++L) {
            const int c = (int)(rev >> (MM_INF_LOOK_BITS - L));
            if (c <= t.maxcode[L]) {
                const int idx = c + t.valoff[L];
                if ((unsigned)idx < MM_INF_MAX_SYMS) v = (unsigned short)(L << 12 | t.syms[idx]);
                break;
            }
        }
        t.look[e] = v;
    }
    MM_INF_SYNC();
    return max | (left > 0) << 9;
}

// the next symbol of table t, after a fill; -1: the bits match no code
MM_HD inline int inf_symbol(Inflate& s, const InfTable& t) {
    const unsigned peek = (unsigned)s.acc & 0x7FFFu;
    const unsigned e = t.look[peek & (MM_INF_LOOK - 1)];
    if (e) {
        inf_bits(s, (int)(e >> 12));
        return (int)(e & 0xFFFu);
    }
    const unsigned rev = inf_rev15(peek);
    for (int L = MM_INF_LOOK_BITS + 1; L <= 15; ++L) {
        const int c = (int)(rev >> (15 - L));
        if (c <= t.maxcode[L]) {
            const int idx = c + t.valoff[L];
            if ((unsigned)idx >= MM_INF_MAX_SYMS) return -1;
            inf_bits(s, L);
            return t.syms[idx];
        }
    }
    return -1;
}

MM_HD inline void inf_put(Inflate& s, unsigned v) {                     // one literal; the caller has o < S
    if (MM_INF_LANE == 0) s.out[s.o] = (unsigned char)v;
    ++s.o;
}

// len bytes (clamped to S - o) from dist back: min(dist, 64) bytes a step, every byte of a step older than the step -- so dist 1 is a
// broadcast of one byte and an overlapping match repeats its period
MM_HD inline void inf_copy_match(Inflate& s, int len, int dist) {
    int todo = len < s.S - s.o ? len : s.S - s.o;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(MM_INF_SERIAL)
    const int step = dist < MM_INF_LANES ? dist : MM_INF_LANES;
    while (todo > 0) {
        const int k = todo < step ? todo : step;
        MM_INF_SYNC();                                                  // the bytes written so far, by any lane
        if (MM_INF_LANE < k) s.out[s.o + MM_INF_LANE] = s.out[s.o - dist + MM_INF_LANE];
        s.o += k;
        todo -= k;
    }
#else
    for (; todo > 0; --todo, ++s.o) s.out[s.o] = s.out[s.o - dist];
#endif
}

// a stored block's bytes: from in[p ..), clamped to S - o and to the stream's end; true if the stream ended first
MM_HD inline bool inf_copy_stored(Inflate& s, int p, int len) {
    const int want = len < s.S - s.o ? len : s.S - s.o;
    const int have = p < s.end ? s.end - p : 0;
    const int k = want < have ? want : have;
    for (int i = MM_INF_LANE; i < k; i += MM_INF_LANES) s.out[s.o + i] = (unsigned char)inf_in(s, p + i);
    s.o += k;
    return want > have;
}

MM_HD inline void inf_fixed_lengths(unsigned char* lens) {
    for (int i = MM_INF_LANE; i < MM_INF_MAX_SYMS; i += MM_INF_LANES) lens[i] = (unsigned char)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
}

// a dynamic block's header (RFC 1951 3.2.7) into the ll and dd tables; a status
MM_HD inline int inf_dynamic_header(Inflate& s) {
    InfShared& sh = *s.sh;
    inf_fill(s);
    const int hlit = (int)inf_bits(s, 5) + 257, hdist = (int)inf_bits(s, 5) + 1, hclen = (int)inf_bits(s, 4) + 4;
    if (inf_overrun(s)) return MM_PNG_ST_OVERRUN;
    if (hlit > 286 || hdist > 30) return MM_PNG_ST_BAD_TABLE;
    MM_INF_SYNC();
    for (int i = MM_INF_LANE; i < 19; i += MM_INF_LANES) sh.lens[i] = 0;
    MM_INF_SYNC();
    for (int i = 0; i < hclen; ++i) {
        inf_fill(s);
        const unsigned v = inf_bits(s, 3);
        const int at = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 7 - (i - 5) / 2 : 8 + (i - 4) / 2;      // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
        if (MM_INF_LANE == 0) sh.lens[at] = (unsigned char)v;
    }
    if (inf_overrun(s)) return MM_PNG_ST_OVERRUN;
    int r = inf_build(sh.cl, sh.lens, 19);
    if (r >> 8) return MM_PNG_ST_BAD_TABLE;                             // over-subscribed or incomplete (all zero included)
    const int total = hlit + hdist;
    int have = 0, prev = 0;
    while (have < total) {                                              // (a symbol a trip: at least one bit)
        inf_fill(s);
        const int sym = inf_symbol(s, sh.cl);
        if (sym < 0) return MM_PNG_ST_BAD_TABLE;
        int rep = 1, v = sym;
        if (sym == 16) { v = prev; rep = 3 + (int)inf_bits(s, 2); }
        else if (sym == 17) { v = 0; rep = 3 + (int)inf_bits(s, 3); }
        else if (sym == 18) { v = 0; rep = 11 + (int)inf_bits(s, 7); }
        if (inf_overrun(s)) return MM_PNG_ST_OVERRUN;
        if ((sym == 16 && have == 0) || have + rep > total) return MM_PNG_ST_BAD_TABLE;
        for (int i = MM_INF_LANE; i < rep; i += MM_INF_LANES) sh.lens[have + i] = (unsigned char)v;      // a repeat runs on from the literal/length lengths into the distance lengths
        have += rep;
        prev = v;
    }
    MM_INF_SYNC();
    if (sh.lens[256] == 0) return MM_PNG_ST_BAD_TABLE;                  // no end-of-block code
    r = inf_build(sh.ll, sh.lens, hlit);
    if ((r & 1 << 8) || ((r & 1 << 9) && (r & 255) != 1)) return MM_PNG_ST_BAD_TABLE;
    r = inf_build(sh.dd, sh.lens + hlit, hdist);
    if ((r & 1 << 8) || ((r & 1 << 9) && (r & 255) > 1)) return MM_PNG_ST_BAD_TABLE;
    s.fixed_ready = false;
    return 0;
}

// the symbols of one block with the tables in place, up to its end-of-block code or S bytes; a status
MM_HD inline int inf_block(Inflate& s) {
    const InfShared& sh = *s.sh;
    for (;;) {                                                          // (a symbol a trip: at least one bit)
        inf_fill(s);
        const int sym = inf_symbol(s, sh.ll);
        if (sym < 0) return MM_PNG_ST_BAD_CODE;
        if (sym < 256) {
            if (inf_overrun(s)) return MM_PNG_ST_OVERRUN;
            inf_put(s, (unsigned)sym);
            if (s.o == s.S) return 0;
            continue;
        }
        if (sym == 256) return inf_overrun(s) ? MM_PNG_ST_OVERRUN : 0;
        if (sym > 285) return MM_PNG_ST_BAD_CODE;
        const int i = sym - 257, le = i < 8 || i == 28 ? 0 : (i >> 2) - 1;
        const int len = (i == 28 ? 258 : i < 8 ? 3 + i : 3 + ((4 + (i & 3)) << le)) + (int)inf_bits(s, le);
        inf_fill(s);
        const int d = inf_symbol(s, sh.dd);
        if (d < 0 || d > 29) return MM_PNG_ST_BAD_CODE;
        const int de = d < 4 ? 0 : (d >> 1) - 1;
        const int dist = (d < 4 ? 1 + d : 1 + ((2 + (d & 1)) << de)) + (int)inf_bits(s, de);
        if (inf_overrun(s)) return MM_PNG_ST_OVERRUN;
        if (dist > s.o) return MM_PNG_ST_BAD_DISTANCE;
        inf_copy_match(s, len, dist);
        if (s.o == s.S) return 0;
    }
}

// The whole stream: in[begin, end) into out[0, S).  The status (0: S bytes exist).
MM_HD inline int inflate_stream(const unsigned char* in, int begin, int end, unsigned char* out, int S, InfShared* sh) {
    Inflate s;
    s.in = in; s.begin = begin; s.end = end; s.out = out; s.S = S; s.o = 0;
    s.acc = 0; s.n = 0; s.pos = begin; s.wbase = begin - 2 * MM_INF_WINDOW; s.fixed_ready = false; s.sh = sh;
    if (S <= 0) return 0;
    for (;;) {                                                          // (a block a trip: at least three bits)
        inf_fill(s);
        const unsigned last = inf_bits(s, 1), type = inf_bits(s, 2);
        if (inf_overrun(s)) return MM_PNG_ST_OVERRUN;
        if (type == 3) return MM_PNG_ST_BAD_BLOCK;
        if (type == 0) {
            inf_bits(s, s.n & 7);                                       // to the byte boundary
            inf_fill(s);
            const unsigned len = inf_bits(s, 16), nlen = inf_bits(s, 16);
            if (inf_overrun(s)) return MM_PNG_ST_OVERRUN;
            if ((len ^ nlen) != 0xFFFFu) return MM_PNG_ST_BAD_BLOCK;
            const int p = s.pos - (s.n >> 3);                           // the first byte not consumed (n is a multiple of 8)
            if (inf_copy_stored(s, p, (int)len)) return MM_PNG_ST_OVERRUN;
            s.pos = p + (int)len; s.n = 0; s.acc = 0; s.wbase = s.pos - 2 * MM_INF_WINDOW;      // the reader starts again behind the block
        } else {
            if (type == 1) {
                if (!s.fixed_ready) {
                    MM_INF_SYNC();
                    inf_fixed_lengths(sh->lens);
                    inf_build(sh->ll, sh->lens, 288);
                    inf_build(sh->dd, sh->lens + 288, 32);
                    s.fixed_ready = true;
                }
            } else {
                const int st = inf_dynamic_header(s);
                if (st) return st;
            }
            const int st = inf_block(s);
            if (st) return st;
        }
        if (s.o == s.S) return 0;
        if (last) return MM_PNG_ST_SHORT;
    }
}

}  // namespace mm
#endif
