// BGZF (SAM/BAM specification section 4.1) on the device: deflate + CRC32 of 65 280-byte blocks, one workgroup per block.
// gfx950 (MI355X).
//
// Per block (k_bgzf_deflate, 256 threads, the block's bytes staged in LDS):
//   match finding  the block is walked in 255 tiles of 256 positions (one per thread).  A 2^13-entry hash table of 4-byte
//                  prefixes holds, per bucket, the LAST position of the tiles already walked (atomicMax: order-free, so the
//                  table after a tile is a pure function of the bytes).  Each position compares against that candidate and
//                  against distance 1 (runs); the longer match is kept in the launch's workspace (4 B per position).
//   parse          thread t owns bytes [255 t, 255 t + 255) and parses them greedily; a match never crosses the end of the
//                  thread's span.  A match is taken only if its estimated cost (length / distance symbols + extra bits)
//                  is below that of the literals it replaces, literal costs from the block's byte histogram -- random
//                  ACGT text stays literal-coded (about 2 bits per base), N-runs become one match per 255 bytes.
//   Huffman        lit/len and distance histograms (LDS atomics), symbols ranked in parallel, code lengths by the in-place
//                  minimum-redundancy algorithm (Moffat-Katajainen) limited to 15 bits (7 for the code-length code) by
//                  the usual Kraft repair; canonical codes (RFC 1951 3.2.2).
//   packing        every thread sums its tokens' bits, an exclusive scan gives its bit offset, tokens are OR-ed into an
//                  LDS image of the block (atomicOr: order-free).  If the dynamic block is not smaller, a stored block.
//   CRC32          raw CRC per thread span, shifted to its place by multiplication with x^(8 k) mod P and XOR-combined.
// k_bgzf_scan + k_bgzf_pack then lay the members out back to back (header, deflate data, CRC32, ISIZE) in one buffer.
// Everything is a function of the uncompressed bytes only: no timing, no "last writer wins".
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "bgzf.h"

namespace msim {

namespace {

constexpr int BZ_THREADS = 256;
constexpr int BZ_SPAN = 255;                 // bytes per thread: BZ_THREADS * BZ_SPAN == BGZF_BLOCK
constexpr int BZ_HBITS = 13;
constexpr int BZ_HSIZE = 1 << BZ_HBITS;
constexpr int BZ_WINDOW = 32768;
constexpr int BZ_OUT_WORDS = BGZF_SLOT / 4;
static_assert(BZ_THREADS * BZ_SPAN == BGZF_BLOCK, "block = threads x span");

struct BzSmem {
    uint8_t in[BGZF_BLOCK + 16];
    union {
        uint32_t table[BZ_HSIZE];
        uint32_t out[BZ_OUT_WORDS];
    } u;
    uint32_t take[BGZF_BLOCK / 32];      // bit p: a match worth taking starts at p (its length / distance: workspace)
    uint32_t crc_table[256];
    uint32_t x2n[32];
    uint32_t byte_hist[256];
    uint16_t litcost[256];               // 1/16 bits
    uint32_t lfreq[288], dfreq[32];
    uint16_t lsrt[288], dsrt[32];        // symbols with freq > 0, ascending (freq, symbol)
    uint32_t lwork[288], dwork[32];
    uint8_t llen[288], dlen[32];
    uint16_t lcode[288], dcode[32];      // bit-reversed canonical codes
    uint32_t nlsym, ndsym;
    uint32_t ntok[BZ_THREADS];
    uint32_t bits[BZ_THREADS];
    uint8_t rle_sym[320], rle_ext[320];
    uint32_t n_rle;
    uint32_t clfreq[19];
    uint16_t clsrt[19];
    uint32_t clwork[19];
    uint8_t cllen[19];
    uint16_t clcode[19];
    uint32_t hlit, hdist, hclen, header_bits;
    uint32_t crc_acc;
    uint32_t stored;
};

__constant__ uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ inline uint32_t multmodp(uint32_t a, uint32_t b) {
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ 0xedb88320u : b >> 1;
    }
    return p;
}

// x^(8 n) mod P (reflected)
__device__ inline uint32_t x8nmodp(const uint32_t *x2n, uint64_t n) {
    uint32_t p = 1u << 31;
    int k = 3;
    while (n) {
        if (n & 1) p = multmodp(x2n[k & 31], p);
        n >>= 1;
        k++;
    }
    return p;
}

__device__ inline uint32_t rev_bits(uint32_t code, int len) { return __brev(code) >> (32 - len); }

// length 3..258 -> symbol 257..285, extra bits, extra value
__device__ inline void len_sym(uint32_t L, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
    if (L <= 10) { sym = 254 + L; eb = 0; ev = 0; return; }
    if (L == 258) { sym = 285; eb = 0; ev = 0; return; }
    const uint32_t x = L - 3, nb = 31 - __clz(x), e = nb - 2;
    sym = 265 + 4 * (nb - 3) + ((x >> e) & 3);
    eb = e;
    ev = x & ((1u << e) - 1);
}

// distance 1..32768 -> symbol 0..29, extra bits, extra value
__device__ inline void dist_sym(uint32_t d, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
    if (d <= 4) { sym = d - 1; eb = 0; ev = 0; return; }
    const uint32_t x = d - 1, nb = 31 - __clz(x), e = nb - 1;
    sym = 2 * nb + ((x >> e) & 1);
    eb = e;
    ev = x & ((1u << e) - 1);
}

__device__ inline uint32_t hash4(const uint8_t *p) {
    const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    return (v * 2654435761u) >> (32 - BZ_HBITS);
}

// Code lengths of the m symbols srt[0..m) (ascending frequency) into len[], at most maxlen bits.  m >= 2.  One thread.
__device__ void huff_lengths(const uint32_t *freq, const uint16_t *srt, int m, uint32_t *A, uint8_t *len, int maxlen) {
    for (int i = 0; i < m; i++) A[i] = freq[srt[i]];
    // in-place minimum-redundancy code lengths (Moffat and Katajainen, 1995)
    A[0] += A[1];
    int root = 0, leaf = 2, next;
    for (next = 1; next < m - 1; next++) {
        if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; }
        else A[next] = A[leaf++];
        if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; }
        else A[next] += A[leaf++];
    }
    A[m - 2] = 0;
    for (next = m - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
    int avbl = 1, used = 0, dpth = 0;
    root = m - 2;
    next = m - 1;
    while (avbl > 0) {
        while (root >= 0 && (int)A[root] == dpth) { used++; root--; }
        while (avbl > used) { A[next--] = dpth; avbl--; }
        avbl = 2 * used;
        dpth++;
        used = 0;
    }
    // A[i] = length of srt[i] (non-increasing in i); limit to maxlen with the Kraft repair
    uint32_t num[33];
    for (int i = 0; i <= 32; i++) num[i] = 0;
    for (int i = 0; i < m; i++) num[A[i] > 32 ? 32 : A[i]]++;
    for (int i = maxlen + 1; i <= 32; i++) { num[maxlen] += num[i]; num[i] = 0; }
    uint32_t total = 0;
    for (int i = maxlen; i > 0; i--) total += num[i] << (maxlen - i);
    while (total != (1u << maxlen)) {
        num[maxlen]--;
        for (int i = maxlen - 1; i > 0; i--)
            if (num[i]) { num[i]--; num[i + 1] += 2; break; }
        total--;
    }
    int j = m;
    for (int l = 1; l <= maxlen; l++)
        for (uint32_t k = num[l]; k > 0; k--) len[srt[--j]] = (uint8_t)l;
}

// canonical codes (bit-reversed for the LSB-first stream).  One thread.
__device__ void huff_codes(const uint8_t *len, int n, uint16_t *code) {
    uint32_t cnt[16], nxt[16];
    for (int i = 0; i < 16; i++) cnt[i] = 0;
    for (int s = 0; s < n; s++) cnt[len[s]]++;
    cnt[0] = 0;
    uint32_t c = 0;
    for (int b = 1; b < 16; b++) { c = (c + cnt[b - 1]) << 1; nxt[b] = c; }
    for (int s = 0; s < n; s++)
        if (len[s]) code[s] = (uint16_t)rev_bits(nxt[len[s]]++, len[s]);
}

// rank the symbols [0, n) with freq > 0 by (freq, symbol) into srt (parallel over the workgroup)
__device__ void rank_symbols(const uint32_t *freq, int n, uint16_t *srt, uint32_t *count) {
    for (int s = threadIdx.x; s < n; s += BZ_THREADS) {
        const uint32_t f = freq[s];
        if (!f) continue;
        uint32_t r = 0;
        for (int q = 0; q < n; q++) {
            const uint32_t g = freq[q];
            r += (g && (g < f || (g == f && q < s))) ? 1u : 0u;
        }
        srt[r] = (uint16_t)s;
        atomicAdd(count, 1u);
    }
}

// Bit sink into the LDS image: a 64-bit accumulator, full words OR-ed in.
struct BitOut {
    uint32_t *w;
    uint32_t word;
    uint64_t acc;
    uint32_t nacc;
    __device__ BitOut(uint32_t *words, uint32_t bitpos) : w(words), word(bitpos >> 5), acc(0), nacc(bitpos & 31) {}
    __device__ inline void put(uint32_t v, uint32_t nb) {
        acc |= (uint64_t)v << nacc;
        nacc += nb;
        if (nacc >= 32) {
            atomicOr(&w[word++], (uint32_t)acc);
            acc >>= 32;
            nacc -= 32;
        }
    }
    __device__ inline void flush() {
        if (nacc) atomicOr(&w[word], (uint32_t)acc);
    }
};

// Cost estimate of a match in 1/16 bits: about 7 bits for the length symbol and 5 for the distance symbol, plus extra bits.
__device__ inline uint32_t match_cost(uint32_t L, uint32_t d) {
    uint32_t s, eb, ev, s2, eb2, ev2;
    len_sym(L, s, eb, ev);
    dist_sym(d, s2, eb2, ev2);
    return 16u * (12u + eb + eb2);
}

__global__ void __launch_bounds__(BZ_THREADS) k_bgzf_deflate(const uint8_t *__restrict__ src, uint64_t n_total,
                                                             uint32_t *__restrict__ ws, uint8_t *__restrict__ slots,
                                                             uint32_t *__restrict__ meta) {
    __shared__ BzSmem S;
    const int tid = threadIdx.x;
    const uint64_t blk = blockIdx.x;
    const uint64_t base = blk * (uint64_t)BGZF_BLOCK;
    const uint32_t n = (uint32_t)((n_total - base) < (uint64_t)BGZF_BLOCK ? (n_total - base) : (uint64_t)BGZF_BLOCK);
    uint32_t *W = ws + blk * (uint64_t)BGZF_BLOCK;
    uint8_t *slot = slots + blk * (uint64_t)BGZF_SLOT;
    const uint8_t *in_g = src + base;

    // ---- stage the block; clear tables
    for (uint32_t i = tid; i < BGZF_BLOCK + 16; i += BZ_THREADS) S.in[i] = i < n ? in_g[i] : 0;
    for (int i = tid; i < BZ_HSIZE; i += BZ_THREADS) S.u.table[i] = 0;
    for (int i = tid; i < 288; i += BZ_THREADS) { S.lfreq[i] = 0; S.llen[i] = 0; }
    if (tid < 32) { S.dfreq[tid] = 0; S.dlen[tid] = 0; }
    if (tid < 19) { S.clfreq[tid] = 0; S.cllen[tid] = 0; }
    {
        uint32_t c = (uint32_t)tid;
        for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ 0xedb88320u : c >> 1;
        S.crc_table[tid] = c;
        S.byte_hist[tid] = 0;
    }
    if (tid == 0) {
        uint32_t p = 1u << 30;                       // x^1
        for (int k = 0; k < 32; k++) { S.x2n[k] = p; p = multmodp(p, p); }
        S.nlsym = 0; S.ndsym = 0; S.crc_acc = 0; S.n_rle = 0;
    }
    __syncthreads();

    // ---- CRC32 of the thread's span, byte histogram
    const uint32_t s0 = (uint32_t)tid * BZ_SPAN, s1 = s0 + BZ_SPAN < n ? s0 + BZ_SPAN : n;
    {
        uint32_t c = 0;
        for (uint32_t i = s0; i < s1; i++) {
            const uint8_t b = S.in[i];
            c = S.crc_table[(c ^ b) & 0xff] ^ (c >> 8);
            atomicAdd(&S.byte_hist[b], 1u);
        }
        uint32_t x = s0 < s1 ? multmodp(x8nmodp(S.x2n, n - s1), c) : 0;
        if (tid == 0) x ^= multmodp(x8nmodp(S.x2n, n), 0xffffffffu);
        atomicXor(&S.crc_acc, x);
    }

    __syncthreads();
    // ---- literal costs from the byte histogram (1/16 bits, at least 1 bit)
    {
        const uint32_t cnt = S.byte_hist[tid];
        uint32_t c = 16 * 12;
        if (cnt) {
            const float bitsf = __log2f((float)n / (float)cnt) * 16.0f;
            c = bitsf < 16.0f ? 16u : (uint32_t)bitsf;
        }
        S.litcost[tid] = (uint16_t)c;
    }
    __syncthreads();

    // ---- match finding, one tile of 256 positions per round.  A match is kept (workspace + bit in S.take) only if it
    // costs less than the literals it replaces; the parse below then reads the workspace only where a match starts.
    for (uint32_t t0 = 0; t0 < n; t0 += BZ_THREADS) {
        const uint32_t p = t0 + tid;
        uint32_t h = 0;
        bool worth = false;
        if (p < n) {
            uint32_t best = 0, bd = 0;
            const uint32_t span_end = (p / BZ_SPAN + 1) * BZ_SPAN;
            uint32_t maxl = span_end - p;
            if (maxl > n - p) maxl = n - p;
            if (maxl > 258) maxl = 258;
            if (maxl >= 3) {
                if (p + 4 <= n) {
                    h = hash4(&S.in[p]);
                    const uint32_t e = S.u.table[h];
                    if (e && p - (e - 1) <= BZ_WINDOW) {
                        const uint32_t c = e - 1;
                        uint32_t L = 0;
                        while (L < maxl && S.in[c + L] == S.in[p + L]) L++;
                        best = L; bd = p - c;
                    }
                }
                if (p >= 1 && S.in[p - 1] == S.in[p]) {
                    uint32_t L = 0;
                    while (L < maxl && S.in[p - 1 + L] == S.in[p + L]) L++;
                    if (L >= best) { best = L; bd = 1; }
                }
            }
            if (best >= 3) {
                const uint32_t cost = match_cost(best, bd);
                uint32_t sum = 0;
                for (uint32_t i = 0; i < best && !worth; i++) {
                    sum += S.litcost[S.in[p + i]];
                    worth = sum > cost;
                }
                if (worth) W[p] = (best << 16) | bd;
            }
        }
        const unsigned long long mask = __ballot(worth);
        if ((tid & 63) == 0) {
            const uint32_t w = (t0 + (tid & ~63u)) >> 5;
            S.take[w] = (uint32_t)mask;
            S.take[w + 1] = (uint32_t)(mask >> 32);
        }
        __syncthreads();
        if (p < n && p + 4 <= n) atomicMax(&S.u.table[h], p + 1);
        __syncthreads();
    }


    // ---- greedy parse of the thread's span: tokens in place in the workspace
    {
        uint32_t k = 0, p = s0;
        while (p < s1) {
            if ((S.take[p >> 5] >> (p & 31)) & 1) {
                const uint32_t m = W[p];
                const uint32_t L = m >> 16;
                uint32_t s, eb, ev;
                len_sym(L, s, eb, ev);
                atomicAdd(&S.lfreq[s], 1u);
                dist_sym(m & 0xffff, s, eb, ev);
                atomicAdd(&S.dfreq[s], 1u);
                W[s0 + k++] = m;
                p += L;
            } else {
                const uint32_t b = S.in[p];
                atomicAdd(&S.lfreq[b], 1u);
                W[s0 + k++] = b;
                p++;
            }
        }
        S.ntok[tid] = k;
    }
    __syncthreads();
    if (tid == 0) {
        S.lfreq[256] = 1;                             // end of block
        uint32_t used = 0;
        for (int s = 0; s < 30; s++) used += S.dfreq[s] ? 1u : 0u;
        if (used < 2) {                               // two distance codes at least: a complete code for every inflater
            if (!S.dfreq[0]) S.dfreq[0] = 1;
            if (!S.dfreq[1]) S.dfreq[1] = 1;
        }
    }
    __syncthreads();
    rank_symbols(S.lfreq, 286, S.lsrt, &S.nlsym);
    rank_symbols(S.dfreq, 30, S.dsrt, &S.ndsym);
    __syncthreads();
    if (tid == 0) {
        huff_lengths(S.lfreq, S.lsrt, (int)S.nlsym, S.lwork, S.llen, 15);
        huff_codes(S.llen, 286, S.lcode);
    } else if (tid == 64) {
        huff_lengths(S.dfreq, S.dsrt, (int)S.ndsym, S.dwork, S.dlen, 15);
        huff_codes(S.dlen, 30, S.dcode);
    }
    __syncthreads();

    // ---- thread 0: the code-length code and the header's size; everyone: the bits of its tokens
    if (tid == 0) {
        uint32_t hlit = 286, hdist = 30;
        while (hlit > 257 && !S.llen[hlit - 1]) hlit--;
        while (hdist > 1 && !S.dlen[hdist - 1]) hdist--;
        const uint32_t tot = hlit + hdist;
        uint32_t nr = 0;
        auto L = [&](uint32_t i) -> uint32_t { return i < hlit ? S.llen[i] : S.dlen[i - hlit]; };
        auto emit = [&](uint32_t sym, uint32_t ext) { S.rle_sym[nr] = (uint8_t)sym; S.rle_ext[nr] = (uint8_t)ext; nr++; S.clfreq[sym]++; };
        uint32_t i = 0;
        while (i < tot) {
            const uint32_t v = L(i);
            uint32_t run = 1;
            while (i + run < tot && L(i + run) == v) run++;
            i += run;
            if (v == 0) {
                while (run >= 11) { const uint32_t r = run < 138 ? run : 138; emit(18, r - 11); run -= r; }
                if (run >= 3) { emit(17, run - 3); run = 0; }
                while (run) { emit(0, 0); run--; }
            } else {
                emit(v, 0);
                run--;
                while (run >= 3) { const uint32_t r = run < 6 ? run : 6; emit(16, r - 3); run -= r; }
                while (run) { emit(v, 0); run--; }
            }
        }
        S.n_rle = nr;
        uint32_t used = 0;
        for (int s = 0; s < 19; s++) used += S.clfreq[s] ? 1u : 0u;
        if (used < 2) {
            if (!S.clfreq[0]) S.clfreq[0] = 1;
            else S.clfreq[1] = 1;
        }
        // rank (19 symbols: a serial insertion sort)
        int m = 0;
        for (int s = 0; s < 19; s++) {
            if (!S.clfreq[s]) continue;
            int j = m++;
            while (j > 0 && S.clfreq[S.clsrt[j - 1]] > S.clfreq[s]) { S.clsrt[j] = S.clsrt[j - 1]; j--; }
            S.clsrt[j] = (uint16_t)s;
        }
        huff_lengths(S.clfreq, S.clsrt, m, S.clwork, S.cllen, 7);
        huff_codes(S.cllen, 19, S.clcode);
        uint32_t hclen = 19;
        while (hclen > 4 && !S.cllen[kClOrder[hclen - 1]]) hclen--;
        uint32_t bits = 3 + 5 + 5 + 4 + 3 * hclen;
        for (uint32_t r = 0; r < nr; r++) {
            const uint32_t s = S.rle_sym[r];
            bits += S.cllen[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
        }
        S.hlit = hlit; S.hdist = hdist; S.hclen = hclen; S.header_bits = bits;
    }
    uint32_t mybits = 0;
    {
        uint32_t b = 0;
        const uint32_t nt = S.ntok[tid];
        for (uint32_t k = 0; k < nt; k++) {
            const uint32_t m = W[s0 + k];
            if (m < 256) {
                b += S.llen[m];
            } else {
                uint32_t s, eb, ev;
                len_sym(m >> 16, s, eb, ev);
                b += S.llen[s] + eb;
                dist_sym(m & 0xffff, s, eb, ev);
                b += S.dlen[s] + eb;
            }
        }
        S.bits[tid] = b;
        mybits = b;
    }
    __syncthreads();
    // exclusive scan of the threads' bit counts (Hillis-Steele over 256)
    for (int off = 1; off < BZ_THREADS; off <<= 1) {
        const uint32_t v = tid >= off ? S.bits[tid - off] : 0u;
        __syncthreads();
        S.bits[tid] += v;
        __syncthreads();
    }
    const uint32_t incl = S.bits[tid];
    const uint32_t total_bits = S.header_bits + S.bits[BZ_THREADS - 1] + S.llen[256];
    const uint32_t dyn_bytes = (total_bits + 7) / 8;
    const bool stored = dyn_bytes >= n + 5;
    __syncthreads();

    uint32_t csize;
    if (stored) {
        csize = n + 5;
        if (tid == 0) {
            slot[0] = 1;                               // BFINAL, BTYPE 00
            slot[1] = (uint8_t)(n & 0xff); slot[2] = (uint8_t)(n >> 8);
            slot[3] = (uint8_t)(~n & 0xff); slot[4] = (uint8_t)((~n >> 8) & 0xff);
        }
        for (uint32_t i = tid; i < n; i += BZ_THREADS) slot[5 + i] = S.in[i];
    } else {
        csize = dyn_bytes;
        for (int i = tid; i < BZ_OUT_WORDS; i += BZ_THREADS) S.u.out[i] = 0;
        __syncthreads();
        if (tid == 0) {
            BitOut o(S.u.out, 0);
            o.put(1, 1);                               // BFINAL
            o.put(2, 2);                               // BTYPE 10
            o.put(S.hlit - 257, 5);
            o.put(S.hdist - 1, 5);
            o.put(S.hclen - 4, 4);
            for (uint32_t i = 0; i < S.hclen; i++) o.put(S.cllen[kClOrder[i]], 3);
            for (uint32_t r = 0; r < S.n_rle; r++) {
                const uint32_t s = S.rle_sym[r];
                o.put(S.clcode[s], S.cllen[s]);
                if (s == 16) o.put(S.rle_ext[r], 2);
                else if (s == 17) o.put(S.rle_ext[r], 3);
                else if (s == 18) o.put(S.rle_ext[r], 7);
            }
            o.flush();
        }
        {
            const uint32_t nt = S.ntok[tid];
            BitOut o(S.u.out, S.header_bits + incl - mybits);
            for (uint32_t k = 0; k < nt; k++) {
                const uint32_t m = W[s0 + k];
                if (m < 256) {
                    o.put(S.lcode[m], S.llen[m]);
                } else {
                    uint32_t s, eb, ev;
                    len_sym(m >> 16, s, eb, ev);
                    o.put(S.lcode[s], S.llen[s]);
                    if (eb) o.put(ev, eb);
                    dist_sym(m & 0xffff, s, eb, ev);
                    o.put(S.dcode[s], S.dlen[s]);
                    if (eb) o.put(ev, eb);
                }
            }
            if (tid == BZ_THREADS - 1) o.put(S.lcode[256], S.llen[256]);
            o.flush();
        }
        __syncthreads();
        uint32_t *slot32 = reinterpret_cast<uint32_t *>(slot);
        for (uint32_t i = tid; i < (csize + 3) / 4; i += BZ_THREADS) slot32[i] = S.u.out[i];
    }
    if (tid == 0) {
        meta[3 * blk + 0] = csize;
        meta[3 * blk + 1] = S.crc_acc ^ 0xffffffffu;
        meta[3 * blk + 2] = n;
    }
}

// offsets of the members (member = 18 + deflate + 8 bytes) and their total at off[nblk].  One workgroup of 1024.
__global__ void __launch_bounds__(1024) k_bgzf_scan(const uint32_t *__restrict__ meta, uint32_t nblk, uint64_t *__restrict__ off) {
    __shared__ uint64_t part[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (nblk + 1023) / 1024;
    const uint32_t a = tid * per, b = a + per < nblk ? a + per : nblk;
    uint64_t s = 0;
    for (uint32_t i = a; i < b; i++) s += meta[3 * i] + 26u;
    part[tid] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint64_t v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint64_t o = part[tid] - s;
    for (uint32_t i = a; i < b; i++) { off[i] = o; o += meta[3 * i] + 26u; }
    if (tid == 1023) off[nblk] = part[1023];
}

__global__ void __launch_bounds__(256) k_bgzf_pack(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ meta,
                                                    const uint64_t *__restrict__ off, uint8_t *__restrict__ dst) {
    const uint64_t blk = blockIdx.x;
    const uint32_t csize = meta[3 * blk], crc = meta[3 * blk + 1], isize = meta[3 * blk + 2];
    uint8_t *o = dst + off[blk];
    const uint8_t *s = slots + blk * (uint64_t)BGZF_SLOT;
    const uint32_t bsize = csize + 26 - 1;
    if (threadIdx.x < 18) {
        const uint8_t hdr[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0,
                                 (uint8_t)(bsize & 0xff), (uint8_t)(bsize >> 8)};
        o[threadIdx.x] = hdr[threadIdx.x];
    } else if (threadIdx.x < 26) {
        const uint32_t k = threadIdx.x - 18;
        const uint32_t v = k < 4 ? crc : isize;
        o[18 + csize + k] = (uint8_t)(v >> (8 * (k & 3)));
    }
    for (uint32_t i = threadIdx.x; i < csize; i += 256) o[18 + i] = s[i];
}


// ---------------------------------------------------------------------------------------------------------------- inflate
// k_bgzf_inflate: RFC 1951 decoder, one member per workgroup of ONE wavefront; the member's output is built in LDS (back-
// references never leave the CU) and written out coalesced once its length and CRC32 have been checked.
//   symbol loop    every lane runs the same bit reader and the same table look-ups (the wave executes them once): the state
//                  is wave-uniform, so no lane has to tell the others what it decoded.  A literal is stored by lane 0; a
//                  match is copied by the wave, lane i taking bytes i, i + 64, ... from out[pos - dist + i mod dist] --
//                  sources lie before `pos` whatever the overlap, so a distance-1 run of 258 is five LDS stores.
//   bit reader     a 64-bit buffer topped up 32 bits at a time from the member's deflate data in global memory; the word
//                  after the one being consumed is always in flight (its latency hides behind ~16 symbols of ACGT text).
//                  Reads past the member's data yield zeros and are found out by the bit count at the end of each block.
//   tables         canonical code lengths -> count / sorted-symbol arrays (lane 0, as zlib's checks want them: over-
//                  subscribed and incomplete sets are refused); a 10-bit (lit/len) and an 8-bit (distance) direct table
//                  are filled by the wave, each lane decoding its indices through the canonical arrays; longer codes take
//                  the canonical walk (at most 15 steps).
//   CRC32          as the encoder: raw CRC per lane span, shifted by x^(8 k) mod P, XOR-combined.
// Bounds: input reads by in_len, output writes by ISIZE <= 65 536, distances by the bytes produced, every loop by a
// constant (symbols by ISIZE + blocks, blocks by the member's bits, IZ_MAX_STEPS over all).  A member that fails a check
// leaves (index << 4 | reason) in the error word (atomicMin: the first one wins) and writes nothing.
constexpr int IZ_THREADS = 64;
constexpr int IZ_LBITS = 10, IZ_DBITS = 8;
constexpr uint32_t IZ_MAX_STEPS = 1u << 20;    // symbols + blocks of one member: 65 536 bytes and 8 * 65 536 / 3 blocks at most

struct IzSmem {
    uint32_t out[BGZF_MAX_ISIZE / 4 + 1];      // (+1: the write-out reads one word past the last byte)
    uint32_t crc_table[256];
    uint32_t x2n[32];
    uint16_t ltab[1 << IZ_LBITS], dtab[1 << IZ_DBITS];   // symbol << 4 | code length; 0: longer than the table / no code
    uint16_t lsym[288], dsym[32], csym[20];    // symbols ordered by (code length, symbol)
    uint16_t lcnt[16], dcnt[16], ccnt[16];     // codes per length
    uint16_t offs[16];
    uint8_t lens[320];                         // lit/len code lengths, then the distance code lengths
    uint8_t cl_lens[20];
    uint32_t flag;
    uint32_t crc_acc;
};

__device__ inline void wave_fence() { __builtin_amdgcn_wave_barrier(); }

// Wave-uniform LSB-first bit reader over in[0, n).
struct IzBits {
    const uint8_t *in;
    uint32_t n;
    uint64_t buf;
    uint32_t cnt;                              // valid bits in buf
    uint32_t pos;                              // bytes taken into buf (may pass n: zeros)
    uint32_t nxt;                              // the word at pos, already loaded
    __device__ inline uint32_t word(uint32_t p) const {
        if (p + 4 <= n) {
            uint32_t w;
            __builtin_memcpy(&w, in + p, 4);
            return w;
        }
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4; k++)
            if (p + k < n) w |= (uint32_t)in[p + k] << (8 * k);
        return w;
    }
    __device__ inline void start(uint32_t at) { pos = at; buf = 0; cnt = 0; nxt = word(at); }
    __device__ inline void refill() {          // at least 32 bits afterwards
        if (cnt <= 32) {
            buf |= (uint64_t)nxt << cnt;
            cnt += 32;
            pos += 4;
            nxt = word(pos);
        }
    }
    __device__ inline uint32_t peek() const { return (uint32_t)buf; }
    __device__ inline void drop(uint32_t k) { buf >>= k; cnt -= k; }
    __device__ inline uint32_t take(uint32_t k) {
        const uint32_t v = (uint32_t)buf & ((1u << k) - 1u);
        drop(k);
        return v;
    }
    __device__ inline uint32_t used_bits() const { return pos * 8u - cnt; }
    __device__ inline bool overrun() const { return used_bits() > n * 8u; }
};

// the symbol whose canonical code starts the LSB-first bits v; len = its length, 0 if no code of <= maxbits bits matches
__device__ inline uint32_t canon_decode(uint32_t v, const uint16_t *cnt, const uint16_t *sym, int maxbits, uint32_t &len) {
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= maxbits; l++) {
        code |= (int)(v & 1u);
        v >>= 1;
        const int count = cnt[l];
        if (code - count < first) { len = (uint32_t)l; return sym[index + (code - first)]; }
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    len = 0;
    return 0;
}

// Code lengths lens[0, n) -> cnt / sym (lane 0) and, if tab, the direct table (the wave).  zlib's rules: an over-subscribed
// set is refused, an incomplete one too unless it is a single 1-bit code of a lit/len or distance set (strict: never).
// Returns false (wave-uniform) for a refused set.
__device__ bool iz_build(IzSmem &S, const uint8_t *lens, int n, uint16_t *cnt, uint16_t *sym, uint16_t *tab, int tbits,
                         bool strict) {
    const int lane = threadIdx.x;
    __syncthreads();                           // the lengths are written
    if (lane == 0) {
        for (int l = 0; l < 16; l++) cnt[l] = 0;
        for (int s = 0; s < n; s++) cnt[lens[s]]++;
        int left = 1, maxl = 0;
        bool ok = true;
        for (int l = 1; l < 16; l++) {
            left = (left << 1) - (int)cnt[l];
            if (left < 0) { ok = false; break; }
            if (cnt[l]) maxl = l;
        }
        if (ok && left > 0 && maxl != 0 && (strict || maxl != 1)) ok = false;
        if (ok) {
            uint32_t o = 0;
            for (int l = 1; l < 16; l++) { S.offs[l] = (uint16_t)o; o += cnt[l]; }
            for (int s = 0; s < n; s++)
                if (lens[s]) sym[S.offs[lens[s]]++] = (uint16_t)s;
        }
        cnt[0] = 0;
        S.flag = ok ? 1u : 0u;
    }
    __syncthreads();
    if (!S.flag) return false;
    if (tab) {
        for (uint32_t i = lane; i < (1u << tbits); i += IZ_THREADS) {
            uint32_t len;
            const uint32_t s = canon_decode(i, cnt, sym, tbits, len);
            tab[i] = len ? (uint16_t)((s << 4) | len) : (uint16_t)0;
        }
        __syncthreads();
    }
    return true;
}

__global__ void __launch_bounds__(IZ_THREADS) k_bgzf_inflate(const uint8_t *__restrict__ src, uint32_t src_len,
                                                             const BgzfMember *__restrict__ meta, uint8_t *__restrict__ dst,
                                                             uint32_t *__restrict__ err) {
    __shared__ IzSmem S;
    const uint32_t lane = threadIdx.x;
    const uint32_t m = blockIdx.x;
    const BgzfMember M = meta[m];
    uint8_t *outb = reinterpret_cast<uint8_t *>(S.out);
    uint32_t fail = 0;
    // (the host pass made these true; a launch with other values must still stay inside its buffers)
    if (M.isize > BGZF_MAX_ISIZE || (uint64_t)M.in_off + M.in_len > src_len) fail = BGZF_E_TRUNC;
    const uint32_t isize = M.isize;

    for (uint32_t i = lane; i < 256; i += IZ_THREADS) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ 0xedb88320u : c >> 1;
        S.crc_table[i] = c;
    }
    if (lane == 0) {
        uint32_t p = 1u << 30;                 // x^1
        for (int k = 0; k < 32; k++) { S.x2n[k] = p; p = multmodp(p, p); }
        S.crc_acc = 0;
        S.out[isize / 4] = 0;                  // (the last word's unused bytes and the one past it: defined)
        if (isize / 4 + 1 <= BGZF_MAX_ISIZE / 4) S.out[isize / 4 + 1] = 0;
    }
    __syncthreads();

    IzBits br;
    br.in = src + M.in_off;
    br.n = fail ? 0u : M.in_len;
    br.start(0);
    uint32_t pos = 0, steps = 0;
    bool last = false;
    while (!fail && !last) {
        if (++steps > IZ_MAX_STEPS) { fail = BGZF_E_STEPS; break; }
        br.refill();
        last = br.take(1) != 0;
        const uint32_t btype = br.take(2);
        if (btype == 3) { fail = BGZF_E_BTYPE; break; }
        if (btype == 0) {
            br.drop(br.cnt & 7u);
            br.refill();
            const uint32_t len = br.take(16), nlen = br.take(16);
            if (br.overrun()) { fail = BGZF_E_TRUNC; break; }
            if ((len ^ nlen) != 0xffffu) { fail = BGZF_E_STORED; break; }
            const uint32_t at = br.pos - br.cnt / 8u;      // the byte after NLEN
            if (at + len > br.n) { fail = BGZF_E_TRUNC; break; }
            if (pos + len > isize) { fail = BGZF_E_PAST; break; }
            for (uint32_t i = lane; i < len; i += IZ_THREADS) outb[pos + i] = br.in[at + i];
            pos += len;
            br.start(at + len);
            continue;
        }
        if (btype == 1) {
            for (uint32_t i = lane; i < 288; i += IZ_THREADS) S.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
            if (lane < 32) S.lens[288 + lane] = 5;
            if (!iz_build(S, S.lens, 288, S.lcnt, S.lsym, S.ltab, IZ_LBITS, false) ||
                !iz_build(S, S.lens + 288, 32, S.dcnt, S.dsym, S.dtab, IZ_DBITS, false)) { fail = BGZF_E_LENS; break; }
        } else {
            const uint32_t hlit = br.take(5) + 257, hdist = br.take(5) + 1, hclen = br.take(4) + 4;
            if (hlit > 286 || hdist > 30) { fail = BGZF_E_LENS; break; }
            for (uint32_t i = 0; i < 19; i++) {
                br.refill();
                const uint32_t v = i < hclen ? br.take(3) : 0u;
                if (lane == 0) S.cl_lens[kClOrder[i]] = (uint8_t)v;
            }
            if (!iz_build(S, S.cl_lens, 19, S.ccnt, S.csym, nullptr, 0, true)) { fail = BGZF_E_LENS; break; }
            const uint32_t total = hlit + hdist;
            uint32_t idx = 0, prev = 0;
            while (idx < total) {              // (every round adds at least one length: at most 316 rounds)
                br.refill();
                uint32_t l;
                const uint32_t s = canon_decode(br.peek(), S.ccnt, S.csym, 7, l);
                if (!l) { fail = BGZF_E_LENS; break; }
                br.drop(l);
                uint32_t rep = 1, val = s;
                if (s == 16) {
                    if (idx == 0) { fail = BGZF_E_LENS; break; }
                    rep = 3 + br.take(2);
                    val = prev;
                } else if (s == 17) {
                    rep = 3 + br.take(3);
                    val = 0;
                } else if (s == 18) {
                    rep = 11 + br.take(7);
                    val = 0;
                }
                if (idx + rep > total) { fail = BGZF_E_LENS; break; }
                for (uint32_t i = lane; i < rep; i += IZ_THREADS) S.lens[idx + i] = (uint8_t)val;
                idx += rep;
                prev = val;
            }
            if (fail) break;
            if (br.overrun()) { fail = BGZF_E_TRUNC; break; }
            __syncthreads();
            if (S.lens[256] == 0) { fail = BGZF_E_LENS; break; }          // no end-of-block code
            if (!iz_build(S, S.lens, (int)hlit, S.lcnt, S.lsym, S.ltab, IZ_LBITS, false) ||
                !iz_build(S, S.lens + hlit, (int)hdist, S.dcnt, S.dsym, S.dtab, IZ_DBITS, false)) { fail = BGZF_E_LENS; break; }
        }
        // ---- the symbols of this block
        for (;;) {
            if (++steps > IZ_MAX_STEPS) { fail = BGZF_E_STEPS; break; }
            br.refill();
            uint32_t v = br.peek(), l, sym;
            const uint32_t e = S.ltab[v & ((1u << IZ_LBITS) - 1u)];
            if (e) {
                sym = e >> 4;
                l = e & 15u;
            } else {
                sym = canon_decode(v, S.lcnt, S.lsym, 15, l);
                if (!l) { fail = BGZF_E_CODE; break; }
            }
            br.drop(l);
            if (sym < 256) {
                if (pos >= isize) { fail = BGZF_E_PAST; break; }
                if (lane == 0) outb[pos] = (uint8_t)sym;
                pos++;
                wave_fence();
                continue;
            }
            if (sym == 256) break;
            sym -= 257;
            if (sym >= 29) { fail = BGZF_E_CODE; break; }
            uint32_t len;
            if (sym < 8) len = 3 + sym;
            else if (sym == 28) len = 258;
            else {
                const uint32_t eb = (sym >> 2) - 1;
                len = 3 + ((4 + (sym & 3u)) << eb) + br.take(eb);
            }
            br.refill();
            v = br.peek();
            uint32_t ds;
            const uint32_t de = S.dtab[v & ((1u << IZ_DBITS) - 1u)];
            if (de) {
                ds = de >> 4;
                l = de & 15u;
            } else {
                ds = canon_decode(v, S.dcnt, S.dsym, 15, l);
                if (!l) { fail = BGZF_E_CODE; break; }
            }
            br.drop(l);
            if (ds >= 30) { fail = BGZF_E_CODE; break; }
            uint32_t dist;
            if (ds < 4) dist = 1 + ds;
            else {
                const uint32_t eb = (ds >> 1) - 1;
                dist = 1 + ((2 + (ds & 1u)) << eb) + br.take(eb);
            }
            if (dist > pos) { fail = BGZF_E_DIST; break; }
            if (pos + len > isize) { fail = BGZF_E_PAST; break; }
            const uint32_t from = pos - dist;
            if (dist >= len || dist >= IZ_THREADS * 5) {     // (258 <= 64 * 5: i < dist for every i)
                for (uint32_t i = lane; i < len; i += IZ_THREADS) outb[pos + i] = outb[from + i];
            } else {
                for (uint32_t i = lane; i < len; i += IZ_THREADS) outb[pos + i] = outb[from + i % dist];
            }
            pos += len;
            wave_fence();
        }
        if (!fail && br.overrun()) fail = BGZF_E_TRUNC;
    }
    if (fail && fail != BGZF_E_STEPS && br.overrun()) fail = BGZF_E_TRUNC;    // (whatever the zeros past the end decoded to)
    if (!fail && pos != isize) fail = BGZF_E_ISIZE;
    __syncthreads();

    // ---- CRC32 of the produced bytes
    if (!fail) {
        const uint32_t span = (isize + IZ_THREADS - 1) / IZ_THREADS;
        const uint32_t a = lane * span < isize ? lane * span : isize, b = a + span < isize ? a + span : isize;
        uint32_t c = 0;
        for (uint32_t i = a; i < b; i++) c = S.crc_table[(c ^ outb[i]) & 0xff] ^ (c >> 8);
        uint32_t x = a < b ? multmodp(x8nmodp(S.x2n, isize - b), c) : 0;
        if (lane == 0) x ^= multmodp(x8nmodp(S.x2n, isize), 0xffffffffu);
        atomicXor(&S.crc_acc, x);
        __syncthreads();
        if ((S.crc_acc ^ 0xffffffffu) != M.crc) fail = BGZF_E_CRC;
    }
    if (fail) {
        if (lane == 0) atomicMin(err, (m << 4) | fail);
        return;
    }

    // ---- write-out: bytes up to the first 4-byte boundary of the destination, whole words, the tail
    uint8_t *o = dst + M.out_off;
    uint32_t head = (uint32_t)((4u - ((uintptr_t)o & 3u)) & 3u);
    if (head > isize) head = isize;
    if (lane < head) o[lane] = outb[lane];
    const uint32_t nw = (isize - head) / 4;
    uint32_t *o32 = reinterpret_cast<uint32_t *>(o + head);
    for (uint32_t w = lane; w < nw; w += IZ_THREADS) {
        const uint32_t s = head + 4 * w;
        o32[w] = __builtin_amdgcn_alignbyte(S.out[(s >> 2) + 1], S.out[s >> 2], s & 3u);
    }
    const uint32_t done = head + 4 * nw;
    if (lane < isize - done) o[done + lane] = outb[done + lane];
}

}  // namespace

const uint8_t BGZF_EOF[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

void bgzf_work_free(BgzfWork &w) {
    for (void *p : {(void *)w.d_ws, (void *)w.d_slots, (void *)w.d_meta, (void *)w.d_off, (void *)w.d_out})
        if (p) (void)hipFree(p);
    if (w.h_total) (void)hipHostFree(w.h_total);
    w = BgzfWork{};
}

// Compress bytes [0, n) of d_src (device) as ceil(n / BGZF_BLOCK) <= BGZF_PIECE_BLOCKS members into w.d_out on `st`;
// *out_bytes = their total size (synchronises `st`).  ev_start / ev_end (optional): recorded around the kernels.
hipError_t bgzf_compress_device(const uint8_t *d_src, uint64_t n, BgzfWork &w, hipStream_t st, uint64_t *out_bytes,
                                hipEvent_t ev_start, hipEvent_t ev_end) {
    *out_bytes = 0;
    if (!n) return hipSuccess;
    const uint64_t nblk = (n + BGZF_BLOCK - 1) / BGZF_BLOCK;
    if (nblk > BGZF_PIECE_BLOCKS) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    if (!w.d_ws) {
        const size_t B = BGZF_PIECE_BLOCKS;
        e = hipMalloc((void **)&w.d_ws, B * BGZF_BLOCK * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc((void **)&w.d_slots, B * BGZF_SLOT);
        if (e == hipSuccess) e = hipMalloc((void **)&w.d_meta, B * 3 * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc((void **)&w.d_off, (B + 1) * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMalloc((void **)&w.d_out, B * (BGZF_SLOT + 32));
        if (e == hipSuccess) e = hipHostMalloc((void **)&w.h_total, sizeof(uint64_t), hipHostMallocDefault);
        if (e != hipSuccess) { bgzf_work_free(w); return e; }
    }
    if (ev_start) (void)hipEventRecord(ev_start, st);
    k_bgzf_deflate<<<dim3((unsigned)nblk), dim3(BZ_THREADS), 0, st>>>(d_src, n, w.d_ws, w.d_slots, w.d_meta);
    k_bgzf_scan<<<dim3(1), dim3(1024), 0, st>>>(w.d_meta, (uint32_t)nblk, w.d_off);
    k_bgzf_pack<<<dim3((unsigned)nblk), dim3(256), 0, st>>>(w.d_slots, w.d_meta, w.d_off, w.d_out);
    e = hipGetLastError();
    if (e == hipSuccess && ev_end) e = hipEventRecord(ev_end, st);
    if (e == hipSuccess) e = hipMemcpyAsync(w.h_total, w.d_off + nblk, sizeof(uint64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = wait_stream(st);
    if (e == hipSuccess) *out_bytes = *w.h_total;
    return e;
}

const char *bgzf_inflate_reason(uint32_t code) {
    switch (code) {
    case BGZF_E_BTYPE: return "bad block type";
    case BGZF_E_LENS: return "invalid code lengths";
    case BGZF_E_CODE: return "invalid code";
    case BGZF_E_DIST: return "distance too far back";
    case BGZF_E_PAST: return "data past ISIZE";
    case BGZF_E_TRUNC: return "truncated";
    case BGZF_E_STORED: return "invalid stored block lengths";
    case BGZF_E_CRC: return "CRC32 mismatch";
    case BGZF_E_ISIZE: return "ISIZE mismatch";
    case BGZF_E_STEPS: return "too many symbols";
    default: return "unknown";
    }
}

bool bgzf_walk(const uint8_t *in, uint64_t n, uint64_t *uncompressed, uint64_t *n_members, std::vector<BgzfMemberHost> *members,
               std::string *why) {
    auto bad = [&](uint64_t at, const char *what) {
        if (why) *why = "offset " + std::to_string(at) + ": " + what;
        return false;
    };
    auto le16 = [&](uint64_t p) { return (uint32_t)in[p] | ((uint32_t)in[p + 1] << 8); };
    auto le32 = [&](uint64_t p) { return le16(p) | (le16(p + 2) << 16); };
    uint64_t pos = 0, total = 0, count = 0;
    if (n < 2 || in[0] != 0x1f || in[1] != 0x8b) return bad(0, "not gzip data");
    while (pos < n) {
        if (n - pos < 18) {
            if (in[pos] == 0x1f && (n - pos < 2 || in[pos + 1] == 0x8b)) return bad(pos, "truncated BGZF member");
            return bad(pos, "not a gzip member");
        }
        if (in[pos] != 0x1f || in[pos + 1] != 0x8b) return bad(pos, "not a gzip member");
        if (in[pos + 2] != 8 || in[pos + 3] != 4) return bad(pos, "gzip without BGZF framing (no extra field)");
        const uint64_t xlen = le16(pos + 10), x0 = pos + 12, x1 = x0 + xlen;
        if (x1 > n) return bad(pos, "truncated BGZF member");
        int64_t bsize = -1;
        for (uint64_t x = x0; x + 4 <= x1;) {
            const uint64_t slen = le16(x + 2);
            if (in[x] == 'B' && in[x + 1] == 'C' && slen == 2 && x + 6 <= x1) bsize = le16(x + 4);
            x += 4 + slen;
        }
        if (bsize < 0) return bad(pos, "gzip without BGZF framing (no BC subfield)");
        const uint64_t end = pos + (uint64_t)bsize + 1;
        if (end > n) return bad(pos, "BSIZE runs past the end of the file (truncated BGZF member)");
        if (end < x1 + 8) return bad(pos, "BSIZE smaller than the member's header and trailer");
        const uint32_t crc = le32(end - 8), isize = le32(end - 4);
        if (isize > BGZF_MAX_ISIZE) return bad(pos, "ISIZE above 65536: not BGZF");
        count++;
        if (isize) {
            if (members) members->push_back(BgzfMemberHost{pos, x1, (uint32_t)(end - 8 - x1), isize, crc});
            total += isize;
        }
        pos = end;
    }
    if (uncompressed) *uncompressed = total;
    if (n_members) *n_members = count;
    return true;
}

hipError_t bgzf_inflate_device(const uint8_t *d_in, uint32_t in_len, const BgzfMember *d_meta, uint32_t n, uint8_t *d_out,
                               uint32_t *d_err, hipStream_t st) {
    hipError_t e = hipMemsetAsync(d_err, 0xff, sizeof(uint32_t), st);
    if (e != hipSuccess || !n) return e;
    k_bgzf_inflate<<<dim3(n), dim3(IZ_THREADS), 0, st>>>(d_in, in_len, d_meta, d_out, d_err);
    return hipGetLastError();
}

}  // namespace msim
