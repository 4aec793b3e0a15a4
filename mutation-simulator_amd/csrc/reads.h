// FASTQ reads drawn from the resident genome ("reads" mode): the rule the device kernel (reads.hip: k_reads_render) and the
// sequential host restatement (msim_dbg_reads_render) share.  Integer arithmetic only; the host passes integer tables
// (mutation_simulator_amd/reads.py builds them), the device does no floating point.  include/msim.h states the rule in full.
//
//   placement  v = Philox4x32-10 (x = i, y = 0, z = 0, TAG_READ) under the run's key; p = below(lo64(v), P) picks contig and
//              start in one draw (the contig is the last eligible one with prefix_w[c] <= p, s = p - prefix_w[c]);
//              u = hi64(v) >> 11 picks the fragment length (frag_min + the first k with u < frag_thr[k]); hi64(v) & 1 the strand
//   bases      read base j of mate m comes from the genome forwards, g[s + j], where m == strand, and as the complement of
//              g[s + f - 1 - j] where they differ; a byte outside A, C, G, T gives 'N' with quality '!' and takes no error
//   errors     w = Philox4x32-10 (x = i, y = m << 16 | j >> 1, z = 0, TAG_RERR): the low 64 bits serve the even cycle, the
//              high 64 the odd one; substitute iff (word >> 11) < err_thr[m][j], by code (b + 1 + ((word & 0x7ff) * 3 >> 11)) & 3
//   record     "@<prefix><i>_<contig number>_<s + 1>_<f>_<+|->/<1|2>\n<bases>\n+\n<quals>\n", the four numbers zero-padded to
//              widths fixed per run: every record of a run is `stride` bytes long
#pragma once
#include <stdint.h>

#include "fast_math.h"
#include "spectrum.h"

namespace msim {
namespace reads {

constexpr uint32_t TAG_READ = 22;      // x = read (pair) index, y = 0: low 64 bits -> contig and start, high 64 -> fragment length (53 bits) and strand (bit 0)
constexpr uint32_t TAG_RERR = 23;      // x = read (pair) index, y = mate << 16 | cycle >> 1: low 64 bits -> the even cycle, high 64 -> the odd one
constexpr uint32_t MAX_LEN = 512, MAX_FRAG = 4096, MAX_PREFIX = 32;
constexpr uint64_t ONE53 = 1ull << 53;

// what a run fixes: the widths of the four numbers of a name and what follows from them
struct Layout {
    uint32_t len, plen, w_i, w_c, w_s, w_f;
    uint32_t name;                     // bytes of the name line, '@' and '\n' included
    uint32_t stride;                   // bytes of a record
};
MSIM_FHD inline uint32_t digits_of(uint64_t v) { uint32_t d = 1; while (v >= 10) { v /= 10; d++; } return d; }
MSIM_FHD inline Layout layout_of(uint32_t len, uint32_t plen, uint64_t max_i, uint64_t max_c, uint64_t max_s, uint64_t max_f) {
    Layout y;
    y.len = len; y.plen = plen;
    y.w_i = digits_of(max_i); y.w_c = digits_of(max_c); y.w_s = digits_of(max_s); y.w_f = digits_of(max_f);
    y.name = plen + y.w_i + y.w_c + y.w_s + y.w_f + 9;     // '@', four '_', the strand, '/', the mate, '\n' -- and the prefix
    y.stride = y.name + 2 * len + 4;                       // ... bases '\n' '+' '\n' quals '\n'
    return y;
}

struct Place { uint32_t c, s, f, strand; };                // c: ordinal among the ELIGIBLE contigs; s: 0-based start

// first k in [0, n) with u < thr[k] (thr ascending, thr[n - 1] = 2^53 > u)
MSIM_FHD inline uint32_t first_above(const uint64_t *thr, uint32_t n, uint64_t u) {
    uint32_t lo = 0, hi = n - 1;                           // the answer lies in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (u < thr[mid]) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// last c in [0, n) with prefix_w[c] <= p (prefix_w[0] = 0, ascending)
MSIM_FHD inline uint32_t last_at_or_below(const uint64_t *prefix_w, uint32_t n, uint64_t p) {
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (prefix_w[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}
MSIM_FHD inline Place place_of(const fastrng::Key &key, uint32_t i, const uint64_t *prefix_w, uint32_t n_elig, uint64_t P,
                               uint32_t frag_min, const uint64_t *frag_thr, uint32_t n_frag) {
    const fastrng::U4 v = fastrng::draw4(key, i, 0, TAG_READ);
    const uint64_t p = fastrng::below(fastrng::lo64(v), P), h = fastrng::hi64(v);
    Place pl;
    pl.c = last_at_or_below(prefix_w, n_elig, p);
    pl.s = (uint32_t)(p - prefix_w[pl.c]);
    pl.f = frag_min + first_above(frag_thr, n_frag, h >> 11);
    pl.strand = (uint32_t)(h & 1u);
    return pl;
}

// offset into the fragment's contig of the genome byte behind cycle j of mate m, and whether it is read off the other strand
MSIM_FHD inline uint32_t genome_offset(const Place &pl, uint32_t mate, uint32_t j, bool *complemented) {
    *complemented = mate != pl.strand;
    return *complemented ? pl.s + pl.f - 1 - j : pl.s + j;
}
// base and quality of one cycle: g the genome byte, word the cycle's 64 random bits
MSIM_FHD inline void cycle_of(uint32_t g, bool complemented, uint64_t word, uint64_t err_thr, uint8_t q, uint8_t *base, uint8_t *qual) {
    uint32_t b = spectrum::base_code(g);
    if (b == spectrum::CODE_INVALID) { *base = 'N'; *qual = '!'; return; }
    if (complemented) b = 3u - b;
    if ((word >> 11) < err_thr) b = (b + 1u + (uint32_t)(((word & 0x7ffu) * 3u) >> 11)) & 3u;
    *base = (uint8_t)(0x54474341u >> (8 * b));             // A, C, G, T
    *qual = q;
}
MSIM_FHD inline uint64_t cycle_word(const fastrng::U4 &w, uint32_t j) { return (j & 1u) ? fastrng::hi64(w) : fastrng::lo64(w); }

// byte k of the name line (0 <= k < y.name): i the read index, cnum the contig's 1-based number in the Fasta
MSIM_FHD inline uint8_t name_byte(const Layout &y, const uint8_t *prefix, uint32_t k, uint64_t i, uint32_t cnum, const Place &pl,
                                  uint32_t mate) {
    if (k == 0) return '@';
    k -= 1;
    if (k < y.plen) return prefix[k];
    k -= y.plen;
    const uint64_t num[4] = {i, cnum, (uint64_t)pl.s + 1, pl.f};
    const uint32_t wid[4] = {y.w_i, y.w_c, y.w_s, y.w_f};
    for (int q = 0; q < 4; q++) {
        if (k < wid[q]) {
            uint64_t v = num[q];
            for (uint32_t d = wid[q] - 1 - k; d; d--) v /= 10;
            return (uint8_t)('0' + v % 10);
        }
        k -= wid[q];
        if (k == 0) return '_';
        k -= 1;
    }
    return k == 0 ? (pl.strand ? '-' : '+') : k == 1 ? '/' : k == 2 ? (uint8_t)('1' + mate) : '\n';
}

}  // namespace reads
}  // namespace msim
