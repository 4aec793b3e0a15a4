// The compare mode ("compare truth.vcf calls.vcf"): what the device kernels (compare.hip) and the sequential host restatement
// (msim_dbg_cmp_counts) share -- the matching rules of include/msim.h, integer and byte arithmetic only.
//
//   interval   an IN / DE record's placements [lo, hi]: the walk to the left and to the right, one base a step, each step
//              checked in this order -- the contig's end (stops silently), the genome byte the step compares (not A, C, G or T:
//              stops, STOP_BASE), the comparison itself (stops silently), the window of the record's pos (stops, STOP_WINDOW)
//   same       two records are one variant: type and length, the other's pos inside the interval (the caller's scan sees to
//              that), an insert's bytes up to the rotation by the distance; every other type field by field
//   partner    the rank of record i in its class among A's records to the left, the record of that rank in B's scan of
//              [lo, hi]
//   join       a side's two haplotype tables as one diploid table U with a genotype byte per record (compare --diploid): where a
//              record of either table lands in U, which records of haplotype 2 are haplotype 1's again (join_dup)
// A, B: position-sorted tables.  A planner's table and msim_dbg_set_records' have pos strictly increasing; a diploid table U has
// pos NON-DECREASING with at most two records at one pos, haplotype 1's first, and never two of one class there: `same` at
// distance 0 means identical, and the join wrote every identical pair once.  partner's rank (a scan to the left while pos >= lo)
// and its scan of B (from the first record at or behind lo) count records of the class, whatever shares their pos, so both stay
// correct on U.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/msim.h"
#include "fast_math.h"
#include "lane_hist.h"

namespace msim {
namespace cmp {

constexpr uint32_t WINDOW_SHIFT = 16;                      // MSIM_CMP_WINDOW = 1 << 16
constexpr uint32_t STOP_WINDOW = 1u, STOP_BASE = 2u;       // why a walk ended (Span::stops): msim_cmp_counts' two tallies
constexpr uint32_t CELLS = 15;                             // (type, bin) pairs that exist: 7 types in bin 0, IN and DE in bins 1..4
static_assert(MSIM_CMP_BINS == 5, "the cells are laid out for five length bins");

// A comparison's counters, by the OUTCOMES a record of a cell can have: 2 (haploid: matched / unmatched) or 3 (diploid: matched /
// genotype-mismatched / unmatched).  A record's flag byte names its outcome: 1 matched, 2 (diploid only) matched with another
// dosage, 0 no partner -- the last outcome.
template <int OUTCOMES>
struct Score {
    static_assert(OUTCOMES == 2 || OUTCOMES == 3, "haploid or diploid");
    static constexpr uint32_t TALLIES = OUTCOMES * CELLS;  // behind the cells' counters: the two tallies
    static constexpr uint32_t COUNTERS = TALLIES + 2;
    static constexpr uint32_t BINS = (COUNTERS + 1) & ~1u; // ... rounded up to an even number of lane-private bins: 32, 48
};

// What the kernels that count a comparison's records share (k_cmp_match<>, k_cmp_tally<>, k_region_tally<>): LANES lanes a
// workgroup and a record a lane and pass; lane-private bins, summed in two halves into the workgroup's slot of `out` -- OUT_WORDS
// counters: HIST_SLOTS slots of 2 x BINS words, the truth's counters in front of the calls' (lane_hist.h).
constexpr int LANES = 256;
template <int OUTCOMES> using Hist = LaneHist<(int)Score<OUTCOMES>::BINS, LANES, 2>;
template <int OUTCOMES> constexpr size_t OUT_WORDS = (size_t)HIST_SLOTS * 2 * Score<OUTCOMES>::BINS;
template <int OUTCOMES>
__device__ __forceinline__ unsigned long long *slot_of(unsigned long long *out) {
    return out + (blockIdx.x & (HIST_SLOTS - 1)) * 2 * Score<OUTCOMES>::BINS;
}

struct Rec { uint32_t pos, stop, extra, type, aux; };
struct Table { const msim_record *recs; uint64_t n; const uint8_t *pool; uint64_t pool_len; };
struct Span { uint32_t lo, hi, stops; };

MSIM_FHD inline Rec rec_at(const msim_record *t, uint64_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 w = reinterpret_cast<const uint4 *>(t)[i];  // one 16-byte load (tables are device allocations: aligned)
    return Rec{w.x, w.y, w.z, w.w & 0xffu, (w.w >> 8) & 0xffu};
#else
    return Rec{t[i].pos, t[i].stop, t[i].extra, t[i].type, t[i].aux};
#endif
}

MSIM_FHD inline bool acgt(uint32_t b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T'; }
MSIM_FHD inline bool known_type(uint32_t type) { return type >= (uint32_t)MSIM_SN && type <= (uint32_t)MSIM_TLI; }
MSIM_FHD inline bool indel(uint32_t type) { return type == (uint32_t)MSIM_IN || type == (uint32_t)MSIM_DE; }
MSIM_FHD inline uint32_t len_bin(uint32_t n) { return n <= 1 ? 0u : n <= 5 ? 1u : n <= 20 ? 2u : n <= 50 ? 3u : 4u; }
// the cell of a record: its type in bin 0, an indel's in its length bin
MSIM_FHD inline uint32_t cell_of(const Rec &r) {
    const uint32_t bin = indel(r.type) ? len_bin(r.stop - r.pos + 1u) : 0u;
    return bin == 0 ? r.type - 1u : (r.type == (uint32_t)MSIM_IN ? 6u : 10u) + bin;
}
// ... and back: counts[type][bin] of the cell
MSIM_FHD inline void cell_index(uint32_t cell, uint32_t *type, uint32_t *bin) {
    if (cell < 7) { *type = cell + 1; *bin = 0; }
    else if (cell < 11) { *type = MSIM_IN; *bin = cell - 6; }
    else { *type = MSIM_DE; *bin = cell - 10; }
}
// the counter of a record with that flag byte
template <int OUTCOMES>
MSIM_FHD inline uint32_t counter_of(const Rec &r, uint32_t flag) { return OUTCOMES * cell_of(r) + (flag ? flag - 1u : OUTCOMES - 1u); }

// host: a[], b[] -- the truth's and the calls' counters, per cell its outcomes -- added to counts[type][bin][side][outcome]
template <int OUTCOMES>
inline void fold_cells(const unsigned long long *a, const unsigned long long *b, uint64_t *counts) {
    for (uint32_t cell = 0; cell < CELLS; cell++) {
        uint32_t type, bin;
        cell_index(cell, &type, &bin);
        uint64_t *dst = counts + ((size_t)type * MSIM_CMP_BINS + bin) * 2 * OUTCOMES;
        for (int k = 0; k < OUTCOMES; k++) { dst[k] += a[OUTCOMES * cell + k]; dst[OUTCOMES + k] += b[OUTCOMES * cell + k]; }
    }
}

// an indel the walk is written for: inside the contig, an insert inside its pool (what table_check guarantees, checked again
// because nothing else keeps a read inside its buffer)
MSIM_FHD inline bool walkable(const Rec &r, uint64_t L, uint64_t pool_len) {
    if (!indel(r.type) || r.stop < r.pos || r.pos >= L) return false;
    const uint64_t n = (uint64_t)r.stop - r.pos + 1;
    return r.type == (uint32_t)MSIM_DE ? r.stop < L : (r.extra <= pool_len && n <= pool_len - r.extra);
}

MSIM_FHD inline Span interval(const uint8_t *g, uint64_t L, const Rec &a, const uint8_t *pool, uint64_t pool_len, bool exact) {
    Span s{a.pos, a.pos, 0u};
    if (exact || !walkable(a, L, pool_len)) return s;
    const uint32_t n = a.stop - a.pos + 1u, win = a.pos >> WINDOW_SHIFT;
    const bool del = a.type == (uint32_t)MSIM_DE;
    const uint8_t *S = pool + a.extra;
    {   // to the left: g[p - 1] against the deletion's last base g[p + n - 1] / the insert's last byte, which rotates
        uint32_t p = a.pos, k = n - 1;
        while (p > 0) {
            const uint32_t in = g[p - 1];
            if (!acgt(in)) { s.stops |= STOP_BASE; break; }
            if (in != (del ? (uint32_t)g[(uint64_t)p + n - 1] : (uint32_t)S[k])) break;
            if (((p - 1) >> WINDOW_SHIFT) != win) { s.stops |= STOP_WINDOW; break; }
            p--;
            k = k ? k - 1 : n - 1;
        }
        s.lo = p;
    }
    {   // to the right: the base behind the deletion g[p + n] against its first g[p] / g[p] against the insert's first byte
        uint64_t p = a.pos;
        uint32_t k = 0;
        while (del ? p + n < L : p + 1 < L) {
            const uint32_t in = del ? g[p + n] : g[p];
            if (!acgt(in)) { s.stops |= STOP_BASE; break; }
            if (in != (del ? (uint32_t)g[p] : (uint32_t)S[k])) break;
            if (((p + 1) >> WINDOW_SHIFT) != win) { s.stops |= STOP_WINDOW; break; }
            p++;
            k = k + 1 == n ? 0 : k + 1;
        }
        s.hi = (uint32_t)p;
    }
    return s;
}

// Is b the variant a is?  For indels the caller has b.pos inside a's interval; an insert's bytes: S_b[i] == S_a[(i + d) mod n],
// d = b.pos - a.pos.  pool_b / pool_b_len: the pool b's insert lies in (a's own was checked by walkable()).
MSIM_FHD inline bool same(const Rec &a, const uint8_t *pool_a, bool a_walkable, const Rec &b, const uint8_t *pool_b,
                          uint64_t pool_b_len) {
    if (a.type != b.type) return false;
    if (!indel(a.type))
        return a.pos == b.pos && a.aux == b.aux && (a.type == (uint32_t)MSIM_SN || a.stop == b.stop) &&
               (a.type != (uint32_t)MSIM_TLI || a.extra == b.extra);
    if (!a_walkable || b.stop < b.pos || b.stop - b.pos != a.stop - a.pos) return false;
    if (a.type == (uint32_t)MSIM_DE) return true;
    const uint32_t n = a.stop - a.pos + 1u;
    if (b.extra > pool_b_len || n > pool_b_len - b.extra) return false;
    const int64_t d = (int64_t)b.pos - (int64_t)a.pos;
    uint32_t k = (uint32_t)(((d % (int64_t)n) + (int64_t)n) % (int64_t)n);
    const uint8_t *Sa = pool_a + a.extra, *Sb = pool_b + b.extra;
    for (uint32_t i = 0; i < n; i++) {
        if (Sb[i] != Sa[k]) return false;
        k = k + 1 == n ? 0 : k + 1;
    }
    return true;
}

// The record of B that A's record i matches, or -1; *span: i's interval and why its walks ended.
MSIM_FHD inline int64_t partner(const uint8_t *g, uint64_t L, const Table &A, uint64_t i, const Table &B, bool exact, Span *span) {
    const Rec a = rec_at(A.recs, i);
    const Span s = interval(g, L, a, A.pool, A.pool_len, exact);
    *span = s;
    const bool ok = !indel(a.type) || walkable(a, L, A.pool_len);
    uint64_t rank = 0;                                     // records of a's class in front of it
    for (uint64_t j = i; j > 0; j--) {
        const Rec o = rec_at(A.recs, j - 1);
        if (o.pos < s.lo) break;
        if (same(a, A.pool, ok, o, A.pool, A.pool_len)) rank++;
    }
    uint64_t lo = 0, hi = B.n;                             // the first record of B at or behind s.lo
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (rec_at(B.recs, mid).pos < s.lo) lo = mid + 1; else hi = mid;
    }
    for (uint64_t j = lo; j < B.n; j++) {
        const Rec o = rec_at(B.recs, j);
        if (o.pos > s.hi) break;
        if (same(a, A.pool, ok, o, B.pool, B.pool_len)) {
            if (rank == 0) return (int64_t)j;
            rank--;
        }
    }
    return -1;
}

// ---- the diploid join (msim_cmp_join, msim_dbg_cmp_join) -------------------------------------------------------------------------
// a genotype byte's dosage: the haplotypes that carry the record (bit 0: haplotype 1, bit 1: haplotype 2)
MSIM_FHD inline uint32_t dosage(uint32_t gt) { return (gt & 1u) + ((gt >> 1) & 1u); }
// the flag byte of a matched pair: 1 the same dosage, 2 a genotype mismatch (0: no partner)
MSIM_FHD inline uint8_t pair_flag(uint32_t gt_a, uint32_t gt_b) { return dosage(gt_a) == dosage(gt_b) ? (uint8_t)1 : (uint8_t)2; }

// the records of t in front of pos: the index of the first record at or behind it (t.n: none)
MSIM_FHD inline uint64_t first_at(const Table &t, uint32_t pos) {
    uint64_t lo = 0, hi = t.n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (rec_at(t.recs, mid).pos < pos) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// what `same` asks of its first record in place of walkable(): a length, an insert inside its pool.  (The join compares at
// distance 0 and walks nowhere, so the contig's length does not come into it.)
MSIM_FHD inline bool comparable(const Rec &r, uint64_t pool_len) {
    if (!indel(r.type)) return true;
    if (r.stop < r.pos) return false;
    const uint64_t n = (uint64_t)r.stop - r.pos + 1;
    return r.type == (uint32_t)MSIM_DE || (r.extra <= pool_len && n <= pool_len - r.extra);
}
// Is H2's record j a record of H1 again?  *in_front: H1's records at or in front of its pos -- where it lands among them, H1's
// record coming first at equal pos.
MSIM_FHD inline bool join_dup(const Table &H1, const Table &H2, uint64_t j, uint64_t *in_front) {
    const Rec b = rec_at(H2.recs, j);
    const uint64_t i = first_at(H1, b.pos);
    *in_front = i;
    if (i >= H1.n) return false;
    const Rec a = rec_at(H1.recs, i);
    if (a.pos != b.pos) return false;
    *in_front = i + 1;
    return same(a, H1.pool, comparable(a, H1.pool_len), b, H2.pool, H2.pool_len);
}

}  // namespace cmp
}  // namespace msim
