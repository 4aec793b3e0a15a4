// compare --blocks ("rescue unmatched records by replaying blocks"): what the device kernels (cmp_blocks.hip) and the sequential
// host restatement (msim_dbg_cmp_counts_blocks) share -- the block rule of include/msim.h, integer and byte arithmetic only.
//
//   foot_end   the last input base a record's footprint covers: stop for DE, DU, IV and TL, pos for SN, IN and TLI
//   is_head    does record i of one table start a block?  Its predecessor in its own table and its predecessor in the other one
//              (a binary search) are the two records whose footprint can reach it: a table's records do not overlap, so the
//              last record of a table in front of a pos is the one of that table that ends last
//   walk       from a head through the merged order (truth first at equal pos) to the record that starts the next block: is any
//              record unmatched (a candidate), which stop rule ends the walk early, the block's index ranges in both tables
//   Cursor     one side's bytes over the block's input bases [lo, hi], one byte a step or one stretch of memory a step: (record
//              index, input position, offset inside the record's own output) -- the rewrite's rules record by record (tests/apply_ref.py is the restatement the
//              tests hold it against).  Nothing is buffered: two cursors are stepped side by side and compared.
// Every table index is checked against its table's size, every base read against L, every pool read against the pool's length.
#pragma once
#include "compare.h"

namespace msim {
namespace blk {

constexpr uint32_t MAX_RECORDS = MSIM_CMP_BLOCK_RECORDS, MAX_SPAN = MSIM_CMP_BLOCK_SPAN;
// block_tallies[5] of msim_cmp_counts_blocks
constexpr uint32_t T_CANDIDATE = 0, T_REPLAYED = 1, T_EQUAL = 2, T_LIMIT = 3, T_TRANSLOCATION = 4, TALLIES = 5;
// what a walk found
constexpr uint32_t NOT_A_CANDIDATE = 0, REPLAY = 1, OVER_LIMIT = 2, TRANSLOCATION = 3;

struct Desc { uint32_t ia0, ia1, ib0, ib1; };              // a block to replay: truth records [ia0, ia1), calls records [ib0, ib1)

MSIM_FHD inline bool spans(uint32_t type) {
    return type == (uint32_t)MSIM_DE || type == (uint32_t)MSIM_DU || type == (uint32_t)MSIM_IV || type == (uint32_t)MSIM_TL;
}
MSIM_FHD inline uint32_t foot_end(const cmp::Rec &r) { return spans(r.type) && r.stop > r.pos ? r.stop : r.pos; }
MSIM_FHD inline bool translocation(uint32_t type) { return type == (uint32_t)MSIM_TL || type == (uint32_t)MSIM_TLI; }

// the first record of t behind pos (t.n: none)
MSIM_FHD inline uint64_t first_behind(const cmp::Table &t, uint32_t pos) {
    uint64_t lo = 0, hi = t.n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (cmp::rec_at(t.recs, mid).pos <= pos) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// does a record at pos stand within `gap` bases behind a footprint that ends at `end` (or inside it)?
MSIM_FHD inline bool reaches(uint32_t end, uint32_t pos, uint32_t gap) { return (int64_t)pos - (int64_t)end <= (int64_t)gap; }

// Record i of `own` (the truth's table iff own_is_truth) against the other table: on a head *other = the other table's records in
// front of it in merged order -- where the walk of a block that starts here begins there.
MSIM_FHD inline bool is_head(const cmp::Table &own, uint64_t i, const cmp::Table &oth, bool own_is_truth, uint32_t gap, uint64_t *other) {
    const cmp::Rec r = cmp::rec_at(own.recs, i);
    if (i > 0 && reaches(foot_end(cmp::rec_at(own.recs, i - 1)), r.pos, gap)) return false;   // (one load spares most records the search)
    const uint64_t k = own_is_truth ? cmp::first_at(oth, r.pos) : first_behind(oth, r.pos);
    *other = k;
    if (k > 0 && k <= oth.n && reaches(foot_end(cmp::rec_at(oth.recs, k - 1)), r.pos, gap)) return false;
    return true;
}

// The block that starts with truth record ia / calls record ib (one of them is its head; the other index: is_head's *other).
// fa, fb: the flag bytes of the match (0 / 1).  Returns what the block is; d: its index ranges when it is to be replayed.
MSIM_FHD inline uint32_t walk(const cmp::Table &A, const cmp::Table &B, const uint8_t *fa, const uint8_t *fb, uint64_t ia, uint64_t ib,
                              uint32_t gap, Desc *d) {
    const uint64_t ia0 = ia, ib0 = ib;
    uint32_t lo = 0, end = 0, n = 0, stopped = 0;
    bool unmatched = false, load_a = true, load_b = true;
    cmp::Rec a{}, b{};
    for (;;) {
        const bool have_a = ia < A.n, have_b = ib < B.n;
        if (!have_a && !have_b) break;
        if (have_a && load_a) a = cmp::rec_at(A.recs, ia);                   // (one load a step: the side the last step took)
        if (have_b && load_b) b = cmp::rec_at(B.recs, ib);
        load_a = load_b = false;
        const bool take_a = have_a && (!have_b || a.pos <= b.pos);           // truth first at equal pos
        const cmp::Rec &r = take_a ? a : b;
        if (n == 0) { lo = r.pos; end = r.pos; }
        else if (!reaches(end, r.pos, gap)) break;                           // the next block's head
        const uint32_t e = foot_end(r);
        if (e > end) end = e;
        n++;
        if (!(take_a ? fa[ia] : fb[ib])) unmatched = true;
        if (!stopped) {                                                      // the first record that meets a stop rule decides
            if (translocation(r.type)) stopped = TRANSLOCATION;
            else if (n > MAX_RECORDS || e - lo > MAX_SPAN) stopped = OVER_LIMIT;
        }
        if (take_a) { ia++; load_a = true; } else { ib++; load_b = true; }
        if (stopped && unmatched) break;                                     // (a stopped block is walked on only to learn whether it is a candidate)
    }
    if (!unmatched) return NOT_A_CANDIDATE;
    if (stopped) return stopped;
    *d = Desc{(uint32_t)ia0, (uint32_t)ia, (uint32_t)ib0, (uint32_t)ib};
    return REPLAY;
}

// ---- the rewrite's bytes (mutator.py:75-77, 449-455): the LUT of apply.hip again, as tables the compiler folds -- the host
// restatement has no context to take the device's LUT from.  (Tables, not switches: written as switches over the byte these functions
// returned 'G' for C, N and T on the device -- and the right bytes on the host --, which the device tests caught; the cause was not
// established, NOTES 29.)
struct ByteMap { uint8_t v[256]; };
// the identity but for from[i] -> to[i]
constexpr ByteMap byte_map(const char *from, const char *to) {
    ByteMap m{};
    for (int i = 0; i < 256; i++) m.v[i] = (uint8_t)i;
    for (int i = 0; from[i]; i++) m.v[(uint8_t)from[i]] = (uint8_t)to[i];
    return m;
}
constexpr ByteMap NON_AMBIGUOUS = byte_map("KSYMWRBDHV-", "GCCAAACAAAN");
// column `aux` of an SN on a de-ambiguated base: the transition, the two transversions (0: the reference's KeyError)
constexpr ByteMap snp_map(uint32_t aux) {
    const ByteMap ti = byte_map("AGTC", "GACT");
    const char *col = aux == 1 ? "TCGAN" : "CTAGN";        // of A, G, T, C, N
    ByteMap m{};
    for (int i = 0; i < 256; i++) {
        const uint8_t r = NON_AMBIGUOUS.v[i];
        uint8_t out = aux == 0 ? ti.v[r] : (uint8_t)0;
        for (int k = 0; aux != 0 && k < 5; k++) if (r == (uint8_t)"AGTCN"[k]) out = (uint8_t)col[k];
        m.v[i] = out;
    }
    return m;
}
constexpr ByteMap reverse_complement_map() {
    const ByteMap comp = byte_map("ACGTUMRWSYKVHDB", "TGCAAKYWSRMBDHV");
    ByteMap m{};
    for (int i = 0; i < 256; i++) m.v[i] = comp.v[NON_AMBIGUOUS.v[i]];
    return m;
}
// an SN's output byte on input byte x; 0: the rewrite has none (its KeyError: a transversion of a base outside A, C, G, T, N)
MSIM_FHD inline uint32_t snp_byte(uint32_t x, uint32_t aux) {
    constexpr ByteMap TI = snp_map(0), TV0 = snp_map(1), TV1 = snp_map(2);
    const uint32_t i = x & 0xffu;
    return aux == 0 ? TI.v[i] : aux == 1 ? TV0.v[i] : TV1.v[i];
}
// an IV's output byte for input byte x: the complement of the de-ambiguated base
MSIM_FHD inline uint32_t iv_byte(uint32_t x) {
    constexpr ByteMap RC = reverse_complement_map();
    return RC.v[x & 0xffu];
}

constexpr int END = -1, BAD = -2;                          // Cursor::next: the stream is over / has no bytes the rewrite would write

// One side's output over the input bases [at, hi] with the records [k, k1) of table t: next() gives the next byte, END behind the
// last, BAD for a record the rewrite is not written for (an insert outside its pool, a span beyond the contig, an SN without an
// outcome) -- the block is then unequal.  A record that starts in front of the input position (an overlap no planner makes) is
// passed over, so every call moves k, at or off forward: the cursor ends.
struct Cursor {
    uint64_t k, k1, at, hi;                                // the next record, the block's last + 1; the next input base, the last one
    uint32_t off;                                          // inside a record: the bytes of its own output already given
    bool loaded, in_rec;                                   // r is record k; the cursor stands inside it
    cmp::Rec r;

    // hi < L: the caller's (replay_equal)
    MSIM_FHD Cursor(uint64_t k0, uint64_t k1_, uint32_t lo, uint32_t hi_) : k(k0), k1(k1_), at(lo), hi(hi_), off(0), loaded(false), in_rec(false), r{} {}

    MSIM_FHD void leave(uint64_t next_at) { in_rec = loaded = false; k++; at = next_at; }

    // between records, at <= hi: r becomes the next record at or behind `at`; is there one?
    MSIM_FHD bool settle(const cmp::Table &t) {
        while (k < k1 && k < t.n) {
            if (!loaded) { r = cmp::rec_at(t.recs, k); loaded = true; }
            if (r.pos >= at) return true;
            k++;
            loaded = false;
        }
        return false;
    }

    // The cursor's next bytes where they lie in memory as they come out -- the contig's bases it copies between records, a DU's
    // span (either copy), an IN's insert: *p and the length, which advance() then consumes in whole or in part.  0: ask next().
    // *reversed: an IV's bytes, which come out of memory backwards from *p and complemented -- of use only to see that two cursors
    // stand in the same inversion.  Two cursors that stand on the SAME stretch need not read it, and two different forward
    // stretches compare in a plain loop: the replay spends its steps on what the records write differently.
    MSIM_FHD uint32_t stretch(const uint8_t *g, uint64_t L, const cmp::Table &t, const uint8_t **p, bool *reversed) {
        *reversed = false;
        if (!in_rec) {
            if (at > hi) return 0;
            const bool more = settle(t);
            if (!(more && r.pos == at)) {
                const uint64_t end = more && r.pos <= hi ? r.pos : hi + 1;          // (at < end <= hi + 1 <= L)
                *p = g + at;
                return (uint32_t)(end - at);
            }
            in_rec = true;
            off = 0;
        }
        const uint32_t n = r.stop >= r.pos ? r.stop - r.pos + 1u : 0u;
        if (r.type == (uint32_t)MSIM_IN && n && r.extra <= t.pool_len && n <= t.pool_len - r.extra && off < n) {
            *p = t.pool + (uint64_t)r.extra + off;
            return n - off;
        }
        if (r.type == (uint32_t)MSIM_DU && n && r.stop < L && (off < n || off - n < n)) {
            const uint32_t o = off >= n ? off - n : off;
            *p = g + (uint64_t)r.pos + o;
            return n - o;
        }
        if (r.type == (uint32_t)MSIM_IV && n && r.stop < L && off < n) {
            *reversed = true;
            *p = g + ((uint64_t)r.stop - off);
            return n - off;
        }
        return 0;
    }
    MSIM_FHD void advance(uint32_t n) { if (in_rec) off += n; else at += n; }

    MSIM_FHD int next(const uint8_t *g, uint64_t L, const cmp::Table &t) {
        for (;;) {
            if (!in_rec) {
                if (at > hi) return END;
                if (!(settle(t) && r.pos == at)) return (int)g[at++];               // (at <= hi < L)
                in_rec = true;
                off = 0;
            }
            // inside record r, which starts at input base `at` (<= hi): byte `off` of what it writes
            const uint32_t n = r.stop >= r.pos ? r.stop - r.pos + 1u : 0u;
            switch (r.type) {
                case MSIM_SN: {
                    const uint32_t alt = snp_byte(g[at], r.aux);
                    leave(at + 1);
                    return alt ? (int)alt : BAD;
                }
                case MSIM_IN: {
                    if (!n || r.extra > t.pool_len || n > t.pool_len - r.extra) return BAD;
                    if (off < n) return (int)t.pool[(uint64_t)r.extra + off++];
                    const int x = (int)g[at];              // the base it stands in front of
                    leave(at + 1);
                    return x;
                }
                case MSIM_DE:
                    if (!n || r.stop >= L) return BAD;
                    leave((uint64_t)r.stop + 1);
                    continue;
                case MSIM_DU:
                    if (!n || r.stop >= L) return BAD;
                    if (off < n || off - n < n) { const uint32_t o = off++; return (int)g[(uint64_t)r.pos + (o >= n ? o - n : o)]; }
                    leave((uint64_t)r.stop + 1);
                    continue;
                case MSIM_IV:
                    if (!n || r.stop >= L) return BAD;
                    if (off < n) return (int)iv_byte(g[(uint64_t)r.stop - off++]);
                    leave((uint64_t)r.stop + 1);
                    continue;
                default:
                    return BAD;                            // TL, TLI (never replayed), an unknown type
            }
        }
    }
};

// the block's input bases: from the first pos to the largest footprint end (a table's records end in table order)
MSIM_FHD inline void input_span(const cmp::Table &A, const cmp::Table &B, const Desc &d, uint32_t *lo, uint32_t *hi) {
    uint32_t l = 0xffffffffu, h = 0;
    if (d.ia0 < d.ia1 && d.ia1 <= A.n) {
        l = cmp::rec_at(A.recs, d.ia0).pos;
        h = foot_end(cmp::rec_at(A.recs, (uint64_t)d.ia1 - 1));
    }
    if (d.ib0 < d.ib1 && d.ib1 <= B.n) {
        const uint32_t p = cmp::rec_at(B.recs, d.ib0).pos, e = foot_end(cmp::rec_at(B.recs, (uint64_t)d.ib1 - 1));
        if (p < l) l = p;
        if (e > h) h = e;
    }
    *lo = l;
    *hi = h;
}

// Do the truth's records of the block alone and the calls' records alone write the same bytes over the block's input bases?
// *steps (optional): the bytes it compared to find out.
MSIM_FHD inline bool replay_equal(const uint8_t *g, uint64_t L, const cmp::Table &A, const cmp::Table &B, const Desc &d, uint32_t *steps = nullptr) {
    if (d.ia1 > A.n || d.ib1 > B.n || d.ia0 > d.ia1 || d.ib0 > d.ib1) return false;
    uint32_t lo, hi;
    input_span(A, B, d, &lo, &hi);
    if (lo > hi || hi >= L) return false;
    Cursor ca(d.ia0, d.ia1, lo, hi), cb(d.ib0, d.ib1, lo, hi);
    for (uint32_t done = 0;;) {
        const uint8_t *pa, *pb;
        bool ra, rb;
        const uint32_t la = ca.stretch(g, L, A, &pa, &ra), lb = cb.stretch(g, L, B, &pb, &rb);
        if (la && lb && ra == rb && (pa == pb || !ra)) {   // both in memory: the same bytes are equal unread, others compare in a loop
            const uint32_t n = la < lb ? la : lb;
            done += pa == pb ? 1u : n;
            if (steps) *steps = done;
            if (pa != pb)
                for (uint32_t i = 0; i < n; i++) if (pa[i] != pb[i]) return false;
            ca.advance(n);
            cb.advance(n);
            continue;
        }
        const int x = ca.next(g, L, A), y = cb.next(g, L, B);
        if (steps) *steps = ++done;
        if (x == BAD || y == BAD || x != y) return false;
        if (x == END) return true;
    }
}

// an equal block: every unmatched record of it, on both sides, is matched as part of a block
MSIM_FHD inline void rescue(uint8_t *fa, uint8_t *fb, const Desc &d) {
    for (uint64_t i = d.ia0; i < d.ia1; i++) if (!fa[i]) fa[i] = 2;
    for (uint64_t j = d.ib0; j < d.ib1; j++) if (!fb[j]) fb[j] = 2;
}

// ---- the device pass (cmp_blocks.hip), as compare.hip enqueues it -------------------------------------------------------------------
// The counters the two kernels leave on the device: HIST_SLOTS copies of PASS_BINS tallies (lane_hist.h; the host sums them), and
// behind them three words: the descriptors appended; the bytes the replay's lanes compared; 64 x the most bytes a lane of each wave
// compared, summed over the waves -- the lane-steps the replay's waves occupied (their ratio: what divergence leaves of a wave).
constexpr uint32_t PASS_BINS = 8;                          // TALLIES, rounded up to an even number of lane-private bins
constexpr size_t PASS_COUNT_AT = (size_t)16 * PASS_BINS, PASS_STEPS_AT = PASS_COUNT_AT + 1, PASS_WAVE_STEPS_AT = PASS_COUNT_AT + 2,
                 PASS_WORDS = PASS_COUNT_AT + 3;           // (16: HIST_SLOTS, asserted in cmp_blocks.hip)

}  // namespace blk

struct Ctx;
// k_blk_scan and k_blk_replay on `stream`: flag bytes 0 / 1 in, 0 / 1 / 2 out.  desc: room for `cap` descriptors (a block to
// replay holds a record: the two tables' records together are enough); out: PASS_WORDS words, zeroed by the caller; between: an
// event recorded between the two kernels.
int blocks_enqueue(Ctx *c, hipStream_t stream, const uint8_t *g, uint64_t L, const cmp::Table &A, const cmp::Table &B, uint8_t *fa,
                   uint8_t *fb, uint32_t gap, blk::Desc *desc, uint64_t cap, unsigned long long *out, hipEvent_t between);

}  // namespace msim
