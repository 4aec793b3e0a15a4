// The compare mode's device side (msim_cmp_*): a HELD record table (the truth, A) scored against the contig's current one (the
// calls, B), both planned on the same resident contig -- rules in include/msim.h, shared arithmetic in compare.h.
//   hold     msim_cmp_hold: a device copy of the contig's active table and insert pool, kept beside the contig
//   match    k_cmp_match: one lane per A record and step -- its interval from a walk over the resident bases, its rank from a
//            scan of A to the left, a binary search of B for the interval's start, a scan of B for the record of that rank;
//            the lane stores its own flag byte and its partner's (no two lanes share a partner) and counts the record
//   tally    k_cmp_tally: one lane per B record, counted by its flag byte
// Both kernels are templates over the outcomes a record of a cell can have (compare.h: Score) and count into lane-private bins
// (lane_hist.h): 2, a haploid comparison -- 15 cells x matched / unmatched, two tallies: 32 bins; 3, a diploid one -- 15 cells x
// matched / genotype-mismatched / unmatched, two tallies, one spare: 48 bins.
// compare --diploid (msim_cmp_join, msim_cmp_counts_diploid): a side's two haplotype tables are JOINED into one diploid table with a
// genotype byte per record (k_join_flag, k_scan_u32, k_join_put2, k_join_put1), and the truth's diploid table is scored against
// the calls' by the same two kernels, a matched pair's flag byte saying whether the two dosages agree.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "cmp_blocks.h"
#include "cmp_phase.h"
#include "cmp_regions.h"
#include "compare.h"
#include "counter_trip.h"
#include "ctx.h"
#include "lane_hist.h"
#include "scan_kernels.h"

namespace msim {

struct Held {                                  // msim_cmp_hold's copy of one contig's table
    bool have = false;
    Scratch<msim_record> d_recs;
    Scratch<uint8_t> d_pool;
    uint64_t n_rec = 0, pool_len = 0;
    Scratch<uint8_t> d_flag_a, d_flag_b;                   // one byte per held / per current record (the last msim_cmp_counts)
    uint64_t n_flag_b = 0;
    bool counted = false;
    int counted_outcomes = 0;                              // of that count: 2 (msim_cmp_counts), 3 (msim_cmp_counts_blocks)
    uint32_t counted_flags = 0;                            // its flags
    uint64_t counted_gen = 0;                              // the contig's table generation it saw
};

struct Dip {                                   // msim_cmp_join's result: one side's diploid table of one contig
    bool have = false;
    Scratch<msim_record> d_recs;               // n records (allocated for n1 + n2)
    Scratch<uint8_t> d_pool;                   // haplotype 1's pool, then haplotype 2's
    Scratch<uint8_t> d_gt;                     // a genotype byte per record
    Scratch<uint8_t> d_flag;                   // a flag byte per record (the last msim_cmp_counts_diploid)
    uint64_t n = 0, pool_len = 0;
};
struct DipPair {
    Dip side[2];                               // MSIM_CMP_TRUTH, MSIM_CMP_CALLS
    bool counted = false;
    uint32_t counted_flags = 0;                // the flags of that msim_cmp_counts_diploid
};

struct CompareState {
    std::vector<Held> held;                    // by contig index
    std::vector<DipPair> dip;                  // by contig index (a sibling of `held`: msim_cmp_hold replaces a Held whole)
    CounterTrip out;                           // HIST_SLOTS x (A's counters, B's counters); its events time the join as well
    Scratch<uint32_t> d_front;                // the join's scratch, per haplotype-2 record: haplotype 1's records at or in front
                                               //   of its pos, bit 31: it is a duplicate of the last of them;
    Scratch<uint32_t> d_excl;                  //   the duplicates in front of it;
    Scratch<uint32_t> d_tile;                  //   per scan tile its duplicates (then their exclusive scan, the total last)
    double kernel_ms = 0, join_ms = 0;
    // compare --blocks (msim_cmp_counts_blocks; kernels in cmp_blocks.hip)
    CounterTrip blk_out;                       // the match's counters (two outcomes), the final tally's (three), the block pass's;
                                               //   its events time the match
    Scratch<blk::Desc> d_desc;                 // the blocks to replay
    EventPair tm_blk, tm_tally;
    hipEvent_t ev_blk_mid = nullptr;           // between k_blk_scan and k_blk_replay
    double blocks_ms = 0, scan_ms = 0, replay_ms = 0;
    uint64_t replay_steps = 0, replay_wave_steps = 0;      // msim_dbg_cmp_blocks_split
    PhaseState *phase = nullptr;               // compare --phased (cmp_phase.hip; made on first use)
    RegionState *regions = nullptr;            // compare --regions / --stratify (cmp_regions.hip; made on first use)
};

namespace {

constexpr int LANES = cmp::LANES;
constexpr uint32_t CMP_PASS = LANES;                       // records of a workgroup's pass: one a lane (a walk is long enough)
static_assert(CMP_PASS == MSIM_CMP_PASS, "msim.h and compare.hip must agree on the pass");
static_assert((1u << cmp::WINDOW_SHIFT) == MSIM_CMP_WINDOW, "msim.h and compare.h must agree on the window");
constexpr unsigned CMP_MAX_BLOCKS = 2048;                  // more passes than that stride: eight workgroups a CU (16 KB of LDS each)
static_assert(sizeof(msim_record) == sizeof(uint4), "a record is one 16-byte load");

// Lane-private bins and slots: compare.h (Hist, OUT_WORDS, slot_of) -- 16 KB of LDS a workgroup and eight workgroups a CU with
// two outcomes, 24 KB and six with three.  A table has fewer than 2^31 records, so fewer than 2^23 passes; beyond CMP_MAX_BLOCKS
// passes the grid strides, a workgroup takes at most 4096 of them and a lane adds at most once per counter and pass: 16 bits
// hold it, in either instantiation.
using cmp::OUT_WORDS;

// the two tables' genotype bytes, which a haploid comparison neither has nor passes to its kernel
template <int OUTCOMES> struct Gt { const uint8_t *a, *b; };
template <> struct Gt<2> { Gt(const uint8_t *, const uint8_t *) {} };

// flag_b was zeroed before the launch.  Every index below is checked against its table's size -- a genotype byte is read at
// such an index --; the bases are read inside [0, L) only, the pools inside their lengths (compare.h: walkable, same).
template <int OUTCOMES>
__global__ __launch_bounds__(LANES) void k_cmp_match(const uint8_t *__restrict__ g, uint64_t L, cmp::Table A, cmp::Table B, uint32_t exact,
                                                     uint64_t n_pass, uint8_t *__restrict__ flag_a, uint8_t *__restrict__ flag_b,
                                                     unsigned long long *__restrict__ out, Gt<OUTCOMES> gt) {
    using S = cmp::Score<OUTCOMES>;
    __shared__ cmp::Hist<OUTCOMES> hist;
    hist.zero();
    for (uint64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        const uint64_t i = pass * CMP_PASS + threadIdx.x;
        if (i >= A.n) continue;
        const cmp::Rec a = cmp::rec_at(A.recs, i);
        if (!cmp::known_type(a.type)) { flag_a[i] = 0; continue; }
        cmp::Span s;
        const int64_t j = cmp::partner(g, L, A, i, B, exact != 0, &s);
        uint8_t f = 0;
        if (j >= 0 && (uint64_t)j < B.n) {
            if constexpr (OUTCOMES == 3) f = cmp::pair_flag(gt.a[i], gt.b[j]);
            else f = 1;
            flag_b[j] = f;                                 // a plain byte store: this lane is the only one with this partner
        }
        flag_a[i] = f;
        hist.add(cmp::counter_of<OUTCOMES>(a, f), 1u);
        if (s.stops & cmp::STOP_WINDOW) hist.add(S::TALLIES, 1u);
        if (s.stops & cmp::STOP_BASE) hist.add(S::TALLIES + 1, 1u);
    }
    hist.flush(cmp::slot_of<OUTCOMES>(out));
}

template <int OUTCOMES>
__global__ __launch_bounds__(LANES) void k_cmp_tally(const msim_record *__restrict__ recs, uint64_t n_rec, uint64_t n_pass,
                                                     const uint8_t *__restrict__ flag, unsigned long long *__restrict__ out) {
    __shared__ cmp::Hist<OUTCOMES> hist;
    hist.zero();
    for (uint64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        const uint64_t i = pass * CMP_PASS + threadIdx.x;
        if (i >= n_rec) continue;
        const cmp::Rec b = cmp::rec_at(recs, i);
        if (cmp::known_type(b.type)) hist.add(cmp::counter_of<OUTCOMES>(b, flag[i]), 1u);
    }
    hist.flush(cmp::slot_of<OUTCOMES>(out));
}

// ---- the join: haplotype 1's table (H1) and haplotype 2's (H2) into one diploid table U ------------------------------------------
// One lane per record of either table.  A scan tile is JOIN_TILE records of H2; k_join_put2 takes them in runs of 64 (run s = round *
// JOIN_WAVES + wave), one ballot a run -- haplotype.hip's compaction pattern:
//   flag      k_join_flag: an H2 record binary-searches H1 for its pos, tests the record there with cmp::same and stores what it
//             found in one word -- H1's records at or in front of its pos (fewer than 2^31), bit 31: it is a duplicate -- so
//             that nobody searches H1 again; the tile's duplicates are counted
//   scan      k_scan_u32 over the tiles' counts (scan_kernels.h), the total behind them
//   put 2     k_join_put2: the duplicates in front of every H2 record (stored: H1's lanes need them), and every H2 record that is
//             no duplicate to  own index - duplicates in front + H1's records at or in front of its pos,  genotype 2, an
//             insertion's extra rebased by H1's pool length
//   put 1     k_join_put1: every H1 record to  own index + H2's records in front of its pos - the duplicates among those,
//             genotype 3 where H2's record at its pos is a duplicate, else 1
// Every index is checked against its table's size and every write against U's allocation (n1 + n2 records).
constexpr int JOIN_WAVES = LANES / 64;
constexpr int JOIN_ROUNDS = 4;
constexpr int JOIN_SLOTS = JOIN_WAVES * JOIN_ROUNDS;
constexpr uint32_t JOIN_TILE = 64u * JOIN_SLOTS;
static_assert(JOIN_TILE == MSIM_CMP_JOIN_TILE, "msim.h and compare.hip must agree on the join's scan tile");
constexpr uint32_t JOIN_DUP = 1u << 31;

// (one record a lane, the tile's 1024 lanes one workgroup: a lane's search is a chain of dependent loads, and four of them one
// behind the other in a lane of a 256-lane workgroup took three times as long, NOTES 27)
__global__ __launch_bounds__(JOIN_TILE) void k_join_flag(cmp::Table H1, cmp::Table H2, uint32_t *__restrict__ front, uint32_t *__restrict__ tile_cnt) {
    __shared__ uint32_t wcnt[JOIN_SLOTS];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t j = (uint64_t)blockIdx.x * JOIN_TILE + threadIdx.x;
    bool d = false;
    if (j < H2.n) {
        uint64_t in_front;
        d = cmp::join_dup(H1, H2, j, &in_front);
        front[j] = (uint32_t)in_front | (d ? JOIN_DUP : 0u);
    }
    const uint32_t cnt = (uint32_t)__popcll(__ballot(d));
    if (lane == 0) wcnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < JOIN_SLOTS; w++) t += wcnt[w];
        tile_cnt[blockIdx.x] = t;
    }
}

__device__ __forceinline__ void join_store(msim_record *__restrict__ U, uint8_t *__restrict__ gt, uint64_t cap, uint64_t at, uint4 v, uint8_t g) {
    if (at >= cap) return;
    reinterpret_cast<uint4 *>(U)[at] = v;
    gt[at] = g;
}

// tile_off: the exclusive scan of k_join_flag's counts
__global__ __launch_bounds__(LANES) void k_join_put2(cmp::Table H1, cmp::Table H2, const uint32_t *__restrict__ front,
                                                     const uint32_t *__restrict__ tile_off, uint32_t *__restrict__ excl,
                                                     msim_record *__restrict__ U, uint8_t *__restrict__ gt, uint64_t cap) {
    __shared__ uint32_t scnt[JOIN_SLOTS];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * JOIN_TILE;
    unsigned long long b[JOIN_ROUNDS];
    uint32_t found[JOIN_ROUNDS];
#pragma unroll
    for (int r = 0; r < JOIN_ROUNDS; r++) {
        const uint64_t j = base + (uint64_t)(r * JOIN_WAVES + (int)wave) * 64 + lane;
        found[r] = j < H2.n ? front[j] : 0u;
        b[r] = __ballot((found[r] & JOIN_DUP) != 0);
        if (lane == 0) scnt[r * JOIN_WAVES + (int)wave] = (uint32_t)__popcll(b[r]);
    }
    __syncthreads();
    const uint32_t off0 = tile_off[blockIdx.x];
    const unsigned long long below = (1ull << lane) - 1;
#pragma unroll
    for (int r = 0; r < JOIN_ROUNDS; r++) {
        const int slot = r * JOIN_WAVES + (int)wave;
        uint32_t pre = 0;
#pragma unroll
        for (int s = 0; s < JOIN_SLOTS; s++) pre += s < slot ? scnt[s] : 0u;
        const uint64_t j = base + (uint64_t)slot * 64 + lane;
        if (j >= H2.n) continue;
        const uint32_t before = off0 + pre + (uint32_t)__popcll(b[r] & below);
        excl[j] = before;
        if ((b[r] >> lane) & 1ull) continue;               // H1's copy is the one written
        uint4 v = reinterpret_cast<const uint4 *>(H2.recs)[j];
        const uint64_t in_front = found[r];                // H1's records at or in front of this pos: at equal pos H1's comes first
        if ((v.w & 0xffu) == (uint32_t)MSIM_IN) v.z += (uint32_t)H1.pool_len;   // (the two pool lengths sum to less than 2^32)
        join_store(U, gt, cap, j - before + in_front, v, 2);
    }
}

// total: the duplicates of all of H2 (the word behind the tiles' scan)
__global__ __launch_bounds__(LANES) void k_join_put1(cmp::Table H1, cmp::Table H2, const uint32_t *__restrict__ front,
                                                     const uint32_t *__restrict__ excl, const uint32_t *__restrict__ total,
                                                     msim_record *__restrict__ U, uint8_t *__restrict__ gt, uint64_t cap) {
    const uint64_t i = (uint64_t)blockIdx.x * LANES + threadIdx.x;
    if (i >= H1.n) return;
    const uint4 v = reinterpret_cast<const uint4 *>(H1.recs)[i];
    const uint64_t k = cmp::first_at(H2, v.x);             // H2's records in front of this pos
    const uint32_t before = k < H2.n ? excl[k] : *total;
    const bool both = k < H2.n && (front[k] & JOIN_DUP) != 0 && cmp::rec_at(H2.recs, k).pos == v.x;
    join_store(U, gt, cap, i + k - before, v, both ? 3 : 1);
}

// a[]: the truth's counters (per cell its outcomes -- matched / missed, or matched / genotype-mismatched / missed --, the two
// tallies), b[]: the calls' (the last outcome: extra)
template <int OUTCOMES>
void finish(const unsigned long long *a, const unsigned long long *b, uint64_t *counts, uint64_t tallies[2]) {
    cmp::fold_cells<OUTCOMES>(a, b, counts);
    tallies[0] += a[cmp::Score<OUTCOMES>::TALLIES];
    tallies[1] += a[cmp::Score<OUTCOMES>::TALLIES + 1];
}

int state_of(Ctx *c, CompareState **out) {
    const int rc = lazy_state(c, &c->compare, OUT_WORDS<3>, "the compare mode's result buffers and events");   // (the larger of the two layouts)
    *out = c->compare;
    return rc;
}

Held *held_of(Ctx *c, int contig) {
    CompareState *S = c->compare;
    if (!S || contig < 0 || (size_t)contig >= S->held.size() || !S->held[(size_t)contig].have) return nullptr;
    return &S->held[(size_t)contig];
}

// What a call on a contig's held table begins with: the planned contig on the device, the held table, the state -- refused in
// this order.  own_refusal: what the caller found wrong with an argument of its own, judged behind the contig.
int held_contig(Ctx *c, int contig, Contig **g, Held **h, CompareState **S, const char *own_refusal = nullptr) {
    const int rc = ctx_device_contig(c, contig, true, g);
    if (rc) return rc;
    if (own_refusal) return fail(c, MSIM_ERR_ARG, own_refusal);
    if (!(*h = held_of(c, contig))) return fail(c, MSIM_ERR_ARG, "contig has no held table (msim_cmp_hold)");
    return state_of(c, S);
}

// a contig's current table and a held one, as the kernels take them
cmp::Table table_of(const Contig &g) { return {g.d_recs.p(), g.n_rec, g.pool_len ? g.d_pool.p() + PAD : nullptr, g.pool_len}; }
cmp::Table table_of(const Held &h) { return {h.d_recs.p(), h.n_rec, h.d_pool.p(), h.pool_len}; }

// one side of a comparison: its table, its genotype bytes (a haploid side: none), its flag bytes (one per record)
struct Side { cmp::Table t; const uint8_t *gt; uint8_t *flag; };

// What a count of the held table against the contig's current one begins with: a flag byte per current record, the two sides.
int held_sides(Ctx *c, const Contig &g, Held &h, Side *a, Side *b) {
    h.counted = false;
    MSIM_HIP(c, dev_at_least(h.d_flag_b, (size_t)g.n_rec));      // exactly a byte per record
    h.n_flag_b = g.n_rec;
    *a = Side{table_of(h), nullptr, h.d_flag_a.p()};
    *b = Side{table_of(g), nullptr, h.d_flag_b.p()};
    return MSIM_OK;
}

// b's flags zeroed and a's records matched against b: every record of a its flag byte and counter, its partner in b the flag
template <int OUTCOMES>
int launch_match(Ctx *c, const Contig &g, const Side &a, const Side &b, uint32_t flags, unsigned long long *out) {
    if (b.t.n) MSIM_HIP(c, hipMemsetAsync(b.flag, 0, (size_t)b.t.n, c->stream));
    if (!a.t.n) return MSIM_OK;
    const PassGrid pg = pass_grid(a.t.n, CMP_PASS, CMP_MAX_BLOCKS);
    hipLaunchKernelGGL(k_cmp_match<OUTCOMES>, pg.grid, dim3(LANES), 0, c->stream, g.d_in.p() + PAD, g.len, a.t, b.t, flags & MSIM_CMP_EXACT,
                       pg.n_pass, a.flag, b.flag, out, Gt<OUTCOMES>{a.gt, b.gt});
    MSIM_HIP(c, hipGetLastError());
    return MSIM_OK;
}
// a side's records counted by their flag bytes
template <int OUTCOMES>
int launch_tally(Ctx *c, const Side &x, unsigned long long *out) {
    if (!x.t.n) return MSIM_OK;
    const PassGrid pg = pass_grid(x.t.n, CMP_PASS, CMP_MAX_BLOCKS);
    hipLaunchKernelGGL(k_cmp_tally<OUTCOMES>, pg.grid, dim3(LANES), 0, c->stream, x.t.recs, x.t.n, pg.n_pass, (const uint8_t *)x.flag, out);
    MSIM_HIP(c, hipGetLastError());
    return MSIM_OK;
}

// The two launches of a comparison on contig g, A against B: b's flags zeroed, a's records matched, b's tallied, the counters
// fetched and summed into counts and tallies.
template <int OUTCOMES>
int counts_device(Ctx *c, CompareState *S, const Contig &g, const Side &a, const Side &b, uint32_t flags, uint64_t *counts, uint64_t tallies[2]) {
    constexpr size_t BINS = cmp::Score<OUTCOMES>::BINS;
    if (!a.t.n && !b.t.n) return MSIM_OK;
    int rc;
    if ((rc = S->out.begin(c, OUT_WORDS<OUTCOMES>)) || (rc = launch_match<OUTCOMES>(c, g, a, b, flags, S->out.d.p())) ||
        (rc = launch_tally<OUTCOMES>(c, b, S->out.d.p() + BINS)) || (rc = S->out.finish(c, &S->kernel_ms)))
        return rc;
    unsigned long long bins[2 * BINS];
    hist_sum_slots(S->out.h.p(), 2 * BINS, bins, 2 * BINS);
    finish<OUTCOMES>(bins, bins + BINS, counts, tallies);
    return MSIM_OK;
}

// the held table against the contig's current one
int counts_held(Ctx *c, CompareState *S, const Contig &g, Held &h, uint32_t flags, uint64_t *counts, uint64_t tallies[2]) {
    Side a, b;
    int rc = held_sides(c, g, h, &a, &b);
    if (rc) return rc;
    rc = counts_device<2>(c, S, g, a, b, flags, counts, tallies);
    h.counted = !rc;
    h.counted_outcomes = 2;
    h.counted_flags = flags;
    h.counted_gen = g.table_gen;
    return rc;
}

// ---- compare --blocks: the held table against the current one, unmatched records rescued block by block ---------------------------
// The words of blk_out: k_cmp_match<2>'s counters (its two walk tallies are used, its cells are not), k_cmp_tally<3>'s over both
// tables with the final flag bytes, the block pass's (cmp_blocks.h).
constexpr size_t BLK_MATCH_AT = 0, BLK_TALLY_AT = OUT_WORDS<2>, BLK_PASS_AT = BLK_TALLY_AT + OUT_WORDS<3>,
                 BLK_OUT_WORDS = BLK_PASS_AT + blk::PASS_WORDS;

void finish_blocks(const unsigned long long *words, uint64_t *counts, uint64_t tallies[2], uint64_t block_tallies[5]) {
    constexpr size_t B2 = cmp::Score<2>::BINS, B3 = cmp::Score<3>::BINS;
    unsigned long long m[2 * B2], t[2 * B3], p[blk::PASS_BINS];
    hist_sum_slots(words + BLK_MATCH_AT, 2 * B2, m, 2 * B2);
    hist_sum_slots(words + BLK_TALLY_AT, 2 * B3, t, 2 * B3);
    hist_sum_slots(words + BLK_PASS_AT, blk::PASS_BINS, p, blk::PASS_BINS);
    cmp::fold_cells<3>(t, t + B3, counts);
    tallies[0] += m[cmp::Score<2>::TALLIES];
    tallies[1] += m[cmp::Score<2>::TALLIES + 1];
    for (uint32_t k = 0; k < blk::TALLIES; k++) block_tallies[k] += p[k];
}

// Three timed stretches on one trip: the match (the trip's own events), the block pass with an event between its two kernels, the
// final tallies.
int counts_held_blocks(Ctx *c, CompareState *S, const Contig &g, Held &h, uint32_t flags, uint32_t gap, uint64_t *counts, uint64_t tallies[2],
                       uint64_t block_tallies[5]) {
    CounterTrip &trip = S->blk_out;
    if (!trip) MSIM_HIP(c, trip.create(BLK_OUT_WORDS));     // (made on first use)
    if (!S->tm_blk.e1) { S->tm_blk.destroy(); MSIM_HIP(c, S->tm_blk.create()); }
    if (!S->tm_tally.e1) { S->tm_tally.destroy(); MSIM_HIP(c, S->tm_tally.create()); }
    if (!S->ev_blk_mid) MSIM_HIP(c, hipEventCreate(&S->ev_blk_mid));
    Side a, b;
    int rc = held_sides(c, g, h, &a, &b);
    if (rc) return rc;
    h.counted_outcomes = 3;
    h.counted_flags = flags;
    h.counted_gen = g.table_gen;
    const uint64_t total = a.t.n + b.t.n;
    if (!total) { h.counted = true; return MSIM_OK; }
    MSIM_HIP(c, dev_at_least(S->d_desc, (size_t)total * sizeof(blk::Desc)));
    unsigned long long *out = trip.d.p();
    if ((rc = trip.begin(c, BLK_OUT_WORDS)) || (rc = launch_match<2>(c, g, a, b, flags, out + BLK_MATCH_AT))) return rc;
    MSIM_HIP(c, trip.tm.end(c->stream));
    MSIM_HIP(c, S->tm_blk.begin(c->stream));
    if ((rc = blocks_enqueue(c, c->stream, g.d_in.p() + PAD, g.len, a.t, b.t, a.flag, b.flag, gap, S->d_desc.p(), total, out + BLK_PASS_AT, S->ev_blk_mid)))
        return rc;
    MSIM_HIP(c, S->tm_blk.end(c->stream));
    MSIM_HIP(c, S->tm_tally.begin(c->stream));
    if ((rc = launch_tally<3>(c, a, out + BLK_TALLY_AT)) || (rc = launch_tally<3>(c, b, out + BLK_TALLY_AT + cmp::Score<3>::BINS))) return rc;
    MSIM_HIP(c, S->tm_tally.end(c->stream));                // (in front of the copy: the kernels alone)
    if ((rc = trip.copy_wait(c)) || (rc = trip.tm.add_elapsed(c, &S->kernel_ms)) || (rc = S->tm_tally.add_elapsed(c, &S->kernel_ms)) ||
        (rc = S->tm_blk.add_elapsed(c, &S->blocks_ms)))
        return rc;
    const unsigned long long *pass = trip.h.p() + BLK_PASS_AT;
    if (pass[blk::PASS_COUNT_AT] > total) return fail(c, MSIM_ERR_HIP, "internal: more blocks to replay than the two tables hold records");
    float scan = 0, replay = 0;
    MSIM_HIP(c, hipEventElapsedTime(&scan, S->tm_blk.e0, S->ev_blk_mid));
    MSIM_HIP(c, hipEventElapsedTime(&replay, S->ev_blk_mid, S->tm_blk.e1));
    S->scan_ms += scan;
    S->replay_ms += replay;
    S->replay_steps += pass[blk::PASS_STEPS_AT];
    S->replay_wave_steps += pass[blk::PASS_WAVE_STEPS_AT];
    finish_blocks(trip.h.p(), counts, tallies, block_tallies);
    h.counted = true;
    return MSIM_OK;
}

// the truth's diploid table against the calls'
int counts_joined(Ctx *c, CompareState *S, const Contig &g, DipPair &p, uint32_t flags, uint64_t *counts, uint64_t tallies[2]) {
    const auto side = [](Dip &d) { return Side{{d.d_recs.p(), d.n, d.d_pool.p(), d.pool_len}, d.d_gt.p(), d.d_flag.p()}; };
    p.counted = false;
    const int rc = counts_device<3>(c, S, g, side(p.side[MSIM_CMP_TRUTH]), side(p.side[MSIM_CMP_CALLS]), flags, counts, tallies);
    p.counted = !rc;
    p.counted_flags = flags;
    return rc;
}

DipPair *dip_of(Ctx *c, int contig) {
    CompareState *S = c->compare;
    if (!S || contig < 0 || (size_t)contig >= S->dip.size()) return nullptr;
    DipPair &p = S->dip[(size_t)contig];
    return p.side[0].have && p.side[1].have ? &p : nullptr;
}

// H1 = the held table h, H2 = the contig's active table: the launches of the join into d (sizes checked by the caller)
int join_device(Ctx *c, CompareState *S, const Contig &g, const Held &h, Dip &d) {
    const uint64_t n1 = h.n_rec, n2 = g.n_rec, cap = n1 + n2;
    d.pool_len = h.pool_len + g.pool_len;
    d.n = 0;
    MSIM_HIP(c, dev_exact(d.d_recs, (size_t)cap * sizeof(msim_record)));
    MSIM_HIP(c, dev_exact(d.d_gt, (size_t)cap));
    MSIM_HIP(c, dev_exact(d.d_flag, (size_t)cap));
    MSIM_HIP(c, dev_exact(d.d_pool, (size_t)d.pool_len));
    if (!cap) return MSIM_OK;                              // two empty tables (and so two empty pools): nothing launched
    const uint32_t tiles = (uint32_t)((n2 + JOIN_TILE - 1) / JOIN_TILE);
    MSIM_HIP(c, dev_at_least(S->d_front, (size_t)std::max<uint64_t>(n2, 1) * sizeof(uint32_t)));
    MSIM_HIP(c, dev_at_least(S->d_excl, (size_t)std::max<uint64_t>(n2, 1) * sizeof(uint32_t)));
    MSIM_HIP(c, dev_at_least(S->d_tile, ((size_t)tiles + 1) * sizeof(uint32_t)));
    const cmp::Table H1 = table_of(h), H2 = table_of(g);
    uint32_t dups = 0;
    MSIM_HIP(c, S->out.tm.begin(c->stream));
    if (n2) {
        hipLaunchKernelGGL(k_join_flag, dim3(tiles), dim3(JOIN_TILE), 0, c->stream, H1, H2, S->d_front.p(), S->d_tile.p());
        hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, c->stream, S->d_tile.p(), tiles);
        hipLaunchKernelGGL(k_join_put2, dim3(tiles), dim3(LANES), 0, c->stream, H1, H2, (const uint32_t *)S->d_front.p(),
                           (const uint32_t *)S->d_tile.p(), S->d_excl.p(), d.d_recs.p(), d.d_gt.p(), cap);
        MSIM_HIP(c, hipGetLastError());
    } else {
        MSIM_HIP(c, hipMemsetAsync(S->d_tile.p(), 0, sizeof(uint32_t), c->stream));   // the total: no duplicates
    }
    if (n1) {
        hipLaunchKernelGGL(k_join_put1, dim3((unsigned)((n1 + LANES - 1) / LANES)), dim3(LANES), 0, c->stream, H1, H2,
                           (const uint32_t *)S->d_front.p(), (const uint32_t *)S->d_excl.p(), (const uint32_t *)S->d_tile.p() + tiles,
                           d.d_recs.p(), d.d_gt.p(), cap);
        MSIM_HIP(c, hipGetLastError());
    }
    if (h.pool_len) MSIM_HIP(c, hipMemcpyAsync(d.d_pool.p(), h.d_pool.p(), (size_t)h.pool_len, hipMemcpyDeviceToDevice, c->stream));
    if (g.pool_len)
        MSIM_HIP(c, hipMemcpyAsync(d.d_pool.p() + h.pool_len, g.d_pool.p() + PAD, (size_t)g.pool_len, hipMemcpyDeviceToDevice, c->stream));
    MSIM_HIP(c, S->out.tm.end(c->stream));                  // (the kernels and the two pool copies)
    MSIM_HIP(c, hipMemcpyAsync(&dups, S->d_tile.p() + tiles, sizeof dups, hipMemcpyDeviceToHost, c->stream));
    MSIM_HIP(c, wait_stream(c->stream));
    const int rc = S->out.tm.add_elapsed(c, &S->join_ms);
    if (rc) return rc;
    if (dups > n1 || dups > n2) return fail(c, MSIM_ERR_HIP, "internal: the join counted more duplicates than a table holds");
    d.n = cap - dups;
    return MSIM_OK;
}

// (host restatements) a table the rules are written for: known types, pos non-decreasing (strict: strictly increasing)
int dbg_table_ok(const char *name, const msim_record *t, uint64_t n, bool strict) {
    for (uint64_t i = 0; i < n; i++) {
        if (!cmp::known_type(t[i].type)) return fail(nullptr, MSIM_ERR_ARG, std::string(name) + " record " + std::to_string(i) + ": unknown type");
        if (i && (strict ? t[i].pos <= t[i - 1].pos : t[i].pos < t[i - 1].pos))
            return fail(nullptr, MSIM_ERR_ARG, std::string(name) + " record " + std::to_string(i) + ": the table is not sorted by pos");
    }
    return MSIM_OK;
}
int dbg_gt_ok(const char *name, const uint8_t *gt, uint64_t n) {
    for (uint64_t i = 0; i < n; i++)
        if (gt[i] < 1 || gt[i] > 3) return fail(nullptr, MSIM_ERR_ARG, std::string(name) + " record " + std::to_string(i) + ": genotype byte outside 1..3");
    return MSIM_OK;
}
// The comparison as one sequential loop over two host tables the caller has judged (a side's flag bytes: wanted or NULL).
template <int OUTCOMES>
void dbg_counts(const uint8_t *bases, uint64_t L, const Side &a, const Side &b, uint32_t flags, uint64_t *counts, uint64_t tallies[2]) {
    using S = cmp::Score<OUTCOMES>;
    memset(counts, 0, (size_t)8 * MSIM_CMP_BINS * 2 * OUTCOMES * sizeof(uint64_t));
    memset(tallies, 0, 2 * sizeof(uint64_t));
    std::vector<uint8_t> fb((size_t)b.t.n, 0);
    unsigned long long ca[S::COUNTERS] = {}, cb[S::COUNTERS] = {};
    for (uint64_t i = 0; i < a.t.n; i++) {
        cmp::Span s;
        const int64_t j = cmp::partner(bases, L, a.t, i, b.t, (flags & MSIM_CMP_EXACT) != 0, &s);
        uint8_t f = 0;
        if (j >= 0 && (uint64_t)j < b.t.n) {
            if constexpr (OUTCOMES == 3) f = cmp::pair_flag(a.gt[i], b.gt[(size_t)j]);
            else f = 1;
            fb[(size_t)j] = f;
        }
        if (a.flag) a.flag[i] = f;
        ca[cmp::counter_of<OUTCOMES>(cmp::rec_at(a.t.recs, i), f)]++;
        if (s.stops & cmp::STOP_WINDOW) ca[S::TALLIES]++;
        if (s.stops & cmp::STOP_BASE) ca[S::TALLIES + 1]++;
    }
    for (uint64_t i = 0; i < b.t.n; i++) {
        cb[cmp::counter_of<OUTCOMES>(cmp::rec_at(b.t.recs, i), fb[(size_t)i])]++;
        if (b.flag) b.flag[i] = fb[(size_t)i];
    }
    finish<OUTCOMES>(ca, cb, counts, tallies);
}

// the join's two refusals
int join_sizes_ok(Ctx *c, uint64_t n1, uint64_t n2, uint64_t pool1, uint64_t pool2) {
    if (n1 >= (1ull << 31) || n2 >= (1ull << 31) || n1 + n2 >= (1ull << 31))
        return fail(c, MSIM_ERR_UNSUPPORTED, "the two haplotype tables hold 2^31 records or more");
    if (pool1 >= (1ull << 32) || pool2 >= (1ull << 32) || pool1 + pool2 >= (1ull << 32))
        return fail(c, MSIM_ERR_UNSUPPORTED, "the two insert pools hold 4 GiB or more");
    return MSIM_OK;
}

}  // namespace

void compare_drop_all(Ctx *c) {
    if (!c->compare) return;
    c->compare->held.clear();
    c->compare->dip.clear();
    phase_drop(c->compare->phase, -1);
    regions_drop(c->compare->regions, -1);
}

bool compare_dip_view(Ctx *c, int contig, int side, DipView *v, bool *counted, uint32_t *counted_flags) {
    CompareState *S = c->compare;
    *v = DipView{};
    *counted = false;
    *counted_flags = 0;
    if (!S || contig < 0 || (size_t)contig >= S->dip.size() || (side != MSIM_CMP_TRUTH && side != MSIM_CMP_CALLS)) return false;
    const DipPair &p = S->dip[(size_t)contig];
    const Dip &d = p.side[side];
    if (!d.have) return false;
    *v = DipView{true, {d.d_recs.p(), d.n, d.d_pool.p(), d.pool_len}, d.d_gt.p(), d.d_flag.p()};
    *counted = p.counted && p.side[0].have && p.side[1].have;
    *counted_flags = p.counted_flags;
    return true;
}

bool compare_region_tables(Ctx *c, int contig, bool diploid, RegionTables *v, const char **why) {
    *v = RegionTables{};
    if (diploid) {
        DipPair *p = dip_of(c, contig);
        if (!p) { *why = "contig has no diploid table of both sides (msim_cmp_join)"; return false; }
        for (int s = 0; s < 2; s++) {
            const Dip &d = p->side[s];
            v->t[s] = cmp::Table{d.d_recs.p(), d.n, d.d_pool.p(), d.pool_len};
            v->flag[s] = d.d_flag.p();
        }
        v->counted = p->counted;
        v->outcomes = 3;
        v->counted_flags = p->counted_flags;
        return true;
    }
    Held *h = held_of(c, contig);
    if (!h) { *why = "contig has no held table (msim_cmp_hold)"; return false; }
    const Contig &g = c->contigs[(size_t)contig];
    if (!g.planned) { *why = "contig has no current table: plan it first"; return false; }
    v->t[MSIM_CMP_TRUTH] = table_of(*h);
    v->t[MSIM_CMP_CALLS] = table_of(g);
    v->flag[MSIM_CMP_TRUTH] = h->d_flag_a.p();
    v->flag[MSIM_CMP_CALLS] = h->d_flag_b.p();
    v->counted = h->counted && g.n_rec == h->n_flag_b && g.table_gen == h->counted_gen;   // (msim_cmp_fetch's test, and the generation)
    v->outcomes = h->counted_outcomes;
    v->counted_flags = h->counted_flags;
    v->table_gen = g.table_gen;
    return true;
}

int compare_region_slot(Ctx *c, RegionState ***slot) {
    CompareState *S;
    const int rc = state_of(c, &S);
    if (rc) return rc;
    *slot = &S->regions;
    return MSIM_OK;
}

int compare_phase_slot(Ctx *c, PhaseState ***slot) {
    CompareState *S;
    const int rc = state_of(c, &S);
    if (rc) return rc;
    *slot = &S->phase;
    return MSIM_OK;
}

void compare_state_destroy(Ctx *c) {
    CompareState *S = c->compare;
    if (!S) return;
    compare_drop_all(c);
    phase_state_destroy(S->phase);
    S->phase = nullptr;
    regions_state_destroy(S->regions);
    S->regions = nullptr;
    S->tm_blk.destroy();
    S->tm_tally.destroy();
    if (S->ev_blk_mid) (void)hipEventDestroy(S->ev_blk_mid);
    delete S;
    c->compare = nullptr;
}

void compare_reset_timing(Ctx *c) {
    if (!c->compare) return;
    CompareState &S = *c->compare;
    S.kernel_ms = S.join_ms = S.blocks_ms = S.scan_ms = S.replay_ms = 0;
    S.replay_steps = S.replay_wave_steps = 0;
    phase_reset_timing(S.phase);
    regions_reset_timing(S.regions);
}

}  // namespace msim

using namespace msim;

extern "C" {

// A device copy of the contig's ACTIVE table (with a haplotype selected: that haplotype's) and insert pool; a table held before
// is replaced.  The copy is the context's: a new plan of the contig and msim_release_result leave it alone.
int msim_cmp_hold(msim_ctx *p, int contig) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    Contig *g;
    int rc = ctx_device_contig(c, contig, true, &g);
    if (rc) return rc;
    CompareState *S;
    if ((rc = state_of(c, &S))) return rc;
    if (S->held.size() <= (size_t)contig) S->held.resize((size_t)contig + 1);
    Held &h = S->held[(size_t)contig] = Held{};
    regions_unmark(S->regions, contig);
    if (g->n_rec) {
        MSIM_HIP(c, dev_alloc(h.d_recs, (size_t)g->n_rec * sizeof(msim_record)));
        MSIM_HIP(c, dev_alloc(h.d_flag_a, (size_t)g->n_rec));
        MSIM_HIP(c, hipMemcpyAsync(h.d_recs.p(), g->d_recs.p(), (size_t)g->n_rec * sizeof(msim_record), hipMemcpyDeviceToDevice, c->stream));
    }
    if (g->pool_len) {
        MSIM_HIP(c, dev_alloc(h.d_pool, (size_t)g->pool_len));
        MSIM_HIP(c, hipMemcpyAsync(h.d_pool.p(), g->d_pool.p() + PAD, (size_t)g->pool_len, hipMemcpyDeviceToDevice, c->stream));
    }
    MSIM_HIP(c, wait_stream(c->stream));
    h.n_rec = g->n_rec;
    h.pool_len = g->pool_len;
    h.have = true;
    return MSIM_OK;
}

int msim_cmp_release(msim_ctx *p, int contig) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    if (c->host_only || !c->compare) return MSIM_OK;
    MSIM_HIP(c, wait_stream(c->stream));
    if (contig < 0) { compare_drop_all(c); return MSIM_OK; }
    if (Held *h = held_of(c, contig)) *h = Held{};
    if (contig >= 0 && (size_t)contig < c->compare->dip.size()) c->compare->dip[(size_t)contig] = DipPair{};
    phase_drop(c->compare->phase, contig);
    regions_drop(c->compare->regions, contig);
    return MSIM_OK;
}

int msim_cmp_counts(msim_ctx *p, int contig, uint32_t flags, uint64_t *counts, uint64_t tallies[2]) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !counts || !tallies) return MSIM_ERR_ARG;
    if (flags & ~(uint32_t)MSIM_CMP_EXACT) return fail(c, MSIM_ERR_ARG, "unknown compare flag");
    Contig *g;
    Held *h;
    CompareState *S;
    const int rc = held_contig(c, contig, &g, &h, &S);
    if (rc) return rc;
    memset(counts, 0, (size_t)8 * MSIM_CMP_BINS * 4 * sizeof(uint64_t));
    memset(tallies, 0, 2 * sizeof(uint64_t));
    TraceRange tr("msim compare");
    return counts_held(c, S, *g, *h, flags, counts, tallies);
}

int msim_cmp_counts_blocks(msim_ctx *p, int contig, uint32_t flags, uint32_t gap, uint64_t *counts, uint64_t tallies[2], uint64_t block_tallies[5]) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !counts || !tallies || !block_tallies) return MSIM_ERR_ARG;
    if (flags & ~(uint32_t)MSIM_CMP_EXACT) return fail(c, MSIM_ERR_ARG, "unknown compare flag");
    Contig *g;
    Held *h;
    CompareState *S;
    const int rc = held_contig(c, contig, &g, &h, &S, gap > MSIM_CMP_BLOCK_SPAN ? "the block gap is larger than MSIM_CMP_BLOCK_SPAN" : nullptr);
    if (rc) return rc;
    memset(counts, 0, (size_t)8 * MSIM_CMP_BINS * 6 * sizeof(uint64_t));
    memset(tallies, 0, 2 * sizeof(uint64_t));
    memset(block_tallies, 0, 5 * sizeof(uint64_t));
    TraceRange tr("msim compare blocks");
    return counts_held_blocks(c, S, *g, *h, flags, gap, counts, tallies, block_tallies);
}

int msim_cmp_blocks_timing(msim_ctx *p, double *kernel_ms) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    if (kernel_ms) *kernel_ms = c->compare ? c->compare->blocks_ms : 0.0;
    return MSIM_OK;
}

// measurement support (tools/compare_bench.py --blocks; exported, not part of msim.h): msim_cmp_blocks_timing by kernel -- ms[0]
// k_blk_scan, ms[1] k_blk_replay -- and the replay's lane-steps since msim_reset_stats: steps[0] the bytes its lanes compared,
// steps[1] 64 x the longest lane of every wave, summed (what the waves occupied)
int msim_dbg_cmp_blocks_split(msim_ctx *p, double ms[2], uint64_t steps[2]) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !ms || !steps) return MSIM_ERR_ARG;
    const CompareState *S = c->compare;
    ms[0] = S ? S->scan_ms : 0.0;
    ms[1] = S ? S->replay_ms : 0.0;
    steps[0] = S ? S->replay_steps : 0;
    steps[1] = S ? S->replay_wave_steps : 0;
    return MSIM_OK;
}

int msim_cmp_fetch(msim_ctx *p, int contig, uint64_t *n_held, uint64_t *held_pool_len, msim_record *held, uint8_t *held_pool,
                   uint8_t *held_flags, uint8_t *current_flags) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    if (c->host_only) return fail(c, MSIM_ERR_HIP, "host-only context: this call needs the GPU");
    Held *h = held_of(c, contig);
    if (!h) return fail(c, MSIM_ERR_ARG, "contig has no held table (msim_cmp_hold)");
    if (n_held) *n_held = h->n_rec;
    if (held_pool_len) *held_pool_len = h->pool_len;
    if (held_flags || current_flags) {
        const Contig &g = c->contigs[(size_t)contig];
        if (!h->counted || !g.planned || g.n_rec != h->n_flag_b)
            return fail(c, MSIM_ERR_ARG, "the flags are those of the contig's last msim_cmp_counts: call it first");
    }
    if (held && h->n_rec) MSIM_HIP(c, hipMemcpyAsync(held, h->d_recs.p(), (size_t)h->n_rec * sizeof(msim_record), hipMemcpyDeviceToHost, c->stream));
    if (held_pool && h->pool_len) MSIM_HIP(c, hipMemcpyAsync(held_pool, h->d_pool.p(), (size_t)h->pool_len, hipMemcpyDeviceToHost, c->stream));
    if (held_flags && h->n_rec) MSIM_HIP(c, hipMemcpyAsync(held_flags, h->d_flag_a.p(), (size_t)h->n_rec, hipMemcpyDeviceToHost, c->stream));
    if (current_flags && h->n_flag_b) MSIM_HIP(c, hipMemcpyAsync(current_flags, h->d_flag_b.p(), (size_t)h->n_flag_b, hipMemcpyDeviceToHost, c->stream));
    MSIM_HIP(c, wait_stream(c->stream));
    return MSIM_OK;
}

int msim_cmp_timing(msim_ctx *p, double *kernel_ms) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    if (kernel_ms) *kernel_ms = c->compare ? c->compare->kernel_ms : 0.0;
    return MSIM_OK;
}

// ---- compare --diploid ----------------------------------------------------------------------------------------------------------
// The contig's held table (haplotype 1) and its active table (haplotype 2) become its diploid table of `side`; the held table
// is consumed, the active one untouched.
int msim_cmp_join(msim_ctx *p, int contig, int side) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    Contig *g;
    Held *h;
    CompareState *S;
    int rc = held_contig(c, contig, &g, &h, &S,
                         side != MSIM_CMP_TRUTH && side != MSIM_CMP_CALLS ? "unknown side (MSIM_CMP_TRUTH, MSIM_CMP_CALLS)" : nullptr);
    if (rc || (rc = join_sizes_ok(c, h->n_rec, g->n_rec, h->pool_len, g->pool_len))) return rc;
    if (S->dip.size() <= (size_t)contig) S->dip.resize((size_t)contig + 1);
    DipPair &pair = S->dip[(size_t)contig];
    pair.counted = false;
    Dip &d = pair.side[side] = Dip{};
    phase_drop_side(S->phase, contig, side);
    regions_unmark(S->regions, contig);
    TraceRange tr("msim compare join");
    rc = join_device(c, S, *g, *h, d);
    if (rc) { d = Dip{}; return rc; }
    d.have = true;
    *h = Held{};
    return MSIM_OK;
}

int msim_cmp_counts_diploid(msim_ctx *p, int contig, uint32_t flags, uint64_t *counts, uint64_t tallies[2]) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !counts || !tallies) return MSIM_ERR_ARG;
    if (flags & ~(uint32_t)MSIM_CMP_EXACT) return fail(c, MSIM_ERR_ARG, "unknown compare flag");
    Contig *g;
    int rc = ctx_device_contig(c, contig, false, &g);
    if (rc) return rc;
    DipPair *pair = dip_of(c, contig);
    if (!pair) return fail(c, MSIM_ERR_ARG, "contig has no diploid table of both sides (msim_cmp_join)");
    CompareState *S;
    if ((rc = state_of(c, &S))) return rc;
    memset(counts, 0, (size_t)8 * MSIM_CMP_BINS * 6 * sizeof(uint64_t));
    memset(tallies, 0, 2 * sizeof(uint64_t));
    TraceRange tr("msim compare diploid");
    return counts_joined(c, S, *g, *pair, flags, counts, tallies);
}

int msim_cmp_fetch_diploid(msim_ctx *p, int contig, int side, uint64_t *n, uint64_t *pool_len, msim_record *recs, uint8_t *pool,
                           uint8_t *gt, uint8_t *flags) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    if (c->host_only) return fail(c, MSIM_ERR_HIP, "host-only context: this call needs the GPU");
    if (side != MSIM_CMP_TRUTH && side != MSIM_CMP_CALLS) return fail(c, MSIM_ERR_ARG, "unknown side (MSIM_CMP_TRUTH, MSIM_CMP_CALLS)");
    DipPair *pair = dip_of(c, contig);
    if (!pair) return fail(c, MSIM_ERR_ARG, "contig has no diploid table of both sides (msim_cmp_join)");
    const Dip &d = pair->side[side];
    if (n) *n = d.n;
    if (pool_len) *pool_len = d.pool_len;
    if (flags && !pair->counted) return fail(c, MSIM_ERR_ARG, "the flags are those of the contig's last msim_cmp_counts_diploid: call it first");
    if (recs && d.n) MSIM_HIP(c, hipMemcpyAsync(recs, d.d_recs.p(), (size_t)d.n * sizeof(msim_record), hipMemcpyDeviceToHost, c->stream));
    if (pool && d.pool_len) MSIM_HIP(c, hipMemcpyAsync(pool, d.d_pool.p(), (size_t)d.pool_len, hipMemcpyDeviceToHost, c->stream));
    if (gt && d.n) MSIM_HIP(c, hipMemcpyAsync(gt, d.d_gt.p(), (size_t)d.n, hipMemcpyDeviceToHost, c->stream));
    if (flags && d.n) MSIM_HIP(c, hipMemcpyAsync(flags, d.d_flag.p(), (size_t)d.n, hipMemcpyDeviceToHost, c->stream));
    MSIM_HIP(c, wait_stream(c->stream));
    return MSIM_OK;
}

int msim_cmp_join_timing(msim_ctx *p, double *kernel_ms) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    if (kernel_ms) *kernel_ms = c->compare ? c->compare->join_ms : 0.0;
    return MSIM_OK;
}

// measurement support (tools/compare_bench.py --diploid; exported, not part of msim.h): a device-to-device copy of the bytes the
// join of the contig's held and current table reads and writes once -- both tables' records and pools read, as many bytes
// written (an upper bound: a merged pair is written once) -- timed by HIP events: the join's streaming floor
int msim_dbg_cmp_join_copy_floor(msim_ctx *p, int contig, double *ms) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !ms) return MSIM_ERR_ARG;
    Contig *g;
    Held *h;
    CompareState *S;
    const int rc = held_contig(c, contig, &g, &h, &S);
    if (rc) return rc;
    const cmp::Table H = table_of(*h), G = table_of(*g);
    const CopySource one[4] = {{H.recs, (size_t)H.n * sizeof(msim_record)}, {G.recs, (size_t)G.n * sizeof(msim_record)},
                               {H.pool, (size_t)H.pool_len}, {G.pool, (size_t)G.pool_len}};
    return copy_floor(c, S->out.tm, one, 4, ms);
}

// measurement support (tools/compare_bench.py; exported, not part of msim.h): a device-to-device copy of the held and the current
// table's record bytes into the context's scratch, timed by HIP events -- the streaming floor the compare kernels are held against
int msim_dbg_cmp_copy_floor(msim_ctx *p, int contig, double *ms) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !ms) return MSIM_ERR_ARG;
    Contig *g;
    Held *h;
    CompareState *S;
    const int rc = held_contig(c, contig, &g, &h, &S);
    if (rc) return rc;
    const cmp::Table H = table_of(*h), G = table_of(*g);
    const CopySource tables[2] = {{H.recs, (size_t)H.n * sizeof(msim_record)}, {G.recs, (size_t)G.n * sizeof(msim_record)}};
    return copy_floor(c, S->out.tm, tables, 2, ms);
}

// ---- sequential host restatement: no context, no GPU -------------------------------------------------------------------
int msim_dbg_cmp_counts(const uint8_t *bases, uint64_t L, const msim_record *truth, uint64_t n_truth, const uint8_t *truth_pool,
                        uint64_t truth_pool_len, const msim_record *calls, uint64_t n_calls, const uint8_t *calls_pool,
                        uint64_t calls_pool_len, uint32_t flags, uint64_t *counts, uint64_t tallies[2], uint8_t *truth_flags,
                        uint8_t *calls_flags) {
    if ((!bases && L) || (!truth && n_truth) || (!calls && n_calls) || (!truth_pool && truth_pool_len) ||
        (!calls_pool && calls_pool_len) || !counts || !tallies || (flags & ~(uint32_t)MSIM_CMP_EXACT))
        return MSIM_ERR_ARG;
    for (uint64_t i = 0; i < n_truth; i++)
        if (!cmp::known_type(truth[i].type)) return fail(nullptr, MSIM_ERR_ARG, "truth record " + std::to_string(i) + ": unknown type");
    for (uint64_t i = 0; i < n_calls; i++)
        if (!cmp::known_type(calls[i].type)) return fail(nullptr, MSIM_ERR_ARG, "calls record " + std::to_string(i) + ": unknown type");
    dbg_counts<2>(bases, L, Side{{truth, n_truth, truth_pool, truth_pool_len}, nullptr, truth_flags},
                  Side{{calls, n_calls, calls_pool, calls_pool_len}, nullptr, calls_flags}, flags, counts, tallies);
    return MSIM_OK;
}

// msim_cmp_counts_blocks as sequential loops: the match (dbg_counts), then every record of either table in turn -- head test, walk,
// replay, rescue (cmp_blocks.h) --, then the counters from the final flag bytes.
int msim_dbg_cmp_counts_blocks(const uint8_t *bases, uint64_t L, const msim_record *truth, uint64_t n_truth, const uint8_t *truth_pool,
                               uint64_t truth_pool_len, const msim_record *calls, uint64_t n_calls, const uint8_t *calls_pool,
                               uint64_t calls_pool_len, uint32_t flags, uint32_t gap, uint64_t *counts, uint64_t tallies[2],
                               uint64_t block_tallies[5], uint8_t *truth_flags, uint8_t *calls_flags) {
    if ((!bases && L) || (!truth && n_truth) || (!calls && n_calls) || (!truth_pool && truth_pool_len) ||
        (!calls_pool && calls_pool_len) || !counts || !tallies || !block_tallies || (flags & ~(uint32_t)MSIM_CMP_EXACT))
        return MSIM_ERR_ARG;
    if (gap > MSIM_CMP_BLOCK_SPAN) return fail(nullptr, MSIM_ERR_ARG, "the block gap is larger than MSIM_CMP_BLOCK_SPAN");
    if (n_truth >= (1ull << 31) || n_calls >= (1ull << 31)) return fail(nullptr, MSIM_ERR_ARG, "more than 2^31 records");
    int rc;
    if ((rc = dbg_table_ok("truth", truth, n_truth, true)) || (rc = dbg_table_ok("calls", calls, n_calls, true))) return rc;
    std::vector<uint8_t> fa((size_t)n_truth, 0), fb((size_t)n_calls, 0);
    std::vector<uint64_t> haploid((size_t)8 * MSIM_CMP_BINS * 4);
    const cmp::Table A{truth, n_truth, truth_pool, truth_pool_len}, B{calls, n_calls, calls_pool, calls_pool_len};
    dbg_counts<2>(bases, L, Side{A, nullptr, fa.data()}, Side{B, nullptr, fb.data()}, flags, haploid.data(), tallies);
    memset(block_tallies, 0, 5 * sizeof(uint64_t));
    for (uint64_t i = 0; i < n_truth + n_calls; i++) {
        const bool own_is_truth = i < n_truth;
        const uint64_t own = own_is_truth ? i : i - n_truth;
        uint64_t other;
        if (!blk::is_head(own_is_truth ? A : B, own, own_is_truth ? B : A, own_is_truth, gap, &other)) continue;
        blk::Desc d{};
        const uint32_t what = blk::walk(A, B, fa.data(), fb.data(), own_is_truth ? own : other, own_is_truth ? other : own, gap, &d);
        if (what == blk::NOT_A_CANDIDATE) continue;
        block_tallies[blk::T_CANDIDATE]++;
        block_tallies[what == blk::REPLAY ? blk::T_REPLAYED : what == blk::OVER_LIMIT ? blk::T_LIMIT : blk::T_TRANSLOCATION]++;
        if (what != blk::REPLAY || !blk::replay_equal(bases, L, A, B, d)) continue;
        blk::rescue(fa.data(), fb.data(), d);
        block_tallies[blk::T_EQUAL]++;
    }
    unsigned long long ca[cmp::Score<3>::COUNTERS] = {}, cb[cmp::Score<3>::COUNTERS] = {};
    for (uint64_t i = 0; i < n_truth; i++) ca[cmp::counter_of<3>(cmp::rec_at(truth, i), fa[(size_t)i])]++;
    for (uint64_t i = 0; i < n_calls; i++) cb[cmp::counter_of<3>(cmp::rec_at(calls, i), fb[(size_t)i])]++;
    memset(counts, 0, (size_t)8 * MSIM_CMP_BINS * 6 * sizeof(uint64_t));
    cmp::fold_cells<3>(ca, cb, counts);
    if (truth_flags && n_truth) memcpy(truth_flags, fa.data(), (size_t)n_truth);
    if (calls_flags && n_calls) memcpy(calls_flags, fb.data(), (size_t)n_calls);
    return MSIM_OK;
}

// The join as a sequential merge of the two tables: out[n1 + n2], out_gt[n1 + n2], out_pool[pool1_len + pool2_len], *n_out.
int msim_dbg_cmp_join(const msim_record *h1, uint64_t n1, const uint8_t *pool1, uint64_t pool1_len, const msim_record *h2, uint64_t n2,
                      const uint8_t *pool2, uint64_t pool2_len, msim_record *out, uint8_t *out_pool, uint8_t *out_gt, uint64_t *n_out) {
    if ((!h1 && n1) || (!h2 && n2) || (!pool1 && pool1_len) || (!pool2 && pool2_len) || !n_out || ((n1 || n2) && (!out || !out_gt)) ||
        ((pool1_len || pool2_len) && !out_pool))
        return MSIM_ERR_ARG;
    int rc = join_sizes_ok(nullptr, n1, n2, pool1_len, pool2_len);
    if (rc || (rc = dbg_table_ok("haplotype 1", h1, n1, true)) || (rc = dbg_table_ok("haplotype 2", h2, n2, true))) return rc;
    uint64_t i = 0, j = 0, k = 0;
    while (i < n1 || j < n2) {
        if (j == n2 || (i < n1 && h1[i].pos <= h2[j].pos)) {               // at equal pos haplotype 1's record first
            const cmp::Rec a = cmp::rec_at(h1, i);
            const bool both = j < n2 && h2[j].pos == a.pos &&
                              cmp::same(a, pool1, cmp::comparable(a, pool1_len), cmp::rec_at(h2, j), pool2, pool2_len);
            out[k] = h1[i++];
            out_gt[k++] = both ? 3 : 1;
            if (both) j++;
        } else {
            out[k] = h2[j++];
            if (out[k].type == MSIM_IN) out[k].extra += (uint32_t)pool1_len;
            out_gt[k++] = 2;
        }
    }
    if (pool1_len) memcpy(out_pool, pool1, (size_t)pool1_len);
    if (pool2_len) memcpy(out_pool + pool1_len, pool2, (size_t)pool2_len);
    *n_out = k;
    return MSIM_OK;
}

int msim_dbg_cmp_counts_diploid(const uint8_t *bases, uint64_t L, const msim_record *truth, uint64_t n_truth, const uint8_t *truth_pool,
                                uint64_t truth_pool_len, const uint8_t *truth_gt, const msim_record *calls, uint64_t n_calls,
                                const uint8_t *calls_pool, uint64_t calls_pool_len, const uint8_t *calls_gt, uint32_t flags,
                                uint64_t *counts, uint64_t tallies[2], uint8_t *truth_flags, uint8_t *calls_flags) {
    if ((!bases && L) || ((!truth || !truth_gt) && n_truth) || ((!calls || !calls_gt) && n_calls) || (!truth_pool && truth_pool_len) ||
        (!calls_pool && calls_pool_len) || !counts || !tallies || (flags & ~(uint32_t)MSIM_CMP_EXACT))
        return MSIM_ERR_ARG;
    int rc;
    if ((rc = dbg_table_ok("truth", truth, n_truth, false)) || (rc = dbg_table_ok("calls", calls, n_calls, false)) ||
        (rc = dbg_gt_ok("truth", truth_gt, n_truth)) || (rc = dbg_gt_ok("calls", calls_gt, n_calls)))
        return rc;
    dbg_counts<3>(bases, L, Side{{truth, n_truth, truth_pool, truth_pool_len}, truth_gt, truth_flags},
                  Side{{calls, n_calls, calls_pool, calls_pool_len}, calls_gt, calls_flags}, flags, counts, tallies);
    return MSIM_OK;
}

}  // extern "C"
