// compare --regions / --stratify (msim_cmp_regions_*, msim_cmp_counts_regions): the records of a comparison scored inside BED
// intervals, on the tables and the flag bytes the count calls of compare.hip left -- rule in include/msim.h, shared arithmetic in
// cmp_regions.h.  A contig keeps up to MSIM_CMP_REGION_SETS sets, two uint32 arrays each, beside its held tables.
//   mark     k_region_mark: one lane per record of ONE table and pass -- the record's anchor from one cmp::interval walk over the
//            resident bases, one binary search in global memory per resident set, one mark byte stored (bit s: inside set s).
//            Launched once per table; the walk, the expensive part, is done once for all sets.
//   tally    k_region_tally<OUTCOMES>: streaming, one lane per record -- record, flag byte, mark byte; a record inside every set
//            of the mask is counted where k_cmp_tally counts it, every other record in one "outside" counter (the bin of the
//            match's first walk tally, which a tally never uses).  Lane-private bins and slots as in compare.hip.
// Both grids are capped and stride over the passes.  The bases are read inside [0, L) only and the pools inside their lengths
// (compare.h: walkable), starts / ends inside [0, n) (cmp_regions.h: inside); every record index is checked against its table.
#include <cstring>
#include <string>
#include <vector>

#include "cmp_regions.h"
#include "counter_trip.h"
#include "ctx.h"
#include "lane_hist.h"

namespace msim {

namespace {
struct RegionSet {                             // msim_cmp_regions_set's copy of one set
    bool have = false;
    Scratch<uint32_t> d_starts, d_ends;
    uint64_t n = 0;
};
struct RegionContig {
    RegionSet set[rgn::SETS];
    Scratch<uint8_t> d_mark[2];                // a mark byte per record: MSIM_CMP_TRUTH, MSIM_CMP_CALLS (the last msim_cmp_regions_mark)
    uint64_t n_mark[2] = {0, 0};
    bool marked = false;
    uint32_t marked_flags = 0;                 // the flags of that mark
    uint64_t marked_gen = 0;                   // the contig's table generation it saw (held / current only)
};
}  // namespace

struct RegionState {
    std::vector<RegionContig> contigs;         // by contig index
    CounterTrip out;                           // HIST_SLOTS x (the truth's counters, the calls' counters); its events time the mark too
    double kernel_ms = 0;
};

namespace {

constexpr int LANES = cmp::LANES;
constexpr uint32_t PASS = LANES;                           // records of a workgroup's pass: one a lane
static_assert(PASS == MSIM_CMP_PASS, "msim.h and cmp_regions.hip must agree on the pass");
constexpr unsigned MAX_BLOCKS = 2048;                      // more passes than that stride (compare.hip: CMP_MAX_BLOCKS)
static_assert(sizeof(msim_record) == sizeof(uint4), "a record is one 16-byte load");
constexpr uint32_t KNOWN_FLAGS = MSIM_CMP_EXACT | MSIM_CMP_DIPLOID;

// compare.hip's layout (compare.h: Hist, OUT_WORDS, slot_of).  A table has fewer than 2^31 records, the grid strides beyond
// MAX_BLOCKS passes, a workgroup takes at most 4096 of them and a lane adds once per pass: 16 bits hold it.
using cmp::OUT_WORDS;
template <int OUTCOMES> constexpr uint32_t OUTSIDE = cmp::Score<OUTCOMES>::TALLIES;      // the "outside" counter's bin

__global__ __launch_bounds__(LANES) void k_region_mark(const uint8_t *__restrict__ g, uint64_t L, cmp::Table T, uint32_t exact, uint64_t n_pass,
                                                       rgn::Sets sets, uint8_t *__restrict__ mark) {
    for (uint64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        const uint64_t i = pass * PASS + threadIdx.x;
        if (i >= T.n) continue;
        mark[i] = rgn::mark_of(g, L, cmp::rec_at(T.recs, i), T.pool, T.pool_len, exact != 0, sets);
    }
}

template <int OUTCOMES>
__global__ __launch_bounds__(LANES) void k_region_tally(const msim_record *__restrict__ recs, uint64_t n_rec, uint64_t n_pass,
                                                        const uint8_t *__restrict__ flag, const uint8_t *__restrict__ mark, uint32_t mask,
                                                        unsigned long long *__restrict__ out) {
    __shared__ cmp::Hist<OUTCOMES> hist;
    hist.zero();
    for (uint64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        const uint64_t i = pass * PASS + threadIdx.x;
        if (i >= n_rec) continue;
        const cmp::Rec r = cmp::rec_at(recs, i);
        if (!cmp::known_type(r.type)) continue;            // (k_cmp_tally counts no such record either)
        const uint32_t f = flag[i];
        const bool in = (mark[i] & mask) == mask && f < (uint32_t)OUTCOMES;
        hist.add(in ? cmp::counter_of<OUTCOMES>(r, f) : OUTSIDE<OUTCOMES>, 1u);
    }
    hist.flush(cmp::slot_of<OUTCOMES>(out));
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
// a[]: the truth's counters of the records inside (per cell its outcomes), b[]: the calls'; each side's outside counter behind them
template <int OUTCOMES>
void finish(const unsigned long long *a, const unsigned long long *b, uint64_t *counts, uint64_t outside[2]) {
    cmp::fold_cells<OUTCOMES>(a, b, counts);
    outside[0] += a[OUTSIDE<OUTCOMES>];
    outside[1] += b[OUTSIDE<OUTCOMES>];
}

int state_of(Ctx *c, RegionState **out) {
    RegionState **slot;
    int rc = compare_region_slot(c, &slot);
    if (!rc) rc = lazy_state(c, slot, OUT_WORDS<3>, "the region pass's result buffers and events");   // (the larger of the two layouts)
    if (!rc) *out = *slot;
    return rc;
}

RegionContig &contig_of(RegionState *R, int contig) {
    if (R->contigs.size() <= (size_t)contig) R->contigs.resize((size_t)contig + 1);
    return R->contigs[(size_t)contig];
}

// a device call's prologue: a GPU context, known flags, a contig of that index (held / current: planned), its tables
int region_call(Ctx *c, int contig, uint32_t flags, Contig **g, RegionTables *t, RegionState **R) {
    if (c->host_only) return fail(c, MSIM_ERR_HIP, "host-only context: this call needs the GPU");
    const bool diploid = (flags & MSIM_CMP_DIPLOID) != 0;
    int rc = ctx_device_contig(c, contig, !diploid, g);
    if (rc) return rc;
    if (flags & ~KNOWN_FLAGS) return fail(c, MSIM_ERR_ARG, "unknown compare flag");
    const char *why = "";
    if (!compare_region_tables(c, contig, diploid, t, &why)) return fail(c, MSIM_ERR_ARG, why);
    return state_of(c, R);
}

// the marks of the contig are those of these tables: the refusal, or nullptr
const char *marks_refusal(const RegionContig &rc, const RegionTables &t, uint32_t flags) {
    if (!rc.marked) return "the marks are those of the contig's last msim_cmp_regions_mark: call it first (a set, a hold or a join forgets them)";
    if ((rc.marked_flags ^ flags) & MSIM_CMP_DIPLOID) return "msim_cmp_regions_mark marked the contig's other tables (MSIM_CMP_DIPLOID)";
    if ((rc.marked_flags ^ flags) & MSIM_CMP_EXACT) return "msim_cmp_regions_mark ran with another MSIM_CMP_EXACT bit";
    if (rc.n_mark[0] != t.t[0].n || rc.n_mark[1] != t.t[1].n || rc.marked_gen != t.table_gen)
        return "the contig's tables have changed since msim_cmp_regions_mark";
    return nullptr;
}

template <int OUTCOMES>
int counts_device(Ctx *c, RegionState *R, const RegionContig &rc, const RegionTables &t, uint32_t mask, uint64_t *counts, uint64_t outside[2]) {
    constexpr size_t BINS = cmp::Score<OUTCOMES>::BINS;
    if (!t.t[0].n && !t.t[1].n) return MSIM_OK;
    int rc_trip = R->out.begin(c, OUT_WORDS<OUTCOMES>);
    if (rc_trip) return rc_trip;
    for (int s = 0; s < 2; s++) {
        const uint64_t n = t.t[s].n;
        if (!n) continue;
        const PassGrid pg = pass_grid(n, PASS, MAX_BLOCKS);
        hipLaunchKernelGGL(k_region_tally<OUTCOMES>, pg.grid, dim3(LANES), 0, c->stream, t.t[s].recs, n, pg.n_pass, t.flag[s],
                           (const uint8_t *)rc.d_mark[s].p(), mask, R->out.d.p() + (s ? BINS : 0));
        MSIM_HIP(c, hipGetLastError());
    }
    if ((rc_trip = R->out.finish(c, &R->kernel_ms))) return rc_trip;
    unsigned long long bins[2 * BINS];
    hist_sum_slots(R->out.h.p(), 2 * BINS, bins, 2 * BINS);
    finish<OUTCOMES>(bins, bins + BINS, counts, outside);
    return MSIM_OK;
}

// (host restatement) one table's marks and counters
template <int OUTCOMES>
void dbg_side(const uint8_t *bases, uint64_t L, const cmp::Table &t, const uint8_t *flag, bool exact, const rgn::Sets &sets, uint32_t mask,
              unsigned long long *cnt, uint8_t *marks) {
    for (uint64_t i = 0; i < t.n; i++) {
        const cmp::Rec r = cmp::rec_at(t.recs, i);
        const uint8_t m = rgn::mark_of(bases, L, r, t.pool, t.pool_len, exact, sets);
        if (marks) marks[i] = m;
        const uint32_t f = flag[i];
        cnt[(m & mask) == mask && f < (uint32_t)OUTCOMES ? cmp::counter_of<OUTCOMES>(r, f) : OUTSIDE<OUTCOMES>]++;
    }
}

}  // namespace

void regions_unmark(RegionState *R, int contig) {
    if (!R || contig < 0 || (size_t)contig >= R->contigs.size()) return;
    R->contigs[(size_t)contig].marked = false;
}

void regions_drop(RegionState *R, int contig) {
    if (!R) return;
    if (contig < 0) R->contigs.clear();
    else if ((size_t)contig < R->contigs.size()) R->contigs[(size_t)contig] = RegionContig{};
}

void regions_state_destroy(RegionState *R) { delete R; }

void regions_reset_timing(RegionState *R) {
    if (R) R->kernel_ms = 0;
}

}  // namespace msim

using namespace msim;

extern "C" {

int msim_cmp_regions_set(msim_ctx *p, int contig, int set, const uint32_t *starts, const uint32_t *ends, uint64_t n) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || ((!starts || !ends) && n)) return MSIM_ERR_ARG;
    if (c->host_only) return fail(c, MSIM_ERR_HIP, "host-only context: this call needs the GPU");
    Contig *g;
    int rc = ctx_device_contig(c, contig, false, &g);
    if (rc) return rc;
    if (set < 0 || set >= (int)rgn::SETS) return fail(c, MSIM_ERR_ARG, "region set index outside 0 .. MSIM_CMP_REGION_SETS - 1");
    if (!rgn::normal_form(starts, ends, n, g->len))
        return fail(c, MSIM_ERR_ARG, "region set not in normal form (start < end <= the contig's length, start behind the end in front of it)");
    RegionState *R;
    if ((rc = state_of(c, &R))) return rc;
    RegionContig &rcg = contig_of(R, contig);
    MSIM_HIP(c, wait_stream(c->stream));                    // (nothing reads the arrays that go)
    rcg.marked = false;
    RegionSet &s = rcg.set[set] = RegionSet{};
    if (n) {
        MSIM_HIP(c, dev_alloc(s.d_starts, (size_t)n * sizeof(uint32_t)));
        MSIM_HIP(c, dev_alloc(s.d_ends, (size_t)n * sizeof(uint32_t)));
        MSIM_HIP(c, hipMemcpyAsync(s.d_starts.p(), starts, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        MSIM_HIP(c, hipMemcpyAsync(s.d_ends.p(), ends, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        MSIM_HIP(c, wait_stream(c->stream));
    }
    s.n = n;
    s.have = true;
    return MSIM_OK;
}

int msim_cmp_regions_drop(msim_ctx *p, int contig, int set) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    if (c->host_only) return fail(c, MSIM_ERR_HIP, "host-only context: this call needs the GPU");
    if (set < -1 || set >= (int)rgn::SETS) return fail(c, MSIM_ERR_ARG, "region set index outside -1 .. MSIM_CMP_REGION_SETS - 1");
    RegionState **slot = nullptr;
    if (!c->compare || compare_region_slot(c, &slot) || !*slot) return MSIM_OK;
    RegionState *R = *slot;
    MSIM_HIP(c, wait_stream(c->stream));
    if (contig < 0 || set < 0) { regions_drop(R, contig); return MSIM_OK; }
    if ((size_t)contig >= R->contigs.size()) return MSIM_OK;
    RegionContig &rcg = R->contigs[(size_t)contig];
    rcg.set[set] = RegionSet{};
    rcg.marked = false;
    return MSIM_OK;
}

int msim_cmp_regions_mark(msim_ctx *p, int contig, uint32_t flags) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    Contig *g;
    RegionTables t;
    RegionState *R;
    int rc = region_call(c, contig, flags, &g, &t, &R);
    if (rc) return rc;
    RegionContig &rcg = contig_of(R, contig);
    rcg.marked = false;
    rgn::Sets sets{};
    for (uint32_t s = 0; s < rgn::SETS; s++) {
        const RegionSet &rs = rcg.set[s];
        if (!rs.have) continue;
        sets.s[s] = rgn::Set{rs.d_starts.p(), rs.d_ends.p(), rs.n};
        sets.resident |= 1u << s;
    }
    for (int s = 0; s < 2; s++)
        MSIM_HIP(c, dev_at_least(rcg.d_mark[s], (size_t)t.t[s].n));
    TraceRange tr("msim compare regions mark");
    if (t.t[0].n || t.t[1].n) {
        MSIM_HIP(c, R->out.tm.begin(c->stream));
        for (int s = 0; s < 2; s++) {
            if (!t.t[s].n) continue;
            const PassGrid pg = pass_grid(t.t[s].n, PASS, MAX_BLOCKS);
            hipLaunchKernelGGL(k_region_mark, pg.grid, dim3(LANES), 0, c->stream, g->d_in.p() + PAD, g->len, t.t[s], flags & MSIM_CMP_EXACT, pg.n_pass,
                               sets, rcg.d_mark[s].p());
            MSIM_HIP(c, hipGetLastError());
        }
        MSIM_HIP(c, R->out.tm.end(c->stream));
        MSIM_HIP(c, wait_stream(c->stream));
        if ((rc = R->out.tm.add_elapsed(c, &R->kernel_ms))) return rc;
    }
    rcg.n_mark[0] = t.t[0].n;
    rcg.n_mark[1] = t.t[1].n;
    rcg.marked_flags = flags;
    rcg.marked_gen = t.table_gen;
    rcg.marked = true;
    return MSIM_OK;
}

int msim_cmp_counts_regions(msim_ctx *p, int contig, uint32_t flags, uint32_t mask, uint64_t *counts, uint64_t outside[2]) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !counts || !outside) return MSIM_ERR_ARG;
    Contig *g;
    RegionTables t;
    RegionState *R;
    int rc = region_call(c, contig, flags, &g, &t, &R);
    if (rc) return rc;
    const RegionContig &rcg = contig_of(R, contig);
    if (!t.counted) return fail(c, MSIM_ERR_ARG, "msim_cmp_counts_regions tallies the flag bytes of the contig's last count call again: call it first");
    if ((t.counted_flags ^ flags) & MSIM_CMP_EXACT) return fail(c, MSIM_ERR_ARG, "the contig's last count call ran with another MSIM_CMP_EXACT bit");
    if (const char *why = marks_refusal(rcg, t, flags)) return fail(c, MSIM_ERR_ARG, why);
    uint32_t resident = 0;
    for (uint32_t s = 0; s < rgn::SETS; s++) resident |= rcg.set[s].have ? 1u << s : 0u;
    if (mask & ~resident) return fail(c, MSIM_ERR_ARG, "the mask names a region set that is not resident");
    memset(counts, 0, (size_t)8 * MSIM_CMP_BINS * 2 * (size_t)t.outcomes * sizeof(uint64_t));
    outside[0] = outside[1] = 0;
    TraceRange tr("msim compare regions");
    return t.outcomes == 3 ? counts_device<3>(c, R, rcg, t, mask, counts, outside) : counts_device<2>(c, R, rcg, t, mask, counts, outside);
}

int msim_cmp_fetch_regions(msim_ctx *p, int contig, uint32_t flags, uint8_t *truth_marks, uint8_t *calls_marks) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    Contig *g;
    RegionTables t;
    RegionState *R;
    const int rc = region_call(c, contig, flags, &g, &t, &R);
    if (rc) return rc;
    const RegionContig &rcg = contig_of(R, contig);
    if (const char *why = marks_refusal(rcg, t, flags)) return fail(c, MSIM_ERR_ARG, why);
    uint8_t *dst[2] = {truth_marks, calls_marks};
    for (int s = 0; s < 2; s++)
        if (dst[s] && rcg.n_mark[s]) MSIM_HIP(c, hipMemcpyAsync(dst[s], rcg.d_mark[s].p(), (size_t)rcg.n_mark[s], hipMemcpyDeviceToHost, c->stream));
    MSIM_HIP(c, wait_stream(c->stream));
    return MSIM_OK;
}

int msim_cmp_regions_timing(msim_ctx *p, double *kernel_ms) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    if (c->host_only) return fail(c, MSIM_ERR_HIP, "host-only context: this call needs the GPU");
    RegionState **slot = nullptr;
    if (kernel_ms) *kernel_ms = 0.0;
    if (c->compare && !compare_region_slot(c, &slot) && *slot && kernel_ms) *kernel_ms = (*slot)->kernel_ms;
    return MSIM_OK;
}

// ---- sequential host restatement: no context, no GPU ----------------------------------------------------------------------------
int msim_dbg_cmp_counts_regions(const uint8_t *bases, uint64_t L, const msim_record *truth, uint64_t n_truth, const uint8_t *truth_pool,
                                uint64_t truth_pool_len, const uint8_t *truth_flags, const msim_record *calls, uint64_t n_calls,
                                const uint8_t *calls_pool, uint64_t calls_pool_len, const uint8_t *calls_flags, int outcomes,
                                uint32_t flags, uint32_t n_sets, const uint32_t *starts, const uint32_t *ends, const uint64_t *set_off,
                                uint32_t mask, uint64_t *counts, uint64_t outside[2], uint8_t *truth_marks, uint8_t *calls_marks) {
    if ((!bases && L) || ((!truth || !truth_flags) && n_truth) || ((!calls || !calls_flags) && n_calls) || (!truth_pool && truth_pool_len) ||
        (!calls_pool && calls_pool_len) || !counts || !outside || (flags & ~(uint32_t)MSIM_CMP_EXACT) || (n_sets && !set_off))
        return MSIM_ERR_ARG;
    if (outcomes != 2 && outcomes != 3) return fail(nullptr, MSIM_ERR_ARG, "outcomes: 2 (msim_cmp_counts) or 3 (msim_cmp_counts_blocks, msim_cmp_counts_diploid)");
    if (n_sets > rgn::SETS) return fail(nullptr, MSIM_ERR_ARG, "more than MSIM_CMP_REGION_SETS region sets");
    if (n_sets < 32 && (mask >> n_sets)) return fail(nullptr, MSIM_ERR_ARG, "the mask names a region set that is not resident");
    for (uint64_t i = 0; i < n_truth; i++)
        if (!cmp::known_type(truth[i].type)) return fail(nullptr, MSIM_ERR_ARG, "truth record " + std::to_string(i) + ": unknown type");
    for (uint64_t i = 0; i < n_calls; i++)
        if (!cmp::known_type(calls[i].type)) return fail(nullptr, MSIM_ERR_ARG, "calls record " + std::to_string(i) + ": unknown type");
    rgn::Sets sets{};
    for (uint32_t s = 0; s < n_sets; s++) {
        if (set_off[s + 1] < set_off[s]) return MSIM_ERR_ARG;
        const uint64_t n = set_off[s + 1] - set_off[s];
        if (n && (!starts || !ends)) return MSIM_ERR_ARG;
        sets.s[s] = rgn::Set{n ? starts + set_off[s] : nullptr, n ? ends + set_off[s] : nullptr, n};
        if (!rgn::normal_form(sets.s[s].starts, sets.s[s].ends, n, L))
            return fail(nullptr, MSIM_ERR_ARG, "region set " + std::to_string(s) + " not in normal form (start < end <= the contig's length, start behind the end in front of it)");
        sets.resident |= 1u << s;
    }
    const bool exact = (flags & MSIM_CMP_EXACT) != 0;
    const cmp::Table A{truth, n_truth, truth_pool, truth_pool_len}, B{calls, n_calls, calls_pool, calls_pool_len};
    unsigned long long ca[cmp::Score<3>::COUNTERS] = {}, cb[cmp::Score<3>::COUNTERS] = {};
    memset(counts, 0, (size_t)8 * MSIM_CMP_BINS * 2 * (size_t)outcomes * sizeof(uint64_t));
    outside[0] = outside[1] = 0;
    if (outcomes == 3) {
        dbg_side<3>(bases, L, A, truth_flags, exact, sets, mask, ca, truth_marks);
        dbg_side<3>(bases, L, B, calls_flags, exact, sets, mask, cb, calls_marks);
        finish<3>(ca, cb, counts, outside);
    } else {
        dbg_side<2>(bases, L, A, truth_flags, exact, sets, mask, ca, truth_marks);
        dbg_side<2>(bases, L, B, calls_flags, exact, sets, mask, cb, calls_marks);
        finish<2>(ca, cb, counts, outside);
    }
    return MSIM_OK;
}

}  // extern "C"
