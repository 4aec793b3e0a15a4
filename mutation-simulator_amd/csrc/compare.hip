// The compare mode's device side (msim_cmp_*): a HELD record table (the truth, A) scored against the contig's current one (the
// calls, B), both planned on the same resident contig -- rules in include/msim.h, shared arithmetic in compare.h.
//   hold     msim_cmp_hold: a device copy of the contig's active table and insert pool, kept beside the contig
//   match    k_cmp_match: one lane per A record and step -- its interval from a walk over the resident bases, its rank from a
//            scan of A to the left, a binary search of B for the interval's start, a scan of B for the record of that rank;
//            the lane stores its own flag byte and its partner's (no two lanes share a partner) and counts the record
//   tally    k_cmp_tally: one lane per B record, counted by its flag byte
// Both kernels count into 32 lane-private bins (15 cells x matched / unmatched, two tallies: lane_hist.h).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "compare.h"
#include "ctx.h"
#include "lane_hist.h"

namespace msim {

struct Held {                                  // msim_cmp_hold's copy of one contig's table
    bool have = false;
    Scratch<msim_record> d_recs;
    Scratch<uint8_t> d_pool;
    uint64_t n_rec = 0, pool_len = 0;
    Scratch<uint8_t> d_flag_a, d_flag_b;                   // one byte per held / per current record (the last msim_cmp_counts)
    uint64_t n_flag_b = 0;
    bool counted = false;
};

struct CompareState {
    std::vector<Held> held;                    // by contig index
    Scratch<unsigned long long> d_out;         // HIST_SLOTS x (A's counters, B's counters)
    Pinned<unsigned long long> h_out;          // pinned copy of them
    EventPair tm;
    double kernel_ms = 0;
};

namespace {

constexpr int LANES = 256;
constexpr uint32_t CMP_PASS = LANES;                       // records of a workgroup's pass: one a lane (a walk is long enough)
static_assert(CMP_PASS == MSIM_CMP_PASS, "msim.h and compare.hip must agree on the pass");
static_assert((1u << cmp::WINDOW_SHIFT) == MSIM_CMP_WINDOW, "msim.h and compare.h must agree on the window");
constexpr unsigned CMP_MAX_BLOCKS = 2048;                  // more passes than that stride: eight workgroups a CU (16 KB of LDS each)
constexpr int CMP_BINS = (int)cmp::COUNTERS;
constexpr size_t OUT_WORDS = (size_t)HIST_SLOTS * 2 * CMP_BINS;
static_assert(sizeof(msim_record) == sizeof(uint4), "a record is one 16-byte load");

// 32 lane-private bins, summed in two halves into the workgroup's slot of `out`: 2 x CMP_BINS words a slot, A's counters in
// front of B's (lane_hist.h).  A table has fewer than 2^31 records, so fewer than 2^23 passes; beyond CMP_MAX_BLOCKS passes the
// grid strides, a workgroup takes at most 4096 of them and a lane adds at most once per counter and pass: 16 bits hold it.
using CmpHist = LaneHist<CMP_BINS, LANES, 2>;
__device__ __forceinline__ unsigned long long *slot_of(unsigned long long *out) { return out + (blockIdx.x & (HIST_SLOTS - 1)) * 2 * CMP_BINS; }

// flag_b was zeroed before the launch.  Every index below is checked against its table's size; the bases are read inside
// [0, L) only, the pools inside their lengths (compare.h: walkable, same).
__global__ __launch_bounds__(LANES) void k_cmp_match(const uint8_t *__restrict__ g, uint64_t L, cmp::Table A, cmp::Table B, uint32_t exact,
                                                     uint64_t n_pass, uint8_t *__restrict__ flag_a, uint8_t *__restrict__ flag_b,
                                                     unsigned long long *__restrict__ out) {
    __shared__ CmpHist hist;
    hist.zero();
    for (uint64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        const uint64_t i = pass * CMP_PASS + threadIdx.x;
        if (i >= A.n) continue;
        const cmp::Rec a = cmp::rec_at(A.recs, i);
        if (!cmp::known_type(a.type)) { flag_a[i] = 0; continue; }
        cmp::Span s;
        const int64_t j = cmp::partner(g, L, A, i, B, exact != 0, &s);
        flag_a[i] = j >= 0 ? 1 : 0;
        if (j >= 0 && (uint64_t)j < B.n) flag_b[j] = 1;    // a plain byte store: this lane is the only one with this partner
        hist.add(2 * cmp::cell_of(a) + (j >= 0 ? 0u : 1u), 1u);
        if (s.stops & cmp::STOP_WINDOW) hist.add(2 * cmp::CELLS, 1u);
        if (s.stops & cmp::STOP_BASE) hist.add(2 * cmp::CELLS + 1, 1u);
    }
    hist.flush(slot_of(out));
}

__global__ __launch_bounds__(LANES) void k_cmp_tally(const msim_record *__restrict__ recs, uint64_t n_rec, uint64_t n_pass,
                                                     const uint8_t *__restrict__ flag, unsigned long long *__restrict__ out) {
    __shared__ CmpHist hist;
    hist.zero();
    for (uint64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        const uint64_t i = pass * CMP_PASS + threadIdx.x;
        if (i >= n_rec) continue;
        const cmp::Rec b = cmp::rec_at(recs, i);
        if (cmp::known_type(b.type)) hist.add(2 * cmp::cell_of(b) + (flag[i] ? 0u : 1u), 1u);
    }
    hist.flush(slot_of(out));
}

// counters[0]: A's (matched / missed per cell, the two tallies), counters[1]: B's (matched / extra per cell)
void cmp_finish(const unsigned long long *a, const unsigned long long *b, uint64_t *counts, uint64_t tallies[2]) {
    for (uint32_t cell = 0; cell < cmp::CELLS; cell++) {
        uint32_t type, bin;
        cmp::cell_index(cell, &type, &bin);
        uint64_t *dst = counts + ((size_t)type * MSIM_CMP_BINS + bin) * 4;
        dst[0] += a[2 * cell]; dst[1] += a[2 * cell + 1];
        dst[2] += b[2 * cell]; dst[3] += b[2 * cell + 1];
    }
    tallies[0] += a[2 * cmp::CELLS];
    tallies[1] += a[2 * cmp::CELLS + 1];
}

int state_of(Ctx *c, CompareState **out) {
    if (!c->compare) {
        CompareState *S = new CompareState;
        c->compare = S;
        MSIM_HIP(c, dev_alloc(S->d_out, OUT_WORDS * sizeof(unsigned long long)));
        MSIM_HIP(c, pin_alloc(S->h_out, OUT_WORDS * sizeof(unsigned long long)));
        MSIM_HIP(c, S->tm.create());
    }
    *out = c->compare;
    return MSIM_OK;
}

Held *held_of(Ctx *c, int contig) {
    CompareState *S = c->compare;
    if (!S || contig < 0 || (size_t)contig >= S->held.size() || !S->held[(size_t)contig].have) return nullptr;
    return &S->held[(size_t)contig];
}

int counts_device(Ctx *c, CompareState *S, const Contig &g, Held &h, uint32_t flags, uint64_t *counts, uint64_t tallies[2]) {
    h.counted = false;
    if (g.n_rec > h.d_flag_b.cap) {                        // exactly a byte per record
        MSIM_HIP(c, h.d_flag_b.release());
        MSIM_HIP(c, dev_alloc(h.d_flag_b, (size_t)g.n_rec));
    }
    h.n_flag_b = g.n_rec;
    if (h.n_rec || g.n_rec) {
        const cmp::Table A{h.d_recs.p(), h.n_rec, h.d_pool.p(), h.pool_len};
        const cmp::Table B{g.d_recs.p(), g.n_rec, g.pool_len ? g.d_pool.p() + PAD : nullptr, g.pool_len};
        const uint64_t pass_a = (h.n_rec + CMP_PASS - 1) / CMP_PASS, pass_b = (g.n_rec + CMP_PASS - 1) / CMP_PASS;
        MSIM_HIP(c, hipMemsetAsync(S->d_out.p(), 0, OUT_WORDS * sizeof(unsigned long long), c->stream));
        MSIM_HIP(c, S->tm.begin(c->stream));
        if (g.n_rec) MSIM_HIP(c, hipMemsetAsync(h.d_flag_b.p(), 0, (size_t)g.n_rec, c->stream));
        if (h.n_rec) {
            hipLaunchKernelGGL(k_cmp_match, dim3((unsigned)std::min<uint64_t>(pass_a, CMP_MAX_BLOCKS)), dim3(LANES), 0, c->stream,
                               g.d_in.p() + PAD, g.len, A, B, flags & MSIM_CMP_EXACT, pass_a, h.d_flag_a.p(), h.d_flag_b.p(), S->d_out.p());
            MSIM_HIP(c, hipGetLastError());
        }
        if (g.n_rec) {
            hipLaunchKernelGGL(k_cmp_tally, dim3((unsigned)std::min<uint64_t>(pass_b, CMP_MAX_BLOCKS)), dim3(LANES), 0, c->stream,
                               (const msim_record *)g.d_recs.p(), g.n_rec, pass_b, (const uint8_t *)h.d_flag_b.p(), S->d_out.p() + CMP_BINS);
            MSIM_HIP(c, hipGetLastError());
        }
        MSIM_HIP(c, S->tm.end(c->stream));                  // (in front of the copy: the kernels alone)
        MSIM_HIP(c, hipMemcpyAsync(S->h_out.p(), S->d_out.p(), OUT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        MSIM_HIP(c, wait_stream(c->stream));
        const int rc = S->tm.add_elapsed(c, &S->kernel_ms);
        if (rc) return rc;
        unsigned long long bins[2 * CMP_BINS];
        hist_sum_slots(S->h_out.p(), 2 * CMP_BINS, bins, 2 * CMP_BINS);
        cmp_finish(bins, bins + CMP_BINS, counts, tallies);
    }
    h.counted = true;
    return MSIM_OK;
}

}  // namespace

void compare_drop_all(Ctx *c) {
    if (!c->compare) return;
    c->compare->held.clear();
}

void compare_state_destroy(Ctx *c) {
    CompareState *S = c->compare;
    if (!S) return;
    compare_drop_all(c);
    S->tm.destroy();
    delete S;
    c->compare = nullptr;
}

void compare_reset_timing(Ctx *c) {
    if (c->compare) c->compare->kernel_ms = 0;
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
    return MSIM_OK;
}

int msim_cmp_counts(msim_ctx *p, int contig, uint32_t flags, uint64_t *counts, uint64_t tallies[2]) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !counts || !tallies) return MSIM_ERR_ARG;
    if (flags & ~(uint32_t)MSIM_CMP_EXACT) return fail(c, MSIM_ERR_ARG, "unknown compare flag");
    Contig *g;
    int rc = ctx_device_contig(c, contig, true, &g);
    if (rc) return rc;
    Held *h = held_of(c, contig);
    if (!h) return fail(c, MSIM_ERR_ARG, "contig has no held table (msim_cmp_hold)");
    CompareState *S;
    if ((rc = state_of(c, &S))) return rc;
    memset(counts, 0, (size_t)8 * MSIM_CMP_BINS * 4 * sizeof(uint64_t));
    memset(tallies, 0, 2 * sizeof(uint64_t));
    TraceRange tr("msim compare");
    return counts_device(c, S, *g, *h, flags, counts, tallies);
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

// measurement support (tools/compare_bench.py; exported, not part of msim.h): a device-to-device copy of the held and the current
// table's record bytes into the context's scratch, timed by HIP events -- the streaming floor the compare kernels are held against
int msim_dbg_cmp_copy_floor(msim_ctx *p, int contig, double *ms) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !ms) return MSIM_ERR_ARG;
    Contig *g;
    int rc = ctx_device_contig(c, contig, true, &g);
    if (rc) return rc;
    Held *h = held_of(c, contig);
    if (!h) return fail(c, MSIM_ERR_ARG, "contig has no held table (msim_cmp_hold)");
    CompareState *S;
    if ((rc = state_of(c, &S))) return rc;
    const CopySource tables[2] = {{h->d_recs.p(), (size_t)h->n_rec * sizeof(msim_record)}, {g->d_recs.p(), (size_t)g->n_rec * sizeof(msim_record)}};
    return copy_floor(c, S->tm, tables, 2, ms);
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
    memset(counts, 0, (size_t)8 * MSIM_CMP_BINS * 4 * sizeof(uint64_t));
    memset(tallies, 0, 2 * sizeof(uint64_t));
    std::vector<uint8_t> fb((size_t)n_calls, 0);
    unsigned long long a[cmp::COUNTERS] = {}, b[cmp::COUNTERS] = {};
    const cmp::Table A{truth, n_truth, truth_pool, truth_pool_len}, B{calls, n_calls, calls_pool, calls_pool_len};
    for (uint64_t i = 0; i < n_truth; i++) {
        cmp::Span s;
        const int64_t j = cmp::partner(bases, L, A, i, B, (flags & MSIM_CMP_EXACT) != 0, &s);
        if (truth_flags) truth_flags[i] = j >= 0 ? 1 : 0;
        if (j >= 0) fb[(size_t)j] = 1;
        a[2 * cmp::cell_of(cmp::rec_at(truth, i)) + (j >= 0 ? 0 : 1)]++;
        if (s.stops & cmp::STOP_WINDOW) a[2 * cmp::CELLS]++;
        if (s.stops & cmp::STOP_BASE) a[2 * cmp::CELLS + 1]++;
    }
    for (uint64_t i = 0; i < n_calls; i++) {
        b[2 * cmp::cell_of(cmp::rec_at(calls, i)) + (fb[(size_t)i] ? 0 : 1)]++;
        if (calls_flags) calls_flags[i] = fb[(size_t)i];
    }
    cmp_finish(a, b, counts, tallies);
    return MSIM_OK;
}

}  // extern "C"
