// PLAN on the device: host orchestration of the three engines that reproduce the reference's two MT19937
// streams bit for bit (kernels: plan_kernels.h).                                    gfx950 (MI355X) only.
//
// What the reference does per contig (mutator.py:144-226, util.py:94-109, mutator.py:428-463):
//   random.sample(range(n), k)  -> first k DISTINCT accepted draws of  word >> (32 - bits) < n
//   sorted, + d * rank          -> candidate positions
//   numpy.random.choice(types)  -> a type per candidate (2 NumPy words each)
//   boundary pass               -> keep / drop, randint() for lengths
//   per kept SNP, in position order: uniform(0,1) [2 words], transversion: randbelow(2) [>= 1 word]
//
// All of it is a deterministic function of the word streams, so it can be evaluated out of order as long as
// the *stream positions* come out identical.  The device owns both streams (jump-ahead cascade + chunk
// generation on side streams, ensure_words) and does all per-record work; what differs between the engines is
// how much of the decision logic is a sequential chain that the host has to walk (over device-generated words):
//   plan_contig_gpu            SNP sampler: nothing (fully asynchronous)            -- BASELINE config 2
//   plan_contig_gpu_mixed      SV mix: the boundary chain over non-SNP candidates   -- BASELINE configs 3, 5
//   plan_contig_gpu_hostsample many small deterministic-SNP ranges: the stream cuts   -- BASELINE config 4
// Everything else (translocations, overlapping ranges, ValueError cases) goes through plan_host.cpp.
// DESIGN.md section 3 has the reasoning and the measurements.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>
#include <sys/mman.h>

#include "ctx.h"
#include "mt_jump_table.h"
#include "plan_gpu.h"
#include "plan_kernels.h"

namespace msim {

// ====================================================================== host orchestration
struct GpuStream {
    uint32_t *d_raw = nullptr;          // x[0 .. cap)
    uint64_t cap = 0;
    uint32_t *d_states = nullptr;       // chunk start states
    uint32_t states_cap = 0;            // allocated states
    uint32_t n_states = 0;              // valid states = n_src * (m_done + 1)
    uint32_t lvl = 0, n_src = 1, m_done = 0;   // cascade position: level, states at its start, multipliers done
    SnpMap *d_maps = nullptr;           // CPython stream only: SNP transducer maps of the absolute 8192-word blocks
    SnpLane *d_lanes = nullptr;         //   ... and per lane of every block its masks + map (plan_kernels.h: SnpLane), maps_cap blocks
    size_t maps_cap = 0;                //   (entries)
    uint32_t mapped_blocks = 0;         //   blocks [0, mapped_blocks) are mapped (enqueued on the generation stream)
    unsigned long long maps_ti_lim = 0; //   with this transition threshold
    uint32_t *d_z = nullptr;            // extensions of the current level's source states (k_mt_extend)
    size_t z_cap = 0;                   // in source states
    int z_lvl = -1;                     // level whose sources d_z holds
    uint32_t n_chunks = 0;              // chunks generated
    uint64_t pos = 0;                   // next unconsumed index into x (exact, host copy)
    uint64_t last_session_words = 0;    // words the previous (re)seeded session asked for (its windows' ends): sizing hint
    uint64_t max_upto = 0;              // ... of this session so far
    bool live = false;                  // device copy is the authoritative stream
    // generation runs on its own HIP stream; batch b covers chunks [.., ready_hi[b]) and signals ready_ev[b]
    std::vector<uint32_t> ready_hi;
    std::vector<hipEvent_t> words_ev;   // ... and words_ev[b] as soon as its words are there (the SNP maps of the batch follow)
    uint32_t waited_words = 0;          // the plan stream already waited for the WORDS of chunks below this
    // A session's first two cascade levels and its first generation batch run ON the plan stream (nothing else is there yet and
    // the first contig's chain waits for exactly them): every hand-over between streams costs 50-80 us of idle queue, three of
    // them sat in front of the first chain kernel.  casc_ev: behind the last such launch, for the jump stream to wait on.
    hipEvent_t casc_ev = nullptr;
    bool casc_pending = false;
    std::vector<hipEvent_t> ready_ev;
    uint32_t waited_chunks = 0;         // the plan stream already waited for chunks below this
};

// The scratch blocks own their memory (dev_block.h).  Scratch: device memory; Staging: pinned host memory (host_stage_alloc
// below).  They are grown through Grow alone, which has one rule per kind of block.
static hipError_t host_stage_free(void *p);
using PinBlock = Block<host_stage_free>;
template <class T> struct Staging : PinBlock { T *p() const { return static_cast<T *>(raw); } };

constexpr int N_SETS = 32;               // scratch sets: one per in-flight contig, so the plan stream does not have to
                                         // wait for the emit stream (a cross-stream wait costs tens of us of idle
                                         // queue even when it is about to be satisfied); 288 GB of HBM make this free

struct SampleSet {                       // scratch of one sampled range
    Scratch<uint32_t> acc;                                // accepted draws, stream order
    Scratch<uint32_t> cnt;                                // per-workgroup accept counts / offsets
    Scratch<uint32_t> bitmap;                             // n-bit de-dup bitmap
    Scratch<uint32_t> cnt2;                               // per-workgroup popcounts / ranks
    Scratch<uint32_t> bins;                               // first-k draws grouped by value bin
    Scratch<uint32_t> cursors;                            // per-bin fill counters
    // anchored windows (enqueue_sample_ahead): bookkeeping of the core window and of the head interval, the accepted draws of
    // the head interval with their per-block offsets, and the event behind the set's off-chain work
    uint8_t *ahead = nullptr;                             // PlanState core | PlanState head | SpecHdr
    Scratch<uint32_t> hcnt, hacc;
    hipEvent_t prep_done = nullptr;
    hipEvent_t chain_done = nullptr;                      // behind the set's last kernel on the plan stream (anchored windows)
    uint8_t last_user = 0;                                // since the last finish: 1 a sample on the chain, 2 an anchored window
    hipEvent_t emit_done = nullptr;
    hipEvent_t wait_ev = nullptr;                         // what marks its last emit: its own emit_done or its group's event
    bool pending = false;
};
struct SnpSet {                          // scratch of one contig's SNP draws
    Scratch<SnpMap> maps;
    Scratch<uint8_t> aux8;                                // one-range contigs: the outcomes by rank (folded into the records by k_bitmap_expand)
    unsigned long long *base = nullptr;                   // device word: stream position the draws start at
    hipEvent_t emit_done = nullptr;
    hipEvent_t wait_ev = nullptr;                         // (as SampleSet::wait_ev)
    bool pending = false;
};

struct SnpDefer { SnpSet *T; uint32_t W2, nb2; };           // what a deferred emit pass needs (enqueue_snp_stage)
// A contig whose chain is enqueued and whose emission waits for its group (plan_kernels.h: EmitJobs)
struct EmitItem { int contig; SampleSet *S; SnpSet *T; uint32_t bmw, bnb, start, K, W2, nb2; msim_record *recs; bool apply; };

struct MixedSet {                        // scratch of one SV-mix range (section 6)
    Scratch<uint32_t> cand_pos;                           // candidates in position order
    Scratch<uint8_t> cand_type;                           // MSIM_* id | KEEP_BIT
    Scratch<uint32_t> cand_stop;                          // non-SNP candidates: stop from the host chain
    Scratch<uint32_t> nsn_pos;                            // compacted non-SNP candidates
    Scratch<uint8_t> nsn_type;
    Scratch<uint32_t> nsn_rank;                           // their candidate index
    Scratch<uint32_t> nsn_stop;
    Scratch<uint32_t> sn_index;                           // kept-SNP ordinal -> record index
    Scratch<uint32_t> cnt;                                // five per-workgroup counter arrays
    Scratch<uint32_t> words;                              // tempered word window for the host chain
    unsigned long long *p0_slot = nullptr;                // host-cut contigs: stream position their window started at
    Scratch<WalkRange> walk_d;                            // device-walked / host-cut contigs: range table
    Staging<WalkRange> walk_h;                            //   its pinned staging (one per set: the copy is asynchronous)
    Scratch<uint32_t> wbits;                              //   contig-wide bitmap of sampled positions (zero between uses)
    bool wbits_dirty = false;                             //   a failed pass may have left bits behind
    Scratch<uint32_t> wcnt;                               //   per-workgroup popcounts / ranks of its expansion
    Scratch<uint32_t> tables;                             // host-chain engine: accept tables over the word window
    Scratch<uint32_t> cand_extra;                         //   translocations: linked span start per candidate,
    Scratch<uint8_t> cand_aux;                            //   flags (reversed / insert_pos > 0 / tombstone),
    Scratch<uint32_t> nsn_extra;                          //   and their staging in chain order
    Scratch<uint8_t> nsn_aux;
    Scratch<uint8_t> mm_d;                                //   range table | settings' type tables | visit_from
    Staging<uint8_t> mm_h;                                //   its pinned staging (one per set: the copies are asynchronous)
    hipEvent_t emit_done = nullptr;
    bool pending = false;
};

// The CPython stream's position as the host knows it between two exact readings (anchored windows): mean and variance of the
// words consumed since, and a hard lower bound.
struct ChainEst {
    bool ok = false;
    double e = 0, v = 0;
    uint64_t lo = 0;
    // mean + 16 sigma of the position, never beyond `bound` (the sum of the windows)
    uint64_t hi(uint64_t bound) const {
        if (!ok) return bound;
        const double m = v > 0.0 ? 16.0 * std::sqrt(1.1 * v) + 256.0 : 0.0;
        return std::min<uint64_t>(bound, (uint64_t)std::ceil(e + m));
    }
    void add(const StreamMoments &m, uint64_t least) { if (ok) { e += m.e; v += m.v; lo += least; } }
};
// What the host decides about one sampled range before anything is launched (sample_step): the window, whether its heavy part
// runs off the chain and then on which interval [lo, H] of possible starts, the bounds handed to the kernels.
struct SampleStep {
    bool bad = false;                    // window beyond 2^32 words
    bool ahead = false;                  // anchored window (count / scatter / de-dup off the chain)
    uint64_t lo = 0, H = 0, expect = 0;
    uint32_t soft_half = 0, W = 0;
    uint64_t pos_in = 0;                 // bound of the start (the chain path's window origin)
    uint64_t e_lim = ~0ull;              // bound of the end
};
struct SnpStep { bool bad = false; uint32_t W2 = 0; uint64_t pos_in = 0, e_lim = ~0ull; };
struct SampleSet;
struct Hoisted {                         // a sample whose off-chain part is enqueued (msim_plan_pass)
    SampleStep st; int64_t start, k;     //   what it was laid out for: must be what the contig's own turn arrives at
    SampleSet *S;
    hipEvent_t batch_done;               //   behind the launches of its batch; wait_it: the chain has not waited for it yet
    bool wait_it;
};

struct GpuPlan {
    GpuStream s[2];
    MixedSet mixed[N_SETS];
    uint32_t mixed_unit = 0;
    Staging<uint32_t> h_words;                            // pinned host staging of the boundary chain
    Staging<uint32_t> h_npos;
    Staging<uint8_t> h_ntype;
    Staging<uint32_t> h_nstop;
    Staging<uint32_t> h_win;                              // host-chain engine: the tempered word window (h_words holds the tables)
    Staging<uint32_t> h_nrank;                            //   candidate ordinals of the chain
    Staging<uint32_t> h_nextra;                           //   translocations: what __link_tls decided, chain order
    Staging<uint8_t> h_naux;
    MixSets mm_sets;                                       //   what gpu_plan_multimix_eligible derived for the contig being planned
    const msim_range *mm_for = nullptr; int mm_n = 0;
    hipEvent_t seed_ev = nullptr;       // recorded behind the launches that start a session's streams (streams_to_device)
    hipStream_t gen_stream = nullptr;   // chunk generation (latency-bound, ~300 us per batch)
    hipStream_t jump_stream = nullptr;  // jump cascade: never waits for a generation batch
    std::vector<hipEvent_t> ev_pool;
    uint32_t *d_poly = nullptr;
    PlanState *d_ps = nullptr;
    PlanState *h_mail = nullptr;        // pinned, device-visible mailbox
    // handover without a stream synchronisation (SV mix): sequence number of the mailbox (never 0), written last
    uint32_t *h_sig = nullptr;
    uint32_t epoch = 0;
    hipStream_t copy_stream = nullptr;  // candidates D2H beside the plan stream
    hipEvent_t ev_cand = nullptr, ev_piece[3] = {}, ev_cpiece[3] = {};
    SampleSet sample[N_SETS];
    SnpSet snp[N_SETS];
    uint32_t unit = 0, snp_unit = 0;    // rotation counters
    hipEvent_t chain_ev[2 * N_SETS] = {};
    uint32_t chain_i = 0;
    // ONE event per emission group, behind its rewrite launch, instead of two per contig between the expansion and the rewrite:
    // an event record is a packet on the queue (~6-10 us of it each) -- four of them and the APPLY's two stood between a pair's
    // expansion and its rewrite (70 us in the trace of a step whose emission train is the bound)
    hipEvent_t grp_ev[2 * N_SETS] = {};
    uint32_t grp_i = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;   // chain-time span since the last finish
    bool ps_valid = false;              // device PlanState carries the current session's position
    bool unverified = false;            // work enqueued since the last finish (flags / exact position unknown)
    std::vector<EmitItem> emit_items;   // SNP sampler: contigs waiting for their emission group (gpu_emit_flush)
    uint32_t emit_d = 1;                //   ... and the sampling distance they share
    uint64_t verified_pos = 0;          // exact position at the last finish
    uint64_t reserve_words[2] = {0, 0};
    // per context, read when it is created (tests run several group sizes / stream spans in one process):
    int emit_group = 0;                 //   contigs per emission group (MSIM_EMIT_GROUP; 0 = by the context's role: see plan_contig_gpu)
    int emit_train = 0;                 //   launches of an emission group's train: 3, 6, or 0 = by the context's role (gpu_emit_flush; MSIM_EMIT_TRAIN)
    uint32_t max_chunks = MT_JUMP_MAX_CHUNKS;   //   chunks one (re)seeded session may span (MSIM_DBG_JUMP_MAX_CHUNKS lowers it)
    uint32_t rebases = 0;               //   sessions ended because the next contig would not fit into the span
    uint32_t cand_cap = 0xffffffffu;    //   test knob (MSIM_DBG_CAND_CAP): caps the 16-sigma bound of the chain's candidates, so
                                        //   that the "beyond the bound" paths of the SV-mix and host-chain engines run
    // anchored windows: the CPython stream's position as the host knows it between two exact readings -- mean and variance of
    // the words consumed since (the sampler's rejections and duplicates, the SNP draws' transversion loops), a hard lower bound
    hipStream_t prep_stream = nullptr;  //   the off-chain part of the samples: the stream of the sample being enqueued,
    hipStream_t prep_streams[8] = {};   //   one of these in turn (contigs' off-chain parts are independent of each other)
    // THREE streams at NORMAL priority + ONE in the low-priority pool (round 6; four at the chain's priority in round 5).  Measured
    // on one box, c2 3 Gb, ms per step of a rank that owns 0 / 3 / 12 of 24 contigs (tools/compat_steps.py,
    // profiles/r06_prep_streams.txt):
    //   4 at the chain's priority 2.27 / 2.46 / 3.45   3 there 2.24 / 2.46 / 3.62   2 there 2.11 / 2.93 / 4.03   1 there 2.00 / 4.35 / 5.3
    //   4 normal 2.13 / 2.77 / 3.52   3 normal 2.10 / 2.29 / 3.30   2 normal 2.08 / 2.61 / 3.59   1 normal 1.98 / 3.8 / 4.6
    // and for a rank that owns everything (profiles/r06_prep_stream_pools.txt): 3 normal 3.60-3.70, **3 normal + 1 low 3.43-3.62**,
    // 2 normal + 1 low 3.77-3.82, 3 normal + 1 at the chain's priority 3.67-3.69, 3 normal + 2 low 4.0.
    // Stream layouts are an EMPIRICAL matter on this runtime (up to four hardware queues per priority, which outlive the streams
    // that asked for them), and a layout can slow every LATER pass of the process that has a host chain by ~6 us per kernel launch
    // (the SV-mix engine's plan spans 7.0 -> 10.0 ms per 3 Gb step, c3 30 -> 35 ms): round 5's four streams at the chain's priority
    // did (its "regression" of c3 from 94 to 84 Gbases/s in the driver's line, which measures c3 behind chain-only c2 steps), so do
    // three there, a fourth stream in the low-priority pool beside this one's three (copy stream), GPU_MAX_HW_QUEUES >= 6.  Most
    // of it reads as "nine queues in the process is one too many" (this context: plan | emission, three side streams, the SV-mix
    // engine's copy stream sharing one of them | generation, jump cascade, the fourth side stream = eight) -- round 5's layout
    // does not fit a pure count, and an isolated probe of launch latency against the number of streams shows nothing
    // (tools/hw_queue_probe.py, profiles/r06_hw_queue_probe.txt): the effect needs the real kernels.  NOTES section 10 has every A/B.
    int n_prep = 4, n_prep_low = 1, prep_i = 0, prep_prio = 0;
    double ahead_sigma = 8.0;
    uint32_t prep_waited[8] = {};       //   ... already waited for the words of chunks below this (per stream)
    // Who plans ahead.  Round 5: only a context that has been asked for msim_plan_chain in this pass or the last one (a rank that
    // owns every contig was bound by its emission + APPLY train either way: 4.1 ms on the chain, 4.2-4.7 ahead).  Round 6: with the
    // train in three launches, one event per group and groups of four (gpu_emit_flush) everybody: 3.66 ms against 4.03-4.12
    // (profiles/r06_emission_train.txt).
    int ahead = 2;                      //   0 never (MSIM_NO_AHEAD), 1 sharded ranks only (round 5's default), 2 always
    uint32_t pass_chain_only = 0;       //   msim_plan_chain calls in this pass
    bool sharded_rank = false;          //   ... there were some in this pass or in the one before
    ChainEst est;
    // msim_plan_pass: samples whose off-chain part went out ahead of their contigs' turn, in item order; plan_contig_gpu takes
    // the front one when it reaches the sample (gpu_plan_pass_prep)
    std::deque<Hoisted> hoisted;
    int pass_batch = PREP_G, pass_first = 1;   //   jobs per prep launch / in a segment's first one (MSIM_PASS_BATCH, MSIM_PASS_FIRST):
                                               //   the first chain of a segment waits for the first launch alone (NOTES section 31)
    bool pass_hoist = true;                    //   MSIM_NO_PASS_HOIST: msim_plan_pass issues every prep at its contig's turn
    int pass_streams = 0;                      //   MSIM_PASS_STREAMS: a segment's prep launches rotate over the first so many prep streams (0: all)
    bool pass_gate = false;                    //   MSIM_PASS_GATE: a segment's prep starts behind the SNP maps of the words it reads
    // An anchored contig with one drawing range: fringe, tail and SNP cut go out as ONE launch (k_chain_fused).  ahead_chain fills
    // in the sample's share and holds it; enqueue_snp_stage adds its own and launches.  MSIM_NO_CHAIN_FUSE: the three launches.
    bool chain_fuse = true;
    uint64_t chains_fused = 0;                 //   ... such launches since the context was created (msim_dbg_chains_fused)
    struct { bool on = false; ChainJob J; uint32_t G = 0; SampleSet *S = nullptr; bool grouped = false; } held;
};

GpuPlan *gpu_plan_create() {
    GpuPlan *g = new GpuPlan();
    if (const char *e = getenv("MSIM_EMIT_GROUP")) g->emit_group = std::min(EMIT_G, std::max(0, atoi(e)));
    if (const char *e = getenv("MSIM_DBG_JUMP_MAX_CHUNKS"))
        g->max_chunks = (uint32_t)std::min<long>(MT_JUMP_MAX_CHUNKS, std::max<long>(2, atol(e)));
    if (const char *e = getenv("MSIM_DBG_CAND_CAP")) g->cand_cap = (uint32_t)std::min<long>(0xffffffffl, std::max<long>(1, atol(e)));
    if (const char *e = getenv("MSIM_EMIT_TRAIN")) g->emit_train = atoi(e) == 3 ? 3 : atoi(e) == 6 ? 6 : 0;
    if (getenv("MSIM_NO_AHEAD")) g->ahead = 0;
    else if (const char *e = getenv("MSIM_AHEAD")) g->ahead = std::min(2, std::max(0, atoi(e)));
    if (const char *e = getenv("MSIM_PREP_STREAMS")) { g->n_prep = std::min(8, std::max(1, atoi(e))); g->n_prep_low = 0; }
    if (const char *e = getenv("MSIM_PREP_LOW")) g->n_prep_low = std::min(g->n_prep, std::max(0, atoi(e)));
    if (const char *e = getenv("MSIM_PREP_PRIO")) g->prep_prio = atoi(e);
    if (const char *e = getenv("MSIM_AHEAD_SIGMA")) g->ahead_sigma = std::min(16.0, std::max(0.0, atof(e)));
    if (const char *e = getenv("MSIM_PASS_BATCH")) g->pass_batch = std::min(PREP_G, std::max(1, atoi(e)));
    if (const char *e = getenv("MSIM_PASS_FIRST")) g->pass_first = std::min(PREP_G, std::max(1, atoi(e)));
    if (getenv("MSIM_NO_PASS_HOIST")) g->pass_hoist = false;
    if (const char *e = getenv("MSIM_PASS_GATE")) g->pass_gate = atoi(e) != 0;
    if (const char *e = getenv("MSIM_PASS_STREAMS")) g->pass_streams = std::min(8, std::max(0, atoi(e)));
    if (const char *e = getenv("MSIM_NO_CHAIN_FUSE")) g->chain_fuse = atoi(e) == 0;
    return g;
}

// Page-locked staging buffers of the engines with a host chain (Grow::own): plain 2 MB-aligned memory on huge pages,
// registered with the runtime.  Measured on the bench box per GiB: hipHostMalloc 182 ms + 90 ms to free; aligned_alloc +
// MADV_HUGEPAGE + hipHostRegister 43 ms, unregister + free 37 ms -- and copies are just as asynchronous and as fast
// (57 GB/s; into plain touched memory the "async" copy blocks the caller).  A 1 Gb contig needs 1.7 GB of them at once.
// (mapped, not malloc'ed: a freed block must leave the address space -- glibc would hand a heap block to the next caller
//  while the runtime may still know the range as registered.  The size sits in a header page in front of the block.)
constexpr size_t STAGE_HUGE = (size_t)2 << 20;
static void *host_stage_alloc(size_t sz, hipError_t *err) {
    *err = hipSuccess;
    const size_t total = sz + 2 * STAGE_HUGE;              // room to align the block and for the header in front of it
    void *raw = mmap(nullptr, total, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (raw == MAP_FAILED) return nullptr;
    uint8_t *q = reinterpret_cast<uint8_t *>(((uintptr_t)raw + STAGE_HUGE + STAGE_HUGE - 1) & ~(uintptr_t)(STAGE_HUGE - 1));
    size_t *hdr = reinterpret_cast<size_t *>(q - 4096);
    hdr[0] = (size_t)(uintptr_t)raw;
    hdr[1] = total;
#ifdef MADV_HUGEPAGE
    (void)madvise(q, sz, MADV_HUGEPAGE);
#endif
    *err = hipHostRegister(q, sz, hipHostRegisterDefault);
    if (*err != hipSuccess) { munmap(raw, total); return nullptr; }
    return q;
}
static hipError_t host_stage_free(void *p) {               // p: a block host_stage_alloc gave, never null (Block::release checks)
    (void)hipDeviceSynchronize();                          // (what hipHostFree does by itself: no copy may still use the block)
    const hipError_t e = hipHostUnregister(p);
    const size_t *hdr = reinterpret_cast<const size_t *>(static_cast<uint8_t *>(p) - 4096);
    munmap(reinterpret_cast<void *>((uintptr_t)hdr[0]), hdr[1]);
    return e;
}

// How the scratch blocks grow, one rule per kind; none keeps a block's contents.  One Grow per contig being planned.
struct Grow {
    Ctx *c;
    bool grew = false;                                     // this contig has already drained the streams for a device block
    // Device scratch of a set.  A block is about to be replaced: nothing may be in flight (once per contig).
    int operator()(DevBlock &b, size_t want_bytes) {
        if (b.cap >= want_bytes) return MSIM_OK;
        if (!grew) {
            if (c->gpu) for (auto st : c->gpu->prep_streams) if (st) MSIM_HIP(c, wait_stream(st));
            MSIM_HIP(c, wait_stream(c->stream));
            MSIM_HIP(c, wait_stream(c->emit_stream));
            grew = true;
        }
        MSIM_HIP(c, b.release());
        const size_t sz = want_bytes + want_bytes / 4 + 4096;
        MSIM_HIP(c, hipMalloc(&b.raw, sz));
        b.cap = sz;
        return MSIM_OK;
    }
    // A set's own pinned table (walk_h, mm_h): no stream to wait for, mixed_acquire has waited for the set's emit_done on the host.
    // (also how shared() replaces a block, behind its wait)
    int own(PinBlock &b, size_t want_bytes) {
        if (b.cap >= want_bytes) return MSIM_OK;
        (void)b.release();
        const size_t sz = (want_bytes + want_bytes / 4 + STAGE_HUGE) & ~(STAGE_HUGE - 1);
        hipError_t e;
        void *q = host_stage_alloc(sz, &e);
        if (!q) return e != hipSuccess ? hip_fail(c, e, "hipHostRegister(host staging buffer)") : fail(c, MSIM_ERR_NOMEM, "host staging buffer");
        b.raw = q;
        b.cap = sz;
        return MSIM_OK;
    }
    // The context's shared pinned blocks (GpuPlan::h_*), a group at a time.  An earlier contig's copies may still use the old
    // blocks: before the first of the group is replaced, the plan stream and the copy stream are waited for, once.
    struct Want { PinBlock &b; size_t bytes; };
    int shared(std::initializer_list<Want> group) {
        bool waited = false;
        for (const Want &w : group) {
            if (w.b.cap >= w.bytes) continue;
            if (!waited) {
                MSIM_HIP(c, wait_stream(c->stream));
                if (c->gpu && c->gpu->copy_stream) MSIM_HIP(c, wait_stream(c->gpu->copy_stream));
                waited = true;
            }
            if (int rc = own(w.b, w.bytes)) return rc;
        }
        return MSIM_OK;
    }
};

struct DbgDev {                                            // device blocks of one test-hook call, freed when it returns
    std::vector<DevBlock> blocks;
    template <class T> hipError_t bytes(T **out, size_t sz) {            // exactly sz bytes
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, sz);
        if (e == hipSuccess) { blocks.emplace_back(); blocks.back().raw = q; }
        *out = static_cast<T *>(q);
        return e;
    }
    template <class T> hipError_t get(T **out, size_t n) { return bytes(out, std::max<size_t>(n * sizeof(T), 4) + PAD); }
};

void gpu_plan_destroy(GpuPlan *g) {
    if (!g) return;
    if (g->jump_stream) { (void)wait_stream(g->jump_stream); (void)hipStreamDestroy(g->jump_stream); }
    if (g->gen_stream) { (void)wait_stream(g->gen_stream); (void)hipStreamDestroy(g->gen_stream); }
    for (auto st : g->prep_streams) if (st) { (void)wait_stream(st); (void)hipStreamDestroy(st); }
    for (auto &s : g->s) {
        if (s.d_raw) (void)hipFree(s.d_raw);
        if (s.d_states) (void)hipFree(s.d_states);
        if (s.d_z) (void)hipFree(s.d_z);
        if (s.d_maps) (void)hipFree(s.d_maps);
        if (s.d_lanes) (void)hipFree(s.d_lanes);
        for (auto e : s.ready_ev) (void)hipEventDestroy(e);
        for (auto e : s.words_ev) if (e) (void)hipEventDestroy(e);
        if (s.casc_ev) (void)hipEventDestroy(s.casc_ev);
    }
    for (auto e : g->ev_pool) (void)hipEventDestroy(e);
    for (auto &t : g->sample) {                            // (the sets' Scratch / Staging blocks free themselves: delete g)
        if (t.ahead) (void)hipFree(t.ahead);
        if (t.prep_done) (void)hipEventDestroy(t.prep_done);
        if (t.chain_done) (void)hipEventDestroy(t.chain_done);
        if (t.emit_done) (void)hipEventDestroy(t.emit_done);
    }
    for (auto &t : g->snp) {
        if (t.base) (void)hipFree(t.base);
        if (t.emit_done) (void)hipEventDestroy(t.emit_done);
    }
    for (auto &t : g->mixed) {
        if (t.p0_slot) (void)hipFree(t.p0_slot);
        if (t.emit_done) (void)hipEventDestroy(t.emit_done);
    }
    for (auto e : g->chain_ev) if (e) (void)hipEventDestroy(e);
    for (auto e : g->grp_ev) if (e) (void)hipEventDestroy(e);
    if (g->t0) (void)hipEventDestroy(g->t0);
    if (g->t1) (void)hipEventDestroy(g->t1);
    if (g->seed_ev) (void)hipEventDestroy(g->seed_ev);
    if (g->d_poly) (void)hipFree(g->d_poly);
    if (g->d_ps) (void)hipFree(g->d_ps);
    if (g->h_mail) (void)hipHostFree(g->h_mail);
    if (g->h_sig) (void)hipHostFree(g->h_sig);
    if (g->copy_stream) (void)hipStreamDestroy(g->copy_stream);
    if (g->ev_cand) (void)hipEventDestroy(g->ev_cand);
    for (auto e : g->ev_cpiece) if (e) (void)hipEventDestroy(e);
    for (auto e : g->ev_piece) if (e) (void)hipEventDestroy(e);
    delete g;
}

void gpu_plan_invalidate(GpuPlan *g) {
    g->unit = g->snp_unit = g->mixed_unit = 0;            // a new pass: contig i meets scratch set i again (sizes fit)
    g->sharded_rank = g->pass_chain_only > 0;
    g->pass_chain_only = 0;
    for (auto &s : g->s) {
        if (s.live) s.last_session_words = std::max<uint64_t>(s.pos, s.max_upto);
        s.live = false;
    }
}
void gpu_plan_reserve(GpuPlan *g, uint64_t py_words, uint64_t np_words) { g->reserve_words[0] = py_words; g->reserve_words[1] = np_words; }

// Words one (re)seeded session can address: the jump polynomials (mt_jump_table.h) reach MT_JUMP_MAX_CHUNKS chunks from its origin.
static inline uint64_t span_words(const GpuPlan *g) { return (uint64_t)MT_N + (uint64_t)g->max_chunks * MT_CHUNK_WORDS; }

// The reference's generators have no length limit (mutator.py:105-142 draws from the two global streams for as long as the genome
// lasts; util.py:104), the jump tables have: 8192 chunks = 1.31 G words from a session's origin (-sn 0.01: ~20 Gb of genome).
// Before a contig is handed to a device engine: will its windows fit into what is left of the span?  If not, the session is
// RE-BASED -- everything in flight is finished, the 624-word window at each stream's exact position goes to the host generators
// (gpu_plan_sync_to_host: any such window is a valid state) and the engine's streams_to_device makes it the origin of a new
// session; a synchronisation and a fresh cascade every 1.3 G words.  *fits = false: not even an empty span holds this contig
// (hundreds of millions of candidates on one contig) -- AUTO plans it on the host, which has no such limit.
// The need is an upper bound built from the engines' own window formulas (plan_windows.h: the very functions enqueue_sample_chain,
// the host-cut and host-chain windows and window_of call; enqueue_snp_stage, mixed_link_translocations), summed as if every stage
// started at the end of the previous one's window.  bad: a range no device engine takes (their eligibility refuses it).
StreamNeed stream_need(const msim_params &P, const msim_range *ranges, int n_ranges) {
    const int64_t d = min_block(P);
    double py = 0, K = 0, K_chain = 0, pool_mean = 0, pool_var = 0, e_small = 0, var_small = 0;
    bool has_tl = false, bad = false;
    int n_big = 0;
    for (int i = 0; i < n_ranges; i++) {
        const msim_range &r = ranges[i];
        if (r.k <= 0) continue;
        const double k = (double)r.k, n = (double)range_population(r, d);
        const bool pool = n <= (double)r.setsize;                        // pool path: no rejection, any n
        K += k;
        if (n < k || (!pool && n >= 4294967296.0)) bad = true;           // ValueError: whoever plans it raises it / multi-word getrandbits
        else if (!pool && r.k >= 4096) {                                 // a window of its own (enqueue_sample_chain)
            py += big_sample_window(n, set_path_need_bounded(n, k));
            n_big++;
        } else {                                                         // small ranges share one window (host-cut / host-chain engines)
            const StreamMoments m = small_sample_moments(n, k, (double)r.setsize);
            e_small += m.e; var_small += m.v;
        }
        bool chain = P.block[MSIM_SN] != d;                              // an SNP that blocks rides the chain too
        for (int j = 0; j < r.n_types; j++) {
            const int t = r.types[j];
            if (t == MSIM_SN || !type_drawable(r, j)) continue;
            chain = true;
            if (t == MSIM_TL || t == MSIM_TLI) has_tl = true;
            if (t == MSIM_IN) {
                const double q = type_probability(r, j);
                const double mx = (double)std::max<int64_t>(r.max_len[t], 1);
                pool_mean += k * q * mx;                                 // (every insert at its longest: a bound, not an estimate)
                pool_var += k * q * mx * mx;
            }
        }
        if (chain) K_chain += k;
    }
    py += e_small + 16.0 * std::sqrt(var_small);
    if (K_chain > 0) py += randint_window(K_chain, 0.5);                                    // randint windows (acceptance >= 1/2)
    if (has_tl) py += 6.0 * K_chain + 16.0 * std::sqrt(25.0 * K_chain + 1.0) + 4096.0;      // __link_tls
    py += 4.0 * K + 16.0 * std::sqrt(4.0 * K) + 16384.0 + 3.0 * SNP_BLOCK2;                 // SNP draws (<= 4 words each, expected)
    py += 2.0 * 65536.0 + 8192.0 * n_big;
    return StreamNeed{py, 2.0 * K + pool_mean + 16.0 * std::sqrt(pool_var) + 4096.0, bad};
}

static bool sampler_eligible(const msim_params &P, const msim_range *ranges, int n_ranges);
// The rule itself, on positions the caller names (gpu_plan_make_room: where the streams stand; pass_segment: where they will).
struct RoomVerdict { bool fits, rebase; };
static RoomVerdict room_for(const StreamNeed &need, uint64_t span_w, bool live0, uint64_t pos0, bool live1, uint64_t pos1) {
    const double py = need.py, np = need.np, span = (double)(span_w - MT_N);
    RoomVerdict v;
    v.fits = need.bad || (std::isfinite(py) && py < span && np < span);   // (bad: the engines' eligibility refuses these themselves)
    v.rebase = false;
    if (need.bad || !v.fits) return v;
    const double at0 = live0 ? (double)pos0 : (double)MT_N, at1 = live1 ? (double)pos1 : (double)MT_N;
    v.rebase = (live0 || live1) && (at0 + py > (double)span_w || at1 + np > (double)span_w);
    return v;
}
int gpu_plan_make_room(Ctx *c, GpuPlan *g, const msim_range *ranges, int n_ranges, bool *fits) {
    const GpuStream &s0 = g->s[0], &s1 = g->s[1];
    const RoomVerdict v = room_for(stream_need(c->params, ranges, n_ranges), span_words(g), s0.live, s0.pos, s1.live, s1.pos);
    *fits = v.fits;
    if (v.rebase) {
        const int rc = gpu_plan_sync_to_host(c, g);          // both streams: exact positions -> host states; the next engine reseeds
        if (rc) return rc;
        g->rebases++;
        c->t.stream_rebases++;
    }
    return MSIM_OK;
}

// Side streams of the stream machinery: the jump cascade and chunk generation run beside the plan chain.
static int ensure_side_streams(Ctx *c, GpuPlan *g) {
    if (g->gen_stream) return MSIM_OK;
    // distinct priorities -> distinct hardware queues (streams of one priority may share a queue and
    // then serialise): the cascade must not queue behind a generation batch
    int lo = 0, hi = 0;
    MSIM_HIP(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
    (void)hi;
    // bulk side work at the LOWEST priority: its workgroups (123 KB of LDS each for a jump) must not crowd out
    // the chain kernels of the first contigs, which already wait for nothing but free CU resources
    MSIM_HIP(c, hipStreamCreateWithPriority(&g->gen_stream, hipStreamNonBlocking, lo));
    MSIM_HIP(c, hipStreamCreateWithPriority(&g->jump_stream, hipStreamNonBlocking, lo));
    return MSIM_OK;
}

// Make x[0 .. upto) available to kernels on the PLAN stream.  Jumps and chunk generation are
// enqueued on the generation stream, level by level (after cascade level r the states of chunks
// < 2^(r+1) exist and those chunks can be generated), each batch followed by an event; the plan
// stream only waits for the batch that covers what it is about to read.  With the sizing hint the
// whole session is enqueued at the first call, so the cascade overlaps the planning of the first
// contigs instead of preceding it.
// maps = false: the caller reads the words only (a sample's chain) -- it need not wait for the batch's SNP maps, which the first
// batch of a step delivers ~110 us behind its words
static int ensure_words(Ctx *c, GpuPlan *g, int si, uint64_t upto, bool maps = true, bool wait_plan = true) {
    GpuStream &s = g->s[si];
    {
        int rc0 = ensure_side_streams(c, g);
        if (rc0) return rc0;
    }
    // (the hint for the next session on this context is what this one ASKED for, not what it generated: a first session extends
    //  by doubling, and repeating its 943 chunks where 690 are read cost a third round of jumps and a third more words to
    //  generate and to map, every step: c2 3.89-3.95 -> 3.75-3.87 ms)
    s.max_upto = std::max(s.max_upto, upto);
    const uint64_t have = MT_N + (uint64_t)s.n_chunks * MT_CHUNK_WORDS;
    if (upto > have) {
        // batch the extension: an explicit hint, or what the previous session on this context needed
        // A generation batch costs ~300 us of latency whatever its size, so never extend piecemeal: take
        // what the previous session on this context went through, else at least double the stream.
        const uint64_t span = span_words(g);               // what the jump tables reach from this session's origin
        // (gpu_plan_make_room re-bases the session between contigs so that a plan never gets here; should a window estimate
        //  ever fall short, the caller's recovery for overflowed windows applies: mutator.py re-plans through the host planner)
        if (upto > span) return fail(c, MSIM_ERR_HIP, "GPU sampler: a stream window overflowed its session's jump-table span (results discarded)");
        uint64_t want = std::max<uint64_t>(upto, s.pos + g->reserve_words[si]);
        want = std::max<uint64_t>(want, std::min<uint64_t>(s.last_session_words, want * 64));
        if (s.n_chunks) want = std::max<uint64_t>(want, 2 * have);
        want = std::min<uint64_t>(want, span);             // hints never reach beyond the span
        const uint32_t need_chunks = (uint32_t)((want - MT_N + MT_CHUNK_WORDS - 1) / MT_CHUNK_WORDS);
        // states the cascade will hold once it covers need_chunks: whole levels, then part of one
        uint32_t want_states = 1;
        for (int l = 0; l < MT_JUMP_LEVELS && want_states < need_chunks; l++) {
            const uint32_t R = (uint32_t)MT_JUMP_RADIX[l];
            if ((uint64_t)want_states * R >= need_chunks) { want_states *= (need_chunks + want_states - 1) / want_states; break; }
            want_states *= R;
        }
        if (!g->d_poly) {
            MSIM_HIP(c, hipMalloc(&g->d_poly, sizeof(MT_JUMP_POLY)));
            MSIM_HIP(c, hipMemcpy(g->d_poly, MT_JUMP_POLY, sizeof(MT_JUMP_POLY), hipMemcpyHostToDevice));
        }
        const uint64_t want_cap = MT_N + (uint64_t)need_chunks * MT_CHUNK_WORDS;
        if (want_states > s.states_cap || want_cap > s.cap) {      // grow (rare): quiesce every stream first
            MSIM_HIP(c, wait_stream(g->jump_stream));
            MSIM_HIP(c, wait_stream(g->gen_stream));
            for (auto st : g->prep_streams) if (st) MSIM_HIP(c, wait_stream(st));
            MSIM_HIP(c, wait_stream(c->stream));
            MSIM_HIP(c, wait_stream(c->emit_stream));     // record emission reads the word arrays too
            if (want_states > s.states_cap) {
                uint32_t *ns = nullptr;
                MSIM_HIP(c, hipMalloc(&ns, (size_t)want_states * MT_N * sizeof(uint32_t)));
                if (s.d_states) {
                    MSIM_HIP(c, hipMemcpy(ns, s.d_states, (size_t)s.n_states * MT_N * sizeof(uint32_t), hipMemcpyDeviceToDevice));
                    MSIM_HIP(c, hipFree(s.d_states));
                }
                s.d_states = ns;
                s.states_cap = want_states;
            }
            if (si == 0 && want_cap / SNP_BLOCK2 + 2 > s.maps_cap) {
                SnpMap *nm = nullptr;
                SnpLane *nl = nullptr;
                const size_t cap = (size_t)(want_cap / SNP_BLOCK2 + 2) * 5 / 4;
                MSIM_HIP(c, hipMalloc(&nm, cap * sizeof(SnpMap)));
                MSIM_HIP(c, hipMalloc(&nl, cap * SNP_THREADS * sizeof(SnpLane)));
                if (s.d_maps) {
                    MSIM_HIP(c, hipMemcpy(nm, s.d_maps, (size_t)s.mapped_blocks * sizeof(SnpMap), hipMemcpyDeviceToDevice));
                    MSIM_HIP(c, hipMemcpy(nl, s.d_lanes, (size_t)s.mapped_blocks * SNP_THREADS * sizeof(SnpLane), hipMemcpyDeviceToDevice));
                    MSIM_HIP(c, hipFree(s.d_maps));
                    MSIM_HIP(c, hipFree(s.d_lanes));
                }
                s.d_maps = nm;
                s.d_lanes = nl;
                s.maps_cap = cap;
            }
            if (want_cap > s.cap) {
                uint32_t *nr = nullptr;
                MSIM_HIP(c, hipMalloc(&nr, want_cap * sizeof(uint32_t)));
                if (s.d_raw) {
                    MSIM_HIP(c, hipMemcpy(nr, s.d_raw, have * sizeof(uint32_t), hipMemcpyDeviceToDevice));
                    MSIM_HIP(c, hipFree(s.d_raw));
                }
                s.d_raw = nr;
                s.cap = want_cap;
            }
        }
        static const bool lead_on_plan = getenv("MSIM_NO_LEAD_ON_PLAN") == nullptr;
        auto join_plan_cascade = [&]() -> int {             // the jump stream continues behind what the plan stream did of the cascade
            if (s.casc_pending) {
                MSIM_HIP(c, hipStreamWaitEvent(g->jump_stream, s.casc_ev, 0));
                s.casc_pending = false;
            }
            return MSIM_OK;
        };
        auto take_event = [&](hipEvent_t &ev) -> int {
            if (!g->ev_pool.empty()) { ev = g->ev_pool.back(); g->ev_pool.pop_back(); }
            else MSIM_HIP(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            return MSIM_OK;
        };
        while (s.n_chunks < need_chunks) {
            const uint32_t hi = std::min<uint32_t>(need_chunks, s.n_states);
            // A generation batch costs ~110-140 us of latency whatever its size and batches queue in order; a cascade level costs an
            // extension (50 us) and its jumps, 256 of them at a time (one 88 KB workgroup per CU): ~100 us per round.  Radices
            // 256 x 4 x 8 (round 5; 16 x 16 x 16 x 2 before): the 689 jumps of a 3 Gb -sn 0.01 session are three rounds in two
            // launches, both on the plan stream, and ONE generation batch + ONE map pass follow -- the first chain kernel starts
            // later than it did (0.52 ms against 0.44) but nothing of the cascade runs beside the first contigs' chains any more,
            // which used to stretch them to 2-3 x their time: c2 4.04-4.16 -> 3.92-3.95 ms per step, a chain-only rank 2.60 -> 2.43.
            // MSIM_GEN_FIRST_LEVELS=1: the first batch behind the first level already (256 chunks, 41 M words: the first four
            // contigs), the second level beside their chains -- 3.96-4.01.
            static const uint32_t first_levels = getenv("MSIM_GEN_FIRST_LEVELS") ? (uint32_t)std::max(1, atoi(getenv("MSIM_GEN_FIRST_LEVELS"))) : 2u;
            const uint32_t first_states = first_levels >= 2 ? (uint32_t)(MT_JUMP_RADIX[0] * MT_JUMP_RADIX[1]) : (uint32_t)MT_JUMP_RADIX[0];
            if (hi > s.n_chunks && hi >= std::min<uint32_t>(need_chunks, first_states)) {
                // states [n_chunks, hi) are complete: generate those chunks (the session's first batch on the plan stream itself,
                // right behind the cascade levels that ran there; later ones on the generation stream behind the jump stream)
                const bool first = lead_on_plan && s.n_chunks == 0 && s.casc_pending;
                hipStream_t gs = first ? c->stream : g->gen_stream;
                int rc = MSIM_OK;
                if (!first) {
                    if ((rc = join_plan_cascade())) return rc;
                    hipEvent_t st_ev;
                    rc = take_event(st_ev);
                    if (rc) return rc;
                    MSIM_HIP(c, hipEventRecord(st_ev, g->jump_stream));
                    MSIM_HIP(c, hipStreamWaitEvent(g->gen_stream, st_ev, 0));
                    s.ready_ev.push_back(st_ev);            // recycled with the batch events at the next reseed
                    s.ready_hi.push_back(0);
                    s.words_ev.push_back(nullptr);
                }
                hipLaunchKernelGGL(k_mt_generate, dim3(hi - s.n_chunks), dim3(GEN_THREADS), 0, gs, s.d_states,
                                   s.d_raw, s.n_chunks);
                MSIM_HIP(c, hipGetLastError());
                hipEvent_t wev = nullptr;
                if (si == 0 || first) {
                    rc = take_event(wev);
                    if (rc) return rc;
                    MSIM_HIP(c, hipEventRecord(wev, gs));
                    if (first) {                            // the map pass (and whatever follows there) stays on the generation stream
                        MSIM_HIP(c, hipStreamWaitEvent(g->gen_stream, wev, 0));
                        s.waited_words = hi;                // (the plan stream made these words itself)
                    }
                }
                if (si == 0) {                              // SNP transducer maps of every block the batch completed
                    const uint32_t n_words = (uint32_t)(MT_N + (uint64_t)hi * MT_CHUNK_WORDS);
                    const uint32_t complete = n_words / SNP_BLOCK2;
                    if (complete > s.mapped_blocks) {
                        hipLaunchKernelGGL(k_snp_maps_abs, dim3(complete - s.mapped_blocks), dim3(SNP_THREADS), 0, g->gen_stream,
                                           s.d_raw, n_words, (unsigned long long)c->params.ti_lim, s.mapped_blocks, s.d_maps, s.d_lanes);
                        MSIM_HIP(c, hipGetLastError());
                        s.mapped_blocks = complete;
                    }
                }
                hipEvent_t ev;
                rc = take_event(ev);
                if (rc) return rc;
                MSIM_HIP(c, hipEventRecord(ev, g->gen_stream));
                s.ready_hi.push_back(hi);
                s.ready_ev.push_back(ev);
                s.words_ev.push_back(wev);
                s.n_chunks = hi;
            }
            if (s.n_chunks < need_chunks) {                // extend the cascade (mixed radix, one launch per level)
                if (s.m_done == (uint32_t)MT_JUMP_RADIX[s.lvl] - 1) {       // level complete: the next one starts
                    s.lvl++;
                    s.n_src = s.n_states;
                    s.m_done = 0;
                }
                const uint32_t R = (uint32_t)MT_JUMP_RADIX[s.lvl];
                const uint32_t m_need = std::min<uint32_t>(R - 1, (need_chunks + s.n_src - 1) / s.n_src - 1);
                uint32_t level_base = 0;
                for (uint32_t l = 0; l < s.lvl; l++) level_base += (uint32_t)MT_JUMP_RADIX[l] - 1;
                const bool on_plan = lead_on_plan && s.lvl <= 1 && s.n_chunks == 0;
                hipStream_t js = on_plan ? c->stream : g->jump_stream;
                if (!on_plan) { const int rcj = join_plan_cascade(); if (rcj) return rcj; }
                if (s.z_lvl != (int)s.lvl) {               // extend this level's source states once
                    if (s.z_cap < s.n_src) {
                        MSIM_HIP(c, wait_stream(g->jump_stream));   // the old buffer may still be read
                        MSIM_HIP(c, wait_stream(c->stream));
                        if (s.d_z) MSIM_HIP(c, hipFree(s.d_z));
                        s.d_z = nullptr; s.z_cap = 0;
                        MSIM_HIP(c, hipMalloc(&s.d_z, (size_t)s.n_src * JUMP_ZP * sizeof(uint32_t)));
                        s.z_cap = s.n_src;
                    }
                    hipLaunchKernelGGL(k_mt_extend, dim3(s.n_src), dim3(GEN_THREADS), 0, js, s.d_states, s.d_z);
                    MSIM_HIP(c, hipGetLastError());
                    s.z_lvl = (int)s.lvl;
                }
                hipLaunchKernelGGL(k_mt_jump, dim3(s.n_src * (m_need - s.m_done)), dim3(JUMP_THREADS), 0,
                                   js, s.d_states, s.d_z, s.n_src,
                                   g->d_poly + (size_t)level_base * MT_POLY_WORDS, s.m_done + 1);
                MSIM_HIP(c, hipGetLastError());
                if (on_plan) {
                    if (!s.casc_ev) MSIM_HIP(c, hipEventCreateWithFlags(&s.casc_ev, hipEventDisableTiming));
                    MSIM_HIP(c, hipEventRecord(s.casc_ev, c->stream));
                    s.casc_pending = true;
                }
                s.m_done = m_need;
                s.n_states = s.n_src * (s.m_done + 1);
            }
        }
    }
    // the plan stream waits for the batch that covers `upto`
    if (wait_plan && upto > MT_N) {
        const uint32_t need = (uint32_t)((upto - MT_N + MT_CHUNK_WORDS - 1) / MT_CHUNK_WORDS);
        if (need > (maps ? s.waited_chunks : s.waited_words)) {
            for (size_t b = 0; b < s.ready_hi.size(); b++) {
                if (s.ready_hi[b] >= need) {
                    const bool words_only = !maps && s.words_ev[b];
                    MSIM_HIP(c, hipStreamWaitEvent(c->stream, words_only ? s.words_ev[b] : s.ready_ev[b], 0));
                    s.waited_words = std::max(s.waited_words, s.ready_hi[b]);
                    if (!words_only) s.waited_chunks = s.ready_hi[b];
                    break;
                }
            }
        }
    }
    return MSIM_OK;
}

// host generators -> device streams, both in one go.  The order matters at a step boundary (a pass reseeds, a cohort run reseeds
// per genome, a long genome re-bases every 1.3 G words): every host wait comes FIRST, while the side streams are idle and a
// query of them returns at once; then the device work, one launch per stream with the state in its arguments (k_reseed: h.mt may
// change right after, the arguments were copied at the launch); then ONE event the side streams are ordered behind.  No host wait
// depends on anything enqueued here.  (Stream by stream it was: two copies from a pinned slot, an event, barrier packets on the
// side queues -- and the second stream's routine began by waiting for exactly those queues.)
static int streams_to_device(Ctx *c, GpuPlan *g) {
    if (g->s[0].live && g->s[1].live) return MSIM_OK;
    for (int si = 0; si < 2; si++) {
        GpuStream &s = g->s[si];
        if (s.live) continue;
        if (!s.d_states) {
            MSIM_HIP(c, hipMalloc(&s.d_states, (size_t)MT_N * sizeof(uint32_t)));
            s.states_cap = 1;
        }
        if (!s.d_raw) {
            MSIM_HIP(c, hipMalloc(&s.d_raw, (size_t)MT_N * sizeof(uint32_t)));
            s.cap = MT_N;
        }
    }
    if (!g->d_ps) MSIM_HIP(c, hipMalloc(&g->d_ps, sizeof(PlanState)));
    {
        int rc0 = ensure_side_streams(c, g);
        if (rc0) return rc0;
    }
    MSIM_HIP(c, wait_stream(g->jump_stream));     // nothing of the old session in flight
    MSIM_HIP(c, wait_stream(g->gen_stream));
    for (auto st : g->prep_streams) if (st) MSIM_HIP(c, wait_stream(st));
    if (!g->seed_ev) MSIM_HIP(c, hipEventCreateWithFlags(&g->seed_ev, hipEventDisableTiming));
    static_assert(sizeof(SeedWords) == sizeof(HostMT::mt), "k_reseed carries a host generator's state words");
    for (int si = 0; si < 2; si++) {
        GpuStream &s = g->s[si];
        if (s.live) continue;
        HostMT &h = si ? c->np : c->py;
        SeedWords sw;
        memcpy(sw.w, h.mt, sizeof sw.w);
        hipLaunchKernelGGL(k_reseed, dim3(1), dim3(256), 0, c->stream, sw, s.d_states, s.d_raw, si == 0 ? g->d_ps : (PlanState *)nullptr,
                           (unsigned long long)h.idx);
        MSIM_HIP(c, hipGetLastError());
    }
    MSIM_HIP(c, hipEventRecord(g->seed_ev, c->stream));
    MSIM_HIP(c, hipStreamWaitEvent(g->jump_stream, g->seed_ev, 0));
    MSIM_HIP(c, hipStreamWaitEvent(g->gen_stream, g->seed_ev, 0));
    for (auto st : g->prep_streams) if (st) MSIM_HIP(c, hipStreamWaitEvent(st, g->seed_ev, 0));
    for (int si = 0; si < 2; si++) {
        GpuStream &s = g->s[si];
        if (s.live) continue;
        HostMT &h = si ? c->np : c->py;
        for (auto e : s.ready_ev) g->ev_pool.push_back(e);
        s.ready_ev.clear();
        s.ready_hi.clear();
        for (auto e : s.words_ev) if (e) g->ev_pool.push_back(e);
        s.words_ev.clear();
        s.waited_chunks = 0;
        s.waited_words = 0;
        if (si == 0) for (auto &w : g->prep_waited) w = 0;
        s.casc_pending = false;
        s.n_states = 1;
        s.lvl = 0; s.n_src = 1; s.m_done = 0;
        s.z_lvl = -1;
        s.n_chunks = 0;
        s.mapped_blocks = 0;
        s.maps_ti_lim = c->params.ti_lim;
        s.pos = (uint64_t)h.idx;
        s.max_upto = 0;
        s.live = true;
        if (si == 0) { g->ps_valid = true; g->verified_pos = s.pos; }      // (k_reseed started the bookkeeping block at s.pos)
    }
    return MSIM_OK;
}

// The engines' prologue, in two parts because the SNP sampler reserves its record table between them.
// session_open: both host generators are device streams (nothing to do inside a session); the device PlanState and its mailbox exist.
static int session_open(Ctx *c, GpuPlan *g) {
    int rc;
    if ((rc = streams_to_device(c, g))) return rc;
    if (!g->h_mail) MSIM_HIP(c, hipHostMalloc(&g->h_mail, sizeof(PlanState), hipHostMallocMapped));
    return MSIM_OK;
}
// chain_open: t0 marks where unverified work starts; the device PlanState holds the stream position.  sampler = false (every
// engine but the SNP sampler, which keeps an estimate of the position across contigs): that estimate ends here.
static int chain_open(Ctx *c, GpuPlan *g, bool sampler) {
    if (!g->t0) { MSIM_HIP(c, hipEventCreate(&g->t0)); MSIM_HIP(c, hipEventCreate(&g->t1)); }
    if (!g->unverified) MSIM_HIP(c, hipEventRecord(g->t0, c->stream));
    if (!g->ps_valid) {
        hipLaunchKernelGGL(k_state_init, dim3(1), dim3(1), 0, c->stream, g->d_ps, (unsigned long long)g->s[0].pos);
        g->ps_valid = true;
    }
    if (!sampler) { g->unverified = true; g->est.ok = false; }
    return MSIM_OK;
}

// device stream -> host generator (any 624-word window ending at pos is a valid state)
int gpu_plan_sync_to_host(Ctx *c, GpuPlan *g) {
    int frc = gpu_plan_finish(c, g);
    if (frc) return frc;
    for (int si = 0; si < 2; si++) {
        GpuStream &s = g->s[si];
        if (!s.live) continue;
        HostMT &h = si ? c->np : c->py;
        const uint64_t consumed = s.pos;                  // index of the next word
        int rc = ensure_words(c, g, si, consumed);
        if (rc) return rc;
        if (consumed >= MT_N) {
            MSIM_HIP(c, hipMemcpyAsync(h.mt, s.d_raw + (consumed - MT_N), sizeof h.mt, hipMemcpyDeviceToHost, c->stream));
            h.idx = MT_N;
        } else {
            MSIM_HIP(c, hipMemcpyAsync(h.mt, s.d_raw, sizeof h.mt, hipMemcpyDeviceToHost, c->stream));
            h.idx = (int)consumed;
        }
        MSIM_HIP(c, wait_stream(c->stream));
        h.state_changed();
        s.last_session_words = std::max<uint64_t>(s.pos, s.max_upto);
        s.live = false;
    }
    return MSIM_OK;
}

bool gpu_plan_eligible(const Ctx *c, const msim_range *ranges, int n_ranges) { return sampler_eligible(c->params, ranges, n_ranges); }
static bool sampler_eligible(const msim_params &P, const msim_range *ranges, int n_ranges) {
    const int64_t d = min_block(P);
    if (P.block[MSIM_SN] != d) return false;              // an SNP could block its successor
    int64_t prev_stop = -1;
    for (int i = 0; i < n_ranges; i++) {
        const msim_range &r = ranges[i];
        if (r.k == 0) continue;                           // draws nothing (mutator.py:163-164)
        if (r.k < 4096) return false;                     // tiny ranges: the sequential host walk is faster
        // overlapping or unsorted drawing ranges: the reference merges the per-range dicts with update()
        // (mutator.py:121, later range wins) -- only the host planner reproduces that
        if (r.start <= prev_stop) return false;
        prev_stop = r.stop;
        const int64_t n = range_population(r, d);
        if (r.k < 0 || n < r.k) return false;             // ValueError: let the host planner raise it
        if (n <= r.setsize || n >= (1ll << 32)) return false;   // pool path / multi-word getrandbits
        if (r.start < 0 || r.stop >= (1ll << 32)) return false;
        if (!range_is_deterministic_sn(r)) return false;  // the type draw: every threshold 0 or >= 2^53
    }
    return true;                                          // (a contig that draws nothing is trivially fine)
}

// Everything enqueued so far has completed: collect the sticky flags and the exact stream position.
int gpu_plan_finish(Ctx *c, GpuPlan *g, bool ride_errs) {
    {
        const int rc = gpu_emit_flush(c);                  // (a group that is still waiting goes out now)
        if (rc) return rc;
    }
    if (!g->unverified) return MSIM_OK;
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(1), 0, c->stream, g->d_ps, g->h_mail);
    MSIM_HIP(c, hipGetLastError());
    MSIM_HIP(c, hipEventRecord(g->t1, c->stream));
    if (ride_errs) {                                       // (the counter-based engine does the same behind its lanes: apply_finish)
        const int rc = apply_ride_err_copies(c);
        if (rc) return rc;
    }
    MSIM_HIP(c, wait_stream(c->stream));
    MSIM_HIP(c, wait_stream(c->emit_stream));
    float ms = 0;
    MSIM_HIP(c, hipEventElapsedTime(&ms, g->t0, g->t1));
    c->t.plan_gpu_ms += ms;
    g->unverified = false;
    for (auto &t : g->sample) { t.pending = false; t.last_user = 0; }
    for (auto &t : g->snp) t.pending = false;
    for (auto &t : g->mixed) t.pending = false;
    const PlanState h = *g->h_mail;
    if (h.flags & (FLAG_SAMPLE_OVERFLOW | FLAG_SNP_OVERFLOW)) {
        g->s[0].live = g->s[1].live = false;
        for (auto &t : g->mixed) t.wbits_dirty = true;
        return fail(c, MSIM_ERR_HIP, "GPU sampler: a stream window overflowed its margin (16 sigma; 8 for the start of a sample planned ahead of the chain; results discarded)");
    }
    c->t.py_words += h.pos - g->verified_pos;
    c->t.snp_ahead_margin_permille = std::max<uint64_t>(c->t.snp_ahead_margin_permille, h.ahead_margin_used);
    g->verified_pos = h.pos;
    g->s[0].pos = h.pos;
    return MSIM_OK;
}

// test support (MSIM_DBG_FORCE_OVERFLOW): what a 16-sigma window overflow leaves behind
// A device engine gave up in the middle of a contig (a host wait met its deadline, a HIP call failed): whatever the device
// streams' session holds is no longer a position the host knows.  The session ends here -- the next plan starts from the host
// generators, which the caller sets (msim_seed / msim_set_mt_state: mutator.py restores them before it re-plans).
void gpu_plan_abandon(GpuPlan *g) {
    g->hoisted.clear();
    g->s[0].live = g->s[1].live = false;
    g->unverified = false;
    g->ps_valid = false;
    g->est.ok = false;
}

int gpu_plan_force_overflow(Ctx *c, GpuPlan *g) {
    if (!g->d_ps) return MSIM_OK;
    hipLaunchKernelGGL(k_raise_flag, dim3(1), dim3(1), 0, c->stream, g->d_ps, (uint32_t)FLAG_SAMPLE_OVERFLOW);
    MSIM_HIP(c, hipGetLastError());
    g->unverified = true;
    return MSIM_OK;
}

static hipEvent_t next_chain_event(GpuPlan *g) {
    hipEvent_t &e = g->chain_ev[g->chain_i++ % (2 * N_SETS)];
    if (!e) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
    return e;
}

// A scratch set may still be read by the emit work of its previous user.  Skip the cross-stream wait when that
// work is known to have finished.
static int wait_if_pending(Ctx *c, bool &pending, hipEvent_t ev) {
    if (!pending) return MSIM_OK;
    if (hipEventQuery(ev) == hipSuccess) { pending = false; return MSIM_OK; }
    (void)hipGetLastError();                               // hipErrorNotReady is not an error
    MSIM_HIP(c, hipStreamWaitEvent(c->stream, ev, 0));
    return MSIM_OK;
}

// Capacity of one sub-list of a bin: expected k/n_bins per bin (the last bin is partial), 16 sigma + slack.  Sub-list s of a bin is
// filled by the scatter workgroups with index == s (mod 16).  Only the workgroups up to the one holding the k-th accepted draw
// contribute (the window has slack behind it), each at most 8192 * p_acc draws, of which the bin's share is min(1, 2^20 / n).
static uint32_t sample_bin_cap(uint64_t n, uint32_t k, double p_acc) {
    const uint32_t nbk = (uint32_t)((double)k / p_acc / SPL_BLOCK) + 3;
    const double mean = (double)((nbk + BIN_SUBS - 1) / BIN_SUBS) * SPL_BLOCK * p_acc * std::min(1.0, (double)BIN_VALUES / (double)n);
    return (uint32_t)std::min<double>((double)k + 16.0, 1.25 * mean + 16.0 * std::sqrt(mean) + 512.0);
}

// Enqueue the chain of one sampled range on the plan stream: where does random.sample() end (exact stream
// cut in the device PlanState) and which values did it draw (the set, as a bitmap in S.bitmap).
struct SampleLaunch { SampleSet *S; uint32_t W, bmw, bnb; };
// raw_other / ps_other: a word buffer and a bookkeeping block of the caller's instead of the CPython stream's (the fast RNG
// mode samples every contig from words of its own, position 0: nothing to generate, nothing chained).
// e_limit: the host's (tighter) bound of where the sample ends -- the next stage's window is laid out from min(pos_hi + W,
// e_limit), so a cut beyond that raises the overflow flag instead of letting the next stage read words nobody made.
static int enqueue_sample_chain(Ctx *c, GpuPlan *g, const msim_range &r, int64_t d, uint64_t pos_hi, Grow &grow,
                                SampleLaunch &out, const uint32_t *raw_other = nullptr, PlanState *ps_other = nullptr,
                                uint64_t e_limit = ~0ull) {
    const uint32_t *raw = raw_other ? raw_other : g->s[0].d_raw;
    PlanState *ps = ps_other ? ps_other : g->d_ps;
    int rc;
    const uint32_t k = (uint32_t)r.k;
    const uint64_t n = (uint64_t)range_population(r, d);
    const int bits = bit_length64(n);
    const double p_acc = randbelow_acceptance((double)n);
    const double wd = big_sample_window((double)n, set_path_need((double)n, (double)k));
    if (wd >= 4.0e9) return fail(c, MSIM_ERR_UNSUPPORTED, "sample window beyond 2^32 words");
    const uint32_t W = (uint32_t)wd;
    SampleSet &S = g->sample[g->unit++ % N_SETS];
    S.last_user = 1;
    if ((rc = wait_if_pending(c, S.pending, S.wait_ev))) return rc;            // its last emit may still read it
    const uint32_t nb = (W + ACC_BLOCK - 1) / ACC_BLOCK;
    const size_t bm_words64 = (size_t)((n + 63) / 64);
    const uint32_t bmw = (uint32_t)bm_words64;
    const uint32_t bnb = (bmw + BM_THREADS - 1) / BM_THREADS;
    if ((rc = grow(S.cnt, (size_t)(nb + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = grow(S.cnt2, emit_cnt2_words(bmw) * sizeof(uint32_t)))) return rc;   // (either train's layout: plan_kernels.h)
    if ((rc = grow(S.acc, (size_t)W * sizeof(uint32_t)))) return rc;
    if ((rc = grow(S.bitmap, bm_words64 * 8))) return rc;
    if (!S.emit_done) MSIM_HIP(c, hipEventCreateWithFlags(&S.emit_done, hipEventDisableTiming));
    if (!raw_other) {
        if ((rc = ensure_words(c, g, 0, pos_hi + W + 1, false))) return rc;
        raw = g->s[0].d_raw;                               // (may have been reallocated)
    }
    const uint64_t pos_limit = (raw_other || e_limit == ~0ull) ? ~0ull : std::min<uint64_t>(pos_hi + W, e_limit);
    // ---- chain (plan stream): where does this sample end?
    const uint32_t n_bins = (uint32_t)((n + BIN_VALUES - 1) >> BIN_SHIFT);
    const bool binned = n_bins <= (uint32_t)MAX_BINS;
    const uint32_t bin_cap = binned ? sample_bin_cap(n, k, p_acc) : 0u;
    if (binned) {
        if ((rc = grow(S.bins, (size_t)n_bins * BIN_SUBS * bin_cap * sizeof(uint32_t)))) return rc;
        if ((rc = grow(S.cursors, (size_t)MAX_BINS * BIN_SUBS * sizeof(uint32_t)))) return rc;
        if ((rc = grow(S.bitmap, (size_t)n_bins * BIN_WORDS * 4))) return rc;
    }
    hipLaunchKernelGGL(k_accept_count, dim3(nb), dim3(ACC_THREADS), 0, c->stream, raw, ps, W,
                       (uint32_t)(32 - bits), (uint32_t)n, S.cnt.p(), ps, binned ? S.cursors.p() : nullptr,
                       binned ? n_bins * BIN_SUBS : 0u);
    // the counts' prefix sums: made by their two consumers themselves where the tail kernel can hold them in LDS (every real
    // contig) -- a launch less on the chain; else by a scan of their own
    static const bool no_fold_scan = getenv("MSIM_NO_SCAN_FOLD") != nullptr;
    const uint32_t raw_counts = (binned && nb < (uint32_t)TAIL_LDS_OFFS && !no_fold_scan) ? 1u : 0u;
    if (!raw_counts) hipLaunchKernelGGL(k_scan_u32_w4, dim3(1), dim3(256), 0, c->stream, S.cnt.p(), nb);   // (four waves: see the kernel)
    if (binned) {
        hipLaunchKernelGGL(k_bin_scatter, dim3((W + SPL_BLOCK - 1) / SPL_BLOCK), dim3(ACC_THREADS), 0, c->stream, raw, ps, W,
                           (uint32_t)(32 - bits), (uint32_t)n, k, S.cnt.p(), n_bins, bin_cap, S.cursors.p(), S.bins.p(), S.acc.p(),
                           ps, raw_counts);
        hipLaunchKernelGGL(k_bin_dedupe, dim3(n_bins), dim3(512), 0, c->stream, S.bins.p(), S.cursors.p(), bin_cap, S.bitmap.p(),
                           ps);
        hipLaunchKernelGGL(k_sample_tail, dim3(1), dim3(TAIL_THREADS), 0, c->stream, raw, S.acc.p(), k, S.cnt.p(), nb, W,
                           (uint32_t)(32 - bits), (uint32_t)n, k, S.bitmap.p(), ps, raw_counts, (const PlanState *)nullptr,
                           (const SpecHdr *)nullptr, (unsigned long long)pos_limit);
    } else {
        MSIM_HIP(c, hipMemsetAsync(S.bitmap.p(), 0, bm_words64 * 8, c->stream));
        hipLaunchKernelGGL(k_accept_scatter, dim3(nb), dim3(ACC_THREADS), 0, c->stream, raw, ps, W,
                           (uint32_t)(32 - bits), (uint32_t)n, S.cnt.p(), S.acc.p());
        hipLaunchKernelGGL(k_bitmap_insert, dim3((k + 1023) / 1024), dim3(256), 0, c->stream, S.acc.p(), k, S.bitmap.p(), ps);
        hipLaunchKernelGGL(k_sample_tail, dim3(1), dim3(TAIL_THREADS), 0, c->stream, raw, S.acc.p(), 0u, S.cnt.p(), nb, W,
                           (uint32_t)(32 - bits), (uint32_t)n, k, S.bitmap.p(), ps, 0u, (const PlanState *)nullptr,
                           (const SpecHdr *)nullptr, (unsigned long long)pos_limit);
    }
    MSIM_HIP(c, hipGetLastError());
    out.S = &S; out.W = W; out.bmw = bmw; out.bnb = bnb;
    return MSIM_OK;
}

// ---- anchored windows: the same sample with its heavy part OFF the chain (plan_kernels.h: k_ahead_fringe has the argument).
// The host knows the sample's start to within [lo, H]; count, scatter and de-dup of the first k_core accepted draws from H and
// the compaction of the accepted draws of [lo, H) run on the prep stream as soon as the words exist; the chain keeps the
// fringe pass (needs the exact start), the tail rounds and the cut.  e_limit: the cut may not lie beyond it (what the caller
// will have made sure exists for the stage that follows).
// maps: wait for the batch's SNP maps too (not for their sake: a pass's prep that starts behind them leaves the device to the map
// pass, which the first contig's chain waits for -- MSIM_PASS_GATE)
static int prep_wait_words(Ctx *c, GpuPlan *g, uint64_t upto, bool maps = false) {
    GpuStream &s = g->s[0];
    if (upto <= MT_N) return MSIM_OK;
    const uint32_t need = (uint32_t)((upto - MT_N + MT_CHUNK_WORDS - 1) / MT_CHUNK_WORDS);
    uint32_t &waited = g->prep_waited[g->prep_i];
    if (need <= waited && !maps) return MSIM_OK;
    for (size_t b = 0; b < s.ready_hi.size(); b++) {
        if (s.ready_hi[b] >= need) {
            MSIM_HIP(c, hipStreamWaitEvent(g->prep_stream, s.words_ev[b] && !maps ? s.words_ev[b] : s.ready_ev[b], 0));
            waited = s.ready_hi[b];
            break;
        }
    }
    return MSIM_OK;
}

// The launch geometry of an anchored window: a pure function of the range and of [lo, H].  took = false: counts beyond what the
// chain's kernels hold in LDS (the sample stays on the chain).  W is sized for all K draws from H: the core needs fewer.
struct AheadGeom { uint32_t K, n, shift, W, F, nb, nbh, a_max, k_core, bmw, bnb, n_bins, bin_cap; bool took; };
static AheadGeom ahead_geometry(const msim_range &r, int64_t d, uint64_t lo, uint64_t H, uint32_t W) {
    AheadGeom a{};
    a.K = (uint32_t)r.k;
    const uint64_t n = (uint64_t)range_population(r, d);
    const double p_acc = randbelow_acceptance((double)n);
    a.n = (uint32_t)n; a.shift = (uint32_t)(32 - bit_length64(n)); a.W = W; a.F = (uint32_t)(H - lo);
    a.nb = (W + ACC_BLOCK - 1) / ACC_BLOCK;
    a.nbh = (a.F + ACC_BLOCK - 1) / ACC_BLOCK;
    a.took = a.nb < (uint32_t)TAIL_LDS_OFFS && a.nbh <= (uint32_t)AHEAD_MAX_HEAD_BLOCKS;
    const double F = (double)a.F;
    a.a_max = a.F ? (uint32_t)std::min<double>(F, F * p_acc + 16.0 * std::sqrt(F * p_acc * (1.0 - p_acc)) + 64.0) : 0u;
    a.k_core = a.K - a.a_max;
    a.bmw = (uint32_t)((n + 63) / 64);
    a.bnb = (a.bmw + BM_THREADS - 1) / BM_THREADS;
    a.n_bins = (uint32_t)((n + BIN_VALUES - 1) >> BIN_SHIFT);
    a.bin_cap = sample_bin_cap(n, a.K, p_acc);
    return a;
}

// The next prep stream in turn becomes g->prep_stream (created on first use).
static int next_prep_stream(Ctx *c, GpuPlan *g, int among = 0) {      // among: only the first so many of them (0: all)
    g->prep_i = (g->prep_i + 1) % (among > 0 ? std::min(among, g->n_prep) : g->n_prep);
    if (!g->prep_streams[g->prep_i]) {
        int plo = 0, phi = 0;
        MSIM_HIP(c, hipDeviceGetStreamPriorityRange(&plo, &phi));
        const int prio = g->prep_i >= g->n_prep - g->n_prep_low ? plo : g->prep_prio > 0 ? plo : g->prep_prio < 0 ? phi : 0;
        MSIM_HIP(c, hipStreamCreateWithPriority(&g->prep_streams[g->prep_i], hipStreamNonBlocking, prio));
        if (g->seed_ev) MSIM_HIP(c, hipStreamWaitEvent(g->prep_streams[g->prep_i], g->seed_ev, 0));   // (the session's first 624 words come from k_reseed)
    }
    g->prep_stream = g->prep_streams[g->prep_i];
    return MSIM_OK;
}

// An anchored window's scratch set: the next one in turn, grown to the window, ordered on g->prep_stream behind whatever may
// still read it.
// grouped: the contig's emission goes out with a group (gpu_emit_flush) -- the group's event, behind its rewrite launch, then also
// covers the chain kernels enqueued for it (the emit stream waited for the plan stream's position at the flush), so no event of the
// set's own is recorded behind them: one packet less per contig on the chain's queue
static int ahead_take_set(Ctx *c, GpuPlan *g, const AheadGeom &a, Grow &grow, bool grouped, SampleSet *&out) {
    int rc;
    hipStream_t ps_ = g->prep_stream;
    SampleSet &S = g->sample[g->unit++ % N_SETS];
    const size_t bm_words64 = (size_t)a.bmw;
    if ((rc = grow(S.cnt, (size_t)(a.nb + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = grow(S.cnt2, emit_cnt2_words(a.bmw) * sizeof(uint32_t)))) return rc;   // (either train's layout: plan_kernels.h)
    if ((rc = grow(S.acc, (size_t)a.W * sizeof(uint32_t)))) return rc;
    if ((rc = grow(S.bins, (size_t)a.n_bins * BIN_SUBS * a.bin_cap * sizeof(uint32_t)))) return rc;
    if ((rc = grow(S.cursors, (size_t)MAX_BINS * BIN_SUBS * sizeof(uint32_t)))) return rc;
    if ((rc = grow(S.bitmap, std::max(bm_words64 * 8, (size_t)a.n_bins * BIN_WORDS * 4)))) return rc;
    if ((rc = grow(S.hcnt, (size_t)(a.nbh + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = grow(S.hacc, ((size_t)a.nbh * ACC_BLOCK + 64) * sizeof(uint32_t)))) return rc;
    if (!S.ahead) MSIM_HIP(c, hipMalloc(&S.ahead, 2 * sizeof(PlanState) + sizeof(SpecHdr)));
    if (!S.emit_done) MSIM_HIP(c, hipEventCreateWithFlags(&S.emit_done, hipEventDisableTiming));
    if (!S.prep_done) MSIM_HIP(c, hipEventCreateWithFlags(&S.prep_done, hipEventDisableTiming));
    if (S.pending) {                                       // the set's last emission may still read it
        if (hipEventQuery(S.wait_ev) == hipSuccess) S.pending = false;
        else { (void)hipGetLastError(); MSIM_HIP(c, hipStreamWaitEvent(ps_, S.wait_ev, 0)); }
    }
    // ... and so may the chain of the contig that had the set N_SETS contigs ago (the host may be that far ahead of the device):
    // an anchored window left an event behind its last chain kernel; behind a sample on the chain, whatever the plan stream holds
    if (!S.chain_done) MSIM_HIP(c, hipEventCreateWithFlags(&S.chain_done, hipEventDisableTiming));
    if (S.last_user == 1) MSIM_HIP(c, hipEventRecord(S.chain_done, c->stream));
    if ((S.last_user == 1 || S.last_user == 2) && hipEventQuery(S.chain_done) != hipSuccess) {
        (void)hipGetLastError();
        MSIM_HIP(c, hipStreamWaitEvent(ps_, S.chain_done, 0));
    }
    S.last_user = grouped ? 3 : 2;                         // (3: its group's event -- S.wait_ev, checked above -- stands for chain_done)
    out = &S;
    return MSIM_OK;
}

static PrepJob prep_job(const SampleSet &S, const AheadGeom &a, uint64_t lo, uint64_t H) {
    PrepJob T{};
    T.ps_core = reinterpret_cast<PlanState *>(S.ahead); T.ps_head = T.ps_core + 1; T.hdr = reinterpret_cast<SpecHdr *>(T.ps_head + 1);
    T.cnt = S.cnt.p(); T.cursors = S.cursors.p(); T.hcnt = S.hcnt.p(); T.hacc = S.hacc.p(); T.bins = S.bins.p(); T.acc = S.acc.p();
    T.bitmap = S.bitmap.p();
    T.H = H; T.lo = lo;
    T.W = a.W; T.F = a.F; T.nb = a.nb; T.nbh = a.nbh; T.shift = a.shift; T.n = a.n; T.k_core = a.k_core; T.n_bins = a.n_bins;
    T.bin_cap = a.bin_cap;
    return T;
}

// ---- off the chain: count, scatter, de-dup of J.n samples on g->prep_stream, `done` recorded behind them.  One sample: the
// single-job kernels; several: one launch per stage for all of them (plan_kernels.h: PrepJobs).
static int prep_launch(Ctx *c, GpuPlan *g, PrepJobs &J, hipEvent_t done) {
    hipStream_t ps_ = g->prep_stream;
    const uint32_t *raw = g->s[0].d_raw;
    if (J.n == 1) {
        const PrepJob &T = J.j[0];
        hipLaunchKernelGGL(k_ahead_count, dim3(T.nb + T.nbh), dim3(ACC_THREADS), 0, ps_, raw, T.ps_core, T.ps_head, T.hdr,
                           T.H, T.lo, T.W, T.F, T.nb, T.shift, T.n, T.cnt, T.cursors, T.n_bins * BIN_SUBS, T.hcnt, T.hacc);
        hipLaunchKernelGGL(k_bin_scatter, dim3((T.W + SPL_BLOCK - 1) / SPL_BLOCK), dim3(ACC_THREADS), 0, ps_, raw, T.ps_core, T.W, T.shift,
                           T.n, T.k_core, T.cnt, T.n_bins, T.bin_cap, T.cursors, T.bins, T.acc, T.ps_core, 1u);
        hipLaunchKernelGGL(k_bin_dedupe, dim3(T.n_bins), dim3(512), 0, ps_, T.bins, T.cursors, T.bin_cap, T.bitmap, T.ps_core);
    } else {
        uint32_t cblk = 0, sblk = 0, dblk = 0;
        for (uint32_t i = 0; i < J.n; i++) {
            PrepJob &T = J.j[i];
            T.cblk0 = cblk; T.sblk0 = sblk; T.dblk0 = dblk;
            cblk += T.nb + T.nbh; sblk += (T.W + SPL_BLOCK - 1) / SPL_BLOCK; dblk += T.n_bins;
        }
        hipLaunchKernelGGL(k_ahead_count_b, dim3(cblk), dim3(ACC_THREADS), 0, ps_, raw, J);
        hipLaunchKernelGGL(k_bin_scatter_b, dim3(sblk), dim3(ACC_THREADS), 0, ps_, raw, J);
        hipLaunchKernelGGL(k_bin_dedupe_b, dim3(dblk), dim3(512), 0, ps_, J);
    }
    MSIM_HIP(c, hipGetLastError());
    MSIM_HIP(c, hipEventRecord(done, ps_));
    return MSIM_OK;
}

// ---- on the chain: fringe (exact start), tail rounds, cut.  wait_for: the event behind the sample's off-chain part (nullptr:
// the plan stream has waited for it already -- an earlier sample of the same batch).
// fuse: nothing is launched here -- the launch is held (g->held) until enqueue_snp_stage knows the SNP stage's share of it.
static int ahead_chain(Ctx *c, GpuPlan *g, SampleSet &S, const msim_range &r, const AheadGeom &a, const SampleStep &st, hipEvent_t wait_for,
                       bool grouped, bool fuse, SampleLaunch &out) {
    int rc;
    // (the plan stream waits for the words here, as a sample on the chain would; a set laid out ahead of its turn had them
    //  generated then, on the side streams alone)
    if ((rc = ensure_words(c, g, 0, st.H + a.W + 1, false))) return rc;
    const uint32_t *raw = g->s[0].d_raw;
    PlanState *ps_core = reinterpret_cast<PlanState *>(S.ahead), *ps_head = ps_core + 1;
    SpecHdr *hdr = reinterpret_cast<SpecHdr *>(ps_head + 1);
    if (wait_for) MSIM_HIP(c, hipStreamWaitEvent(c->stream, wait_for, 0));
    const double dups_est = (double)a.K * (double)a.K / (2.0 * (double)a.n);
    const uint32_t items_est = a.a_max + (uint32_t)(dups_est + 16.0 * std::sqrt(dups_est) + 64.0);
    const uint32_t G = std::max(1u, std::min(256u, (items_est + ACC_THREADS * FRINGE_ITEMS - 1) / (ACC_THREADS * FRINGE_ITEMS)));
    if (fuse) {
        ChainJob &J = g->held.J;
        J = ChainJob{};
        J.ps = g->d_ps; J.ps_core = ps_core; J.ps_head = ps_head; J.hdr = hdr;      // (raw: the launch takes the array as it is then)
        J.hcnt = S.hcnt.p(); J.hacc = S.hacc.p(); J.acc = S.acc.p(); J.bitmap = S.bitmap.p();
        J.lo = st.lo; J.expect = st.expect;
        J.F = a.F; J.nbh = a.nbh; J.K = a.K; J.k_core = a.k_core; J.shift = a.shift; J.n = a.n; J.soft_half = st.soft_half;
        J.cnt = S.cnt.p(); J.nb = a.nb; J.W = a.W; J.pos_limit = st.e_lim;
        g->held.G = G; g->held.S = &S; g->held.grouped = grouped; g->held.on = true;
    } else {
        hipLaunchKernelGGL(k_ahead_fringe, dim3(G), dim3(ACC_THREADS), 0, c->stream, raw, g->d_ps, ps_core, ps_head, hdr,
                           (unsigned long long)st.lo, a.F, S.hcnt.p(), a.nbh, S.hacc.p(), S.acc.p(), a.K, a.k_core, a.shift, a.n, S.bitmap.p(),
                           (unsigned long long)st.expect, st.soft_half);
        hipLaunchKernelGGL(k_sample_tail, dim3(1), dim3(TAIL_THREADS), 0, c->stream, raw, S.acc.p(), a.k_core, S.cnt.p(), a.nb, a.W, a.shift, a.n,
                           a.k_core, S.bitmap.p(), g->d_ps, 1u, ps_core, hdr, (unsigned long long)st.e_lim);
        MSIM_HIP(c, hipGetLastError());
        if (!grouped) MSIM_HIP(c, hipEventRecord(S.chain_done, c->stream));
    }
    out.S = &S; out.W = a.W; out.bmw = a.bmw; out.bnb = a.bnb;
    c->t.snp_samples_ahead++;
    static const bool log_ahead = getenv("MSIM_DBG_AHEAD_LOG") != nullptr;
    if (log_ahead) fprintf(stderr, "msim: sample ahead of the chain: K %u, start in [%llu, %llu], core %u draws\n", a.K, (unsigned long long)st.lo, (unsigned long long)st.H, a.k_core);
    (void)r;
    return MSIM_OK;
}

// An anchored window at its contig's own turn: set, off-chain launches and chain in one go -- or, where msim_plan_pass sent the
// off-chain part ahead (g->hoisted), the chain alone.
static int enqueue_sample_ahead(Ctx *c, GpuPlan *g, const msim_range &r, int64_t d, const SampleStep &st, Grow &grow, SampleLaunch &out,
                                bool grouped, bool fuse) {
    int rc;
    const AheadGeom a = ahead_geometry(r, d, st.lo, st.H, st.W);
    if (!g->hoisted.empty()) {
        const Hoisted h = g->hoisted.front();
        g->hoisted.pop_front();
        if (h.start != r.start || h.k != r.k || h.st.lo != st.lo || h.st.H != st.H || h.st.W != st.W || h.st.e_lim != st.e_lim ||
            h.st.expect != st.expect || h.st.soft_half != st.soft_half)
            return fail(c, MSIM_ERR_HIP, "GPU sampler: a sample laid out ahead of its pass does not match its contig's turn (results discarded)");
        return ahead_chain(c, g, *h.S, r, a, st, h.wait_it ? h.batch_done : (hipEvent_t) nullptr, grouped, fuse, out);
    }
    if ((rc = next_prep_stream(c, g))) return rc;
    SampleSet *S = nullptr;
    if ((rc = ahead_take_set(c, g, a, grow, grouped, S))) return rc;
    if ((rc = ensure_words(c, g, 0, st.H + a.W + 1, false))) return rc;
    if ((rc = prep_wait_words(c, g, st.H + a.W + 1))) return rc;
    PrepJobs J;
    J.n = 1;
    J.j[0] = prep_job(*S, a, st.lo, st.H);
    if ((rc = prep_launch(c, g, J, S->prep_done))) return rc;
    return ahead_chain(c, g, *S, r, a, st, S->prep_done, grouped, fuse, out);
}

// SNP draws of a contig's K (kept) SNPs in position order, starting at the device position (ps->snp_base): the chain
// part (k_snp_scan_cut_abs: exact end of the draws) on the plan stream, the aux bytes (k_snp_emit_abs) on the emit
// stream.  pos_hi: upper bound of the start position on entry, of the end position on return.
// aux8_out (SNP sampler, one drawing range): the outcomes go to a compact byte array by rank instead of into the records; the
// caller launches the bitmap expansion behind this stage and hands it that array (*aux8_out).
// defer (with aux8_out): the emit pass is not launched here at all -- the caller queues it for the contig's emission group.
static int enqueue_snp_stage(Ctx *c, GpuPlan *g, Contig &ct, uint64_t K, const uint32_t *sn_index, uint64_t &pos_hi, Grow &grow,
                             uint8_t **aux8_out = nullptr, SnpDefer *defer = nullptr, uint64_t e_limit = ~0ull, bool take_held = false) {
    // take_held: the caller's sample left its launch in g->held (ahead_chain): this stage completes it and sends it
    const bool fused = take_held && g->held.on;
    g->held.on = false;
    const msim_params &P = c->params;
    GpuStream &py = g->s[0];
    int rc;
    const double p_tv = 1.0 - std::min(1.0, (double)P.ti_lim / 9007199254740992.0);
    const double w2 = (double)K * (2.0 + 2.0 * p_tv) + 16.0 * std::sqrt(4.0 * (double)K) + 16384.0;
    if (w2 >= 4.0e9) return fail(c, MSIM_ERR_UNSUPPORTED, "SNP draw window beyond 2^32 words");
    const uint32_t W2 = (uint32_t)w2;
    const uint32_t nb2 = W2 / SNP_BLOCK2 + 2;              // window blocks incl. the partial first one
    SnpSet &T = g->snp[g->snp_unit++ % N_SETS];
    if ((rc = wait_if_pending(c, T.pending, T.wait_ev))) return rc;
    if ((rc = grow(T.maps, (size_t)(nb2 + 1) * sizeof(SnpMap)))) return rc;
    if (aux8_out) {
        if ((rc = grow(T.aux8, (size_t)K + 64))) return rc;
        *aux8_out = T.aux8.p();
    }
    if (!T.base) MSIM_HIP(c, hipMalloc(&T.base, 64));
    if (!T.emit_done) MSIM_HIP(c, hipEventCreateWithFlags(&T.emit_done, hipEventDisableTiming));
    // words AND absolute maps up to the end of the last window block
    if ((rc = ensure_words(c, g, 0, ((pos_hi + W2) / SNP_BLOCK2 + 2) * SNP_BLOCK2))) return rc;
    if (py.maps_ti_lim != P.ti_lim) {                      // titv changed inside a session: the maps are stale
        if (!py.ready_ev.empty()) MSIM_HIP(c, hipStreamWaitEvent(c->stream, py.ready_ev.back(), 0));
        if (py.mapped_blocks)
            hipLaunchKernelGGL(k_snp_maps_abs, dim3(py.mapped_blocks), dim3(SNP_THREADS), 0, c->stream, py.d_raw,
                               (uint32_t)(MT_N + (uint64_t)py.n_chunks * MT_CHUNK_WORDS), (unsigned long long)P.ti_lim, 0u, py.d_maps, py.d_lanes);
        py.maps_ti_lim = P.ti_lim;
    }
    const unsigned long long snp_limit = e_limit == ~0ull ? ~0ull : std::min<uint64_t>(pos_hi + W2, e_limit);
    if (fused) {                                           // the sample's fringe and tail and this stage's cut: one launch
        ChainJob &J = g->held.J;
        J.raw = py.d_raw;
        J.lanes = py.d_lanes; J.abs_maps = py.d_maps; J.win_maps = T.maps.p(); J.base_out = T.base;
        J.snp_limit = snp_limit; J.W2 = W2; J.nb2 = nb2; J.K2 = (uint32_t)K;
        hipLaunchKernelGGL(k_chain_fused, dim3(g->held.G), dim3(ACC_THREADS), 0, c->stream, J);
        MSIM_HIP(c, hipGetLastError());
        if (!g->held.grouped) MSIM_HIP(c, hipEventRecord(g->held.S->chain_done, c->stream));
        g->chains_fused++;
    } else {
        hipLaunchKernelGGL(k_snp_scan_cut_abs, dim3(1), dim3(SNP_THREADS), 0, c->stream, py.d_lanes, g->d_ps, W2,
                           py.d_maps, T.maps.p(), nb2, (uint32_t)K, T.base, snp_limit);
        MSIM_HIP(c, hipGetLastError());
    }
    if (defer) { defer->T = &T; defer->W2 = W2; defer->nb2 = nb2; }
    if (!c->chain_only && !defer) {                       // (chain only: where the draws END is all that is wanted)
        hipEvent_t ce = next_chain_event(g);
        MSIM_HIP(c, hipEventRecord(ce, c->stream));
        MSIM_HIP(c, hipStreamWaitEvent(c->emit_stream, ce, 0));
        hipLaunchKernelGGL(k_snp_emit_abs, dim3(nb2), dim3(SNP_THREADS), 0, c->emit_stream, py.d_lanes, T.base, W2,
                           T.maps.p(), nb2, ct.d_recs.p(), (uint32_t)K, sn_index, aux8_out ? T.aux8.p() : (uint8_t *)nullptr);
        MSIM_HIP(c, hipGetLastError());
        if (!aux8_out) {                                  // (else: the caller records it behind the expansion that reads aux8)
            MSIM_HIP(c, hipEventRecord(T.emit_done, c->emit_stream));
            T.wait_ev = T.emit_done;
            T.pending = true;
        }
    }
    pos_hi += W2;
    return MSIM_OK;
}

// The launches of a train in front of its rewrite, on `es` (gpu_emit_flush; gpu_dbg_emit_train on a caller's bitmaps).  J carries
// the jobs' buffers and sizes (bmw, bnb, nb2); their places in the grids are laid out here.  Jobs without SNP draws (nb2 == 0
// throughout: aux8 is already there) launch no outcome blocks.
static void emit_train_launch(hipStream_t es, const SnpLane *lanes, EmitJobs &J, bool train3) {
    uint32_t blk = 0, eblk = 0, cblk = 0, xblk = 0;
    for (uint32_t i = 0; i < J.n; i++) {
        EmitJob &T = J.j[i];
        T.blk0 = blk; T.eblk0 = eblk; T.cblk0 = cblk; T.xblk0 = xblk;
        blk += T.bnb; eblk += T.nb2; cblk += emit_supers(T.bmw); xblk += emit_blocks(T.bmw);
    }
    J.total_blk = blk; J.total_eblk = eblk; J.total_cblk = cblk;
    if (train3) {
        if (eblk + cblk) hipLaunchKernelGGL(k_snp_emit_count_b, dim3(eblk + cblk), dim3(SNP_THREADS), 0, es, lanes, J);
        if (xblk) hipLaunchKernelGGL(k_bitmap_expand_tiles_b, dim3(xblk), dim3(BM_THREADS), 0, es, J);
    } else {
        if (blk) hipLaunchKernelGGL(k_bitmap_count_b, dim3(blk), dim3(BM_THREADS), 0, es, J);
        hipLaunchKernelGGL(k_scan_u32_b, dim3(J.n), dim3(256), 0, es, J);
        if (eblk) hipLaunchKernelGGL(k_snp_emit_abs_b, dim3(eblk), dim3(SNP_THREADS), 0, es, lanes, J);
        if (blk) hipLaunchKernelGGL(k_bitmap_expand_b, dim3(blk), dim3(BM_THREADS), 0, es, J);
    }
}

// The emission group: count, scan, SNP outcomes and expansion of every queued contig in one launch per stage on the emission
// stream, behind the chain of the last one; then the APPLYs msim_apply_contig marked (one tile-index launch for all of them,
// apply.hip: apply_batch_device), the rewrite kernels back to back.
int gpu_emit_flush(Ctx *c) {
    GpuPlan *g = c->gpu;
    if (!g || g->emit_items.empty()) return MSIM_OK;
    std::vector<EmitItem> items;
    items.swap(g->emit_items);
    EmitJobs J;
    memset(&J, 0, sizeof J);
    J.n = (uint32_t)items.size();
    J.d = g->emit_d;
    for (uint32_t i = 0; i < J.n; i++) {
        const EmitItem &it = items[i];
        EmitJob &T = J.j[i];
        T.bm = reinterpret_cast<const uint64_t *>(it.S->bitmap.p()); T.cnt2 = it.S->cnt2.p(); T.recs = it.recs; T.aux8 = it.T->aux8.p();
        T.base = it.T->base; T.win_maps = it.T->maps.p();
        T.bmw = it.bmw; T.bnb = it.bnb; T.start = it.start; T.K = it.K; T.W2 = it.W2; T.nb2 = it.nb2;
    }
    hipStream_t es = c->emit_stream;
    // The train in three launches (MSIM_EMIT_TRAIN=6: the six of rounds 4-5: count, scan, outcomes, expansion, tile index,
    // rewrite): outcomes + popcounts in one grid; the expansion makes its rank base from two levels of counts and writes the
    // APPLY tile index of the contigs that are applied with their group; the rewrite.
    // Which one: measured on one box, c2 3 Gb, ms per step (profiles/r06_emission_train.txt).  A rank that owns everything and
    // samples on the chain is bound by that chain, and the denser train slows the chain's kernels more than the six small
    // launches with their gaps did: 3.88 (six) against 4.07-4.14 (three).  Where the samples' heavy kernels run off the chain
    // (anchored windows: ranks of a sharded step, MSIM_AHEAD=2) the train is the bound: a rank owning 12 of 24 contigs 3.35-3.47
    // (six) -> 3.18-3.21 (three); owning 3: 2.38-2.40 / 2.34-2.41.
    const bool ahead_in_use = g->ahead == 2 || (g->ahead == 1 && g->sharded_rank);
    const bool train3 = g->emit_train == 3 || (g->emit_train == 0 && ahead_in_use);
    std::vector<int> applies;
    if (train3) {
        for (uint32_t i = 0; i < J.n; i++) {
            const EmitItem &it = items[i];
            EmitJob &T = J.j[i];
            T.first = nullptr; T.err = nullptr; T.n_tiles = 0;
            if (it.apply && (size_t)it.contig < c->contigs.size()) {
                Contig &ct = c->contigs[(size_t)it.contig];
                ct.apply_stream = es;                      // (apply_batch_device takes contigs with a stream of their own)
                uint32_t shift = 0;
                const int rc = apply_prepare_tile_index(c, ct, es, &T.first, &T.n_tiles, &shift, &T.err);
                if (rc) return rc;
                J.tile_shift = shift;
                if (!T.n_tiles) T.first = nullptr;
                applies.push_back(it.contig);
            }
        }
    }
    hipEvent_t ce = next_chain_event(g);
    MSIM_HIP(c, hipEventRecord(ce, c->stream));
    MSIM_HIP(c, hipStreamWaitEvent(es, ce, 0));
    emit_train_launch(es, g->s[0].d_lanes, J, train3);
    MSIM_HIP(c, hipGetLastError());
    for (const EmitItem &it : items) {
        if (!train3 && it.apply && (size_t)it.contig < c->contigs.size()) {
            c->contigs[(size_t)it.contig].apply_stream = es;      // (apply_batch_device takes contigs with a stream of their own)
            applies.push_back(it.contig);
        }
    }
    const int arc = applies.empty() ? MSIM_OK : apply_batch_device(c, applies, true);
    // the group's event: behind the rewrite (a scratch set meets its next user a step later -- what it waits for may as well
    // include the APPLY)
    hipEvent_t &ge = g->grp_ev[g->grp_i++ % (2 * N_SETS)];
    if (!ge) MSIM_HIP(c, hipEventCreateWithFlags(&ge, hipEventDisableTiming));
    MSIM_HIP(c, hipEventRecord(ge, es));
    for (const EmitItem &it : items) {
        it.S->wait_ev = ge; it.S->pending = true;
        it.T->wait_ev = ge; it.T->pending = true;
    }
    return arc;
}

// test support (msim_dbg_emit_train): the train of gpu_emit_flush over bitmaps and SNP outcomes the caller made, in buffers of
// its own, synchronous.  Job i: bm[i] (n_words[i] words), start[i], the contig's length len[i], aux8[i] by rank; out: recs[i]
// (cap_recs[i] records of room; n_recs[i] = the bitmap's set bits) and, train 3 and first[i] given, the tile index of
// len[i] bytes (n_tiles + 1 entries, n_tiles = ceil(len / tile); tile = 1 << tile_shift as apply.hip has it).
int gpu_dbg_emit_train(Ctx *c, int n_jobs, const uint64_t *const *bm, const uint32_t *n_words, const uint32_t *start,
                       const uint64_t *len, const uint8_t *const *aux8, uint32_t d, int train, uint32_t tile_shift,
                       msim_record *const *recs, const uint64_t *cap_recs, uint64_t *n_recs, int32_t *const *first) {
    if (n_jobs < 1 || n_jobs > EMIT_G || (train != 3 && train != 6) || !bm || !n_words || !start || !len || !aux8 || !recs ||
        !cap_recs || !n_recs || tile_shift < 4 || tile_shift > 30)
        return fail(c, MSIM_ERR_ARG, "msim_dbg_emit_train: bad argument");
    DbgDev dev;
    std::vector<uint64_t> cnt((size_t)n_jobs, 0);
    unsigned long long *d_err = nullptr;
    MSIM_HIP(c, dev.bytes(&d_err, sizeof(unsigned long long) * EMIT_G));
    EmitJobs J;
    memset(&J, 0, sizeof J);
    J.n = (uint32_t)n_jobs; J.d = d; J.tile_shift = tile_shift;
    hipStream_t es = c->emit_stream;
    for (int i = 0; i < n_jobs; i++) {
        if (!bm[i] || !n_words[i] || n_words[i] > (1u << 26) || !recs[i] || !aux8[i])
            return fail(c, MSIM_ERR_ARG, "msim_dbg_emit_train: a job without a bitmap or without room for its records");
        for (uint32_t q = 0; q < n_words[i]; q++) cnt[(size_t)i] += (uint64_t)__builtin_popcountll(bm[i][q]);
        n_recs[i] = cnt[(size_t)i];
        const uint64_t last = (uint64_t)start[i] + 64ull * n_words[i] + (uint64_t)d * cnt[(size_t)i];
        if (cnt[(size_t)i] > cap_recs[i] || last >= (1ull << 32) || len[i] >= (1ull << 32))
            return fail(c, MSIM_ERR_ARG, "msim_dbg_emit_train: more records than room, or positions beyond 2^32");
        const size_t n_tiles = (size_t)((len[i] + (1ull << tile_shift) - 1) >> tile_shift);
        const size_t sz[5] = {(size_t)n_words[i] * 8, emit_cnt2_words(n_words[i]) * sizeof(uint32_t),
                              (size_t)(cnt[(size_t)i] + 1) * sizeof(msim_record), (size_t)cnt[(size_t)i] + 1,
                              (n_tiles + 1) * sizeof(int32_t)};
        void *p[5];
        for (int q = 0; q < 5; q++) MSIM_HIP(c, dev.bytes(&p[q], sz[q]));
        MSIM_HIP(c, hipMemcpyAsync(p[0], bm[i], sz[0], hipMemcpyHostToDevice, es));
        MSIM_HIP(c, hipMemcpyAsync(p[3], aux8[i], (size_t)cnt[(size_t)i], hipMemcpyHostToDevice, es));
        MSIM_HIP(c, hipMemsetAsync(p[4], 0xee, sz[4], es));
        EmitJob &T = J.j[i];
        T.bm = static_cast<const uint64_t *>(p[0]); T.cnt2 = static_cast<uint32_t *>(p[1]);
        T.recs = static_cast<msim_record *>(p[2]); T.aux8 = static_cast<uint8_t *>(p[3]);
        T.bmw = n_words[i]; T.bnb = (n_words[i] + BM_THREADS - 1) / BM_THREADS; T.start = start[i]; T.K = (uint32_t)cnt[(size_t)i];
        if (train == 3 && first && first[i] && n_tiles) {
            T.first = static_cast<int32_t *>(p[4]); T.n_tiles = (uint32_t)n_tiles; T.err = d_err + i;
        }
    }
    emit_train_launch(es, nullptr, J, train == 3);
    MSIM_HIP(c, hipGetLastError());
    for (int i = 0; i < n_jobs; i++) {
        MSIM_HIP(c, hipMemcpyAsync(recs[i], J.j[i].recs, (size_t)cnt[(size_t)i] * sizeof(msim_record), hipMemcpyDeviceToHost, es));
        if (J.j[i].first)
            MSIM_HIP(c, hipMemcpyAsync(first[i], J.j[i].first, ((size_t)J.j[i].n_tiles + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, es));
    }
    MSIM_HIP(c, wait_stream(es));
    return MSIM_OK;
}

// test support (msim_dbg_snp_draws): the SNP transducer's three passes -- k_snp_maps_abs over the whole blocks, k_snp_scan_cut_abs
// from `start`, k_snp_emit_abs into a byte array by rank -- over words the caller made, in buffers of its own, synchronous.
// The window is everything from `start` to the end of the last whole block.  lanes / maps: one guard block beyond the mapped
// ones; aux: aux_off guard bytes, K outcomes, 16 guard bytes (include/msim.h).  The outcome pass runs as k_snp_emit_abs: the
// body the train's k_snp_emit_abs_b / k_snp_emit_count_b share; their job table (emit_job_of, eblk0) runs in the whole-path tests only (tests/test_gpu_emit_train_vs_host.py).
int gpu_dbg_snp_draws(Ctx *c, const uint32_t *words, uint64_t n_words, uint64_t ti_lim, uint64_t start, uint32_t K, uint32_t aux_off,
                      uint32_t *lanes, uint32_t *maps, uint64_t *end_pos, uint32_t *flags, uint8_t *aux) {
    const uint64_t n_blocks = n_words / SNP_BLOCK2;
    if (!words || !lanes || !maps || !end_pos || !flags || !aux || !n_blocks || n_words >= (1ull << 28) || start >= n_blocks * SNP_BLOCK2 ||
        !K || K > n_words || aux_off >= 64)
        return fail(c, MSIM_ERR_ARG, "msim_dbg_snp_draws: bad argument");
    static_assert(sizeof(SnpLane) == 16 && sizeof(SnpMap) == 16, "msim_dbg_snp_draws hands both out as four uint32");
    const uint32_t W = (uint32_t)(n_blocks * SNP_BLOCK2 - start);
    const uint32_t nb = (uint32_t)(n_blocks - start / SNP_BLOCK2);
    const size_t sz_lanes = (size_t)(n_blocks + 1) * SNP_THREADS * sizeof(SnpLane), sz_maps = (size_t)(n_blocks + 1) * sizeof(SnpMap);
    const size_t sz_aux = (size_t)aux_off + K + 16;
    const size_t sz_raw = (size_t)n_words * 4, sz_win = (size_t)(nb + 1) * sizeof(SnpMap);
    DbgDev dev;
    uint32_t *d_raw; SnpLane *d_lanes; SnpMap *d_maps, *d_win; PlanState *d_ps; unsigned long long *d_base; uint8_t *d_aux;
    MSIM_HIP(c, dev.bytes(&d_raw, sz_raw)); MSIM_HIP(c, dev.bytes(&d_lanes, sz_lanes)); MSIM_HIP(c, dev.bytes(&d_maps, sz_maps));
    MSIM_HIP(c, dev.bytes(&d_win, sz_win)); MSIM_HIP(c, dev.bytes(&d_ps, sizeof(PlanState))); MSIM_HIP(c, dev.bytes(&d_base, 64));
    MSIM_HIP(c, dev.bytes(&d_aux, sz_aux));
    hipStream_t st = c->stream;
    PlanState ps;
    memset(&ps, 0, sizeof ps);
    ps.pos = ps.snp_base = start;
    MSIM_HIP(c, hipMemcpyAsync(d_raw, words, sz_raw, hipMemcpyHostToDevice, st));
    MSIM_HIP(c, hipMemcpyAsync(d_ps, &ps, sizeof ps, hipMemcpyHostToDevice, st));
    MSIM_HIP(c, hipMemsetAsync(d_lanes, 0xee, sz_lanes, st));
    MSIM_HIP(c, hipMemsetAsync(d_maps, 0xee, sz_maps, st));
    MSIM_HIP(c, hipMemsetAsync(d_win, 0, sz_win, st));
    MSIM_HIP(c, hipMemsetAsync(d_aux, 0xee, sz_aux, st));
    hipLaunchKernelGGL(k_snp_maps_abs, dim3((uint32_t)n_blocks), dim3(SNP_THREADS), 0, st, d_raw, (uint32_t)n_words,
                       (unsigned long long)ti_lim, 0u, d_maps, d_lanes);
    hipLaunchKernelGGL(k_snp_scan_cut_abs, dim3(1), dim3(SNP_THREADS), 0, st, d_lanes, d_ps, W, d_maps, d_win, nb, K, d_base, ~0ull);
    hipLaunchKernelGGL(k_snp_emit_abs, dim3(nb), dim3(SNP_THREADS), 0, st, d_lanes, d_base, W, d_win, nb,
                       (msim_record *)nullptr, K, (const uint32_t *)nullptr, d_aux + aux_off);
    MSIM_HIP(c, hipGetLastError());
    MSIM_HIP(c, hipMemcpyAsync(lanes, d_lanes, sz_lanes, hipMemcpyDeviceToHost, st));
    MSIM_HIP(c, hipMemcpyAsync(maps, d_maps, sz_maps, hipMemcpyDeviceToHost, st));
    MSIM_HIP(c, hipMemcpyAsync(aux, d_aux, sz_aux, hipMemcpyDeviceToHost, st));
    MSIM_HIP(c, hipMemcpyAsync(&ps, d_ps, sizeof ps, hipMemcpyDeviceToHost, st));
    MSIM_HIP(c, wait_stream(st));
    *end_pos = ps.pos;
    *flags = ps.flags;
    return MSIM_OK;
}

// test support (msim_dbg_sample_tail): one launch of k_sample_tail over tables the caller made, in buffers of its own, synchronous.
// Everything the kernel can index with is checked here first (include/msim.h lists what a caller has to hand in): the window lies
// inside `words`, the list covers every accepted index the rounds can reach, every list entry is a bit of the bitmap.
int gpu_dbg_sample_tail(Ctx *c, const uint32_t *words, uint64_t n_words, const uint32_t *acc, uint64_t n_acc, uint32_t acc_first,
                        const uint32_t *blocks, uint32_t n_blocks, uint32_t raw_counts, uint32_t W, uint32_t shift, uint32_t n,
                        uint32_t k, uint32_t *bitmap, uint32_t bm_guard, msim_dbg_tail_state *state, int anchored, uint64_t win_pos,
                        uint32_t need0, uint32_t d1, uint64_t pos_limit) {
    if (!words || !acc || !blocks || !bitmap || !state || !n_blocks || !W || !n || shift >= 32 || n_words >= (1ull << 31) ||
        n_blocks != (W + ACC_BLOCK - 1) / ACC_BLOCK || (raw_counts && n_blocks > (uint32_t)TAIL_LDS_OFFS) || raw_counts > 1)
        return fail(c, MSIM_ERR_ARG, "msim_dbg_sample_tail: bad argument");
    const uint64_t p0 = anchored ? win_pos : state->pos;
    uint64_t total = 0;
    if (raw_counts) for (uint32_t i = 0; i < n_blocks; i++) total += blocks[i];
    else total = blocks[n_blocks];
    const uint64_t first_pos = (uint64_t)k + (anchored ? need0 : 0u);
    if (p0 > n_words || W > n_words - p0 || total >= (1ull << 32) || acc_first > first_pos || total > (uint64_t)acc_first + n_acc)
        return fail(c, MSIM_ERR_ARG, "msim_dbg_sample_tail: the window or the list does not cover what the kernel may read");
    for (uint64_t i = 0; i < n_acc; i++)
        if (acc[i] >= n) return fail(c, MSIM_ERR_ARG, "msim_dbg_sample_tail: a list entry beyond the population");
    const size_t bm_words = ((size_t)n + 31) / 32, sz_bm = (bm_words + 2 * (size_t)bm_guard) * 4;
    const size_t sz_raw = std::max<size_t>((size_t)n_words * 4, 4), sz_acc = std::max<size_t>((size_t)n_acc * 4, 4);
    const size_t sz_blk = ((size_t)n_blocks + 1) * 4;
    DbgDev dev;
    uint32_t *d_raw, *d_acc, *d_blk, *d_bm; PlanState *d_ps; SpecHdr *d_hdr;
    MSIM_HIP(c, dev.bytes(&d_raw, sz_raw)); MSIM_HIP(c, dev.bytes(&d_acc, sz_acc)); MSIM_HIP(c, dev.bytes(&d_blk, sz_blk));
    MSIM_HIP(c, dev.bytes(&d_bm, sz_bm)); MSIM_HIP(c, dev.bytes(&d_ps, 2 * sizeof(PlanState))); MSIM_HIP(c, dev.bytes(&d_hdr, sizeof(SpecHdr)));
    hipStream_t st = c->stream;
    PlanState ps[2];
    memset(ps, 0, sizeof ps);
    ps[0].pos = state->pos; ps[0].snp_base = state->snp_base; ps[0].flags = state->flags; ps[0].dups = state->dups;
    ps[0].accepted_used = state->accepted_used;
    ps[1].pos = ps[1].snp_base = win_pos;
    SpecHdr hdr{need0, d1, 0, 0};
    MSIM_HIP(c, hipMemcpyAsync(d_raw, words, (size_t)n_words * 4, hipMemcpyHostToDevice, st));
    if (n_acc) MSIM_HIP(c, hipMemcpyAsync(d_acc, acc, (size_t)n_acc * 4, hipMemcpyHostToDevice, st));
    MSIM_HIP(c, hipMemcpyAsync(d_blk, blocks, ((size_t)n_blocks + (raw_counts ? 0 : 1)) * 4, hipMemcpyHostToDevice, st));
    MSIM_HIP(c, hipMemcpyAsync(d_bm, bitmap, sz_bm, hipMemcpyHostToDevice, st));
    MSIM_HIP(c, hipMemcpyAsync(d_ps, ps, sizeof ps, hipMemcpyHostToDevice, st));
    MSIM_HIP(c, hipMemcpyAsync(d_hdr, &hdr, sizeof hdr, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_sample_tail, dim3(1), dim3(TAIL_THREADS), 0, st, d_raw, d_acc, acc_first, d_blk, n_blocks, W, shift, n, k,
                       d_bm + bm_guard, d_ps, raw_counts, anchored ? (const PlanState *)(d_ps + 1) : (const PlanState *)nullptr,
                       anchored ? (const SpecHdr *)d_hdr : (const SpecHdr *)nullptr, (unsigned long long)pos_limit);
    MSIM_HIP(c, hipGetLastError());
    MSIM_HIP(c, hipMemcpyAsync(bitmap, d_bm, sz_bm, hipMemcpyDeviceToHost, st));
    MSIM_HIP(c, hipMemcpyAsync(ps, d_ps, sizeof(PlanState), hipMemcpyDeviceToHost, st));
    MSIM_HIP(c, wait_stream(st));
    state->pos = ps[0].pos; state->snp_base = ps[0].snp_base; state->flags = ps[0].flags; state->dups = ps[0].dups;
    state->accepted_used = ps[0].accepted_used;
    return MSIM_OK;
}

// test support (msim_dbg_chain_step): the chain of one anchored contig -- fringe, tail rounds, stream cut, SNP scan and cut -- over
// tables the caller made, as the ONE launch (k_chain_fused) or as the three stand-alone launches, in buffers of its own,
// synchronous.  The lanes and maps of the SNP stage come from the map pass over the whole blocks of `words`.  Everything the
// kernels can index with is checked first (include/msim.h lists what a caller hands in).
int gpu_dbg_chain_step(Ctx *c, const uint32_t *words, uint64_t n_words, const uint32_t *hcnt, const uint32_t *hacc, uint64_t n_hacc,
                       const uint32_t *tail, uint64_t n_tail, const uint32_t *cnt, uint32_t *bitmap, uint32_t *win_maps,
                       msim_dbg_chain *io) {
    if (!words || !hcnt || !hacc || !tail || !cnt || !bitmap || !win_maps || !io)
        return fail(c, MSIM_ERR_ARG, "msim_dbg_chain_step: bad argument");
    msim_dbg_chain &d = *io;
    const uint64_t n_blocks2 = n_words / SNP_BLOCK2;
    const uint32_t nb = (d.W + ACC_BLOCK - 1) / ACC_BLOCK, nbh = (d.F + ACC_BLOCK - 1) / ACC_BLOCK;
    const uint64_t H = d.lo + d.F;
    if (!n_blocks2 || n_words >= (1ull << 28) || !d.W || !d.n || d.shift >= 32 || !d.G || d.G > 256 || !d.W2 || !d.K2 || d.k_core > d.K ||
        d.K >= (1u << 30) || d.core_dups >= (1u << 30) || nb > (uint32_t)TAIL_LDS_OFFS || nbh > (uint32_t)AHEAD_MAX_HEAD_BLOCKS ||
        d.bm_guard > 4096 || d.fused > 1)
        return fail(c, MSIM_ERR_ARG, "msim_dbg_chain_step: bad argument");
    const uint32_t nb2 = d.W2 / SNP_BLOCK2 + 2;
    // the head interval and the window lie inside the words; wherever the SNP draws may start (the cut, the clamp, the old base),
    // their window's blocks are mapped ones
    if (d.lo > n_words || H > n_words || d.W > n_words - H || d.state.snp_base > H + d.W ||
        (H + d.W) / SNP_BLOCK2 + nb2 > n_blocks2 || d.K2 > n_words)
        return fail(c, MSIM_ERR_ARG, "msim_dbg_chain_step: the head interval, the window or the SNP window does not lie inside the words");
    // the head counts are what the words say (the fringe pass subtracts what it counts itself from them), the head list has a
    // segment per block, the tail list covers whatever index the fringe and the rounds can reach
    if (n_hacc < (uint64_t)nbh * ACC_BLOCK) return fail(c, MSIM_ERR_ARG, "msim_dbg_chain_step: head list shorter than its blocks' segments");
    for (uint32_t b = 0; b < nbh; b++) {
        uint32_t n_acc = 0;
        for (uint32_t i = b * ACC_BLOCK; i < std::min<uint32_t>(d.F, (b + 1) * ACC_BLOCK); i++) n_acc += (mt_temper(words[d.lo + i]) >> d.shift) < d.n;
        if (hcnt[b] != n_acc) return fail(c, MSIM_ERR_ARG, "msim_dbg_chain_step: a head count that is not the words' count");
    }
    uint64_t total = 0;
    for (uint32_t i = 0; i < nb; i++) total += cnt[i];
    const uint64_t items = (uint64_t)d.K - d.k_core + d.core_dups;
    if (total >= (1ull << 31) || n_tail < items || (total > d.k_core && n_tail < total - d.k_core))
        return fail(c, MSIM_ERR_ARG, "msim_dbg_chain_step: the tail list does not cover what the kernels may read");
    for (uint64_t i = 0; i < n_tail; i++)
        if (tail[i] >= d.n) return fail(c, MSIM_ERR_ARG, "msim_dbg_chain_step: a list entry beyond the population");
    static_assert(sizeof(SnpLane) == 16 && sizeof(SnpMap) == 16 && sizeof(SpecHdr) == 16, "msim_dbg_chain_step hands them out as four uint32");
    const size_t bm_words = ((size_t)d.n + 31) / 32, sz_bm = (bm_words + 2 * (size_t)d.bm_guard) * 4;
    const size_t sz_raw = (size_t)n_words * 4, sz_lanes = (size_t)n_blocks2 * SNP_THREADS * sizeof(SnpLane), sz_maps = (size_t)n_blocks2 * sizeof(SnpMap);
    const size_t sz_win = (size_t)(nb2 + 2) * sizeof(SnpMap);                 // nb2 blocks, the totals entry, one guard entry
    const size_t sz_hcnt = ((size_t)nbh + 2) * 4, sz_hacc = std::max<size_t>((size_t)n_hacc * 4, 4) + 256, sz_tail = std::max<size_t>((size_t)n_tail * 4, 4);
    const size_t sz_cnt = ((size_t)nb + 2) * 4;
    DbgDev dev;
    uint32_t *d_raw, *d_hcnt, *d_hacc, *d_tail, *d_cnt, *d_bm; SnpLane *d_lanes; SnpMap *d_maps, *d_win; PlanState *d_ps; SpecHdr *d_hdr;
    unsigned long long *d_base;
    MSIM_HIP(c, dev.bytes(&d_raw, sz_raw)); MSIM_HIP(c, dev.bytes(&d_hcnt, sz_hcnt)); MSIM_HIP(c, dev.bytes(&d_hacc, sz_hacc));
    MSIM_HIP(c, dev.bytes(&d_tail, sz_tail)); MSIM_HIP(c, dev.bytes(&d_cnt, sz_cnt)); MSIM_HIP(c, dev.bytes(&d_bm, sz_bm));
    MSIM_HIP(c, dev.bytes(&d_lanes, sz_lanes)); MSIM_HIP(c, dev.bytes(&d_maps, sz_maps)); MSIM_HIP(c, dev.bytes(&d_win, sz_win));
    MSIM_HIP(c, dev.bytes(&d_ps, 3 * sizeof(PlanState))); MSIM_HIP(c, dev.bytes(&d_hdr, sizeof(SpecHdr))); MSIM_HIP(c, dev.bytes(&d_base, 64));
    hipStream_t st = c->stream;
    PlanState ps[3];                                       // the chain's, the core window's, the head interval's
    memset(ps, 0, sizeof ps);
    ps[0].pos = d.state.pos; ps[0].snp_base = d.state.snp_base; ps[0].flags = d.state.flags; ps[0].dups = d.state.dups;
    ps[0].accepted_used = d.state.accepted_used; ps[0].ahead_margin_used = d.state.rsv;
    ps[1].pos = ps[1].snp_base = H; ps[1].dups = d.core_dups; ps[1].flags = d.core_flags;
    ps[2].pos = ps[2].snp_base = d.lo; ps[2].flags = d.head_flags;
    const SpecHdr hdr{0, 0, 0, 0};                         // (as the prep's count body leaves it)
    MSIM_HIP(c, hipMemcpyAsync(d_raw, words, sz_raw, hipMemcpyHostToDevice, st));
    if (nbh) MSIM_HIP(c, hipMemcpyAsync(d_hcnt, hcnt, (size_t)nbh * 4, hipMemcpyHostToDevice, st));
    if (n_hacc) MSIM_HIP(c, hipMemcpyAsync(d_hacc, hacc, (size_t)n_hacc * 4, hipMemcpyHostToDevice, st));
    if (n_tail) MSIM_HIP(c, hipMemcpyAsync(d_tail, tail, (size_t)n_tail * 4, hipMemcpyHostToDevice, st));
    MSIM_HIP(c, hipMemsetAsync(d_cnt, 0, sz_cnt, st));
    MSIM_HIP(c, hipMemcpyAsync(d_cnt, cnt, (size_t)nb * 4, hipMemcpyHostToDevice, st));
    MSIM_HIP(c, hipMemcpyAsync(d_bm, bitmap, sz_bm, hipMemcpyHostToDevice, st));
    MSIM_HIP(c, hipMemcpyAsync(d_ps, ps, sizeof ps, hipMemcpyHostToDevice, st));
    MSIM_HIP(c, hipMemcpyAsync(d_hdr, &hdr, sizeof hdr, hipMemcpyHostToDevice, st));
    MSIM_HIP(c, hipMemsetAsync(d_win, 0xee, sz_win, st));
    MSIM_HIP(c, hipMemsetAsync(d_base, 0xee, 64, st));
    hipLaunchKernelGGL(k_snp_maps_abs, dim3((uint32_t)n_blocks2), dim3(SNP_THREADS), 0, st, d_raw, (uint32_t)n_words,
                       (unsigned long long)d.ti_lim, 0u, d_maps, d_lanes);
    if (d.fused) {
        ChainJob J{};
        J.raw = d_raw; J.ps = d_ps; J.ps_core = d_ps + 1; J.ps_head = d_ps + 2; J.hdr = d_hdr;
        J.hcnt = d_hcnt; J.hacc = d_hacc; J.acc = d_tail; J.bitmap = d_bm + d.bm_guard;
        J.lo = d.lo; J.expect = d.expect;
        J.F = d.F; J.nbh = nbh; J.K = d.K; J.k_core = d.k_core; J.shift = d.shift; J.n = d.n; J.soft_half = d.soft_half;
        J.cnt = d_cnt; J.nb = nb; J.W = d.W; J.pos_limit = d.pos_limit;
        J.lanes = d_lanes; J.abs_maps = d_maps; J.win_maps = d_win; J.base_out = d_base;
        J.snp_limit = d.snp_limit; J.W2 = d.W2; J.nb2 = nb2; J.K2 = d.K2;
        hipLaunchKernelGGL(k_chain_fused, dim3(d.G), dim3(ACC_THREADS), 0, st, J);
    } else {
        hipLaunchKernelGGL(k_ahead_fringe, dim3(d.G), dim3(ACC_THREADS), 0, st, d_raw, d_ps, d_ps + 1, d_ps + 2, d_hdr, (unsigned long long)d.lo,
                           d.F, d_hcnt, nbh, d_hacc, d_tail, d.K, d.k_core, d.shift, d.n, d_bm + d.bm_guard, (unsigned long long)d.expect,
                           d.soft_half);
        hipLaunchKernelGGL(k_sample_tail, dim3(1), dim3(TAIL_THREADS), 0, st, d_raw, d_tail, d.k_core, d_cnt, nb, d.W, d.shift, d.n, d.k_core,
                           d_bm + d.bm_guard, d_ps, 1u, (const PlanState *)(d_ps + 1), (const SpecHdr *)d_hdr, (unsigned long long)d.pos_limit);
        hipLaunchKernelGGL(k_snp_scan_cut_abs, dim3(1), dim3(SNP_THREADS), 0, st, d_lanes, d_ps, d.W2, d_maps, d_win, nb2, d.K2, d_base,
                           (unsigned long long)d.snp_limit);
    }
    MSIM_HIP(c, hipGetLastError());
    MSIM_HIP(c, hipMemcpyAsync(bitmap, d_bm, sz_bm, hipMemcpyDeviceToHost, st));
    MSIM_HIP(c, hipMemcpyAsync(win_maps, d_win, sz_win, hipMemcpyDeviceToHost, st));
    MSIM_HIP(c, hipMemcpyAsync(ps, d_ps, sizeof(PlanState), hipMemcpyDeviceToHost, st));
    MSIM_HIP(c, hipMemcpyAsync(d.hdr, d_hdr, sizeof(SpecHdr), hipMemcpyDeviceToHost, st));
    MSIM_HIP(c, hipMemcpyAsync(&d.base, d_base, 8, hipMemcpyDeviceToHost, st));
    MSIM_HIP(c, wait_stream(st));
    d.state.pos = ps[0].pos; d.state.snp_base = ps[0].snp_base; d.state.flags = ps[0].flags; d.state.dups = ps[0].dups;
    d.state.accepted_used = ps[0].accepted_used; d.state.rsv = ps[0].ahead_margin_used;
    return MSIM_OK;
}
uint64_t gpu_plan_chains_fused(const GpuPlan *g) { return g ? g->chains_fused : 0; }

bool gpu_emit_pending(Ctx *c, int contig, bool mark_apply) {
    GpuPlan *g = c->gpu;
    if (!g) return false;
    for (EmitItem &it : g->emit_items)
        if (it.contig == contig) { if (mark_apply) it.apply = true; return true; }
    return false;
}

StreamMoments sample_words_moments(uint64_t n, uint64_t k) {
    const double n_d = (double)n, k_d = (double)k;
    const double p_acc = n_d / (double)(1ull << bit_length64(n));
    const double l1p = std::log1p(-k_d / n_d);
    const double EA = -n_d * l1p, VA = std::max(0.0, n_d * (k_d / (n_d - k_d) + l1p));
    return StreamMoments{EA / p_acc, EA * (1.0 - p_acc) / (p_acc * p_acc) + VA / (p_acc * p_acc)};
}
StreamMoments snp_words_moments(uint64_t K, unsigned long long ti_lim) {
    const double p_tv = 1.0 - std::min(1.0, (double)ti_lim / 9007199254740992.0);
    return StreamMoments{(double)K * (2.0 + 2.0 * p_tv), (double)K * (2.0 * p_tv + 4.0 * p_tv * (1.0 - p_tv))};
}

// ---- part (a) of a contig's plan: the host's arithmetic, nothing launched.  plan_contig_gpu runs these steps at the contig's
// turn; msim_plan_pass runs them over the contigs to come (pass_segment), on a copy of the estimate, to send their samples'
// off-chain parts ahead -- the same functions, so both arrive at the same windows.
static bool no_aux_fold() { static const bool v = getenv("MSIM_NO_AUX_FOLD") != nullptr; return v; }
// one drawing range and a record table to write: the contig's emission goes out with a group (gpu_emit_flush)
static bool contig_is_grouped(int n_draw, bool chain_only) {
    static const bool no_group = getenv("MSIM_NO_EMIT_GROUP") != nullptr;
    return n_draw == 1 && !chain_only && !no_aux_fold() && !no_group;
}
// One sampled range: its window, whether its heavy part leaves the chain, and est / pos_hi (the bound of the device position)
// behind it.  can_ahead: the context plans ahead and the contig's shape allows it.
static SampleStep sample_step(double ahead_sigma, ChainEst &est, uint64_t &pos_hi, const msim_range &r, int64_t d, bool can_ahead) {
    SampleStep st;
    const uint32_t k = (uint32_t)r.k;
    // moments of the words this sample consumes: A accepted draws until k distinct values (duplicates: a coupon collector's
    // first k), each after a geometric number of rejected words (_randbelow)
    const double n_d = (double)range_population(r, d);
    const StreamMoments ms = sample_words_moments((uint64_t)n_d, (uint64_t)k);
    const double wd = big_sample_window(n_d, set_path_need(n_d, (double)k));
    if (wd >= 4.0e9) { st.bad = true; return st; }
    st.W = (uint32_t)wd;
    if (can_ahead && est.ok && (uint64_t)n_d <= ((uint64_t)MAX_BINS << BIN_SHIFT) && 4.0 * (double)k <= n_d) {
        // the interval costs what it holds (its accepted draws go through the fringe pass on the chain): ahead_sigma
        // (8) standard deviations instead of the windows' 16 -- a start outside it is reported like an overflowed window
        const double m = est.v > 0.0 ? ahead_sigma * std::sqrt(1.1 * est.v) + 256.0 : 0.0;
        st.expect = (uint64_t)std::max(0.0, est.e);
        st.soft_half = (uint32_t)std::min(4.0e9, m);
        st.lo = std::max<uint64_t>(est.lo, (uint64_t)std::max(0.0, std::floor(est.e - m)));
        st.H = std::max<uint64_t>(st.lo, std::min<uint64_t>(pos_hi, (uint64_t)std::ceil(est.e + m)));
        // (a sample smaller than the uncertainty of its start stays on the chain; so does one whose start is known exactly --
        //  behind a synchronisation the chain is empty and nothing is gained by making it wait for the prep stream)
        static const bool ahead_first = getenv("MSIM_AHEAD_FIRST") != nullptr;
        st.ahead = 2 * (st.H - st.lo) <= (uint64_t)k && (est.v > 0.0 || ahead_first) && ahead_geometry(r, d, st.lo, st.H, st.W).took;
    }
    est.add(ms, k);
    // the sample ends at or in front of e_lim (and inside its window): what the SNP stage's windows are laid out from
    st.e_lim = est.hi(~0ull);
    if (st.ahead) pos_hi = std::min<uint64_t>(st.H + st.W, st.e_lim) - st.W;
    st.pos_in = pos_hi;
    pos_hi += st.W;
    if (!st.ahead) pos_hi = est.hi(pos_hi);
    return st;
}
// The SNP draws of a contig's K SNPs: a uniform() = 2 words, a transversion's randbelow(2) = a geometric(1/2) loop.
static SnpStep snp_step(ChainEst &est, uint64_t &pos_hi, uint64_t K, const msim_params &P) {
    SnpStep sn;
    est.add(snp_words_moments(K, P.ti_lim), 2 * K);
    sn.e_lim = est.hi(~0ull);
    sn.pos_in = pos_hi;
    const double p_tv = 1.0 - std::min(1.0, (double)P.ti_lim / 9007199254740992.0);
    const double w2 = (double)K * (2.0 + 2.0 * p_tv) + 16.0 * std::sqrt(4.0 * (double)K) + 16384.0;
    if (w2 >= 4.0e9) { sn.bad = true; return sn; }
    sn.W2 = (uint32_t)w2;
    pos_hi += sn.W2;
    pos_hi = est.hi(pos_hi);
    return sn;
}

// Asynchronous: enqueues the contig's chain (stream positions) on the plan stream and its emit work
// (records) on the emit stream; nothing is waited for.  Flags and the exact position are collected
// by gpu_plan_finish at the next synchronising call.
int plan_contig_gpu(Ctx *c, GpuPlan *g, Contig &ct, const msim_range *ranges, int n_ranges) {
    const msim_params &P = c->params;
    const int64_t d = min_block(P);
    int rc;
    if ((rc = session_open(c, g))) return rc;
    uint64_t K = 0;
    for (int i = 0; i < n_ranges; i++) K += (uint64_t)ranges[i].k;
    if (K >= (1ull << 31)) return fail(c, MSIM_ERR_UNSUPPORTED, "more than 2^31 mutations on one contig");
    Grow grow{c};
    if (!c->chain_only) {   // the record table may still be read by an earlier apply of this contig
        const size_t want = std::max<uint64_t>(K, 1) * sizeof(msim_record);
        if (ct.d_recs.cap < want || ct.d_pool.cap < 2 * PAD) {
            MSIM_HIP(c, wait_stream(c->stream));
            MSIM_HIP(c, wait_stream(c->emit_stream));
        }
        if ((rc = dev_reserve(c, ct.d_recs, want))) return rc;
        if ((rc = dev_reserve(c, ct.d_pool, 2 * PAD))) return rc;
    }
    ct.n_rec = K;
    ct.pool_len = 0;
    ct.plan_empty = K == 0;
    ct.all_snp = true;                                    // every record is an SNP: output offset == position

    GpuStream &py = g->s[0];
    if ((rc = chain_open(c, g, true))) return rc;
    uint64_t pos_hi = py.pos;                             // upper bound of the device position
    uint64_t rec_base = 0;
    if (c->chain_only) { g->pass_chain_only++; g->sharded_rank = true; }
    if (!g->unverified) g->est = ChainEst{true, (double)py.pos, 0.0, py.pos};   // py.pos is exact: the estimate of the position starts here
    // One drawing range (ARGS mode): the SNP outcomes are folded into the records by the expansion, which then runs behind
    // the SNP stage.  Several ranges keep the order expansion -> outcomes patched in (their bitmaps rotate through N_SETS
    // scratch sets and cannot all wait for the contig's one SNP stage).
    int n_draw = 0;
    for (int i = 0; i < n_ranges; i++) n_draw += ranges[i].k != 0;
    const bool fold_aux = n_draw == 1 && !c->chain_only && !no_aux_fold();
    // ... and such contigs go through the emission stages in groups of EMIT_G (gpu_emit_flush), one launch per stage
    const bool grouped = contig_is_grouped(n_draw, c->chain_only);
    // A full group goes out when the NEXT contig is planned, in front of its chain: by then msim_apply_contig has marked the
    // group's last contig too, so all of its APPLYs share the group's tile-index launch.
    // (pairs.  Measured with the calling thread on the GPU's NUMA node, where runs repeat within 0.05 ms: pairs 4.10-4.21 ms per
    //  c2 step with the rewrite launches at 0.72-0.74 of the HBM peak, threes 4.22-4.31 at 0.75-0.77, fours 4.29-4.32 at 0.78,
    //  sixes 4.36-4.38 at 0.79 -- a larger group is a better rewrite launch and a longer stretch in which the chain's kernels
    //  crawl beside it, plus more left to do behind the last chain; groups cut by their bases instead of their count, 250-400 Mb
    //  with at most 4-6 contigs, were no better than threes; one per group = the ungrouped 4.6-5.1)
    // (round 6: with the samples' heavy kernels off the chain -- anchored windows, now every context's default -- the train is the
    //  bound and larger groups pay: fours 3.67-3.70 ms, threes 3.69-3.82, pairs 3.76-3.81 on a box where pairs with every sample
    //  on the chain take 3.90-4.00; profiles/r06_emission_train.txt)
    const bool ahead_role = g->ahead == 2 || (g->ahead == 1 && g->sharded_rank);
    const int group = g->emit_group ? g->emit_group : (ahead_role ? 4 : 2);
    if (!g->emit_items.empty() && (!grouped || g->emit_d != (uint32_t)d || g->emit_items.size() >= (size_t)group))
        if ((rc = gpu_emit_flush(c))) return rc;
    struct { SampleSet *S; uint32_t bmw, bnb, start; } late = {nullptr, 0, 0, 0};
    g->held.on = false;
    for (int i = 0; i < n_ranges; i++) {
        const msim_range &r = ranges[i];
        if (r.k == 0) continue;
        const uint32_t k = (uint32_t)r.k;
        SampleLaunch sl;
        const bool can_ahead = ahead_role && (grouped || (c->chain_only && n_draw == 1));
        const SampleStep st = sample_step(g->ahead_sigma, g->est, pos_hi, r, d, can_ahead);
        if (st.bad) return fail(c, MSIM_ERR_UNSUPPORTED, "sample window beyond 2^32 words");
        const bool ahead = st.ahead;
        // (an anchored window implies one drawing range: the whole chain of the contig is then one launch, sent by the SNP stage)
        if (ahead && (rc = enqueue_sample_ahead(c, g, r, d, st, grow, sl, grouped, g->chain_fuse && n_draw == 1))) return rc;
        if (!ahead && (rc = enqueue_sample_chain(c, g, r, d, st.pos_in, grow, sl, nullptr, nullptr, st.e_lim))) return rc;
        SampleSet &S = *sl.S;
        const uint32_t bmw = sl.bmw, bnb = sl.bnb;
        if (grouped) {
            late = {&S, bmw, bnb, (uint32_t)r.start};
        } else if (!c->chain_only) {
            // (a held launch belongs to a grouped or walked contig: this event would be recorded in front of the sample's kernels)
            if (g->held.on) return fail(c, MSIM_ERR_HIP, "GPU sampler: a held chain launch in front of an ungrouped emission");
            hipEvent_t ce = next_chain_event(g);
            MSIM_HIP(c, hipEventRecord(ce, c->stream));
            // ---- emit (emit stream): the bitmap is the sorted sample -> records
            MSIM_HIP(c, hipStreamWaitEvent(c->emit_stream, ce, 0));
            hipLaunchKernelGGL(k_bitmap_count, dim3(bnb), dim3(BM_THREADS), 0, c->emit_stream,
                               reinterpret_cast<const uint64_t *>(S.bitmap.p()), bmw, S.cnt2.p());
            hipLaunchKernelGGL(k_scan_u32_w4, dim3(1), dim3(256), 0, c->emit_stream, S.cnt2.p(), bnb);
            if (fold_aux) {                               // the expansion follows the SNP stage (below): it writes complete records
                late = {&S, bmw, bnb, (uint32_t)r.start};
            } else {
                hipLaunchKernelGGL(k_bitmap_expand, dim3(bnb), dim3(BM_THREADS), 0, c->emit_stream,
                                   reinterpret_cast<const uint64_t *>(S.bitmap.p()), bmw, S.cnt2.p(), (uint32_t)r.start, (uint32_t)d,
                                   ct.d_recs.p() + rec_base, (const uint8_t *)nullptr);
                MSIM_HIP(c, hipGetLastError());
                MSIM_HIP(c, hipEventRecord(S.emit_done, c->emit_stream));
                S.wait_ev = S.emit_done;
                S.pending = true;
            }
        }
        rec_base += k;
    }
    if (!K && g->held.on) return fail(c, MSIM_ERR_HIP, "GPU sampler: a held chain launch and no SNP stage to send it");
    if (K) {                                          // SNP draws in position order (chain: scan + cut; aux off the chain)
        uint8_t *aux8 = nullptr;
        SnpDefer df{nullptr, 0, 0};
        // (e_lim: the bound the position is tightened to behind this stage -- the kernel flags a cut beyond it)
        const SnpStep sn = snp_step(g->est, pos_hi, K, P);
        uint64_t snp_pos = sn.pos_in;
        if ((rc = enqueue_snp_stage(c, g, ct, K, nullptr, snp_pos, grow, late.S ? &aux8 : nullptr, grouped ? &df : nullptr, sn.e_lim, true))) return rc;
        if (grouped) {
            g->emit_d = (uint32_t)d;
            g->emit_items.push_back(EmitItem{ct.index, late.S, df.T, late.bmw, late.bnb, late.start, (uint32_t)K, df.W2, df.nb2,
                                             ct.d_recs.p(), false});
            if (g->emit_items.size() >= (size_t)EMIT_G && (rc = gpu_emit_flush(c))) return rc;   // (the launch's job table is full)
        } else if (late.S) {
            SampleSet &S = *late.S;
            SnpSet &T = g->snp[(g->snp_unit - 1) % N_SETS];        // (the set enqueue_snp_stage just took)
            hipLaunchKernelGGL(k_bitmap_expand, dim3(late.bnb), dim3(BM_THREADS), 0, c->emit_stream,
                               reinterpret_cast<const uint64_t *>(S.bitmap.p()), late.bmw, S.cnt2.p(), late.start, (uint32_t)d,
                               ct.d_recs.p(), (const uint8_t *)aux8);
            MSIM_HIP(c, hipGetLastError());
            MSIM_HIP(c, hipEventRecord(S.emit_done, c->emit_stream));
            S.wait_ev = S.emit_done;
            S.pending = true;
            MSIM_HIP(c, hipEventRecord(T.emit_done, c->emit_stream));
            T.wait_ev = T.emit_done;
            T.pending = true;
        }
    }
    py.pos = pos_hi;                                       // bound until gpu_plan_finish reads the exact value
    g->s[1].pos += 2 * K;                                  // numpy.random.choice(size=k): 2 words per candidate
    c->t.np_words += 2 * K;
    g->unverified = true;
    ct.planned = true;
    return MSIM_OK;
}

// ---- msim_plan_pass: the samples' off-chain parts of a whole segment of contigs, ahead of their chains.
// Where the pass stands as the host knows it: what plan_contig_gpu reads of the plan's state before it launches anything.
struct PassCursor { ChainEst est; uint64_t py_pos, np_pos; bool unverified, live, sharded_rank; };
struct PassRules { int ahead; double ahead_sigma; uint64_t span_w; int max_sets; };
struct PassStep { SampleStep st; const msim_range *r; bool chain_only; };
// One item that the SNP sampler takes, walked on the cursor as plan_contig_gpu walks it on the plan.  Returns false (cursor
// untouched) where the sampler would not get it as it stands: another engine's, a re-base in front of it, no room at all.
// *hoist: exactly one drawing range, and its sample is an anchored window (out->st: laid out how).
static bool pass_walk_item(const msim_params &P, const PassRules &R, PassCursor &cur, const msim_pass_item &it, bool *hoist, PassStep *out) {
    *hoist = false;
    const bool chain_only = it.contig < 0;
    if (it.n_ranges < 0 || (it.n_ranges && !it.ranges) || (chain_only && it.len >= (1ull << 32))) return false;
    if (!sampler_eligible(P, it.ranges, it.n_ranges)) return false;
    const RoomVerdict room = room_for(stream_need(P, it.ranges, it.n_ranges), R.span_w, cur.live, cur.py_pos, cur.live, cur.np_pos);
    if (!room.fits || room.rebase) return false;
    uint64_t K = 0;
    int n_draw = 0;
    for (int i = 0; i < it.n_ranges; i++) { K += (uint64_t)it.ranges[i].k; n_draw += it.ranges[i].k != 0; }
    if (K >= (1ull << 31)) return false;
    const int64_t d = min_block(P);
    PassCursor w = cur;
    w.sharded_rank = cur.sharded_rank || chain_only;
    if (!w.unverified) w.est = ChainEst{true, (double)w.py_pos, 0.0, w.py_pos};
    const bool ahead_role = R.ahead == 2 || (R.ahead == 1 && w.sharded_rank);
    const bool can_ahead = ahead_role && (contig_is_grouped(n_draw, chain_only) || (chain_only && n_draw == 1));
    uint64_t pos_hi = w.py_pos;
    bool any_ahead = false;
    for (int i = 0; i < it.n_ranges; i++) {
        if (it.ranges[i].k == 0) continue;
        const SampleStep st = sample_step(R.ahead_sigma, w.est, pos_hi, it.ranges[i], d, can_ahead);
        if (st.bad) return false;
        if (st.ahead) { any_ahead = true; if (out) *out = PassStep{st, &it.ranges[i], chain_only}; }
    }
    if (K && snp_step(w.est, pos_hi, K, P).bad) return false;
    w.py_pos = pos_hi;
    w.np_pos += 2 * K;
    w.unverified = true;
    *hoist = w.live && n_draw == 1 && any_ahead;
    cur = w;
    return true;
}
// THE SEGMENTING RULE: how many of items[0 .. n) form a segment whose prep goes out in front of the first one's chain -- the
// leading items the SNP sampler takes with one anchored window each, up to the first one that is another engine's or stays on the
// chain (it changes the estimate as it always did: at its own turn), that would re-base the session (judged on the bound of
// the position the items before it leave), or that would need a scratch set too many (R.max_sets: a set whose previous user
// has not been through its emission group yet is never handed out).  The cursor ends behind the segment.
static int pass_segment(const msim_params &P, const PassRules &R, PassCursor &cur, const msim_pass_item *items, int n, std::vector<PassStep> *steps) {
    int m = 0;
    while (m < n && m < R.max_sets) {
        PassCursor w = cur;
        PassStep ps{};
        bool hoist = false;
        if (!pass_walk_item(P, R, w, items[m], &hoist, &ps) || !hoist) break;
        cur = w;
        if (steps) steps->push_back(ps);
        m++;
    }
    return m;
}
// N_SETS sets in turn; the EMIT_G contigs planned last may still wait for their emission group, which is what marks their sets
// as in use (SampleSet::wait_ev) -- so a segment takes at most N_SETS - EMIT_G sets in front of its first chain.
constexpr int PASS_MAX_SETS = N_SETS - EMIT_G;

int gpu_plan_pass_prep(Ctx *c, GpuPlan *g, const msim_pass_item *items, int n) {
    if (!g->pass_hoist || !g->hoisted.empty() || n < 1) return MSIM_OK;
    const PassRules R{g->ahead, g->ahead_sigma, span_words(g), PASS_MAX_SETS};
    PassCursor cur{g->est, g->s[0].pos, g->s[1].pos, g->unverified, g->s[0].live && g->s[1].live && g->ps_valid, g->sharded_rank};
    std::vector<PassStep> steps;
    const int m = pass_segment(c->params, R, cur, items, n, &steps);
    if (m < 1) return MSIM_OK;
    int rc;
    const int64_t d = min_block(c->params);
    uint64_t upto = 0;
    for (const PassStep &ps : steps) upto = std::max<uint64_t>(upto, ps.st.H + ps.st.W + 1);
    if ((rc = ensure_words(c, g, 0, upto, false, false))) return rc;      // (generated on the side streams; the chain waits at its turn)
    for (int at = 0; at < m;) {
        const int nj = std::min(m - at, at == 0 ? g->pass_first : g->pass_batch);
        if ((rc = next_prep_stream(c, g, g->pass_streams))) return rc;
        AheadGeom geo[PREP_G];
        SampleSet *sets[PREP_G];
        uint64_t b_upto = 0;
        for (int q = 0; q < nj; q++) {
            const PassStep &ps = steps[(size_t)(at + q)];
            geo[q] = ahead_geometry(*ps.r, d, ps.st.lo, ps.st.H, ps.st.W);
            Grow grow{c};
            if ((rc = ahead_take_set(c, g, geo[q], grow, contig_is_grouped(1, ps.chain_only), sets[q]))) return rc;
            b_upto = std::max<uint64_t>(b_upto, ps.st.H + ps.st.W + 1);
        }
        if ((rc = prep_wait_words(c, g, b_upto, g->pass_gate))) return rc;
        PrepJobs J;
        J.n = (uint32_t)nj;
        for (int q = 0; q < nj; q++) J.j[q] = prep_job(*sets[q], geo[q], steps[(size_t)(at + q)].st.lo, steps[(size_t)(at + q)].st.H);
        if ((rc = prep_launch(c, g, J, sets[0]->prep_done))) return rc;     // ONE event per batch: its first set's
        for (int q = 0; q < nj; q++) {
            const PassStep &ps = steps[(size_t)(at + q)];
            g->hoisted.push_back(Hoisted{ps.st, ps.r->start, ps.r->k, sets[q], sets[0]->prep_done, q == 0});
        }
        at += nj;
    }
    return MSIM_OK;
}
// A pass ended in the middle of a segment (an error at some contig's turn): the prep of the contigs behind it is in flight on sets
// nobody will chain on -- wait for it, so that the sets' next users find them idle.
void gpu_plan_pass_abort(Ctx *c, GpuPlan *g) {
    if (g->hoisted.empty()) return;
    g->hoisted.clear();
    for (auto st : g->prep_streams) if (st) (void)wait_stream(st);
    (void)c;
}
bool gpu_plan_pass_hoisting(const GpuPlan *g) { return !g->hoisted.empty(); }

// test support (msim_dbg_pass_segments): pass_segment over a whole item list, from streams that stand exactly at py_pos / np_pos.
// seg[i]: 0 = the item takes the per-contig path, s >= 1 = it is in the pass's s-th segment.  An item of another engine is stepped
// over by the bound of its windows, with the estimate dropped (the engines with a host chain leave an exact position behind).
int gpu_dbg_pass_segments(const msim_params *P, const msim_pass_item *items, int n, uint64_t py_pos, uint64_t np_pos,
                          uint32_t max_chunks, int ahead, int32_t *seg) {
    const uint64_t span_w = (uint64_t)MT_N + (uint64_t)(max_chunks ? std::min<uint32_t>(MT_JUMP_MAX_CHUNKS, std::max<uint32_t>(2, max_chunks)) : (uint32_t)MT_JUMP_MAX_CHUNKS) * MT_CHUNK_WORDS;
    const PassRules R{ahead, 8.0, span_w, PASS_MAX_SETS};
    PassCursor cur{ChainEst{}, py_pos, np_pos, false, true, false};
    int32_t id = 0;
    for (int i = 0; i < n;) {
        const int m = pass_segment(*P, R, cur, items + i, n - i, nullptr);
        if (m) {
            id++;
            for (int q = 0; q < m; q++) seg[i + q] = id;
            i += m;
            continue;
        }
        bool hoist = false;
        if (!pass_walk_item(*P, R, cur, items[i], &hoist, nullptr)) {
            // a re-base, or an item the sampler does not take: either way a synchronisation, an exact position behind it
            cur.unverified = false;
            cur.est.ok = false;
            const bool ok_args = items[i].n_ranges >= 0 && (!items[i].n_ranges || items[i].ranges);
            const StreamNeed need = ok_args ? stream_need(*P, items[i].ranges, items[i].n_ranges) : StreamNeed{0, 0, true};
            if (ok_args && room_for(need, span_w, true, cur.py_pos, true, cur.np_pos).rebase) cur.py_pos = cur.np_pos = MT_N;
            if (!pass_walk_item(*P, R, cur, items[i], &hoist, nullptr) && !need.bad && std::isfinite(need.py)) {
                cur.py_pos += (uint64_t)need.py;           // (another engine's: stepped over by the bound of its windows)
                cur.np_pos += (uint64_t)need.np;
            }
        }
        seg[i++] = 0;
    }
    return MSIM_OK;
}

// ====================================================================== SV mixes (section 6 kernels)
static bool range_draws_translocations(const msim_range &r) {
    for (int j = 0; j < r.n_types; j++)
        if ((r.types[j] == MSIM_TL || r.types[j] == MSIM_TLI) && type_drawable(r, j)) return true;
    return false;
}

// SV mix on one large set-path range (ARGS mode: one range per contig): SNPs plus any of IN/DE/DU/IV/TL/TLI.
bool gpu_plan_mixed_eligible(const Ctx *c, const msim_range *ranges, int n_ranges) {
    const msim_params &P = c->params;
    const int64_t d = min_block(P);
    if (P.block[MSIM_SN] != d) return false;              // an SNP could block its successor: the chain needs all candidates
    const msim_range *one = nullptr;
    for (int i = 0; i < n_ranges; i++) {
        if (ranges[i].k == 0) continue;
        if (one) return false;                            // several drawing ranges: host planner
        one = &ranges[i];
    }
    if (!one) return false;
    const msim_range &r = *one;
    if (r.k < 4096 || r.k >= (1ll << 31)) return false;
    const int64_t n = range_population(r, d);
    if (n < r.k || n <= r.setsize || n >= (1ll << 32)) return false;
    if (r.start < 0 || r.stop >= (1ll << 32)) return false;
    if (r.n_types < 1 || r.n_types > 8) return false;
    for (int j = 0; j < r.n_types; j++) {
        if (!type_drawable(r, j)) continue;
        const int t = r.types[j];
        if (t == MSIM_SN) continue;
        if (t == MSIM_TLI) continue;                      // an insertion site: no length draw
        if (t != MSIM_IN && t != MSIM_DE && t != MSIM_DU && t != MSIM_IV && t != MSIM_TL) return false;
        const int64_t w = r.max_len[t] - r.min_len[t] + 1;
        if (r.min_len[t] < 1 || w < 1 || w >= (1ll << 32)) return false;
        if (t == MSIM_IN && (double)r.k * (double)r.max_len[t] >= 4.0e9) return false;     // insert pool offsets are 32-bit
    }
    for (int t = 1; t <= 7; t++)
        if (P.block[t] >= (1ll << 32)) return false;
    if (range_draws_translocations(r)) {                  // their walk exists over accept tables only (ChainWalk::run_tl)
        ChainClasses cc;
        if (!chain_classes(r, cc)) return false;
    }
    return true;
}

static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#endif
}

// Wait for a word in pinned host memory that a kernel on `s` raises to `want`.  The stream is queried now and then so
// that a failed launch or a device fault ends the wait with an error instead of a hang; a stream that neither drains nor
// raises the word ends it at the deadline of every host wait (ctx.h: MSIM_WAIT_TIMEOUT_S).
static int spin_until(Ctx *c, const uint32_t *word, uint32_t want, hipStream_t s) {
    std::chrono::steady_clock::time_point t0{};
    double limit = -1;
    for (uint64_t it = 1;; it++) {
        if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == want) return MSIM_OK;
        cpu_relax();
        if ((it & 0x3ffff) == 0) {
            const hipError_t e = hipStreamQuery(s);
            if (e == hipSuccess) {
                if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == want) return MSIM_OK;
                return fail(c, MSIM_ERR_HIP, "plan stream drained without raising its signal");
            }
            if (e != hipErrorNotReady) return hip_fail(c, e, "hipStreamQuery(plan stream)");
            const auto now = std::chrono::steady_clock::now();
            if (limit < 0) { t0 = now; limit = wait_limit_seconds(); }
            else if (limit > 0 && std::chrono::duration<double>(now - t0).count() > limit)
                return hip_fail(c, MSIM_WAIT_TIMED_OUT, "spin_until(mailbox signal of the plan stream)");
        }
    }
}

// (an event the host chain is about to need: polled without a pause -- it is microseconds away; `what` names it at the deadline)
static int spin_event(Ctx *c, hipEvent_t ev, const char *what = "spin_event(copy piece of the host chain)") {
    for (uint32_t it = 1;; it++) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return MSIM_OK;
        if (e != hipErrorNotReady) return hip_fail(c, e, "hipEventQuery");
        cpu_relax();
        if ((it & 0xfff) == 0) {                           // ~ every few ms: hand over to the bounded wait
            const hipError_t w = wait_event(ev);
            if (w == hipSuccess) return MSIM_OK;
            return hip_fail(c, w, what);
        }
    }
}

static int ensure_signals(Ctx *c, GpuPlan *g) {
    if (!g->h_sig) {
        MSIM_HIP(c, hipHostMalloc(&g->h_sig, 4096, hipHostMallocMapped));
        memset(g->h_sig, 0, 4096);
    }
    if (!g->copy_stream) {
        {   // The candidates' copy stream: normal priority (MSIM_COPY_PRIO=1 / -1: the low-priority pool / the plan stream's), where
            // it shares a hardware queue with an (idle) side stream.  In the low pool it had a queue of its own and c3 behind c2
            // passes gained 2 % (30.5 -> 29.8 ms) -- until the fourth side stream went there: both in the low pool cost c3 5 ms per
            // step (GpuPlan::n_prep has the story).
            int lo = 0, hi = 0;
            MSIM_HIP(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
            const char *e = getenv("MSIM_COPY_PRIO");
            const int prio = !e ? 0 : atoi(e) > 0 ? lo : atoi(e) < 0 ? hi : 0;
            MSIM_HIP(c, hipStreamCreateWithPriority(&g->copy_stream, hipStreamNonBlocking, prio));
        }
        MSIM_HIP(c, hipEventCreateWithFlags(&g->ev_cand, hipEventDisableTiming));
        for (auto &e : g->ev_piece) MSIM_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (auto &e : g->ev_cpiece) MSIM_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    return MSIM_OK;
}

// ---- The piecewise hand-over of the engines with a host chain: what the device made for the host (candidates, accept tables,
// word window) goes to pinned memory in three pieces -- 1/8, 3/8, 1/2 of the positions -- with an event behind each, and the
// host starts on the first piece while the others are in flight: it consumes a table at ~3 GB/s, the copies deliver 50 GB/s.
// The candidates travel the same way: with one copy of 3.75 MB (a big contig of config 3) it was the candidates, not the table,
// that the walk waited for.  One piece: a plain copy with its event (the host-chain engine's candidates).
// A lane is one array of a hand-over: `stride` bytes per position, `tail` positions more in the last piece (the accept tables'
// end-of-window sentinel where the pieces are counted in words).  Lanes share the pieces; per piece their copies go out in order.
struct HandLane { void *dst; const void *src; size_t stride, tail; };
struct Handover {
    Ctx *c = nullptr;
    hipEvent_t *ev = nullptr;            // one per piece (GpuPlan::ev_piece / ev_cpiece / ev_cand)
    const char *what = nullptr;          // names the wait at its deadline (spin_event)
    size_t cut[4] = {0, 0, 0, 0};
    int pieces = 0, next = 0;            // next: first piece the host has not taken yet
    double wait_us = 0;                  // what the host spent in more()
    // sender: positions [from, to) of every lane, copied on `s` with ev_[q] recorded behind piece q (an empty piece too)
    int send(Ctx *c_, hipStream_t s, hipEvent_t *ev_, const char *what_, size_t from, size_t to, std::initializer_list<HandLane> lanes,
             int pieces_ = 3) {
        const size_t c1 = pieces_ == 1 ? to : from + (to - from) / 8, c2 = pieces_ == 1 ? to : from + (to - from) / 2;
        *this = Handover{c_, ev_, what_, {from, c1, c2, to}, pieces_, 0, 0.0};
        for (int q = 0; q < pieces; q++) {
            const size_t a = cut[q], b = cut[q + 1];
            for (const HandLane &l : lanes) {
                const size_t bl = b + (q == pieces - 1 ? l.tail : 0);
                if (bl > a)
                    MSIM_HIP(c, hipMemcpyAsync(static_cast<uint8_t *>(l.dst) + a * l.stride, static_cast<const uint8_t *>(l.src) + a * l.stride,
                                               (bl - a) * l.stride, hipMemcpyDeviceToHost, s));
            }
            MSIM_HIP(c, hipEventRecord(ev[q], s));
        }
        return MSIM_OK;
    }
    bool drained() const { return next >= pieces; }      // the host has taken every piece (or nothing was sent)
    hipEvent_t last() const { return ev[pieces - 1]; }   // behind the last copy
    // consumer: block until the next piece has landed; *avail = positions [.., *avail) are there.  Drained: nothing happens.
    int more(size_t *avail) {
        if (drained()) return MSIM_OK;
        const auto w0 = std::chrono::steady_clock::now();
        const int rc = spin_event(c, ev[next], what);
        wait_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - w0).count();
        if (!rc) *avail = cut[++next];
        return rc;
    }
    WordFeed feed() { return WordFeed{[](void *u, size_t *avail) { return static_cast<Handover *>(u)->more(avail); }, this}; }
};

// The chain's candidates go to the host beside the plan stream, on the copy stream, and before their number is known there: a
// 16-sigma bound of it first (from = 0: behind everything on the plan stream so far), the rest -- if ever -- after the poll.
// ids: nsn_pos or nsn_rank -> its pinned block; types likewise.  pieces: 3, or 1 copy.  ev_cand: behind every copy so far.
static int cands_to_host(Ctx *c, GpuPlan *g, Handover &ho, HandLane ids, HandLane types, size_t from, size_t to, int pieces) {
    if (!from) {
        hipEvent_t se = next_chain_event(g);
        MSIM_HIP(c, hipEventRecord(se, c->stream));
        MSIM_HIP(c, hipStreamWaitEvent(g->copy_stream, se, 0));
    }
    const bool one = pieces == 1;                          // (its event is ev_cand itself)
    const int rc = ho.send(c, g->copy_stream, one ? &g->ev_cand : g->ev_cpiece, one ? "spin_event(candidates of the host chain, copy stream)"
                           : "spin_event(candidate piece, copy stream)", from, to, {ids, types}, pieces);
    if (!rc && !one) MSIM_HIP(c, hipEventRecord(g->ev_cand, g->copy_stream));
    return rc;
}

// A device engine gives up on a contig (a window overflowed, the host chain failed): nothing of the session is known any more
static void plan_failed(GpuPlan *g) { g->s[0].live = g->s[1].live = false; g->unverified = false; }

// Exact stream position + counts from the mailbox, chain time accounted -- without draining the stream: the mailbox
// kernel writes a sequence word last and the host polls it (a stream synchronisation costs 25-35 us of wake-up
// latency per call, twice per contig)
// behind_mailbox: device work the caller can already enqueue behind the mailbox kernel -- the host would otherwise sit in the
// poll and only then start launching it (20-35 us of launches + their latency, per contig)
template <class F>
static int mixed_poll(Ctx *c, GpuPlan *g, PlanState &h, F &&behind_mailbox) {
    int rc = ensure_signals(c, g);
    if (rc) return rc;
    if (++g->epoch == 0) g->epoch = 1;
    MSIM_HIP(c, hipEventRecord(g->t1, c->stream));
    hipLaunchKernelGGL(k_publish_seq, dim3(1), dim3(1), 0, c->stream, g->d_ps, g->h_mail, g->h_sig, g->epoch);
    MSIM_HIP(c, hipGetLastError());
    if ((rc = behind_mailbox())) return rc;
    if ((rc = spin_until(c, g->h_sig, g->epoch, c->stream))) return rc;
    float ms = 0;
    hipError_t e = hipEventElapsedTime(&ms, g->t0, g->t1);
    if (e == hipErrorNotReady) { MSIM_HIP(c, wait_event(g->t1)); e = hipEventElapsedTime(&ms, g->t0, g->t1); }
    MSIM_HIP(c, e);
    c->t.plan_gpu_ms += ms;
    h = *g->h_mail;
    if (h.flags & (FLAG_SAMPLE_OVERFLOW | FLAG_SNP_OVERFLOW)) {
        plan_failed(g);
        return fail(c, MSIM_ERR_HIP, "GPU sampler: a stream window overflowed its margin (16 sigma; 8 for the start of a sample planned ahead of the chain; results discarded)");
    }
    c->t.py_words += h.pos - g->verified_pos;
    g->verified_pos = h.pos;
    g->s[0].pos = h.pos;
    MSIM_HIP(c, hipEventRecord(g->t0, c->stream));        // the next span starts here
    return MSIM_OK;
}

static int mixed_poll(Ctx *c, GpuPlan *g, PlanState &h) {
    return mixed_poll(c, g, h, []() { return MSIM_OK; });
}

// The plan stream is about to idle while the host walks a chain: close the timed GPU span (t1 must have been
// recorded before the synchronisation that just returned) and reopen it when device work is enqueued again.
static int span_close(Ctx *c, GpuPlan *g) {
    float ms = 0;
    MSIM_HIP(c, hipEventElapsedTime(&ms, g->t0, g->t1));
    c->t.plan_gpu_ms += ms;
    return MSIM_OK;
}

// The previous contig's deferred APPLY goes out when this contig's host chain starts -- and behind the last of the copies
// that chain waits for, so that the rewrite kernel really runs on an idle device: launched right away it shared the CUs
// with k_accept_tables and the D2H copies of the window (c3: 1.54 -> 1.92 ms of rewrite kernel per step).
static int flush_deferred_apply_behind(Ctx *c, hipEvent_t last_copy) {
    if (c->deferred_apply >= 0) MSIM_HIP(c, hipStreamWaitEvent(c->emit_stream, last_copy, 0));
    return flush_deferred_apply(c, true);                  // (groups: an incomplete one stays for its successors)
}

// M.cnt: five u32 counter arrays of nbk + 2 entries, then (8-byte aligned) one 64-bit array of the same length
static inline size_t mixed_cnt_words(uint32_t nbk) { return ((size_t)5 * (nbk + 2) + 1) & ~(size_t)1; }
static inline size_t mixed_cnt_bytes(uint32_t nbk) { return mixed_cnt_words(nbk) * 4 + (size_t)(nbk + 2) * 8; }

// ---- The launches of the SV-mix and host-chain engines' device halves, each group in one place: the engines below and the
// test hooks (gpu_dbg_candidates, gpu_dbg_accept_tables, gpu_dbg_mixed_emit) call the same functions, so a hook runs the
// product's grids and arguments.  Nothing here waits or checks; the caller asks hipGetLastError.
// bitmap -> candidate positions and types of one range (cnt2: (bmw + 255) / 256 + 1 words)
static void cand_front_launch(hipStream_t s, const uint64_t *bm, uint32_t bmw, uint32_t *cnt2, uint32_t start, uint32_t d,
                              const uint32_t *np_raw, unsigned long long np_base, const TypeTable &tt, uint32_t *cand_pos,
                              uint8_t *cand_type) {
    const uint32_t bnb = (bmw + BM_THREADS - 1) / BM_THREADS;
    hipLaunchKernelGGL(k_bitmap_count, dim3(bnb), dim3(BM_THREADS), 0, s, bm, bmw, cnt2);
    hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, s, cnt2, bnb);
    hipLaunchKernelGGL(k_bitmap_expand_cand, dim3(bnb), dim3(BM_THREADS), 0, s, bm, bmw, cnt2, start, d, np_raw, np_base, tt,
                       cand_pos, cand_type);
}
// candidate types by ordinal alone (host-chain engine: no positions yet)
static void types_multi_launch(hipStream_t s, const uint32_t *np_raw, unsigned long long np_base, uint32_t K, const MixRangeDev *rt,
                               uint32_t n_draw, const TypeTable *sets, uint8_t *cand_type) {
    const uint32_t nbk = (K + CB_BLOCK - 1) / CB_BLOCK;
    hipLaunchKernelGGL(k_types_multi, dim3(nbk), dim3(CB_THREADS), 0, s, np_raw, np_base, K, rt, n_draw, sets, cand_type);
}
// the chain's candidates compacted (cnt: nbk + 1 words; cand_pos / nsn_pos may be null: k_nsn_scatter); their number -> ps->n_nsn
static void nsn_compact_launch(hipStream_t s, const uint32_t *cand_pos, const uint8_t *cand_type, uint32_t k, uint32_t *cnt,
                               uint32_t *nsn_pos, uint8_t *nsn_type, uint32_t *nsn_rank, PlanState *ps, bool all) {
    const uint32_t nbk = (k + CB_BLOCK - 1) / CB_BLOCK;
    hipLaunchKernelGGL(k_nsn_count, dim3(nbk), dim3(CB_THREADS), 0, s, cand_type, k, cnt, all ? 1u : 0u);
    hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, s, cnt, nbk);
    hipLaunchKernelGGL(k_nsn_scatter, dim3(nbk), dim3(CB_THREADS), 0, s, cand_pos, cand_type, k, cnt, nbk, nsn_pos, nsn_type, nsn_rank,
                       ps, all ? 1u : 0u);
}
// accept tables over words [p0, p0 + n) resp. from ps->pos on: (n + 1) << lg entries
static void accept_tables_launch(hipStream_t s, const uint32_t *raw, unsigned long long p0, uint32_t n, const ChainClasses &cc,
                                 uint32_t lg, uint32_t *T) {
    const size_t n_slots = (size_t)(n + 1) << lg;
    hipLaunchKernelGGL(k_accept_tables, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, s, raw, p0, n, cc, lg, T);
}
static void accept_tables_ps_launch(hipStream_t s, const uint32_t *raw, const PlanState *ps, uint32_t n, const ChainClasses &cc,
                                    uint32_t lg, uint32_t *T) {
    const size_t n_slots = ((size_t)n + 1) << lg;
    hipLaunchKernelGGL(k_accept_tables_ps, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, s, raw, ps, n, cc, lg, T);
}
// what the host chain decided, from chain order back to candidate order
static void stop_scatter_launch(hipStream_t s, const uint32_t *nsn_rank, const uint32_t *nsn_stop, uint32_t n, uint32_t *cand_stop) {
    hipLaunchKernelGGL(k_stop_scatter, dim3((n + 255) / 256), dim3(256), 0, s, nsn_rank, nsn_stop, n, cand_stop);
}
static void link_scatter_launch(hipStream_t s, const uint32_t *nsn_rank, const uint32_t *nsn_extra, const uint8_t *nsn_aux, uint32_t n,
                                uint32_t *cand_extra, uint8_t *cand_aux) {
    hipLaunchKernelGGL(k_link_scatter, dim3((n + 255) / 256), dim3(256), 0, s, nsn_rank, nsn_extra, nsn_aux, n, cand_extra, cand_aux);
}
// The candidate tables steps 3 and 4 of an SV-mix plan work on.  cnt: mixed_cnt_bytes(nbk); cand_extra / cand_aux: contigs with
// translocations, else null; rt / visit_from: several drawing ranges, else null (k_keep_flags).
struct MixedTables {
    uint32_t k;
    const uint32_t *cand_pos; uint8_t *cand_type; const uint32_t *cand_stop; const uint32_t *cand_extra; const uint8_t *cand_aux;
    uint32_t *cnt, *sn_index;
    const MixRangeDev *rt; uint32_t n_draw; const uint32_t *visit_from; bool sn_chained;
    uint32_t nbk() const { return (k + CB_BLOCK - 1) / CB_BLOCK; }
    uint32_t *bmax() const { return cnt + (nbk() + 2); }
    uint32_t *cnt_keep() const { return cnt + 2 * (nbk() + 2); }
    uint32_t *cnt_sn() const { return cnt + 3 * (nbk() + 2); }
    uint32_t *cnt_ins() const { return cnt + 4 * (nbk() + 2); }
    long long *blk_delta() const { return reinterpret_cast<long long *>(cnt + mixed_cnt_words(nbk())); }   // (8-byte aligned: see mixed_cnt_bytes)
};
// keep flags and counts; n_rec, n_sn, pool_len, len_delta -> *ps
static void keep_flags_launch(hipStream_t s, const msim_params &P, const MixedTables &M, PlanState *ps) {
    const uint32_t nbk = M.nbk();
    BlockTable bt{};
    for (int t = 1; t <= 7; t++) bt.p1[t] = (uint32_t)std::min<int64_t>(P.block[t] + 1, 0xffffffffll);
    hipLaunchKernelGGL(k_blk_reduce, dim3(nbk), dim3(CB_THREADS), 0, s, M.cand_pos, M.cand_type, M.cand_stop, M.k, bt, M.bmax(),
                       M.rt, M.n_draw);
    hipLaunchKernelGGL(k_scan_max_u32, dim3(1), dim3(1024), 0, s, M.bmax(), nbk);
    hipLaunchKernelGGL(k_keep_flags, dim3(nbk), dim3(CB_THREADS), 0, s, M.cand_pos, M.cand_type, M.cand_stop, M.k, bt,
                       M.bmax(), M.cnt_keep(), M.cnt_sn(), M.cnt_ins(), M.blk_delta(), M.rt, M.n_draw, M.visit_from,
                       M.sn_chained ? 1u : 0u, M.cand_extra, M.cand_aux);
    hipLaunchKernelGGL(k_scan4, dim3(4), dim3(1024), 0, s, M.cnt_keep(), M.cnt_sn(), M.cnt_ins(), M.blk_delta(), nbk, ps);
}
// records with their output offsets, SNP ordinals, insert pool (pool: padded to whole dwords, k_pool_fill)
static void emit_records_launch(hipStream_t s, const MixedTables &M, msim_record *recs, uint32_t *rec_off, const uint32_t *np_raw,
                                unsigned long long np_base, uint32_t pool_len, uint8_t *pool) {
    hipLaunchKernelGGL(k_emit_records, dim3(M.nbk()), dim3(CB_THREADS), 0, s, M.cand_pos, M.cand_type, M.cand_stop, M.k,
                       M.cnt_keep(), M.cnt_sn(), M.cnt_ins(), M.blk_delta(), recs, M.sn_index, rec_off, M.cand_extra, M.cand_aux);
    if (pool_len)
        hipLaunchKernelGGL(k_pool_fill, dim3((pool_len / 4 + 256) / 256), dim3(256), 0, s, np_raw, np_base, pool_len, pool);
}

// Steps 3 and 4 of an SV-mix plan, shared by the single-range engine and the host-chain engine: the stops of the chain's
// candidates are in M.cand_stop -> keep flags and counts -> records, insert pool, SNP draws.  p_s: where the SNP draws of
// __mutate_sequence start in the CPython stream.  rt / visit_from / sn_chained: see k_keep_flags (nullptr for one range).
static int mixed_emit(Ctx *c, GpuPlan *g, Contig &ct, MixedSet &M, uint32_t k, uint64_t p_s, const MixRangeDev *rt,
                      uint32_t n_draw, const uint32_t *visit_from, bool sn_chained, Grow &grow, bool has_tl = false) {
    const uint32_t *c_extra = has_tl ? M.cand_extra.p() : nullptr;
    const uint8_t *c_aux = has_tl ? M.cand_aux.p() : nullptr;
    const msim_params &P = c->params;
    GpuStream &py = g->s[0], &np = g->s[1];
    int rc;
    const MixedTables mt{k, M.cand_pos.p(), M.cand_type.p(), M.cand_stop.p(), c_extra, c_aux, M.cnt.p(), M.sn_index.p(), rt, n_draw, visit_from, sn_chained};
    hipLaunchKernelGGL(k_set_pos, dim3(1), dim3(1), 0, c->stream, g->d_ps, (unsigned long long)p_s);

    // ---- 3. keep flags, counts
    keep_flags_launch(c->stream, P, mt, g->d_ps);
    MSIM_HIP(c, hipGetLastError());
    PlanState h;
    if ((rc = mixed_poll(c, g, h))) return rc;
    const uint32_t n_rec = h.n_rec, n_sn = h.n_sn, pool_len = h.pool_len;

    // ---- 4. records, insert pool, SNP draws
    if (!c->chain_only) {   // the record table / pool may still be read by an earlier apply of this contig
        const size_t want = std::max<uint64_t>(n_rec, 1) * sizeof(msim_record);
        if (ct.d_recs.cap < want || ct.d_pool.cap < pool_len + 2 * PAD) {
            MSIM_HIP(c, wait_stream(c->stream));
            MSIM_HIP(c, wait_stream(c->emit_stream));
        }
        if ((rc = dev_reserve(c, ct.d_recs, want))) return rc;
        if ((rc = dev_reserve(c, ct.d_pool, pool_len + 2 * PAD))) return rc;
        if ((rc = dev_reserve(c, ct.d_off, std::max<uint64_t>(n_rec, 1) * sizeof(uint32_t)))) return rc;
    }
    ct.n_rec = n_rec;
    ct.pool_len = pool_len;
    ct.plan_empty = n_rec == 0;
    ct.all_snp = h.n_rec == h.n_sn;
    ct.delta_known = true;
    ct.known_delta = h.len_delta;
    ct.off_ready = !c->chain_only;                         // k_emit_records leaves every record's output offset in d_off
    if (pool_len && (rc = ensure_words(c, g, 1, np.pos + pool_len + 1))) return rc;
    uint64_t pos_hi = p_s;
    hipEvent_t ce = next_chain_event(g);
    MSIM_HIP(c, hipEventRecord(ce, c->stream));
    MSIM_HIP(c, hipStreamWaitEvent(c->emit_stream, ce, 0));
    if (!c->chain_only) {
        emit_records_launch(c->emit_stream, mt, ct.d_recs.p(), ct.d_off.p(), np.d_raw, (unsigned long long)np.pos, pool_len, ct.d_pool.p() + PAD);
        MSIM_HIP(c, hipGetLastError());
    }
    np.pos += pool_len;
    c->t.np_words += pool_len;
    if (n_sn) {                                          // SNP draws in position order (chain: scan + cut; aux off the chain)
        if ((rc = enqueue_snp_stage(c, g, ct, n_sn, M.sn_index.p(), pos_hi, grow))) return rc;
    }
    MSIM_HIP(c, hipEventRecord(M.emit_done, c->emit_stream));
    M.pending = true;
    py.pos = pos_hi;                                       // bound until the next sync reads the exact value
    g->unverified = true;
    g->est.ok = false;                                    // (the SNP sampler's estimate of the position ends here)
    ct.planned = true;
    return MSIM_OK;
}

// __link_tls of the SV-mix engine (mutator.py:130-131 -- after the boundary pass, before __mutate_sequence): its draws follow
// the boundary pass's in the CPython stream, so once the walk knows where that ended, a 16-sigma window of tempered words
// from there comes over and plan_host.cpp links on it.  consumed grows by the words linking drew.
static int mixed_link_translocations(Ctx *c, GpuPlan *g, MixedSet &M, uint32_t n_nsn, uint64_t p_b, size_t &consumed, Grow &grow) {
    size_t n_tl = 0, n_tli = 0;
    count_translocations(g->h_ntype.p(), g->h_nstop.p(), n_nsn, &n_tl, &n_tli);
    uint32_t Wl = 0;
    int rc;
    if (n_tl) {                                            // (no TL: `if tls:` is false and nothing is drawn)
        // |n_tl - n_tli| deletions, min - 1 shuffle swaps and one coin per pair (randint(0, 1) takes two bits and rejects half
        // of them): every draw accepts a word with probability >= 1/2 -- at most 2 words expected, variance 2
        const double mn = (double)std::min(n_tl, n_tli), draws = (double)(std::max(n_tl, n_tli) - std::min(n_tl, n_tli)) + 2.0 * mn;
        const double wl = 2.0 * draws + 16.0 * std::sqrt(2.0 * draws + 1.0) + 4096.0;
        if (wl >= 4.0e9) return fail(c, MSIM_ERR_UNSUPPORTED, "linking window beyond 2^32 words");
        Wl = (uint32_t)wl;
        const uint64_t p_l = p_b + consumed;
        if ((rc = ensure_words(c, g, 0, p_l + Wl + 1))) return rc;
        if ((rc = grow(M.words, (size_t)Wl * 4 + 64))) return rc;
        if ((rc = grow.shared({{g->h_win, (size_t)Wl * 4}}))) return rc;
        hipLaunchKernelGGL(k_temper_window, dim3((Wl + 255) / 256), dim3(256), 0, c->stream, g->s[0].d_raw, (unsigned long long)p_l, Wl,
                           M.words.p());
        MSIM_HIP(c, hipGetLastError());
        MSIM_HIP(c, hipMemcpyAsync(g->h_win.p(), M.words.p(), (size_t)Wl * 4, hipMemcpyDeviceToHost, c->stream));
        MSIM_HIP(c, wait_stream(c->stream));
    }
    size_t used = 0;
    if ((rc = link_translocations(c, g->h_win.p(), Wl, g->h_npos.p(), g->h_ntype.p(), g->h_nstop.p(), g->h_nextra.p(), g->h_naux.p(), n_nsn, &used))) return rc;
    consumed += used;
    return MSIM_OK;
}

// ---- What the SV-mix, host-cut and host-chain engines share besides the hand-over
// The next scratch set.  Its last emit may still read it: the plan stream waits for that -- or the HOST does, where the host is
// about to write the set's pinned staging (walk_h / mm_h), whose copy to the device may still be in flight.
static int mixed_acquire(Ctx *c, GpuPlan *g, bool host_writes_staging, MixedSet *&out) {
    MixedSet &M = g->mixed[g->mixed_unit++ % N_SETS];
    int rc;
    if (host_writes_staging) {
        if (M.pending) MSIM_HIP(c, wait_event(M.emit_done));
        M.pending = false;
    } else if ((rc = wait_if_pending(c, M.pending, M.emit_done))) return rc;
    if (!M.emit_done) MSIM_HIP(c, hipEventCreateWithFlags(&M.emit_done, hipEventDisableTiming));
    out = &M;
    return MSIM_OK;
}

static TypeTable type_table_of(const msim_range &r) {
    TypeTable tt{};
    tt.n = (uint32_t)r.n_types;
    for (int j = 0; j < r.n_types; j++) { tt.thr[j] = r.cdf_thr[j]; tt.type[j] = (uint8_t)r.types[j]; }
    return tt;
}

// the share of a range's candidates that is on the chain: every type but SNP that its draw can produce
static double chain_share(const msim_range &r) {
    double q = 0;
    for (int j = 0; j < r.n_types; j++)
        if (r.types[j] != MSIM_SN && type_drawable(r, j)) q += type_probability(r, j);
    return std::min(1.0, q);
}

// What the host decided about the chain's n candidates, from chain order back to candidate order (k candidates): the stops and,
// with translocations, what __link_tls decided (linked spans, flags, tombstones).  visit_*: the host-chain engine's visit table,
// which travels between the stops' copy and their scatter.  No launch is checked here: the caller asks hipGetLastError.
static int verdicts_to_device(Ctx *c, GpuPlan *g, MixedSet &M, uint32_t n, uint32_t k, bool has_tl, uint32_t *visit_d = nullptr,
                              const uint32_t *visit_h = nullptr, size_t n_visit = 0) {
    if (n) MSIM_HIP(c, hipMemcpyAsync(M.nsn_stop.p(), g->h_nstop.p(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (n_visit) MSIM_HIP(c, hipMemcpyAsync(visit_d, visit_h, n_visit * 4, hipMemcpyHostToDevice, c->stream));
    if (n) stop_scatter_launch(c->stream, M.nsn_rank.p(), M.nsn_stop.p(), n, M.cand_stop.p());
    if (has_tl) {
        MSIM_HIP(c, hipMemsetAsync(M.cand_aux.p(), 0, (size_t)k, c->stream));
        if (n) {
            MSIM_HIP(c, hipMemcpyAsync(M.nsn_extra.p(), g->h_nextra.p(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
            MSIM_HIP(c, hipMemcpyAsync(M.nsn_aux.p(), g->h_naux.p(), (size_t)n, hipMemcpyHostToDevice, c->stream));
            link_scatter_launch(c->stream, M.nsn_rank.p(), M.nsn_extra.p(), M.nsn_aux.p(), n, M.cand_extra.p(), M.cand_aux.p());
        }
    }
    return MSIM_OK;
}

int plan_contig_gpu_mixed(Ctx *c, GpuPlan *g, Contig &ct, const msim_range *ranges, int n_ranges) {
    const msim_params &P = c->params;
    const int64_t d = min_block(P);
    const msim_range *rp = nullptr;
    for (int i = 0; i < n_ranges; i++) if (ranges[i].k) rp = &ranges[i];
    const msim_range &r = *rp;
    const uint32_t k = (uint32_t)r.k;
    int rc;
    if ((rc = session_open(c, g)) || (rc = chain_open(c, g, false))) return rc;
    GpuStream &py = g->s[0], &np = g->s[1];
    Grow grow{c};
    MixedSet *Mp;
    if ((rc = mixed_acquire(c, g, false, Mp))) return rc;
    MixedSet &M = *Mp;
    const uint32_t nbk = (k + CB_BLOCK - 1) / CB_BLOCK;
    if ((rc = grow(M.cand_pos, (size_t)k * 4 + 64))) return rc;
    if ((rc = grow(M.cand_type, (size_t)k + 64))) return rc;
    if ((rc = grow(M.cand_stop, (size_t)k * 4 + 64))) return rc;
    if ((rc = grow(M.nsn_pos, (size_t)k * 4 + 64))) return rc;
    if ((rc = grow(M.nsn_type, (size_t)k + 64))) return rc;
    if ((rc = grow.shared({{g->h_npos, (size_t)k * 4 + 64}, {g->h_ntype, (size_t)k + 64},
                           {g->h_nstop, (size_t)k * 4 + 64}}))) return rc;
    if ((rc = grow(M.nsn_rank, (size_t)k * 4 + 64))) return rc;
    if ((rc = grow(M.nsn_stop, (size_t)k * 4 + 64))) return rc;
    if ((rc = grow(M.sn_index, (size_t)k * 4 + 64))) return rc;
    if ((rc = grow(M.cnt, mixed_cnt_bytes(nbk)))) return rc;
    const bool has_tl = range_draws_translocations(r);
    if (has_tl) {                                          // what __link_tls decides, per candidate and in chain order
        if ((rc = grow(M.cand_extra, (size_t)k * 4 + 64))) return rc;
        if ((rc = grow(M.cand_aux, (size_t)k + 64))) return rc;
        if ((rc = grow(M.nsn_extra, (size_t)k * 4 + 64))) return rc;
        if ((rc = grow(M.nsn_aux, (size_t)k + 64))) return rc;
        if ((rc = grow.shared({{g->h_nextra, (size_t)k * 4 + 64}, {g->h_naux, (size_t)k + 64}}))) return rc;
    }
    uint32_t *cnt_nsn = M.cnt.p();                             // (the other four counter arrays: mixed_emit)

    // ---- 1. sample -> bitmap; bitmap -> candidates with types; non-SNP candidates compacted
    SampleLaunch sl;
    if ((rc = enqueue_sample_chain(c, g, r, d, py.pos, grow, sl))) return rc;
    SampleSet &S = *sl.S;
    const uint64_t np_base = np.pos;                       // exact: the NumPy stream never rejects
    if ((rc = ensure_words(c, g, 1, np_base + 2ull * k + 1))) return rc;
    cand_front_launch(c->stream, reinterpret_cast<const uint64_t *>(S.bitmap.p()), sl.bmw, S.cnt2.p(), (uint32_t)r.start, (uint32_t)d, np.d_raw,
                      (unsigned long long)np_base, type_table_of(r), M.cand_pos.p(), M.cand_type.p());
    nsn_compact_launch(c->stream, M.cand_pos.p(), M.cand_type.p(), k, cnt_nsn, M.nsn_pos.p(), M.nsn_type.p(), M.nsn_rank.p(), g->d_ps, false);
    MSIM_HIP(c, hipGetLastError());
    S.pending = false;                                     // consumed on the plan stream itself
    // The host walks the non-SNP candidates.  Their copy starts at once: a 16-sigma bound of the type draw's binomial, in pieces
    if ((rc = ensure_signals(c, g))) return rc;
    const double q_nsn = chain_share(r);
    const uint32_t n_hi = std::min(g->cand_cap, (uint32_t)std::min<double>(k, q_nsn * k + 16.0 * std::sqrt(q_nsn * (1.0 - q_nsn) * k) + 64.0));
    const HandLane c_pos{g->h_npos.p(), M.nsn_pos.p(), 4, 0}, c_type{g->h_ntype.p(), M.nsn_type.p(), 1, 0};
    Handover cands, cands_rest, tabs;
    if ((rc = cands_to_host(c, g, cands, c_pos, c_type, 0, n_hi, 3))) return rc;
    // The accept tables of the boundary walk depend on where the sample ended (the device knows) and on the window's size --
    // which follows from the number of non-SNP candidates, known only after the poll: they are launched BEHIND the mailbox
    // kernel over a 16-sigma bound of it, so that they are under way while the host still polls.
    const double acc_min = randint_acceptance_min(r);      // least acceptance of randint among the types this range draws
    auto window_of = [&](double n) { return randint_window(n, acc_min); };
    ChainClasses cc;
    const bool tables = chain_classes(r, cc);              // the host walks "next accepted draw" tables (ctx.h)
    const uint32_t lg = chain_lg_rows(cc);
    const bool early = tables && n_hi > 0 && window_of((double)n_hi) < 4.0e9;
    const uint32_t Wb_hi = early ? (uint32_t)window_of((double)n_hi) : 0u;
    // the tables' hand-over, Wb + 1 rows of 1 << lg entries: on the plan stream, behind the kernel that makes them
    auto tables_to_host = [&](uint32_t Wb) {
        return tabs.send(c, c->stream, g->ev_piece, "spin_event(accept-table piece, plan stream)", 0, (size_t)Wb + 1,
                         {HandLane{g->h_words.p(), M.words.p(), (size_t)4 << lg, 0}});
    };
    if (early) {
        const size_t bytes = ((size_t)(Wb_hi + 1) << lg) * 4;
        if ((rc = grow.shared({{g->h_words, bytes}}))) return rc;
        if ((rc = grow(M.words, bytes))) return rc;
        if ((rc = ensure_words(c, g, 0, py.pos + sl.W + Wb_hi + 2))) return rc;      // (the sample ends below py.pos + W)
    }
    PlanState h;
    const auto tq0 = std::chrono::steady_clock::now();
    rc = mixed_poll(c, g, h, [&]() -> int {
        if (!early) return MSIM_OK;
        accept_tables_ps_launch(c->stream, py.d_raw, g->d_ps, Wb_hi, cc, lg, M.words.p());
        MSIM_HIP(c, hipGetLastError());
        return tables_to_host(Wb_hi);
    });
    if (rc) return rc;
    const auto tq1 = std::chrono::steady_clock::now();
    const uint32_t n_nsn = h.n_nsn;
    const uint64_t p_b = h.pos;                            // the boundary pass draws from here
    np.pos = np_base + 2ull * k;
    c->t.np_words += 2ull * k;

    // ---- 2. the sequential chain over the non-SNP candidates, on the host
    size_t consumed = 0;
    const bool early_ok = early && n_nsn > 0 && n_nsn <= n_hi;    // (beyond 16 sigma: the window is built again, exactly, below)
    if (early && !early_ok) MSIM_HIP(c, wait_stream(c->stream));   // nobody reads that table: the blocks are free again
    if (n_nsn) {
        const double wb = window_of((double)n_nsn);
        if (wb >= 4.0e9) return fail(c, MSIM_ERR_UNSUPPORTED, "boundary window beyond 2^32 words");
        const uint32_t Wb = early_ok ? Wb_hi : (uint32_t)wb;
        const size_t words_bytes = tables ? ((size_t)(Wb + 1) << lg) * 4 : (size_t)Wb * 4;
        if (!early_ok) {
            if ((rc = grow.shared({{g->h_words, words_bytes}}))) return rc;
            if ((rc = grow(M.words, words_bytes))) return rc;
            if ((rc = ensure_words(c, g, 0, p_b + Wb + 1))) return rc;
        }
        if (n_nsn > n_hi && (rc = cands_to_host(c, g, cands_rest, c_pos, c_type, n_hi, n_nsn, 1))) return rc;   // beyond 16 sigma
        if (tables) {
            if (!early_ok) {                               // (not launched behind the mailbox: now, with the exact window)
                accept_tables_launch(c->stream, py.d_raw, (unsigned long long)p_b, Wb, cc, lg, M.words.p());
                MSIM_HIP(c, hipGetLastError());
                if ((rc = tables_to_host(Wb))) return rc;
            }
            MSIM_HIP(c, hipEventRecord(g->t1, c->stream));
            if (c->deferred_apply >= 0) MSIM_HIP(c, hipStreamWaitEvent(c->emit_stream, g->ev_cand, 0));   // (... and behind the candidates' copies)
            if ((rc = flush_deferred_apply_behind(c, tabs.last()))) return rc;   // the previous contig's APPLY
            const auto w0 = std::chrono::steady_clock::now();
            ChainWalk cw;
            if ((rc = cw.init(c, r, ct.len, cc, Wb))) return rc;
            static const bool prof = getenv("MSIM_CHAIN_PROF") != nullptr;
            double t_wait = 0, t_run = 0;
            auto tp = std::chrono::steady_clock::now();
            auto lap = [&](double &acc) { const auto n = std::chrono::steady_clock::now(); acc += std::chrono::duration<double, std::micro>(n - tp).count(); tp = n; };
            // candidates and table both arrive in pieces; the walk runs over what is there and waits for whichever ran out
            size_t avail_c = 0, avail_w = 0;
            while (!rc && cw.j < n_nsn) {
                const bool need_c = cw.j >= avail_c, need_w = (cw.ws >> cw.lg_rows) >= avail_w;
                if (!need_c && !need_w) break;             // (run stops for one of the two reasons only)
                if (need_c) {
                    const size_t had = avail_c;
                    Handover &from = cands.drained() ? cands_rest : cands;   // (the rest: beyond 16 sigma)
                    if (from.drained() || (rc = from.more(&avail_c))) break;
                    avail_c = std::min<size_t>(avail_c, n_nsn);
                    if (!ChainWalk::types_ok(g->h_ntype.p() + had, avail_c - had, has_tl)) {
                        rc = fail(c, MSIM_ERR_HIP, "boundary chain: candidate type outside the range's draw");
                        break;
                    }
                }
                if (need_w) {
                    if (tabs.drained() || (rc = tabs.more(&avail_w))) break;   // (drained: the window is used up, finish() reports it)
                }
                lap(t_wait);
                if (has_tl) cw.run_tl(g->h_npos.p(), g->h_ntype.p(), avail_c, g->h_words.p(), avail_w, g->h_nstop.p());
                else cw.run(g->h_npos.p(), g->h_ntype.p(), avail_c, g->h_words.p(), avail_w, g->h_nstop.p());
                lap(t_run);
            }
            if (!rc) rc = spin_event(c, g->ev_cand, "spin_event(candidates of the host chain, copy stream)");       // (every copy into the pinned blocks has landed before they are reused)
            if (prof) fprintf(stderr, "chain: n_nsn %u Wb %u wait %.0f us run %.0f us (%.2f ns/cand) w %zu | poll %.0f us, enqueue %.0f us\n", n_nsn, Wb, t_wait, t_run, t_run * 1e3 / n_nsn, cw.ws >> cw.lg_rows,
                              std::chrono::duration<double, std::micro>(tq1 - tq0).count(), std::chrono::duration<double, std::micro>(w0 - tq1).count());
            if (!rc) rc = cw.finish(c, n_nsn, &consumed);
            c->t.host_walk_run_ms += t_run * 1e-3;
            c->t.host_walk_wait_ms += t_wait * 1e-3 + std::chrono::duration<double, std::milli>(tq1 - tq0).count();
            c->t.host_walk_candidates += n_nsn;
            c->t.plan_host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
            if (!rc) {
                MSIM_HIP(c, wait_event(g->t1));   // long complete
                rc = span_close(c, g);
            }
        } else {
            hipLaunchKernelGGL(k_temper_window, dim3((Wb + 255) / 256), dim3(256), 0, c->stream, py.d_raw,
                               (unsigned long long)p_b, Wb, M.words.p());
            MSIM_HIP(c, hipGetLastError());
            MSIM_HIP(c, hipMemcpyAsync(g->h_words.p(), M.words.p(), words_bytes, hipMemcpyDeviceToHost, c->stream));
            MSIM_HIP(c, hipEventRecord(g->t1, c->stream));
            if ((rc = flush_deferred_apply(c, true))) return rc;
            MSIM_HIP(c, wait_stream(c->stream));
            MSIM_HIP(c, wait_stream(g->copy_stream));
            if ((rc = span_close(c, g))) return rc;
            size_t kept_host = 0;
            long long delta_host = 0;                      // both are summed on the device, where the stops end up
            rc = chain_boundary_host(c, r, ct.len, g->h_npos.p(), g->h_ntype.p(), n_nsn, g->h_words.p(), Wb, g->h_nstop.p(),
                                     &consumed, &kept_host, &delta_host);
        }
        if (!rc && has_tl) rc = mixed_link_translocations(c, g, M, n_nsn, p_b, consumed, grow);
        if (rc) { plan_failed(g); return rc; }
        MSIM_HIP(c, hipEventRecord(g->t0, c->stream));    // the host chain is not GPU time
    }
    if ((rc = verdicts_to_device(c, g, M, n_nsn, k, has_tl))) return rc;
    if (has_tl) MSIM_HIP(c, hipGetLastError());
    const uint64_t p_s = p_b + consumed;                   // the SNP draws of __mutate_sequence start here
    return mixed_emit(c, g, ct, M, k, p_s, nullptr, 0, nullptr, false, grow, has_tl);
}


// ====================================================================== host-cut contigs
// Deterministic-SNP ranges of any size and number (RMT gene-blocking files: thousands of small ranges per
// contig, pool-path hot spots): the stream cuts form a chain of thousands of tiny data-dependent samples,
// so the host finds them (plan_host.cpp: cut_ranges_host) -- over words the DEVICE generated, and nothing
// but the cuts: the device repeats the acceptance test over every range's interval, builds the sorted sample
// in a contig-wide bitmap and from it the records (k_interval_bits, k_walk_expand); the SNP transducer of
// section 5 and APPLY follow as for every other engine.
bool gpu_plan_hostsample_eligible(const Ctx *c, const msim_range *ranges, int n_ranges) {
    const msim_params &P = c->params;
    const int64_t d = min_block(P);
    if (P.block[MSIM_SN] != d) return false;
    int64_t prev_stop = -1;
    uint64_t K = 0;
    for (int i = 0; i < n_ranges; i++) {
        const msim_range &r = ranges[i];
        if (r.k == 0) continue;
        const int64_t n = range_population(r, d);
        if (r.k < 0 || n < r.k || n >= (1ll << 32)) return false;        // ValueError / multi-word: host planner decides
        if (r.start <= prev_stop || r.stop >= (1ll << 32)) return false; // overlapping or unsorted ranges: dict semantics
        if (!range_is_deterministic_sn(r)) return false;
        prev_stop = r.stop;
        K += (uint64_t)r.k;
    }
    return K > 0 && K < (1ull << 31);
}

int plan_contig_gpu_hostsample(Ctx *c, GpuPlan *g, Contig &ct, const msim_range *ranges, int n_ranges) {
    static const bool prof = getenv("MSIM_CHAIN_PROF") != nullptr;
    static std::chrono::steady_clock::time_point last_exit;
    const auto tp0 = std::chrono::steady_clock::now();
    const msim_params &P = c->params;
    const int64_t d = min_block(P);
    int rc;
    if ((rc = session_open(c, g)) || (rc = chain_open(c, g, false))) return rc;
    GpuStream &py = g->s[0];
    // word window: expected consumption of every sample + 16 sigma of the total
    uint64_t K = 0, K_pool = 0;
    uint32_t n_draw = 0;
    double e_words = 0, var = 0;
    for (int i = 0; i < n_ranges; i++) {
        const msim_range &r = ranges[i];
        if (r.k == 0) continue;
        n_draw++;
        const double k = (double)r.k, n = (double)range_population(r, d);
        K += (uint64_t)r.k;
        if (n <= (double)r.setsize) K_pool += (uint64_t)r.k;
        const StreamMoments m = small_sample_moments(n, k, (double)r.setsize);
        e_words += m.e; var += m.v;
    }
    const double wd = e_words + 16.0 * std::sqrt(var) + 65536.0;
    if (wd >= 4.0e9) return fail(c, MSIM_ERR_UNSUPPORTED, "sample window beyond 2^32 words");
    const uint32_t W = (uint32_t)wd;
    Grow grow{c};
    MixedSet *Mp;
    if ((rc = mixed_acquire(c, g, true, Mp))) return rc;   // (the host writes the set's pinned range table below)
    MixedSet &M = *Mp;
    // what the host hands back: one cut per drawing range (+ the end) and the pool-path positions
    const size_t n_back = (size_t)n_draw + 1 + K_pool;
    if ((rc = grow(M.words, (size_t)W * 4))) return rc;
    if ((rc = grow(M.cand_pos, n_back * 4 + 64))) return rc;
    if ((rc = grow(M.walk_d, (size_t)n_draw * sizeof(WalkRange) + 64))) return rc;
    if ((rc = grow.own(M.walk_h, (size_t)n_draw * sizeof(WalkRange) + 64))) return rc;
    if ((rc = grow.shared({{g->h_words, (size_t)W * 4}, {g->h_npos, n_back * 4 + 64}}))) return rc;
    if (!M.p0_slot) MSIM_HIP(c, hipMalloc(&M.p0_slot, 64));
    const uint32_t bmw = (uint32_t)((ct.len + 63) / 64);  // contig-wide bitmap, 64-bit words
    const uint32_t bnb = (bmw + BM_THREADS - 1) / BM_THREADS;
    {
        const size_t want = (size_t)bmw * 8 + 64;
        if (M.wbits.cap < want) {
            const size_t before = M.wbits.cap;
            if ((rc = grow(M.wbits, want))) return rc;
            if (M.wbits.cap != before) MSIM_HIP(c, hipMemset(M.wbits.p(), 0, M.wbits.cap));   // k_walk_expand leaves it zeroed
        }
        if (M.wbits_dirty) {
            MSIM_HIP(c, hipMemsetAsync(M.wbits.p(), 0, M.wbits.cap, c->stream));
            M.wbits_dirty = false;
        }
    }
    if ((rc = grow(M.wcnt, (size_t)(bnb + 2) * sizeof(uint32_t)))) return rc;
    if (!c->chain_only) {   // the record table may still be read by an earlier apply of this contig
        const size_t want = (size_t)K * sizeof(msim_record);
        if (ct.d_recs.cap < want || ct.d_pool.cap < 2 * PAD) {
            MSIM_HIP(c, wait_stream(c->stream));
            MSIM_HIP(c, wait_stream(c->emit_stream));
        }
        if ((rc = dev_reserve(c, ct.d_recs, want))) return rc;
        if ((rc = dev_reserve(c, ct.d_pool, 2 * PAD))) return rc;
    }
    {
        uint32_t at = 0, base = 0;
        for (int i = 0; i < n_ranges; i++) {
            const msim_range &r = ranges[i];
            if (r.k == 0) continue;
            const int64_t n = range_population(r, d);
            WalkRange w;
            w.start = (uint32_t)r.start; w.k = (uint32_t)r.k; w.n = (uint32_t)n; w.rec_base = base;
            w.pool = n <= r.setsize ? 1u : 0u;
            M.walk_h.p()[at++] = w;
            base += (uint32_t)r.k;
        }
    }
    if ((rc = ensure_words(c, g, 0, py.pos + W + 1))) return rc;
    hipLaunchKernelGGL(k_temper_window_ps, dim3((W + 255) / 256), dim3(256), 0, c->stream, py.d_raw, g->d_ps, W, M.words.p());
    MSIM_HIP(c, hipGetLastError());
    if ((rc = ensure_signals(c, g))) return rc;
    Handover win;                                          // the window comes over in pieces
    if ((rc = win.send(c, c->stream, g->ev_piece, "spin_event(word-window piece, plan stream)", 0, W, {HandLane{g->h_words.p(), M.words.p(), 4, 0}})))
        return rc;
    MSIM_HIP(c, hipEventRecord(g->t1, c->stream));
    MSIM_HIP(c, hipMemcpyAsync(M.walk_d.p(), M.walk_h.p(), (size_t)n_draw * sizeof(WalkRange), hipMemcpyHostToDevice, c->stream));
    const auto tp1 = std::chrono::steady_clock::now();
    // ---- the host finds the stream cuts (and samples the pool-path ranges); everything per position stays here
    size_t consumed = 0, n_pool_pos = 0;
    uint32_t *h_cut = g->h_npos.p(), *h_pool = g->h_npos.p() + n_draw + 1;
    const WordFeed feed = win.feed();
    if ((rc = flush_deferred_apply_behind(c, win.last()))) return rc;   // the previous contig's APPLY
    {
        const auto cw0 = std::chrono::steady_clock::now();
        rc = cut_ranges_host(c, ranges, n_ranges, d, g->h_words.p(), W, h_cut, h_pool, &n_pool_pos, &consumed, &feed);
        const double all_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - cw0).count();
        c->t.host_walk_wait_ms += win.wait_us * 1e-3;
        c->t.host_walk_run_ms += std::max(0.0, all_ms - win.wait_us * 1e-3);
        c->t.host_cut_words += consumed;
    }
    if (!rc) {
        MSIM_HIP(c, wait_event(g->t1));           // all pieces landed (usually long ago): the pinned window is free again
        rc = span_close(c, g);
    }
    if (rc) { plan_failed(g); M.wbits_dirty = true; return rc; }
    const auto tp3 = std::chrono::steady_clock::now();
    MSIM_HIP(c, hipEventRecord(g->t0, c->stream));        // the host chain is not GPU time
    MSIM_HIP(c, hipMemcpyAsync(M.cand_pos.p(), g->h_npos.p(), ((size_t)n_draw + 1 + n_pool_pos) * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_advance_pos_save, dim3(1), dim3(1), 0, c->stream, g->d_ps, (unsigned long long)consumed, M.p0_slot);
    MSIM_HIP(c, hipGetLastError());
    if (!c->chain_only) {   // records on the emit stream (ordered after any earlier APPLY that still reads this contig's table): the
        // words of every range -> contig-wide bitmap -> sorted sample -> records
        hipEvent_t ce0 = next_chain_event(g);
        MSIM_HIP(c, hipEventRecord(ce0, c->stream));
        MSIM_HIP(c, hipStreamWaitEvent(c->emit_stream, ce0, 0));
        hipLaunchKernelGGL(k_interval_bits, dim3(((uint32_t)consumed + 255) / 256), dim3(256), 0, c->emit_stream, py.d_raw,
                           M.p0_slot, (uint32_t)consumed, M.cand_pos.p(), M.walk_d.p(), n_draw, reinterpret_cast<uint32_t *>(M.wbits.p()));
        if (n_pool_pos)
            hipLaunchKernelGGL(k_list_to_bits, dim3(((uint32_t)n_pool_pos + 255) / 256), dim3(256), 0, c->emit_stream,
                               M.cand_pos.p() + n_draw + 1, (uint32_t)n_pool_pos, reinterpret_cast<uint32_t *>(M.wbits.p()));
        hipLaunchKernelGGL(k_bitmap_count, dim3(bnb), dim3(BM_THREADS), 0, c->emit_stream,
                           reinterpret_cast<const uint64_t *>(M.wbits.p()), bmw, M.wcnt.p());
        hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, c->emit_stream, M.wcnt.p(), bnb);
        hipLaunchKernelGGL(k_walk_expand, dim3(bnb), dim3(BM_THREADS), 0, c->emit_stream,
                           reinterpret_cast<uint64_t *>(M.wbits.p()), bmw, M.wcnt.p(), M.walk_d.p(), n_draw, (uint32_t)d, ct.d_recs.p());
        MSIM_HIP(c, hipGetLastError());
    }
    ct.n_rec = K;
    ct.pool_len = 0;
    ct.plan_empty = false;
    ct.all_snp = true;
    uint64_t pos_hi = py.pos + consumed;
    if (K) {                                          // SNP draws in position order (chain: scan + cut; aux off the chain)
        if ((rc = enqueue_snp_stage(c, g, ct, K, nullptr, pos_hi, grow))) return rc;
    }
    MSIM_HIP(c, hipEventRecord(M.emit_done, c->emit_stream));
    M.pending = true;
    py.pos = pos_hi;
    g->s[1].pos += 2 * K;                                  // numpy.random.choice(size=k) per drawing range
    c->t.np_words += 2 * K;
    ct.planned = true;
    if (prof) {
        const auto tp4 = std::chrono::steady_clock::now();
        auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        fprintf(stderr, "hostcut: n_draw %u K %llu W %u | outside %.0f setup %.0f wait %.0f cut %.0f post %.0f us\n", n_draw, (unsigned long long)K, W,
                us(last_exit, tp0), us(tp0, tp1), win.wait_us, us(tp1, tp3) - win.wait_us, us(tp3, tp4));
        last_exit = tp4;
    }
    return MSIM_OK;
}


// ====================================================================== host-chain engine
// Contigs the three engines above decline but whose stream structure is still a plain chain: several drawing ranges with
// their own settings (RMT: gene blocks + an SV `std` line, hot / cold ranges), SV types on many small ranges, an SNP
// block above the sampling distance.  Per range the reference runs sample -> type draw -> boundary pass before it touches
// the next range (mutator.py:116-123,144-214), so the CPython stream interleaves samples and randint draws and the whole
// contig is ONE chain: the host walks it (plan_host.cpp: multimix_walk_host) over a window of tempered words, the accept
// tables of every randint class (k_accept_tables_ps) and the candidate TYPES -- a function of the candidate's ordinal
// alone (k_types_multi), hence known before any position is -- all produced on the device.  Back on the device: the
// SNP filter (blocked ends clipped per range), the visit filter across range borders, records, insert pool, SNP draws.
constexpr uint64_t MM_MIN_K = 1024;                      // below: the host planner is as fast as the round trips

bool gpu_plan_multimix_eligible(const Ctx *c, GpuPlan *g, uint64_t L, const msim_range *ranges, int n_ranges) {
    g->mm_for = nullptr;
    if (!multimix_prepare(c, L, ranges, n_ranges, g->mm_sets)) return false;
    if (g->mm_sets.K < MM_MIN_K) return false;
    g->mm_for = ranges; g->mm_n = n_ranges;
    return true;
}

int plan_contig_gpu_multimix(Ctx *c, GpuPlan *g, Contig &ct, const msim_range *ranges, int n_ranges) {
    static const bool prof = getenv("MSIM_CHAIN_PROF") != nullptr;
    const auto tp0 = std::chrono::steady_clock::now();
    const msim_params &P = c->params;
    const int64_t d = min_block(P);
    int rc;
    if (g->mm_for != ranges || g->mm_n != n_ranges) {
        if (!multimix_prepare(c, ct.len, ranges, n_ranges, g->mm_sets)) return fail(c, MSIM_ERR_UNSUPPORTED, "outside the host-chain engine");
    }
    g->mm_for = nullptr;
    const MixSets &ms = g->mm_sets;
    const uint32_t K = (uint32_t)ms.K, n_draw = ms.n_draw, n_sets = (uint32_t)ms.rep.size();
    const uint32_t lg = chain_lg_rows(ms.gcc);
    if ((rc = session_open(c, g)) || (rc = chain_open(c, g, false))) return rc;
    GpuStream &py = g->s[0], &np = g->s[1];
    // ---- sizes: the word window (every sample + every randint, 16 sigma of the total) and the chain length
    double e_words = 0, var = 0, e_ch = 0, var_ch = 0;
    std::vector<double> q_nsn(n_sets, 0.0), acc_min(n_sets, 1.0), q_tl(n_sets, 0.0);
    for (uint32_t s = 0; s < n_sets; s++) {
        const msim_range &r = ranges[ms.rep[s]];
        for (int j = 0; j < r.n_types; j++)
            if (type_drawable(r, j) && (r.types[j] == MSIM_TL || r.types[j] == MSIM_TLI)) q_tl[s] += type_probability(r, j);
        acc_min[s] = randint_acceptance_min(r);                       // (multimix_prepare let only widths 1 .. 2^24 - 1 through)
        q_nsn[s] = chain_share(r);
    }
    {
        uint32_t di = 0;
        for (int i = 0; i < n_ranges; i++) {
            const msim_range &r = ranges[i];
            if (r.k == 0) continue;
            const uint32_t s = ms.set_of[di++];
            const double k = (double)r.k, n = (double)range_population(r, d);
            const StreamMoments sm = small_sample_moments(n, k, (double)r.setsize);
            e_words += sm.e; var += sm.v;
            const double m = k * q_nsn[s];                                                 // randint draws: at most one per non-SNP
            e_ch += m; var_ch += m * (1.0 - q_nsn[s]);
            e_words += m / acc_min[s];
            var += m / (acc_min[s] * acc_min[s]);
            if (ms.has_tl) { e_words += 5.0 * k * q_tl[s]; var += 25.0 * k * q_tl[s]; }   // __link_tls: deletions, shuffle, one coin
                                                                                            // per pair, <= 2 words per draw on average
        }
    }
    const double wd = e_words + 16.0 * std::sqrt(var) + 65536.0;
    if (wd >= 1.0e9) return fail(c, MSIM_ERR_UNSUPPORTED, "host-chain window beyond 2^30 words");
    const uint32_t W = (uint32_t)wd;
    const uint32_t n_hi = std::min(g->cand_cap, ms.sn_chained ? K : (uint32_t)std::min<double>(K, e_ch + 16.0 * std::sqrt(var_ch) + 64.0));
    Grow grow{c};
    MixedSet *Mp;
    if ((rc = mixed_acquire(c, g, true, Mp))) return rc;   // (the host writes the set's pinned tables below)
    MixedSet &M = *Mp;
    const uint32_t nbk = (K + CB_BLOCK - 1) / CB_BLOCK;
    const size_t n_slots = ((size_t)W + 1) << lg;
    if ((rc = grow(M.cand_pos, (size_t)K * 4 + 64))) return rc;
    if ((rc = grow(M.cand_type, (size_t)K + 64))) return rc;
    if ((rc = grow(M.cand_stop, (size_t)K * 4 + 64))) return rc;
    if ((rc = grow(M.nsn_type, (size_t)K + 64))) return rc;
    if ((rc = grow(M.nsn_rank, (size_t)K * 4 + 64))) return rc;
    if ((rc = grow(M.nsn_stop, (size_t)K * 4 + 64))) return rc;
    if ((rc = grow(M.sn_index, (size_t)K * 4 + 64))) return rc;
    if ((rc = grow(M.cnt, mixed_cnt_bytes(nbk)))) return rc;
    if ((rc = grow(M.words, (size_t)W * 4 + 64))) return rc;
    if ((rc = grow(M.tables, n_slots * 4 + 64))) return rc;
    if (ms.has_tl) {
        if ((rc = grow(M.cand_extra, (size_t)K * 4 + 64))) return rc;
        if ((rc = grow(M.cand_aux, (size_t)K + 64))) return rc;
        if ((rc = grow(M.nsn_extra, (size_t)K * 4 + 64))) return rc;
        if ((rc = grow(M.nsn_aux, (size_t)K + 64))) return rc;
    }
    // range table | type tables | visit_from, one device block and one pinned block per scratch set
    const size_t off_sets = ((size_t)n_draw * sizeof(MixRangeDev) + 63) & ~(size_t)63;
    const size_t off_visit = (off_sets + (size_t)n_sets * sizeof(TypeTable) + 63) & ~(size_t)63;
    const size_t mm_bytes = off_visit + (size_t)n_draw * 4 + 64;
    if ((rc = grow(M.mm_d, mm_bytes))) return rc;
    if ((rc = grow.own(M.mm_h, mm_bytes))) return rc;
    const size_t tl4 = ms.has_tl ? (size_t)K * 4 + 64 : 0, tl1 = ms.has_tl ? (size_t)K + 64 : 0;   // (0: the block is not wanted)
    if ((rc = grow.shared({{g->h_words, n_slots * 4}, {g->h_win, (size_t)W * 4}, {g->h_npos, (size_t)K * 4 + 64},
                        {g->h_ntype, (size_t)K + 64}, {g->h_nstop, (size_t)K * 4 + 64}, {g->h_nrank, (size_t)K * 4 + 64},
                        {g->h_nextra, tl4}, {g->h_naux, tl1}}))) return rc;
    MixRangeDev *rt_h = reinterpret_cast<MixRangeDev *>(M.mm_h.p());
    TypeTable *sets_h = reinterpret_cast<TypeTable *>(M.mm_h.p() + off_sets);
    uint32_t *visit_h = reinterpret_cast<uint32_t *>(M.mm_h.p() + off_visit);
    const MixRangeDev *rt_d = reinterpret_cast<const MixRangeDev *>(M.mm_d.p());
    const TypeTable *sets_d = reinterpret_cast<const TypeTable *>(M.mm_d.p() + off_sets);
    uint32_t *visit_d = reinterpret_cast<uint32_t *>(M.mm_d.p() + off_visit);
    {
        uint32_t di = 0, base = 0;
        for (int i = 0; i < n_ranges; i++) {
            const msim_range &r = ranges[i];
            if (r.k == 0) continue;
            rt_h[di] = MixRangeDev{base, (uint32_t)(r.stop + 1), ms.set_of[di], 0u};
            base += (uint32_t)r.k;
            di++;
        }
        for (uint32_t s = 0; s < n_sets; s++) sets_h[s] = type_table_of(ranges[ms.rep[s]]);
    }
    // ---- 1. device: word window, accept tables, candidate types, the chain's candidates
    const uint64_t np_base = np.pos;                       // exact: the NumPy stream never rejects
    if ((rc = ensure_words(c, g, 0, py.pos + W + 1))) return rc;
    if ((rc = ensure_words(c, g, 1, np_base + 2ull * K + 1))) return rc;
    if ((rc = ensure_signals(c, g))) return rc;
    MSIM_HIP(c, hipMemcpyAsync(M.mm_d.p(), M.mm_h.p(), off_visit, hipMemcpyHostToDevice, c->stream));
    types_multi_launch(c->stream, np.d_raw, (unsigned long long)np_base, K, rt_d, n_draw, sets_d, M.cand_type.p());
    nsn_compact_launch(c->stream, nullptr, M.cand_type.p(), K, M.cnt.p(), nullptr, M.nsn_type.p(), M.nsn_rank.p(), g->d_ps, ms.sn_chained);
    MSIM_HIP(c, hipGetLastError());
    const HandLane c_rank{g->h_nrank.p(), M.nsn_rank.p(), 4, 0}, c_type{g->h_ntype.p(), M.nsn_type.p(), 1, 0};
    Handover cands, win;
    if ((rc = cands_to_host(c, g, cands, c_rank, c_type, 0, n_hi, 1))) return rc;   // a 16-sigma bound of their number, in one copy
    hipLaunchKernelGGL(k_temper_window_ps, dim3((W + 255) / 256), dim3(256), 0, c->stream, py.d_raw, g->d_ps, W, M.words.p());
    accept_tables_ps_launch(c->stream, py.d_raw, g->d_ps, W, ms.gcc, lg, M.tables.p());
    MSIM_HIP(c, hipGetLastError());
    // Window and tables come over in the same pieces, the tables with their end-of-window sentinel.  Their copies go out
    // behind the mailbox kernel, before the host polls: nothing of them depends on what the poll tells.
    PlanState h;
    rc = mixed_poll(c, g, h, [&]() -> int {                // exact stream position + the chain's length
        return win.send(c, c->stream, g->ev_piece, "spin_event(word-window piece, plan stream)", 0, W,
                        {HandLane{g->h_win.p(), M.words.p(), 4, 0}, HandLane{g->h_words.p(), M.tables.p(), (size_t)4 << lg, 1}});
    });
    if (rc) return rc;
    const uint32_t n_ch = h.n_nsn;
    const uint64_t p0 = h.pos;
    np.pos = np_base + 2ull * K;
    c->t.np_words += 2ull * K;
    if (n_ch > n_hi && (rc = cands_to_host(c, g, cands, c_rank, c_type, n_hi, n_ch, 1))) return rc;   // beyond 16 sigma
    MSIM_HIP(c, hipEventRecord(g->t1, c->stream));
    if (c->deferred_apply >= 0) MSIM_HIP(c, hipStreamWaitEvent(c->emit_stream, g->ev_cand, 0));   // (behind the candidates' copies too)
    if ((rc = flush_deferred_apply_behind(c, win.last()))) return rc;   // the previous contig's APPLY
    const auto tp1 = std::chrono::steady_clock::now();
    // ---- 2. the chain, on the host
    size_t consumed = 0, n_there = 0;
    const WordFeed feed = win.feed();
    rc = cands.more(&n_there);                             // all of the chain's candidates (one copy, or the rest of them)
    const auto mw0 = std::chrono::steady_clock::now();
    c->t.host_walk_wait_ms += std::chrono::duration<double, std::milli>(mw0 - tp1).count();
    if (!rc) rc = multimix_walk_host(c, ct.len, ranges, n_ranges, d, ms, g->h_win.p(), g->h_words.p(), W, g->h_nrank.p(), g->h_ntype.p(), n_ch,
                                     g->h_npos.p(), g->h_nstop.p(), visit_h, &consumed, &feed, ms.has_tl ? g->h_nextra.p() : nullptr,
                                     ms.has_tl ? g->h_naux.p() : nullptr);
    {
        const double all_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - mw0).count();
        c->t.host_walk_wait_ms += win.wait_us * 1e-3;
        c->t.host_walk_run_ms += std::max(0.0, all_ms - win.wait_us * 1e-3);
        c->t.host_walk_candidates += K;
    }
    if (!rc) {
        MSIM_HIP(c, wait_event(g->t1));           // all pieces landed (usually long ago): the pinned blocks are free again
        rc = span_close(c, g);
    }
    if (rc) { plan_failed(g); return rc; }
    const auto tp2 = std::chrono::steady_clock::now();
    MSIM_HIP(c, hipEventRecord(g->t0, c->stream));        // the host chain is not GPU time
    // ---- 3. back on the device
    MSIM_HIP(c, hipMemcpyAsync(M.cand_pos.p(), g->h_npos.p(), (size_t)K * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = verdicts_to_device(c, g, M, n_ch, K, ms.has_tl, visit_d, visit_h, n_draw))) return rc;
    MSIM_HIP(c, hipGetLastError());
    rc = mixed_emit(c, g, ct, M, K, p0 + consumed, rt_d, n_draw, visit_d, ms.sn_chained, grow, ms.has_tl);
    if (prof) {
        const auto tp3 = std::chrono::steady_clock::now();
        auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        fprintf(stderr, "hostchain: n_draw %u sets %u K %u chain %u W %u lg %u | pre %.0f walk %.0f (%.2f ns/cand) post %.0f us\n", n_draw, n_sets, K,
                n_ch, W, lg, us(tp0, tp1), us(tp1, tp2), us(tp1, tp2) * 1e3 / K, us(tp2, tp3));
    }
    return rc;
}

// ====================================================================== test support: the device halves on hand-built tables
// msim_dbg_candidates / msim_dbg_accept_tables / msim_dbg_mixed_emit: the launch helpers above over tables the caller made, in
// device buffers of their own, synchronous, touching no contig and no stream session.  Each checks on the host what the
// planners guarantee and refuses everything else (MSIM_ERR_ARG) before anything is allocated or launched.
namespace {
bool dbg_type_table_ok(const TypeTable &tt) {
    if (tt.n < 1 || tt.n > 8) return false;
    for (uint32_t j = 0; j < tt.n; j++) {
        if (tt.type[j] < 1 || tt.type[j] > 7) return false;
        if (j && tt.thr[j] < tt.thr[j - 1]) return false;
    }
    return true;
}
}  // namespace

// Form (a), bm given: one range's bitmap (n_words words), start, d -> cand_pos / cand_type (k_bitmap_count, k_scan_u32,
// k_bitmap_expand_cand over sets[0]), then the compaction.  Form (b), bm null: K candidates typed by ordinal over rt[n_draw] and
// sets[n_sets] (k_types_multi), the compaction without positions.  np_raw: RAW NumPy-stream words, at least two per candidate.
// Outputs hold `cap` entries each (cand_pos / nsn_pos unused in form (b)); *k_out candidates, *n_nsn on the chain.
int gpu_dbg_candidates(Ctx *c, const uint64_t *bm, uint32_t n_words, uint32_t start, uint32_t d, uint32_t K, const void *rt_v,
                       uint32_t n_draw, const void *sets_v, uint32_t n_sets, const uint32_t *np_raw, uint64_t n_np, uint32_t all,
                       uint32_t *cand_pos, uint8_t *cand_type, uint32_t *nsn_pos, uint8_t *nsn_type, uint32_t *nsn_rank, uint64_t cap,
                       uint32_t *k_out, uint32_t *n_nsn) {
    const MixRangeDev *rt = static_cast<const MixRangeDev *>(rt_v);
    const TypeTable *sets = static_cast<const TypeTable *>(sets_v);
    if (!sets || n_sets < 1 || n_sets > 8 || !cand_type || !nsn_type || !nsn_rank || !k_out || !n_nsn || all > 1 || (n_np && !np_raw))
        return fail(c, MSIM_ERR_ARG, "msim_dbg_candidates: bad argument");
    for (uint32_t q = 0; q < n_sets; q++)
        if (!dbg_type_table_ok(sets[q])) return fail(c, MSIM_ERR_ARG, "msim_dbg_candidates: type table outside 1..8 types, types 1..7, non-decreasing thresholds");
    uint64_t k = K;
    if (bm) {
        if (!n_words || n_words > (1u << 26) || n_sets != 1 || !cand_pos || !nsn_pos)
            return fail(c, MSIM_ERR_ARG, "msim_dbg_candidates: a bitmap takes 1..2^26 words, one type table and room for positions");
        k = 0;
        for (uint32_t q = 0; q < n_words; q++) k += (uint64_t)__builtin_popcountll(bm[q]);
        if ((uint64_t)start + 64ull * n_words + (uint64_t)d * k >= (1ull << 32))
            return fail(c, MSIM_ERR_ARG, "msim_dbg_candidates: positions beyond 2^32");
    } else {
        if (!rt || n_draw < 1 || K < 1 || K > (1u << 28) || rt[0].rec_base != 0)
            return fail(c, MSIM_ERR_ARG, "msim_dbg_candidates: a range table starts at candidate 0 and has 1..2^28 candidates");
        for (uint32_t q = 0; q < n_draw; q++)
            if (rt[q].set_id >= n_sets || rt[q].rec_base >= K || (q && rt[q].rec_base <= rt[q - 1].rec_base))
                return fail(c, MSIM_ERR_ARG, "msim_dbg_candidates: rec_base not strictly increasing below K, or set_id out of range");
    }
    if (k > cap || 2 * k > n_np) return fail(c, MSIM_ERR_ARG, "msim_dbg_candidates: more candidates than room, or fewer than two words each");
    *k_out = (uint32_t)k; *n_nsn = 0;
    if (!k) return MSIM_OK;                                // (the engines never plan a range without candidates, and a grid of no
                                                           //  workgroups is no launch: an empty bitmap comes back empty, unlaunched)
    const uint32_t ku = (uint32_t)k, nbk = (ku + CB_BLOCK - 1) / CB_BLOCK;
    DbgDev dev;
    uint64_t *d_bm = nullptr; uint32_t *d_cnt2 = nullptr, *d_np = nullptr, *d_pos = nullptr, *d_npos = nullptr, *d_nrank = nullptr, *d_cnt = nullptr;
    uint8_t *d_type = nullptr, *d_ntype = nullptr; MixRangeDev *d_rt = nullptr; TypeTable *d_sets = nullptr; PlanState *d_ps = nullptr;
    hipStream_t s = c->stream;
    MSIM_HIP(c, dev.get(&d_np, (size_t)n_np));
    MSIM_HIP(c, dev.get(&d_type, k)); MSIM_HIP(c, dev.get(&d_ntype, k)); MSIM_HIP(c, dev.get(&d_nrank, k));
    MSIM_HIP(c, dev.get(&d_cnt, (size_t)nbk + 2)); MSIM_HIP(c, dev.get(&d_ps, 1));
    MSIM_HIP(c, hipMemcpyAsync(d_np, np_raw, (size_t)n_np * 4, hipMemcpyHostToDevice, s));
    MSIM_HIP(c, hipMemsetAsync(d_ps, 0, sizeof(PlanState), s));
    if (bm) {
        MSIM_HIP(c, dev.get(&d_bm, n_words)); MSIM_HIP(c, dev.get(&d_cnt2, emit_cnt2_words(n_words)));
        MSIM_HIP(c, dev.get(&d_pos, k)); MSIM_HIP(c, dev.get(&d_npos, k));
        MSIM_HIP(c, hipMemcpyAsync(d_bm, bm, (size_t)n_words * 8, hipMemcpyHostToDevice, s));
        cand_front_launch(s, d_bm, n_words, d_cnt2, start, d, d_np, 0ull, sets[0], d_pos, d_type);
    } else {
        MSIM_HIP(c, dev.get(&d_rt, n_draw)); MSIM_HIP(c, dev.get(&d_sets, n_sets));
        MSIM_HIP(c, hipMemcpyAsync(d_rt, rt, (size_t)n_draw * sizeof(MixRangeDev), hipMemcpyHostToDevice, s));
        MSIM_HIP(c, hipMemcpyAsync(d_sets, sets, (size_t)n_sets * sizeof(TypeTable), hipMemcpyHostToDevice, s));
        types_multi_launch(s, d_np, 0ull, ku, d_rt, n_draw, d_sets, d_type);
    }
    nsn_compact_launch(s, d_pos, d_type, ku, d_cnt, d_npos, d_ntype, d_nrank, d_ps, all != 0);
    MSIM_HIP(c, hipGetLastError());
    PlanState h;
    MSIM_HIP(c, hipMemcpyAsync(&h, d_ps, sizeof h, hipMemcpyDeviceToHost, s));
    MSIM_HIP(c, wait_stream(s));
    if (h.n_nsn > ku) return fail(c, MSIM_ERR_HIP, "msim_dbg_candidates: more chain candidates than candidates");
    *n_nsn = h.n_nsn;
    if (bm) MSIM_HIP(c, hipMemcpyAsync(cand_pos, d_pos, k * 4, hipMemcpyDeviceToHost, s));
    MSIM_HIP(c, hipMemcpyAsync(cand_type, d_type, k, hipMemcpyDeviceToHost, s));
    if (h.n_nsn) {
        if (bm) MSIM_HIP(c, hipMemcpyAsync(nsn_pos, d_npos, (size_t)h.n_nsn * 4, hipMemcpyDeviceToHost, s));
        MSIM_HIP(c, hipMemcpyAsync(nsn_type, d_ntype, (size_t)h.n_nsn, hipMemcpyDeviceToHost, s));
        MSIM_HIP(c, hipMemcpyAsync(nsn_rank, d_nrank, (size_t)h.n_nsn * 4, hipMemcpyDeviceToHost, s));
    }
    MSIM_HIP(c, wait_stream(s));
    return MSIM_OK;
}

// Both accept-table kernels over RAW CPython-stream words [p0, p0 + n): k_accept_tables at p0, k_accept_tables_ps behind
// k_set_pos(p0).  T / T_ps: (n + 1) << lg_rows entries each, zero where the kernels write nothing (rows >= the class count).
int gpu_dbg_accept_tables(Ctx *c, const uint32_t *raw, uint64_t n_words, uint64_t p0, uint32_t n, const uint32_t *sh,
                          const uint32_t *width, uint32_t n_classes, uint32_t *T, uint32_t *T_ps) {
    ChainClasses cc;
    if (!T || !T_ps || (n_words && !raw) || n > (1u << 26) || p0 > n_words || n > n_words - p0 || !dbg_chain_classes(sh, width, n_classes, cc))
        return fail(c, MSIM_ERR_ARG, "msim_dbg_accept_tables: window outside the words given, or a class that is no (32 - bit_length(width), width) pair of a table entry");
    const uint32_t lg = chain_lg_rows(cc);
    const size_t n_slots = ((size_t)n + 1) << lg;
    DbgDev dev;
    uint32_t *d_raw = nullptr, *d_T = nullptr, *d_Tps = nullptr; PlanState *d_ps = nullptr;
    hipStream_t s = c->stream;
    MSIM_HIP(c, dev.get(&d_raw, (size_t)n_words)); MSIM_HIP(c, dev.get(&d_T, n_slots)); MSIM_HIP(c, dev.get(&d_Tps, n_slots));
    MSIM_HIP(c, dev.get(&d_ps, 1));
    if (n_words) MSIM_HIP(c, hipMemcpyAsync(d_raw, raw, (size_t)n_words * 4, hipMemcpyHostToDevice, s));
    MSIM_HIP(c, hipMemsetAsync(d_T, 0, n_slots * 4, s));
    MSIM_HIP(c, hipMemsetAsync(d_Tps, 0, n_slots * 4, s));
    MSIM_HIP(c, hipMemsetAsync(d_ps, 0, sizeof(PlanState), s));
    accept_tables_launch(s, d_raw, (unsigned long long)p0, n, cc, lg, d_T);
    hipLaunchKernelGGL(k_set_pos, dim3(1), dim3(1), 0, s, d_ps, (unsigned long long)p0);
    accept_tables_ps_launch(s, d_raw, d_ps, n, cc, lg, d_Tps);
    MSIM_HIP(c, hipGetLastError());
    MSIM_HIP(c, hipMemcpyAsync(T, d_T, n_slots * 4, hipMemcpyDeviceToHost, s));
    MSIM_HIP(c, hipMemcpyAsync(T_ps, d_Tps, n_slots * 4, hipMemcpyDeviceToHost, s));
    MSIM_HIP(c, wait_stream(s));
    return MSIM_OK;
}

// Steps 3 and 4 of an SV-mix plan (mixed_emit's launches) over the caller's candidates and chain verdicts: k_stop_scatter,
// k_link_scatter (ch_extra / ch_aux given), keep_flags_launch, emit_records_launch.  L: the contig's length.  recs / rec_off /
// sn_index hold k entries, pool cap_pool bytes; counts[0..2] = n_rec, n_sn, pool_len.
int gpu_dbg_mixed_emit(Ctx *c, uint64_t L, uint32_t k, const uint32_t *cand_pos, const uint8_t *cand_type, uint32_t n_ch,
                       const uint32_t *ch_rank, const uint32_t *ch_stop, const uint32_t *ch_extra, const uint8_t *ch_aux,
                       uint32_t n_draw, const void *rt_v, const uint32_t *visit_from, uint32_t sn_chained, const uint32_t *np_raw,
                       uint64_t n_np, msim_record *recs, uint32_t *rec_off, uint32_t *sn_index, uint8_t *pool, uint64_t cap_pool,
                       uint32_t *counts, int64_t *len_delta) {
    const MixRangeDev *rt = static_cast<const MixRangeDev *>(rt_v);
    const msim_params &P = c->params;
    const bool has_tl = ch_extra != nullptr;
    if (!c->have_params || k < 1 || k > (1u << 28) || L < 1 || L >= (1ull << 32) || !cand_pos || !cand_type || n_ch > k ||
        (n_ch && (!ch_rank || !ch_stop)) || (ch_extra != nullptr) != (ch_aux != nullptr) || sn_chained > 1 || (n_np && !np_raw) ||
        (rt != nullptr) != (visit_from != nullptr) || (rt ? n_draw < 1 : n_draw != 0) || !recs || !rec_off || !sn_index || !counts ||
        !len_delta || (cap_pool && !pool))
        return fail(c, MSIM_ERR_ARG, "msim_dbg_mixed_emit: bad argument");
    for (int t = 1; t <= 7; t++)
        if (P.block[t] < 0) return fail(c, MSIM_ERR_ARG, "msim_dbg_mixed_emit: negative block");
    // ---- what the planners guarantee
    std::vector<uint32_t> stop(k, CHAIN_DROPPED), extra(k, 0);
    std::vector<uint8_t> aux(k, 0);
    {
        uint32_t q = 0;
        for (uint32_t j = 0; j < k; j++) {
            const uint8_t t = cand_type[j];
            if (t < 1 || t > 7 || cand_pos[j] >= L || (j && cand_pos[j] <= cand_pos[j - 1]))
                return fail(c, MSIM_ERR_ARG, "msim_dbg_mixed_emit: types 1..7 at strictly increasing positions below the contig's length");
            if ((t == MSIM_TL || t == MSIM_TLI) && !has_tl)
                return fail(c, MSIM_ERR_ARG, "msim_dbg_mixed_emit: a translocation without ch_extra / ch_aux");
            // off the chain an SNP must not block: sample_with_minimum_distance leaves more than block[SN] = d between positions
            if (!sn_chained && j && cand_type[j - 1] == MSIM_SN && (int64_t)cand_pos[j] - (int64_t)cand_pos[j - 1] <= P.block[MSIM_SN])
                return fail(c, MSIM_ERR_ARG, "msim_dbg_mixed_emit: without sn_chained an SNP could block its successor");
            if (t == MSIM_SN && !sn_chained) continue;
            if (q >= n_ch || ch_rank[q] != j)
                return fail(c, MSIM_ERR_ARG, "msim_dbg_mixed_emit: ch_rank does not list exactly the chain's candidates, in order");
            const uint32_t s = ch_stop[q];
            if (has_tl) { extra[j] = ch_extra[q]; aux[j] = ch_aux[q]; }
            q++;
            stop[j] = s;
            if ((aux[j] & ~(CHAIN_TOMBSTONE | 3u)) || ((aux[j] & CHAIN_TOMBSTONE) && t != MSIM_TL && t != MSIM_TLI) || ((aux[j] & 3u) && t != MSIM_TLI))
                return fail(c, MSIM_ERR_ARG, "msim_dbg_mixed_emit: ch_aux flags outside what linking sets");
            if (s == CHAIN_DROPPED) continue;
            bool ok;
            if (t == MSIM_TLI) ok = s < L && extra[j] < L;                       // the linked TL's span (or stop 0: unlinked)
            else if (t == MSIM_SN) ok = s == cand_pos[j];
            else if (t == MSIM_IN) ok = s >= cand_pos[j] && s < 0xfffffffeu;     // (an insert's stop is a length, not a place)
            else ok = s >= cand_pos[j] && s < L;
            if (!ok) return fail(c, MSIM_ERR_ARG, "msim_dbg_mixed_emit: a stop that is neither CHAIN_DROPPED nor in [pos, 2^32 - 1) within the contig");
        }
        if (q != n_ch) return fail(c, MSIM_ERR_ARG, "msim_dbg_mixed_emit: ch_rank lists candidates off the chain");
    }
    if (rt) {
        if (rt[0].rec_base != 0) return fail(c, MSIM_ERR_ARG, "msim_dbg_mixed_emit: the range table starts at candidate 0");
        for (uint32_t r = 0; r < n_draw; r++) {
            const uint32_t a = rt[r].rec_base, b = r + 1 < n_draw ? rt[r + 1].rec_base : k;
            if (a >= b || b > k || cand_pos[b - 1] >= rt[r].clip || (b < k && rt[r].clip > cand_pos[b]))
                return fail(c, MSIM_ERR_ARG, "msim_dbg_mixed_emit: rec_base not strictly increasing below k, or a clip that does not part its range from the next");
        }
    }
    // (visit_from is taken as given: any value is memory-safe, and only a boundary pass can say which ones are consistent --
    //  tests/mixed_ref.py derives it from the same run as the stops)
    // The keep rule, sequentially -- k_keep_flags' own arithmetic, NOT an independent check of it: it sizes the output buffers and
    // bounds the kernels' 32-bit sums.
    uint64_t n_rec = 0, n_ins = 0;
    long long shift = 0;
    {
        BlockTable bt{};
        for (int t = 1; t <= 7; t++) bt.p1[t] = (uint32_t)std::min<int64_t>(P.block[t] + 1, 0xffffffffll);
        uint32_t run = 0, r = 0;
        for (uint32_t j = 0; j < k; j++) {
            uint32_t clip = 0xffffffffu;
            bool vis = true;
            if (rt) {
                while (r + 1 < n_draw && rt[r + 1].rec_base <= j) r++;
                clip = rt[r].clip;
                vis = cand_pos[j] >= visit_from[r];
            }
            const uint8_t t = cand_type[j];
            bool keep;
            if (t == MSIM_SN) keep = (sn_chained ? stop[j] != CHAIN_DROPPED : cand_pos[j] >= run) && vis;
            else keep = stop[j] != CHAIN_DROPPED && vis && !(aux[j] & CHAIN_TOMBSTONE);
            run = std::max(run, std::min(clip, blocked_end(cand_pos[j], t, stop[j], bt)));
            if (!keep) continue;
            const long long off = (long long)cand_pos[j] + shift;
            if (off < 0 || off >= (1ll << 32)) return fail(c, MSIM_ERR_ARG, "msim_dbg_mixed_emit: an output offset outside [0, 2^32)");
            n_rec++;
            if (t == MSIM_IN) n_ins += (uint64_t)stop[j] - cand_pos[j] + 1;
            shift += record_delta(t, cand_pos[j], t == MSIM_SN ? cand_pos[j] : stop[j], extra[j]);
        }
        const long long out_len = (long long)L + shift;
        if (out_len < 0 || out_len >= (1ll << 32) || n_ins >= (1ull << 32) || n_ins > n_np || n_ins > cap_pool)
            return fail(c, MSIM_ERR_ARG, "msim_dbg_mixed_emit: mutated length or insert bases outside [0, 2^32), or fewer words / less room than insert bases");
    }
    // ---- device
    const uint32_t nbk = (k + CB_BLOCK - 1) / CB_BLOCK;
    DbgDev dev;
    uint32_t *d_pos = nullptr, *d_stop = nullptr, *d_extra = nullptr, *d_crank = nullptr, *d_cstop = nullptr, *d_cextra = nullptr, *d_cnt = nullptr,
             *d_snidx = nullptr, *d_visit = nullptr, *d_np = nullptr, *d_off = nullptr;
    uint8_t *d_type = nullptr, *d_aux = nullptr, *d_caux = nullptr, *d_pool = nullptr;
    MixRangeDev *d_rt = nullptr; PlanState *d_ps = nullptr; msim_record *d_recs = nullptr;
    hipStream_t s = c->stream, es = c->emit_stream;
    MSIM_HIP(c, dev.get(&d_pos, k)); MSIM_HIP(c, dev.get(&d_type, k)); MSIM_HIP(c, dev.get(&d_stop, k));
    MSIM_HIP(c, dev.get(&d_crank, n_ch)); MSIM_HIP(c, dev.get(&d_cstop, n_ch));
    MSIM_HIP(c, dev.get(&d_cnt, mixed_cnt_bytes(nbk) / 4)); MSIM_HIP(c, dev.get(&d_snidx, k)); MSIM_HIP(c, dev.get(&d_np, (size_t)n_np));
    MSIM_HIP(c, dev.get(&d_ps, 1)); MSIM_HIP(c, dev.get(&d_recs, std::max<uint64_t>(n_rec, 1))); MSIM_HIP(c, dev.get(&d_off, std::max<uint64_t>(n_rec, 1)));
    MSIM_HIP(c, dev.get(&d_pool, (size_t)n_ins + 2 * PAD));
    MSIM_HIP(c, hipMemcpyAsync(d_pos, cand_pos, (size_t)k * 4, hipMemcpyHostToDevice, s));
    MSIM_HIP(c, hipMemcpyAsync(d_type, cand_type, (size_t)k, hipMemcpyHostToDevice, s));
    MSIM_HIP(c, hipMemsetAsync(d_stop, 0xee, (size_t)k * 4, s));          // (the engines leave the SNPs' entries unwritten too)
    MSIM_HIP(c, hipMemsetAsync(d_ps, 0, sizeof(PlanState), s));
    if (n_np) MSIM_HIP(c, hipMemcpyAsync(d_np, np_raw, (size_t)n_np * 4, hipMemcpyHostToDevice, s));
    if (n_ch) {
        MSIM_HIP(c, hipMemcpyAsync(d_crank, ch_rank, (size_t)n_ch * 4, hipMemcpyHostToDevice, s));
        MSIM_HIP(c, hipMemcpyAsync(d_cstop, ch_stop, (size_t)n_ch * 4, hipMemcpyHostToDevice, s));
        stop_scatter_launch(s, d_crank, d_cstop, n_ch, d_stop);
    }
    if (has_tl) {
        MSIM_HIP(c, dev.get(&d_extra, k)); MSIM_HIP(c, dev.get(&d_aux, k)); MSIM_HIP(c, dev.get(&d_cextra, n_ch)); MSIM_HIP(c, dev.get(&d_caux, n_ch));
        MSIM_HIP(c, hipMemsetAsync(d_extra, 0xee, (size_t)k * 4, s));
        MSIM_HIP(c, hipMemsetAsync(d_aux, 0, (size_t)k, s));
        if (n_ch) {
            MSIM_HIP(c, hipMemcpyAsync(d_cextra, ch_extra, (size_t)n_ch * 4, hipMemcpyHostToDevice, s));
            MSIM_HIP(c, hipMemcpyAsync(d_caux, ch_aux, (size_t)n_ch, hipMemcpyHostToDevice, s));
            link_scatter_launch(s, d_crank, d_cextra, d_caux, n_ch, d_extra, d_aux);
        }
    }
    if (rt) {
        MSIM_HIP(c, dev.get(&d_rt, n_draw)); MSIM_HIP(c, dev.get(&d_visit, n_draw));
        MSIM_HIP(c, hipMemcpyAsync(d_rt, rt, (size_t)n_draw * sizeof(MixRangeDev), hipMemcpyHostToDevice, s));
        MSIM_HIP(c, hipMemcpyAsync(d_visit, visit_from, (size_t)n_draw * 4, hipMemcpyHostToDevice, s));
    }
    const MixedTables mt{k, d_pos, d_type, d_stop, d_extra, d_aux, d_cnt, d_snidx, d_rt, n_draw, d_visit, sn_chained != 0};
    keep_flags_launch(s, P, mt, d_ps);
    MSIM_HIP(c, hipGetLastError());
    PlanState h;
    MSIM_HIP(c, hipMemcpyAsync(&h, d_ps, sizeof h, hipMemcpyDeviceToHost, s));
    MSIM_HIP(c, wait_stream(s));
    counts[0] = h.n_rec; counts[1] = h.n_sn; counts[2] = h.pool_len; *len_delta = h.len_delta;
    // the buffers are sized by the host's count: a device count that differs is reported, and nothing is emitted into them
    if (h.n_rec != n_rec || h.pool_len != n_ins || h.n_sn > h.n_rec)
        return fail(c, MSIM_ERR_HIP, "msim_dbg_mixed_emit: the device kept " + std::to_string(h.n_rec) + " records (" + std::to_string(h.n_sn) + " SNPs, " +
                                     std::to_string(h.pool_len) + " insert bases), the keep rule on the host " + std::to_string(n_rec) + " (" +
                                     std::to_string(n_ins) + " insert bases)");
    emit_records_launch(es, mt, d_recs, d_off, d_np, 0ull, h.pool_len, d_pool + PAD);
    MSIM_HIP(c, hipGetLastError());
    if (n_rec) {
        MSIM_HIP(c, hipMemcpyAsync(recs, d_recs, (size_t)n_rec * sizeof(msim_record), hipMemcpyDeviceToHost, es));
        MSIM_HIP(c, hipMemcpyAsync(rec_off, d_off, (size_t)n_rec * 4, hipMemcpyDeviceToHost, es));
    }
    if (h.n_sn) MSIM_HIP(c, hipMemcpyAsync(sn_index, d_snidx, (size_t)h.n_sn * 4, hipMemcpyDeviceToHost, es));
    if (n_ins) MSIM_HIP(c, hipMemcpyAsync(pool, d_pool + PAD, (size_t)n_ins, hipMemcpyDeviceToHost, es));
    MSIM_HIP(c, wait_stream(es));
    return MSIM_OK;
}

// test hook: which of the context's streams still have work queued (hipStreamQuery; never blocks)
void gpu_plan_stream_status(Ctx *c, GpuPlan *g, int out[8]) {
    auto q = [](hipStream_t s) { if (!s) return -1; const hipError_t e = hipStreamQuery(s); (void)hipGetLastError(); return e == hipSuccess ? 0 : e == hipErrorNotReady ? 1 : 2; };
    out[0] = q(c->stream); out[1] = q(c->emit_stream); out[2] = q(g->gen_stream); out[3] = q(g->jump_stream);
    out[4] = (int)g->s[0].n_chunks; out[5] = (int)g->s[0].n_states; out[6] = (int)g->s[0].ready_ev.size(); out[7] = (int)g->s[0].waited_chunks;
}

}  // namespace msim
