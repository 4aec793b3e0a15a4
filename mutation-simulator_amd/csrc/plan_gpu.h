// GPU sampler interface (plan_gpu.hip)
#pragma once
#include "ctx.h"
#include "plan_windows.h"

namespace msim {

struct GpuPlan;
GpuPlan *gpu_plan_create();
void gpu_plan_destroy(GpuPlan *g);
// host generator states changed (msim_seed / msim_set_mt_state / host planner ran): drop device streams
void gpu_plan_invalidate(GpuPlan *g);
// bring the host generators up to the device streams' positions (before the host planner runs or
// msim_get_mt_state answers)
int gpu_plan_sync_to_host(Ctx *c, GpuPlan *g);
// optional sizing hint: generate at least this many words ahead on the first extension
void gpu_plan_reserve(GpuPlan *g, uint64_t py_words, uint64_t np_words);
// wait for everything enqueued, collect flags + exact stream position (no-op if nothing is pending)
// ride_errs (the context's drain): what apply_finish reads next -- every contig's KeyError and length words -- is copied on the
// emit stream BEFORE the host waits here, so that the device's last operation is that copy and the host blocks once
int gpu_plan_finish(Ctx *c, GpuPlan *g, bool ride_errs = false);
bool gpu_plan_eligible(const Ctx *c, const msim_range *ranges, int n_ranges);
int plan_contig_gpu(Ctx *c, GpuPlan *g, Contig &ct, const msim_range *ranges, int n_ranges);
// SV mixes (SNPs + IN/DE/DU/IV on one large range): sample, type draw, filter, records, insert pool and SNP
// draws on the device; only the boundary chain over the non-SNP candidates runs on the host
bool gpu_plan_mixed_eligible(const Ctx *c, const msim_range *ranges, int n_ranges);
int plan_contig_gpu_mixed(Ctx *c, GpuPlan *g, Contig &ct, const msim_range *ranges, int n_ranges);
// deterministic-SNP ranges of any size and number (RMT mode): the host walks the chain of samples over words the
// device generated; records, SNP draws and APPLY stay on the device
bool gpu_plan_hostsample_eligible(const Ctx *c, const msim_range *ranges, int n_ranges);
int plan_contig_gpu_hostsample(Ctx *c, GpuPlan *g, Contig &ct, const msim_range *ranges, int n_ranges);
// everything else that is still a plain chain: several ranges with their own settings, SV types on many small ranges,
// SNP block above the sampling distance -- the host walks samples and boundary passes in one go over device-made
// words, accept tables and candidate types
bool gpu_plan_multimix_eligible(const Ctx *c, GpuPlan *g, uint64_t L, const msim_range *ranges, int n_ranges);
int plan_contig_gpu_multimix(Ctx *c, GpuPlan *g, Contig &ct, const msim_range *ranges, int n_ranges);
// SNP sampler: contigs with one drawing range queue their emission (records, SNP outcomes) and go through its stages in groups;
// gpu_emit_flush sends what is queued (every entry point that needs a result does), gpu_emit_pending tells whether a contig is
// still queued (mark_apply: its APPLY follows its group's emission -- msim_apply_contig)
int gpu_emit_flush(Ctx *c);
bool gpu_emit_pending(Ctx *c, int contig, bool mark_apply);
// test support (msim_dbg_emit_train): one group's train over the caller's bitmaps and outcomes
int gpu_dbg_emit_train(Ctx *c, int n_jobs, const uint64_t *const *bm, const uint32_t *n_words, const uint32_t *start,
                       const uint64_t *len, const uint8_t *const *aux8, uint32_t d, int train, uint32_t tile_shift,
                       msim_record *const *recs, const uint64_t *cap_recs, uint64_t *n_recs, int32_t *const *first);
// test support (msim_dbg_snp_draws): the SNP transducer's map, scan and outcome passes over the caller's words
int gpu_dbg_snp_draws(Ctx *c, const uint32_t *words, uint64_t n_words, uint64_t ti_lim, uint64_t start, uint32_t K, uint32_t aux_off,
                      uint32_t *lanes, uint32_t *maps, uint64_t *end_pos, uint32_t *flags, uint8_t *aux);
// test support (msim_dbg_sample_tail): one launch of the sampler's tail rounds + cut over the caller's tables
int gpu_dbg_sample_tail(Ctx *c, const uint32_t *words, uint64_t n_words, const uint32_t *acc, uint64_t n_acc, uint32_t acc_first,
                        const uint32_t *blocks, uint32_t n_blocks, uint32_t raw_counts, uint32_t W, uint32_t shift, uint32_t n,
                        uint32_t k, uint32_t *bitmap, uint32_t bm_guard, msim_dbg_tail_state *state, int anchored, uint64_t win_pos,
                        uint32_t need0, uint32_t d1, uint64_t pos_limit);
// test support (msim_dbg_chain_step): one anchored contig's chain -- fringe, tail, both cuts -- over the caller's tables, as the one
// fused launch or as the three stand-alone ones; msim_dbg_chains_fused: fused launches the context's sampler has sent
int gpu_dbg_chain_step(Ctx *c, const uint32_t *words, uint64_t n_words, const uint32_t *hcnt, const uint32_t *hacc, uint64_t n_hacc,
                       const uint32_t *tail, uint64_t n_tail, const uint32_t *cnt, uint32_t *bitmap, uint32_t *win_maps,
                       msim_dbg_chain *io);
uint64_t gpu_plan_chains_fused(const GpuPlan *g);
// test support (msim_dbg_candidates / msim_dbg_accept_tables / msim_dbg_mixed_emit): the device halves of the SV-mix and host-chain
// engines -- the engines' own launch helpers -- over tables the caller made (plan_gpu.hip);
// rt: MixRangeDev[n_draw], sets: TypeTable[n_sets] (plan_kernels.h)
int gpu_dbg_candidates(Ctx *c, const uint64_t *bm, uint32_t n_words, uint32_t start, uint32_t d, uint32_t K, const void *rt,
                       uint32_t n_draw, const void *sets, uint32_t n_sets, const uint32_t *np_raw, uint64_t n_np, uint32_t all,
                       uint32_t *cand_pos, uint8_t *cand_type, uint32_t *nsn_pos, uint8_t *nsn_type, uint32_t *nsn_rank, uint64_t cap,
                       uint32_t *k_out, uint32_t *n_nsn);
int gpu_dbg_accept_tables(Ctx *c, const uint32_t *raw, uint64_t n_words, uint64_t p0, uint32_t n, const uint32_t *sh,
                          const uint32_t *width, uint32_t n_classes, uint32_t *T, uint32_t *T_ps);
int gpu_dbg_mixed_emit(Ctx *c, uint64_t L, uint32_t k, const uint32_t *cand_pos, const uint8_t *cand_type, uint32_t n_ch,
                       const uint32_t *ch_rank, const uint32_t *ch_stop, const uint32_t *ch_extra, const uint8_t *ch_aux,
                       uint32_t n_draw, const void *rt, const uint32_t *visit_from, uint32_t sn_chained, const uint32_t *np_raw,
                       uint64_t n_np, msim_record *recs, uint32_t *rec_off, uint32_t *sn_index, uint8_t *pool, uint64_t cap_pool,
                       uint32_t *counts, int64_t *len_delta);
int gpu_plan_force_overflow(Ctx *c, GpuPlan *g);          // test support
void gpu_plan_abandon(GpuPlan *g);                        // a device engine failed mid-contig: the session is over
// before a contig goes to a device engine: room for its windows in the current session's jump-table span, re-basing the session
// where there is not (*fits = false: no span holds it -- the host planner's)
int gpu_plan_make_room(Ctx *c, GpuPlan *g, const msim_range *ranges, int n_ranges, bool *fits);
// ... and the need itself: words of the CPython and the NumPy stream the contig's windows can ask for (a pure function of its
// arguments, summed from plan_windows.h; bad: a range every device engine's eligibility refuses)
struct StreamNeed { double py, np; bool bad; };
StreamNeed stream_need(const msim_params &P, const msim_range *ranges, int n_ranges);

// msim_plan_pass: the leading items of items[0 .. n) whose samples' off-chain parts can go out ahead of their chains (the
// segmenting rule: plan_gpu.hip, pass_segment) get them enqueued, batched; plan_contig_gpu then finds them waiting when each
// contig's turn comes.  Nothing to hoist: nothing happens.  gpu_plan_pass_abort: the pass ended early -- what is still waiting
// is dropped, behind a wait for the prep streams.
int gpu_plan_pass_prep(Ctx *c, GpuPlan *g, const msim_pass_item *items, int n);
void gpu_plan_pass_abort(Ctx *c, GpuPlan *g);
bool gpu_plan_pass_hoisting(const GpuPlan *g);            // some hoisted sample still waits for its contig's turn
// test support (msim_dbg_pass_segments): the segmenting rule over an item list, pure host code
int gpu_dbg_pass_segments(const msim_params *P, const msim_pass_item *items, int n, uint64_t py_pos, uint64_t np_pos,
                          uint32_t max_chunks, int ahead, int32_t *seg);

void gpu_plan_stream_status(Ctx *c, GpuPlan *g, int out[8]);

// Mean and variance of the CPython stream's words one stage consumes -- what the SNP sampler's anchored windows lay out the
// interval of a sample's start from (plan_gpu.hip: plan_contig_gpu; checked against simulation in tests/test_ahead_moments.py).
//   sample: random.sample(range(n), k) by the set path draws until k DISTINCT values are there -- A accepted draws, a coupon
//     collector's first k: E A = sum n/(n-i) = -n ln(1 - k/n), Var A = sum (i/n)/(1-i/n)^2 = n (k/(n-k) + ln(1 - k/n)) --,
//     each after a geometric number of getrandbits(bits) words with success p = n / 2^bits (_randbelow's rejection):
//     E = E A / p, Var = E A (1-p)/p^2 + Var A / p^2
//   SNP draws of K SNPs (mutator.py:428-463): uniform() = 2 words; with probability p_tv a transversion's randint(0, 1) =
//     _randbelow(2) = getrandbits(2) until < 2, a geometric(1/2) loop: E = K (2 + 2 p_tv), Var = K (2 p_tv + 4 p_tv (1 - p_tv))
StreamMoments sample_words_moments(uint64_t n, uint64_t k);
StreamMoments snp_words_moments(uint64_t K, unsigned long long ti_lim);

}  // namespace msim
