/*
 * msim.h -- C-ABI of libmsim.so: the MI355X-native mutation-injection path.
 *
 * The reference (mkpython3/Mutation-Simulator 3.0.2) is pure Python and has NO plugin / FFI /
 * native boundary of its own: the hot path sits behind the Python class `Mutator`
 * (mutation_simulator/mutator.py:73-479, called from __main__.py:80-85).  This header is the
 * boundary a maintainer would bind with ctypes to replace that class's internals; each entry
 * point cites the reference code whose work it takes over (paths relative to
 * /root/reference/mutation_simulator/).  INTEGRATION.md shows the ctypes stub.
 *
 * Contract: plain C, opaque handle, caller-owned host buffers, int return codes (0 = ok) with
 * msim_last_error() for the text; one context per process/GPU; like the reference (a single
 * thread driving two global RNGs) a context is NOT thread-safe.  No Python, torch or HIP types
 * cross this line.  Everything floating point on the path (rate sums -> k, chances -> cdf, titv ->
 * p_ti) is evaluated by the caller with the reference's own Python expressions and arrives here
 * as integers (see msim_range / msim_params), so the device work is integer/byte only.
 *
 * Two phases -- possible because RNG use never depends on genome content:
 *   PLAN   two MT19937 streams -> a position-sorted table of 16-byte mutation records per contig
 *   APPLY  records + uint8 genome in HBM -> mutated uint8 stream in HBM (HBM-bandwidth bound)
 */
#ifndef MSIM_H
#define MSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSIM_ABI_VERSION 8

/* ---- return codes ---------------------------------------------------------------------------- */
#define MSIM_OK               0
#define MSIM_ERR_ARG          1   /* bad argument / call order                                      */
#define MSIM_ERR_HIP          2   /* HIP runtime failure (no device, OOM, launch error)             */
#define MSIM_ERR_VALUE        3   /* reference raises ValueError("Sample larger than population or
                                     is negative") -- util.py:104 via random.sample                */
#define MSIM_ERR_KEY          4   /* reference raises KeyError(base): transversion of a base outside
                                     A,G,T,C,N -- mutator.py:449-455; see msim_key_error()         */
#define MSIM_ERR_UNSUPPORTED  5   /* valid for the reference, outside this build: contigs (or their mutated
                                     form) of 4 GiB and more, 2^31 mutations on one contig, an output file
                                     that cannot be written at an offset, MSIM_PLAN_GPU forced on a contig
                                     no device engine takes (README "Limits")                          */
#define MSIM_ERR_NOMEM        6
#define MSIM_ERR_IO           7   /* a write queued by the *_file entry points failed (msim_last_error)   */

/* ---- mutation types: numerically identical to mut_types.py:6-12 --------------------------------- */
#define MSIM_SN  1
#define MSIM_IN  2
#define MSIM_DE  3
#define MSIM_DU  4
#define MSIM_IV  5
#define MSIM_TL  6
#define MSIM_TLI 7

/* ---- msim_create flags --------------------------------------------------------------------- */
#define MSIM_PLAN_AUTO   0u      /* per contig: a device PLAN engine where one applies, else the host planner */
#define MSIM_PLAN_HOST   1u      /* force the sequential host planner (cross-check / debugging)               */
#define MSIM_PLAN_GPU    2u      /* force a device engine; MSIM_ERR_UNSUPPORTED where none can run             */
#define MSIM_RNG_FAST    4u      /* NOT stream-compatible with the reference: a counter-based generator (Philox4x32-10) replaces
                                    the two MT19937 streams, so that no draw depends on another one, PLAN has no sequential chain
                                    and the host does nothing (csrc/plan_fast.hip, fast_math.h).  The CONSTRUCTION is the
                                    reference's -- k = int(len * rate) candidates per range as a uniform k-subset with the minimum
                                    distance (util.py:93-109), a type per candidate from the range's chances, a uniform length,
                                    IV dropped / DU, DE clamped at the contig end, the boundary pass with its blocked ranges reset
                                    per range (mutator.py:144-265), the rewrite's visit rule, transition with probability p_ti,
                                    insert bases uniform in ATGC -- same distributions, different numbers.  SN / IN / DE / DU / IV
                                    on any number of sorted, non-overlapping ranges; translocations and overlapping RMT ranges:
                                    MSIM_ERR_UNSUPPORTED; a sample larger than its population: MSIM_ERR_VALUE like the reference.
                                    msim_seed / msim_set_mt_state are ignored, msim_set_fast_key seeds it.  msim_plan_contig only
                                    QUEUES the contig; everything queued goes to the device as one batch (one launch per stage over
                                    all contigs) at the next call that needs a result -- plan a whole genome, then ask.        */
/* Device PLAN engines: the device owns both MT19937 streams and does all per-record work;
 * SNP-only large ranges need nothing from the host, SV mixes hand the boundary chain over their non-SNP
 * candidates to the host, contigs with many small SNP ranges hand it the chain of sample() calls, contigs whose
 * ranges have their own SV settings (or whose SNPs block) hand it both -- always over words the device generated.
 * Results are bit-identical whichever engine runs; msim_timing.contigs_* tells which one did.                  */

typedef struct msim_ctx msim_ctx;

/* One mutation -- the reference's `Mutation` object (mutator.py:26-50) in 16 bytes.
 * Positions are 0-based inclusive like the reference's.  Tables are sorted by pos and hold only
 * the mutations __mutate_sequence actually visits (entries swallowed by an earlier DE/IV/DU span,
 * mutator.py:376/386/398, are dropped: they draw no random numbers and emit nothing).            */
typedef struct msim_record {
    uint32_t pos;     /* Mutation.start (dict key)                                               */
    uint32_t stop;    /* Mutation.stop; for IN: pos + insert_len - 1 (mutator.py:344)            */
    uint32_t extra;   /* IN: offset of the insert's bases in the contig's insert pool;
                         TLI: Mutation.start of the linked TL span (stop = its Mutation.stop)        */
    uint8_t  type;    /* MSIM_SN .. MSIM_TLI                                                     */
    uint8_t  aux;     /* SN: 0 = transition, 1/2 = transversion table column 0/1 (mutator.py:428-463);
                         TLI: bit 0 = trans_reverse, bit 1 = trans_insert_pos > 0 (mutator.py:281-284) */
    uint16_t rsv;
} msim_record;

/* One RangeDefinition that has mutations (rmt.py:166-189 + MutationSettings rmt.py:79-163),
 * reduced to the integers __get_mutations (mutator.py:144-214) needs.                            */
typedef struct msim_range {
    int64_t  start, stop;     /* 0-based inclusive                                                */
    int64_t  k;               /* int(((stop-start)+1) * sum(rates))           mutator.py:225       */
    int64_t  setsize;         /* CPython sample(): 21 + 4**ceil(log(3k,4)) if k>5 else 21          */
    int32_t  n_types;         /* len(mut_chances), dict order                 mutator.py:171-173   */
    int32_t  types[8];        /* MSIM_* ids in that order                                          */
    uint64_t cdf_thr[8];      /* ceil(cdf_j * 2^53), cdf = cumsum(p)/cumsum(p)[-1]: the type drawn
                                 for a 53-bit NumPy sample m is types[#{j: cdf_thr[j] <= m}]       */
    int64_t  min_len[8];      /* mut_lengs["min"/"max"], indexed by MSIM_* id                      */
    int64_t  max_len[8];
} msim_range;

/* SimulationSettings.mut_block / .titv (rmt.py:326-352) */
typedef struct msim_params {
    int64_t  block[8];        /* indexed by MSIM_* id; min over ids 1..7 is the sampling distance d */
    uint64_t ti_lim;          /* floor(p_ti * 2^53) + 1, p_ti = titv*(1/(titv+1)); 0 if p_ti is NaN:
                                 transition iff the 53-bit sample m < ti_lim  (p <= p_ti,
                                 mutator.py:436-438)                                               */
} msim_params;

typedef struct msim_timing {  /* milliseconds; device stages are HIP-event times on the ctx stream */
    double plan_host_ms;      /* host planner wall time (sequential RNG chain)                      */
    double plan_gpu_ms;       /* GPU sampler kernels                                                */
    double upload_ms;         /* record table H2D                                                   */
    double apply_ms;          /* APPLY kernels (scan + tile index + rewrite): the time during which */
    double apply_kernel_ms;   /* at least one was in flight; the rewrite kernel alone (roofline     */
                              /* kernel), likewise -- launches on different streams may overlap     */
    uint64_t apply_launches;  /* rewrite-kernel launches accumulated since msim_reset_stats         */
    uint64_t bytes_in, bytes_out, records;   /* algorithmic traffic of those launches               */
    uint64_t py_words, np_words;             /* MT19937 words consumed from each stream             */
    /* contigs planned per PLAN engine since msim_reset_stats: which engine a run went through   */
    uint64_t contigs_snp;        /* SNP sampler: everything on the device                                              */
    uint64_t contigs_svmix;      /* one large SV-mix range: the boundary chain on the host                             */
    uint64_t contigs_hostcut;    /* many deterministic-SNP ranges: the stream cuts on the host                         */
    uint64_t contigs_hostchain;  /* several ranges with their own settings / SNPs that block: samples + chain on the host */
    uint64_t contigs_host;       /* sequential host planner (translocations, overlapping ranges, tiny contigs)         */
    uint64_t contigs_batch;      /* contigs that went through msim_batch_run (host planner, one APPLY per batch)       */
    uint64_t contigs_fast;       /* MSIM_RNG_FAST contexts: contigs planned with the counter-based generator            */
    uint64_t stream_rebases;     /* device MT19937 sessions re-based: the jump tables span 8192 chunks (1.31 G words) from a
                                    session's origin; before a contig that would not fit, the state at the streams' exact
                                    positions becomes the next session's origin (no limit on a run's stream length)     */
    uint64_t snp_samples_ahead;  /* SNP sampler: samples -- of owned contigs and of contigs walked for their stream positions
                                    (msim_plan_chain) alike -- whose count / scatter / de-dup ran off the stream-position chain,
                                    on a window anchored at the host's bound of the start (every
                                    context's default since round 6, MSIM_AHEAD=1: sharded ranks only, MSIM_NO_AHEAD: never) */
    /* The host-sequential stages of the bit-compatible engines, apart from what surrounds them (round 6, ABI 8): a slower
       host core shows in host_walk_run_ms per item, a slower link or device in host_walk_wait_ms -- so that "slower box" and
       "slower code" can be told apart from one bench line.                                                              */
    double host_walk_run_ms;     /* the host walking: boundary chains (SV mix, host chain), stream cuts (host cut)        */
    double host_walk_wait_ms;    /* ... and waiting: for the mailbox, for the pieces of its word window / candidates      */
    uint64_t host_walk_candidates;  /* candidates those chains walked (SV mix: the non-SNP ones; host chain: all)        */
    uint64_t host_cut_words;     /* stream words the host-cut engine's cuts went through                                  */
    uint64_t snp_ahead_margin_permille;  /* anchored windows: the largest |exact start - expected start| of a sample planned
                                    ahead of the chain, in permille of the deviation the host allowed for (8 sigma + 256 words:
                                    1000 = the soft edge; beyond: MSIM_ERR_HIP, the caller re-plans) -- the maximum since
                                    msim_reset_stats / the session's start.  Telemetry of the moment model behind the windows */
} msim_timing;

/* ---- lifetime -------------------------------------------------------------------------------- */
int  msim_abi_version(void);
/* Initialise the HIP runtime for `device_id` (idempotent, thread-safe, no context): the first HIP call of a process costs
 * ~0.2 s; a caller with host work of its own to do first (reading and indexing the FASTA) runs this beside it.        */
int  msim_warm_up(int device_id);
/* The CPUs of the NUMA node the device hangs on, as a Linux cpulist ("64-127,192-255"; "" when the host has one node or sysfs
 * does not tell).  On a two-socket host a run whose host threads stay on the GPU's socket moves its bytes once across the
 * inter-socket links instead of twice (CLI end to end: 0.30 -> 0.25-0.27 s); libmsim pins its own output channels' threads
 * there (MSIM_IO_CPUS=none / a cpulist overrides), the caller decides about its own.  Initialises the HIP runtime.
 * It matters for the launching thread too: the queues' packets live in its node's memory -- a -sn 0.01 step over a 3 Gb
 * genome (~160 dependent launches) takes 4.2 ms from the GPU's socket and 4.4 ms from the other one.                   */
int  msim_device_host_cpus(int device_id, char *cpulist, int cap);
int  msim_create(int device_id, uint32_t flags, msim_ctx **out);     /* Mutator.__init__ mutator.py:79 */
void msim_destroy(msim_ctx *ctx);                                     /* Mutator.close    mutator.py:95 */
const char *msim_last_error(const msim_ctx *ctx);                     /* "" when none; ctx may be NULL  */
int  msim_device_name(const msim_ctx *ctx, char *dst, int cap);
int  msim_sync(msim_ctx *ctx);
/* Change the PLAN mode of a live context (0 = AUTO, MSIM_PLAN_HOST, MSIM_PLAN_GPU).  The host package uses it to
 * re-plan a contig through the sequential host planner when a device engine reports that a stream window
 * overflowed its margin -- 16 sigma; 8 for the interval in which a sample planned ahead of the stream-position chain
 * (msim_timing.snp_samples_ahead) expects its start -- (the streams are put back with msim_set_mt_state first). */
int  msim_set_plan_mode(msim_ctx *ctx, uint32_t mode);

/* ---- the two global RNGs the reference draws from ---------------------------------------------- */
/* random.seed(int) == init_by_array(little-endian 32-bit limbs of abs(seed));
 * numpy.random.seed(int) == init_genrand(seed).  (mutator.py:4,8; util.py:5)                      */
int msim_seed(msim_ctx *ctx, const uint32_t *py_key, int n_key, uint32_t np_seed);
/* Hand over / read back raw MT19937 states (random.getstate()[1], numpy.random.get_state()[1:3]) so a
 * caller that seeded the Python generators itself gets the reference's exact stream, and can put the
 * advanced state back afterwards.  stream: 0 = CPython `random`, 1 = numpy.random.                 */
int msim_set_mt_state(msim_ctx *ctx, int stream, const uint32_t mt[624], int pos);
int msim_get_mt_state(msim_ctx *ctx, int stream, uint32_t mt[624], int *pos);

/* Optional sizing hint for the GPU sampler: how many words of each stream the coming plan calls
 * will roughly consume, so stream chunks are generated in one batch.  Never changes results.      */
int msim_reserve_streams(msim_ctx *ctx, uint64_t py_words, uint64_t np_words);
/* MSIM_RNG_FAST contexts: the generator's key; also restarts the contig ordinal that every msim_plan_contig /
 * msim_plan_chain call advances (so ranks that skip contigs they do not own stay aligned with those that plan them). */
int msim_set_fast_key(msim_ctx *ctx, uint64_t key);

/* ---- genome in HBM ----------------------------------------------------------------------------- */
/* Upload one contig (upper-cased bases, what pyfaidx hands the reference: util.py:84-88).
 * Contigs are numbered in call order like fasta[i].                                                */
int msim_add_contig(msim_ctx *ctx, const uint8_t *bases_upper, uint64_t len, int *contig);
/* Synthesize i.i.d. uniform A/C/G/T directly in HBM, 32 bases per 64-bit hash:
 *   base(i) = "ACGT"[(mix64(seed + (i >> 5)) >> (2 * (i & 31))) & 3],   mix64 = the splitmix64 finaliser
 * (k_synth in csrc/apply.hip; host twin synth_host in tests/test_gpu_parity.py).  Benchmark input.          */
int msim_add_contig_synthetic(msim_ctx *ctx, uint64_t len, uint64_t seed, int *contig);
int msim_contig_length(msim_ctx *ctx, int contig, uint64_t *len);
int msim_read_contig(msim_ctx *ctx, int contig, uint64_t offset, uint64_t n, uint8_t *dst);
int msim_clear(msim_ctx *ctx);            /* drop all contigs and results, keep RNG states          */

/* ---- PLAN: Mutator.__get_mutations + the RNG draws of __mutate_sequence -------------------------- */
int msim_set_params(msim_ctx *ctx, const msim_params *params);
/* One iteration of mutate()'s contig loop up to the rewrite (mutator.py:111-131 + the SNP/insert
 * draws of :334-358 in position order).  Consumes both streams exactly as the reference does and
 * leaves the contig's record table (+ insert pool) in HBM.  Contigs must be planned in index order
 * -- the streams are chained across contigs.                                                       */
int msim_plan_contig(msim_ctx *ctx, int contig, const msim_range *ranges, int n_ranges);
/* The same iteration for a contig this process does NOT mutate (multi-GPU runs: a rank that does not own a contig):
 * both streams advance exactly as msim_plan_contig on a contig of `len` bases would leave them -- the chain across
 * contigs stays intact -- but no record table, insert pool or SNP outcome is produced and no contig is created.   */
int msim_plan_chain(msim_ctx *ctx, uint64_t len, const msim_range *ranges, int n_ranges);
/* A whole pass in one call: item by item exactly what the same sequence of msim_plan_contig / msim_plan_chain /
 * msim_apply_contig calls does, in item order -- records, insert pools, mutated streams, KeyError words, both stream positions,
 * msim_timing and the error codes come out the same, errors stay sticky and asynchronous, and the call returns at the first item
 * that fails (the items behind it are not planned).  What the call adds is knowledge of the contigs to come: for a run of
 * consecutive items that the SNP sampler plans from ONE drawing range with an anchored window (msim_timing.snp_samples_ahead),
 * the samples' count / scatter / de-dup -- which need only the host's bound of where each sample starts -- are enqueued for the
 * whole run first, eight samples a launch, and the contigs' stream-position chains follow as before.  A -sn 0.01 pass over a
 * 3 Gb genome then has no LDS-heavy kernel left to run beside its rewrite launches (NOTES section 31).
 * Such a run ends in front of an item of any other engine (SV mix, host cut, host chain, host planner, MSIM_RNG_FAST, a host-only
 * context), a sample that stays on the chain, an item in front of which the device streams' session would be re-based, and
 * after 24 items; everything else takes the per-contig path in its place in the order.  Always correct, faster only where it
 * can hoist.  MSIM_NO_PASS_HOIST=1: nothing is hoisted.  MSIM_PASS_BATCH / MSIM_PASS_FIRST: samples per prep launch (8) and in
 * a run's first one (1: the run's first chain waits for that launch alone).  MSIM_PASS_STREAMS / MSIM_PASS_GATE: schedule
 * experiments (NOTES section 31).                                                                                          */
#define MSIM_PASS_APPLY 1u             /* msim_apply_contig(contig) right behind the item's plan (contig >= 0)              */
typedef struct msim_pass_item {
    int32_t  contig;                   /* contig id, or -1: walk only (msim_plan_chain)                                    */
    uint32_t flags;                    /* MSIM_PASS_APPLY                                                                  */
    uint64_t len;                      /* contig == -1: its length                                                        */
    const msim_range *ranges;          /* as msim_plan_contig                                                              */
    int32_t  n_ranges;
    int32_t  rsv;
} msim_pass_item;
int msim_plan_pass(msim_ctx *ctx, const msim_pass_item *items, int n_items);
/* Test support: the rule that cuts a pass into those runs ("segments"), the very function msim_plan_pass calls, over an item list
 * alone -- pure host code, no context.  The streams are taken to stand exactly at py_pos / np_pos of a session that spans
 * max_chunks chunks (0: the jump tables' 8192); ahead: MSIM_AHEAD's value (2 = every context plans ahead).  seg[i] = 0: item i
 * takes the per-contig path; s >= 1: it belongs to the pass's s-th segment.  An item the SNP sampler does not take, and a re-base,
 * count as a synchronisation: the position behind them is exact.                                                            */
int msim_dbg_pass_segments(const msim_params *params, const msim_pass_item *items, int n_items, uint64_t py_pos, uint64_t np_pos,
                           uint32_t max_chunks, int ahead, int32_t *seg);
/* 1 if the last plan of this contig left `muts` empty (warning at mutator.py:125-129).             */
int msim_plan_was_empty(msim_ctx *ctx, int contig, int *empty);

/* ---- settings -> msim_range tables, natively ------------------------------------------------------ */
/* One MutationSettings object (rmt.py:79-163) as the reference holds it: floats stay floats until here.  */
typedef struct msim_settings_desc {
    double   rate_sum;        /* sum(mut_rates.values()) -- Python's left-to-right float sum, evaluated by the caller (one number) */
    int32_t  n_types;         /* len(mut_chances), dict order                                       */
    int32_t  types[8];        /* MSIM_* ids in that order                                            */
    double   chances[8];      /* mut_chances.values()                                                */
    int64_t  min_len[8];      /* mut_lengs["min"/"max"], indexed by MSIM_* id                        */
    int64_t  max_len[8];
} msim_settings_desc;
/* The msim_range table of a contig from its ranges' (start, stop, settings index) triples: what mutator.py:157-174,225 and
 * CPython's sample() derive per range, with the same IEEE operations --
 *   k        = (int64) ((double)(stop - start + 1) * rate_sum)                  int(((stop - start) + 1) * sum(rates))
 *   setsize  = 21 + 4^ceil(log4(3 k)) for k > 5, else 21, in integers (3 k is never a power of 4; exact for k < 2^33)
 *   cdf_thr  = ceil(cdf_j * 2^53), cdf = cumsum(chances) / cumsum(chances)[-1]  numpy.random.choice(p=...)
 * An RMT file in the style of the reference's examples gives a genome 35 000 ranges over three settings objects: this is
 * their marshalling, off the Python interpreter.  Pure host code, no context.  MSIM_ERR_ARG: a settings index out of range.  */
int msim_build_ranges(const msim_settings_desc *sets, int n_sets, const int64_t *start, const int64_t *stop,
                      const int32_t *set_id, int64_t n, msim_range *out);

/* ---- APPLY: Mutator.__mutate_sequence (mutator.py:318-426) -------------------------------------- */
/* Execution model: msim_plan_contig (SNP sampler engine) and msim_apply_contig (device-planned tables) only
 * ENQUEUE work -- the chain that fixes stream positions on one HIP stream, record emission and the rewrite
 * kernel on another, overlapping the next contig's chain.  (The SV-mix and host-cut engines wait inside
 * msim_plan_contig for the device data their host chain reads -- the boundary walk, the stream cuts.)  Deferred outcomes (the reference's KeyError, an
 * internal window overflow) are reported by the next call that synchronises: msim_sync,
 * msim_result_sizes(out_len), msim_fetch_*, msim_result_checksum, msim_get_mt_state, msim_stats, the text calls.
 * Enqueued does not mean launched at once: contigs the SNP sampler planned from ONE drawing range (ARGS mode) gather in groups
 * (fours by default) whose emission stages and rewrite go to the device as one launch each; the APPLYs of contigs
 * planned by an engine with a host chain wait for the walks of the contigs behind them and go out three at a time --
 * when the next msim_plan_contig arrives or at any other entry point, whichever comes first (plan + apply a whole genome,
 * then ask: that is the fast order; asking after every contig is as correct and launches per contig).                  */
int msim_apply_contig(msim_ctx *ctx, int contig);
/* If apply hit the reference's KeyError: the offending (ambiguity-converted) base and position.
 * contig == -1: the first contig (in index order) that hit it.                                    */
int msim_key_error(msim_ctx *ctx, int contig, uint8_t *base, uint64_t *pos);

int msim_result_sizes(msim_ctx *ctx, int contig, uint64_t *out_len, uint64_t *n_records,
                      uint64_t *insert_pool_len);
int msim_fetch_sequence(msim_ctx *ctx, int contig, uint64_t offset, uint64_t n, uint8_t *dst);
int msim_fetch_records(msim_ctx *ctx, int contig, msim_record *dst, uint8_t *insert_pool_dst);
/* 64-bit FNV-style checksum of the mutated stream computed on the device (parity at full size).   */
int msim_result_checksum(msim_ctx *ctx, int contig, uint64_t *sum);
int msim_release_result(msim_ctx *ctx, int contig);
/* Device address of the mutated stream (valid until the contig is re-applied / released / cleared), for
 * communication layers that move results GPU-to-GPU (RCCL gather of sharded contigs).
 * Synchronises like msim_fetch_sequence.                                                            */
int msim_result_device_ptr(msim_ctx *ctx, int contig, uint64_t *device_address, uint64_t *len);

/* ---- VCF text (vcf_writer.py:118-126 + record construction mutator.py:334-399) ------------------ */
/* Render the record lines of one contig.  Stateless host helper: `bases` is the INPUT contig.
 * Call with out == NULL to get the size.  Lines whose REF == ALT are suppressed like the reference. */
int msim_render_vcf(const msim_record *recs, uint64_t n_records, const uint8_t *insert_pool,
                    const uint8_t *bases, uint64_t len, const char *seq_name,
                    char *out, uint64_t cap, uint64_t *needed);

/* The same lines with a phased genotype column: gt[i] is record i's genotype byte (bit 0: on haplotype 1, bit 1: on haplotype 2;
 * 1, 2 or 3 -- anything else: MSIM_ERR_ARG) and its line ends in "GT\t1|0", "0|1" or "1|1".  Indexed by RECORD: a suppressed
 * line shifts nothing.  gt == NULL: msim_render_vcf's bytes.  The cross-check of the device text of a genotyped contig.   */
int msim_render_vcf_gt(const msim_record *recs, const uint8_t *gt, uint64_t n_records, const uint8_t *insert_pool,
                       const uint8_t *bases, uint64_t len, const char *seq_name, char *out, uint64_t cap, uint64_t *needed);

/* ---- diploid runs: two haplotypes of one record table (csrc/haplotype.hip) ------------------------------------------------ */
/* A record table is a list of independent edits -- no record consumes input another one consumes, a TLI copies its span from
 * the INPUT -- so any subset of it is a table APPLY takes.  A diploid run plans once, gives every record a GENOTYPE byte (bit 0:
 * on haplotype 1, bit 1: on haplotype 2; never 0) kept beside the table (msim_record.rsv stays 0), and applies the two subsets.
 *   msim_genotype_contig   draws the genotypes of a planned contig's table on the device; synchronises like msim_fetch_records
 *                          (pending emission groups are flushed, device-side sizes collected).  Philox4x32-10, counter
 *                          (record index in the full table, 0, seq, tag 20), key = the 64-bit `key`; neither MT19937 stream moves:
 *                            heterozygous iff (low 64 bits >> 11) < het_thr   het_thr = ceil(F * 2^53) <= 2^53, the caller's float
 *                            phase = bit 0 of the high 64 bits                0: haplotype 1, 1: haplotype 2
 *                          else the record is on both.  A TLI takes the draw of the TL record whose pos is its `extra` (a
 *                          translocation moves as a whole); without such a record in the table it keeps its own.
 *   msim_set_genotypes / msim_fetch_genotypes   install / read the array (one byte per record of the FULL table; a value
 *                          outside 1..3: MSIM_ERR_ARG).  Fetching from a contig without genotypes: MSIM_ERR_ARG.
 *   msim_select_haplotype  hap 1 or 2: the records with that bit set, in table order, become the contig's ACTIVE table -- same
 *                          pos / stop / extra / type / aux, same insert pool, host-known size; msim_apply_contig takes it through
 *                          the device scan.  hap 0: the full table is the active one again.  The active table is what
 *                          msim_apply_contig, msim_result_sizes, msim_fetch_records, msim_render_chain_device and the framed
 *                          fetches behind APPLY read; a selection leaves the contig un-applied.  msim_render_vcf_device(_file)
 *                          always render the FULL table, with the phased GT column once the contig has genotypes.
 *                          Selecting 1 or 2 without genotypes: MSIM_ERR_ARG.
 * A new plan of the contig, msim_clear and msim_release_result drop the genotypes and the selection.  On a host-only context
 * the three calls run sequential restatements over the host's table.                                                     */
int msim_genotype_contig(msim_ctx *ctx, int contig, uint64_t key, uint32_t seq, uint64_t het_thr);
int msim_set_genotypes(msim_ctx *ctx, int contig, const uint8_t *gt);
int msim_fetch_genotypes(msim_ctx *ctx, int contig, uint8_t *dst);
int msim_select_haplotype(msim_ctx *ctx, int contig, int hap);

/* ---- liftover chain: the record table as a coordinate map (UCSC chain format; liftOver, CrossMap, bcftools consensus -c) ---- */
/* One chain per contig, reference = target, mutated = query, both on the + strand:
 *   chain <score> <tName> <tSize> + <tStart> <tEnd> <qName> <qSize> + <qStart> <qEnd> <id>\n
 *   <size>\t<dt>\t<dq>\n   per aligned block but the last,   <size>\n   for the last one,   \n
 * SNPs are substitutions inside blocks.  Every other record is one gap in the walk of __mutate_sequence (mutator.py:318-426):
 * IN / TLI insert dq bases in front of base pos; DE / TL skip dt = stop - pos + 1 reference bases; IV leaves its span unmapped
 * on both sides (dt = dq: one chain has one strand); DU keeps its first copy aligned and inserts the second behind it.  Gaps
 * with no aligned base between them share one line (dt / dq summed); in front of the first block they become tStart / qStart,
 * behind the last one they shorten tEnd / qEnd.  score = the aligned bases, tSize = len, qSize = the mutated length.  A contig
 * without an aligned base (length 0, wholly deleted) has no chain: *needed = 0.
 * Stateless host helper, the twin of msim_render_vcf (reads no bases): out == NULL reports the size, cap < *needed is
 * MSIM_ERR_ARG.                                                                                                          */
int msim_render_chain(const msim_record *recs, uint64_t n_records, uint64_t len, const char *t_name,
                      const char *q_name, uint64_t id, char *out, uint64_t cap, uint64_t *needed);
/* The same bytes rendered by HIP kernels from the record table in HBM.  The contig must be planned (msim_plan_contig,
 * msim_vcf_plan_contig); applied it need not be.  Two-call protocol of msim_render_vcf_device.                           */
int msim_render_chain_device(msim_ctx *ctx, int contig, const char *t_name, const char *q_name,
                             uint64_t id, char *out, uint64_t cap, uint64_t *needed);

/* ---- text on the device ------------------------------------------------ */
/* The same record lines as msim_render_vcf, rendered by HIP kernels from the record table, insert pool and
 * input contig already in HBM (mutator.py:334-421 + vcf_writer.py:44-52,118-126).  Two-call protocol:
 * out == NULL renders into a device buffer and reports the size in *needed; a following call for the same
 * contig with out != NULL (cap >= *needed) copies the text to the host.                               */
int msim_render_vcf_device(msim_ctx *ctx, int contig, const char *seq_name, char *out, uint64_t cap,
                           uint64_t *needed);
/* The mutated contig as FASTA body text: '\n' after every `bpl` bases, none after a partial last line --
 * what FastaWriter.write emits between two headers (fasta_writer.py:40-58).  *needed = L + L / bpl.
 * Same two-call protocol.                                                                             */
int msim_fetch_sequence_framed(msim_ctx *ctx, int contig, uint32_t bpl, uint8_t *out, uint64_t cap,
                               uint64_t *needed);
/* The same two texts written into an open output file, off the calling thread: bytes [offset, offset + *written) of `fd`
 * (a regular file; libmsim keeps its own duplicate of the descriptor) receive what FastaWriter / VcfWriter would write()
 * there (fasta_writer.py:40-58, vcf_writer.py:118-126).  The call renders on the device, reports the size and QUEUES the
 * transfer on the output channel of that file kind (file_io.hip: a thread, a HIP stream and a pinned ring per channel --
 * device -> ring -> pwrite in 8 MiB pieces); it returns while the bytes are on their way, so that the caller's next contig
 * (ingest, PLAN, APPLY) overlaps them.  msim_file_wait (also msim_sync, msim_destroy) returns once everything queued is in
 * its file -- call it before the files are read, truncated or closed for good -- and reports the first failure of a queued
 * transfer (MSIM_ERR_IO: no space ...; MSIM_ERR_HIP).  MSIM_ERR_UNSUPPORTED: `fd` is no regular file (a pipe ...): use the
 * buffer calls above and write().  At most two transfers per channel are in flight: a third call waits for the oldest.     */
int msim_render_vcf_device_file(msim_ctx *ctx, int contig, const char *seq_name, int fd, uint64_t offset, uint64_t *written);
int msim_fetch_sequence_framed_file(msim_ctx *ctx, int contig, uint32_t bpl, int fd, uint64_t offset, uint64_t *written);
int msim_file_wait(msim_ctx *ctx);
/* BGZF output (SAM/BAM specification 4.1; compressed on the device, bgzf.hip).  msim_bgzf_open puts the output channel
 * `channel` (0 the FASTA, 1 the VCF) into BGZF mode on `fd` (a regular file, written from offset 0).  From then on every
 * transfer queued on that channel -- msim_fetch_sequence_framed_file / msim_render_vcf_device_file / msim_batch_fetch_file
 * and msim_bgzf_append -- is appended, in queue order, to ONE uncompressed stream that is cut into 65 280-byte blocks and
 * written as BGZF members; the `fd` those calls get is not used and their `offset` must equal the stream's current length
 * (MSIM_ERR_ARG otherwise).  msim_bgzf_append copies `n` host bytes (the caller may reuse them at once).  msim_bgzf_close
 * compresses the tail, appends the 28-byte EOF marker, waits for the channel and reports the compressed and uncompressed
 * byte counts; the channel is a plain one again.  The compressed bytes are a function of the uncompressed stream only.
 * msim_bgzf_compress: host bytes -> a whole BGZF file (members + EOF marker) in `out`, cap >= msim_bgzf_bound(n);
 * *device_ms (optional): the compression kernels' time on the device (events), copies excluded.                      */
int msim_bgzf_open(msim_ctx *ctx, int channel, int fd);
int msim_bgzf_append(msim_ctx *ctx, int channel, const uint8_t *bytes, uint64_t n);
int msim_bgzf_close(msim_ctx *ctx, int channel, uint64_t *compressed, uint64_t *uncompressed);
uint64_t msim_bgzf_bound(uint64_t n);
int msim_bgzf_compress(msim_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *written,
                       float *device_ms);
/* BGZF input (what msim_bgzf_* above and bgzip write).  msim_bgzf_probe is a host pass over the member chain (no context, no
 * device): *uncompressed = the sum of the members' ISIZE, *members = the members of the chain, empty ones (ISIZE 0: the EOF
 * marker, also in the middle of concatenated files) included; either may be NULL.  MSIM_ERR_VALUE (text: msim_last_error(NULL))
 * for bytes that are not gzip, gzip without BGZF framing (no extra field / no 'BC' subfield), a BSIZE that runs past the
 * end, a truncated last member and an ISIZE above 65 536; a missing EOF marker is accepted.
 * msim_bgzf_inflate: a whole BGZF file (host bytes) -> its uncompressed bytes in `out`, cap >= *uncompressed of the probe
 * (MSIM_ERR_ARG otherwise), *written = that count.  One RFC 1951 decoder per member on the device (stored, fixed and dynamic
 * blocks, any number of them per member), 1024 members per launch, uploads, kernels and downloads of neighbouring pieces
 * overlapped; empty members are skipped.  Every member's length and CRC32 are checked on the device against its trailer.
 * MSIM_ERR_VALUE for what the probe refuses and for a member that does not decode: "... member at offset <file offset of
 * the first such member>: <bad block type | invalid code lengths | invalid code | distance too far back | data past ISIZE |
 * truncated | invalid stored block lengths | CRC32 mismatch | ISIZE mismatch>"; `out` is then undefined, the context stays
 * usable.  Nothing is in flight into `out` or out of `in` when the call returns, whatever it returns (a wait that ran into
 * MSIM_WAIT_TIMEOUT_S is followed by an unbounded one).  `out` is best page-locked (msim_host_alloc).
 * *device_ms (optional): the inflate kernels' time on the device (events), copies excluded.                             */
int msim_bgzf_probe(const uint8_t *in, uint64_t n, uint64_t *uncompressed, uint64_t *members);
int msim_bgzf_inflate(msim_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *written,
                      float *device_ms);
/* ---- VCF replay: the mutated genome again from the reference and the VCF (csrc/vcf_parse.hip) ------------------------------ */
/* The inverse of the rendering above: every data line of a VCF this library (or Mutation-Simulator 3.0.2, vcf_writer.py:118-126)
 * wrote becomes one msim_record of the contig its CHROM names -- SN for a line whose INFO is ".", IN for SVTYPE=INS / INS:ME (the
 * inserted bytes go into the insert pool as they stand), DE for DEL / DEL:ME (length from REF), IV for INV, DU for DUP -- after
 * REF has been compared with the contig's resident bases and ALT with what the record type produces.  The one base an INS / DEL
 * line shares between REF and ALT (leading: ALT[0] == REF / ALT == REF[0], preferred; else trailing) stays as the genome has it.
 *   msim_vcf_load         uploads the whole text once and finds its lines, its header lines ('#...' in front of the first data
 *                         line) and its groups: the runs of data lines with the same CHROM.  On a host-only context: kept on the host.
 *   msim_vcf_groups       the groups (at most 65 537 are kept: more runs than a context has contigs cannot all be matched);
 *                         *n_groups = how many `out` could hold.  name_off: where the group's first line -- its CHROM -- starts
 *                         in the text.  The caller matches names to contigs.
 *   msim_vcf_plan_contig  parses group `group` (-1: the contig has no lines) against contig `contig` and leaves the contig PLANNED,
 *                         exactly as msim_plan_contig's host planner leaves one: msim_apply_contig and everything behind it go on
 *                         unchanged.  No generator is touched.  MSIM_ERR_VALUE, before anything is installed or launched on the
 *                         contig, for what the rewrite is not written for: "VCF line <1-based line>: <reason>", the first offending
 *                         line -- other than 10 fields; POS no number, 0 or beyond the contig; positions not increasing or inside
 *                         the input an earlier line consumed; REF not the genome's; ALT not what the type produces; multi-allelic,
 *                         symbolic or breakend alleles; another SVTYPE; FORMAT / sample other than GT / 1; an SNP ALT no
 *                         transition or transversion gives; an insert byte that is no letter; a mutated length of 2^32 or more
 *                         (decided from length + inserted + duplicated bytes, deletions not counted).  The context stays usable; the contig
 *                         is left UNPLANNED after a refusal (either parser), whatever it held before.
 *   msim_vcf_timing       device time (HIP events) of the load's and of all plans' kernels since msim_vcf_load
 *   msim_vcf_release      drops the text.
 * A host-only context runs a sequential parser behind the same calls; it keeps no bases of its own (msim_add_contig reads none
 * there), so msim_vcf_host_bases hands it the contig's `len` upper-cased bases first (copied; a no-op on a device context).
 * msim_fetch_records reads either parser's table.                                                                             */
typedef struct msim_vcf_group {
    uint64_t name_off;     /* offset of the group's first line in the text                                                     */
    uint64_t first_line;   /* 0-based index of that line among ALL lines of the text (line number - 1)                         */
    uint64_t n_lines;
    uint32_t name_len;     /* bytes of CHROM (256: longer than a contig name this mode takes)                                  */
    uint32_t rsv;
} msim_vcf_group;
int msim_vcf_load(msim_ctx *ctx, const uint8_t *text, uint64_t n, uint64_t *n_lines, uint64_t *n_groups);
int msim_vcf_groups(msim_ctx *ctx, msim_vcf_group *out, uint64_t cap, uint64_t *n_groups);
/* Which grammar msim_vcf_plan_contig reads the lines with; called between msim_vcf_load (which selects grammar 0 again) and the
 * first msim_vcf_plan_contig.  grammar 0: the simulator's dialect described above (sample_index 0, haplotype 0 or 1).
 * grammar 1, "consensus": any VCF, one haplotype of one sample, as `bcftools consensus -s SAMPLE -H N` applies it.  A line has 8
 * fields or 10 and more, every data line as many as the first; ID, QUAL, FILTER and INFO are not looked at.  sample_index is the
 * 0-based sample column (field 10 + sample_index; MSIM_ERR_ARG when the first data line has no such column), haplotype the 1-based
 * entry of its GT (FORMAT's first key) split at '/' and '|'; a haploid GT serves every haplotype.  Entry '.' or 0, or a selected
 * ALT '*': the line is skipped unread.  Entry k: REF -> the k-th ALT, both upper-cased, a REF byte matching the genome's base as it
 * stands or de-ambiguated.  One base REF and ALT share (their first bytes, preferred; else their last) stays as the genome has
 * it; what is left becomes a DE, an IN behind it, or both -- an SN record where a single base changes to what a transition or
 * transversion gives.  Further refusals: an allele index beyond the ALTs or a multi-allelic ALT field longer than 4096 bytes,
 * and "replacement or insertion that reaches behind the contig's last base" (reason 13), which has no record form.
 * Overlapping lines, and a line that starts at the base directly behind a pure insertion's anchor, are refused as out of
 * order.  On a device context the call reserves 96 bytes of parser state per line of the file's largest group.              */
int msim_vcf_select(msim_ctx *ctx, uint32_t grammar, uint32_t sample_index, uint32_t haplotype);
int msim_vcf_plan_contig(msim_ctx *ctx, int contig, int64_t group);
int msim_vcf_host_bases(msim_ctx *ctx, int contig, const uint8_t *bases);
int msim_vcf_timing(msim_ctx *ctx, double *load_kernel_ms, double *plan_kernel_ms);
int msim_vcf_release(msim_ctx *ctx);

/* Ingest one FASTA record straight from file text: `body` = the bytes after the header line, n_bases bases
 * in lines of `lenc` bases every `lenb` bytes (the .fai columns; uniform line width is what pyfaidx
 * requires, util.py:77-91).  Line terminators are skipped and a-z upper-cased on the device
 * (sequence_always_upper=True, util.py:84-88).  Replaces msim_add_contig + host-side parsing.           */
int msim_add_contig_text(msim_ctx *ctx, const uint8_t *body, uint64_t body_bytes, uint64_t n_bases,
                         uint32_t lenc, uint32_t lenb, int *contig);

/* Page-locked host memory for the caller's ingest / egress buffers: any host pointer is accepted by the text calls above,
 * but copies to and from page-locked memory run at the link's speed without a staging pass (and without the page faults
 * of a freshly allocated buffer) -- the CLI double-buffers its contigs through a few of these (mutator.py).            */
int msim_host_alloc(msim_ctx *ctx, uint64_t bytes, void **ptr);
int msim_host_free(msim_ctx *ctx, void *ptr);

/* ---- interchromosomal translocations (the reference's second pass, it_mutator.py) --------------------------------- */
/* __write_with_bp (it_mutator.py:121-146) for one contig: a NEW contig whose mutated stream is contig `a` cut at bp_a[0..n_bp)
 * and contig `b` cut at bp_b[0..n_bp), the segments taken alternately -- a's first, b's second, a's third ... (segment i =
 * bases [bp[i-1], bp[i]) with bp[-1] = 0 and bp[n_bp] = the contig's length; 0-based, as pairwise() over [0] + bp + [len]
 * cuts them).  The segments are read from the contigs' INPUT bases (the IT pass reads the file the mutation pass wrote).
 * n_bp = 0: a copy of a (__write_chrom_full, it_mutator.py:148-156; b is ignored).  The result counts as applied:
 * msim_fetch_sequence(_framed), msim_result_sizes and msim_result_checksum read it; it has no records.              */
int msim_splice_contigs(msim_ctx *ctx, int a, int b, uint64_t n_bp, const uint64_t *bp_a, const uint64_t *bp_b, int *contig);
/* sample_with_minimum_distance(start, stop, k, d) (util.py:93-109) on the context's CPython stream: the breakpoints of one
 * contig (it_mutator.py:96-119 calls it with (1, len, k, 1)).  setsize: CPython's 21 + 4^ceil(log4(3k)) for k > 5, else 21
 * (the caller evaluates the float expression, as for msim_range).  out: k ascending positions.  Works on a host-only
 * context.  MSIM_ERR_VALUE: "Sample larger than population or is negative" -- nothing was drawn.                       */
int msim_sample_min_distance(msim_ctx *ctx, int64_t start, int64_t stop, int64_t k, int64_t d, int64_t setsize, int64_t *out);

/* ---- many small contigs in one pass ------------------------------------------------------------------------------- */
/* mutate()'s loop body (mutator.py:111-141) for a run of SMALL contigs at once -- assemblies with thousands of scaffolds:
 * per contig the file text of the record (as for msim_add_contig_text), its ranges and its name.  The RNG streams are
 * consumed contig by contig exactly as by msim_plan_contig; ONE APPLY runs over the concatenation; the host frames the
 * FASTA bodies (fasta_writer.py:40-58) and renders the VCF lines (vcf_writer.py:118-126).  Results stay in the context
 * until the next batch; the FASTA text is framed when it is asked for -- by msim_batch_fetch straight into the caller's
 * memory (a mapped span of the output file), by msim_batch_view into a buffer of the context -- so the deflines
 * (msim_batch_contig.header) must stay valid until then.  MSIM_ERR_KEY: msim_batch_key_contig tells which contig hit the
 * reference's KeyError.                                                                                                */
typedef struct msim_batch_contig {
    const uint8_t *body; uint64_t body_bytes; uint64_t n_bases; uint32_t lenc, lenb;   /* as msim_add_contig_text     */
    const msim_range *ranges; int32_t n_ranges;                                        /* as msim_plan_contig         */
    const char *name;                                                                  /* CHROM of its VCF lines      */
    const char *header;      /* NULL: the FASTA text holds the framed bodies only.  Else the defline without '>': the text
                                is the complete run of records as FastaWriter writes them (fasta_writer.py:31-38) --
                                '>' header '\n' body, with a '\n' before a header iff the body before it ended mid-line */
    uint32_t name_len, header_len;   /* 0: `name` / `header` are NUL-terminated strings.  Else their length in bytes: they may
                                then point straight into the FASTA file text (an assembly has 10^5 deflines; nobody has
                                to copy them) */
} msim_batch_contig;
int msim_batch_run(msim_ctx *ctx, const msim_batch_contig *contigs, int n);
/* per contig: bytes of its part of the FASTA text (header line included where given), bytes of its VCF lines, plan-was-empty flag (mutator.py:125-129), records */
int msim_batch_sizes(msim_ctx *ctx, int n, uint64_t *fasta_bytes, uint64_t *vcf_bytes, int32_t *empty, uint64_t *n_records);
/* the framed bodies / the VCF lines of all contigs of the batch, back to back in contig order (either may be NULL)       */
int msim_batch_fetch(msim_ctx *ctx, uint8_t *fasta_text, uint64_t fasta_cap, char *vcf_text, uint64_t vcf_cap);
/* The last batch's two texts queued for their output files (see msim_fetch_sequence_framed_file: same channels, same
 * msim_file_wait): the FASTA text is framed into libmsim's buffer by its host threads and written from there, the VCF text
 * as it was rendered; either descriptor may be -1 (not wanted).  The texts' sizes: msim_batch_view (fasta_text == NULL).
 * The next msim_batch_run waits, where it overwrites them, until the channel has let go of the buffers.                  */
int msim_batch_fetch_file(msim_ctx *ctx, int fasta_fd, uint64_t fasta_offset, int vcf_fd, uint64_t vcf_offset);
/* the same texts in place (valid until the next batch / destroy): no copy of a few hundred MB.  *last_line_bases: bases on
 * the partial last line of the FASTA text (what FastaWriter needs to know to continue after it)                           */
int msim_batch_view(msim_ctx *ctx, const uint8_t **fasta_text, uint64_t *fasta_bytes, const char **vcf_text,
                    uint64_t *vcf_bytes, uint64_t *last_line_bases);
int msim_batch_key_contig(msim_ctx *ctx, int *contig);

/* ---- FASTA index pass of the host loader (replaces pyfaidx's index, util.py:77-91) ---------------------------------- */
/* Pure host code, no context: per record of a FASTA text the facts pyfaidx's index holds -- where the defline text and the
 * body sit, bases, bases per line (lenc), bytes per line (lenb) -- and pyfaidx's consistency verdict.  The body is NOT
 * touched otherwise: it goes to the device as text (msim_add_contig_text).  Call with records = NULL to count.
 * MSIM_ERR_VALUE: sequence text before the first defline (pyfaidx: FastaIndexingError).                                */
#define MSIM_FASTA_HAS_BODY    1u   /* at least one line follows the defline                                              */
#define MSIM_FASTA_BAD_LINES   2u   /* a line before the last non-empty one differs from the first line's length, or the
                                       last non-empty line is longer ("Line length of fasta file is not consistent")       */
#define MSIM_FASTA_NONUNIFORM  4u   /* mixed "\n" / "\r\n" terminators inside the record: no fixed stride for the device  */
typedef struct msim_fasta_record {
    uint64_t h0, h1;       /* defline text [h0, h1): without '>' and without the line terminator                          */
    uint64_t b0, b1;       /* body text [b0, b1): from the first base to the end of the record's last line (exclusive)     */
    uint64_t n_bases;
    uint32_t lenc, lenb;   /* bases / bytes of the first body line (bytes include its terminator)                          */
    uint32_t flags, rsv;
} msim_fasta_record;
int msim_fasta_index(const uint8_t *text, uint64_t n, msim_fasta_record *records, uint64_t cap, uint64_t *n_records);

/* ---- multi-GPU: one process per GPU, contigs' APPLY sharded, gather over RCCL ------------------ */
/* mutate()'s contig loop (mutator.py:111-141) is the unit of sharding: PLAN is replayed on every rank (the two
 * MT19937 streams chain across contigs), each rank APPLYs the contigs it owns, and the one exchange step is the
 * gather of the mutated contigs to `root` -- grouped ncclSend / ncclRecv, every peer over its own xGMI link.
 * librccl is dlopen()ed by msim_comm_init; the 128-byte ncclUniqueId travels over the caller's control plane. */
#define MSIM_COMM_ID_BYTES 128
int msim_comm_unique_id(uint8_t id[MSIM_COMM_ID_BYTES]);                       /* on one rank; broadcast the bytes */
int msim_comm_init(msim_ctx *ctx, const uint8_t id[MSIM_COMM_ID_BYTES], int rank, int world);   /* collective   */
int msim_comm_destroy(msim_ctx *ctx);
/* Mutated length of a planned contig where PLAN alone fixes it (SNP-only tables, SV mixes planned on the device):
 * every rank then knows every contig's size without an exchange.  *known = 0: only the applying rank knows it. */
int msim_planned_out_len(msim_ctx *ctx, int contig, uint64_t *out_len, int *known);
/* Slot i = contig contig_ids[i] (this context's id), applied by rank owner[i].  A slot has three PARTS: 0 the mutated stream
 * (out_len[i] bytes), 1 its record table (n_records[i] records of 16 bytes: the binary VCF, what __mutate_sequence hands the
 * VcfWriter, mutator.py:334-421), 2 its insert pool (pool_len[i] bytes).  n_records / pool_len NULL: streams only.  Sizes of
 * contigs a rank does not own come over the caller's control plane (msim_result_sizes on the owner).  Synchronises, then moves
 * every part to `root`.  device_addrs[3 i + part] (optional) = where the part now lives on this rank: the contig's own buffer
 * (owner), a receive buffer of the context (root), 0 elsewhere / for an empty part.  Valid until the next gather / clear.   */
/* A failure of this call on ONE rank (a slot that rank has not applied, a size that disagrees with its result) is fatal
 * for the communicator: its peers have posted the matching transfers and wait for them.  Tear the communicator down
 * (msim_comm_destroy on every rank) -- agree on the slots over the control plane first, as gather.Communicator does.      */
int msim_gather_to_root(msim_ctx *ctx, int n, const int *contig_ids, const int *owner, const uint64_t *out_len,
                        const uint64_t *n_records, const uint64_t *pool_len, int root, uint64_t *device_addrs);
/* The transfers `rank` posts for that gather, without touching a GPU: ops[5k..] = kind (0 send, 1 recv, 2 already
 * local), slot, part, peer, bytes -- in posting order ((slot, part) order on both sides of every pair); capacity 3 n ops. */
int msim_gather_plan(int n, const int *owner, const uint64_t *out_len, const uint64_t *n_records, const uint64_t *pool_len,
                     int rank, int world, int root, int64_t *ops, int *n_ops);
/* bytes at a device address msim_gather_to_root reported -> host (the root reading a remote contig's records / pool to
 * render its VCF lines with msim_render_vcf).                                                                            */
int msim_gather_fetch(msim_ctx *ctx, uint64_t device_addr, uint64_t bytes, void *dst);

/* ---- context-dependent SNPs: a 96-channel mutational spectrum (csrc/spectrum.hip, spectrum.h) ------------------------------- */
/* A second way to draw SNPs, the only PLAN engine that reads the genome: every ELIGIBLE site of a contig mutates independently,
 * with a probability its trinucleotide decides.  code(A, C, G, T) = 0..3, every other byte (N, IUPAC, U, -) is invalid; site p
 * is eligible iff 1 <= p <= L - 2 and b[p-1], b[p], b[p+1] are valid; ctx = 16 code(b[p-1]) + 4 code(b[p]) + code(b[p+1]).
 *   msim_context_counts        device census of a resident contig: counts[ctx] over its eligible sites, *n_valid their sum.
 *   msim_plan_contig_spectrum  thr[3 ctx + i], i = 0..2: the cumulative probabilities of the SN record's aux values 0, 1, 2 in
 *                              context ctx (0 the transition, 1 / 2 the transversion table's columns), scaled by 2^64, each triple
 *                              non-decreasing (MSIM_ERR_ARG otherwise) -- the caller's exact arithmetic
 *                              (mutation_simulator_amd/spectrum.py).  For an eligible site p: v = Philox4x32-10, counter
 *                              (p >> 1, 0, seq, tag 21) under the 64-bit `key`; r = the high 64 bits of v for an odd p, the low
 *                              64 for an even one; j = #{i : thr[3 ctx + i] <= r}; j == 3: nothing, else the record
 *                              {pos = p, stop = p, extra = 0, MSIM_SN, aux = j, rsv = 0}.  Records come out in position order
 *                              and the contig is left PLANNED as the VCF replay's parser leaves one (an SNP-only table of
 *                              host-known size, no insert pool): msim_plan_was_empty, msim_apply_contig, the renderers,
 *                              msim_genotype_contig and the chain follow unchanged.  Works in any device context (a fast
 *                              context's queue is flushed first); no MT19937 stream moves, msim_set_params is not needed.
 *                              MSIM_ERR_HIP on a host-only context; MSIM_ERR_UNSUPPORTED for 2^31 records or more.
 *   msim_spectrum_timing       the census's and the plans' kernel time on the device (HIP events) since the context was made or
 *                              msim_reset_stats.
 * MSIM_SPECTRUM_TILE: the bases one workgroup of the sampler takes -- where the kernels' edge cases lie.
 * msim_dbg_context_counts / msim_dbg_spectrum_plan: the same two results by sequential host loops over the caller's bases --
 * no context, no GPU (error text: msim_last_error with a NULL context).  recs == NULL: *n_recs only; cap < *n_recs: MSIM_ERR_ARG. */
#define MSIM_SPECTRUM_TILE 4096
int msim_context_counts(msim_ctx *ctx, int contig, uint64_t counts[64], uint64_t *n_valid);
int msim_plan_contig_spectrum(msim_ctx *ctx, int contig, const uint64_t thr[192], uint64_t key, uint32_t seq);
int msim_spectrum_timing(msim_ctx *ctx, double *census_ms, double *plan_ms);
int msim_dbg_context_counts(const uint8_t *bases, uint64_t L, uint64_t counts[64], uint64_t *n_valid);
int msim_dbg_spectrum_plan(const uint8_t *bases, uint64_t L, const uint64_t thr[192], uint64_t key, uint32_t seq,
                           msim_record *recs, uint64_t cap, uint64_t *n_recs);
/* The sampler's inverse, a PROFILE: a planned contig's record table counted against its resident reference bases.
 *   msim_sbs_counts      an SN record at p has a channel iff p is an eligible site (above); the channel is the pyrimidine-folded
 *                        N[X>Y]N of (ctx, aux): substitution-major (C>A, C>G, C>T, T>A, T>C, T>G), then the 5' base, then the 3'
 *                        base; a purine centre is read off the other strand.  The context is always the REFERENCE's: neighbouring
 *                        SNPs do not see each other, and an applied contig counts as before.  tallies[0]: SN records without a
 *                        channel (the contig's first or last base, a neighbourhood holding N, IUPAC, U or -); tallies[t],
 *                        t = MSIM_SN .. MSIM_TLI: the records of type t -- so sum(channels) + tallies[0] == tallies[MSIM_SN].
 *                        Any planned contig that is not released, whichever call left its table (the planners of every engine,
 *                        msim_plan_contig_spectrum, msim_vcf_plan_contig, msim_dbg_set_records); with a haplotype selected, the
 *                        table msim_fetch_records returns.  Synchronises like msim_fetch_records; changes nothing on the contig,
 *                        no generator moves.  An empty table: zeros, nothing launched.  MSIM_ERR_HIP on a host-only context.
 *   msim_sbs_timing      the profile kernel's time on the device (HIP events) since the context was made or msim_reset_stats.
 * MSIM_SBS_PASS: the records one workgroup of the kernel takes per pass -- where its edge cases lie.
 * msim_dbg_sbs_counts: the same result by a sequential host loop over the caller's bases and records -- no context, no GPU
 * (MSIM_ERR_ARG for a record of unknown type; error text: msim_last_error with a NULL context).                               */
#define MSIM_SBS_CHANNELS 96
#define MSIM_SBS_TALLIES   8
#define MSIM_SBS_PASS   1024
int msim_sbs_counts(msim_ctx *ctx, int contig, uint64_t channels[96], uint64_t tallies[8]);
int msim_sbs_timing(msim_ctx *ctx, double *kernel_ms);
int msim_dbg_sbs_counts(const uint8_t *bases, uint64_t L, const msim_record *recs, uint64_t n_records,
                        uint64_t channels[96], uint64_t tallies[8]);

/* ---- compare: a truth table scored against a calls table (csrc/compare.hip, compare.h) ----------------------------------------- */
/* Two record tables planned on the SAME resident contig -- A, the truth, HELD beside the contig; B, the calls, the contig's current
 * table -- joined record by record.  Which records are one variant:
 *   SN                same pos and same aux.
 *   DU, IV, TL, TLI   identical pos, stop and aux; TLI also extra.
 *   DE, IN            same type, same length n = stop - pos + 1, and one a shifted placement of the other.  With g the contig's
 *                     bases and L its length: a deletion of g[p..q] may move one base left iff p > 0 and g[p-1] == g[q], one base
 *                     right iff q + 1 < L and g[q+1] == g[p]; an insertion of S in front of base p may move left iff p > 0 and
 *                     g[p-1] == S[n-1] (S becomes S[n-1] + S[:n-1]), right iff p + 1 <= L - 1 and g[p] == S[0] (S becomes
 *                     S[1:] + g[p]).  So an insertion b at distance d = pos_b - pos_a inside a's interval is a iff
 *                     S_b[i] == S_a[(i + d) mod n] for all i.  No pool is rewritten.
 *                     A step is taken only if the genome byte it brings in (g[p-1] to the left; g[q+1] / g[p] to the right) is A, C,
 *                     G or T -- a run of N never shifts -- and a record never leaves the window of MSIM_CMP_WINDOW bases its pos lies
 *                     in (pos >> 16).  A step is checked in this order: the contig's end, that byte, the comparison, the window.
 *                     Every A indel so gets the interval [lo, hi] of its placements, each record normalised on its own against the
 *                     reference (as `bcftools norm` does): neighbouring variants do not see each other.
 * One to one: inside one class (type, length, interval, an insert's bytes up to rotation) the i-th record of A by position matches the
 * i-th of B.  One lane per A record finds its rank by scanning A to the left while pos >= lo, binary-searches B for lo, scans B up to
 * hi for the record of that rank in the class and sets that record's flag byte; a second launch tallies B from the flags.
 * MSIM_CMP_EXACT: lo = hi = pos for every record -- the literal comparison.
 *   counts[type][bin][4]   type = MSIM_SN .. MSIM_TLI (row 0 unused); bin: for IN and DE the length bin 1, 2-5, 6-20, 21-50, 51 and
 *                          above, bin 0 for every other type; the four values: truth matched, truth missed, calls matched, calls
 *                          extra.  Truth matched == calls matched in every cell.
 *   tallies[2]             A indels whose walk a window edge stopped; A indels whose walk a byte outside A, C, G, T stopped.
 *   msim_cmp_hold      a device copy of the contig's current table (records and insert pool; with a haplotype selected the table
 *                      msim_fetch_records returns) becomes its HELD table, replacing one held before.  It survives a new plan of the
 *                      contig and msim_release_result; msim_cmp_release (contig -1: every contig's), msim_clear and msim_destroy
 *                      drop it.
 *   msim_cmp_counts    held against current.  Synchronises like msim_sbs_counts; changes neither table.  Two empty tables: zeros,
 *                      nothing launched.  MSIM_ERR_ARG without a held table or on an unplanned contig, MSIM_ERR_HIP on a host-only
 *                      context.
 *   msim_cmp_fetch     the held table's sizes, and into whichever destination is not NULL its records, its pool and the flag bytes of
 *                      the contig's last msim_cmp_counts: one per held record, one per current record, 1 = matched (MSIM_ERR_ARG
 *                      when the flags are asked for and there was no such call, or the current table has changed since).
 *   msim_cmp_timing    the two kernels' time on the device (HIP events) since the context was made or msim_reset_stats.
 * MSIM_CMP_PASS: the records one workgroup of the kernels takes per pass -- where their edge cases lie.
 * msim_dbg_cmp_counts: the same counts, tallies and flags (either flag array may be NULL) by a sequential host loop over the
 * caller's bases and two tables -- no context, no GPU (MSIM_ERR_ARG for a record of unknown type; error text: msim_last_error with
 * a NULL context).                                                                                                                  */
#define MSIM_CMP_EXACT  1u
#define MSIM_CMP_BINS   5
#define MSIM_CMP_PASS   256
#define MSIM_CMP_WINDOW 65536
int msim_cmp_hold(msim_ctx *ctx, int contig);
int msim_cmp_release(msim_ctx *ctx, int contig);
int msim_cmp_counts(msim_ctx *ctx, int contig, uint32_t flags, uint64_t *counts, uint64_t tallies[2]);
int msim_cmp_fetch(msim_ctx *ctx, int contig, uint64_t *n_held, uint64_t *held_pool_len, msim_record *held, uint8_t *held_pool,
                   uint8_t *held_flags, uint8_t *current_flags);
int msim_cmp_timing(msim_ctx *ctx, double *kernel_ms);
int msim_dbg_cmp_counts(const uint8_t *bases, uint64_t L, const msim_record *truth, uint64_t n_truth, const uint8_t *truth_pool,
                        uint64_t truth_pool_len, const msim_record *calls, uint64_t n_calls, const uint8_t *calls_pool,
                        uint64_t calls_pool_len, uint32_t flags, uint64_t *counts, uint64_t tallies[2], uint8_t *truth_flags,
                        uint8_t *calls_flags);

/* ---- compare --blocks: unmatched records rescued by replaying blocks (csrc/cmp_blocks.hip, cmp_blocks.h) ---------------------------- */
/* The match above scores every record on its own: an MNP written as one line against two SNPs, or a duplication reported as the
 * insertion it also is, counts once as missed and once as extra although both files describe the same sequence.  This pass, haploid
 * only, runs behind the match (flag bytes 0 or 1 on both tables) and rescues such records; it never takes a match away.
 * Blocks.  A record's FOOTPRINT END is its stop for DE, DU, IV and TL and its pos for SN, IN and TLI.  In merged position order (the
 *   truth's record first at equal pos) a record belongs to the block of its predecessors iff pos - end <= gap, `end` the largest
 *   footprint end of the records in front of it in either table; otherwise it starts a block.  A table's records do not overlap, so
 *   the record in front of it in its own table and the one in front of it in the other table (a binary search) decide.
 * Candidates.  A block that holds a record with flag byte 0, on either side, is a candidate.  It is walked in merged order, and the
 *   walk ends at the first record that
 *     - is a TL or a TLI (its bytes come from elsewhere on the contig): the block HOLDS A TRANSLOCATION and is not replayed; or
 *     - is the block's record number MSIM_CMP_BLOCK_RECORDS + 1 (both sides together), or has a footprint end more than
 *       MSIM_CMP_BLOCK_SPAN bases behind the block's first pos: the block is OVER A LIMIT and is not replayed.
 *   A record that meets both is a translocation.
 * Replay.  Every other candidate is replayed over its input bases [lo, hi], its first pos to its largest footprint end: the bytes the
 *   rewrite (msim_apply_contig) writes there with the truth's records of the block alone, and the bytes it writes with the calls'
 *   alone -- an SN's outcome on the de-ambiguated base, an IN's bytes in front of the base it stands at, a DU's span twice, an IV's
 *   reverse complement.  The two streams are compared byte for byte, lengths included; a stream with an SN the rewrite has no outcome
 *   for (MSIM_ERR_KEY) equals nothing.  On equality every flag-0 record of the block, on both sides, gets flag byte 2, "matched as
 *   part of a block"; flag-1 records keep their byte; on inequality nothing changes.  So a shifted pair of indels the match paired
 *   stays matched even with an SNP between the two placements, where a replay of that neighbourhood alone would differ.
 *   counts[type][bin][6]   truth matched, truth block-matched, truth missed, calls matched, calls block-matched, calls extra.
 *   tallies[2]             as msim_cmp_counts'.
 *   block_tallies[5]       candidates, replayed, equal, over a limit, holding a translocation; candidates = replayed + over a limit +
 *                          holding a translocation.
 *   msim_cmp_counts_blocks   held against current, as msim_cmp_counts and with its errors; MSIM_CMP_EXACT is allowed (the match is
 *                            then literal and the replay rescues the shifted indels inside a gap); MSIM_ERR_ARG for gap >
 *                            MSIM_CMP_BLOCK_SPAN.  msim_cmp_fetch then returns flag bytes 0, 1 or 2.  The match's and the final
 *                            tally's time adds to msim_cmp_timing.
 *   msim_cmp_blocks_timing   the block pass's two kernels on the device (HIP events) since the context was made or msim_reset_stats.
 * Limits.  A block is compared as a whole: one unmatched record that stands alone among matched ones is not rescued by dropping a
 *   neighbour; blocks holding a translocation or over a limit stay as the match left them; genotypes are not considered.
 * msim_dbg_cmp_counts_blocks: the same counts, tallies, block tallies and flags (either flag array may be NULL) by sequential host
 * loops -- no context, no GPU (MSIM_ERR_ARG for a record of unknown type, a table not strictly increasing in pos, gap > MSIM_CMP_BLOCK_SPAN). */
#define MSIM_CMP_BLOCK_GAP     50
#define MSIM_CMP_BLOCK_RECORDS 64
#define MSIM_CMP_BLOCK_SPAN    4096
int msim_cmp_counts_blocks(msim_ctx *ctx, int contig, uint32_t flags, uint32_t gap, uint64_t *counts, uint64_t tallies[2],
                           uint64_t block_tallies[5]);
int msim_cmp_blocks_timing(msim_ctx *ctx, double *kernel_ms);
int msim_dbg_cmp_counts_blocks(const uint8_t *bases, uint64_t L, const msim_record *truth, uint64_t n_truth, const uint8_t *truth_pool,
                               uint64_t truth_pool_len, const msim_record *calls, uint64_t n_calls, const uint8_t *calls_pool,
                               uint64_t calls_pool_len, uint32_t flags, uint32_t gap, uint64_t *counts, uint64_t tallies[2],
                               uint64_t block_tallies[5], uint8_t *truth_flags, uint8_t *calls_flags);

/* ---- compare --diploid: genotypes scored against a diploid truth (csrc/compare.hip, compare.h) ------------------------------------ */
/* A side's (the truth's, the calls') two haplotype tables of one contig are JOINED into one diploid table U of distinct variants with
 * a genotype byte each, and the truth's U is matched against the calls' U; a pair's DOSAGES are then compared.  Phase is ignored on
 * both sides: 0|1, 1|0, 0/1 and 1/0 are one het, 1|1 and 1/1 hom, and a haploid 1 -- which serves both haplotypes, as in the
 * consensus grammar -- counts as hom.
 * Join.  H1, H2: position-sorted tables (pos strictly increasing), each with its own insert pool.  U carries one genotype byte per
 *   record, bit 0: on haplotype 1, bit 1: on haplotype 2 (the byte of msim_set_genotypes).  A record of H2 is the same variant as a
 *   record of H1 iff they have the same pos and are one variant at distance 0: every type the same type and pos; SN, DU, IV, TL and
 *   TLI the same aux; IN, DE, DU, IV, TL and TLI the same length (stop); IN the same insert bytes, compared as bytes, not as pool
 *   offsets; TLI the same extra.  Such a pair is written once, as H1's copy, with genotype 3; every other record with genotype 1
 *   (from H1) or 2 (from H2).  U is sorted by pos, at equal pos the record from H1 first: at most two records of U share a pos,
 *   and never two of one class (identical pairs were merged), which is why the matching's rank and scan stay correct on U.  U's pool
 *   is H1's pool followed by H2's: the extra of an IN record that came from H2 is rebased by H1's pool length, no other type's
 *   extra is touched.  MSIM_ERR_UNSUPPORTED when the two tables hold 2^31 records or more, or the two pools 2^32 bytes or more.
 * Match.  Every record of the truth's U finds its record in the calls' U by the rules above, window, stops and MSIM_CMP_EXACT
 *   unchanged.  A pair whose dosages (the set bits of the two genotype bytes) are equal is a true positive, flag byte 1 on both
 *   records; a pair whose dosages differ is a genotype mismatch, flag byte 2 on both; no partner: flag byte 0.
 *   counts[type][bin][6]   truth matched, truth genotype-mismatched, truth missed, calls matched, calls genotype-mismatched, calls
 *                          extra.  In every cell truth matched == calls matched and truth mismatched == calls mismatched (a pair is
 *                          one type and one length).  tallies[2] as msim_cmp_counts'.
 * Limits.  Two records on different haplotypes that are shifted placements of one another stay two het records (only identical
 *   records merge); phase is not compared; each haplotype goes through its grammar on its own.
 *   msim_cmp_join             the contig's HELD table is haplotype 1, its current table haplotype 2; the result becomes the contig's
 *                             diploid table of `side`, kept in the context.  The held table is consumed; the current table is not
 *                             changed.  The diploid table survives a new plan of the contig and is consumed by msim_cmp_release
 *                             (of the contig, or -1), msim_clear, msim_destroy and a new join on the same contig and side.  Two
 *                             empty inputs: an empty diploid table, nothing launched.  MSIM_ERR_ARG without a held table, on an
 *                             unplanned contig or an unknown side, MSIM_ERR_HIP on a host-only context.
 *   msim_cmp_counts_diploid   the truth's diploid table against the calls'; MSIM_ERR_ARG before both sides exist.  It neither
 *                             reads nor changes the contig's tables or msim_cmp_counts' state.  Its kernels' time adds to
 *                             msim_cmp_timing.
 *   msim_cmp_fetch_diploid    one side's sizes and, into whichever destination is not NULL, its records, pool, genotype bytes and
 *                             the flag bytes of the last msim_cmp_counts_diploid (MSIM_ERR_ARG before both sides exist, or when
 *                             the flags are asked for before such a call).
 *   msim_cmp_join_timing      the join's kernels and pool copies on the device (HIP events) since the context was made or
 *                             msim_reset_stats.
 * MSIM_CMP_JOIN_TILE: the records one workgroup of the join's scan takes -- where its edge cases lie.
 * msim_dbg_cmp_join / msim_dbg_cmp_counts_diploid: the same by sequential host loops, no context, no GPU.  The join writes
 * out[n1 + n2], out_gt[n1 + n2] and out_pool[pool1_len + pool2_len] and the number of records to *n_out; the counts take a
 * genotype byte per record and give the flag bytes (either array may be NULL).  MSIM_ERR_ARG for a record of unknown type, a
 * table out of order, a genotype byte outside 1..3, a NULL table with a count; the join's two MSIM_ERR_UNSUPPORTED cases.           */
#define MSIM_CMP_TRUTH 0
#define MSIM_CMP_CALLS 1
#define MSIM_CMP_JOIN_TILE 1024
int msim_cmp_join(msim_ctx *ctx, int contig, int side);
int msim_cmp_counts_diploid(msim_ctx *ctx, int contig, uint32_t flags, uint64_t *counts, uint64_t tallies[2]);
int msim_cmp_fetch_diploid(msim_ctx *ctx, int contig, int side, uint64_t *n, uint64_t *pool_len, msim_record *recs, uint8_t *pool,
                           uint8_t *gt, uint8_t *flags);
int msim_cmp_join_timing(msim_ctx *ctx, double *kernel_ms);
int msim_dbg_cmp_join(const msim_record *h1, uint64_t n1, const uint8_t *pool1, uint64_t pool1_len, const msim_record *h2, uint64_t n2,
                      const uint8_t *pool2, uint64_t pool2_len, msim_record *out, uint8_t *out_pool, uint8_t *out_gt, uint64_t *n_out);
int msim_dbg_cmp_counts_diploid(const uint8_t *bases, uint64_t L, const msim_record *truth, uint64_t n_truth, const uint8_t *truth_pool,
                                uint64_t truth_pool_len, const uint8_t *truth_gt, const msim_record *calls, uint64_t n_calls,
                                const uint8_t *calls_pool, uint64_t calls_pool_len, const uint8_t *calls_gt, uint32_t flags,
                                uint64_t *counts, uint64_t tallies[2], uint8_t *truth_flags, uint8_t *calls_flags);

/* ---- compare --diploid --phased: switch and flip errors against a phased truth (csrc/cmp_phase.hip, cmp_phase.h) ------------------- */
/* Every record of a side's diploid table U carries a PHASE WORD: 0 not phased; MSIM_PHASE_CONTIG phased with no phase set named (the
 * contig is the set); 1 .. 0xFFFFFFFE phased in the set its PS names.  The word of a VCF line (vcf_cons_phase, csrc/vcf_parse.h): the
 * sample column and FORMAT are found from the back as the consensus grammar finds them; the GT subfield is phased iff it holds at
 * least one '|' and no '/' (a haploid GT, a VCF of 8 fields, a GT with '/': word 0); FORMAT's keys are split at ':' and the key that
 * is exactly PS selects the sample subfield of the same index -- one to ten decimal digits with a value in 1 .. 0xFFFFFFFE give that
 * value; no PS key, a sample with fewer subfields, an empty subfield or '.' give MSIM_PHASE_CONTIG; anything else (a sign, a letter,
 * 0, a value too large) gives word 0 and the record is tallied as UNREADABLE -- the run is not refused.
 * Pairs.  A truth record is INFORMATIVE iff its flag byte (msim_cmp_counts_diploid) is 1, its genotype byte is 1 or 2, its word is
 *   nonzero and the word of its partner -- the calls' record the match paired it with -- is nonzero.  Such a pair has the key (truth
 *   word, calls word) and the orientation o: 1 when the two genotype bytes differ, 0 when they are equal.  The informative pairs are
 *   taken in the truth table's order (pos non-decreasing, haplotype 1's record first at equal pos); every other record is transparent.
 * Tally.  A BLOCK is a maximal run of consecutive pairs with equal key.  A pair carries a RAW SWITCH BIT iff its predecessor is in
 *   the same block and has the other orientation.  Inside a block a maximal run of r consecutive raw switch bits counts as r / 2
 *   FLIPS and r % 2 SWITCHES (the greedy left-to-right pairing of whatshap compare).  A block's HAMMING distance is min(its pairs
 *   with o = 0, its pairs with o = 1).
 *   out[MSIM_CMP_PHASE_COUNTS]: truth phased hets (genotype 1 or 2, word nonzero), calls phased hets, pairs, blocks, blocks of one
 *   pair, assessed adjacencies (pairs - blocks), raw switch bits, switches, flips, Hamming, pairs in blocks of two or more.
 * Limits.  Interleaved or nested phase sets are cut into more blocks than a per-set sort would give; a line that yields a DE and an
 *   IN counts as two pairs; a het whose partner is a genotype mismatch is not assessed; one sample per side.
 *   msim_cmp_phase_mark     directly behind a consensus-grammar msim_vcf_plan_contig of `contig`, while its text is loaded: the
 *                           (pos, word) of every record of the table just planned are kept as the MARKS of (contig, side,
 *                           haplotype 1 or 2); tally[3]: phased, unphased, unreadable records.  An empty table: empty marks, nothing
 *                           launched.  MSIM_ERR_ARG where the contig's last call was no such plan, for an unknown side or haplotype.
 *   msim_cmp_phase_join     behind msim_cmp_join of that side: U's records get their words -- genotype 1 or 3 from haplotype 1's
 *                           marks, genotype 2 from haplotype 2's, found by pos -- and the marks are consumed.  MSIM_ERR_ARG without
 *                           both haplotypes' marks or without the side's diploid table.
 *   msim_cmp_phase_set      the words of U directly (as msim_set_genotypes sets genotype bytes); MSIM_ERR_ARG without the side's
 *                           diploid table or when n is not its record count.
 *   msim_cmp_phase_counts   behind msim_cmp_counts_diploid with the same flags (MSIM_ERR_ARG before that call, with other flags, or
 *                           before both sides have words).  It changes neither the tables nor the flag bytes nor any count of
 *                           msim_cmp_counts_diploid.
 *   msim_cmp_fetch_phase    a side's words and, for the truth (MSIM_ERR_ARG for the calls, or before msim_cmp_phase_counts), a
 *                           state byte per record: 0 not informative, 1 informative, 2 added with a raw switch bit, 4 added with
 *                           orientation 1.  Either destination may be NULL.
 *   msim_cmp_phase_timing   the phase kernels' time on the device (HIP events) since the context was made or msim_reset_stats.
 * Words, marks and state bytes are consumed where the diploid tables are: msim_cmp_release, msim_clear, msim_destroy; a new
 * msim_cmp_join of a contig and side consumes that side's words.  MSIM_ERR_HIP on a host-only context.
 * MSIM_CMP_PHASE_TILE: the records (and the pairs) one workgroup of the passes takes -- where their edge cases lie.
 * msim_dbg_cmp_phase: out[] and the truth's state bytes (may be NULL) by sequential host loops over two diploid tables with their
 * genotype bytes and words -- no context, no GPU; the refusals of msim_dbg_cmp_counts_diploid.  msim_dbg_vcf_phase_word: the word of
 * one VCF line (n bytes, no terminator) of a file with nf0 fields a line, sample column `sample` (0-based); *unreadable (may be
 * NULL): the line's PS was present and not a readable value.                                                                         */
#define MSIM_PHASE_CONTIG     0xFFFFFFFFu
#define MSIM_CMP_PHASE_TILE   256
#define MSIM_CMP_PHASE_COUNTS 11
int msim_cmp_phase_mark(msim_ctx *ctx, int contig, int side, int haplotype, uint64_t tally[3]);
int msim_cmp_phase_join(msim_ctx *ctx, int contig, int side);
int msim_cmp_phase_set(msim_ctx *ctx, int contig, int side, const uint32_t *words, uint64_t n);
int msim_cmp_phase_counts(msim_ctx *ctx, int contig, uint32_t flags, uint64_t out[MSIM_CMP_PHASE_COUNTS]);
int msim_cmp_fetch_phase(msim_ctx *ctx, int contig, int side, uint32_t *words, uint8_t *state);
int msim_cmp_phase_timing(msim_ctx *ctx, double *kernel_ms);
int msim_dbg_cmp_phase(const uint8_t *bases, uint64_t L, const msim_record *truth, uint64_t n_truth, const uint8_t *truth_pool,
                       uint64_t truth_pool_len, const uint8_t *truth_gt, const uint32_t *truth_words, const msim_record *calls,
                       uint64_t n_calls, const uint8_t *calls_pool, uint64_t calls_pool_len, const uint8_t *calls_gt,
                       const uint32_t *calls_words, uint32_t flags, uint64_t out[MSIM_CMP_PHASE_COUNTS], uint8_t *truth_state);
int msim_dbg_vcf_phase_word(const uint8_t *line, uint64_t n, uint32_t nf0, uint32_t sample, uint32_t *word, uint32_t *unreadable);

/* ---- compare --regions / --stratify: records scored inside BED intervals (csrc/cmp_regions.hip, cmp_regions.h, bed.cpp) ------------ */
/* A REGION SET of a contig of L bases is a list of n half-open 0-based intervals [start, end) in normal form: start < end <= L and
 * start[i] > end[i-1] -- overlapping and abutting intervals have been merged.  n == 0 is the empty set: nothing is inside it.
 * Anchor.  A record's ANCHOR is, for IN and DE, the leftmost of its placements -- lo of the interval the match gives it (rules
 *   above: walk, window and base stops unchanged) --; with MSIM_CMP_EXACT, and for every other type, its pos.  A record is INSIDE a
 *   set iff some interval holds its anchor: an upper-bound binary search over the starts, then anchor < end of the interval in front.
 *   Matched partners are of one class and one window and so share lo: both records of a pair fall on the same side of every region
 *   edge however the two files placed the indel, and truth matched == calls matched holds in every cell of every restriction.
 * Limit.  Only the anchor counts: a DE, DU, IV or TL that reaches out of an interval is inside if its anchor is, and one that reaches
 *   into an interval from an anchor in front of it is outside.
 * A contig keeps up to MSIM_CMP_REGION_SETS resident sets.  The MARK of a record is one byte, bit s set iff the record is inside set
 * s (bits of sets that are not resident: 0; a record of unknown type: 0).  `flags`: MSIM_CMP_EXACT, and MSIM_CMP_DIPLOID for the
 * contig's two diploid tables (msim_cmp_join) in place of its held and current table.
 *   msim_cmp_regions_set      set `set` (0 .. MSIM_CMP_REGION_SETS - 1) of the contig, replacing one set before; the contig's marks are
 *                             forgotten.  MSIM_ERR_ARG for a set index out of range, a list not in normal form or an end beyond the
 *                             contig's length.
 *   msim_cmp_regions_drop     one set (set -1: all of the contig's; contig -1: every contig's) and the contig's marks.  Sets and marks
 *                             also go where held tables go: msim_cmp_release, msim_clear, msim_destroy.
 *   msim_cmp_regions_mark     the mark bytes of both tables -- held and current (the contig planned), or the two diploid tables --
 *                             with one walk per record and one search per record and resident set.  MSIM_ERR_ARG without the tables
 *                             the flags name.  Two empty tables: nothing launched.
 *   msim_cmp_counts_regions   behind msim_cmp_regions_mark AND behind the count call whose flag bytes it tallies again --
 *                             msim_cmp_counts or msim_cmp_counts_blocks; with MSIM_CMP_DIPLOID msim_cmp_counts_diploid --, all three
 *                             with the same MSIM_CMP_EXACT bit.  counts: the layout and width of that count call ([..][4]; [..][6]
 *                             behind the blocks and the diploid call), holding only the records inside EVERY set of `mask`;
 *                             outside[2]: the truth's and the calls' records that are not.  mask == 0: the count call's own counts,
 *                             outside 0.  MSIM_ERR_ARG before either call, with another exact bit, after a set of the contig changed
 *                             since the mark, after a new hold, join or current table since the mark, for a mask bit whose set is
 *                             not resident.
 *   msim_cmp_fetch_regions    the mark bytes of the last msim_cmp_regions_mark with these flags' tables: one per truth record, one per
 *                             calls record (either destination may be NULL); the refusals of msim_cmp_counts_regions' mark.
 *   msim_cmp_regions_timing   the two kernels' time on the device (HIP events) since the context was made or msim_reset_stats.
 * All of them: MSIM_ERR_HIP on a host-only context.
 * msim_dbg_cmp_counts_regions: the same counts, outside[2] and both mark arrays (either may be NULL) by sequential host loops over
 * the caller's bases, two tables with their flag bytes (those of the count call with `outcomes` 2 or 3 outcomes) and n_sets <=
 * MSIM_CMP_REGION_SETS sets -- set s is starts / ends [set_off[s], set_off[s + 1]) --, no context, no GPU.  MSIM_ERR_ARG for a record
 * of unknown type, a set not in normal form or beyond L, outcomes other than 2 or 3, a mask bit at or above n_sets.
 * msim_bed_scan: one sequential pass over BED text, no context.  Lines end at '\n' (a '\r' in front of it is dropped; the last line
 * needs none); empty lines and lines beginning with '#', "track" or "browser" are skipped; fields are split on runs of tab or blank;
 * the first three are the name, start and end, both decimal digits only and at most 4294967295; a line with start == end is valid
 * and dropped.  Per kept interval: starts[], ends[], lines[] (its 1-based line); per RUN of consecutive kept lines with one name:
 * run_name_off[], run_name_len[] (into the text), run_first[] (its first interval), run_count[].  Two calls: with the arrays NULL
 * *n_intervals and *n_runs are the sizes; then they are the capacities (MSIM_ERR_ARG when too small) and become the sizes.
 * MSIM_ERR_VALUE with "BED line N: fewer than three fields | start is no number | end is no number | end in front of start" for the
 * first offending line (msim_last_error with a NULL context).                                                                      */
#define MSIM_CMP_REGION_SETS 8
#define MSIM_CMP_DIPLOID     2u
int msim_cmp_regions_set(msim_ctx *ctx, int contig, int set, const uint32_t *starts, const uint32_t *ends, uint64_t n);
int msim_cmp_regions_drop(msim_ctx *ctx, int contig, int set);
int msim_cmp_regions_mark(msim_ctx *ctx, int contig, uint32_t flags);
int msim_cmp_counts_regions(msim_ctx *ctx, int contig, uint32_t flags, uint32_t mask, uint64_t *counts, uint64_t outside[2]);
int msim_cmp_fetch_regions(msim_ctx *ctx, int contig, uint32_t flags, uint8_t *truth_marks, uint8_t *calls_marks);
int msim_cmp_regions_timing(msim_ctx *ctx, double *kernel_ms);
int msim_dbg_cmp_counts_regions(const uint8_t *bases, uint64_t L, const msim_record *truth, uint64_t n_truth, const uint8_t *truth_pool,
                                uint64_t truth_pool_len, const uint8_t *truth_flags, const msim_record *calls, uint64_t n_calls,
                                const uint8_t *calls_pool, uint64_t calls_pool_len, const uint8_t *calls_flags, int outcomes,
                                uint32_t flags, uint32_t n_sets, const uint32_t *starts, const uint32_t *ends, const uint64_t *set_off,
                                uint32_t mask, uint64_t *counts, uint64_t outside[2], uint8_t *truth_marks, uint8_t *calls_marks);
int msim_bed_scan(const uint8_t *text, uint64_t n_text, uint32_t *starts, uint32_t *ends, uint64_t *lines, uint64_t *n_intervals,
                  uint64_t *run_name_off, uint32_t *run_name_len, uint64_t *run_first, uint64_t *run_count, uint64_t *n_runs);

/* ---- reads: FASTQ records drawn from the resident genome (csrc/reads.hip, reads.h) ------------------------------------------ */
/* A read (pair) is a pure function of (key, read index i): no generator of the mutation engines is touched, nothing chains, and
 * every record of a run is `stride` bytes long, so read i lies at byte i * stride of its file and any range renders on its own.
 * The caller passes integer tables only (mutation_simulator_amd/reads.py builds them); the device does no floating point.
 *
 * Tables.  frag_min and frag_thr[n_frag], 1 <= n_frag <= 4096: ascending uint64, the last equal to 2^53 -- fragment length
 * frag_min + k has the mass (frag_thr[k] - frag_thr[k - 1]) / 2^53; frag_min >= len; fmax = frag_min + n_frag - 1.  A single-end
 * run passes frag_min = len, n_frag = 1.  err_thr[2][len]: ceil(p_j * 2^53), the substitution probability of cycle j of mate 1,
 * then of mate 2; qual[2][len]: the quality bytes ('!' .. '~').  prefix: letters, digits and ._- only, at most 32 bytes.
 * n_reads: the run's N, 1 <= N < 2^32 (it fixes the width of the index field).
 *
 * Eligible contigs, in context order: those with length >= fmax; weight w_c = length - fmax + 1, P = their sum, prefix_w the
 * exclusive prefix sums.  Philox4x32-10 under the 64-bit key, counter (x, y, 0, tag):
 *   placement  v = draw(x = i, y = 0, tag 22); p = mulhi64(low 64 bits of v, P); the contig is the last eligible one with
 *              prefix_w[c] <= p, the 0-based start s = p - prefix_w[c]; u = (high 64 bits of v) >> 11, f = frag_min + the first k
 *              with u < frag_thr[k]; strand = bit 0 of the high 64 bits.  The fragment is bases [s, s + f) of the contig and
 *              always fits: there is no rejection loop.  The price: the last fmax - f starts of a contig are never drawn when
 *              f < fmax.
 *   bases      the fragment in its own orientation is those bases (strand 0) or their reverse complement (strand 1); mate 1 is
 *              its first len bases, mate 2 the reverse complement of its last len.  A genome byte outside A, C, G, T (the
 *              resident bases are upper-cased) reads 'N', takes no error and gets quality '!'.
 *   errors     cycle j of mate m (0, 1): w = draw(x = i, y = m << 16 | j >> 1, tag 23), word = the high 64 bits of w for an odd
 *              j, the low 64 for an even one; substitute iff (word >> 11) < err_thr[m][j]; the new base is index
 *              (b + 1 + (((word & 0x7FF) * 3) >> 11)) & 3 in the order A, C, G, T, b the index of the read's base -- the three
 *              alternatives come out 683 : 683 : 682 of 2048.
 *   record     "@<prefix><i>_<n>_<s + 1>_<f>_<+|->/<1|2>\n<len bases>\n+\n<len quals>\n": n the 1-based number of the contig in
 *              the context (the Fasta), + for strand 0; the four numbers are zero-padded decimals whose widths are fixed per run
 *              by the largest values they can take: N - 1, the number of the last eligible contig, the longest eligible contig's
 *              length, fmax.  stride = bytes of the prefix and the four widths + 2 len + 13.
 *
 *   msim_reads_setup        checks the tables (MSIM_ERR_ARG), finds the eligible contigs among the context's (MSIM_ERR_VALUE when
 *                           there is none, MSIM_ERR_UNSUPPORTED for one of 4 GiB or more) and uploads everything; *stride,
 *                           *n_eligible and *P describe the run.  The tables are copied.  msim_clear ends the setup.
 *   msim_reads_render       records [first, first + count) of mate 0 or 1 (1: a paired setup only) into out[cap], count * stride
 *                           bytes.  first + count may reach 2^32 where the index still fits its field; at most 1 GiB a call.
 *   msim_reads_render_file  the same text through output channel `mate` to bytes [offset, offset + *written) of `fd`: queued as
 *                           msim_fetch_sequence_framed_file queues a contig, BGZF mode included (msim_bgzf_open on the channel).
 *   msim_reads_timing       the render kernel's time on the device (HIP events) since the context was made or msim_reset_stats,
 *                           and how many reads of mate 1 / mate 2 rendered since the last setup hold only N (either may be NULL);
 *                           waits for the context's stream.
 *   msim_reads_release      waits for the channels and frees the run's tables.
 * All of them: MSIM_ERR_HIP on a host-only context.
 * msim_dbg_reads_render: the same text by a sequential host loop over the caller's bases -- contig k is
 * bases[offsets[k], offsets[k + 1]), upper case -- no context, no GPU (error text: msim_last_error with a NULL context).
 * out == NULL: *stride, *n_eligible and *P only.                                                                              */
typedef struct msim_reads_params {
    uint64_t key;
    uint64_t n_reads;
    uint32_t len, paired, frag_min, n_frag;
    const uint64_t *frag_thr;
    const uint64_t *err_thr;
    const uint8_t *qual;
    const char *prefix;
} msim_reads_params;
int msim_reads_setup(msim_ctx *ctx, const msim_reads_params *params, uint64_t *stride, uint64_t *n_eligible, uint64_t *P);
int msim_reads_render(msim_ctx *ctx, int mate, uint64_t first, uint64_t count, uint8_t *out, uint64_t cap);
int msim_reads_render_file(msim_ctx *ctx, int mate, uint64_t first, uint64_t count, int fd, uint64_t offset, uint64_t *written);
int msim_reads_timing(msim_ctx *ctx, double *kernel_ms, uint64_t all_n[2]);
int msim_reads_release(msim_ctx *ctx);
int msim_dbg_reads_render(const msim_reads_params *params, const uint8_t *bases, const uint64_t *offsets, uint32_t n_contigs, int mate,
                          uint64_t first, uint64_t count, uint8_t *out, uint64_t cap, uint64_t *stride, uint64_t *n_eligible,
                          uint64_t *P);

/* ---- test support: the SNP ti/tv transducer on the caller's words -------------------------------------------------- */
/* Runs the three passes that turn CPython-stream words into SNP outcomes -- the map pass over whole blocks of
 * MSIM_SNP_BLOCK_WORDS words, the scan that finds where the K-th SNP's draws end, the outcome pass -- over `words` (raw,
 * untempered), in buffers of the call's own: synchronous, no contig, no stream session.  ti_lim: a uniform 53-bit sample
 * below it is a transition.  The draws start at word `start`; only the n_words / MSIM_SNP_BLOCK_WORDS whole blocks are
 * mapped and drawn from.
 *   lanes:  (n_blocks + 1) * 256 * 4 uint32 -- per lane of every block A, B, T masks and packed map; the last block's
 *           worth is a guard the call fills with 0xee and no pass may touch
 *   maps:   (n_blocks + 1) * 4 uint32 -- per block the counts from the three start states and the end states; guard as above
 *   end_pos: the word behind the one the K-th SNP completes on; flags: 2 = fewer than K SNPs complete (end_pos unset)
 *   aux:    aux_off + K + 16 bytes -- aux_off (< 64) guard bytes 0xee, the K outcomes by rank (0 transition, 1 / 2 the
 *           transversion column), 16 guard bytes; the outcome array starts aux_off bytes behind a 256-byte boundary     */
#define MSIM_SNP_BLOCK_WORDS 8192
int msim_dbg_snp_draws(msim_ctx *ctx, const uint32_t *words, uint64_t n_words, uint64_t ti_lim, uint64_t start, uint32_t K,
                       uint32_t aux_off, uint32_t *lanes, uint32_t *maps, uint64_t *end_pos, uint32_t *flags, uint8_t *aux);

/* ---- test support: the sampler's tail rounds and stream cut on the caller's tables -------------------------------- */
/* One launch of the kernel that ends a random.sample() on the device -- the tail rounds (every duplicate costs one more accepted
 * draw, first occurrences win) and the exact stream cut (one past the word that holds the last accepted draw consumed) -- over
 * tables the caller made, in buffers of the call's own: synchronous, no contig, no stream session.
 *   words:  raw (untempered) CPython-stream words; the sample's window is words[p0, p0 + W), p0 = state->pos or, anchored,
 *           win_pos; a draw is accepted when temper(word) >> shift < n
 *   acc:    the accepted draws of the window in order from accepted index acc_first on (n_acc of them; all < n)
 *   blocks: raw_counts 1: the accepted draws per block of 2048 window words (n_blocks = ceil(W / 2048) <= 8192 entries);
 *           raw_counts 0: their exclusive prefix sums, n_blocks + 1 entries
 *   k:      accepted draws already consumed in front of the rounds (anchored: + need0); the rounds start with state->dups
 *           duplicates to replace (anchored: d1)
 *   bitmap: bm_guard guard words, ceil(n / 32) words, bm_guard guard words -- in and out, guards included
 *   state:  in and out; flags bit 0 = the window does not hold enough accepted draws, or the cut lay beyond pos_limit
 *           (then clamped to it)                                                                                         */
typedef struct msim_dbg_tail_state { uint64_t pos, snp_base; uint32_t flags, dups, accepted_used, rsv; } msim_dbg_tail_state;
int msim_dbg_sample_tail(msim_ctx *ctx, const uint32_t *words, uint64_t n_words, const uint32_t *acc, uint64_t n_acc,
                         uint32_t acc_first, const uint32_t *blocks, uint32_t n_blocks, uint32_t raw_counts, uint32_t W,
                         uint32_t shift, uint32_t n, uint32_t k, uint32_t *bitmap, uint32_t bm_guard, msim_dbg_tail_state *state,
                         int anchored, uint64_t win_pos, uint32_t need0, uint32_t d1, uint64_t pos_limit);

/* ---- test support: an anchored contig's whole stream chain on the caller's tables -------------------------------- */
/* The chain of a contig whose sample is an anchored window with one drawing range -- the fringe pass (the accepted draws of
 * [start, H) and the first need0 of the tail list go into the bitmap, duplicates counted), the tail rounds, the stream cut, the
 * scan and cut of the K2 SNPs' draws from there -- over tables the caller made, in buffers of the call's own: synchronous, no
 * contig, no stream session.  fused = 1: the ONE launch the sampler sends (NOTES section 34); 0: the three
 * stand-alone launches (MSIM_NO_CHAIN_FUSE=1).  Both must leave the same bytes wherever no overflow flag is raised, and the
 * same flag where one is.
 *   words:  raw (untempered) CPython-stream words, fewer than 2^28; the head interval is words[lo, lo + F), H = lo + F, the
 *           sample's window words[H, H + W); the SNP stage's lanes and maps are made by the map pass over the whole blocks of
 *           MSIM_SNP_BLOCK_WORDS words, and W2 / MSIM_SNP_BLOCK_WORDS + 2 of them must follow the block of word H + W
 *   hcnt:   accepted draws per block of 2048 words of the head interval (ceil(F / 2048) <= 1024 entries; checked against words)
 *   hacc:   those draws in order, block b's from index 2048 b on (n_hacc >= 2048 ceil(F / 2048))
 *   tail:   the window's accepted draws in order from accepted index k_core on (all < n); n_tail covers K - k_core + core_dups
 *           entries and everything up to the window's last accepted draw
 *   cnt:    accepted draws per block of 2048 window words (ceil(W / 2048) <= 8192 entries)
 *   bitmap: bm_guard guard words, ceil(n / 32) words, bm_guard guard words -- in and out, guards included
 *   win_maps: out, (W2 / MSIM_SNP_BLOCK_WORDS + 4) * 4 uint32: per SNP window block count and state at its start, the totals
 *           entry, one guard entry; what no launch writes stays 0xee
 *   io:     in: the layout (G = workgroups of the fringe grid, 1..256; core_dups / core_flags / head_flags: what the prep left
 *           behind); in and out: state (rsv = the largest margin used, permille); out: hdr = need0, d1, the ticket word
 *           (fused: G), 0; base = the saved start of the SNP draws                                                          */
typedef struct msim_dbg_chain {
    uint64_t lo, expect, pos_limit, snp_limit, ti_lim;
    uint32_t F, K, k_core, shift, n, W, W2, K2, soft_half, G, core_dups, core_flags, head_flags, bm_guard, fused, rsv;
    msim_dbg_tail_state state;
    uint32_t hdr[4];
    uint64_t base;
} msim_dbg_chain;
int msim_dbg_chain_step(msim_ctx *ctx, const uint32_t *words, uint64_t n_words, const uint32_t *hcnt, const uint32_t *hacc,
                        uint64_t n_hacc, const uint32_t *tail, uint64_t n_tail, const uint32_t *cnt, uint32_t *bitmap,
                        uint32_t *win_maps, msim_dbg_chain *io);
/* Fused chain launches the context's SNP sampler has sent since it was created (0 with MSIM_NO_CHAIN_FUSE=1). */
int msim_dbg_chains_fused(msim_ctx *ctx, uint64_t *n);

/* ---- stats -------------------------------------------------------------------------------------- */
int msim_stats(msim_ctx *ctx, msim_timing *out);
int msim_reset_stats(msim_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* MSIM_H */
