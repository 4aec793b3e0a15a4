// Context-dependent SNPs ("--spectrum"): the one PLAN engine that reads the genome (msim.h: msim_context_counts,
// msim_plan_contig_spectrum).  Every eligible site mutates independently with a probability its trinucleotide decides;
// the arithmetic is spectrum.h's, shared with the host restatements at the end of this file.
//
// Device path (gfx950), everything on the context's stream:
//   census   k_ctx_census: 16 bases a lane by one 16-byte load + the two halo bytes, counted into 64 lane-private bins
//            (lane_hist.h)
//   plan     k_spectrum_draw: a tile of MSIM_SPECTRUM_TILE bases a workgroup; per site the context, the Philox draw (one
//            call per two sites) and the compare against the context's last threshold (64 x 8 B in LDS; the other two are
//            read on a hit only) -> per lane a 32-bit OUTCOME word (2 bits a site), per tile the hit count
//            k_scan_u32 over the tile counts (scan_kernels.h)
//            k_spectrum_emit: reads the outcome words only -- no base, no draw a second time -- and stores the records at
//            tile offset + prefix of the lanes in front (wave scan by shuffles + the waves' sums), 16 bytes a store
//   profile  k_sbs_count (msim_sbs_counts), the sampler's inverse: one 16-byte record a lane and step, the three bases around an
//            SN record's position gathered from the resident contig, counted into 104 lane-private bins (96 channels + 8
//            tallies: lane_hist.h)
// The host waits once between scan and emit: the record table is allocated at its exact size.
#include <cstring>
#include <string>

#include "counter_trip.h"
#include "ctx.h"
#include "lane_hist.h"
#include "scan_kernels.h"
#include "spectrum.h"

namespace msim {

using fastrng::Key;
using fastrng::U4;

struct SpectrumState {
    CounterTrip census;                       // 64 census bins
    CounterTrip sbs;                          // HIST_SLOTS x 104 profile bins (spectrum::SBS_BINS)
    Scratch<uint64_t> d_thr;                  // 192 thresholds
    Scratch<uint32_t> d_words;                // one outcome word per lane of every tile (dev_reserve)
    Scratch<uint32_t> d_tile;                 // hits per tile, then their exclusive scan; [n_tiles]: the total (dev_reserve)
    Pinned<unsigned long long> h_pin;         // pinned: [0..191] thresholds on their way up, [192] the plan's total
    EventPair tm;                             // the plan's stretches
    double census_ms = 0, plan_ms = 0, sbs_ms = 0;
};

namespace {

static_assert(spectrum::TILE == MSIM_SPECTRUM_TILE, "msim.h and spectrum.h must agree on the tile");
constexpr int LANES = (int)spectrum::TILE_LANES, SITES = (int)spectrum::SITES_PER_LANE;
constexpr int CENSUS_AHEAD = 4;
constexpr unsigned CENSUS_MAX_BLOCKS = 2048;  // longer contigs stride (k_ctx_census counts on that: 2^20 tiles / 2048 = 512 a workgroup)

// bases [p0 - 1, p0 + 17) of the contig: the lane's 16 sites and their halo, zeros -- no base -- outside [0, L)
struct LaneBytes { uint32_t q[4], left, right; };
__device__ __forceinline__ LaneBytes lane_load(const uint8_t *__restrict__ b, uint64_t L, uint64_t p0) {
    LaneBytes x{{0, 0, 0, 0}, 0, 0};
    if (p0 < L) {                                           // (the allocation's slack covers a partial last piece)
        const uint4 w = *reinterpret_cast<const uint4 *>(b + p0);
        x.q[0] = w.x; x.q[1] = w.y; x.q[2] = w.z; x.q[3] = w.w;
        if (p0 > 0) x.left = b[p0 - 1];
        if (p0 + SITES < L) x.right = b[p0 + SITES];
        else if (p0 + SITES > L) {                          // the contig's last lane: the bytes behind its end
            const uint32_t n = (uint32_t)(L - p0);          // 1..15 bases
#pragma unroll
            for (int k = 0; k < 4; k++)
                x.q[k] = n >= 4u * k + 4u ? x.q[k] : n <= 4u * k ? 0u : x.q[k] & ((1u << (8 * (n - 4u * k))) - 1u);
        }
    }
    return x;
}
// ... and their codes (a zero byte is no base: CODE_INVALID)
__device__ __forceinline__ void lane_codes(const LaneBytes &x, uint32_t code[SITES + 2]) {
    code[0] = spectrum::base_code(x.left);
    code[SITES + 1] = spectrum::base_code(x.right);
#pragma unroll
    for (int i = 0; i < SITES; i++) {
        const uint32_t ch = (x.q[i >> 2] >> (8 * (i & 3))) & 0xffu;
        code[i + 1] = spectrum::base_code(ch);
    }
}
// site i of the lane (0..15): eligible iff no code of the three has the invalid bit
__device__ __forceinline__ bool site_ctx(const uint32_t code[SITES + 2], int i, uint32_t &ctx) {
    ctx = (16 * code[i] + 4 * code[i + 1] + code[i + 2]) & 63u;     // (masked: an ineligible site's value indexes nothing out of range)
    return ((code[i] | code[i + 1] | code[i + 2]) & spectrum::CODE_INVALID) == 0;
}

// 64 lane-private bins, summed in four quarters into the one copy of the result (lane_hist.h).  A workgroup takes at most 512
// tiles (the grid stops at CENSUS_MAX_BLOCKS only beyond that many tiles in all, and a contig has fewer than 2^20), 16 sites a
// lane each: 8192 a counter at most.
__global__ __launch_bounds__(LANES) void k_ctx_census(const uint8_t *__restrict__ b, uint64_t L, uint64_t n_tiles,
                                                      unsigned long long *__restrict__ counts) {
    __shared__ LaneHist<64, LANES, 4> hist;
    hist.zero();
    // CENSUS_AHEAD tiles a round, all their loads in flight before the first is counted (16 waves a CU with one 16-byte load
    // each are little for the memory system to work on; measured it is worth 2 %: the decode below bounds the kernel, NOTES 20)
    for (uint64_t first = blockIdx.x; first < n_tiles; first += (uint64_t)gridDim.x * CENSUS_AHEAD) {
        LaneBytes x[CENSUS_AHEAD];
#pragma unroll
        for (int k = 0; k < CENSUS_AHEAD; k++) {
            const uint64_t tile = first + (uint64_t)k * gridDim.x;
            x[k] = lane_load(b, L, tile < n_tiles ? tile * spectrum::TILE + (uint64_t)threadIdx.x * SITES : L);
        }
#pragma unroll
        for (int k = 0; k < CENSUS_AHEAD; k++) {
            uint32_t code[SITES + 2];
            lane_codes(x[k], code);
#pragma unroll
            for (int i = 0; i < SITES; i++) {
                uint32_t ctx;
                const uint32_t one = site_ctx(code, i, ctx) ? 1u : 0u;
                hist.add(ctx, one);
            }
        }
    }
    hist.flush(counts);
}

__global__ __launch_bounds__(LANES) void k_spectrum_draw(const uint8_t *__restrict__ b, uint64_t L, const uint64_t *__restrict__ thr,
                                                         Key key, uint32_t *__restrict__ words, uint32_t *__restrict__ tile_cnt) {
    __shared__ uint64_t s_thr[192];
    __shared__ uint64_t s_top[64];                          // thr[3 ctx + 2]: at or above it nothing happens
    __shared__ uint32_t s_cnt[LANES / 64];
    if (threadIdx.x < 192) s_thr[threadIdx.x] = thr[threadIdx.x];
    if (threadIdx.x < 64) s_top[threadIdx.x] = thr[3 * threadIdx.x + 2];
    __syncthreads();
    const uint64_t p0 = (uint64_t)blockIdx.x * spectrum::TILE + (uint64_t)threadIdx.x * SITES;
    uint32_t code[SITES + 2];
    lane_codes(lane_load(b, L, p0), code);
    uint32_t word = 0, hits = 0;
#pragma unroll
    for (int k = 0; k < SITES / 2; k++) {                   // p0 is even: sites 2k (low 64 bits) and 2k + 1 (high 64 bits) share a call
        const U4 v = fastrng::draw4(key, (uint32_t)(p0 >> 1) + k, 0, fastrng::TAG_CTX);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int i = 2 * k + h;
            const uint64_t r = h ? fastrng::hi64(v) : fastrng::lo64(v);
            uint32_t ctx, j = 3;
            if (site_ctx(code, i, ctx) && r < s_top[ctx]) {
                j = (uint32_t)(s_thr[3 * ctx] <= r) + (uint32_t)(s_thr[3 * ctx + 1] <= r);
                hits++;
            }
            word |= j << (2 * i);
        }
    }
    words[(uint64_t)blockIdx.x * LANES + threadIdx.x] = word;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = hits;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < LANES / 64; w++) s += s_cnt[w];
        tile_cnt[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(LANES) void k_spectrum_emit(const uint32_t *__restrict__ words, const uint32_t *__restrict__ tile_off,
                                                         msim_record *__restrict__ recs) {
    __shared__ uint32_t s_cnt[LANES / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t word = words[(uint64_t)blockIdx.x * LANES + threadIdx.x];
    uint32_t open = (~word | (~word >> 1)) & 0x55555555u;   // bit 2i: site i's outcome is not 3
    const uint32_t mine = (uint32_t)__popc(open);
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) s_cnt[wave] = incl;
    __syncthreads();
    uint64_t dst = tile_off[blockIdx.x] + (incl - mine);
#pragma unroll
    for (int w = 0; w < LANES / 64 - 1; w++) if (w < wave) dst += s_cnt[w];
    const uint32_t p0 = blockIdx.x * spectrum::TILE + threadIdx.x * SITES;   // (contigs are below 2^32 bases)
    uint4 *out = reinterpret_cast<uint4 *>(recs);
    while (open) {
        const uint32_t bit = (uint32_t)__ffs((int)open) - 1;
        open &= open - 1;
        const uint32_t p = p0 + (bit >> 1), j = (word >> bit) & 3u;
        out[dst++] = make_uint4(p, p, 0u, (uint32_t)MSIM_SN | (j << 8));     // pos, stop, extra, {type, aux, rsv}
    }
}

// ---- the profile: SN records counted into their SBS-96 channels (msim_sbs_counts) ------------------------------------------
constexpr int SBS_AHEAD = 4;                                // records a lane and pass: their loads and gathers are in flight together
constexpr uint32_t SBS_PASS = LANES * SBS_AHEAD;            // records of a workgroup's pass, contiguous: 1 KB a wave and load
static_assert(SBS_PASS == MSIM_SBS_PASS, "msim.h and spectrum.hip must agree on the pass");
constexpr unsigned SBS_MAX_BLOCKS = 512;                    // more passes than that stride (k_sbs_count counts on it); two workgroups a CU:
                                                            // every workgroup pays for zeroing and summing 52 KB of counters (NOTES 21)
constexpr int SBS_BINS = (int)spectrum::SBS_BINS;
static_assert(sizeof(msim_record) == sizeof(uint4), "a record is one 16-byte load");

// The bin of one record ({pos, stop, extra, type | aux << 8 | rsv << 16}): an SN record's channel, 96 (tallies[0]) for an SN
// record without one, 96 + type for every other type; *one = 0 for what is no record (type 0: the padding of the last pass).
// tallies[1] has no bin: the host sums it.  b[p - 1] and b[p + 1] are read only where they lie inside [0, L).
__device__ __forceinline__ uint32_t sbs_bin(const uint8_t *__restrict__ b, uint64_t L, const uint4 &rec, uint32_t *one) {
    const uint32_t p = rec.x, type = rec.w & 0xffu, aux = (rec.w >> 8) & 0xffu;
    *one = (type >= (uint32_t)MSIM_SN && type <= (uint32_t)MSIM_TLI) ? 1u : 0u;
    if (type != (uint32_t)MSIM_SN) return 96u + (*one ? type : 0u);
    uint32_t bin = 96u;
    if (p >= 1 && (uint64_t)p + 1 < L && aux < 3) {
        const uint32_t l = spectrum::base_code(b[p - 1]), m = spectrum::base_code(b[p]), r = spectrum::base_code(b[p + 1]);
        if (((l | m | r) & spectrum::CODE_INVALID) == 0) bin = spectrum::sbs_channel(l, m, r, aux);
    }
    return bin;
}

// 104 lane-private bins, summed in two halves into the workgroup's slot of `out` (lane_hist.h; 52 KB a workgroup, three
// workgroups a CU) -- a real spectrum puts most records into a handful of channels.  A table has fewer than 2^31 records, so
// fewer than 2^21 passes; the grid stops at SBS_MAX_BLOCKS only beyond that many passes: a workgroup takes at most 4096 of
// them, SBS_AHEAD records a lane each -- 16 384 a counter at most, whatever the table holds.
__global__ __launch_bounds__(LANES) void k_sbs_count(const uint8_t *__restrict__ b, uint64_t L, const uint4 *__restrict__ recs,
                                                     uint64_t n_rec, uint64_t n_pass, unsigned long long *__restrict__ out) {
    __shared__ LaneHist<SBS_BINS, LANES, 2> hist;
    hist.zero();
    for (uint64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        uint4 rec[SBS_AHEAD];
#pragma unroll
        for (int k = 0; k < SBS_AHEAD; k++) {
            const uint64_t i = pass * SBS_PASS + (uint64_t)k * LANES + threadIdx.x;
            rec[k] = i < n_rec ? recs[i] : make_uint4(0u, 0u, 0u, 0u);
        }
        uint32_t bin[SBS_AHEAD], one[SBS_AHEAD];
#pragma unroll
        for (int k = 0; k < SBS_AHEAD; k++) bin[k] = sbs_bin(b, L, rec[k], &one[k]);
#pragma unroll
        for (int k = 0; k < SBS_AHEAD; k++) hist.add(bin[k], one[k]);
    }
    hist.flush(out + (blockIdx.x & (HIST_SLOTS - 1)) * SBS_BINS);
}

// bins 0..95 the channels, 96.. the tallies; tallies[1] = every SN record = the channels' sum + tallies[0]
void sbs_finish(const unsigned long long *slots, uint64_t channels[96], uint64_t tallies[8]) {
    unsigned long long bins[SBS_BINS];
    hist_sum_slots(slots, SBS_BINS, bins, SBS_BINS);
    uint64_t sn = bins[96];
    for (int i = 0; i < 96; i++) { channels[i] = bins[i]; sn += bins[i]; }
    for (int t = 0; t < 8; t++) tallies[t] = bins[96 + t];
    tallies[1] = sn;
}

constexpr size_t CENSUS_WORDS = 64, SBS_WORDS = (size_t)HIST_SLOTS * SBS_BINS;

inline uint64_t tiles_of(uint64_t L) { return (L + spectrum::TILE - 1) / spectrum::TILE; }

int state_of(Ctx *c, SpectrumState **out) {
    if (!c->spectrum) {
        SpectrumState *S = new SpectrumState;
        c->spectrum = S;
        MSIM_HIP(c, S->census.create(CENSUS_WORDS));
        MSIM_HIP(c, S->sbs.create(SBS_WORDS));
        MSIM_HIP(c, dev_alloc(S->d_thr, 192 * sizeof(uint64_t)));
        MSIM_HIP(c, pin_alloc(S->h_pin, 193 * sizeof(unsigned long long)));
        MSIM_HIP(c, S->tm.create());
    }
    *out = c->spectrum;
    return MSIM_OK;
}

// end of a timed stretch (begun by tm.begin) that has its copy to the host inside: wait for the stream, add the time
int stretch_end(Ctx *c, SpectrumState *S, double *acc) {
    MSIM_HIP(c, S->tm.end(c->stream));
    MSIM_HIP(c, wait_stream(c->stream));
    return S->tm.add_elapsed(c, acc);
}

int census_device(Ctx *c, SpectrumState *S, const Contig &g, uint64_t counts[64]) {
    if (!g.len) { memset(counts, 0, 64 * sizeof(uint64_t)); return MSIM_OK; }
    int rc = S->census.begin(c, CENSUS_WORDS);
    if (rc) return rc;
    const PassGrid pg = pass_grid(g.len, spectrum::TILE, CENSUS_MAX_BLOCKS);    // (a pass: one tile)
    hipLaunchKernelGGL(k_ctx_census, pg.grid, dim3(LANES), 0, c->stream, g.d_in.p() + PAD, g.len, pg.n_pass, S->census.d.p());
    MSIM_HIP(c, hipGetLastError());
    if ((rc = S->census.finish(c, &S->census_ms))) return rc;
    for (int i = 0; i < 64; i++) counts[i] = S->census.h.p()[i];
    return MSIM_OK;
}

// the contig's ACTIVE table (the caller drained the context: the table is complete, its size collected, nothing writes it)
int sbs_device(Ctx *c, SpectrumState *S, const Contig &g, uint64_t channels[96], uint64_t tallies[8]) {
    memset(channels, 0, 96 * sizeof(uint64_t));
    memset(tallies, 0, 8 * sizeof(uint64_t));
    if (!g.n_rec) return MSIM_OK;
    int rc = S->sbs.begin(c, SBS_WORDS);
    if (rc) return rc;
    const PassGrid pg = pass_grid(g.n_rec, SBS_PASS, SBS_MAX_BLOCKS);
    hipLaunchKernelGGL(k_sbs_count, pg.grid, dim3(LANES), 0, c->stream, g.d_in.p() + PAD, g.len, reinterpret_cast<const uint4 *>(g.d_recs.p()), g.n_rec,
                       pg.n_pass, S->sbs.d.p());
    MSIM_HIP(c, hipGetLastError());
    if ((rc = S->sbs.finish(c, &S->sbs_ms))) return rc;
    sbs_finish(S->sbs.h.p(), channels, tallies);
    return MSIM_OK;
}

// leaves the contig planned as plan_device (vcf_parse.hip) does: an SNP-only table of host-known size, no insert pool
int plan_device(Ctx *c, SpectrumState *S, Contig *g, const uint64_t thr[192], uint64_t key64, uint32_t seq) {
    int rc = ctx_drain(c);                                 // this contig's buffers may still be read by its last APPLY
    if (rc) return rc;
    contig_reset(*g);
    c->text_kind = 0;
    g->apply_stream = nullptr;
    const uint64_t n_tiles = tiles_of(g->len);
    uint64_t n_rec = 0;
    if (n_tiles) {
        rc = dev_reserve(c, S->d_words, (size_t)n_tiles * LANES * sizeof(uint32_t));
        if (!rc) rc = dev_reserve(c, S->d_tile, (size_t)(n_tiles + 1) * sizeof(uint32_t));
        if (rc) return rc;
        memcpy(S->h_pin.p(), thr, 192 * sizeof(uint64_t));
        MSIM_HIP(c, hipMemcpyAsync(S->d_thr.p(), S->h_pin.p(), 192 * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        const Key key{(uint32_t)key64, (uint32_t)(key64 >> 32), seq};
        MSIM_HIP(c, S->tm.begin(c->stream));
        hipLaunchKernelGGL(k_spectrum_draw, dim3((unsigned)n_tiles), dim3(LANES), 0, c->stream, g->d_in.p() + PAD, g->len, S->d_thr.p(), key,
                           S->d_words.p(), S->d_tile.p());
        hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, c->stream, S->d_tile.p(), (uint32_t)n_tiles);
        MSIM_HIP(c, hipGetLastError());
        MSIM_HIP(c, hipMemcpyAsync(S->h_pin.p() + 192, S->d_tile.p() + n_tiles, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if ((rc = stretch_end(c, S, &S->plan_ms))) return rc;
        n_rec = *reinterpret_cast<const uint32_t *>(S->h_pin.p() + 192);
        if (n_rec >= (1ull << 31)) return fail(c, MSIM_ERR_UNSUPPORTED, "2^31 or more mutations on one contig");
    }
    if (n_rec) {
        rc = dev_reserve(c, g->d_recs, (size_t)n_rec * sizeof(msim_record));
        if (rc) return rc;
        MSIM_HIP(c, S->tm.begin(c->stream));
        hipLaunchKernelGGL(k_spectrum_emit, dim3((unsigned)n_tiles), dim3(LANES), 0, c->stream, S->d_words.p(), S->d_tile.p(), g->d_recs.p());
        MSIM_HIP(c, hipGetLastError());
        if ((rc = stretch_end(c, S, &S->plan_ms))) return rc;
    }
    rc = dev_reserve(c, g->d_pool, 2 * PAD);
    if (rc) return rc;
    g->n_rec = n_rec;
    g->pool_len = 0;
    g->plan_empty = n_rec == 0;
    g->all_snp = true;
    g->planned = true;
    return MSIM_OK;
}

bool thresholds_ordered(const uint64_t thr[192], int *bad_ctx) {
    for (int x = 0; x < 64; x++)
        if (thr[3 * x] > thr[3 * x + 1] || thr[3 * x + 1] > thr[3 * x + 2]) { *bad_ctx = x; return false; }
    return true;
}

}  // namespace

void spectrum_state_destroy(Ctx *c) {
    SpectrumState *S = c->spectrum;
    if (!S) return;
    S->tm.destroy();
    delete S;
    c->spectrum = nullptr;
}

void spectrum_reset_timing(Ctx *c) {
    if (c->spectrum) c->spectrum->census_ms = c->spectrum->plan_ms = c->spectrum->sbs_ms = 0;
}

}  // namespace msim

using namespace msim;

extern "C" {

int msim_context_counts(msim_ctx *p, int contig, uint64_t counts[64], uint64_t *n_valid) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !counts || !n_valid) return MSIM_ERR_ARG;
    Contig *g;
    int rc = ctx_device_contig(c, contig, false, &g);
    if (rc) return rc;
    SpectrumState *S;
    if ((rc = state_of(c, &S))) return rc;
    TraceRange tr("msim context census");
    if ((rc = census_device(c, S, *g, counts))) return rc;
    uint64_t n = 0;
    for (int i = 0; i < 64; i++) n += counts[i];
    *n_valid = n;
    return MSIM_OK;
}

int msim_plan_contig_spectrum(msim_ctx *p, int contig, const uint64_t thr[192], uint64_t key, uint32_t seq) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !thr) return MSIM_ERR_ARG;
    Contig *g;
    int rc = ctx_device_contig(c, contig, false, &g);      // (a fast context's queue goes out first)
    if (rc) return rc;
    int bad = 0;
    if (!thresholds_ordered(thr, &bad))
        return fail(c, MSIM_ERR_ARG, "spectrum thresholds of context " + std::to_string(bad) + " are not non-decreasing");
    SpectrumState *S;
    if ((rc = state_of(c, &S))) return rc;
    TraceRange tr("msim PLAN contig (spectrum)");
    return plan_device(c, S, g, thr, key, seq);
}

int msim_spectrum_timing(msim_ctx *p, double *census_ms, double *plan_ms) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    if (census_ms) *census_ms = c->spectrum ? c->spectrum->census_ms : 0.0;
    if (plan_ms) *plan_ms = c->spectrum ? c->spectrum->plan_ms : 0.0;
    return MSIM_OK;
}

// The contig's record table counted against its resident reference bases.  Planned is enough, applied does not matter: d_in
// stays the reference.  With a haplotype selected the active table is that haplotype's (what msim_fetch_records returns).
int msim_sbs_counts(msim_ctx *p, int contig, uint64_t channels[96], uint64_t tallies[8]) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !channels || !tallies) return MSIM_ERR_ARG;
    Contig *g;
    int rc = ctx_device_contig(c, contig, true, &g);
    if (rc) return rc;
    SpectrumState *S;
    if ((rc = state_of(c, &S))) return rc;
    TraceRange tr("msim SBS-96 profile");
    return sbs_device(c, S, *g, channels, tallies);
}

int msim_sbs_timing(msim_ctx *p, double *kernel_ms) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    if (kernel_ms) *kernel_ms = c->spectrum ? c->spectrum->sbs_ms : 0.0;
    return MSIM_OK;
}

// measurement support (tools/sbs_profile_bench.py; exported, not part of msim.h): a device-to-device copy of the contig's active
// record table into the context's scratch, timed by HIP events -- the streaming floor msim_sbs_counts' kernel is held against
int msim_dbg_sbs_copy_floor(msim_ctx *p, int contig, double *ms) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !ms) return MSIM_ERR_ARG;
    Contig *g;
    int rc = ctx_device_contig(c, contig, true, &g);
    if (rc) return rc;
    SpectrumState *S;
    if ((rc = state_of(c, &S))) return rc;
    const CopySource table{g->d_recs.p(), (size_t)g->n_rec * sizeof(msim_record)};
    return copy_floor(c, S->tm, &table, 1, ms);
}

// ---- sequential host restatements: no context, no GPU ------------------------------------------------------------------
int msim_dbg_context_counts(const uint8_t *bases, uint64_t L, uint64_t counts[64], uint64_t *n_valid) {
    if ((!bases && L) || !counts || !n_valid) return MSIM_ERR_ARG;
    memset(counts, 0, 64 * sizeof(uint64_t));
    uint64_t n = 0;
    for (uint64_t q = 1; q + 1 < L; q++) {
        const uint32_t a = spectrum::base_code(bases[q - 1]), m = spectrum::base_code(bases[q]), z = spectrum::base_code(bases[q + 1]);
        if ((a | m | z) & spectrum::CODE_INVALID) continue;
        counts[16 * a + 4 * m + z]++;
        n++;
    }
    *n_valid = n;
    return MSIM_OK;
}

int msim_dbg_spectrum_plan(const uint8_t *bases, uint64_t L, const uint64_t thr[192], uint64_t key, uint32_t seq, msim_record *recs,
                           uint64_t cap, uint64_t *n_recs) {
    if ((!bases && L) || !thr || !n_recs) return MSIM_ERR_ARG;
    if (L >= (1ull << 32)) return fail(nullptr, MSIM_ERR_UNSUPPORTED, "contig of 4 GiB or more");
    int bad = 0;
    if (!thresholds_ordered(thr, &bad))
        return fail(nullptr, MSIM_ERR_ARG, "spectrum thresholds of context " + std::to_string(bad) + " are not non-decreasing");
    const Key k{(uint32_t)key, (uint32_t)(key >> 32), seq};
    uint64_t n = 0;
    for (uint64_t q = 1; q + 1 < L; q++) {
        const uint32_t a = spectrum::base_code(bases[q - 1]), m = spectrum::base_code(bases[q]), z = spectrum::base_code(bases[q + 1]);
        if ((a | m | z) & spectrum::CODE_INVALID) continue;
        const U4 v = fastrng::draw4(k, (uint32_t)(q >> 1), 0, fastrng::TAG_CTX);
        const uint32_t j = spectrum::outcome(thr + 3 * (16 * a + 4 * m + z), spectrum::site_bits(v, q));
        if (j == 3) continue;
        if (recs) {
            if (n >= cap) return fail(nullptr, MSIM_ERR_ARG, "buffers too small");
            recs[n] = msim_record{(uint32_t)q, (uint32_t)q, 0u, (uint8_t)MSIM_SN, (uint8_t)j, 0};
        }
        n++;
    }
    if (n >= (1ull << 31)) return fail(nullptr, MSIM_ERR_UNSUPPORTED, "2^31 or more mutations on one contig");
    *n_recs = n;
    return MSIM_OK;
}

int msim_dbg_sbs_counts(const uint8_t *bases, uint64_t L, const msim_record *recs, uint64_t n_records, uint64_t channels[96],
                        uint64_t tallies[8]) {
    if ((!bases && L) || (!recs && n_records) || !channels || !tallies) return MSIM_ERR_ARG;
    memset(channels, 0, 96 * sizeof(uint64_t));
    memset(tallies, 0, 8 * sizeof(uint64_t));
    for (uint64_t i = 0; i < n_records; i++) {
        const msim_record &r = recs[i];
        if (r.type < MSIM_SN || r.type > MSIM_TLI) return fail(nullptr, MSIM_ERR_ARG, "record " + std::to_string(i) + ": unknown type");
        tallies[r.type]++;
        if (r.type != MSIM_SN) continue;
        const uint64_t q = r.pos;
        uint32_t a = spectrum::CODE_INVALID, m = a, z = a;
        if (q >= 1 && q + 1 < L && r.aux < 3) {
            a = spectrum::base_code(bases[q - 1]); m = spectrum::base_code(bases[q]); z = spectrum::base_code(bases[q + 1]);
        }
        if ((a | m | z) & spectrum::CODE_INVALID) tallies[0]++;
        else channels[spectrum::sbs_channel(a, m, z, r.aux)]++;
    }
    return MSIM_OK;
}

}  // extern "C"
