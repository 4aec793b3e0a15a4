// compare --diploid --phased (msim_cmp_phase_*): switch errors, flips and blockwise Hamming distance of the calls' phasing against the
// truth's, on the two diploid tables msim_cmp_join left and the flag bytes of msim_cmp_counts_diploid -- rules in include/msim.h, shared
// arithmetic in cmp_phase.h.  One lane per record (or pair) and one workgroup per MSIM_CMP_PHASE_TILE of them, everywhere:
//   mark      k_cons_phase: one lane per record of the table the consensus parser just left -- through the parser's record-to-line
//             index it reaches its line and evaluates vcf_cons_phase (vcf_parse.h); (pos, word) are kept as the haplotype's MARKS
//   join      k_phase_join: one lane per record of a side's diploid table U -- a binary search of the marks of the haplotype its
//             genotype byte names gives its word
//   pairs     k_phase_pairs: one lane per truth record -- is it informative (cmp::partner again, only for a phased het the match
//             flagged 1), its orientation and its partner's word; the tile's informative records are counted
//   compact   k_scan_u32 over the tiles' counts, k_phase_compact: the pairs in truth-table order as a dense sequence
//   tally     k_phase_reduce, k_phase_tilescan, k_phase_tally: one scan of phase::Scan over the dense sequence (a tile's total, the
//             totals' prefixes, the tile again with its prefix); a block is counted at its last pair, a switch run at its last bit
// Counters are summed over the workgroup (wave shuffles, then LDS) and added to the result with one atomic per counter and workgroup.
// Every index is checked against its table's size; the dense sequence is no longer than the truth's table, which sizes its buffers.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "cmp_phase.h"
#include "counter_trip.h"
#include "ctx.h"
#include "scan_kernels.h"
#include "vcf_parse.h"

namespace msim {

namespace {
struct Mark { uint32_t pos, word; };
struct Marks {                                 // msim_cmp_phase_mark's result for one haplotype
    bool have = false;
    Scratch<Mark> d;
    uint64_t n = 0;
};
struct PhaseSide {
    Marks marks[2];                            // haplotype 1, haplotype 2
    bool have_words = false;
    Scratch<uint32_t> d_words;                 // a word per record of the side's U
    uint64_t n = 0;
};
struct PhaseContig {
    PhaseSide side[2];                         // MSIM_CMP_TRUTH, MSIM_CMP_CALLS
    Scratch<uint8_t> d_state;                  // a state byte per truth record (the last msim_cmp_phase_counts)
    uint64_t n_state = 0;
    bool counted = false;
};
}  // namespace

struct PhaseState {
    std::vector<PhaseContig> contigs;          // by contig index
    // the pass's scratch (grow-only): per truth record its partner's word; per tile its pairs (then their exclusive scan, the total
    // last); the dense sequence -- key, orientation, truth record --; per dense tile its Scan total and the prefix in front of it
    Scratch<uint32_t> d_pkey, d_tile, d_src;
    Scratch<uint2> d_key;
    Scratch<uint8_t> d_orient;
    Scratch<phase::Scan> d_agg, d_pre;
    CounterTrip out;                           // PHASE_OUT_WORDS counters; its events time the word join as well
    double kernel_ms = 0;
};

namespace {

constexpr int LANES = MSIM_CMP_PHASE_TILE, WAVES = LANES / 64;
constexpr uint32_t TILE = MSIM_CMP_PHASE_TILE;
static_assert(LANES == 256, "the kernels are written for four waves a workgroup");
static_assert(sizeof(msim_record) == sizeof(uint4), "a record is one 16-byte load");
// the device's counters: phase::C_* (C_ASSESSED is left to the host), the mark's three tallies behind them
constexpr uint32_t OUT_MARK = phase::COUNTS, PHASE_OUT_WORDS = 16;

// the workgroup's sums of K values a lane, in every lane (two barriers)
template <int K>
__device__ __forceinline__ void block_sums(const unsigned long long (&v)[K], unsigned long long *lds, unsigned long long (&total)[K]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                       // (whoever read lds last has done so)
#pragma unroll
    for (int q = 0; q < K; q++) {
        unsigned long long x = v[q];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) x += __shfl_down(x, d, 64);
        if (lane == 0) lds[wave * K + q] = x;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < K; q++) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) t += lds[w * K + q];
        total[q] = t;
    }
}

// the lanes of the workgroup in front of this one with f set; *total: all of them
__device__ __forceinline__ uint32_t block_rank(bool f, uint32_t *lds, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(f);
    __syncthreads();
    if (lane == 0) lds[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) { const uint32_t s = lds[w]; pre += w < wave ? s : 0u; tot += s; }
    *total = tot;
    return pre + (uint32_t)__popcll(b & ((1ull << lane) - 1));
}

// the inclusive scan of phase::Scan over the workgroup's lanes; *total: the last lane's
__device__ __forceinline__ phase::Scan block_scan(phase::Scan v, phase::Scan *lds, phase::Scan *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    phase::Scan inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const phase::Scan u{__shfl_up(inc.block, d, 64), __shfl_up(inc.ones, d, 64), __shfl_up(inc.calm, d, 64)};
        if (lane >= d) inc = phase::join(u, inc);
    }
    __syncthreads();
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    phase::Scan base{0, 0, 0}, tot{0, 0, 0};
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        const phase::Scan s = lds[w];
        if (w < wave) base = phase::join(base, s);
        tot = phase::join(tot, s);
    }
    *total = tot;
    return phase::join(base, inc);
}

// ---- mark and join -------------------------------------------------------------------------------------------------------------------
// recline[r] < n_lines is checked: the line's bytes are [ls[idx], ls[idx + 1] - 1), idx < the text's lines.
__global__ __launch_bounds__(LANES) void k_cons_phase(const uint8_t *__restrict__ t, const uint64_t *__restrict__ ls, const uint32_t *__restrict__ tabcum,
                                                      const uint32_t *__restrict__ recline, const msim_record *__restrict__ recs, uint64_t n_rec,
                                                      uint64_t first, uint64_t n_lines, uint32_t nf0, uint32_t sample, Mark *__restrict__ marks,
                                                      unsigned long long *__restrict__ out) {
    __shared__ unsigned long long lds[WAVES * 3];
    const uint64_t r = (uint64_t)blockIdx.x * TILE + threadIdx.x;
    unsigned long long v[3] = {0, 0, 0}, total[3];         // phased, unphased, unreadable
    if (r < n_rec) {
        const uint32_t line = recline[r];
        uint32_t word = 0;
        bool unreadable = false;
        if (line < n_lines) {
            const uint64_t idx = first + line;
            word = vcf_cons_phase(t, ls[idx], ls[idx + 1] - 1, tabcum[idx + 1] - tabcum[idx], nf0, sample, &unreadable);
        }
        marks[r] = Mark{cmp::rec_at(recs, r).pos, word};
        v[unreadable ? 2 : word ? 0 : 1] = 1;
    }
    block_sums<3>(v, lds, total);
    if (threadIdx.x < 3 && total[threadIdx.x]) atomicAdd(&out[OUT_MARK + threadIdx.x], total[threadIdx.x]);
}

// the word of the mark at `pos` (marks: pos strictly increasing), 0: none there
__device__ __forceinline__ uint32_t mark_word(const Mark *__restrict__ m, uint64_t n, uint32_t pos) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (m[mid].pos < pos) lo = mid + 1; else hi = mid;
    }
    if (lo >= n) return 0;
    const Mark x = m[lo];
    return x.pos == pos ? x.word : 0u;
}

__global__ __launch_bounds__(LANES) void k_phase_join(const msim_record *__restrict__ U, const uint8_t *__restrict__ gt, uint64_t n,
                                                      const Mark *__restrict__ m1, uint64_t n1, const Mark *__restrict__ m2, uint64_t n2,
                                                      uint32_t *__restrict__ words) {
    const uint64_t i = (uint64_t)blockIdx.x * TILE + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = gt[i], pos = cmp::rec_at(U, i).pos;
    words[i] = (g & 1u) ? mark_word(m1, n1, pos) : g == 2u ? mark_word(m2, n2, pos) : 0u;
}

// ---- the pass ------------------------------------------------------------------------------------------------------------------------
// One lane per record of either table (the grid covers the longer one): the truth's record i is judged, the calls' record i only
// counted.  state[i]: 0 or ST_INFORMATIVE with the orientation; pkey[i]: the partner's word; tile_cnt[tile]: the tile's pairs.
__global__ __launch_bounds__(LANES) void k_phase_pairs(const uint8_t *__restrict__ g, uint64_t L, cmp::Table A, cmp::Table B,
                                                       const uint8_t *__restrict__ gt_a, const uint8_t *__restrict__ gt_b,
                                                       const uint8_t *__restrict__ flag_a, const uint32_t *__restrict__ w_a,
                                                       const uint32_t *__restrict__ w_b, uint32_t exact, uint8_t *__restrict__ state,
                                                       uint32_t *__restrict__ pkey, uint32_t *__restrict__ tile_cnt, uint32_t tiles_a,
                                                       unsigned long long *__restrict__ out) {
    __shared__ unsigned long long lds[WAVES * 3];
    const uint64_t i = (uint64_t)blockIdx.x * TILE + threadIdx.x;
    unsigned long long v[3] = {0, 0, 0}, total[3];         // pairs, truth phased hets, calls phased hets
    if (i < A.n) {
        uint32_t key_b;
        const uint8_t st = phase::pair_state(g, L, A, i, B, exact != 0, flag_a[i], gt_a, gt_b, w_a, w_b, &key_b);
        state[i] = st;
        pkey[i] = key_b;
        v[0] = st != 0;
        v[1] = phase::phased_het(gt_a[i], w_a[i]);
    }
    if (i < B.n) v[2] = phase::phased_het(gt_b[i], w_b[i]);
    block_sums<3>(v, lds, total);
    if (threadIdx.x == 0) {
        if (blockIdx.x < tiles_a) tile_cnt[blockIdx.x] = (uint32_t)total[0];
        if (total[1]) atomicAdd(&out[phase::C_TRUTH_HETS], total[1]);
        if (total[2]) atomicAdd(&out[phase::C_CALLS_HETS], total[2]);
    }
}

// tile_off: the exclusive scan of k_phase_pairs' counts.  cap: the dense buffers' records (the truth's).
__global__ __launch_bounds__(LANES) void k_phase_compact(uint64_t n, const uint8_t *__restrict__ state, const uint32_t *__restrict__ w_a,
                                                         const uint32_t *__restrict__ pkey, const uint32_t *__restrict__ tile_off,
                                                         uint2 *__restrict__ key, uint8_t *__restrict__ orient, uint32_t *__restrict__ src, uint64_t cap) {
    __shared__ uint32_t lds[WAVES];
    const uint64_t i = (uint64_t)blockIdx.x * TILE + threadIdx.x;
    const uint8_t st = i < n ? state[i] : (uint8_t)0;
    uint32_t total;
    const uint64_t at = (uint64_t)tile_off[blockIdx.x] + block_rank(st != 0, lds, &total);
    if (!st || at >= cap) return;
    key[at] = make_uint2(w_a[i], pkey[i]);
    orient[at] = (st & phase::ST_ORIENTATION) ? 1 : 0;
    src[at] = (uint32_t)i;
}

// pair k of P: what it adds to the scan (k >= P: nothing)
__device__ __forceinline__ phase::Scan pair_element(const uint2 *__restrict__ key, const uint8_t *__restrict__ orient, uint64_t k, uint64_t P, uint2 *own,
                                                    uint32_t *o) {
    if (k >= P) return phase::Scan{0, 0, 0};
    const uint2 x = key[k];
    const uint32_t ox = orient[k];
    *own = x;
    *o = ox;
    bool starts = true, sw = false;
    if (k > 0) {
        const uint2 p = key[k - 1];
        starts = p.x != x.x || p.y != x.y;
        sw = !starts && orient[k - 1] != ox;
    }
    return phase::element((uint32_t)k, starts, ox, sw);
}

// n_pairs: the word behind the tiles' scan; cap: the dense buffers' records
__global__ __launch_bounds__(LANES) void k_phase_reduce(const uint2 *__restrict__ key, const uint8_t *__restrict__ orient, const uint32_t *__restrict__ n_pairs,
                                                        uint64_t cap, phase::Scan *__restrict__ agg) {
    __shared__ phase::Scan lds[WAVES];
    const uint64_t found = *n_pairs, P = found < cap ? found : cap, k = (uint64_t)blockIdx.x * TILE + threadIdx.x;
    uint2 own;
    uint32_t o;
    phase::Scan total;
    (void)block_scan(pair_element(key, orient, k, P, &own, &o), lds, &total);
    if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// one workgroup: pre[t] = the join of agg[0 .. t), t = 0 .. n_tiles
__global__ __launch_bounds__(LANES) void k_phase_tilescan(const phase::Scan *__restrict__ agg, uint32_t n_tiles, phase::Scan *__restrict__ pre) {
    __shared__ phase::Scan lds[WAVES];
    phase::Scan carry{0, 0, 0};
    if (threadIdx.x == 0) pre[0] = carry;
    for (uint32_t base = 0; base < n_tiles; base += TILE) {
        const uint32_t t = base + threadIdx.x;
        phase::Scan total;
        const phase::Scan inc = block_scan(t < n_tiles ? agg[t] : phase::Scan{0, 0, 0}, lds, &total);
        if (t < n_tiles) pre[t + 1] = phase::join(carry, inc);
        carry = phase::join(carry, total);
    }
}

// n_rec: the truth's records (state's bytes)
__global__ __launch_bounds__(LANES) void k_phase_tally(const uint2 *__restrict__ key, const uint8_t *__restrict__ orient, const uint32_t *__restrict__ src,
                                                       const uint32_t *__restrict__ n_pairs, uint64_t cap, const phase::Scan *__restrict__ pre,
                                                       uint8_t *__restrict__ state, uint64_t n_rec, unsigned long long *__restrict__ out) {
    __shared__ phase::Scan lds[WAVES];
    __shared__ unsigned long long sums[WAVES * 8];
    const uint64_t found = *n_pairs, P = found < cap ? found : cap, k = (uint64_t)blockIdx.x * TILE + threadIdx.x;
    uint2 own = make_uint2(0, 0);
    uint32_t o = 0;
    phase::Scan total;
    const phase::Scan e = pair_element(key, orient, k, P, &own, &o);
    const phase::Scan inc = phase::join(pre[blockIdx.x], block_scan(e, lds, &total));
    // pairs, blocks, singletons, raw switch bits, switches, flips, Hamming, pairs in blocks of two or more
    unsigned long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sum[8];
    if (k < P) {
        const bool sw = e.calm == 0;
        bool ends = true, sw_next = false;                 // the block ends here; the next pair carries a raw switch bit
        if (k + 1 < P) {
            const uint2 nx = key[k + 1];
            ends = nx.x != own.x || nx.y != own.y;
            sw_next = !ends && orient[k + 1] != o;
        }
        v[0] = 1;
        v[1] = e.block != 0;
        v[3] = sw;
        if (sw && !sw_next) {                              // the run's last bit: inc.calm - 1 is the pair in front of its first
            const uint64_t r = k + 1 - inc.calm;
            v[4] = phase::run_switches(r);
            v[5] = phase::run_flips(r);
        }
        if (ends) {                                        // inc.block - 1 is the block's first pair
            const uint64_t size = k + 2 - inc.block, ones = inc.ones;
            v[2] = size == 1;
            v[6] = ones < size - ones ? ones : size - ones;
            v[7] = size >= 2 ? size : 0;
        }
        const uint32_t i = src[k];
        if (i < n_rec) state[i] = (uint8_t)(phase::ST_INFORMATIVE | (sw ? phase::ST_SWITCH : 0) | (o ? phase::ST_ORIENTATION : 0));
    }
    block_sums<8>(v, sums, sum);
    constexpr uint32_t AT[8] = {phase::C_PAIRS, phase::C_BLOCKS, phase::C_SINGLETONS, phase::C_RAW, phase::C_SWITCHES, phase::C_FLIPS, phase::C_HAMMING,
                                phase::C_PAIRS_BLOCKED};
    if (threadIdx.x < 8 && sum[threadIdx.x]) atomicAdd(&out[AT[threadIdx.x]], sum[threadIdx.x]);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
unsigned tiles_of(uint64_t n) { return (unsigned)((n + TILE - 1) / TILE); }

int state_of(Ctx *c, PhaseState **out) {
    PhaseState **slot;
    int rc = compare_phase_slot(c, &slot);
    if (!rc) rc = lazy_state(c, slot, PHASE_OUT_WORDS, "the phase pass's result buffers and events");
    if (!rc) *out = *slot;
    return rc;
}

PhaseContig &contig_of(PhaseState *P, int contig) {
    if (P->contigs.size() <= (size_t)contig) P->contigs.resize((size_t)contig + 1);
    return P->contigs[(size_t)contig];
}

const char *side_refusal(int side) { return side != MSIM_CMP_TRUTH && side != MSIM_CMP_CALLS ? "unknown side (MSIM_CMP_TRUTH, MSIM_CMP_CALLS)" : nullptr; }

// a device call's prologue: a GPU context and a contig of that index
int device_contig(Ctx *c, int contig, Contig **g) {
    if (c->host_only) return fail(c, MSIM_ERR_HIP, "host-only context: this call needs the GPU");
    return ctx_device_contig(c, contig, false, g);
}

int counts_device(Ctx *c, PhaseState *P, const Contig &g, PhaseContig &pc, const DipView &a, const DipView &b, uint32_t flags, uint64_t *out) {
    const uint64_t na = a.t.n, nb = b.t.n;
    pc.counted = false;
    if (!na && !nb) { pc.n_state = 0; pc.counted = true; return MSIM_OK; }
    const unsigned tiles_a = tiles_of(na);
    int rc;
    MSIM_HIP(c, dev_at_least(pc.d_state, (size_t)na));
    if ((rc = dev_reserve(c, P->d_pkey, (size_t)std::max<uint64_t>(na, 1) * sizeof(uint32_t))) ||
        (rc = dev_reserve(c, P->d_src, (size_t)std::max<uint64_t>(na, 1) * sizeof(uint32_t))) ||
        (rc = dev_reserve(c, P->d_key, (size_t)std::max<uint64_t>(na, 1) * sizeof(uint2))) ||
        (rc = dev_reserve(c, P->d_orient, (size_t)std::max<uint64_t>(na, 1))) ||
        (rc = dev_reserve(c, P->d_tile, ((size_t)tiles_a + 1) * sizeof(uint32_t))) ||
        (rc = dev_reserve(c, P->d_agg, ((size_t)tiles_a + 1) * sizeof(phase::Scan))) ||
        (rc = dev_reserve(c, P->d_pre, ((size_t)tiles_a + 1) * sizeof(phase::Scan))))
        return rc;
    const uint32_t *w_a = pc.side[MSIM_CMP_TRUTH].d_words.p(), *w_b = pc.side[MSIM_CMP_CALLS].d_words.p();
    if ((rc = P->out.begin(c, PHASE_OUT_WORDS))) return rc;
    hipLaunchKernelGGL(k_phase_pairs, dim3(tiles_of(std::max(na, nb))), dim3(LANES), 0, c->stream, g.d_in.p() + PAD, g.len, a.t, b.t, a.gt, b.gt, a.flag, w_a,
                       w_b, flags & MSIM_CMP_EXACT, pc.d_state.p(), P->d_pkey.p(), P->d_tile.p(), tiles_a, P->out.d.p());
    MSIM_HIP(c, hipGetLastError());
    if (na) {
        const uint32_t *n_pairs = P->d_tile.p() + tiles_a;
        hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, c->stream, P->d_tile.p(), tiles_a);
        hipLaunchKernelGGL(k_phase_compact, dim3(tiles_a), dim3(LANES), 0, c->stream, na, (const uint8_t *)pc.d_state.p(), w_a, (const uint32_t *)P->d_pkey.p(),
                           (const uint32_t *)P->d_tile.p(), P->d_key.p(), P->d_orient.p(), P->d_src.p(), na);
        hipLaunchKernelGGL(k_phase_reduce, dim3(tiles_a), dim3(LANES), 0, c->stream, (const uint2 *)P->d_key.p(), (const uint8_t *)P->d_orient.p(), n_pairs, na,
                           P->d_agg.p());
        hipLaunchKernelGGL(k_phase_tilescan, dim3(1), dim3(LANES), 0, c->stream, (const phase::Scan *)P->d_agg.p(), tiles_a, P->d_pre.p());
        hipLaunchKernelGGL(k_phase_tally, dim3(tiles_a), dim3(LANES), 0, c->stream, (const uint2 *)P->d_key.p(), (const uint8_t *)P->d_orient.p(),
                           (const uint32_t *)P->d_src.p(), n_pairs, na, (const phase::Scan *)P->d_pre.p(), pc.d_state.p(), na, P->out.d.p());
        MSIM_HIP(c, hipGetLastError());
    }
    if ((rc = P->out.finish(c, &P->kernel_ms))) return rc;
    const unsigned long long *h = P->out.h.p();
    if (h[phase::C_PAIRS] > na || h[phase::C_BLOCKS] > h[phase::C_PAIRS])
        return fail(c, MSIM_ERR_HIP, "internal: the phase pass counted more pairs than the truth holds records");
    for (uint32_t k = 0; k < phase::COUNTS; k++) out[k] = h[k];
    out[phase::C_ASSESSED] = h[phase::C_PAIRS] - h[phase::C_BLOCKS];
    pc.n_state = na;
    pc.counted = true;
    return MSIM_OK;
}

}  // namespace

void phase_drop_side(PhaseState *P, int contig, int side) {
    if (!P || contig < 0 || (size_t)contig >= P->contigs.size() || side < 0 || side > 1) return;
    PhaseContig &pc = P->contigs[(size_t)contig];
    PhaseSide &s = pc.side[side];
    s.have_words = false;
    (void)s.d_words.release();
    s.n = 0;
    pc.counted = false;
}

void phase_drop(PhaseState *P, int contig) {
    if (!P) return;
    if (contig < 0) P->contigs.clear();
    else if ((size_t)contig < P->contigs.size()) P->contigs[(size_t)contig] = PhaseContig{};
}

void phase_state_destroy(PhaseState *P) { delete P; }

void phase_reset_timing(PhaseState *P) {
    if (P) P->kernel_ms = 0;
}

}  // namespace msim

using namespace msim;

extern "C" {

int msim_cmp_phase_mark(msim_ctx *p, int contig, int side, int haplotype, uint64_t tally[3]) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !tally) return MSIM_ERR_ARG;
    Contig *g;
    int rc = device_contig(c, contig, &g);
    if (rc) return rc;
    if (const char *why = side_refusal(side)) return fail(c, MSIM_ERR_ARG, why);
    if (haplotype != 1 && haplotype != 2) return fail(c, MSIM_ERR_ARG, "unknown haplotype (1, 2)");
    VcfPlanView v;
    if (!vcf_last_plan(c, contig, &v))
        return fail(c, MSIM_ERR_ARG, "msim_cmp_phase_mark belongs directly behind a consensus-grammar msim_vcf_plan_contig of the contig, its text loaded");
    PhaseState *P;
    if ((rc = state_of(c, &P))) return rc;
    tally[0] = tally[1] = tally[2] = 0;
    Marks &m = contig_of(P, contig).side[side].marks[haplotype - 1];
    m = Marks{};
    if (v.n_rec) {
        MSIM_HIP(c, dev_alloc(m.d, (size_t)v.n_rec * sizeof(Mark)));
        if ((rc = P->out.begin(c, PHASE_OUT_WORDS))) { m = Marks{}; return rc; }
        hipLaunchKernelGGL(k_cons_phase, dim3(tiles_of(v.n_rec)), dim3(LANES), 0, c->stream, v.text, v.ls, v.tabcum, v.recline,
                           (const msim_record *)g->d_recs.p(), v.n_rec, v.first, v.n_lines, v.nf0, v.sample, m.d.p(), P->out.d.p());
        MSIM_HIP(c, hipGetLastError());
        if ((rc = P->out.finish(c, &P->kernel_ms))) { m = Marks{}; return rc; }
        for (int k = 0; k < 3; k++) tally[k] = P->out.h.p()[OUT_MARK + k];
    }
    m.n = v.n_rec;
    m.have = true;
    return MSIM_OK;
}

int msim_cmp_phase_join(msim_ctx *p, int contig, int side) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    Contig *g;
    int rc = device_contig(c, contig, &g);
    if (rc) return rc;
    if (const char *why = side_refusal(side)) return fail(c, MSIM_ERR_ARG, why);
    DipView d;
    bool counted;
    uint32_t counted_flags;
    if (!compare_dip_view(c, contig, side, &d, &counted, &counted_flags)) return fail(c, MSIM_ERR_ARG, "contig has no diploid table of that side (msim_cmp_join)");
    PhaseState *P;
    if ((rc = state_of(c, &P))) return rc;
    PhaseContig &pc = contig_of(P, contig);
    PhaseSide &s = pc.side[side];
    if (!s.marks[0].have || !s.marks[1].have) return fail(c, MSIM_ERR_ARG, "contig has no marks of both haplotypes of that side (msim_cmp_phase_mark)");
    pc.counted = false;
    s.have_words = false;
    MSIM_HIP(c, dev_exact(s.d_words, (size_t)d.t.n * sizeof(uint32_t)));
    if (d.t.n) {
        MSIM_HIP(c, P->out.tm.begin(c->stream));
        hipLaunchKernelGGL(k_phase_join, dim3(tiles_of(d.t.n)), dim3(LANES), 0, c->stream, d.t.recs, d.gt, d.t.n, (const Mark *)s.marks[0].d.p(), s.marks[0].n,
                           (const Mark *)s.marks[1].d.p(), s.marks[1].n, s.d_words.p());
        MSIM_HIP(c, hipGetLastError());
        MSIM_HIP(c, P->out.tm.end(c->stream));
        MSIM_HIP(c, wait_stream(c->stream));
        if ((rc = P->out.tm.add_elapsed(c, &P->kernel_ms))) return rc;
    }
    s.marks[0] = Marks{};
    s.marks[1] = Marks{};
    s.n = d.t.n;
    s.have_words = true;
    return MSIM_OK;
}

int msim_cmp_phase_set(msim_ctx *p, int contig, int side, const uint32_t *words, uint64_t n) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || (!words && n)) return MSIM_ERR_ARG;
    Contig *g;
    int rc = device_contig(c, contig, &g);
    if (rc) return rc;
    if (const char *why = side_refusal(side)) return fail(c, MSIM_ERR_ARG, why);
    DipView d;
    bool counted;
    uint32_t counted_flags;
    if (!compare_dip_view(c, contig, side, &d, &counted, &counted_flags)) return fail(c, MSIM_ERR_ARG, "contig has no diploid table of that side (msim_cmp_join)");
    if (n != d.t.n) return fail(c, MSIM_ERR_ARG, "msim_cmp_phase_set: " + std::to_string(n) + " words for a diploid table of " + std::to_string(d.t.n) + " records");
    PhaseState *P;
    if ((rc = state_of(c, &P))) return rc;
    PhaseContig &pc = contig_of(P, contig);
    PhaseSide &s = pc.side[side];
    pc.counted = false;
    s.have_words = false;
    MSIM_HIP(c, dev_exact(s.d_words, (size_t)n * sizeof(uint32_t)));
    if (n) {
        MSIM_HIP(c, hipMemcpyAsync(s.d_words.p(), words, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        MSIM_HIP(c, wait_stream(c->stream));
    }
    s.n = n;
    s.have_words = true;
    return MSIM_OK;
}

int msim_cmp_phase_counts(msim_ctx *p, int contig, uint32_t flags, uint64_t out[MSIM_CMP_PHASE_COUNTS]) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !out) return MSIM_ERR_ARG;
    Contig *g;
    int rc = device_contig(c, contig, &g);
    if (rc) return rc;
    if (flags & ~(uint32_t)MSIM_CMP_EXACT) return fail(c, MSIM_ERR_ARG, "unknown compare flag");
    DipView a, b;
    bool counted = false, counted_b;
    uint32_t counted_flags = 0, flags_b;
    if (!compare_dip_view(c, contig, MSIM_CMP_TRUTH, &a, &counted, &counted_flags) || !compare_dip_view(c, contig, MSIM_CMP_CALLS, &b, &counted_b, &flags_b))
        return fail(c, MSIM_ERR_ARG, "contig has no diploid table of both sides (msim_cmp_join)");
    if (!counted || counted_flags != flags)
        return fail(c, MSIM_ERR_ARG, "msim_cmp_phase_counts belongs behind msim_cmp_counts_diploid of the contig with the same flags");
    PhaseState *P;
    if ((rc = state_of(c, &P))) return rc;
    PhaseContig &pc = contig_of(P, contig);
    const PhaseSide &sa = pc.side[MSIM_CMP_TRUTH], &sb = pc.side[MSIM_CMP_CALLS];
    if (!sa.have_words || !sb.have_words || sa.n != a.t.n || sb.n != b.t.n)
        return fail(c, MSIM_ERR_ARG, "contig has no phase words of both sides (msim_cmp_phase_join, msim_cmp_phase_set)");
    memset(out, 0, MSIM_CMP_PHASE_COUNTS * sizeof(uint64_t));
    TraceRange tr("msim compare phase");
    return counts_device(c, P, *g, pc, a, b, flags, out);
}

int msim_cmp_fetch_phase(msim_ctx *p, int contig, int side, uint32_t *words, uint8_t *state) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    Contig *g;
    int rc = device_contig(c, contig, &g);
    if (rc) return rc;
    if (const char *why = side_refusal(side)) return fail(c, MSIM_ERR_ARG, why);
    PhaseState *P;
    if ((rc = state_of(c, &P))) return rc;
    PhaseContig &pc = contig_of(P, contig);
    const PhaseSide &s = pc.side[side];
    if (!s.have_words) return fail(c, MSIM_ERR_ARG, "contig has no phase words of that side (msim_cmp_phase_join, msim_cmp_phase_set)");
    if (state && side != MSIM_CMP_TRUTH) return fail(c, MSIM_ERR_ARG, "the state bytes are the truth's");
    if (state && !pc.counted) return fail(c, MSIM_ERR_ARG, "the state bytes are those of the contig's last msim_cmp_phase_counts: call it first");
    if (words && s.n) MSIM_HIP(c, hipMemcpyAsync(words, s.d_words.p(), (size_t)s.n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (state && pc.n_state) MSIM_HIP(c, hipMemcpyAsync(state, pc.d_state.p(), (size_t)pc.n_state, hipMemcpyDeviceToHost, c->stream));
    MSIM_HIP(c, wait_stream(c->stream));
    return MSIM_OK;
}

int msim_cmp_phase_timing(msim_ctx *p, double *kernel_ms) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    PhaseState **slot = nullptr;
    if (kernel_ms) *kernel_ms = 0.0;
    if (!c->host_only && c->compare && !compare_phase_slot(c, &slot) && *slot && kernel_ms) *kernel_ms = (*slot)->kernel_ms;
    return MSIM_OK;
}

// measurement support (tools/compare_bench.py --phased; exported, not part of msim.h): a device-to-device copy of the bytes the
// phase pass of the contig reads and writes once -- both tables' records, genotype bytes and words, the truth's flag bytes read;
// per truth record the partner's word, the dense sequence (key, orientation, record) and the state byte written and read again
// (as many bytes copied: an upper bound, the dense sequence is as long as the pairs) -- timed by HIP events: the streaming floor
int msim_dbg_cmp_phase_copy_floor(msim_ctx *p, int contig, double *ms) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !ms) return MSIM_ERR_ARG;
    Contig *g;
    int rc = device_contig(c, contig, &g);
    if (rc) return rc;
    DipView a, b;
    bool counted;
    uint32_t counted_flags;
    if (!compare_dip_view(c, contig, MSIM_CMP_TRUTH, &a, &counted, &counted_flags) || !compare_dip_view(c, contig, MSIM_CMP_CALLS, &b, &counted, &counted_flags))
        return fail(c, MSIM_ERR_ARG, "contig has no diploid table of both sides (msim_cmp_join)");
    PhaseState *P;
    if ((rc = state_of(c, &P))) return rc;
    PhaseContig &pc = contig_of(P, contig);
    const PhaseSide &sa = pc.side[MSIM_CMP_TRUTH], &sb = pc.side[MSIM_CMP_CALLS];
    if (!sa.have_words || !sb.have_words || sa.n != a.t.n || sb.n != b.t.n) return fail(c, MSIM_ERR_ARG, "contig has no phase words of both sides");
    const size_t na = (size_t)a.t.n, nb = (size_t)b.t.n;
    const CopySource src[10] = {{a.t.recs, na * sizeof(msim_record)}, {b.t.recs, nb * sizeof(msim_record)}, {a.gt, na}, {b.gt, nb}, {a.flag, na},
                                {sa.d_words.p(), na * sizeof(uint32_t)}, {sb.d_words.p(), nb * sizeof(uint32_t)},
                                // written and read again: partner words + dense keys + dense records (4 + 8 + 4 bytes a truth record:
                                // its 16-byte record stands for them), orientation + state bytes (its genotype and flag bytes)
                                {a.t.recs, na * sizeof(msim_record)}, {a.gt, na}, {a.flag, na}};
    return copy_floor(c, P->out.tm, src, 10, ms);
}

// ---- sequential host restatement: no context, no GPU ----------------------------------------------------------------------------
int msim_dbg_cmp_phase(const uint8_t *bases, uint64_t L, const msim_record *truth, uint64_t n_truth, const uint8_t *truth_pool,
                       uint64_t truth_pool_len, const uint8_t *truth_gt, const uint32_t *truth_words, const msim_record *calls, uint64_t n_calls,
                       const uint8_t *calls_pool, uint64_t calls_pool_len, const uint8_t *calls_gt, const uint32_t *calls_words, uint32_t flags,
                       uint64_t out[MSIM_CMP_PHASE_COUNTS], uint8_t *truth_state) {
    if ((!bases && L) || ((!truth || !truth_gt || !truth_words) && n_truth) || ((!calls || !calls_gt || !calls_words) && n_calls) ||
        (!truth_pool && truth_pool_len) || (!calls_pool && calls_pool_len) || !out || (flags & ~(uint32_t)MSIM_CMP_EXACT))
        return MSIM_ERR_ARG;
    const struct { const char *name; const msim_record *t; const uint8_t *gt; uint64_t n; } sides[2] = {{"truth", truth, truth_gt, n_truth},
                                                                                                          {"calls", calls, calls_gt, n_calls}};
    for (const auto &s : sides)
        for (uint64_t i = 0; i < s.n; i++) {
            const std::string where = std::string(s.name) + " record " + std::to_string(i);
            if (!cmp::known_type(s.t[i].type)) return fail(nullptr, MSIM_ERR_ARG, where + ": unknown type");
            if (i && s.t[i].pos < s.t[i - 1].pos) return fail(nullptr, MSIM_ERR_ARG, where + ": the table is not sorted by pos");
            if (s.gt[i] < 1 || s.gt[i] > 3) return fail(nullptr, MSIM_ERR_ARG, where + ": genotype byte outside 1..3");
        }
    const cmp::Table A{truth, n_truth, truth_pool, truth_pool_len}, B{calls, n_calls, calls_pool, calls_pool_len};
    const bool exact = (flags & MSIM_CMP_EXACT) != 0;
    memset(out, 0, MSIM_CMP_PHASE_COUNTS * sizeof(uint64_t));
    for (uint64_t i = 0; i < n_truth; i++) out[phase::C_TRUTH_HETS] += phase::phased_het(truth_gt[i], truth_words[i]);
    for (uint64_t j = 0; j < n_calls; j++) out[phase::C_CALLS_HETS] += phase::phased_het(calls_gt[j], calls_words[j]);
    // the pairs in table order: the block so far (its size, its pairs with o = 1), the switch run so far
    bool any = false;
    uint32_t key_a = 0, key_b = 0, last_o = 0;
    uint64_t size = 0, ones = 0, run = 0;
    const auto end_run = [&] { out[phase::C_SWITCHES] += phase::run_switches(run); out[phase::C_FLIPS] += phase::run_flips(run); run = 0; };
    const auto end_block = [&] {
        end_run();
        out[phase::C_BLOCKS]++;
        out[phase::C_SINGLETONS] += size == 1;
        out[phase::C_HAMMING] += std::min(ones, size - ones);
        if (size >= 2) out[phase::C_PAIRS_BLOCKED] += size;
    };
    for (uint64_t i = 0; i < n_truth; i++) {
        cmp::Span s;
        const int64_t j = cmp::partner(bases, L, A, i, B, exact, &s);       // the match's flag byte, as dbg_counts<3> states it
        const uint32_t flag = j >= 0 && (uint64_t)j < n_calls ? cmp::pair_flag(truth_gt[i], calls_gt[(size_t)j]) : 0u;
        uint32_t wb;
        uint8_t st = phase::pair_state(bases, L, A, i, B, exact, flag, truth_gt, calls_gt, truth_words, calls_words, &wb);
        if (st) {
            const uint32_t o = (st & phase::ST_ORIENTATION) ? 1u : 0u;
            const bool starts = !any || key_a != truth_words[i] || key_b != wb;
            if (starts && any) end_block();
            if (starts) { size = ones = 0; key_a = truth_words[i]; key_b = wb; }
            else if (o != last_o) { run++; out[phase::C_RAW]++; st |= phase::ST_SWITCH; }
            else end_run();
            any = true;
            size++;
            ones += o;
            last_o = o;
            out[phase::C_PAIRS]++;
        }
        if (truth_state) truth_state[i] = st;
    }
    if (any) end_block();
    out[phase::C_ASSESSED] = out[phase::C_PAIRS] - out[phase::C_BLOCKS];
    return MSIM_OK;
}

int msim_dbg_vcf_phase_word(const uint8_t *line, uint64_t n, uint32_t nf0, uint32_t sample, uint32_t *word, uint32_t *unreadable) {
    if ((!line && n) || !word) return MSIM_ERR_ARG;
    uint32_t tabs = 0;
    for (uint64_t i = 0; i < n; i++) tabs += line[i] == '\t';
    bool bad = false;
    *word = n ? vcf_cons_phase(line, 0, n, tabs, nf0, sample, &bad) : 0u;
    if (unreadable) *unreadable = bad;
    return MSIM_OK;
}

}  // extern "C"
