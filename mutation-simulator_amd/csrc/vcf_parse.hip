// VCF replay: VCF text -> the record table and insert pool of a contig, validated against its resident bases (msim.h:
// msim_vcf_*).  The inverse of render.cpp / text_gpu.hip; APPLY (apply.hip) is untouched -- a parsed contig is left as
// install_host_table leaves one, and what is refused here is exactly what check_record_table refuses plus what the text
// itself can get wrong.
//
// Device path (gfx950):
//   load    k_tile_reduce / k_tile_scan / k_tile_apply over LineStartF: newlines and tabs counted in 16-byte pieces,
//           scanned, every line's start (64-bit) and the tabs in front of it scattered; k_first_data (the header lines),
//           k_group_flags + the same scan (runs of equal CHROM)
//   plan    k_vcf_lines: one lane per line, short fields only (vcf_parse.h) -> record, insert length
//           scan of the insert lengths -> pool offsets;  k_vcf_neigh: ordering / overlap between neighbours
//           k_vcf_long: one lane per 16-byte piece of the group's text -- REF against the genome, an INV / DUP ALT against
//           what the type produces, insert bytes into the pool -- so that no lane's work grows with a line's length
//   The first failure travels as (line << 4 | reason) through atomicMin on one word, read back with the sizes.
// Consensus grammar (msim_vcf_select(ctx, 1, ..): any VCF, one sample's one haplotype; the load is the same), per contig:
//   k_cons_ends   one lane per line: POS, the start of REF from the front, the end of ALT from the back over the sample columns, the
//                 selected genotype entry (vcf_cons_ends)
//   k_cons_sep    one lane per 16-byte piece of the group's text: the one tab inside a line's REF / ALT span
//   k_cons_lines  one lane per line: the selected ALT, the anchor, 0 / 1 / 2 records and the insert length (vcf_cons_line)
//   scan          record counts and insert lengths (two packed channels); its emit writes the compacted records (ConsEmitF)
//   k_cons_neigh  ordering / overlap between neighbours of the compacted table
//   k_cons_long   one lane per 16-byte piece: REF against the genome in either form, the selected ALT's bytes upper-cased into
//                 the pool
//   No lane walks more than VCF_CONS_WALK bytes of a REF or ALT.
// Host path (msim_create(-1)): the same grammar (vcf_parse_line is shared), the long parts as plain loops, and
// check_record_table at the end.
#include <algorithm>
#include <cstring>
#include <string>

#include "cmp_phase.h"
#include "ctx.h"
#include "plan_gpu.h"
#include "vcf_parse.h"

namespace msim {

constexpr uint64_t VCF_MAX_GROUPS = (uint64_t)MAX_CONTIGS + 1;   // more runs of CHROM than contigs can exist: the host refuses within these

struct VcfState {
    uint64_t n = 0, n_lines = 0, n_header = 0, n_tabs = 0;
    std::vector<msim_vcf_group> groups;
    std::vector<uint64_t> group_end;       // text offset of the line behind every group's last one
    uint64_t n_groups = 0;                 // runs found (groups holds at most VCF_MAX_GROUPS of them)
    // host-only context
    std::vector<uint8_t> h_text;
    std::vector<uint64_t> h_ls;            // n_lines + 1 line starts (the last: one past the text's terminator)
    std::vector<uint32_t> h_tabcum;
    // device
    Scratch<uint8_t> d_text;               // allocation; the text starts at d_text + PAD
    Scratch<uint64_t> d_ls;
    Scratch<uint32_t> d_tabcum;
    Scratch<uint32_t> d_a, d_b, d_c;       // one word per line each: flags / name lengths, then meta / insert lengths / pool offsets
    Scratch<uint64_t> d_tile;              // 3 x n_tiles: packed sums, the two channels' offsets (dev_reserve)
    Scratch<unsigned long long> d_mb;      // 8 words: results of a pass
    Pinned<unsigned long long> h_mb;       //   ... and their pinned copy
    EventPair tm;
    double load_ms = 0, plan_ms = 0;
    // msim_vcf_select
    uint32_t grammar = 0, sample = 0, hap = 1;
    uint32_t nf0 = 0;                      // fields of the first data line
    Scratch<VcfCons> d_cons;               // consensus grammar: one per line
    Scratch<uint32_t> d_recline;           // the line (index within its group) of every compacted record
    // the last msim_vcf_plan_contig, where it was a consensus-grammar plan on the device (msim_cmp_phase_mark reads d_recline)
    int last_contig = -1;                  // -1: none
    uint64_t last_first = 0, last_lines = 0, last_recs = 0;    // the group's first line and line count, the records it gave
    uint64_t last_gen = 0;                 // the contig's table_gen behind that plan: a table installed since is not the parser's
};

namespace {

constexpr int ST = 256, SR = 8;            // scan tile: 256 lanes x 8 rounds
constexpr uint64_t TILE = (uint64_t)ST * SR;

__device__ inline uint64_t block_excl_scan(uint64_t v, uint64_t *lds, uint64_t &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long u = __shfl_up(inc, d);
        if (lane >= d) inc += u;
    }
    __syncthreads();                       // (the previous round's sums have been read)
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    uint64_t base = 0, tot = 0;
    for (int i = 0; i < ST / 64; i++) { const uint64_t s = lds[i]; if (i < w) base += s; tot += s; }
    total = tot;
    return base + inc - v;
}

// F::count(i) -> a packed pair of counts (low / high 32 bits; a tile's sums stay below 2^32 each);
// F::emit(i, low before, high before): exclusive prefixes over all items
template <class F>
__global__ __launch_bounds__(ST) void k_tile_reduce(F f, uint64_t n_items, uint64_t *tile_sum) {
    __shared__ uint64_t lds[ST / 64];
    const uint64_t base = (uint64_t)blockIdx.x * TILE;
    uint64_t v = 0;
    for (int r = 0; r < SR; r++) {
        const uint64_t i = base + (uint64_t)r * ST + threadIdx.x;
        if (i < n_items) v += f.count(i);
    }
    uint64_t total;
    (void)block_excl_scan(v, lds, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// one block: exclusive scan of both channels of the tile sums; totals[0..1]
__global__ __launch_bounds__(ST) void k_tile_scan(const uint64_t *tile_sum, uint64_t n_tiles, uint64_t *off_lo, uint64_t *off_hi,
                                                  unsigned long long *totals) {
    __shared__ uint64_t lds[ST / 64];
    uint64_t carry_lo = 0, carry_hi = 0;
    for (uint64_t base = 0; base < n_tiles; base += ST) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t v = i < n_tiles ? tile_sum[i] : 0;
        uint64_t tot_lo, tot_hi;
        const uint64_t ex_lo = block_excl_scan(v & 0xffffffffull, lds, tot_lo);
        const uint64_t ex_hi = block_excl_scan(v >> 32, lds, tot_hi);
        if (i < n_tiles) { off_lo[i] = carry_lo + ex_lo; off_hi[i] = carry_hi + ex_hi; }
        carry_lo += tot_lo; carry_hi += tot_hi;
    }
    if (threadIdx.x == 0) { totals[0] = carry_lo; totals[1] = carry_hi; }
}

template <class F>
__global__ __launch_bounds__(ST) void k_tile_apply(F f, uint64_t n_items, const uint64_t *off_lo, const uint64_t *off_hi) {
    __shared__ uint64_t lds[ST / 64];
    const uint64_t base = (uint64_t)blockIdx.x * TILE;
    uint64_t carry_lo = off_lo[blockIdx.x], carry_hi = off_hi[blockIdx.x];
    for (int r = 0; r < SR; r++) {
        const uint64_t i = base + (uint64_t)r * ST + threadIdx.x;
        const uint64_t v = i < n_items ? f.count(i) : 0;
        uint64_t tot;
        const uint64_t ex = block_excl_scan(v, lds, tot);
        if (i < n_items) f.emit(i, carry_lo + (ex & 0xffffffffull), carry_hi + (ex >> 32));
        carry_lo += tot & 0xffffffffull; carry_hi += tot >> 32;
    }
}

// 16-byte pieces of the text: newlines (low) and tabs (high); every newline leaves the start of the line behind it and the
// tabs in front of that start
struct LineStartF {
    const uint8_t *text; uint64_t n; uint64_t *ls; uint32_t *tabcum;
    __device__ uint64_t count(uint64_t i) const {
        const uint4 w = *reinterpret_cast<const uint4 *>(text + 16 * i);      // (the allocation's slack covers a partial last piece)
        const uint32_t q[4] = {w.x, w.y, w.z, w.w};
        const uint64_t left = n - 16 * i;
        uint32_t nl = 0, tb = 0;
        for (int j = 0; j < 16; j++) {
            const uint32_t ch = (q[j >> 2] >> (8 * (j & 3))) & 0xff;
            const bool in = (uint64_t)j < left;
            nl += in && ch == '\n';
            tb += in && ch == '\t';
        }
        return (uint64_t)nl | ((uint64_t)tb << 32);
    }
    __device__ void emit(uint64_t i, uint64_t nl, uint64_t tb) const {
        const uint4 w = *reinterpret_cast<const uint4 *>(text + 16 * i);
        const uint32_t q[4] = {w.x, w.y, w.z, w.w};
        const uint64_t left = n - 16 * i;
        for (int j = 0; j < 16 && (uint64_t)j < left; j++) {
            const uint32_t ch = (q[j >> 2] >> (8 * (j & 3))) & 0xff;
            if (ch == '\t') tb++;
            if (ch == '\n') { nl++; ls[nl] = 16 * i + j + 1; tabcum[nl] = (uint32_t)tb; }
        }
    }
};

// word array -> its exclusive prefix (low 32 bits; the caller checks the total)
struct ArrayScanF {
    const uint32_t *in; uint32_t *out;
    __device__ uint64_t count(uint64_t i) const { return in[i]; }
    __device__ void emit(uint64_t i, uint64_t lo, uint64_t) const { out[i] = (uint32_t)lo; }
};

// group starts: flag per data line -> (first line, name length, text offset) of every run of equal CHROM
struct GroupF {
    const uint32_t *flag, *name_len; const uint64_t *ls; uint64_t n_header, cap;
    uint64_t *g_first, *g_off; uint32_t *g_len;
    __device__ uint64_t count(uint64_t i) const { return flag[i]; }
    __device__ void emit(uint64_t i, uint64_t lo, uint64_t) const {
        if (flag[i] && lo < cap) { g_first[lo] = n_header + i; g_off[lo] = ls[n_header + i]; g_len[lo] = name_len[i]; }
    }
};

// the first line that is no header line ('#...'); n_lines when there is none
__global__ void k_first_data(const uint8_t *t, const uint64_t *ls, uint64_t n_lines, unsigned long long *mb) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lines) return;
    auto hash = [&](uint64_t k) { return ls[k + 1] - 1 > ls[k] && t[ls[k]] == '#'; };
    if (!hash(i) && (i == 0 || hash(i - 1))) atomicMin(&mb[0], (unsigned long long)i);
}

__device__ inline uint32_t chrom_len(const uint8_t *t, uint64_t b, uint64_t e) {
    uint32_t n = 0;
    while (b + n < e && t[b + n] != '\t' && n < VCF_FIELD_CAP + 1) n++;
    return n;
}

__global__ void k_group_flags(const uint8_t *t, const uint64_t *ls, uint64_t n_header, uint64_t n_data, uint32_t *flag, uint32_t *name_len) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_data) return;
    const uint64_t b = ls[n_header + i], e = ls[n_header + i + 1] - 1;
    const uint32_t n = chrom_len(t, b, e);
    bool start = i == 0 || n > VCF_FIELD_CAP;
    if (!start) {
        const uint64_t pb = ls[n_header + i - 1], pe = b - 1;
        start = pe - pb < n || !(pe - pb == n || t[pb + n] == '\t');
        for (uint32_t k = 0; k < n && !start; k++) start = t[pb + k] != t[b + k];
    }
    flag[i] = start;
    name_len[i] = n;
}

__device__ inline void report(unsigned long long *mb, uint64_t line1, uint32_t reason) {
    atomicMin(&mb[0], (unsigned long long)((line1 << 4) | reason));
}

// mb: [0] first failure, [1] bytes the lines add to the contig, [3] bit 0: some line is no SNP
__global__ __launch_bounds__(256) void k_vcf_lines(const uint8_t *t, const uint64_t *ls, const uint32_t *tabcum, uint64_t first, uint64_t cnt,
                                                   uint32_t name_len, const uint8_t *in, uint64_t L, msim_record *recs, uint32_t *meta,
                                                   uint32_t *ilen, unsigned long long *mb) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long grow = 0;
    bool sv = false;
    if (i < cnt) {
        const uint64_t idx = first + i;
        VcfLine o;
        const uint32_t reason = vcf_parse_line(t, ls[idx], ls[idx + 1] - 1, tabcum[idx + 1] - tabcum[idx], name_len, in, L, o);
        if (reason) { report(mb, idx + 1, reason); o.pos = o.stop = o.type = o.aux = 0; o.meta = 0; o.ins_len = 0; o.grow = 0; }
        *reinterpret_cast<uint4 *>(&recs[i]) = make_uint4(o.pos, o.stop, 0u, o.type | (o.aux << 8));   // msim_record: pos, stop, extra, type / aux / rsv
        meta[i] = o.meta;
        ilen[i] = o.ins_len;
        grow = o.grow;
        sv = !reason && o.type != MSIM_SN;
    }
    for (int d = 32; d; d >>= 1) grow += __shfl_xor(grow, d);
    const bool any_sv = __any(sv);
    if ((threadIdx.x & 63) == 0) {
        if (grow) atomicAdd(&mb[1], grow);
        if (any_sv) atomicOr(&mb[3], 1ull);
    }
}

__global__ void k_vcf_neigh(msim_record *recs, const uint32_t *meta, const uint32_t *poff, uint64_t first, uint64_t cnt, unsigned long long *mb) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt || !(meta[i] & VCF_META_VALID)) return;
    if (recs[i].type == MSIM_IN) recs[i].extra = poff[i];
    if (i && (meta[i - 1] & VCF_META_VALID)) {
        msim_record p = recs[i - 1];
        if ((uint64_t)recs[i].pos < vcf_next_free(p)) report(mb, first + i + 1, VCF_R_ORDER);
    }
}

// One lane per 16-byte piece of the group's text [ls[first], ls[first + cnt]): every byte of a REF \t ALT span is checked,
// or copied into the insert pool, by the lane whose piece holds it.
__global__ __launch_bounds__(256) void k_vcf_long(const uint8_t *t, const uint64_t *ls, uint64_t first, uint64_t cnt, const msim_record *recs,
                                                  const uint32_t *meta, const uint8_t *in, uint8_t *pool, uint64_t pool_len,
                                                  unsigned long long *mb) {
    if (!(mb[3] & 1)) return;                              // SNPs only: the lanes of k_vcf_lines have seen every byte
    const uint64_t lo = ls[first], hi = ls[first + cnt];
    const uint64_t piece = (lo & ~15ull) + 16 * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    uint64_t x = piece > lo ? piece : lo;
    const uint64_t x1 = piece + 16 < hi ? piece + 16 : hi;
    if (x >= x1) return;
    const uint4 w = *reinterpret_cast<const uint4 *>(t + piece);             // (aligned; the allocation's slack covers both ends)
    const uint64_t w_lo = w.x | ((uint64_t)w.y << 32), w_hi = w.z | ((uint64_t)w.w << 32);
    uint64_t a = 0, b = cnt - 1;                           // the line that holds byte x
    while (a < b) {
        const uint64_t m = (a + b + 1) >> 1;
        if (ls[first + m] <= x) a = m; else b = m - 1;
    }
    uint32_t worst = 0xffffffffu;
    uint64_t worst_line = 0;
    while (x < x1) {
        const uint64_t lb = ls[first + a], next = ls[first + a + 1];
        if (x >= next) { a++; continue; }
        const uint64_t lend = next < x1 ? next : x1;
        const uint32_t m = meta[a];
        if (!(m & VCF_META_VALID)) { x = lend; continue; }
        const msim_record r = recs[a];
        const uint64_t r0 = lb + vcf_meta_r0(m), a1 = next - 1 - vcf_meta_tail(m);
        if (r.type == MSIM_SN || x >= a1) { x = lend; continue; }
        if (x < r0) x = r0;
        const uint64_t stop = a1 < lend ? a1 : lend;
        for (; x < stop; x++) {
            int64_t at;
            const uint32_t j = (uint32_t)(x - piece);
            const uint8_t ch = (uint8_t)((j < 8 ? w_lo : w_hi) >> (8 * (j & 7)));
            const uint32_t reason = vcf_long_byte(r, m & VCF_META_LEAD, a1 - r0, x - r0, ch, in, &at);
            if (reason) {
                if (worst == 0xffffffffu || first + a + 1 < worst_line || (first + a + 1 == worst_line && reason < worst)) {
                    worst = reason; worst_line = first + a + 1;
                }
            } else if (at >= 0 && (uint64_t)r.extra + (uint64_t)at < pool_len) {
                pool[(uint64_t)r.extra + (uint64_t)at] = ch;
            }
        }
        if (x < lend && x >= a1) x = lend;
    }
    if (worst != 0xffffffffu) report(mb, worst_line, worst);
}

// ---- consensus grammar ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cons_ends(const uint8_t *t, const uint64_t *ls, const uint32_t *tabcum, uint64_t first, uint64_t cnt,
                                                   uint32_t name_len, uint32_t nf0, uint32_t sample, uint32_t hap, uint64_t L, VcfCons *cons,
                                                   unsigned long long *mb) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    const uint64_t idx = first + i;
    VcfCons o;
    const uint32_t reason = vcf_cons_ends(t, ls[idx], ls[idx + 1] - 1, tabcum[idx + 1] - tabcum[idx], name_len, nf0, sample, hap, L, o);
    if (reason) { report(mb, idx + 1, reason); o.k = 0; }
    cons[i] = o;
}

// the line that holds text byte x: the largest a in [0, cnt) with ls[first + a] <= x
__device__ inline uint64_t line_of(const uint64_t *ls, uint64_t first, uint64_t cnt, uint64_t x) {
    uint64_t a = 0, b = cnt - 1;
    while (a < b) {
        const uint64_t m = (a + b + 1) >> 1;
        if (ls[first + m] <= x) a = m; else b = m - 1;
    }
    return a;
}

__global__ __launch_bounds__(256) void k_cons_sep(const uint8_t *t, const uint64_t *ls, uint64_t first, uint64_t cnt, VcfCons *cons) {
    const uint64_t lo = ls[first], hi = ls[first + cnt];
    const uint64_t piece = (lo & ~15ull) + 16 * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    uint64_t x = piece > lo ? piece : lo;
    const uint64_t x1 = piece + 16 < hi ? piece + 16 : hi;
    if (x >= x1) return;
    const uint4 w = *reinterpret_cast<const uint4 *>(t + piece);             // (aligned; the allocation's slack covers both ends)
    const uint64_t w_lo = w.x | ((uint64_t)w.y << 32), w_hi = w.z | ((uint64_t)w.w << 32);
    uint64_t a = line_of(ls, first, cnt, x);
    while (x < x1) {
        const uint64_t next = ls[first + a + 1];
        if (x >= next) { a++; continue; }
        const uint64_t lend = next < x1 ? next : x1;
        if (cons[a].k == 0) { x = lend; continue; }
        const uint64_t r0 = cons[a].r0, a1 = cons[a].a1;
        if (x < r0) x = r0;
        const uint64_t stop = a1 < lend ? a1 : lend;
        for (; x < stop; x++) {
            const uint32_t j = (uint32_t)(x - piece);
            if ((uint8_t)((j < 8 ? w_lo : w_hi) >> (8 * (j & 7))) == '\t') cons[a].sep = x;
        }
        x = lend;
    }
}

// mb: [0] first failure, [1] bytes the lines add to the contig, [3] bit 0: some record is no SNP
__global__ __launch_bounds__(256) void k_cons_lines(const uint8_t *t, uint64_t first, uint64_t cnt, const uint8_t *in, uint64_t L, VcfCons *cons,
                                                    unsigned long long *mb) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long grow = 0;
    bool sv = false;
    if (i < cnt) {
        VcfCons o = cons[i];
        const uint32_t reason = vcf_cons_line(t, in, L, o);
        if (reason) report(mb, first + i + 1, reason);
        cons[i] = o;
        grow = o.ilen;
        sv = o.nrec && !o.snp;
    }
    for (int d = 32; d; d >>= 1) grow += __shfl_xor(grow, d);
    const bool any_sv = __any(sv);
    if ((threadIdx.x & 63) == 0) {
        if (grow) atomicAdd(&mb[1], grow);
        if (any_sv) atomicOr(&mb[3], 1ull);
    }
}

// records (low) and insert bytes (high) of every line -> its slot in the compacted table and its place in the pool
struct ConsEmitF {
    VcfCons *cons; msim_record *recs; uint32_t *recline;
    __device__ uint64_t count(uint64_t i) const { return (uint64_t)cons[i].nrec | ((uint64_t)cons[i].ilen << 32); }
    __device__ void emit(uint64_t i, uint64_t slot, uint64_t poff) const {
        const VcfCons o = cons[i];
        if (o.nrec == 0) return;
        cons[i].poff = (uint32_t)poff;
        msim_record r[2];
        vcf_cons_records(o, (uint32_t)poff, r);
        for (uint32_t q = 0; q < o.nrec; q++) { recs[slot + q] = r[q]; recline[slot + q] = (uint32_t)i; }
    }
};

__global__ void k_cons_neigh(const msim_record *recs, const uint32_t *recline, const unsigned long long *n_rec, uint64_t first, unsigned long long *mb) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0 || j >= *n_rec) return;
    if ((uint64_t)recs[j].pos < vcf_next_free(recs[j - 1])) report(mb, first + recline[j] + 1, VCF_R_ORDER);
}

__global__ __launch_bounds__(256) void k_cons_long(const uint8_t *t, const uint64_t *ls, uint64_t first, uint64_t cnt, const VcfCons *cons,
                                                   const uint8_t *in, uint8_t *pool, uint64_t pool_len, unsigned long long *mb) {
    const uint64_t lo = ls[first], hi = ls[first + cnt];
    const uint64_t piece = (lo & ~15ull) + 16 * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    uint64_t x = piece > lo ? piece : lo;
    const uint64_t x1 = piece + 16 < hi ? piece + 16 : hi;
    if (x >= x1) return;
    const uint4 w = *reinterpret_cast<const uint4 *>(t + piece);
    const uint64_t w_lo = w.x | ((uint64_t)w.y << 32), w_hi = w.z | ((uint64_t)w.w << 32);
    uint64_t a = line_of(ls, first, cnt, x);
    uint32_t worst = 0xffffffffu;
    uint64_t worst_line = 0;
    while (x < x1) {
        const uint64_t next = ls[first + a + 1];
        if (x >= next) { a++; continue; }
        const uint64_t lend = next < x1 ? next : x1;
        const uint32_t flags = cons[a].flags;
        if (!flags) { x = lend; continue; }
        const VcfCons o = cons[a];
        const uint64_t ref1 = (flags & VCF_C_REF) ? o.r0 + o.R : o.r0, alt1 = o.s0 + o.A;
        if (x >= alt1) { x = lend; continue; }
        if (x < o.r0) x = o.r0;
        const uint64_t stop = alt1 < lend ? alt1 : lend;
        for (; x < stop; x++) {
            const uint32_t j = (uint32_t)(x - piece);
            const uint8_t ch = (uint8_t)((j < 8 ? w_lo : w_hi) >> (8 * (j & 7)));
            uint32_t reason = VCF_OK;
            if (x < ref1) reason = vcf_cons_ref_byte(o, x - o.r0, ch, in);
            else if (x >= o.s0) {
                int64_t at;
                uint8_t up;
                reason = vcf_cons_alt_byte(o, x - o.s0, ch, &at, &up);
                if (!reason && at >= 0 && (uint64_t)o.poff + (uint64_t)at < pool_len) pool[(uint64_t)o.poff + (uint64_t)at] = up;
            }
            if (reason && (worst == 0xffffffffu || first + a + 1 < worst_line || (first + a + 1 == worst_line && reason < worst))) {
                worst = reason; worst_line = first + a + 1;
            }
        }
        x = lend;
    }
    if (worst != 0xffffffffu) report(mb, worst_line, worst);
}

inline unsigned blocks_for(uint64_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

int vcf_fail(Ctx *c, uint64_t line1, uint32_t reason) {
    const bool cons = c->vcf && c->vcf->grammar;
    return fail(c, MSIM_ERR_VALUE, "VCF line " + std::to_string(line1) + ": " + (cons ? vcf_cons_reason_text(reason) : vcf_reason_text(reason)));
}

// wait for the context's stream; a wait that gave up is followed by an unbounded one when caller memory is part of a copy
int wait_ctx(Ctx *c, bool caller_memory) {
    const hipError_t e = wait_stream(c->stream);
    if (e != hipSuccess && caller_memory) (void)hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "wait_stream(vcf)");
    return MSIM_OK;
}

int fetch_mailbox(Ctx *c, VcfState *S) {
    MSIM_HIP(c, hipMemcpyAsync(S->h_mb.p(), S->d_mb.p(), 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    return wait_ctx(c, false);
}

template <class F>
int run_scan(Ctx *c, VcfState *S, F f, uint64_t n_items, unsigned long long *d_totals) {
    const uint64_t n_tiles = std::max<uint64_t>(1, (n_items + TILE - 1) / TILE);
    int rc = dev_reserve(c, S->d_tile, (size_t)n_tiles * 3 * sizeof(uint64_t));
    if (rc) return rc;
    uint64_t *sum = S->d_tile.p(), *off_lo = sum + n_tiles, *off_hi = off_lo + n_tiles;
    hipLaunchKernelGGL(k_tile_reduce<F>, dim3((unsigned)n_tiles), dim3(ST), 0, c->stream, f, n_items, sum);
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(ST), 0, c->stream, sum, n_tiles, off_lo, off_hi, d_totals);
    hipLaunchKernelGGL(k_tile_apply<F>, dim3((unsigned)n_tiles), dim3(ST), 0, c->stream, f, n_items, off_lo, off_hi);
    MSIM_HIP(c, hipGetLastError());
    return MSIM_OK;
}

// end of a timed stretch of the load (begun by tm.begin): results back, kernel time added
int phase_end(Ctx *c, VcfState *S) {
    MSIM_HIP(c, S->tm.end(c->stream));
    const int rc = fetch_mailbox(c, S);
    return rc ? rc : S->tm.add_elapsed(c, &S->load_ms);
}

// ---- host parser ---------------------------------------------------------------------------------------------------------
uint32_t host_name_len(const uint8_t *t, uint64_t b, uint64_t e) {
    uint32_t n = 0;
    while (b + n < e && t[b + n] != '\t' && n < VCF_FIELD_CAP + 1) n++;
    return n;
}

void load_host(VcfState *S, const uint8_t *text, uint64_t n) {
    S->h_text.assign(text, text + n);
    S->h_ls.assign(1, 0);
    S->h_tabcum.assign(1, 0);
    uint32_t tabs = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (text[i] == '\t') tabs++;
        if (text[i] == '\n') { S->h_ls.push_back(i + 1); S->h_tabcum.push_back(tabs); }
    }
    if (n && text[n - 1] != '\n') { S->h_ls.push_back(n + 1); S->h_tabcum.push_back(tabs); }
    S->n_lines = S->h_ls.size() - 1;
    const uint8_t *t = S->h_text.data();
    uint64_t h = 0;
    while (h < S->n_lines && S->h_ls[h + 1] - 1 > S->h_ls[h] && t[S->h_ls[h]] == '#') h++;
    S->n_header = h;
    for (uint64_t i = h; i < S->n_lines; i++) {
        const uint64_t b = S->h_ls[i], e = S->h_ls[i + 1] - 1;
        const uint32_t len = host_name_len(t, b, e);
        bool start = i == h || len > VCF_FIELD_CAP;
        if (!start) {
            const uint64_t pb = S->h_ls[i - 1], pe = b - 1;
            const uint32_t plen = host_name_len(t, pb, pe);
            start = plen != len || memcmp(t + pb, t + b, len) != 0;
        }
        if (start) {
            S->n_groups++;
            if (S->groups.size() < VCF_MAX_GROUPS) S->groups.push_back(msim_vcf_group{b, i, 0, len, 0});
        }
        if (S->n_groups == S->groups.size()) S->groups.back().n_lines++;
    }
}

int plan_host(Ctx *c, VcfState *S, Contig *g, const msim_vcf_group *grp) {
    contig_reset(*g);                                      // as the device parser: a refusal leaves the contig unplanned
    c->text_kind = 0;
    g->apply_stream = nullptr;
    std::vector<msim_record> recs;
    std::vector<uint8_t> pool;
    const uint8_t *t = S->h_text.data(), *in = g->h_in.data();
    const uint64_t L = g->len;
    uint64_t grow = 0;
    const uint64_t cnt = grp ? grp->n_lines : 0;
    recs.reserve((size_t)cnt);
    for (uint64_t i = 0; i < cnt; i++) {
        const uint64_t idx = grp->first_line + i, b = S->h_ls[idx], e = S->h_ls[idx + 1] - 1;
        VcfLine o;
        uint32_t reason = vcf_parse_line(t, b, e, S->h_tabcum[idx + 1] - S->h_tabcum[idx], grp->name_len, in, L, o);
        if (reason) return vcf_fail(c, idx + 1, reason);
        uint32_t worst = 0xffffffffu;
        auto note = [&](uint32_t r) { if (r < worst) worst = r; };
        auto mismatch = [&](uint8_t ch, bool in_ref) { note(vcf_allele_char(ch) ? VCF_R_ALLELE : in_ref ? VCF_R_REF : VCF_R_ALT); };
        msim_record rec = vcf_record(o, 0);
        if (!recs.empty() && (uint64_t)rec.pos < vcf_next_free(recs.back())) note(VCF_R_ORDER);
        const uint64_t r0 = b + vcf_meta_r0(o.meta), a1 = e - vcf_meta_tail(o.meta), M = a1 - r0;
        const msim_record &r = rec;
        switch (r.type) {
            case MSIM_IN: {                                // ALT = anchor + insert (leading) | insert + anchor
                const uint8_t *ins = t + r0 + 2 + ((o.meta & VCF_META_LEAD) ? 1 : 0);
                rec.extra = (uint32_t)pool.size();
                for (uint64_t q = 0; q < o.ins_len; q++)
                    if (!vcf_letter(ins[q])) note(vcf_allele_char(ins[q]) ? VCF_R_ALLELE : VCF_R_INSERT);
                pool.insert(pool.end(), ins, ins + o.ins_len);
                break;
            }
            case MSIM_DE: {                                // REF = the genome from the anchor (leading) / the first deleted base on
                const uint64_t R = M - 2, g0 = (o.meta & VCF_META_LEAD) ? (uint64_t)r.pos - 1 : r.pos;
                for (uint64_t q = 0; q < R; q++) if (t[r0 + q] != vcf_conv(in[g0 + q])) mismatch(t[r0 + q], true);
                break;
            }
            case MSIM_IV: {
                const uint64_t R = (M - 1) / 2;
                for (uint64_t q = 0; q < R; q++) {
                    if (t[r0 + q] != vcf_conv(in[r.pos + q])) mismatch(t[r0 + q], true);
                    if (t[r0 + R + 1 + q] != vcf_comp(vcf_conv(in[r.stop - q]))) mismatch(t[r0 + R + 1 + q], false);
                }
                break;
            }
            case MSIM_DU: {
                const uint64_t R = (M - 1) / 3;
                for (uint64_t q = 0; q < R; q++) {
                    if (t[r0 + q] != in[r.pos + q]) mismatch(t[r0 + q], true);
                    if (t[r0 + R + 1 + q] != in[r.pos + q]) mismatch(t[r0 + R + 1 + q], false);
                    if (t[r0 + 2 * R + 1 + q] != in[r.pos + q]) mismatch(t[r0 + 2 * R + 1 + q], false);
                }
                break;
            }
            default: break;
        }
        if (worst != 0xffffffffu) return vcf_fail(c, idx + 1, worst);
        grow += o.grow;
        recs.push_back(rec);
    }
    // (the device decides with these sums alone; no intermediate offset can leave [0, 2^32) below this bound either)
    if (grp && L + grow >= (1ull << 32)) return vcf_fail(c, grp->first_line + 1, VCF_R_LENGTH);
    long long delta = 0;
    uint64_t bad = 0;
    const char *what = "";
    if (table_check(c, L, recs.data(), recs.size(), pool.size(), &delta, &bad, &what))
        return fail(c, MSIM_ERR_VALUE, "VCF line " + std::to_string((grp ? grp->first_line : 0) + bad + 1) + ": " + what);
    return table_install(c, g, recs, pool, recs.empty());
}

// the consensus grammar, line after line (vcf_parse.h: the three statements the kernels share)
int plan_host_cons(Ctx *c, VcfState *S, Contig *g, const msim_vcf_group *grp) {
    contig_reset(*g);
    c->text_kind = 0;
    g->apply_stream = nullptr;
    std::vector<msim_record> recs;
    std::vector<uint64_t> recline;
    std::vector<uint8_t> pool, ins;
    const uint8_t *t = S->h_text.data(), *in = g->h_in.data();
    const uint64_t L = g->len;
    uint64_t grow = 0;
    const uint64_t cnt = grp ? grp->n_lines : 0;
    for (uint64_t i = 0; i < cnt; i++) {
        const uint64_t idx = grp->first_line + i, b = S->h_ls[idx], e = S->h_ls[idx + 1] - 1;
        VcfCons o;
        uint32_t worst = vcf_cons_ends(t, b, e, S->h_tabcum[idx + 1] - S->h_tabcum[idx], grp->name_len, S->nf0, S->sample, S->hap, L, o);
        if (worst) return vcf_fail(c, idx + 1, worst);
        if (o.k == 0) continue;
        o.sep = o.r0;
        while (o.sep < o.a1 && t[o.sep] != '\t') o.sep++;
        worst = vcf_cons_line(t, in, L, o);
        const bool shaped = worst == VCF_OK;
        if (!worst) worst = 0xffffffffu;
        auto note = [&](uint32_t r) { if (r && r < worst) worst = r; };
        ins.assign(o.ilen, 0);
        if (o.flags & VCF_C_REF) for (uint64_t j = 0; j < o.R; j++) note(vcf_cons_ref_byte(o, j, t[o.r0 + j], in));
        if (o.flags & VCF_C_ALT)
            for (uint64_t j = 0; j < o.A; j++) {
                int64_t at;
                uint8_t up;
                note(vcf_cons_alt_byte(o, j, t[o.s0 + j], &at, &up));
                if (at >= 0) ins[(size_t)at] = up;
            }
        msim_record r[2];
        if (shaped) {
            vcf_cons_records(o, (uint32_t)pool.size(), r);
            if (o.nrec && !recs.empty() && (uint64_t)r[0].pos < vcf_next_free(recs.back())) note(VCF_R_ORDER);
        }
        if (worst != 0xffffffffu) return vcf_fail(c, idx + 1, worst);
        for (uint32_t q = 0; q < o.nrec; q++) { recs.push_back(r[q]); recline.push_back(idx); }
        pool.insert(pool.end(), ins.begin(), ins.end());
        grow += o.ilen;
    }
    if (grp && L + grow >= (1ull << 32)) return vcf_fail(c, grp->first_line + 1, VCF_R_LENGTH);
    long long delta = 0;
    uint64_t bad = 0;
    const char *what = "";
    if (table_check(c, L, recs.data(), recs.size(), pool.size(), &delta, &bad, &what))
        return fail(c, MSIM_ERR_VALUE, "VCF line " + std::to_string((bad < recline.size() ? recline[(size_t)bad] : (grp ? grp->first_line : 0)) + 1) + ": " + what);
    return table_install(c, g, recs, pool, recs.empty());
}

// ---- device parser ---------------------------------------------------------------------------------------------------------
int load_device(Ctx *c, VcfState *S, const uint8_t *text, uint64_t n) {
    MSIM_HIP(c, pin_alloc(S->h_mb, 8 * sizeof(unsigned long long)));
    MSIM_HIP(c, dev_alloc(S->d_mb, 8 * sizeof(unsigned long long)));
    MSIM_HIP(c, S->tm.create());
    MSIM_HIP(c, dev_alloc(S->d_text, n + 2 * PAD));
    MSIM_HIP(c, hipMemsetAsync(S->d_text.p(), 0, PAD, c->stream));
    MSIM_HIP(c, hipMemsetAsync(S->d_text.p() + PAD + n, 0, PAD, c->stream));
    if (n) MSIM_HIP(c, hipMemcpyAsync(S->d_text.p() + PAD, text, n, hipMemcpyHostToDevice, c->stream));
    int rc = wait_ctx(c, true);                            // (the caller's text is free again)
    if (rc) return rc;
    const uint8_t *t = S->d_text.p() + PAD;
    // pass 1: how many lines
    const uint64_t n_pieces = (n + 15) / 16;
    LineStartF lf{t, n, nullptr, nullptr};
    const uint64_t n_tiles = std::max<uint64_t>(1, (n_pieces + TILE - 1) / TILE);
    rc = dev_reserve(c, S->d_tile, (size_t)n_tiles * 3 * sizeof(uint64_t));
    if (rc) return rc;
    uint64_t *sum = S->d_tile.p(), *off_lo = sum + n_tiles, *off_hi = off_lo + n_tiles;
    MSIM_HIP(c, hipMemsetAsync(S->d_mb.p(), 0, 8 * sizeof(unsigned long long), c->stream));
    MSIM_HIP(c, S->tm.begin(c->stream));
    hipLaunchKernelGGL(k_tile_reduce<LineStartF>, dim3((unsigned)n_tiles), dim3(ST), 0, c->stream, lf, n_pieces, sum);
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(ST), 0, c->stream, sum, n_tiles, off_lo, off_hi, S->d_mb.p() + 4);
    MSIM_HIP(c, hipGetLastError());
    if ((rc = phase_end(c, S))) return rc;
    const uint64_t newlines = S->h_mb.p()[4];
    S->n_tabs = S->h_mb.p()[5];
    const bool open_end = n && text[n - 1] != '\n';
    S->n_lines = newlines + (open_end ? 1 : 0);
    if (S->n_lines >= (1ull << 31)) return fail(c, MSIM_ERR_UNSUPPORTED, "VCF of 2^31 lines or more");
    // pass 2: where they start
    MSIM_HIP(c, dev_alloc(S->d_ls, (S->n_lines + 2) * sizeof(uint64_t)));
    MSIM_HIP(c, dev_alloc(S->d_tabcum, (S->n_lines + 2) * sizeof(uint32_t)));
    MSIM_HIP(c, dev_alloc(S->d_a, (S->n_lines + 1) * sizeof(uint32_t)));
    MSIM_HIP(c, dev_alloc(S->d_b, (S->n_lines + 1) * sizeof(uint32_t)));
    MSIM_HIP(c, dev_alloc(S->d_c, (S->n_lines + 1) * sizeof(uint32_t)));
    MSIM_HIP(c, hipMemsetAsync(S->d_ls.p(), 0, sizeof(uint64_t), c->stream));
    MSIM_HIP(c, hipMemsetAsync(S->d_tabcum.p(), 0, sizeof(uint32_t), c->stream));
    lf.ls = S->d_ls.p(); lf.tabcum = S->d_tabcum.p();
    MSIM_HIP(c, S->tm.begin(c->stream));
    hipLaunchKernelGGL(k_tile_apply<LineStartF>, dim3((unsigned)n_tiles), dim3(ST), 0, c->stream, lf, n_pieces, off_lo, off_hi);
    MSIM_HIP(c, hipGetLastError());
    if (open_end) {                                        // the last line has no terminator: it ends where one would stand
        uint32_t *tabs = reinterpret_cast<uint32_t *>(&S->h_mb.p()[7]);       // (staged in the pinned mailbox: no copy out of this frame)
        S->h_mb.p()[6] = n + 1;
        *tabs = (uint32_t)S->n_tabs;
        MSIM_HIP(c, hipMemcpyAsync(S->d_ls.p() + S->n_lines, &S->h_mb.p()[6], sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        MSIM_HIP(c, hipMemcpyAsync(S->d_tabcum.p() + S->n_lines, tabs, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    }
    // header lines, groups
    S->h_mb.p()[0] = S->n_lines;
    MSIM_HIP(c, hipMemcpyAsync(S->d_mb.p(), S->h_mb.p(), sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
    if (S->n_lines)
        hipLaunchKernelGGL(k_first_data, dim3(blocks_for(S->n_lines, 256)), dim3(256), 0, c->stream, t, S->d_ls.p(), S->n_lines, S->d_mb.p());
    MSIM_HIP(c, hipGetLastError());
    if ((rc = phase_end(c, S))) return rc;
    S->n_header = S->h_mb.p()[0];
    const uint64_t n_data = S->n_lines - S->n_header;
    if (n_data) {
        const uint64_t cap = std::min<uint64_t>(n_data, VCF_MAX_GROUPS);
        Scratch<uint64_t> found;                           // (freed however this block is left)
        MSIM_HIP(c, dev_alloc(found, cap * 20));
        uint64_t *const g_first = found.p(), *const g_off = g_first + cap;
        uint32_t *const g_len = reinterpret_cast<uint32_t *>(g_off + cap);
        MSIM_HIP(c, S->tm.begin(c->stream));
        hipLaunchKernelGGL(k_group_flags, dim3(blocks_for(n_data, 256)), dim3(256), 0, c->stream, t, S->d_ls.p(), S->n_header, n_data, S->d_a.p(), S->d_b.p());
        GroupF gf{S->d_a.p(), S->d_b.p(), S->d_ls.p(), S->n_header, cap, g_first, g_off, g_len};
        rc = run_scan(c, S, gf, n_data, S->d_mb.p() + 4);
        if (!rc) rc = phase_end(c, S);
        std::vector<uint8_t> host;
        if (!rc) {
            S->n_groups = S->h_mb.p()[4];
            const uint64_t k = std::min<uint64_t>(S->n_groups, cap);
            host.resize((size_t)cap * 20);
            const hipError_t e = hipMemcpyAsync(host.data(), g_first, (size_t)cap * 20, hipMemcpyDeviceToHost, c->stream);
            if (e != hipSuccess) rc = hip_fail(c, e, "hipMemcpyAsync(vcf groups)");
            else rc = wait_ctx(c, true);                   // (`host` lives on this frame)
            if (!rc) {
                const uint64_t *hf = reinterpret_cast<const uint64_t *>(host.data()), *ho = hf + cap;
                const uint32_t *hl = reinterpret_cast<const uint32_t *>(ho + cap);
                for (uint64_t q = 0; q < k; q++) {
                    const uint64_t next = q + 1 < k ? hf[q + 1] : S->n_lines;
                    S->groups.push_back(msim_vcf_group{ho[q], hf[q], next - hf[q], hl[q], 0});
                    S->group_end.push_back(q + 1 < k ? ho[q + 1] : n + (open_end ? 1 : 0));
                }
            }
        }
        if (rc) return rc;
    }
    return MSIM_OK;
}

int plan_device(Ctx *c, VcfState *S, Contig *g, const msim_vcf_group *grp) {
    int rc = ctx_drain(c);                                 // this contig's buffers may still be read by its last APPLY
    if (rc) return rc;
    contig_reset(*g);
    c->text_kind = 0;
    g->apply_stream = nullptr;
    const uint64_t cnt = grp ? grp->n_lines : 0;
    uint64_t pool_len = 0;
    bool any_sv = false, too_long = false, check_only = false;
    if (cnt) {
        const uint8_t *t = S->d_text.p() + PAD, *in = g->d_in.p() + PAD;
        const uint64_t first = grp->first_line;
        rc = dev_reserve(c, g->d_recs, (size_t)cnt * sizeof(msim_record));
        if (rc) return rc;
        S->h_mb.p()[0] = ~0ull; S->h_mb.p()[1] = S->h_mb.p()[2] = S->h_mb.p()[3] = 0;
        MSIM_HIP(c, hipMemcpyAsync(S->d_mb.p(), S->h_mb.p(), 4 * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
        MSIM_HIP(c, S->tm.begin(c->stream));
        uint32_t *meta = S->d_a.p(), *ilen = S->d_b.p(), *poff = S->d_c.p();
        hipLaunchKernelGGL(k_vcf_lines, dim3(blocks_for(cnt, 256)), dim3(256), 0, c->stream, t, S->d_ls.p(), S->d_tabcum.p(), first, cnt, grp->name_len, in,
                           g->len, g->d_recs.p(), meta, ilen, S->d_mb.p());
        rc = run_scan(c, S, ArrayScanF{ilen, poff}, cnt, S->d_mb.p() + 4);
        if (rc) return rc;
        hipLaunchKernelGGL(k_vcf_neigh, dim3(blocks_for(cnt, 256)), dim3(256), 0, c->stream, g->d_recs.p(), meta, poff, first, cnt, S->d_mb.p());
        MSIM_HIP(c, hipGetLastError());
        MSIM_HIP(c, S->tm.end(c->stream));
        if ((rc = fetch_mailbox(c, S))) return rc;
        if ((rc = S->tm.add_elapsed(c, &S->plan_ms))) return rc;
        // A refusal found so far does not end the pass: an earlier line may still fail in its long part, and the first
        // offending line is the one to name.  Refused lines add nothing to either sum.  With a refusal pending, or with sums
        // of 2^32 or more (where the 32-bit pool offsets have wrapped), the long pass checks only and writes no pool byte.
        too_long = g->len + S->h_mb.p()[1] >= (1ull << 32);
        check_only = too_long || S->h_mb.p()[0] != ~0ull;
        pool_len = check_only ? 0 : S->h_mb.p()[4];            // (below 2^32 with the bound above: the 32-bit offsets are exact)
        any_sv = S->h_mb.p()[3] & 1;
    }
    rc = dev_reserve(c, g->d_pool, (size_t)pool_len + 2 * PAD);
    if (rc) return rc;
    if (any_sv) {
        const uint64_t first = grp->first_line;
        // the group's text: from its first line's start to the start of the line behind its last one
        const uint64_t bytes = S->group_end[(size_t)(grp - S->groups.data())] - grp->name_off + (grp->name_off & 15);
        MSIM_HIP(c, S->tm.begin(c->stream));
        hipLaunchKernelGGL(k_vcf_long, dim3(blocks_for((bytes + 15) / 16, 256)), dim3(256), 0, c->stream, S->d_text.p() + PAD, S->d_ls.p(), first, cnt,
                           g->d_recs.p(), S->d_a.p(), g->d_in.p() + PAD, g->d_pool.p() + PAD, pool_len, S->d_mb.p());
        MSIM_HIP(c, hipGetLastError());
        MSIM_HIP(c, S->tm.end(c->stream));
        if ((rc = fetch_mailbox(c, S))) return rc;
        if ((rc = S->tm.add_elapsed(c, &S->plan_ms))) return rc;
    }
    if (cnt && S->h_mb.p()[0] != ~0ull) return vcf_fail(c, S->h_mb.p()[0] >> 4, (uint32_t)(S->h_mb.p()[0] & 15));
    if (too_long) return vcf_fail(c, grp->first_line + 1, VCF_R_LENGTH);
    g->n_rec = cnt;
    g->pool_len = pool_len;
    g->plan_empty = cnt == 0;
    g->all_snp = !any_sv;
    g->planned = true;
    return MSIM_OK;
}

int plan_device_cons(Ctx *c, VcfState *S, Contig *g, const msim_vcf_group *grp) {
    int rc = ctx_drain(c);                                 // this contig's buffers may still be read by its last APPLY
    if (rc) return rc;
    contig_reset(*g);
    c->text_kind = 0;
    g->apply_stream = nullptr;
    const uint64_t cnt = grp ? grp->n_lines : 0;
    uint64_t pool_len = 0, n_rec = 0;
    bool any_sv = false, too_long = false;
    if (cnt) {
        const uint8_t *t = S->d_text.p() + PAD, *in = g->d_in.p() + PAD;
        const uint64_t first = grp->first_line;
        rc = dev_reserve(c, g->d_recs, (size_t)cnt * 2 * sizeof(msim_record));
        if (rc) return rc;
        // the group's text: from its first line's start to the start of the line behind its last one, in 16-byte pieces
        const uint64_t bytes = S->group_end[(size_t)(grp - S->groups.data())] - grp->name_off + (grp->name_off & 15);
        const unsigned piece_blocks = blocks_for((bytes + 15) / 16, 256), line_blocks = blocks_for(cnt, 256);
        S->h_mb.p()[0] = ~0ull; S->h_mb.p()[1] = S->h_mb.p()[2] = S->h_mb.p()[3] = 0;
        MSIM_HIP(c, hipMemcpyAsync(S->d_mb.p(), S->h_mb.p(), 4 * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
        MSIM_HIP(c, S->tm.begin(c->stream));
        hipLaunchKernelGGL(k_cons_ends, dim3(line_blocks), dim3(256), 0, c->stream, t, S->d_ls.p(), S->d_tabcum.p(), first, cnt, grp->name_len, S->nf0,
                           S->sample, S->hap, g->len, S->d_cons.p(), S->d_mb.p());
        hipLaunchKernelGGL(k_cons_sep, dim3(piece_blocks), dim3(256), 0, c->stream, t, S->d_ls.p(), first, cnt, S->d_cons.p());
        hipLaunchKernelGGL(k_cons_lines, dim3(line_blocks), dim3(256), 0, c->stream, t, first, cnt, in, g->len, S->d_cons.p(), S->d_mb.p());
        rc = run_scan(c, S, ConsEmitF{S->d_cons.p(), g->d_recs.p(), S->d_recline.p()}, cnt, S->d_mb.p() + 4);
        if (rc) return rc;
        hipLaunchKernelGGL(k_cons_neigh, dim3(blocks_for(2 * cnt, 256)), dim3(256), 0, c->stream, g->d_recs.p(), S->d_recline.p(), S->d_mb.p() + 4, first, S->d_mb.p());
        MSIM_HIP(c, hipGetLastError());
        MSIM_HIP(c, S->tm.end(c->stream));
        if ((rc = fetch_mailbox(c, S))) return rc;
        if ((rc = S->tm.add_elapsed(c, &S->plan_ms))) return rc;
        // as plan_device: a refusal found so far does not end the pass, and with one pending, or with sums of 2^32 or more,
        // the per-byte pass checks only and writes no pool byte
        too_long = g->len + S->h_mb.p()[1] >= (1ull << 32);
        const bool check_only = too_long || S->h_mb.p()[0] != ~0ull;
        n_rec = S->h_mb.p()[4];
        pool_len = check_only ? 0 : S->h_mb.p()[5];
        any_sv = S->h_mb.p()[3] & 1;
        rc = dev_reserve(c, g->d_pool, (size_t)pool_len + 2 * PAD);
        if (rc) return rc;
        MSIM_HIP(c, S->tm.begin(c->stream));
        hipLaunchKernelGGL(k_cons_long, dim3(piece_blocks), dim3(256), 0, c->stream, t, S->d_ls.p(), first, cnt, S->d_cons.p(), in, g->d_pool.p() + PAD, pool_len,
                           S->d_mb.p());
        MSIM_HIP(c, hipGetLastError());
        MSIM_HIP(c, S->tm.end(c->stream));
        if ((rc = fetch_mailbox(c, S))) return rc;
        if ((rc = S->tm.add_elapsed(c, &S->plan_ms))) return rc;
        if (S->h_mb.p()[0] != ~0ull) return vcf_fail(c, S->h_mb.p()[0] >> 4, (uint32_t)(S->h_mb.p()[0] & 15));
        if (too_long) return vcf_fail(c, grp->first_line + 1, VCF_R_LENGTH);
    } else {
        rc = dev_reserve(c, g->d_pool, 2 * PAD);
        if (rc) return rc;
    }
    g->n_rec = n_rec;
    g->pool_len = pool_len;
    g->plan_empty = n_rec == 0;
    g->all_snp = !any_sv;
    g->planned = true;
    return MSIM_OK;
}

}  // namespace

bool vcf_last_plan(const Ctx *c, int contig, VcfPlanView *v) {
    const VcfState *S = c->vcf;
    if (!S || c->host_only || S->grammar != 1 || S->last_contig != contig || contig < 0 || (size_t)contig >= c->contigs.size()) return false;
    const Contig &g = c->contigs[(size_t)contig];
    if (!g.planned || g.hap != 0 || g.table_gen != S->last_gen || g.n_rec != S->last_recs || S->last_first + S->last_lines > S->n_lines) return false;
    *v = VcfPlanView{S->d_text.p() + PAD, S->d_ls.p(), S->d_tabcum.p(), S->d_recline.p(), S->last_first, S->last_lines, S->last_recs, S->nf0, S->sample};
    return true;
}

void vcf_state_destroy(Ctx *c) {
    if (!c->vcf) return;
    if (!c->host_only) {
        (void)hipSetDevice(c->device);
        (void)wait_stream(c->stream);
        c->vcf->tm.destroy();
    }
    delete c->vcf;
    c->vcf = nullptr;
}

}  // namespace msim

using namespace msim;

extern "C" {

int msim_vcf_load(msim_ctx *p, const uint8_t *text, uint64_t n, uint64_t *n_lines, uint64_t *n_groups) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || (!text && n)) return MSIM_ERR_ARG;
    int rc = ctx_flush_queued(c);
    if (rc) return rc;
    if (n >= (1ull << 40)) return fail(c, MSIM_ERR_UNSUPPORTED, "VCF text of 1 TiB or more");
    vcf_state_destroy(c);
    c->vcf = new VcfState;
    c->vcf->n = n;
    if (c->host_only) load_host(c->vcf, text, n);
    else {
        TraceRange tr("msim VCF load");
        rc = load_device(c, c->vcf, text, n);
        if (rc) { vcf_state_destroy(c); return rc; }
    }
    if (n_lines) *n_lines = c->vcf->n_lines;
    if (n_groups) *n_groups = c->vcf->n_groups;
    return MSIM_OK;
}

int msim_vcf_groups(msim_ctx *p, msim_vcf_group *out, uint64_t cap, uint64_t *n_groups) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !n_groups || (cap && !out)) return MSIM_ERR_ARG;
    if (!c->vcf) return fail(c, MSIM_ERR_ARG, "msim_vcf_groups before msim_vcf_load");
    *n_groups = c->vcf->groups.size();
    const uint64_t k = std::min<uint64_t>(cap, c->vcf->groups.size());
    if (k) memcpy(out, c->vcf->groups.data(), (size_t)k * sizeof(msim_vcf_group));
    return MSIM_OK;
}

int msim_vcf_plan_contig(msim_ctx *p, int contig, int64_t group) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    int rc = ctx_flush_queued(c);
    if (rc) return rc;
    VcfState *S = c->vcf;
    if (!S) return fail(c, MSIM_ERR_ARG, "msim_vcf_plan_contig before msim_vcf_load");
    if (contig < 0 || (size_t)contig >= c->contigs.size()) return fail(c, MSIM_ERR_ARG, "no such contig");
    if (group < -1 || (group >= 0 && (uint64_t)group >= S->groups.size())) return fail(c, MSIM_ERR_ARG, "no such VCF group");
    Contig *g = &c->contigs[(size_t)contig];
    const msim_vcf_group *grp = group >= 0 ? &S->groups[(size_t)group] : nullptr;
    if (c->host_only) {
        if (g->len && g->h_in.size() != g->len) return fail(c, MSIM_ERR_ARG, "host-only context: the contig's bases were not given (msim_vcf_host_bases)");
        return S->grammar ? plan_host_cons(c, S, g, grp) : plan_host(c, S, g, grp);
    }
    TraceRange tr("msim VCF plan contig");
    S->last_contig = -1;
    if (!S->grammar) return plan_device(c, S, g, grp);
    rc = plan_device_cons(c, S, g, grp);
    if (!rc) {
        S->last_contig = contig;
        S->last_first = grp ? grp->first_line : 0;
        S->last_lines = grp ? grp->n_lines : 0;
        S->last_recs = g->n_rec;
        S->last_gen = g->table_gen;
    }
    return rc;
}

int msim_vcf_select(msim_ctx *p, uint32_t grammar, uint32_t sample_index, uint32_t haplotype) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    int rc = ctx_flush_queued(c);
    if (rc) return rc;
    VcfState *S = c->vcf;
    if (!S) return fail(c, MSIM_ERR_ARG, "msim_vcf_select before msim_vcf_load");
    if (grammar > 1) return fail(c, MSIM_ERR_ARG, "msim_vcf_select: grammar is 0 (the simulator's dialect) or 1 (consensus)");
    if (grammar == 0) {
        if (sample_index || haplotype > 1) return fail(c, MSIM_ERR_ARG, "msim_vcf_select: the dialect has one haploid sample");
        S->grammar = 0;
        return MSIM_OK;
    }
    if (haplotype < 1) return fail(c, MSIM_ERR_ARG, "msim_vcf_select: haplotypes count from 1");
    uint32_t nf0 = 0;
    if (S->n_lines > S->n_header) {                        // the first data line's fields: every line must have as many
        if (c->host_only) nf0 = S->h_tabcum[S->n_header + 1] - S->h_tabcum[S->n_header] + 1;
        else {
            uint32_t *two = reinterpret_cast<uint32_t *>(&S->h_mb.p()[6]);       // (staged in the pinned mailbox)
            MSIM_HIP(c, hipMemcpyAsync(two, S->d_tabcum.p() + S->n_header, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            if ((rc = wait_ctx(c, false))) return rc;
            nf0 = two[1] - two[0] + 1;
        }
    }
    if (nf0 >= 10 && sample_index >= nf0 - 9)
        return fail(c, MSIM_ERR_ARG, "msim_vcf_select: sample column " + std::to_string(sample_index) + " of " + std::to_string(nf0 - 9));
    if (!c->host_only) {                                   // per-line state for the largest group: 88 + 8 bytes a line
        uint64_t most = 0;
        for (const msim_vcf_group &g : S->groups) most = std::max<uint64_t>(most, g.n_lines);
        if (!S->d_cons) MSIM_HIP(c, dev_alloc(S->d_cons, (most + 1) * sizeof(VcfCons)));
        if (!S->d_recline) MSIM_HIP(c, dev_alloc(S->d_recline, 2 * (most + 1) * sizeof(uint32_t)));
    }
    S->grammar = 1; S->sample = sample_index; S->hap = haplotype; S->nf0 = nf0;
    S->last_contig = -1;
    return MSIM_OK;
}

int msim_vcf_host_bases(msim_ctx *p, int contig, const uint8_t *bases) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    if (!c->host_only) return MSIM_OK;                     // (a device context has them in HBM)
    if (contig < 0 || (size_t)contig >= c->contigs.size()) return fail(c, MSIM_ERR_ARG, "no such contig");
    Contig &g = c->contigs[(size_t)contig];
    if (!bases && g.len) return MSIM_ERR_ARG;
    g.h_in.assign(bases, bases + g.len);
    return MSIM_OK;
}

int msim_vcf_timing(msim_ctx *p, double *load_kernel_ms, double *plan_kernel_ms) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    if (load_kernel_ms) *load_kernel_ms = c->vcf ? c->vcf->load_ms : 0.0;
    if (plan_kernel_ms) *plan_kernel_ms = c->vcf ? c->vcf->plan_ms : 0.0;
    return MSIM_OK;
}

int msim_vcf_release(msim_ctx *p) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    int rc = ctx_flush_queued(c);
    if (!rc) rc = ctx_drain(c);
    vcf_state_destroy(c);
    return rc;
}

}  // extern "C"
