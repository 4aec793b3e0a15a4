// Diploid runs: a genotype byte per record beside the record table, and one haplotype's records compacted into a table of
// their own.  gfx950 (MI355X) only.
//
// The record table PLAN leaves is a list of independent edits -- no record consumes input another one consumes, a TLI copies its
// span from the INPUT -- so any subset of it is a table APPLY takes through its generic route (apply.hip: k_delta_reduce,
// k_scan_sums, k_offsets).  A diploid run therefore plans once, gives every record a genotype (bit 0: on haplotype 1, bit 1: on
// haplotype 2; never 0) and applies the two subsets one after the other.  The genotype lives BESIDE the table (Contig::d_gt):
// msim_record::rsv stays 0 and no kernel of PLAN or APPLY learns anything new.
//
// The draw (k_gt_draw) comes from Philox4x32-10 (fast_math.h), never from the two MT19937 streams: the table, the VCF body and
// the generators' states after a diploid run are the haploid run's.  counter = (record index in the full table, 0, seq, TAG_GT):
//   heterozygous  iff  (lo64 >> 11) < het_thr          het_thr = ceil(F * 2^53), evaluated by the caller
//   phase         =    hi64 & 1                        0: haplotype 1, 1: haplotype 2
// A translocation moves as a whole: a TLI takes the draw of the TL whose pos is the TLI's extra (binary search over pos; the TLI
// keeps its own draw when the table holds no such TL).  It evaluates the TL's DRAW again instead of reading the TL's byte, so that
// one launch has no ordering inside it.
#include <cstring>

#include "ctx.h"
#include "fast_math.h"
#include "scan_kernels.h"

namespace msim {

namespace {

constexpr int HAP_THREADS = 256;
constexpr int HAP_WAVES = HAP_THREADS / 64;
constexpr int HAP_ROUNDS = 4;
constexpr int HAP_SLOTS = HAP_WAVES * HAP_ROUNDS;        // runs of 64 consecutive records of a workgroup
constexpr int HAP_BLOCK = 64 * HAP_SLOTS;                // records per workgroup of k_hap_count / k_hap_compact: 1024

MSIM_FHD inline uint8_t gt_of(const fastrng::U4 &v, uint64_t het_thr) {
    if (!((fastrng::lo64(v) >> 11) < het_thr)) return 3;
    return (fastrng::hi64(v) & 1u) ? (uint8_t)2 : (uint8_t)1;
}

// index of the TL record whose pos is `want`, or n (binary search: the table is sorted by pos, positions are distinct)
MSIM_FHD inline uint32_t find_tl(const msim_record *__restrict__ recs, uint32_t n, uint32_t want) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (recs[mid].pos < want) lo = mid + 1; else hi = mid;
    }
    return (lo < n && recs[lo].pos == want && recs[lo].type == MSIM_TL) ? lo : n;
}

MSIM_FHD inline uint8_t gt_record(const msim_record *__restrict__ recs, uint32_t n, uint32_t i, const fastrng::Key &key, uint64_t het_thr) {
    uint32_t src = i;
    if (recs[i].type == MSIM_TLI) {
        const uint32_t j = find_tl(recs, n, recs[i].extra);
        if (j < n) src = j;
    }
    return gt_of(fastrng::draw4(key, src, 0, fastrng::TAG_GT), het_thr);
}

__global__ __launch_bounds__(HAP_THREADS) void k_gt_draw(const msim_record *__restrict__ recs, uint32_t n, uint32_t k0, uint32_t k1,
                                                         uint32_t seq, unsigned long long het_thr, uint8_t *__restrict__ gt) {
    const uint32_t i = blockIdx.x * HAP_THREADS + threadIdx.x;
    if (i >= n) return;
    const fastrng::Key key{k0, k1, seq};
    gt[i] = gt_record(recs, n, i, key, het_thr);
}

// Records of a workgroup are taken in runs of 64 -- run s = round * HAP_WAVES + wave holds records base + 64 s .. + 63 --, one
// ballot per run: the kept records of a run keep their order (a lane's rank = the kept lanes below it), the runs theirs.
__device__ __forceinline__ unsigned long long hap_ballot(const uint8_t *__restrict__ gt, uint32_t n, uint32_t i, uint32_t hap) {
    const bool keep = i < n && (gt[i] & hap) != 0;
    return __ballot(keep);
}

__global__ __launch_bounds__(HAP_THREADS) void k_hap_count(const uint8_t *__restrict__ gt, uint32_t n, uint32_t hap,
                                                           uint32_t *__restrict__ block_cnt) {
    __shared__ uint32_t wcnt[HAP_WAVES];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t base = blockIdx.x * HAP_BLOCK;
    uint32_t cnt = 0;
#pragma unroll
    for (int r = 0; r < HAP_ROUNDS; r++)
        cnt += (uint32_t)__popcll(hap_ballot(gt, n, base + (uint32_t)(r * HAP_WAVES + (int)wave) * 64 + lane, hap));
    if (lane == 0) wcnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < HAP_WAVES; w++) t += wcnt[w];
        block_cnt[blockIdx.x] = t;
    }
}

// block_off: the exclusive scan of k_hap_count's counts (k_scan_u32).  One 16-byte load and one 16-byte store per kept record.
__global__ __launch_bounds__(HAP_THREADS) void k_hap_compact(const msim_record *__restrict__ recs, const uint8_t *__restrict__ gt,
                                                             uint32_t n, uint32_t hap, const uint32_t *__restrict__ block_off,
                                                             msim_record *__restrict__ out) {
    __shared__ uint32_t scnt[HAP_SLOTS];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t base = blockIdx.x * HAP_BLOCK;
    unsigned long long b[HAP_ROUNDS];
#pragma unroll
    for (int r = 0; r < HAP_ROUNDS; r++) {
        b[r] = hap_ballot(gt, n, base + (uint32_t)(r * HAP_WAVES + (int)wave) * 64 + lane, hap);
        if (lane == 0) scnt[r * HAP_WAVES + (int)wave] = (uint32_t)__popcll(b[r]);
    }
    __syncthreads();
    const uint32_t dst0 = block_off[blockIdx.x];
    const unsigned long long below = (1ull << lane) - 1;
#pragma unroll
    for (int r = 0; r < HAP_ROUNDS; r++) {
        const int slot = r * HAP_WAVES + (int)wave;
        uint32_t pre = 0;
#pragma unroll
        for (int s = 0; s < HAP_SLOTS; s++) pre += s < slot ? scnt[s] : 0u;
        if ((b[r] >> lane) & 1ull) {
            const uint32_t i = base + (uint32_t)slot * 64 + lane;
            const uint4 v = *reinterpret_cast<const uint4 *>(recs + i);      // (tables are 16-byte aligned: hipMalloc + 16 i)
            *reinterpret_cast<uint4 *>(out + dst0 + pre + (uint32_t)__popcll(b[r] & below)) = v;
        }
    }
}

}  // namespace

uint32_t hap_block() { return (uint32_t)HAP_BLOCK; }

void hap_restore_full(Contig &g) {
    if (!g.hap) return;
    g.d_recs_hap = std::move(g.d_recs);
    g.d_recs = std::move(g.full.d_recs);
    g.n_rec = g.full.n_rec;
    g.all_snp = g.full.all_snp;
    g.delta_known = g.full.delta_known;
    g.known_delta = g.full.known_delta;
    g.off_ready = false;               // (d_off holds a haplotype's offsets by now: the full table takes the scan route as well)
    g.applied = false;
    g.h_recs.swap(g.full.h_recs);
    g.full.h_recs.clear(); g.full.h_recs.shrink_to_fit();
    g.hap = 0;
}

void hap_forget(Contig &g) {
    hap_restore_full(g);
    g.have_gt = false;
    g.h_gt.clear(); g.h_gt.shrink_to_fit();
}

int hap_free(Ctx *c, Contig &g) {
    hap_forget(g);
    MSIM_HIP(c, g.d_recs_hap.release());
    MSIM_HIP(c, g.d_gt.release());
    return MSIM_OK;
}

TableView vcf_table(const Contig &g) {
    TableView v;
    v.d_recs = g.hap ? g.full.d_recs.p() : g.d_recs.p();
    v.n_rec = g.hap ? g.full.n_rec : g.n_rec;
    v.all_snp = g.hap ? g.full.all_snp : g.all_snp;
    v.d_gt = g.have_gt ? g.d_gt.p() : nullptr;
    return v;
}

// The draw for every record of the contig's FULL table (the caller drained: the table is complete and host-sized).
int hap_genotype(Ctx *c, Contig &g, uint64_t key, uint32_t seq, uint64_t het_thr) {
    hap_restore_full(g);
    const uint32_t n = (uint32_t)g.n_rec;
    const fastrng::Key k{(uint32_t)key, (uint32_t)(key >> 32), seq};
    if (c->host_only) {
        g.h_gt.resize(n);
        for (uint32_t i = 0; i < n; i++) g.h_gt[i] = gt_record(g.h_recs.data(), n, i, k, het_thr);
        g.have_gt = true;
        return MSIM_OK;
    }
    const int rc = dev_reserve(c, g.d_gt, (size_t)n + PAD);
    if (rc) return rc;
    if (n) {
        hipLaunchKernelGGL(k_gt_draw, dim3((n + HAP_THREADS - 1) / HAP_THREADS), dim3(HAP_THREADS), 0, c->stream, g.d_recs.p(), n,
                           k.k0, k.k1, k.seq, (unsigned long long)het_thr, g.d_gt.p());
        MSIM_HIP(c, hipGetLastError());
        MSIM_HIP(c, wait_stream(c->stream));
    }
    g.have_gt = true;
    return MSIM_OK;
}

int hap_set_genotypes(Ctx *c, Contig &g, const uint8_t *gt) {
    hap_restore_full(g);
    const size_t n = (size_t)g.n_rec;
    for (size_t i = 0; i < n; i++)
        if (gt[i] < 1 || gt[i] > 3) return fail(c, MSIM_ERR_ARG, "genotype byte outside 1..3 (record " + std::to_string(i) + ")");
    if (c->host_only) {
        g.h_gt.assign(gt, gt + n);
        g.have_gt = true;
        return MSIM_OK;
    }
    const int rc = dev_reserve(c, g.d_gt, n + PAD);
    if (rc) return rc;
    if (n) MSIM_HIP(c, hipMemcpyAsync(g.d_gt.p(), gt, n, hipMemcpyHostToDevice, c->stream));
    MSIM_HIP(c, wait_stream(c->stream));
    g.have_gt = true;
    return MSIM_OK;
}

int hap_fetch_genotypes(Ctx *c, Contig &g, uint8_t *dst) {
    const size_t n = (size_t)(g.hap ? g.full.n_rec : g.n_rec);
    if (!n) return MSIM_OK;
    if (c->host_only) { memcpy(dst, g.h_gt.data(), n); return MSIM_OK; }
    MSIM_HIP(c, hipMemcpyAsync(dst, g.d_gt.p(), n, hipMemcpyDeviceToHost, c->stream));
    MSIM_HIP(c, wait_stream(c->stream));
    return MSIM_OK;
}

// hap 1 / 2: the records with that bit set, in table order, become the contig's active table; 0: the full table again.
// The caller drained the context (msim_select_haplotype says why that is the whole ordering argument).
int hap_select(Ctx *c, Contig &g, int hap) {
    hap_restore_full(g);
    if (!hap) return MSIM_OK;
    const uint32_t n = (uint32_t)g.n_rec;
    uint32_t kept = 0;
    Contig::FullTable f;
    f.n_rec = g.n_rec; f.all_snp = g.all_snp; f.delta_known = g.delta_known; f.known_delta = g.known_delta;
    if (c->host_only) {
        std::vector<msim_record> sel;
        for (uint32_t i = 0; i < n; i++)
            if (g.h_gt[i] & hap) sel.push_back(g.h_recs[i]);
        kept = (uint32_t)sel.size();
        f.h_recs.swap(g.h_recs);
        g.h_recs.swap(sel);
    } else {
        const uint32_t nb = (n + HAP_BLOCK - 1) / HAP_BLOCK;
        if (n) {
            int rc = ensure_scratch(c, (size_t)(nb + 1) * sizeof(uint32_t));
            if (rc) return rc;
            uint32_t *d_cnt = reinterpret_cast<uint32_t *>(c->d_scratch.raw);
            hipLaunchKernelGGL(k_hap_count, dim3(nb), dim3(HAP_THREADS), 0, c->stream, g.d_gt.p(), n, (uint32_t)hap, d_cnt);
            hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, c->stream, d_cnt, nb);
            MSIM_HIP(c, hipGetLastError());
            MSIM_HIP(c, hipMemcpyAsync(&kept, d_cnt + nb, sizeof kept, hipMemcpyDeviceToHost, c->stream));
            MSIM_HIP(c, wait_stream(c->stream));
            if (kept > n) return fail(c, MSIM_ERR_HIP, "internal: haplotype selection counted more records than the table holds");
            if (kept) {
                rc = dev_reserve(c, g.d_recs_hap, (size_t)kept * sizeof(msim_record));
                if (rc) return rc;
                hipLaunchKernelGGL(k_hap_compact, dim3(nb), dim3(HAP_THREADS), 0, c->stream, g.d_recs.p(), g.d_gt.p(), n, (uint32_t)hap, d_cnt,
                                   g.d_recs_hap.p());
                MSIM_HIP(c, hipGetLastError());
                MSIM_HIP(c, wait_stream(c->stream));
            }
        }
        f.d_recs = std::move(g.d_recs);
        g.d_recs = std::move(g.d_recs_hap);
    }
    g.full = std::move(f);
    g.hap = hap;
    g.n_rec = kept;
    g.all_snp = g.full.all_snp || kept == 0;     // (a subset of an SNP-only table is one; any other subset takes the general kernels)
    g.delta_known = false;
    g.known_delta = 0;
    g.off_ready = false;
    g.d_dyn = nullptr;                 // (the sizes were collected: from here on this contig's tables are host-sized)
    g.sizes_pending = false;
    g.defer_apply = false;
    g.tile_index_by_plan = false;
    g.applied = false;
    return MSIM_OK;
}

}  // namespace msim
