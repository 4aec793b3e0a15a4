// FASTQ reads drawn from the resident genome ("reads" mode; msim.h: msim_reads_*).  A read is a pure function of (key, read
// index): nothing chains, nothing is scanned -- every record of a run is `stride` bytes long, so read i lies at byte i * stride
// of its file and any range [first, first + count) renders on its own.  The arithmetic is reads.h's, shared with the host
// restatement at the end of this file.
//
// Device path (gfx950), everything on the context's stream:
//   k_reads_render   a workgroup takes R reads (R a multiple of 16: its slab of R * stride bytes starts 16-byte aligned in the
//                    chunk): one lane per read draws the placement (Philox, two binary searches) into LDS; then a wave per
//                    read assembles the record in LDS -- a lane takes two neighbouring cycles, which share one Philox call, and
//                    the wave's genome bytes are contiguous; then the slab streams out in 16-byte stores (the ragged last
//                    workgroup of a call bytewise).  All LDS is dynamic (slab, then the placements, 16-byte aligned).
// Philox bounds it, not HBM: a read costs LEN / 2 + 1 calls and moves stride + LEN bytes.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "reads.h"

namespace msim {

using fastrng::Key;
using fastrng::U4;
using reads::Layout;
using reads::Place;

namespace {

constexpr int LANES = 256, WAVES = LANES / 64;
constexpr uint32_t SLAB_BYTES = 32768;                     // R * stride stays at or below it (R = 16 where 16 records exceed it: 17.5 KB at most)
constexpr uint32_t R_MAX = 256;                            // one placement a lane
constexpr uint64_t CALL_BYTES_MAX = 1ull << 30;            // text of one render call
constexpr int TIMERS = 8;                                  // launches whose events may be unread: two buffers a channel are in flight at most

inline uint32_t reads_per_group(uint32_t stride) {
    const uint32_t r = SLAB_BYTES / stride / 16 * 16;
    return r < 16 ? 16 : r > R_MAX ? R_MAX : r;
}

// what a run fixes, as the kernel takes it (by value)
struct RenderArgs {
    const uint64_t *prefix_w;          // [n_elig]
    const uint8_t *const *base;        // [n_elig] the eligible contigs' bases
    const uint32_t *cnum;              // [n_elig] their 1-based numbers in the Fasta
    const uint64_t *frag_thr;          // [n_frag]
    const uint64_t *err_thr;           // [2][len]
    const uint8_t *qual;               // [2][len]
    uint64_t P;
    Key key;
    Layout y;
    uint32_t n_elig, frag_min, n_frag, R;
    uint8_t prefix[reads::MAX_PREFIX];
};

extern __shared__ __attribute__((aligned(16))) uint8_t reads_smem[];

__global__ __launch_bounds__(LANES) void k_reads_render(const RenderArgs a, uint32_t mate, uint64_t first, uint32_t count,
                                                        uint8_t *__restrict__ out, unsigned long long *__restrict__ all_n) {
    const uint32_t R = a.R, stride = a.y.stride, len = a.y.len;
    uint8_t *slab = reads_smem;
    Place *place = reinterpret_cast<Place *>(reads_smem + ((R * stride + 15u) & ~15u));
    const uint32_t r0 = blockIdx.x * R;                    // the workgroup's first read, counted from `first`
    const uint32_t n = count - r0 < R ? count - r0 : R;
    for (uint32_t r = threadIdx.x; r < n; r += LANES)
        place[r] = reads::place_of(a.key, (uint32_t)(first + r0 + r), a.prefix_w, a.n_elig, a.P, a.frag_min, a.frag_thr, a.n_frag);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t *err_thr = a.err_thr + (size_t)mate * len;
    const uint8_t *qual = a.qual + (size_t)mate * len;
    for (uint32_t r = wave; r < n; r += WAVES) {
        const Place pl = place[r];
        const uint64_t i = first + r0 + r;
        const uint8_t *__restrict__ g = a.base[pl.c];
        uint8_t *rec = slab + r * stride;
        const uint32_t cnum = a.cnum[pl.c];
        for (uint32_t k = lane; k < a.y.name; k += 64) rec[k] = reads::name_byte(a.y, a.prefix, k, i, cnum, pl, mate);
        uint8_t *seq = rec + a.y.name, *ql = seq + len + 3;
        if (lane == 0) { seq[len] = '\n'; seq[len + 1] = '+'; seq[len + 2] = '\n'; ql[len] = '\n'; }
        bool some_base = false;
        for (uint32_t j0 = 2 * lane; j0 < len; j0 += 128) {               // cycles j0 and j0 + 1 share a call
            const U4 w = fastrng::draw4(a.key, (uint32_t)i, (mate << 16) | (j0 >> 1), reads::TAG_RERR);
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                const uint32_t j = j0 + h;
                if (j >= len) break;
                bool comp;
                const uint32_t off = reads::genome_offset(pl, mate, j, &comp);
                uint8_t b, q;
                reads::cycle_of(g[off], comp, reads::cycle_word(w, j), err_thr[j], qual[j], &b, &q);
                seq[j] = b;
                ql[j] = q;
                some_base |= b != 'N';
            }
        }
        if (__ballot(some_base) == 0 && lane == 0) atomicAdd(all_n + mate, 1ull);
    }
    __syncthreads();
    uint8_t *dst = out + (uint64_t)r0 * stride;
    if (n == R) {                                          // R * stride is a multiple of 16, and so is the slab's offset in `out`
        const uint32_t bytes = R * stride;
        for (uint32_t o = threadIdx.x * 16u; o < bytes; o += LANES * 16u)
            *reinterpret_cast<uint4 *>(dst + o) = *reinterpret_cast<const uint4 *>(slab + o);
    } else {
        const uint32_t bytes = n * stride;
        for (uint32_t o = threadIdx.x; o < bytes; o += LANES) dst[o] = slab[o];
    }
}

// the host's half of the rule: which contigs are eligible, their weights' prefix sums, the layout
struct Plan {
    std::vector<uint32_t> idx;         // eligible contigs: index among all contigs (its Fasta number - 1)
    std::vector<uint64_t> prefix_w;
    uint64_t P = 0, fmax = 0;
    Layout y{};
};

int fail_reads(Ctx *c, const std::string &msg) { return fail(c, MSIM_ERR_ARG, "reads: " + msg); }

int check_params(Ctx *c, const msim_reads_params *pr, uint32_t *plen) {
    if (!pr || !pr->frag_thr || !pr->err_thr || !pr->qual || !pr->prefix) return MSIM_ERR_ARG;
    if (pr->len < 1 || pr->len > reads::MAX_LEN) return fail_reads(c, "read length outside 1..512");
    if (pr->n_reads < 1 || pr->n_reads >= (1ull << 32)) return fail_reads(c, "number of reads outside 1..2^32 - 1");
    if (pr->n_frag < 1 || pr->n_frag > reads::MAX_FRAG) return fail_reads(c, "fragment table outside 1..4096 entries");
    if (pr->frag_min < pr->len) return fail_reads(c, "shortest fragment below the read length");
    if (pr->paired > 1) return fail_reads(c, "paired is 0 or 1");
    for (uint32_t k = 0; k < pr->n_frag; k++)
        if (k ? pr->frag_thr[k] < pr->frag_thr[k - 1] : false) return fail_reads(c, "fragment thresholds do not ascend");
    if (pr->frag_thr[pr->n_frag - 1] != reads::ONE53) return fail_reads(c, "the last fragment threshold is not 2^53");
    for (uint32_t j = 0; j < 2 * pr->len; j++) {
        if (pr->err_thr[j] > reads::ONE53) return fail_reads(c, "error threshold above 2^53");
        if (pr->qual[j] < '!' || pr->qual[j] > '~') return fail_reads(c, "quality byte outside '!'..'~'");
    }
    const size_t n = strnlen(pr->prefix, reads::MAX_PREFIX + 1);
    if (n > reads::MAX_PREFIX) return fail_reads(c, "prefix longer than 32 bytes");
    for (size_t k = 0; k < n; k++) {
        const char ch = pr->prefix[k];
        const bool ok = (ch >= 'a' && ch <= 'z') || (ch >= 'A' && ch <= 'Z') || (ch >= '0' && ch <= '9') || ch == '.' || ch == '_' || ch == '-';
        if (!ok) return fail_reads(c, "prefix takes letters, digits and ._- only");
    }
    *plen = (uint32_t)n;
    return MSIM_OK;
}

template <class LenOf> int make_plan(Ctx *c, const msim_reads_params *pr, uint32_t plen, uint64_t n_contigs, LenOf len_of, Plan &pl) {
    pl.fmax = (uint64_t)pr->frag_min + pr->n_frag - 1;
    uint64_t longest = 0;
    for (uint64_t k = 0; k < n_contigs; k++) {
        const uint64_t L = len_of(k);
        if (L < pl.fmax) continue;
        if (L >= (1ull << 32)) return fail(c, MSIM_ERR_UNSUPPORTED, "contig of 4 GiB or more");
        pl.idx.push_back((uint32_t)k);
        pl.prefix_w.push_back(pl.P);
        pl.P += L - pl.fmax + 1;
        longest = std::max(longest, L);
    }
    if (pl.idx.empty()) return fail(c, MSIM_ERR_VALUE, "reads: no contig is as long as the longest fragment (" + std::to_string(pl.fmax) + " bases)");
    pl.y = reads::layout_of(pr->len, plen, pr->n_reads - 1, (uint64_t)pl.idx.back() + 1, longest, pl.fmax);
    return MSIM_OK;
}

// [first, first + count) must be indexes the run's name field holds
int check_range(Ctx *c, const Layout &y, int paired, int mate, uint64_t first, uint64_t count) {
    if (mate < 0 || mate > (paired ? 1 : 0)) return fail_reads(c, "no such mate");
    if (first > (1ull << 32) || count > (1ull << 32) - first) return fail_reads(c, "read index beyond 2^32 - 1");
    if (count && reads::digits_of(first + count - 1) > y.w_i) return fail_reads(c, "read index wider than the run's index field");
    if (count * y.stride > CALL_BYTES_MAX) return fail_reads(c, "more than 1 GiB of text in one call");
    return MSIM_OK;
}

}  // namespace

struct ReadsState {
    bool ready = false;
    RenderArgs args{};
    int paired = 0;
    Scratch<uint8_t> d_tab;                    // every table of the run, one upload
    Scratch<unsigned long long> d_all_n;       // reads of mate 1 / mate 2 that hold only N
    Scratch<uint8_t> d_out;                    // msim_reads_render's text (dev_reserve)
    EventPair tm[TIMERS];
    bool tm_used[TIMERS] = {};
    bool tm_made = false;
    int next_tm = 0;
    double kernel_ms = 0;
};

namespace {

int state_of(Ctx *c, ReadsState **out) {
    if (!c->reads) {
        ReadsState *S = new ReadsState;
        c->reads = S;
        MSIM_HIP(c, dev_alloc(S->d_all_n, 2 * sizeof(unsigned long long)));
        MSIM_HIP(c, hipMemsetAsync(S->d_all_n.p(), 0, 2 * sizeof(unsigned long long), c->stream));
        for (auto &t : S->tm) MSIM_HIP(c, t.create());
        S->tm_made = true;
    }
    *out = c->reads;
    return MSIM_OK;
}

int harvest(Ctx *c, ReadsState *S, int k) {
    if (!S->tm_used[k]) return MSIM_OK;
    MSIM_HIP(c, wait_event(S->tm[k].e1));
    S->tm_used[k] = false;
    return S->tm[k].add_elapsed(c, &S->kernel_ms);
}

// `count` records of `mate` from read `first` on into d_dst (16-byte aligned, count * stride bytes), on the context's stream
int render_device(Ctx *c, ReadsState *S, int mate, uint64_t first, uint64_t count, uint8_t *d_dst) {
    if (!count) return MSIM_OK;
    const RenderArgs &a = S->args;
    const unsigned blocks = (unsigned)((count + a.R - 1) / a.R);
    const size_t lds = (((size_t)a.R * a.y.stride + 15) & ~(size_t)15) + (size_t)a.R * sizeof(Place);
    const int k = S->next_tm;
    S->next_tm = (k + 1) % TIMERS;
    int rc = harvest(c, S, k);
    if (rc) return rc;
    MSIM_HIP(c, S->tm[k].begin(c->stream));
    hipLaunchKernelGGL(k_reads_render, dim3(blocks), dim3(LANES), lds, c->stream, a, (uint32_t)mate, first, (uint32_t)count, d_dst,
                       S->d_all_n.p());
    MSIM_HIP(c, hipGetLastError());
    MSIM_HIP(c, S->tm[k].end(c->stream));
    S->tm_used[k] = true;
    return MSIM_OK;
}

}  // namespace

void reads_state_destroy(Ctx *c) {
    ReadsState *S = c->reads;
    if (!S) return;
    for (auto &t : S->tm) t.destroy();
    delete S;
    c->reads = nullptr;
}

void reads_forget(Ctx *c) {
    if (c->reads) c->reads->ready = false;
}

void reads_reset_timing(Ctx *c) {
    if (!c->reads) return;
    for (int k = 0; k < TIMERS; k++) c->reads->tm_used[k] = false;       // (the caller drained the context)
    c->reads->kernel_ms = 0;
}

}  // namespace msim

using namespace msim;

extern "C" {

int msim_reads_setup(msim_ctx *p, const msim_reads_params *pr, uint64_t *stride, uint64_t *n_eligible, uint64_t *P) {
    CTX_FLUSHED(c, p)
    if (!c || !pr || !stride || !n_eligible || !P) return MSIM_ERR_ARG;
    if (c->host_only) return fail(c, MSIM_ERR_HIP, "host-only context: this call needs the GPU");
    uint32_t plen = 0;
    int rc = check_params(c, pr, &plen);
    if (rc) return rc;
    Plan pl;
    if ((rc = make_plan(c, pr, plen, c->contigs.size(), [&](uint64_t k) { return c->contigs[(size_t)k].len; }, pl))) return rc;
    if ((rc = ctx_drain(c))) return rc;                    // (a render of the last setup may still read its tables)
    ReadsState *S;
    if ((rc = state_of(c, &S))) return rc;
    S->ready = false;
    const size_t ne = pl.idx.size(), len = pr->len;
    // one block: prefix_w | base | frag_thr | err_thr | cnum | qual  (8-byte items first)
    const size_t o_pw = 0, o_base = o_pw + ne * 8, o_ft = o_base + ne * 8, o_et = o_ft + (size_t)pr->n_frag * 8, o_cn = o_et + 2 * len * 8,
                 o_q = o_cn + ne * 4, total = o_q + 2 * len;
    std::vector<uint8_t> h(total);
    memcpy(h.data() + o_pw, pl.prefix_w.data(), ne * 8);
    for (size_t k = 0; k < ne; k++) {
        const uint8_t *b = c->contigs[pl.idx[k]].d_in.p() + PAD;
        const uint32_t num = pl.idx[k] + 1;
        memcpy(h.data() + o_base + k * 8, &b, 8);
        memcpy(h.data() + o_cn + k * 4, &num, 4);
    }
    memcpy(h.data() + o_ft, pr->frag_thr, (size_t)pr->n_frag * 8);
    memcpy(h.data() + o_et, pr->err_thr, 2 * len * 8);
    memcpy(h.data() + o_q, pr->qual, 2 * len);
    if ((rc = dev_reserve(c, S->d_tab, total))) return rc;
    MSIM_HIP(c, hipMemcpyAsync(S->d_tab.p(), h.data(), total, hipMemcpyHostToDevice, c->stream));
    MSIM_HIP(c, hipMemsetAsync(S->d_all_n.p(), 0, 2 * sizeof(unsigned long long), c->stream));
    MSIM_HIP(c, wait_stream(c->stream));                   // (h goes out of scope)
    RenderArgs &a = S->args;
    uint8_t *t = S->d_tab.p();
    a.prefix_w = reinterpret_cast<const uint64_t *>(t + o_pw);
    a.base = reinterpret_cast<const uint8_t *const *>(t + o_base);
    a.frag_thr = reinterpret_cast<const uint64_t *>(t + o_ft);
    a.err_thr = reinterpret_cast<const uint64_t *>(t + o_et);
    a.cnum = reinterpret_cast<const uint32_t *>(t + o_cn);
    a.qual = t + o_q;
    a.P = pl.P;
    a.key = Key{(uint32_t)pr->key, (uint32_t)(pr->key >> 32), 0u};
    a.y = pl.y;
    a.n_elig = (uint32_t)ne;
    a.frag_min = pr->frag_min;
    a.n_frag = pr->n_frag;
    a.R = reads_per_group(pl.y.stride);
    memset(a.prefix, 0, sizeof a.prefix);
    memcpy(a.prefix, pr->prefix, plen);
    S->paired = (int)pr->paired;
    S->ready = true;
    *stride = pl.y.stride;
    *n_eligible = ne;
    *P = pl.P;
    return MSIM_OK;
}

int msim_reads_render(msim_ctx *p, int mate, uint64_t first, uint64_t count, uint8_t *out, uint64_t cap) {
    CTX_FLUSHED(c, p)
    if (!c || (!out && count)) return MSIM_ERR_ARG;
    if (c->host_only) return fail(c, MSIM_ERR_HIP, "host-only context: this call needs the GPU");
    ReadsState *S = c->reads;
    if (!S || !S->ready) return fail_reads(c, "msim_reads_setup has not run");
    int rc = check_range(c, S->args.y, S->paired, mate, first, count);
    if (rc) return rc;
    const uint64_t bytes = count * S->args.y.stride;
    if (cap < bytes) return fail_reads(c, "buffer too small");
    if (!count) return MSIM_OK;
    TraceRange tr("msim reads: render");
    if ((rc = dev_reserve(c, S->d_out, bytes))) return rc;
    if ((rc = render_device(c, S, mate, first, count, S->d_out.p()))) return rc;
    MSIM_HIP(c, hipMemcpyAsync(out, S->d_out.p(), bytes, hipMemcpyDeviceToHost, c->stream));
    MSIM_HIP(c, wait_stream(c->stream));
    return MSIM_OK;
}

int msim_reads_render_file(msim_ctx *p, int mate, uint64_t first, uint64_t count, int fd, uint64_t offset, uint64_t *written) {
    CTX_FLUSHED(c, p)
    if (!c || !written || fd < 0) return MSIM_ERR_ARG;
    if (c->host_only) return fail(c, MSIM_ERR_HIP, "host-only context: this call needs the GPU");
    ReadsState *S = c->reads;
    if (!S || !S->ready) return fail_reads(c, "msim_reads_setup has not run");
    int rc = check_range(c, S->args.y, S->paired, mate, first, count);
    if (rc) return rc;
    if ((rc = file_check(c, fd))) return rc;
    const uint64_t bytes = count * S->args.y.stride;
    *written = bytes;
    if (!count) return MSIM_OK;
    TraceRange tr("msim reads: render -> file");
    int slot;
    DevBlock *buf;
    if ((rc = file_text_buffer(c, mate, &slot, &buf))) return rc;
    if ((rc = dev_reserve(c, *buf, bytes))) return rc;
    if ((rc = render_device(c, S, mate, first, count, static_cast<uint8_t *>(buf->raw)))) return rc;
    return file_enqueue(c, mate, slot, bytes, fd, offset);
}

int msim_reads_timing(msim_ctx *p, double *kernel_ms, uint64_t all_n[2]) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c) return MSIM_ERR_ARG;
    if (kernel_ms) *kernel_ms = 0;
    if (all_n) all_n[0] = all_n[1] = 0;
    ReadsState *S = c->reads;
    if (!S || c->host_only) return MSIM_OK;
    MSIM_HIP(c, wait_stream(c->stream));
    for (int k = 0; k < TIMERS; k++) {
        const int rc = harvest(c, S, k);
        if (rc) return rc;
    }
    if (kernel_ms) *kernel_ms = S->kernel_ms;
    if (all_n) {
        unsigned long long h[2];
        MSIM_HIP(c, hipMemcpy(h, S->d_all_n.p(), sizeof h, hipMemcpyDeviceToHost));
        all_n[0] = h[0]; all_n[1] = h[1];
    }
    return MSIM_OK;
}

int msim_reads_release(msim_ctx *p) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    if (!c->reads) return MSIM_OK;
    int rc = ctx_drain(c);
    if (rc) return rc;
    if ((rc = file_wait(c))) return rc;                    // (the channels' buffers are theirs; the tables are ours)
    ReadsState *S = c->reads;
    S->ready = false;
    MSIM_HIP(c, S->d_tab.release());
    MSIM_HIP(c, S->d_out.release());
    return MSIM_OK;
}

// measurement support (tools/reads_bench.py; exported, not part of msim.h): a device-to-device copy of `bytes` bytes of rendered
// text into the context's scratch, timed by HIP events -- the streaming floor k_reads_render is held against
int msim_dbg_reads_copy_floor(msim_ctx *p, uint64_t bytes, double *ms) {
    CTX_FLUSHED(c, p)
    if (!c || !ms) return MSIM_ERR_ARG;
    if (c->host_only) return fail(c, MSIM_ERR_HIP, "host-only context: this call needs the GPU");
    ReadsState *S;
    int rc = state_of(c, &S);
    if (rc) return rc;
    if ((rc = ctx_drain(c))) return rc;
    if ((rc = dev_reserve(c, S->d_out, bytes))) return rc;
    EventPair tm;
    MSIM_HIP(c, tm.create());
    const CopySource text{S->d_out.p(), (size_t)bytes};
    rc = copy_floor(c, tm, &text, 1, ms);
    tm.destroy();
    return rc;
}

// measurement support (exported, not part of msim.h): msim_reads_render without the copy to the host -- the text stays in the
// context's buffer; msim_reads_timing reads the kernel's time
int msim_dbg_reads_render_device(msim_ctx *p, int mate, uint64_t first, uint64_t count) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    if (c->host_only) return fail(c, MSIM_ERR_HIP, "host-only context: this call needs the GPU");
    ReadsState *S = c->reads;
    if (!S || !S->ready) return fail_reads(c, "msim_reads_setup has not run");
    int rc = check_range(c, S->args.y, S->paired, mate, first, count);
    if (rc) return rc;
    if ((rc = dev_reserve(c, S->d_out, count * S->args.y.stride))) return rc;
    return render_device(c, S, mate, first, count, S->d_out.p());
}

// test support (exported, not part of msim.h): the reads a workgroup of k_reads_render takes at this stride -- where the
// chunk splits' edge cases lie
uint32_t msim_dbg_reads_group(uint32_t stride) { return stride ? reads_per_group(stride) : 0; }

// ---- the sequential host restatement: no context, no GPU -----------------------------------------------------------------
// bases: the contigs' bases one behind the other, contig k = bases[offsets[k], offsets[k + 1]).  out == NULL: the three
// results only.
int msim_dbg_reads_render(const msim_reads_params *pr, const uint8_t *bases, const uint64_t *offsets, uint32_t n_contigs, int mate,
                          uint64_t first, uint64_t count, uint8_t *out, uint64_t cap, uint64_t *stride, uint64_t *n_eligible,
                          uint64_t *P) {
    if (!pr || !offsets || !stride || !n_eligible || !P || (!bases && n_contigs && offsets[n_contigs])) return MSIM_ERR_ARG;
    uint32_t plen = 0;
    int rc = check_params(nullptr, pr, &plen);
    if (rc) return rc;
    for (uint32_t k = 0; k < n_contigs; k++)
        if (offsets[k + 1] < offsets[k]) return fail_reads(nullptr, "contig offsets do not ascend");
    Plan pl;
    if ((rc = make_plan(nullptr, pr, plen, n_contigs, [&](uint64_t k) { return offsets[k + 1] - offsets[k]; }, pl))) return rc;
    *stride = pl.y.stride;
    *n_eligible = pl.idx.size();
    *P = pl.P;
    if (!out) return MSIM_OK;
    if ((rc = check_range(nullptr, pl.y, (int)pr->paired, mate, first, count))) return rc;
    if (cap < count * pl.y.stride) return fail_reads(nullptr, "buffer too small");
    const Key key{(uint32_t)pr->key, (uint32_t)(pr->key >> 32), 0u};
    const Layout &y = pl.y;
    const uint32_t len = pr->len, m = (uint32_t)mate;
    const uint8_t *prefix = reinterpret_cast<const uint8_t *>(pr->prefix);
    for (uint64_t r = 0; r < count; r++) {
        const uint64_t i = first + r;
        const Place at = reads::place_of(key, (uint32_t)i, pl.prefix_w.data(), (uint32_t)pl.idx.size(), pl.P, pr->frag_min, pr->frag_thr,
                                         pr->n_frag);
        const uint8_t *g = bases + offsets[pl.idx[at.c]];
        uint8_t *rec = out + r * y.stride;
        for (uint32_t k = 0; k < y.name; k++) rec[k] = reads::name_byte(y, prefix, k, i, pl.idx[at.c] + 1, at, m);
        uint8_t *seq = rec + y.name, *ql = seq + len + 3;
        seq[len] = '\n'; seq[len + 1] = '+'; seq[len + 2] = '\n'; ql[len] = '\n';
        U4 w{};
        for (uint32_t j = 0; j < len; j++) {
            if (!(j & 1u)) w = fastrng::draw4(key, (uint32_t)i, (m << 16) | (j >> 1), reads::TAG_RERR);
            bool comp;
            const uint32_t off = reads::genome_offset(at, m, j, &comp);
            reads::cycle_of(g[off], comp, reads::cycle_word(w, j), pr->err_thr[(size_t)m * len + j], pr->qual[(size_t)m * len + j], &seq[j],
                            &ql[j]);
        }
    }
    return MSIM_OK;
}

}  // extern "C"
