// msim_batch_*: a batch of small contigs in one pass.   gfx950 (MI355X) only.
// An assembly with thousands of scaffolds pays a fixed ~0.35 ms of HIP API work per contig on the per-contig path
// (allocations, ~40 runtime calls, two or three synchronising fetches): 20 000 scaffolds of 10 kb ran at 27 Mbases/s.
// Here mutate()'s loop body (mutator.py:111-141) runs for MANY small contigs in one pass: the host strips the FASTA
// text and walks the RNG chain contig by contig (plan_contig_host -- these contigs are below every device engine's
// threshold anyway), the record tables are concatenated with their positions shifted to the contig's place in ONE
// super-contig, the GPU runs ONE APPLY over it (records never cross a contig border, so the rewrite kernels need no
// change), and the host frames the mutated stream per contig and renders the VCF lines (msim_render_vcf).
//
// msim_batch_run is BatchRun's phases: lay_out, ingest (a thread of its own) beside plan, vcf_text (likewise) beside apply + text_layout.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <system_error>
#include <thread>
#include <sys/mman.h>

#include "ctx.h"
#include "plan_gpu.h"

namespace msim {

// One malloc'ed host block and its capacity: a move-only owner, grown by its one reserve() (contents are NOT kept), freed with it.
// TEXT: never zero-filled, want + 1/8 + 4 KB.  STAGING of a batch's bases: plain page-aligned memory, want + 1/4 in 2 MB pages.
// Page-locked memory does not pay there: hipHostMalloc pins at ~4 GB/s (90 ms for the 400 MB of a 16 k-contig batch, and as
// long again to release), while copies to and from touched pageable memory run at the link's speed on this platform and into
// fresh pages at 20 GB/s.
enum BlockKind { TEXT, STAGING };
template <BlockKind K> struct HostBlock {
    uint8_t *p = nullptr;
    size_t cap = 0;
    HostBlock() = default;
    HostBlock(HostBlock &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    HostBlock &operator=(HostBlock &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~HostBlock() { free(p); }
    bool reserve(size_t want) {
        if (cap >= want) return true;
        free(p);
        const size_t huge = (size_t)2 << 20;
        const size_t sz = K == STAGING ? (want + want / 4 + huge) & ~(huge - 1) : want + want / 8 + 4096;
        p = static_cast<uint8_t *>(K == STAGING ? aligned_alloc(huge, sz) : malloc(sz));
        cap = p ? sz : 0;
#ifdef MADV_HUGEPAGE
        if (K == STAGING && p) (void)madvise(p, sz, MADV_HUGEPAGE);   // 2 MB pages where the kernel grants them: 512x fewer faults and unmaps
#endif
        return p != nullptr;
    }
};

struct Batch {
    struct Item { uint64_t base = 0, len = 0, out_start = 0, out_len = 0, rec0 = 0, nrec = 0, pool0 = 0, npool = 0, text0 = 0, ntext = 0,
                  vcf0 = 0, nvcf = 0; uint32_t bpl = 0; bool empty = true;
                  const char *header = nullptr; uint32_t header_len = 0; bool nl_before = false; };   // the record's defline (caller's memory)
    std::vector<Item> items;
    std::vector<msim_record> recs_rel;       // per-contig coordinates (what the VCF renderer reads)
    std::vector<uint8_t> pool;
    HostBlock<STAGING> h_in, h_out;
    HostBlock<TEXT> fasta, vcf;              // fasta: framed on demand (batch_framed)
    size_t fasta_len = 0, vcf_len = 0;
    bool framed = false;
    uint64_t last_line_bases = 0;            // bases on the (partial) last line of the FASTA text
    int key_contig = -1;
};

void batch_free(Ctx *c) {
    if (!c->batch) return;
    file_channel_idle(c, 0);                               // (an output channel may still be writing the batch's texts)
    file_channel_idle(c, 1);
    const auto t0 = std::chrono::steady_clock::now();
    delete c->batch;
    c->batch = nullptr;
    if (getenv("MSIM_BATCH_PROF")) fprintf(stderr, "  batch_free %.1f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

// Contigs [0, n) in `parts` consecutive slices, one host thread each (text work of a batch: ingest, framing, VCF lines).
static int batch_threads() {
    static const int t = [] {
        if (const char *e = getenv("MSIM_BATCH_THREADS")) return std::max(1, atoi(e));
        const unsigned hw = std::thread::hardware_concurrency();
        return (int)std::min<unsigned>(16, std::max<unsigned>(1, hw / 2));
    }();
    return t;
}
template <class F> static void parallel_slices(int n, F f) {   // f(part, i0, i1)
    const int parts = std::max(1, std::min(batch_threads(), n / 64));
    if (parts == 1) { f(0, 0, n); return; }
    std::vector<std::thread> th;
    int started = 1;                                       // slices [0, started) run or have run; the rest falls to this thread
    try {
        for (int t = 1; t < parts; t++, started++)
            th.emplace_back(f, t, (int)((long long)n * t / parts), (int)((long long)n * (t + 1) / parts));
    } catch (const std::system_error &) {                  // no more threads to be had: the remaining slices run here
    }
    f(0, 0, (int)((long long)n / parts));
    for (int t = started; t < parts; t++) f(t, (int)((long long)n * t / parts), (int)((long long)n * (t + 1) / parts));
    for (auto &x : th) x.join();
}
// `side` on a helper thread while `here` runs on this one.  The thread lives inside this call and is joined on every way out of
// it, so it has ended before anything its caller holds -- all it can reference -- dies.  No thread to be had: side, then here.
template <class S, class H> static int beside(S side, H here) {
    struct Joined {
        std::thread th;
        ~Joined() { if (th.joinable()) th.join(); }
    } helper;
    try { helper.th = std::thread(side); } catch (const std::system_error &) { side(); }
    return here();
}

// The temporary super-contig: the context's last contig while this lives.  It leaves the context with this object, on EVERY way
// out of msim_batch_run (HIP failures included: a contig left behind would leak its device buffers and shift the ids of the
// caller's later contigs) -- or sooner, by drop().
struct SuperContig {
    Ctx *c;
    Contig *g = nullptr;                                   // (c->contigs does not grow during the batch: g stays valid)
    explicit SuperContig(Ctx *ctx) : c(ctx) {}
    SuperContig(const SuperContig &) = delete;
    int make(uint64_t len) { return new_contig(c, len, &g); }
    void drop() { if (g) { g = nullptr; (void)free_contig(c, c->contigs.back(), false); c->contigs.pop_back(); } }
    ~SuperContig() { drop(); }
};

using Clock = std::chrono::steady_clock;
static double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// One msim_batch_run: its phases, in the order they start, and what they hand to each other.
struct BatchRun {
    Ctx *c; Batch &B; const msim_batch_contig *contigs; int n;
    uint64_t total = 0, out_total = 0;       // bases in, bases out
    std::vector<msim_record> recs_abs;       // the super-contig's table
    long long delta_total = 0; bool all_snp = true;
    hipError_t ingest_err = hipSuccess;      // what the helper threads report
    int vcf_rc = MSIM_OK; const char *vcf_msg = "";
    double ingest_ms = 0, vcf_ms = 0;
    Clock::time_point t_1, t_2, t_3;
    BatchRun(Ctx *ctx, Batch &b, const msim_batch_contig *q, int count) : c(ctx), B(b), contigs(q), n(count) {}

    // ---- 0. the arguments, every contig's place in the super-contig
    int lay_out() {
        B.items.assign((size_t)n, Batch::Item());
        B.recs_rel.clear(); B.pool.clear(); B.fasta_len = 0; B.vcf_len = 0; B.last_line_bases = 0; B.framed = false;
        B.key_contig = -1;
        for (int i = 0; i < n; i++) {
            const msim_batch_contig &q = contigs[i];
            if ((!q.body && q.n_bases) || (q.n_ranges && !q.ranges) || q.n_ranges < 0 || !q.name) return fail(c, MSIM_ERR_ARG, "msim_batch_run: bad contig");
            if (q.n_bases) {
                if (q.lenc == 0 || q.lenb < q.lenc) return fail(c, MSIM_ERR_ARG, "line width / line stride of the FASTA body are inconsistent");
                const uint64_t last = (q.n_bases - 1) / q.lenc * q.lenb + (q.n_bases - 1) % q.lenc;
                if (last >= q.body_bytes) return fail(c, MSIM_ERR_ARG, "FASTA body shorter than n_bases at this line width");
            }
            B.items[(size_t)i].base = total;
            B.items[(size_t)i].len = q.n_bases;
            B.items[(size_t)i].bpl = q.lenc;
            total += q.n_bases;
        }
        if (total >= (1ull << 31)) return fail(c, MSIM_ERR_UNSUPPORTED, "batch of 2 GiB or more: split it");
        return MSIM_OK;
    }

    // ---- 1. FASTA text -> upper-cased bases (pyfaidx's sequence_always_upper, util.py:84-88) on the host and up to the
    //         device -- on a thread of its own, beside PLAN: the RNG chain never looks at a base
    void ingest(uint8_t *d_in) {
        const auto a0 = Clock::now();
        parallel_slices(n, [&](int, int i0, int i1) {
            for (int i = i0; i < i1; i++) {
                const msim_batch_contig &q = contigs[i];
                uint8_t *dst = B.h_in.p + B.items[(size_t)i].base;
                uint64_t done = 0;
                const uint8_t *src = q.body;
                while (done < q.n_bases) {
                    const uint64_t take = std::min<uint64_t>(q.lenc, q.n_bases - done);
                    memcpy(dst + done, src, take);
                    done += take;
                    src += q.lenb;
                }
                for (uint64_t k = 0; k < q.n_bases; k++) {       // (auto-vectorised)
                    const uint8_t b = dst[k];
                    dst[k] = (uint8_t)(b - ((b >= 'a' && b <= 'z') ? 32 : 0));
                }
            }
        });
        ingest_ms = ms_between(a0, Clock::now());
        if (total) {
            ingest_err = hipSetDevice(c->device);
            if (ingest_err == hipSuccess) ingest_err = hipMemcpyAsync(d_in + PAD, B.h_in.p, total, hipMemcpyHostToDevice, c->stream);
        }
    }

    // ---- 2. PLAN: the RNG chain, contig by contig (mutator.py:111-131 + the draws of :334-358)
    int plan() {
        t_1 = Clock::now();
        for (int i = 0; i < n; i++) {                          // (kept for the framing, which runs when the text is asked for)
            Batch::Item &it = B.items[(size_t)i];
            it.header = contigs[i].header;
            it.header_len = contigs[i].header ? (contigs[i].header_len ? contigs[i].header_len : (uint32_t)strlen(contigs[i].header)) : 0u;
        }
        HostPlan hp;
        std::vector<msim_record> abs;                          // (locals in the record loop: this object is shared with the helper threads,
        bool snp = true;                                       //  and what they may see is reloaded and stored per record)
        for (int i = 0; i < n; i++) {
            const msim_batch_contig &q = contigs[i];
            Batch::Item &it = B.items[(size_t)i];
            const uint64_t w_py = c->py.words, w_np = c->np.words;
            const int rc = plan_contig_host(c, q.n_bases, q.ranges, q.n_ranges, hp);
            if (rc) return rc;
            c->t.contigs_batch++;
            c->t.py_words += c->py.words - w_py;
            c->t.np_words += c->np.words - w_np;
            it.empty = hp.empty;
            it.rec0 = B.recs_rel.size(); it.nrec = hp.recs.size();
            it.pool0 = B.pool.size(); it.npool = hp.pool.size();
            long long delta = 0;
            for (const msim_record &r : hp.recs) {
                delta += rec_delta(r);
                msim_record a = r;
                a.pos += (uint32_t)it.base;
                a.stop += (uint32_t)it.base;
                if (r.type == MSIM_IN) a.extra += (uint32_t)it.pool0;
                else if (r.type == MSIM_TLI) a.extra += (uint32_t)it.base;
                if (r.type != MSIM_SN) snp = false;
                abs.push_back(a);
            }
            B.recs_rel.insert(B.recs_rel.end(), hp.recs.begin(), hp.recs.end());
            B.pool.insert(B.pool.end(), hp.pool.begin(), hp.pool.end());
            it.out_start = (uint64_t)((long long)it.base + delta_total);
            it.out_len = (uint64_t)((long long)it.len + delta);
            delta_total += delta;
        }
        if (B.pool.size() >= (1ull << 31)) return fail(c, MSIM_ERR_UNSUPPORTED, "batch insert pool of 2 GiB or more: split it");
        out_total = (uint64_t)((long long)total + delta_total);
        recs_abs.swap(abs); all_snp = snp;
        t_2 = Clock::now();
        return MSIM_OK;
    }

    // ---- 3b. VCF record lines (mutator.py:334-399 + vcf_writer.py:118-126) per contig, on the host -- on a thread of its own,
    //          beside the APPLY: they read the records and the INPUT bases only.
    // Every slice of contigs renders into a buffer of its own, sized by a cheap upper bound (a line is name + fixed fields of
    // < 96 bytes + REF and ALT, each at most span + insert + 1 long, twice for a duplication's ALT); the slices are then joined
    // in contig order.
    void vcf_text() {
        const auto v0 = Clock::now();
        const msim_record *all = B.recs_rel.data();
        struct Part { char *buf = nullptr; uint64_t len = 0; int i0 = 0, i1 = 0; ~Part() { free(buf); } };   // buf: malloc'ed, never zero-filled
        std::vector<Part> parts((size_t)batch_threads());      // a slice's index rises with its contigs; unused ones stay empty
        std::atomic<bool> bad{false};
        parallel_slices(n, [&](int part, int i0, int i1) {
            uint64_t bound = 0;
            for (int i = i0; i < i1; i++) {
                const Batch::Item &it = B.items[(size_t)i];
                const uint64_t nl = (contigs[i].name_len ? contigs[i].name_len : strlen(contigs[i].name)) + 96;
                for (uint64_t k = 0; k < it.nrec; k++) {
                    const msim_record &r = all[it.rec0 + k];
                    const uint64_t span = r.type == MSIM_SN ? 1 : (uint64_t)(r.stop >= r.pos ? r.stop - r.pos + 1 : 0) + 2;
                    uint64_t writes, reads; rec_lengths(r, writes, reads);   // (a TLI writes the linked span and the base itself)
                    bound += nl + 3 * (span + (r.type == MSIM_TLI ? writes - 1 : 0)) + 8;
                }
            }
            Part &pt = parts[(size_t)part];
            char *out = pt.buf = static_cast<char *>(malloc((size_t)bound + 64));
            if (!out) { bad = true; return; }
            pt.i0 = i0; pt.i1 = i1;
            uint64_t at = 0;
            for (int i = i0; i < i1; i++) {
                Batch::Item &it = B.items[(size_t)i];
                it.vcf0 = at;                                  // relative to the slice until the join
                uint64_t need = 0;
                if (it.nrec) {
                    const std::string nm = contigs[i].name_len ? std::string(contigs[i].name, contigs[i].name_len) : std::string();
                    need = render_vcf_unchecked(all + it.rec0, it.nrec, B.pool.data() + it.pool0, B.h_in.p + it.base, it.len,
                                                contigs[i].name_len ? nm.c_str() : contigs[i].name, out + at);
                    if (at + need > bound) bad = true;
                }
                it.nvcf = need;
                at += need;
            }
            pt.len = at;
        });
        if (bad) { vcf_rc = MSIM_ERR_HIP; vcf_msg = "internal: VCF text of a batch: bound too small or out of memory"; return; }
        uint64_t total_vcf = 0;
        for (const Part &pt : parts) total_vcf += pt.len;
        file_channel_idle(c, 1);                              // (the previous batch's VCF text may still be on its way to the file)
        if (!B.vcf.reserve((size_t)total_vcf + 1)) { vcf_rc = MSIM_ERR_NOMEM; vcf_msg = "batch VCF text"; return; }
        uint64_t at = 0;
        for (const Part &pt : parts) {                         // the join, in contig order
            for (int i = pt.i0; i < pt.i1; i++) B.items[(size_t)i].vcf0 += at;
            if (pt.len) memcpy(B.vcf.p + at, pt.buf, (size_t)pt.len);
            at += pt.len;
        }
        B.vcf_len = (size_t)at;
        parts.clear();                                         // (the slices' release belongs to the phase's time)
        vcf_ms = ms_between(v0, Clock::now());
    }

    // ---- 3. ONE APPLY over the super-contig, the mutated bases down into h_out; the super-contig has left the context behind it
    int apply(SuperContig &super) {
        Contig *g = super.g;
        g->n_rec = recs_abs.size(); g->pool_len = B.pool.size();
        g->plan_empty = recs_abs.empty(); g->all_snp = all_snp;
        g->delta_known = true; g->known_delta = delta_total;
        int rc = upload_table(c, g, recs_abs.data(), B.pool.data());
        if (rc) return rc;
        rc = apply_contig_device(c, *g);
        if (rc) return rc;
        if (!B.h_out.reserve(out_total + 64)) return fail(c, MSIM_ERR_NOMEM, "batch staging buffer");
        if (out_total) MSIM_HIP(c, hipMemcpyAsync(B.h_out.p, g->d_out.p(), out_total, hipMemcpyDeviceToHost, c->emit_stream));
        rc = apply_finish(c);                                  // synchronises the emit stream: the copy above included
        if (rc) return rc;
        if (g->out_len != out_total) return fail(c, MSIM_ERR_HIP, "internal: batch planner and device disagree on the mutated length");
        if (g->key_error) {                                    // the reference's KeyError: which contig, which base
            const uint64_t kp = g->key_pos;
            int who = 0;
            for (int i = 0; i < n; i++) if (B.items[(size_t)i].base <= kp && kp < B.items[(size_t)i].base + B.items[(size_t)i].len) who = i;
            B.key_contig = who;
            const uint8_t kb = g->key_base;
            return fail(c, MSIM_ERR_KEY, std::string("KeyError: '") + (char)kb + "'");
        }
        super.drop();
        t_3 = Clock::now();
        return MSIM_OK;
    }

    // ---- 4. the FASTA text's layout; the framing itself runs when the text is asked for, straight into the caller's
    //         memory (msim_batch_fetch) or into a buffer of the context (batch_framed)
    void text_layout() {
        uint64_t text_total = 0;
        for (int i = 0; i < n; i++) {
            Batch::Item &it = B.items[(size_t)i];
            it.nl_before = i > 0 && B.items[(size_t)i - 1].bpl && B.items[(size_t)i - 1].out_len % B.items[(size_t)i - 1].bpl;
            const uint64_t head = it.header ? (it.nl_before ? 1 : 0) + 1 + it.header_len + 1 : 0;
            it.text0 = text_total;
            it.ntext = head + (it.bpl ? it.out_len + it.out_len / it.bpl : it.out_len);
            text_total += it.ntext;
        }
        B.fasta_len = (size_t)text_total;
        B.last_line_bases = B.items.back().bpl ? B.items.back().out_len % B.items.back().bpl : 0;
    }
};

// FASTA framing of a batch's mutated bases into `dst` (B.fasta_len bytes): '\n' after every bpl bases, none after a partial
// last line (fasta_writer.py:40-58).  With a header per contig the text is the complete run of FASTA records as FastaWriter
// would have written them: '>' header '\n' body, and a '\n' before a header iff the previous body ended in a partial line.
static void batch_frame_into(const Batch &B, uint8_t *out) {
    parallel_slices((int)B.items.size(), [&](int, int i0, int i1) {
        for (int i = i0; i < i1; i++) {
            const Batch::Item &it = B.items[(size_t)i];
            const uint8_t *src = B.h_out.p + it.out_start;
            uint8_t *dst = out + it.text0;
            if (it.header) {
                if (it.nl_before) *dst++ = '\n';
                *dst++ = '>';
                memcpy(dst, it.header, it.header_len);
                dst += it.header_len;
                *dst++ = '\n';
            }
            if (!it.bpl) { if (it.out_len) memcpy(dst, src, it.out_len); continue; }
            uint64_t done = 0;
            while (done + it.bpl <= it.out_len) { memcpy(dst, src + done, it.bpl); dst[it.bpl] = '\n'; dst += it.bpl + 1; done += it.bpl; }
            if (done < it.out_len) memcpy(dst, src + done, it.out_len - done);
        }
    });
}
// ... into the context's own buffer, once per batch (msim_batch_view, msim_batch_fetch_file)
static int batch_framed(Ctx *c, Batch &B) {
    if (B.framed) return MSIM_OK;
    file_channel_idle(c, 0);                               // (the previous batch's text may still be read from B.fasta)
    if (!B.fasta.reserve(B.fasta_len + 1)) return fail(c, MSIM_ERR_NOMEM, "batch FASTA text");
    if (B.fasta_len) batch_frame_into(B, B.fasta.p);
    B.framed = true;
    return MSIM_OK;
}

}  // namespace msim

using namespace msim;

extern "C" {

int msim_batch_run(msim_ctx *p, const msim_batch_contig *contigs, int n) {
    CTX_FLUSHED(c, p)
    if (!c || !contigs || n < 1) return MSIM_ERR_ARG;
    if (c->host_only) return fail(c, MSIM_ERR_HIP, "host-only context: this call needs the GPU");
    if (!c->have_params) return fail(c, MSIM_ERR_ARG, "msim_set_params has not been called");
    TraceRange tr("msim batch of small contigs");
    const auto t_0 = Clock::now();
    int rc = ctx_drain(c);
    if (rc) return rc;
    if (c->gpu) {                                          // the host planner continues from wherever the device streams stand
        rc = gpu_plan_sync_to_host(c, c->gpu);
        if (rc) return rc;
    }
    if (!c->batch) c->batch = new Batch();
    BatchRun R(c, *c->batch, contigs, n);
    if ((rc = R.lay_out())) return rc;
    if (!R.B.h_in.reserve(R.total + 64)) return fail(c, MSIM_ERR_NOMEM, "batch staging buffer");
    SuperContig super(c);
    if ((rc = super.make(R.total))) return rc;
    uint8_t *const d_in = super.g->d_in.p();
    rc = beside([&] { R.ingest(d_in); }, [&] { return R.plan(); });
    if (rc) return rc;
    if (R.ingest_err != hipSuccess) { super.drop(); return hip_fail(c, R.ingest_err, "batch input upload"); }
    rc = beside([&] { R.vcf_text(); }, [&] { const int arc = R.apply(super); if (!arc) R.text_layout(); return arc; });
    if (rc) return rc;
    if (R.vcf_rc) return fail(c, R.vcf_rc, R.vcf_msg);
    static const bool prof = getenv("MSIM_BATCH_PROF") != nullptr;
    if (prof)
        fprintf(stderr, "msim_batch_run: %d contigs, %.1f Mb in %.1f ms: plan %.1f (beside it: ingest %.1f), upload+APPLY+download %.1f (beside it: VCF %.1f), wait for VCF %.1f\n",
                n, R.total / 1e6, ms_between(t_0, Clock::now()), ms_between(R.t_1, R.t_2), R.ingest_ms, ms_between(R.t_2, R.t_3), R.vcf_ms,
                ms_between(R.t_3, Clock::now()));
    return MSIM_OK;
}

int msim_batch_sizes(msim_ctx *p, int n, uint64_t *fasta_bytes, uint64_t *vcf_bytes, int32_t *empty, uint64_t *n_records) {
    CTX_FLUSHED(c, p)
    if (!c || !c->batch || (size_t)n != c->batch->items.size()) return MSIM_ERR_ARG;
    for (int i = 0; i < n; i++) {
        const Batch::Item &it = c->batch->items[(size_t)i];
        if (fasta_bytes) fasta_bytes[i] = it.ntext;
        if (vcf_bytes) vcf_bytes[i] = it.nvcf;
        if (empty) empty[i] = it.empty ? 1 : 0;
        if (n_records) n_records[i] = it.nrec;
    }
    return MSIM_OK;
}

int msim_batch_fetch(msim_ctx *p, uint8_t *fasta_text, uint64_t fasta_cap, char *vcf_text, uint64_t vcf_cap) {
    CTX_FLUSHED(c, p)
    if (!c || !c->batch) return MSIM_ERR_ARG;
    Batch &B = *c->batch;
    if (fasta_text) {                                      // framed straight into the caller's memory (a mapped file, say)
        if (fasta_cap < B.fasta_len) return fail(c, MSIM_ERR_ARG, "fasta buffer too small");
        if (B.fasta_len && B.framed) memcpy(fasta_text, B.fasta.p, B.fasta_len);
        else if (B.fasta_len) batch_frame_into(B, fasta_text);
    }
    if (vcf_text) {
        if (vcf_cap < B.vcf_len) return fail(c, MSIM_ERR_ARG, "vcf buffer too small");
        if (B.vcf_len) memcpy(vcf_text, B.vcf.p, B.vcf_len);
    }
    return MSIM_OK;
}

int msim_batch_fetch_file(msim_ctx *p, int fasta_fd, uint64_t fasta_offset, int vcf_fd, uint64_t vcf_offset) {
    CTX_FLUSHED(c, p)
    if (!c || !c->batch) return MSIM_ERR_ARG;
    Batch &B = *c->batch;
    if (fasta_fd >= 0) {
        int rc = file_check(c, fasta_fd);
        if (rc) return rc;
        file_channel_idle(c, 0);                           // (whether or not the text is framed yet)
        if ((rc = batch_framed(c, B))) return rc;
        rc = file_enqueue_host(c, 0, B.fasta.p, B.fasta_len, fasta_fd, fasta_offset);
        if (rc) return rc;
    }
    if (vcf_fd >= 0) {
        int rc = file_check(c, vcf_fd);
        if (rc) return rc;
        rc = file_enqueue_host(c, 1, B.vcf.p, B.vcf_len, vcf_fd, vcf_offset);
        if (rc) return rc;
    }
    return MSIM_OK;
}

int msim_batch_view(msim_ctx *p, const uint8_t **fasta_text, uint64_t *fasta_bytes, const char **vcf_text, uint64_t *vcf_bytes,
                    uint64_t *last_line_bases) {
    CTX_FLUSHED(c, p)
    if (!c || !c->batch) return MSIM_ERR_ARG;
    Batch &B = *c->batch;
    if (fasta_text) {
        const int rc = batch_framed(c, B);
        if (rc) return rc;
        *fasta_text = B.fasta.p;
    }
    if (fasta_bytes) *fasta_bytes = B.fasta_len;
    if (vcf_text) *vcf_text = reinterpret_cast<const char *>(B.vcf.p);
    if (vcf_bytes) *vcf_bytes = B.vcf_len;
    if (last_line_bases) *last_line_bases = B.last_line_bases;
    return MSIM_OK;
}

int msim_batch_key_contig(msim_ctx *p, int *contig) {
    CTX_FLUSHED(c, p)
    if (!c || !contig || !c->batch) return MSIM_ERR_ARG;
    *contig = c->batch->key_contig;
    return MSIM_OK;
}

}  // extern "C"
