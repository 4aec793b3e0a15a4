// C-ABI entry points of libmsim.so (include/msim.h).  gfx950 (MI355X) only.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <thread>

#include <dlfcn.h>

#include "ctx.h"
#include "plan_gpu.h"

namespace msim {

static thread_local std::string g_create_error;

namespace {
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        for (const char *n : {"librocprofiler-sdk-roctx.so.1", "libroctx64.so.4", "libroctx64.so"}) {
            void *h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (!h) continue;
            *reinterpret_cast<void **>(&push) = dlsym(h, "roctxRangePushA");
            *reinterpret_cast<void **>(&pop) = dlsym(h, "roctxRangePop");
            if (push && pop) return;
            push = nullptr; pop = nullptr;
        }
    }
};
Roctx &roctx() { static Roctx r; return r; }
}  // namespace

TraceRange::TraceRange(const char *name) : on(false) {
    Roctx &r = roctx();
    if (r.push) { (void)r.push(name); on = true; }
}
TraceRange::~TraceRange() { if (on) (void)roctx().pop(); }

int fail(Ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}
int hip_fail(Ctx *c, hipError_t e, const char *what) {
    if (e == MSIM_WAIT_TIMED_OUT) {
        char buf[160];
        snprintf(buf, sizeof buf, ": no completion within %g s (MSIM_WAIT_TIMEOUT_S); the work it waits for is still queued or the device hangs",
                 wait_limit_seconds());
        return fail(c, MSIM_ERR_HIP, std::string(what) + buf);
    }
    return fail(c, MSIM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

double wait_limit_seconds() {
    const char *e = getenv("MSIM_WAIT_TIMEOUT_S");
    if (!e || !*e) return 120.0;
    const double v = atof(e);
    return v > 0 ? v : 0.0;
}

template <class Q>
static hipError_t wait_poll(Q &&query) {
    hipError_t e = query();
    if (e != hipErrorNotReady) return e;
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {                                             // spinning: what nearly every wait of a step ends in
        for (int i = 0; i < 16; i++) __builtin_ia32_pause();
        if ((e = query()) != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    const double limit = wait_limit_seconds();
    for (;;) {                                             // long waits (a file's last pieces, a first step's allocations): leave the core
        std::this_thread::sleep_for(std::chrono::microseconds(50));
        if ((e = query()) != hipErrorNotReady) return e;
        if (limit > 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit) return MSIM_WAIT_TIMED_OUT;
    }
}
hipError_t wait_stream(hipStream_t s) { return wait_poll([s]() { return hipStreamQuery(s); }); }
hipError_t wait_event(hipEvent_t ev) { return wait_poll([ev]() { return hipEventQuery(ev); }); }

struct CtxDev {            // small device-side constants owned by the ctx
    Scratch<uint8_t> d_lut;
};
static CtxDev *dev_of(Ctx *c);
uint8_t *ctx_lut(Ctx *c) { return dev_of(c)->d_lut.p(); }

// Everything enqueued has completed and its deferred results are collected: sampler flags + exact
// stream position, APPLY timings + KeyError words.  Returns the sampler's error, if any.
static int drain(Ctx *c);
int ctx_drain(Ctx *c) { return drain(c); }
static int drain(Ctx *c) {
    if (c->host_only) return MSIM_OK;
    TraceRange tr("msim drain (collect deferred results)");
    int rc = c->gpu ? gpu_plan_finish(c, c->gpu, true) : MSIM_OK;
    int rc2 = apply_finish(c);                             // (collects the counter-based engine's flags and sizes too)
    if (rc) return rc;
    if (rc2) return rc2;
    MSIM_HIP(c, wait_stream(c->stream));
    MSIM_HIP(c, wait_stream(c->emit_stream));
    return MSIM_OK;
}
// The APPLYs msim_apply_contig deferred.  only_groups (the engines' flush point at the start of a host walk): an incomplete group
// keeps waiting for its successors -- a full one goes out together through apply_batch_device.
static int defer_group_size() {
    static const int n = getenv("MSIM_NO_DEFER_PAIRS") ? 1 : getenv("MSIM_DEFER_GROUP") ? std::min(4, std::max(1, atoi(getenv("MSIM_DEFER_GROUP")))) : 3;
    return n;
}
bool deferred_apply_holds(const Ctx *c, int contig) {
    if (c->deferred_apply == contig) return contig >= 0;
    for (int q = 0; q < c->n_deferred_more; q++) if (c->deferred_more[q] == contig) return true;
    return false;
}
int flush_deferred_apply(Ctx *c, bool only_groups) {
    if (c->deferred_apply < 0) return MSIM_OK;
    if (only_groups && c->n_deferred_more + 1 < defer_group_size()) return MSIM_OK;
    std::vector<int> ids;
    for (int q = 0; q < c->n_deferred_more; q++) ids.push_back(c->deferred_more[q]);
    ids.push_back(c->deferred_apply);
    c->deferred_apply = -1;
    c->n_deferred_more = 0;
    ids.erase(std::remove_if(ids.begin(), ids.end(), [&](int idx) { return idx < 0 || idx >= (int)c->contigs.size(); }), ids.end());
    if (ids.size() >= 2) {
        for (int idx : ids) c->contigs[(size_t)idx].apply_stream = c->emit_stream;   // (apply_batch_device: contigs with a stream of their own)
        return apply_batch_device(c, ids, true);
    }
    for (int idx : ids) {
        const int rc = apply_contig_device(c, c->contigs[(size_t)idx]);
        if (rc) return rc;
    }
    return MSIM_OK;
}
int ctx_flush_queued(Ctx *c) {
    int rc = flush_deferred_apply(c);
    if (!rc && c->fast) rc = fast_plan_flush(c);           // (fast contexts: the plans queued so far, as one batch)
    if (!rc && c->gpu) rc = gpu_emit_flush(c);             // (SNP sampler: the emission group that is still waiting)
    return rc;
}
int ctx_device_contig(Ctx *c, int contig, bool need_planned, Contig **out) {
    int rc = ctx_flush_queued(c);
    if (rc) return rc;
    if (c->host_only) return fail(c, MSIM_ERR_HIP, "host-only context: this call needs the GPU");
    if (contig < 0 || (size_t)contig >= c->contigs.size()) return fail(c, MSIM_ERR_ARG, "no such contig");
    Contig &g = c->contigs[(size_t)contig];
    if (need_planned) {
        if (!g.planned) return fail(c, MSIM_ERR_ARG, "contig has not been planned");
        if ((rc = ctx_drain(c))) return rc;
    }
    *out = &g;
    return MSIM_OK;
}
int copy_floor(Ctx *c, const EventPair &tm, const CopySource *srcs, int n_srcs, double *ms) {
    *ms = 0;
    size_t total = 0;
    for (int i = 0; i < n_srcs; i++) total += srcs[i].bytes;
    if (!total) return MSIM_OK;
    const int rc = ensure_scratch(c, total);
    if (rc) return rc;
    MSIM_HIP(c, tm.begin(c->stream));
    uint8_t *dst = (uint8_t *)c->d_scratch.raw;
    for (int i = 0; i < n_srcs; dst += srcs[i++].bytes)
        if (srcs[i].bytes) MSIM_HIP(c, hipMemcpyAsync(dst, srcs[i].src, srcs[i].bytes, hipMemcpyDeviceToDevice, c->stream));
    MSIM_HIP(c, tm.end(c->stream));
    MSIM_HIP(c, wait_stream(c->stream));
    return tm.add_elapsed(c, ms);
}
static int key_error_of(Ctx *c, Contig &g) {
    g.key_reported = true;
    return fail(c, MSIM_ERR_KEY, std::string("KeyError: '") + (char)g.key_base + "'");
}

struct CtxFull : Ctx { CtxDev dev; };
static CtxDev *dev_of(Ctx *c) { return &static_cast<CtxFull *>(c)->dev; }

// Translation tables of mutator.py:75-77 and the transversion dict of mutator.py:449-455.
static void build_lut(uint8_t *lut) {
    uint8_t conv[256], comp[256], ti[256];
    for (int i = 0; i < 256; i++) conv[i] = comp[i] = ti[i] = (uint8_t)i;
    const char *a = "KSYMWRBDHV-", *b = "GCCAAACAAAN";
    for (int i = 0; a[i]; i++) conv[(uint8_t)a[i]] = (uint8_t)b[i];
    a = "ACGTUMRWSYKVHDB"; b = "TGCAAKYWSRMBDHV";
    for (int i = 0; a[i]; i++) comp[(uint8_t)a[i]] = (uint8_t)b[i];
    a = "AGTC"; b = "GACT";
    for (int i = 0; a[i]; i++) ti[(uint8_t)a[i]] = (uint8_t)b[i];
    for (int x = 0; x < 256; x++) {
        const uint8_t r = conv[x];
        lut[x] = ti[r];
        const char *pair = nullptr;
        switch (r) {
            case 'A': pair = "TC"; break;
            case 'G': pair = "CT"; break;
            case 'T': pair = "GA"; break;
            case 'C': pair = "AG"; break;
            case 'N': pair = "NN"; break;
            default: break;
        }
        lut[256 + x] = pair ? (uint8_t)pair[0] : 0;      // 0 -> the reference raises KeyError(r)
        lut[512 + x] = pair ? (uint8_t)pair[1] : 0;
        lut[768 + x] = r;
        lut[1024 + x] = comp[r];
    }
}

// forget a contig's plan/apply results; device buffers stay allocated for the next plan of this contig
static void reset_contig(Contig &g);
void contig_reset(Contig &g) { reset_contig(g); }
static void reset_contig(Contig &g) {   // (callers also drop the context's text cache: see text_kind)
    hap_forget(g);                                         // (a selected haplotype's table, the genotypes: gone with the plan)
    g.table_gen++;
    g.planned = g.applied = false;
    g.defer_apply = false;
    g.tile_index_by_plan = false;
    g.delta_known = false;
    g.off_ready = false;
    g.known_delta = 0;
    g.d_dyn = nullptr;
    g.sizes_pending = false;
    g.n_rec_cap = g.out_cap_len = g.n_struct_est = 0;
    g.n_rec = g.pool_len = g.out_len = 0;
    g.h_recs.clear(); g.h_recs.shrink_to_fit();
    g.h_pool.clear(); g.h_pool.shrink_to_fit();
}

int free_contig(Ctx *c, Contig &g, bool keep_input) {
    {
        const int rc = hap_free(c, g);
        if (rc) return rc;
    }
    MSIM_HIP(c, g.d_recs.release());
    MSIM_HIP(c, g.d_pool.release());
    MSIM_HIP(c, g.d_out.release());
    MSIM_HIP(c, g.d_off.release());
    MSIM_HIP(c, g.d_first.release());
    if (g.ea0) { (void)hipEventDestroy(g.ea0); (void)hipEventDestroy(g.ea1); (void)hipEventDestroy(g.ea2); g.ea0 = g.ea1 = g.ea2 = nullptr; }
    g.apply_pending = false;
    g.key_error = false;
    reset_contig(g);
    if (!keep_input) MSIM_HIP(c, g.d_in.release());
    return MSIM_OK;
}

static Contig *get_contig(Ctx *c, int id) {
    if (id < 0 || (size_t)id >= c->contigs.size()) { fail(c, MSIM_ERR_ARG, "no such contig"); return nullptr; }
    return &c->contigs[(size_t)id];
}

int new_contig(Ctx *c, uint64_t len, Contig **out) {
    if (len >= (1ull << 32)) return fail(c, MSIM_ERR_UNSUPPORTED, "contig of 4 GiB or more (multi-word getrandbits)");
    if (c->contigs.size() >= (size_t)MAX_CONTIGS) return fail(c, MSIM_ERR_UNSUPPORTED, "more than 65536 contigs in one context");
    Contig g;
    g.len = len;
    g.index = (int)c->contigs.size();
    if (!c->host_only) {
        // PAD bytes of zero slack on BOTH sides: shifted 16-B reads may start before / end after the data
        MSIM_HIP(c, dev_alloc(g.d_in, len + 2 * PAD));
        MSIM_HIP(c, hipMemsetAsync(g.d_in.p(), 0, PAD, c->stream));
        MSIM_HIP(c, hipMemsetAsync(g.d_in.p() + PAD + len, 0, PAD, c->stream));
    }
    c->contigs.push_back(std::move(g));
    *out = &c->contigs.back();
    return MSIM_OK;
}

// The device half of a table made on the host (install_host_table; the batch of small contigs, which leaves c->t.upload_ms alone)
int upload_table(Ctx *c, Contig *g, const msim_record *recs, const uint8_t *pool) {
    int rc = MSIM_OK;
    if (g->n_rec) {
        rc = dev_reserve(c, g->d_recs, g->n_rec * sizeof(msim_record));
        if (rc) return rc;
        MSIM_HIP(c, hipMemcpyAsync(g->d_recs.p(), recs, g->n_rec * sizeof(msim_record), hipMemcpyHostToDevice, c->stream));
    }
    rc = dev_reserve(c, g->d_pool, g->pool_len + 2 * PAD);
    if (rc) return rc;
    if (g->pool_len) MSIM_HIP(c, hipMemcpyAsync(g->d_pool.p() + PAD, pool, g->pool_len, hipMemcpyHostToDevice, c->stream));
    MSIM_HIP(c, wait_stream(c->stream));          // (the uploads read pageable vectors; APPLY runs on the emit stream)
    g->planned = true;
    return MSIM_OK;
}

}  // namespace msim

using namespace msim;

extern "C" {

int msim_abi_version(void) { return MSIM_ABI_VERSION; }

int msim_warm_up(int device_id) {
    if (device_id < 0) return MSIM_OK;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device_id >= n) return MSIM_ERR_HIP;
    if (hipSetDevice(device_id) != hipSuccess) return MSIM_ERR_HIP;
    return hipFree(nullptr) == hipSuccess ? MSIM_OK : MSIM_ERR_HIP;     // forces the runtime + device context up
}

int msim_device_host_cpus(int device_id, char *cpulist, int cap) {
    if (!cpulist || cap <= 0) return MSIM_ERR_ARG;
    cpulist[0] = 0;
    if (device_id < 0) return MSIM_OK;
    char buf[4096];
    device_host_cpus(device_id, buf, sizeof buf);
    snprintf(cpulist, (size_t)cap, "%s", buf);
    return MSIM_OK;
}

int msim_create(int device_id, uint32_t flags, msim_ctx **out) {
    if (!out) return MSIM_ERR_ARG;
    *out = nullptr;
    if (device_id == -1) {
        // Host-only context: the sequential planner and the text renderer work, every entry point
        // that needs the GPU fails with MSIM_ERR_HIP.  Exists so the planner can be checked against
        // the oracle on machines without a GPU; it cannot produce a mutated sequence.
        CtxFull *c = new (std::nothrow) CtxFull();
        if (!c) return MSIM_ERR_NOMEM;
        c->device = -1;
        c->host_only = true;
        c->flags = flags;
        c->devname = "host-only (no GPU)";
        c->py.init_genrand(5489u);
        c->np.init_genrand(5489u);
        for (int i = 0; i < 8; i++) c->params.block[i] = 1;
        c->params.ti_lim = (1ull << 52) + 1;
        *out = reinterpret_cast<msim_ctx *>(static_cast<Ctx *>(c));
        return MSIM_OK;
    }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(nullptr, MSIM_ERR_HIP, std::string("no HIP device available: ") + hipGetErrorString(e));
    if (device_id < 0 || device_id >= n) return fail(nullptr, MSIM_ERR_ARG, "device_id out of range");
    CtxFull *c = new (std::nothrow) CtxFull();
    if (!c) return MSIM_ERR_NOMEM;
    c->device = device_id;
    c->flags = flags;
    c->py.init_genrand(5489u);
    c->np.init_genrand(5489u);
    for (int i = 0; i < 8; i++) c->params.block[i] = 1;
    c->params.ti_lim = (1ull << 52) + 1;
    auto bail = [&](hipError_t he, const char *what) {
        int rc = hip_fail(nullptr, he, what);
        delete c;
        return rc;
    };
    if ((e = hipSetDevice(device_id)) != hipSuccess) return bail(e, "hipSetDevice");
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) return bail(e, "hipGetDeviceProperties");
    c->devname = std::string(prop.name) + " (" + prop.gcnArchName + ")";
    {   // the plan chain is the critical path of a step: give its stream the highest priority (and with it
        // a hardware queue of its own), so its small kernels are dispatched ahead of the bulk work that
        // runs beside it (jump cascade, chunk generation, record emission, rewrite)
        int lo = 0, hi = 0;
        if ((e = hipDeviceGetStreamPriorityRange(&lo, &hi)) != hipSuccess) return bail(e, "hipDeviceGetStreamPriorityRange");
        if ((e = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, hi)) != hipSuccess) return bail(e, "hipStreamCreate");
    }
    if ((e = hipStreamCreateWithFlags(&c->emit_stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
    hipEvent_t *evs[4] = {&c->ev0, &c->ev1, &c->ev2, &c->ev3};
    for (auto ev : evs)
        if ((e = hipEventCreate(ev)) != hipSuccess) return bail(e, "hipEventCreate");
    uint8_t lut[1280];
    build_lut(lut);
    if ((e = dev_alloc(c->dev.d_lut, sizeof lut)) != hipSuccess) return bail(e, "hipMalloc(lut)");
    if ((e = hipMemcpy(c->dev.d_lut.p(), lut, sizeof lut, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy(lut)");
    if ((e = dev_alloc(c->d_errs, (size_t)2 * MAX_CONTIGS * sizeof(unsigned long long))) != hipSuccess) return bail(e, "hipMalloc(errs)");   // KeyError words + length-check words
    if ((e = pin_alloc(c->h_mail, 64, hipHostMallocMapped)) != hipSuccess) return bail(e, "hipHostMalloc(mailbox)");
    c->gpu = gpu_plan_create();
    *out = reinterpret_cast<msim_ctx *>(static_cast<Ctx *>(c));
    return MSIM_OK;
}

static Ctx *C(msim_ctx *p) { return reinterpret_cast<Ctx *>(p); }
#define NEED_GPU(c) do { if ((c)->host_only) return fail((c), MSIM_ERR_HIP, "host-only context: this call needs the GPU"); } while (0)

void msim_destroy(msim_ctx *p) {
    if (!p) return;
    CtxFull *c = static_cast<CtxFull *>(C(p));
    c->deferred_apply = -1;                                // nobody will ask for their results
    c->n_deferred_more = 0;
    vcf_state_destroy(c);
    if (c->host_only) { file_io_destroy(c); batch_free(c); delete c; return; }
    static const bool prof = getenv("MSIM_BATCH_PROF") != nullptr;
    auto tp = std::chrono::steady_clock::now();
    double ph[6] = {0, 0, 0, 0, 0, 0};
    auto lap = [&](int i) { const auto n = std::chrono::steady_clock::now(); ph[i] += std::chrono::duration<double, std::milli>(n - tp).count(); tp = n; };
    (void)hipSetDevice(c->device);
    file_io_destroy(c);                                    // (finishes what is queued for the output files first)
    (void)wait_stream(c->stream);
    (void)wait_stream(c->emit_stream);
    lap(0);
    for (auto &g : c->contigs) (void)free_contig(c, g, false);
    (void)c->d_scratch.release();
    (void)c->dev.d_lut.release();
    (void)c->d_errs.release();
    (void)c->h_errs.release();
    (void)c->d_text.release();
    (void)c->d_text_scratch.release();
    lap(1);
    batch_free(c);
    lap(2);
    comm_destroy(c);
    spectrum_state_destroy(c);
    compare_state_destroy(c);
    reads_state_destroy(c);
    fast_plan_destroy(c);
    gpu_plan_destroy(c->gpu);
    lap(3);
    (void)c->h_mail.release();
    hipEvent_t evs[4] = {c->ev0, c->ev1, c->ev2, c->ev3};
    for (auto ev : evs) if (ev) (void)hipEventDestroy(ev);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->emit_stream) (void)hipStreamDestroy(c->emit_stream);
    lap(4);
    if (prof) fprintf(stderr, "msim_destroy: drain %.1f ms, contigs+scratch %.1f, batch buffers %.1f, plan engines %.1f, streams %.1f\n", ph[0], ph[1], ph[2], ph[3], ph[4]);
    delete c;
}

const char *msim_last_error(const msim_ctx *p) {
    if (!p) return g_create_error.c_str();
    return reinterpret_cast<const Ctx *>(p)->err.c_str();
}

int msim_device_name(const msim_ctx *p, char *dst, int cap) {
    if (!p || !dst || cap <= 0) return MSIM_ERR_ARG;
    snprintf(dst, (size_t)cap, "%s", reinterpret_cast<const Ctx *>(p)->devname.c_str());
    return MSIM_OK;
}

int msim_sync(msim_ctx *p) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    if (c->host_only) return MSIM_OK;
    int rc = drain(c);
    if (rc) return rc;
    for (auto &g : c->contigs)                             // deferred KeyError of an asynchronous APPLY
        if (g.key_error && !g.key_reported) return key_error_of(c, g);
    return file_wait(c);                                   // ... and what was queued for the output files is there
}

int msim_seed(msim_ctx *p, const uint32_t *py_key, int n_key, uint32_t np_seed) {
    CTX_FLUSHED(c, p)
    if (!c || !py_key || n_key < 1) return MSIM_ERR_ARG;
    {
        int rc = drain(c);
        if (rc) return rc;
    }
    c->py.init_by_array(py_key, n_key);
    c->py.words = 0;
    c->np.init_genrand(np_seed);
    c->np.words = 0;
    if (c->gpu) gpu_plan_invalidate(c->gpu);
    return MSIM_OK;
}

int msim_set_mt_state(msim_ctx *p, int stream, const uint32_t mt[624], int pos) {
    CTX_FLUSHED(c, p)
    if (!c || !mt || pos < 0 || pos > 624 || stream < 0 || stream > 1) return MSIM_ERR_ARG;
    if (c->gpu) {                      // keep the other stream's position before dropping the device copy
        int rc = gpu_plan_sync_to_host(c, c->gpu);
        if (rc) return rc;
    }
    HostMT &g = stream ? c->np : c->py;
    memcpy(g.mt, mt, sizeof g.mt);
    g.idx = pos;
    g.state_changed();
    if (c->gpu) gpu_plan_invalidate(c->gpu);
    return MSIM_OK;
}

int msim_get_mt_state(msim_ctx *p, int stream, uint32_t mt[624], int *pos) {
    CTX_FLUSHED(c, p)
    if (!c || !mt || !pos || stream < 0 || stream > 1) return MSIM_ERR_ARG;
    if (c->gpu) {
        int rc = gpu_plan_sync_to_host(c, c->gpu);
        if (rc) return rc;
    }
    HostMT &g = stream ? c->np : c->py;
    memcpy(mt, g.mt, sizeof g.mt);
    *pos = g.idx;
    return MSIM_OK;
}

int msim_reserve_streams(msim_ctx *p, uint64_t py_words, uint64_t np_words) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    if (c->gpu) gpu_plan_reserve(c->gpu, py_words, np_words);
    return MSIM_OK;
}

int msim_add_contig(msim_ctx *p, const uint8_t *bases, uint64_t len, int *contig) {
    CTX_FLUSHED(c, p)
    if (!c || (!bases && len) || !contig) return MSIM_ERR_ARG;
    Contig *g;
    int rc = new_contig(c, len, &g);
    if (rc) return rc;
    if (!c->host_only) {
        if (len) MSIM_HIP(c, hipMemcpyAsync(g->d_in.p() + PAD, bases, len, hipMemcpyHostToDevice, c->stream));
        MSIM_HIP(c, wait_stream(c->stream));
    }
    *contig = (int)c->contigs.size() - 1;
    return MSIM_OK;
}

int msim_add_contig_synthetic(msim_ctx *p, uint64_t len, uint64_t seed, int *contig) {
    CTX_FLUSHED(c, p)
    if (!c || !contig) return MSIM_ERR_ARG;
    NEED_GPU(c);
    Contig *g;
    int rc = new_contig(c, len, &g);
    if (rc) return rc;
    rc = synth_contig_device(c, g->d_in.p() + PAD, len, seed);
    if (rc) return rc;
    MSIM_HIP(c, wait_stream(c->stream));
    *contig = (int)c->contigs.size() - 1;
    return MSIM_OK;
}

int msim_contig_length(msim_ctx *p, int contig, uint64_t *len) {
    CTX_FLUSHED(c, p)
    if (!c || !len) return MSIM_ERR_ARG;
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    *len = g->len;
    return MSIM_OK;
}

int msim_read_contig(msim_ctx *p, int contig, uint64_t offset, uint64_t n, uint8_t *dst) {
    CTX_FLUSHED(c, p)
    if (!c || (!dst && n)) return MSIM_ERR_ARG;
    NEED_GPU(c);
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    if (offset > g->len || n > g->len - offset) return fail(c, MSIM_ERR_ARG, "read beyond contig end");
    if (n) MSIM_HIP(c, hipMemcpyAsync(dst, g->d_in.p() + PAD + offset, n, hipMemcpyDeviceToHost, c->stream));
    MSIM_HIP(c, wait_stream(c->stream));
    return MSIM_OK;
}

int msim_clear(msim_ctx *p) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    {
        int rc = drain(c);
        if (rc) return rc;
    }
    for (auto &g : c->contigs) {
        int rc = free_contig(c, g, false);
        if (rc) return rc;
    }
    c->contigs.clear();
    compare_drop_all(c);                                   // (held tables belong to contigs that are gone)
    reads_forget(c);
    c->text_kind = 0;
    return MSIM_OK;
}

int msim_set_params(msim_ctx *p, const msim_params *params) {
    CTX_FLUSHED(c, p)
    if (!c || !params) return MSIM_ERR_ARG;
    for (int t = 1; t <= 7; t++)
        if (params->block[t] < 1) return fail(c, MSIM_ERR_ARG, "block values must be >= 1 (rmt.py:326-345)");
    c->params = *params;
    c->have_params = true;
    return MSIM_OK;
}

int msim_set_plan_mode(msim_ctx *p, uint32_t mode) {
    CTX_FLUSHED(c, p)
    if (!c || (mode & ~(MSIM_PLAN_HOST | MSIM_PLAN_GPU)) || mode == (MSIM_PLAN_HOST | MSIM_PLAN_GPU)) return MSIM_ERR_ARG;
    if ((mode & MSIM_PLAN_GPU) && c->host_only) return fail(c, MSIM_ERR_HIP, "host-only context: no device engine to force");
    c->flags = (c->flags & ~(uint32_t)(MSIM_PLAN_HOST | MSIM_PLAN_GPU)) | mode;
    return MSIM_OK;
}

// A record table and insert pool made on the host become the contig's plan (the host planner's result; msim_dbg_set_records):
// kept on the host in a host-only context, uploaded otherwise.  APPLY then computes the output offsets on the device.
static int install_host_table(Ctx *c, Contig *g, std::vector<msim_record> &recs, std::vector<uint8_t> &pool, bool empty) {
    const auto t0 = std::chrono::steady_clock::now();
    g->n_rec = recs.size();
    g->pool_len = pool.size();
    g->plan_empty = empty;
    g->all_snp = true;
    for (const msim_record &r : recs)
        if (r.type != MSIM_SN) { g->all_snp = false; break; }
    if (c->host_only) {
        g->h_recs.swap(recs);
        g->h_pool.swap(pool);
        g->planned = true;
        return MSIM_OK;
    }
    const int rc = upload_table(c, g, recs.data(), pool.data());
    if (rc) return rc;
    c->t.upload_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return MSIM_OK;
}

// One iteration of mutate()'s contig loop up to the rewrite, for contig `g` (id `contig`; chain only: a length-only stand-in,
// id -1): picks the PLAN engine, keeps the streams chained.
static int plan_dispatch(Ctx *c, Contig *g, int contig, const msim_range *ranges, int n_ranges) {
    int rc = MSIM_OK;
    TraceRange tr(c->chain_only ? "msim PLAN contig (chain only)" : "msim PLAN contig");
    if (c->flags & MSIM_RNG_FAST) {                        // counter-based generator: nothing chains, nothing is stream-compatible
        const uint32_t seq = c->fast_seq++;
        // (a contig another rank owns: only its ordinal matters -- but what the reference refuses (ValueError) and what this
        //  mode does not cover is refused on every rank alike)
        if (c->chain_only) return fast_plan_check(c, g->len, ranges, n_ranges);
        if (c->host_only || !c->gpu) return fail(c, MSIM_ERR_HIP, "fast RNG mode needs the GPU");
        if ((rc = flush_deferred_apply(c))) return rc;
        if (g->apply_pending && (rc = apply_finish(c))) return rc;      // this contig's tables may still be read by its last APPLY
        reset_contig(*g);
        c->text_kind = 0;
        rc = plan_contig_fast(c, *g, ranges, n_ranges, c->fast_key, seq);
        if (!rc) c->t.contigs_fast++;
        return rc;
    }
    const bool dev = !c->host_only && c->gpu && !(c->flags & MSIM_PLAN_HOST);
    bool gpu_ok = dev && gpu_plan_eligible(c, ranges, n_ranges);
    bool mixed_ok = dev && !gpu_ok && gpu_plan_mixed_eligible(c, ranges, n_ranges);
    bool hs_ok = dev && !gpu_ok && !mixed_ok && gpu_plan_hostsample_eligible(c, ranges, n_ranges);
    bool mm_ok = dev && !gpu_ok && !mixed_ok && !hs_ok && gpu_plan_multimix_eligible(c, c->gpu, g->len, ranges, n_ranges);
    if (gpu_ok || mixed_ok || hs_ok || mm_ok) {            // the device streams' sessions span 1.31 G words: re-base where this contig
        bool fits = true;                                  // would not fit; a contig no span holds is the host planner's
        if ((rc = gpu_plan_make_room(c, c->gpu, ranges, n_ranges, &fits))) return rc;
        if (!fits) gpu_ok = mixed_ok = hs_ok = mm_ok = false;
    }
    // A deferred APPLY of the previous contig (msim_apply_contig) is enqueued when this plan's host chain starts --
    // by the engine itself -- so that it fills the device's idle time instead of competing with this contig's
    // latency-bound chain kernels.  Every other route enqueues it now.
    if (c->gpu && (!gpu_ok || gpu_emit_pending(c, contig, false)) && (rc = gpu_emit_flush(c))) return rc;   // (another engine / planned again)
    const bool host_chain = mixed_ok || hs_ok || mm_ok;
    const bool engine_flushes = host_chain && !deferred_apply_holds(c, contig);
    if (!engine_flushes && (rc = flush_deferred_apply(c))) return rc;
    reset_contig(*g);
    c->text_kind = 0;
    if ((c->flags & MSIM_PLAN_GPU) && !gpu_ok && !host_chain)
        return fail(c, MSIM_ERR_UNSUPPORTED, "GPU sampler not available for this stream structure");
    if (gpu_ok || host_chain) {
        if (gpu_ok) rc = plan_contig_gpu(c, c->gpu, *g, ranges, n_ranges);
        else {
            if (g->apply_pending && (mixed_ok || mm_ok)) {   // this contig's buffers may still be read by its last APPLY
                rc = apply_finish(c);
                if (rc) return rc;
            }
            if (mixed_ok) rc = plan_contig_gpu_mixed(c, c->gpu, *g, ranges, n_ranges);
            else if (hs_ok) rc = plan_contig_gpu_hostsample(c, c->gpu, *g, ranges, n_ranges);
            else rc = plan_contig_gpu_multimix(c, c->gpu, *g, ranges, n_ranges);
        }
        if (!rc && !c->chain_only)
            (gpu_ok ? c->t.contigs_snp : mixed_ok ? c->t.contigs_svmix : hs_ok ? c->t.contigs_hostcut : c->t.contigs_hostchain)++;
        // test hook: MSIM_DBG_FORCE_OVERFLOW=n raises the window-overflow flag behind the n-th device-planned contig of
        // the process (1-based), so that the callers' recovery (mutator.py: re-plan through the host planner) can be tested
        static const int force_at = getenv("MSIM_DBG_FORCE_OVERFLOW") ? atoi(getenv("MSIM_DBG_FORCE_OVERFLOW")) : 0;
        static int device_plans = 0;
        if (!rc && force_at && ++device_plans == force_at) rc = gpu_plan_force_overflow(c, c->gpu);
        if (rc == MSIM_ERR_HIP) gpu_plan_abandon(c->gpu);      // (a wait's deadline, a failed call: nothing of this session is known any more)
        const int frc = flush_deferred_apply(c, rc == MSIM_OK);   // (an engine that failed never reached its flush point; a single
                                                                   //  contig left waiting by design stays for its successor)
        g->defer_apply = !rc && host_chain && !c->chain_only;
        if (c->chain_only) g->planned = false;              // nothing to apply or fetch
        return rc ? rc : frc;
    }
    if (c->gpu) {                      // the host planner continues from wherever the device streams stand
        rc = gpu_plan_sync_to_host(c, c->gpu);
        if (rc) return rc;
    }
    if (!c->host_only) {               // this contig's buffers may still be read by an asynchronous APPLY
        rc = apply_finish(c);
        if (rc) return rc;
    }
    HostPlan hp;
    const uint64_t w_py = c->py.words, w_np = c->np.words;
    rc = plan_contig_host(c, g->len, ranges, n_ranges, hp);
    if (rc) return rc;
    c->t.py_words += c->py.words - w_py;
    c->t.np_words += c->np.words - w_np;
    if (c->chain_only) return MSIM_OK;                     // the streams have advanced: that is all
    c->t.contigs_host++;
    return install_host_table(c, g, hp.recs, hp.pool, hp.empty);
}

int msim_plan_contig(msim_ctx *p, int contig, const msim_range *ranges, int n_ranges) {
    Ctx *c = C(p);
    if (!c || n_ranges < 0 || (n_ranges && !ranges)) return MSIM_ERR_ARG;
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    if (!c->have_params) return fail(c, MSIM_ERR_ARG, "msim_set_params has not been called");
    return plan_dispatch(c, g, contig, ranges, n_ranges);
}

int msim_plan_chain(msim_ctx *p, uint64_t len, const msim_range *ranges, int n_ranges) {
    Ctx *c = C(p);
    if (!c || n_ranges < 0 || (n_ranges && !ranges)) return MSIM_ERR_ARG;
    if (!c->have_params) return fail(c, MSIM_ERR_ARG, "msim_set_params has not been called");
    if (len >= (1ull << 32)) return fail(c, MSIM_ERR_UNSUPPORTED, "contig of 4 GiB or more (multi-word getrandbits)");
    Contig stand_in;                                       // a length, nothing else: no bases, no tables
    stand_in.len = len;
    c->chain_only = true;
    const int rc = plan_dispatch(c, &stand_in, -1, ranges, n_ranges);
    c->chain_only = false;
    return rc;
}

// A pass in one call.  Every item goes through the per-contig entry points' own code, in order; in front of an item at which no
// hoisted sample is waiting, the sampler looks at the items from there on and sends ahead what it can (gpu_plan_pass_prep).
int msim_plan_pass(msim_ctx *p, const msim_pass_item *items, int n_items) {
    Ctx *c = C(p);
    if (!c || n_items < 0 || (n_items && !items)) return MSIM_ERR_ARG;
    const bool dev = !c->host_only && c->gpu && !(c->flags & (MSIM_PLAN_HOST | MSIM_RNG_FAST)) && c->have_params;
    for (int i = 0; i < n_items; i++) {
        const msim_pass_item &it = items[i];
        int rc = MSIM_OK;
        if (dev && !gpu_plan_pass_hoisting(c->gpu)) {
            // (contigs the context does not know end a segment like any item the sampler would not take: by failing at their turn)
            int n = 0;
            while (i + n < n_items && (items[i + n].contig < 0 || (size_t)items[i + n].contig < c->contigs.size())) n++;
            rc = gpu_plan_pass_prep(c, c->gpu, items + i, n);
        }
        if (!rc) rc = it.contig < 0 ? msim_plan_chain(p, it.len, it.ranges, it.n_ranges) : msim_plan_contig(p, it.contig, it.ranges, it.n_ranges);
        if (!rc && it.contig >= 0 && (it.flags & MSIM_PASS_APPLY)) rc = msim_apply_contig(p, it.contig);
        if (rc) {
            if (dev) gpu_plan_pass_abort(c, c->gpu);
            return rc;
        }
    }
    if (dev) gpu_plan_pass_abort(c, c->gpu);                // (nothing is left waiting behind a pass that ran through)
    return MSIM_OK;
}

int msim_dbg_pass_segments(const msim_params *params, const msim_pass_item *items, int n_items, uint64_t py_pos, uint64_t np_pos,
                           uint32_t max_chunks, int ahead, int32_t *seg) {
    if (!params || n_items < 0 || (n_items && (!items || !seg))) return MSIM_ERR_ARG;
    return gpu_dbg_pass_segments(params, items, n_items, py_pos, np_pos, max_chunks, ahead, seg);
}

int msim_plan_was_empty(msim_ctx *p, int contig, int *empty) {
    CTX_FLUSHED(c, p)
    if (!c || !empty) return MSIM_ERR_ARG;
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    if (!g->planned) return fail(c, MSIM_ERR_ARG, "contig has not been planned");
    if (g->sizes_pending) {                                // the counter-based engine decides on the device what survives
        const int rc = drain(c);
        if (rc) return rc;
    }
    *empty = g->plan_empty ? 1 : 0;
    return MSIM_OK;
}

int msim_apply_contig(msim_ctx *p, int contig) {
    Ctx *c = C(p);
    if (!c) return MSIM_ERR_ARG;
    // fast contexts: a contig whose plan is still queued gets its APPLY enqueued right behind the batch (plan_fast.hip)
    if (c->fast && fast_plan_queued(c, contig, true)) return MSIM_OK;
    // SNP sampler: a contig whose emission still waits for its group is applied right behind that group (plan_gpu.hip)
    if (c->gpu && gpu_emit_pending(c, contig, true)) return MSIM_OK;
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    static const bool no_defer = getenv("MSIM_NO_DEFER") != nullptr;
    const bool defer = g->planned && g->defer_apply && !no_defer && !c->host_only;
    {   // (a contig that will wait itself pairs up with the one already waiting; anything else sends what waits first)
        int rc = (defer && c->n_deferred_more + 1 < defer_group_size() && !deferred_apply_holds(c, contig)) ? MSIM_OK : flush_deferred_apply(c);
        if (!rc && c->fast) rc = fast_plan_flush(c);
        if (rc) return rc;
    }
    NEED_GPU(c);
    if (!g->planned) return fail(c, MSIM_ERR_ARG, "msim_apply_contig before msim_plan_contig");
    TraceRange tr("msim APPLY contig");
    c->text_kind = 0;
    // Contigs of the engines with a host chain: the next contig's plan starts with latency-bound device kernels and
    // then leaves the device idle for a millisecond while the host walks -- that is where this APPLY belongs.  It is
    // enqueued by the next entry point, whichever it is (the next plan at the start of its host chain).
    if (defer) {
        if (c->deferred_apply >= 0) c->deferred_more[c->n_deferred_more++] = c->deferred_apply;   // (the group this one joins)
        c->deferred_apply = contig;
        return MSIM_OK;
    }
    return apply_contig_device(c, *g);
}

int msim_key_error(msim_ctx *p, int contig, uint8_t *base, uint64_t *pos) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    Contig *g = nullptr;
    if (contig == -1) {                                    // first contig that hit it
        for (auto &q : c->contigs) if (q.key_error) { g = &q; break; }
        if (!g) return fail(c, MSIM_ERR_ARG, "no KeyError recorded");
    } else {
        g = get_contig(c, contig);
        if (!g) return MSIM_ERR_ARG;
    }
    if (!g->key_error) return fail(c, MSIM_ERR_ARG, "no KeyError recorded for this contig");
    if (base) *base = g->key_base;
    if (pos) *pos = g->key_pos;
    return MSIM_OK;
}

int msim_result_sizes(msim_ctx *p, int contig, uint64_t *out_len, uint64_t *n_records, uint64_t *pool_len) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    if (!g->planned) return fail(c, MSIM_ERR_ARG, "contig has not been planned");
    if (g->sizes_pending) {
        const int rc = drain(c);
        if (rc) return rc;
    }
    if (out_len) {
        if (!g->applied) return fail(c, MSIM_ERR_ARG, "contig has not been applied");
        int rc = drain(c);
        if (rc) return rc;
        if (g->key_error) return key_error_of(c, *g);
        *out_len = g->out_len;
    }
    if (n_records) *n_records = g->n_rec;
    if (pool_len) *pool_len = g->pool_len;
    return MSIM_OK;
}

int msim_fetch_sequence(msim_ctx *p, int contig, uint64_t offset, uint64_t n, uint8_t *dst) {
    CTX_FLUSHED(c, p)
    if (!c || (!dst && n)) return MSIM_ERR_ARG;
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    if (!g->applied) return fail(c, MSIM_ERR_ARG, "contig has not been applied");
    {
        int rc = drain(c);
        if (rc) return rc;
        if (g->key_error) return key_error_of(c, *g);
    }
    if (offset > g->out_len || n > g->out_len - offset) return fail(c, MSIM_ERR_ARG, "fetch beyond mutated contig end");
    if (n) MSIM_HIP(c, hipMemcpyAsync(dst, g->d_out.p() + offset, n, hipMemcpyDeviceToHost, c->stream));
    MSIM_HIP(c, wait_stream(c->stream));
    return MSIM_OK;
}

int msim_fetch_records(msim_ctx *p, int contig, msim_record *dst, uint8_t *pool_dst) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    if (!g->planned) return fail(c, MSIM_ERR_ARG, "contig has not been planned");
    if (c->host_only) {
        if (dst && g->n_rec) memcpy(dst, g->h_recs.data(), g->n_rec * sizeof(msim_record));
        if (pool_dst && g->pool_len) memcpy(pool_dst, g->h_pool.data(), g->pool_len);
        return MSIM_OK;
    }
    {
        int rc = drain(c);
        if (rc) return rc;
    }
    if (dst && g->n_rec)
        MSIM_HIP(c, hipMemcpyAsync(dst, g->d_recs.p(), g->n_rec * sizeof(msim_record), hipMemcpyDeviceToHost, c->stream));
    if (pool_dst && g->pool_len)
        MSIM_HIP(c, hipMemcpyAsync(pool_dst, g->d_pool.p() + PAD, g->pool_len, hipMemcpyDeviceToHost, c->stream));
    MSIM_HIP(c, wait_stream(c->stream));
    return MSIM_OK;
}

int msim_result_checksum(msim_ctx *p, int contig, uint64_t *sum) {
    CTX_FLUSHED(c, p)
    if (!c || !sum) return MSIM_ERR_ARG;
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    if (!g->applied) return fail(c, MSIM_ERR_ARG, "contig has not been applied");
    {
        int rc = drain(c);
        if (rc) return rc;
        if (g->key_error) return key_error_of(c, *g);
    }
    return checksum_device(c, g->d_out.p(), g->out_len, sum);
}

int msim_result_device_ptr(msim_ctx *p, int contig, uint64_t *device_address, uint64_t *len) {
    CTX_FLUSHED(c, p)
    if (!c || !device_address || !len) return MSIM_ERR_ARG;
    NEED_GPU(c);
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    if (!g->applied) return fail(c, MSIM_ERR_ARG, "contig has not been applied");
    int rc = drain(c);
    if (rc) return rc;
    if (g->key_error) return key_error_of(c, *g);
    *device_address = (uint64_t)(uintptr_t)g->d_out.p();
    *len = g->out_len;
    return MSIM_OK;
}

int msim_planned_out_len(msim_ctx *p, int contig, uint64_t *out_len, int *known) {
    CTX_FLUSHED(c, p)
    if (!c || !out_len || !known) return MSIM_ERR_ARG;
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    *known = 0;
    *out_len = 0;
    if (!g->planned) return MSIM_OK;                       // (a contig this rank only walked the chain for: its owner knows)
    if (g->sizes_pending && !g->all_snp) return MSIM_OK;   // (decided on the device, not collected yet)
    if (g->all_snp || g->n_rec == 0) { *known = 1; *out_len = g->len; }
    else if (g->delta_known) { *known = 1; *out_len = (uint64_t)((long long)g->len + g->known_delta); }
    return MSIM_OK;
}

int msim_release_result(msim_ctx *p, int contig) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    {
        int rc = drain(c);
        if (rc) return rc;
    }
    return free_contig(c, *g, true);
}

// ---- diploid runs: genotypes beside the record table, one haplotype's records as the active table (haplotype.hip) --------
static int genotyped_contig(Ctx *c, int contig, bool need_gt, Contig **out) {
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    if (!g->planned) return fail(c, MSIM_ERR_ARG, "contig has not been planned");
    if (need_gt && !g->have_gt) return fail(c, MSIM_ERR_ARG, "contig has no genotypes (msim_genotype_contig / msim_set_genotypes)");
    const int rc = drain(c);                               // the table is complete, its sizes are collected, nothing reads it
    if (rc) return rc;
    c->text_kind = 0;
    *out = g;
    return MSIM_OK;
}

int msim_genotype_contig(msim_ctx *p, int contig, uint64_t key, uint32_t seq, uint64_t het_thr) {
    CTX_FLUSHED(c, p)
    if (!c || het_thr > (1ull << 53)) return MSIM_ERR_ARG;
    Contig *g;
    const int rc = genotyped_contig(c, contig, false, &g);
    if (rc) return rc;
    TraceRange tr("msim genotype draw");
    return hap_genotype(c, *g, key, seq, het_thr);
}

int msim_set_genotypes(msim_ctx *p, int contig, const uint8_t *gt) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    Contig *g;
    const int rc = genotyped_contig(c, contig, false, &g);
    if (rc) return rc;
    if (!gt && (g->hap ? g->full.n_rec : g->n_rec)) return MSIM_ERR_ARG;
    return hap_set_genotypes(c, *g, gt);
}

int msim_fetch_genotypes(msim_ctx *p, int contig, uint8_t *dst) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    Contig *g;
    const int rc = genotyped_contig(c, contig, true, &g);
    if (rc) return rc;
    if (!dst && (g->hap ? g->full.n_rec : g->n_rec)) return MSIM_ERR_ARG;
    return hap_fetch_genotypes(c, *g, dst);
}

// Ordering of a diploid run's second haplotype against its first.  The compacted table, d_off, the tile index and d_out are the
// contig's own buffers, and the second haplotype's selection and APPLY write all of them again.  Who may still read them?
//   - the first haplotype's APPLY (tile index, rewrite: the contig's apply stream) reads the table and d_off and writes d_out;
//   - its FASTA text: k_frame reads d_out on the context's stream and writes a buffer of the FASTA output channel; what the
//     channel has in flight afterwards -- up to two transfers, device -> pinned ring -> file on the channel's own stream --
//     reads THAT buffer, never d_out (file_io.hip: file_enqueue records its event behind k_frame and returns);
//   - its liftover chain: kernels on the context's stream over the table, waited for inside the call.
// genotyped_contig() drains the context before anything is selected: apply_finish waits for every APPLY in flight on whichever
// stream it runs, then the context's stream and the emit stream are waited for -- k_frame has read the last byte of d_out, and
// the channel's queued transfers own their bytes.  So the selection needs no event of its own, and none of the queued
// transfers has to finish first: the second haplotype's APPLY overlaps the first one's way to its file.
int msim_select_haplotype(msim_ctx *p, int contig, int hap) {
    CTX_FLUSHED(c, p)
    if (!c || hap < 0 || hap > 2) return MSIM_ERR_ARG;
    Contig *g;
    const int rc = genotyped_contig(c, contig, hap != 0, &g);
    if (rc) return rc;
    TraceRange tr("msim select haplotype");
    return hap_select(c, *g, hap);
}

// test support: records of a workgroup of the compaction kernels
uint32_t msim_dbg_hap_block(void) { return hap_block(); }

// ---- text on the device -------------------------------------------------
static int text_copy_out(Ctx *c, uint8_t *out, uint64_t cap, uint64_t *needed) {
    *needed = c->text_len;
    if (!out) return MSIM_OK;
    if (cap < c->text_len) return fail(c, MSIM_ERR_ARG, "text buffer too small (see *needed)");
    if (c->text_len) MSIM_HIP(c, hipMemcpyAsync(out, c->d_text.p(), c->text_len, hipMemcpyDeviceToHost, c->stream));
    MSIM_HIP(c, wait_stream(c->stream));
    return MSIM_OK;
}

// render (unless the preceding size call left the text in d_text)
static int vcf_text_ready(Ctx *c, int contig, const char *seq_name, bool reuse) {
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    if (!g->planned) return fail(c, MSIM_ERR_ARG, "contig has not been planned");
    if (reuse && c->text_kind == 1 && c->text_contig == contig) return MSIM_OK;
    int rc = drain(c);                                                   // record aux bytes come from the emit stream
    if (rc) return rc;
    c->text_kind = 0;
    uint64_t bytes = 0;
    rc = vcf_render_device(c, *g, seq_name, &bytes);
    if (rc) return rc;
    c->text_kind = 1;
    c->text_contig = contig;
    return MSIM_OK;
}

static int framed_text_ready(Ctx *c, int contig, uint32_t bpl, bool reuse) {
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    if (!g->applied) return fail(c, MSIM_ERR_ARG, "contig has not been applied");
    if (reuse && c->text_kind == 2 && c->text_contig == contig && c->text_bpl == bpl) return MSIM_OK;
    int rc = drain(c);
    if (rc) return rc;
    if (g->key_error) return key_error_of(c, *g);
    c->text_kind = 0;
    uint64_t bytes = 0;
    rc = fasta_frame_device(c, *g, bpl, &bytes);
    if (rc) return rc;
    c->text_kind = 2;
    c->text_contig = contig;
    c->text_bpl = bpl;
    return MSIM_OK;
}

int msim_render_vcf_device(msim_ctx *p, int contig, const char *seq_name, char *out, uint64_t cap, uint64_t *needed) {
    CTX_FLUSHED(c, p)
    if (!c || !seq_name || !needed) return MSIM_ERR_ARG;
    NEED_GPU(c);
    TraceRange tr("msim text: VCF lines");
    int rc = vcf_text_ready(c, contig, seq_name, out != nullptr);        // (a size call always renders)
    if (rc) return rc;
    return text_copy_out(c, reinterpret_cast<uint8_t *>(out), cap, needed);
}

// The contig's liftover chain, rendered from its record table (text_gpu.hip: chain_render_device).  Planned is enough: the
// table is the whole input.  Names are part of the text, so a copy call whose names or id differ renders again.
int msim_render_chain_device(msim_ctx *p, int contig, const char *t_name, const char *q_name, uint64_t id, char *out, uint64_t cap,
                             uint64_t *needed) {
    CTX_FLUSHED(c, p)
    if (!c || !t_name || !q_name || !needed) return MSIM_ERR_ARG;
    NEED_GPU(c);
    TraceRange tr("msim text: liftover chain");
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    if (!g->planned) return fail(c, MSIM_ERR_ARG, "contig has not been planned");
    const std::string names = std::string(t_name) + '\n' + q_name;
    if (!(out && c->text_kind == 3 && c->text_contig == contig && c->text_chain_id == id && c->text_chain_names == names)) {
        int rc = drain(c);                                               // the table's last bytes come from the emit stream
        if (rc) return rc;
        c->text_kind = 0;
        rc = chain_render_device(c, *g, t_name, q_name, id, c->chain_kernel_ms >= 0 ? &c->chain_kernel_ms : nullptr);
        if (rc) return rc;
        c->text_kind = 3;
        c->text_contig = contig;
        c->text_chain_id = id;
        c->text_chain_names = names;
    }
    return text_copy_out(c, reinterpret_cast<uint8_t *>(out), cap, needed);
}

// test / measurement support: the chain kernels' device time (HIP events around every run of launches) of the last
// msim_render_chain_device rendering; the first call switches the measurement on (*ms = 0 then).
int msim_dbg_chain_ms(msim_ctx *p, double *ms) {
    CTX_FLUSHED(c, p)
    if (!c || !ms) return MSIM_ERR_ARG;
    if (c->chain_kernel_ms < 0) c->chain_kernel_ms = 0;
    *ms = c->chain_kernel_ms;
    return MSIM_OK;
}

// test support: the chain kernels' tile (records / gaps of a workgroup), where their edge cases lie
uint32_t msim_dbg_chain_tile(void) { return chain_tile(); }

int msim_fetch_sequence_framed(msim_ctx *p, int contig, uint32_t bpl, uint8_t *out, uint64_t cap, uint64_t *needed) {
    CTX_FLUSHED(c, p)
    if (!c || !needed || bpl == 0) return MSIM_ERR_ARG;
    NEED_GPU(c);
    TraceRange tr("msim text: framed FASTA");
    int rc = framed_text_ready(c, contig, bpl, out != nullptr);
    if (rc) return rc;
    return text_copy_out(c, out, cap, needed);
}

// The two texts queued for an output file (file_io.hip).  Rendering runs on the context's stream into a buffer of the output
// channel; the channel's thread copies and writes it while the caller goes on.
int msim_render_vcf_device_file(msim_ctx *p, int contig, const char *seq_name, int fd, uint64_t offset, uint64_t *written) {
    CTX_FLUSHED(c, p)
    if (!c || !seq_name || !written || fd < 0) return MSIM_ERR_ARG;
    NEED_GPU(c);
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    if (!g->planned) return fail(c, MSIM_ERR_ARG, "contig has not been planned");
    TraceRange tr("msim text: VCF lines -> file");
    int rc = file_check(c, fd);
    if (rc) return rc;
    rc = drain(c);                                                       // record aux bytes come from the emit stream
    if (rc) return rc;
    int slot;
    DevBlock *buf;
    rc = file_text_buffer(c, 1, &slot, &buf);
    if (rc) return rc;
    uint64_t bytes = 0;
    rc = vcf_render_device(c, *g, seq_name, &bytes, buf);
    if (rc) return rc;
    *written = bytes;
    return file_enqueue(c, 1, slot, bytes, fd, offset);
}

int msim_fetch_sequence_framed_file(msim_ctx *p, int contig, uint32_t bpl, int fd, uint64_t offset, uint64_t *written) {
    CTX_FLUSHED(c, p)
    if (!c || !written || bpl == 0 || fd < 0) return MSIM_ERR_ARG;
    NEED_GPU(c);
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    if (!g->applied) return fail(c, MSIM_ERR_ARG, "contig has not been applied");
    TraceRange tr("msim text: framed FASTA -> file");
    int rc = file_check(c, fd);
    if (rc) return rc;
    rc = drain(c);
    if (rc) return rc;
    if (g->key_error) return key_error_of(c, *g);
    int slot;
    DevBlock *buf;
    rc = file_text_buffer(c, 0, &slot, &buf);
    if (rc) return rc;
    uint64_t bytes = 0;
    rc = fasta_frame_device(c, *g, bpl, &bytes, buf);
    if (rc) return rc;
    *written = bytes;
    return file_enqueue(c, 0, slot, bytes, fd, offset);
}

int msim_file_wait(msim_ctx *p) {
    Ctx *c = C(p);
    if (!c) return MSIM_ERR_ARG;
    return file_wait(c);
}

// BGZF output (bgzf.hip, file_io.hip): the output channels compress what they write.
int msim_bgzf_open(msim_ctx *p, int channel, int fd) {
    Ctx *c = C(p);
    if (!c || channel < 0 || channel > 1 || fd < 0) return MSIM_ERR_ARG;
    NEED_GPU(c);
    return file_bgzf_open(c, channel, fd);
}

int msim_bgzf_append(msim_ctx *p, int channel, const uint8_t *bytes, uint64_t n) {
    Ctx *c = C(p);
    if (!c || channel < 0 || channel > 1 || (!bytes && n)) return MSIM_ERR_ARG;
    NEED_GPU(c);
    return file_bgzf_append(c, channel, bytes, n);
}

int msim_bgzf_close(msim_ctx *p, int channel, uint64_t *compressed, uint64_t *uncompressed) {
    Ctx *c = C(p);
    if (!c || channel < 0 || channel > 1) return MSIM_ERR_ARG;
    NEED_GPU(c);
    return file_bgzf_close(c, channel, compressed, uncompressed);
}

uint64_t msim_bgzf_bound(uint64_t n) { return bgzf_bound(n); }

int msim_bgzf_compress(msim_ctx *p, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *written,
                       float *device_ms) {
    Ctx *c = C(p);
    if (!c || (!in && n) || !out || !written) return MSIM_ERR_ARG;
    NEED_GPU(c);
    TraceRange tr("msim bgzf: one-shot");
    return bgzf_compress_host(c, in, n, out, cap, written, device_ms);
}

// BGZF input: the member chain on the host, the members' deflate data on the device (bgzf.hip: k_bgzf_inflate).
int msim_bgzf_probe(const uint8_t *in, uint64_t n, uint64_t *uncompressed, uint64_t *members) {
    if (!in && n) return MSIM_ERR_ARG;
    return bgzf_probe_host(in, n, uncompressed, members);
}

int msim_bgzf_inflate(msim_ctx *p, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *written,
                      float *device_ms) {
    Ctx *c = C(p);
    if (!c || (!in && n) || (!out && cap) || !written) return MSIM_ERR_ARG;
    NEED_GPU(c);
    TraceRange tr("msim bgzf: inflate");
    return bgzf_inflate_host(c, in, n, out, cap, written, device_ms);
}

int msim_add_contig_text(msim_ctx *p, const uint8_t *body, uint64_t body_bytes, uint64_t n_bases, uint32_t lenc,
                         uint32_t lenb, int *contig) {
    CTX_FLUSHED(c, p)
    if (!c || !contig || (!body && n_bases)) return MSIM_ERR_ARG;
    NEED_GPU(c);
    if (n_bases) {
        if (lenc == 0 || lenb < lenc) return fail(c, MSIM_ERR_ARG, "line width / line stride of the FASTA body are inconsistent");
        const uint64_t last = (n_bases - 1) / lenc * lenb + (n_bases - 1) % lenc;    // offset of the last base
        if (last >= body_bytes) return fail(c, MSIM_ERR_ARG, "FASTA body shorter than n_bases at this line width");
    }
    TraceRange tr("msim text: FASTA ingest");
    Contig *g;
    int rc = new_contig(c, n_bases, &g);
    if (rc) return rc;
    c->text_kind = 0;                                                    // the staging buffer is about to be reused
    rc = fasta_gather_device(c, body, body_bytes, n_bases, lenc, lenb, g->d_in.p() + PAD);
    if (rc) return rc;
    *contig = (int)c->contigs.size() - 1;
    return MSIM_OK;
}

int msim_set_fast_key(msim_ctx *p, uint64_t key) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    c->fast_key = key;
    c->fast_seq = 0;
    return MSIM_OK;
}

int msim_sample_min_distance(msim_ctx *p, int64_t start, int64_t stop, int64_t k, int64_t d, int64_t setsize, int64_t *out) {
    CTX_FLUSHED(c, p)
    if (!c || (!out && k > 0)) return MSIM_ERR_ARG;
    if (!c->host_only) {
        int rc = drain(c);
        if (rc) return rc;
        if (c->gpu && (rc = gpu_plan_sync_to_host(c, c->gpu))) return rc;      // continue from wherever the device streams stand
    }
    const uint64_t w0 = c->py.words;
    const int rc = sample_min_distance_host(c, start, stop, k, d, setsize, out);
    c->t.py_words += c->py.words - w0;
    return rc;
}

int msim_splice_contigs(msim_ctx *p, int a, int b, uint64_t n_bp, const uint64_t *bp_a, const uint64_t *bp_b, int *contig) {
    CTX_FLUSHED(c, p)
    if (!c || !contig || (n_bp && (!bp_a || !bp_b))) return MSIM_ERR_ARG;
    NEED_GPU(c);
    if (!get_contig(c, a) || (n_bp && !get_contig(c, b))) return MSIM_ERR_ARG;
    TraceRange tr("msim IT: splice two contigs");
    const uint64_t len_a = c->contigs[(size_t)a].len, len_b = n_bp ? c->contigs[(size_t)b].len : 0;
    if (n_bp >= (1ull << 31)) return fail(c, MSIM_ERR_UNSUPPORTED, "2^31 breakpoints or more");
    // segment i = [bp[i-1], bp[i]) of its contig, bp[-1] = 0, bp[n_bp] = the contig's length; even i from a, odd i from b
    const uint32_t n_seg = (uint32_t)n_bp + 1;
    std::vector<uint32_t> seg_out((size_t)n_seg + 1), seg_src(n_seg);
    uint64_t out = 0, pa = 0, pb = 0;
    for (uint32_t i = 0; i < n_seg; i++) {
        const uint64_t ea = i < n_bp ? bp_a[i] : len_a, eb = i < n_bp ? bp_b[i] : len_b;
        if (ea < pa || ea > len_a || (n_bp && (eb < pb || eb > len_b)))
            return fail(c, MSIM_ERR_ARG, "breakpoints must ascend and lie inside their contig");
        seg_out[i] = (uint32_t)out;
        seg_src[i] = (uint32_t)((i & 1u) ? pb : pa);
        out += (i & 1u) ? eb - pb : ea - pa;
        if (out >= (1ull << 32)) return fail(c, MSIM_ERR_UNSUPPORTED, "spliced contig of 4 GiB or more");
        pa = ea;
        pb = eb;
    }
    seg_out[n_seg] = (uint32_t)out;
    int rc = drain(c);
    if (rc) return rc;
    Contig *g;
    rc = new_contig(c, 0, &g);                             // (no input of its own: the result is its mutated stream)
    if (rc) return rc;
    const Contig &ga = c->contigs[(size_t)a];              // (after new_contig: the vector may have moved)
    const Contig *gb = n_bp ? &c->contigs[(size_t)b] : nullptr;
    c->text_kind = 0;
    rc = splice_device(c, ga, gb, seg_out.data(), seg_src.data(), n_seg, *g);
    if (rc) { (void)free_contig(c, *g, false); c->contigs.pop_back(); return rc; }
    g->planned = true;
    g->plan_empty = true;
    g->applied = true;
    *contig = (int)c->contigs.size() - 1;
    return MSIM_OK;
}

int msim_host_alloc(msim_ctx *p, uint64_t bytes, void **ptr) {
    Ctx *c = C(p);
    if (!c || !ptr) return MSIM_ERR_ARG;
    NEED_GPU(c);
    *ptr = nullptr;
    MSIM_HIP(c, hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault));
    return MSIM_OK;
}

int msim_host_free(msim_ctx *p, void *ptr) {
    Ctx *c = C(p);
    if (!c) return MSIM_ERR_ARG;
    NEED_GPU(c);
    if (ptr) MSIM_HIP(c, hipHostFree(ptr));
    return MSIM_OK;
}

// ---- test hooks: NOT part of the ABI (absent from include/msim.h).  They expose the two host-side chains of the
// device PLAN engines (plan_host.cpp) so that the CPU test tier can pin them against CPython's own random.sample /
// random.randint and run them under ASan/UBSan without a GPU (tests/test_cabi_host.py).
int msim_dbg_sample_ranges(msim_ctx *p, const msim_range *ranges, int n_ranges, const uint32_t *words, uint64_t n_words,
                           uint32_t *pos_out, uint64_t *consumed) {
    CTX_FLUSHED(c, p)
    if (!c || !consumed || (n_ranges && !ranges)) return MSIM_ERR_ARG;
    size_t used = 0;
    const int rc = sample_ranges_host(c, ranges, n_ranges, min_block(c->params), words, (size_t)n_words, pos_out, &used);
    *consumed = used;
    return rc;
}

// cut_ranges_host: cut[] needs one slot per drawing range (k > 0) plus one, pool_pos the sum of k over pool-path ranges
int msim_dbg_cut_ranges(msim_ctx *p, const msim_range *ranges, int n_ranges, const uint32_t *words, uint64_t n_words,
                        uint32_t *cut, uint32_t *pool_pos, uint64_t *n_pool_pos, uint64_t *consumed) {
    CTX_FLUSHED(c, p)
    if (!c || !consumed || !n_pool_pos || !cut || (n_ranges && !ranges)) return MSIM_ERR_ARG;
    size_t used = 0, np = 0;
    const int rc = cut_ranges_host(c, ranges, n_ranges, min_block(c->params), words, (size_t)n_words, cut, pool_pos, &np, &used);
    *consumed = used; *n_pool_pos = np;
    return rc;
}

int msim_dbg_chain_boundary(msim_ctx *p, const msim_range *r, uint64_t L, const uint32_t *pos, const uint8_t *type,
                            uint64_t n, const uint32_t *words, uint64_t n_words, uint32_t *stop, uint64_t *consumed,
                            uint64_t *kept, int64_t *len_delta) {
    CTX_FLUSHED(c, p)
    if (!c || !r || !consumed || !kept || !len_delta) return MSIM_ERR_ARG;
    size_t used = 0, nk = 0;
    long long delta = 0;
    const int rc = chain_boundary_host(c, *r, L, pos, type, (size_t)n, words, (size_t)n_words, stop, &used, &nk, &delta);
    *consumed = used; *kept = nk; *len_delta = delta;
    return rc;
}

// The table walk (chain_boundary_tables) over tables built on the host from the same words: same arguments and results
// as msim_dbg_chain_boundary; MSIM_ERR_UNSUPPORTED when the range's lengths do not fit a table entry.
int msim_dbg_chain_boundary_tables(msim_ctx *p, const msim_range *r, uint64_t L, const uint32_t *pos, const uint8_t *type,
                                   uint64_t n, const uint32_t *words, uint64_t n_words, uint32_t *stop, uint64_t *consumed,
                                   uint64_t *kept, int64_t *len_delta) {
    CTX_FLUSHED(c, p)
    if (!c || !r || !consumed || !kept || !len_delta) return MSIM_ERR_ARG;
    ChainClasses cc;
    if (!chain_classes(*r, cc)) return MSIM_ERR_UNSUPPORTED;
    std::vector<uint32_t> T((size_t)(n_words + 1) << chain_lg_rows(cc));
    accept_tables_host(cc, words, (size_t)n_words, T.data());
    size_t used = 0, nk = 0;
    long long delta = 0;
    const int rc = chain_boundary_tables(c, *r, L, pos, type, (size_t)n, cc, T.data(), (size_t)n_words, stop, &used, &nk, &delta);
    *consumed = used; *kept = nk; *len_delta = delta;
    return rc;
}

// The general host-chain engine end to end on the host (multimix_plan_emulated): the record table and insert pool it
// arrives at, for comparison with msim_plan_contig's host planner on the same streams.  Call with recs == NULL for the sizes.
int msim_dbg_multimix_plan(msim_ctx *p, uint64_t L, const msim_range *ranges, int n_ranges, msim_record *recs, uint64_t cap_recs,
                           uint8_t *pool, uint64_t cap_pool, uint64_t *n_recs, uint64_t *pool_len, int *empty) {
    CTX_FLUSHED(c, p)
    if (!c || !n_recs || !pool_len || !empty || (n_ranges && !ranges)) return MSIM_ERR_ARG;
    if (!c->host_only) return fail(c, MSIM_ERR_ARG, "msim_dbg_multimix_plan needs a host-only context");
    HostPlan hp;
    const int rc = multimix_plan_emulated(c, L, ranges, n_ranges, hp);
    if (rc) return rc;
    *n_recs = hp.recs.size(); *pool_len = hp.pool.size(); *empty = hp.empty ? 1 : 0;
    if (recs) {
        if (cap_recs < hp.recs.size() || cap_pool < hp.pool.size()) return fail(c, MSIM_ERR_ARG, "buffers too small");
        if (!hp.recs.empty()) memcpy(recs, hp.recs.data(), hp.recs.size() * sizeof(msim_record));
        if (!hp.pool.empty() && pool) memcpy(pool, hp.pool.data(), hp.pool.size());
    }
    return MSIM_OK;
}

// The counter-based engine (MSIM_RNG_FAST) restated sequentially on the host (fast_plan_emulated): what msim_plan_contig of
// a fast context leaves for the same key, contig ordinal and ranges.  Works on a host-only context.  recs == NULL: sizes only.
int msim_dbg_fast_plan(msim_ctx *p, uint64_t L, const msim_range *ranges, int n_ranges, uint64_t key, uint32_t seq, msim_record *recs,
                       uint64_t cap_recs, uint8_t *pool, uint64_t cap_pool, uint64_t *n_recs, uint64_t *pool_len, int *empty) {
    CTX_FLUSHED(c, p)
    if (!c || !n_recs || !pool_len || !empty || (n_ranges && !ranges)) return MSIM_ERR_ARG;
    if (!c->have_params) return fail(c, MSIM_ERR_ARG, "msim_set_params has not been called");
    HostPlan hp;
    const int rc = fast_plan_emulated(c, L, ranges, n_ranges, key, seq, hp);
    if (rc) return rc;
    *n_recs = hp.recs.size(); *pool_len = hp.pool.size(); *empty = hp.empty ? 1 : 0;
    if (recs) {
        if (cap_recs < hp.recs.size() || cap_pool < hp.pool.size()) return fail(c, MSIM_ERR_ARG, "buffers too small");
        if (!hp.recs.empty()) memcpy(recs, hp.recs.data(), hp.recs.size() * sizeof(msim_record));
        if (!hp.pool.empty() && pool) memcpy(pool, hp.pool.data(), hp.pool.size());
    }
    return MSIM_OK;
}

// test support (tests/test_apply_ref_host.py, tests/test_gpu_apply_tables.py): is this a table the rewrite kernels are written
// for (ctx.h: rec_lengths; apply.hip: rec_view)?  What every planner guarantees, checked: known types, records strictly increasing in
// pos and consuming disjoint input (SN / IN / TLI their own base, DE / DU / IV / TL pos..stop), every span inside the contig,
// every insert inside the pool, an SNP's aux a LUT column, every output offset and the mutated length in [0, 2^32).
// A TLI whose span is empty (extra > stop: __link_tls found no TL, plan_host.cpp) is a planner's table and passes.
// off (optional): the output offset of every record; *delta: mutated length - length.
// bad_index / bad_what (optional): which record was refused and why, for callers that word the refusal themselves (vcf_parse.hip).
static int check_record_table(Ctx *c, uint64_t L, const msim_record *recs, uint64_t n, uint64_t pool_len, std::vector<uint32_t> *off,
                              long long *delta, uint64_t *bad_index = nullptr, const char **bad_what = nullptr) {
    auto bad = [&](uint64_t i, const char *what) {
        if (bad_index) *bad_index = i;
        if (bad_what) *bad_what = what;
        return fail(c, MSIM_ERR_ARG, "record " + std::to_string(i) + ": " + what);
    };
    if (n >= (1ull << 31)) return fail(c, MSIM_ERR_ARG, "more than 2^31 records");
    long long run = 0;                                     // length change of the records so far
    uint64_t next_free = 0;                                // first input position no earlier record consumed
    if (off) off->resize((size_t)n);
    for (uint64_t i = 0; i < n; i++) {
        const msim_record &r = recs[i];
        if (r.type < MSIM_SN || r.type > MSIM_TLI) return bad(i, "unknown type");
        if (r.pos >= L) return bad(i, "position beyond the contig");
        if (i && r.pos < next_free) return bad(i, "not behind the input its predecessor consumed (positions strictly increasing, no overlap)");
        const long long len = (long long)r.stop - (long long)r.pos + 1;
        uint64_t last = r.pos;                             // last input position this record consumes
        switch (r.type) {
            case MSIM_SN:
                if (r.stop != r.pos) return bad(i, "SNP with stop != pos");
                if (r.aux > 2) return bad(i, "SNP outcome (aux) outside 0..2");
                break;
            case MSIM_IN:
                if (len < 1) return bad(i, "stop < pos");
                if (r.extra > pool_len || (uint64_t)len > pool_len - r.extra) return bad(i, "insert outside the insert pool");
                break;
            case MSIM_DE: case MSIM_TL: case MSIM_DU: case MSIM_IV:
                if (len < 1) return bad(i, "stop < pos");
                if (r.stop >= L) return bad(i, "stop beyond the contig");
                last = r.stop;
                break;
            default:                                       // MSIM_TLI: copy of in[extra .. stop]
                if (r.extra <= r.stop && r.stop >= L) return bad(i, "linked span beyond the contig");
                break;
        }
        const long long d = rec_delta(r);                  // (ctx.h: the rewrite kernels' own rule)
        const long long o = (long long)r.pos + run;
        if (o < 0 || o >= (1ll << 32)) return bad(i, "output offset outside [0, 2^32)");
        if (off) (*off)[(size_t)i] = (uint32_t)o;
        run += d;
        next_free = last + 1;
    }
    const long long out_len = (long long)L + run;
    if (out_len < 0 || out_len >= (1ll << 32)) return fail(c, MSIM_ERR_ARG, "mutated length outside [0, 2^32)");
    *delta = run;
    return MSIM_OK;
}

// Installs the caller's record table and insert pool on an existing contig, as the host planner installs its own
// (install_host_table); msim_apply_contig then takes the device-scan route.  Nothing reaches a kernel unless
// check_record_table passes: MSIM_ERR_ARG otherwise, nothing launched, the contig as it was.
// flags & 1: the output offsets and the length change are computed here and left in d_off / known_delta as the host-chain
// engines leave theirs (off_ready, delta_known): APPLY skips the device scan, and the contig may go through msim_dbg_apply_batch.
int msim_dbg_set_records(msim_ctx *p, int contig, const msim_record *recs, uint64_t n_records, const uint8_t *insert_pool,
                         uint64_t pool_len, uint32_t flags) {
    CTX_FLUSHED(c, p)
    if (!c || (n_records && !recs) || (pool_len && !insert_pool) || (flags & ~1u)) return MSIM_ERR_ARG;
    Contig *g = get_contig(c, contig);
    if (!g) return MSIM_ERR_ARG;
    const bool with_offsets = flags & 1u;
    std::vector<uint32_t> off;
    long long delta = 0;
    int rc = check_record_table(c, g->len, recs, n_records, pool_len, with_offsets ? &off : nullptr, &delta);
    if (rc) return rc;
    if ((rc = drain(c))) return rc;                        // this contig's buffers may still be read by its last APPLY
    reset_contig(*g);
    c->text_kind = 0;
    g->apply_stream = nullptr;
    std::vector<msim_record> rv(recs, recs + n_records);
    std::vector<uint8_t> pv(insert_pool, insert_pool + pool_len);
    if ((rc = install_host_table(c, g, rv, pv, n_records == 0))) return rc;
    if (!with_offsets) return MSIM_OK;
    g->delta_known = true;
    g->known_delta = delta;
    if (c->host_only || g->all_snp || !n_records) return MSIM_OK;      // (SNP-only: offset == position, no table)
    rc = dev_reserve(c, g->d_off, (size_t)n_records * sizeof(uint32_t));
    if (rc) return rc;
    MSIM_HIP(c, hipMemcpyAsync(g->d_off.p(), off.data(), (size_t)n_records * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    MSIM_HIP(c, wait_stream(c->stream));
    g->off_ready = true;
    return MSIM_OK;
}

// What flush_deferred_apply does for a group of host-chain contigs: one tile-index launch for all of them, their rewrites as
// one launch per kernel variant (apply_batch_device).  Every contig must hold a table installed with offsets (or an SNP-only one).
int msim_dbg_apply_batch(msim_ctx *p, const int *contigs, int n) {
    CTX_FLUSHED(c, p)
    if (!c || !contigs || n < 1) return MSIM_ERR_ARG;
    NEED_GPU(c);
    std::vector<int> ids(contigs, contigs + n);
    for (int i = 0; i < n; i++) {
        Contig *g = get_contig(c, ids[(size_t)i]);
        if (!g) return MSIM_ERR_ARG;
        if (!g->planned || g->d_dyn || !(g->all_snp || (g->off_ready && g->delta_known)))
            return fail(c, MSIM_ERR_ARG, "msim_dbg_apply_batch: a contig without a table installed with its offsets");
        for (int q = 0; q < i; q++) if (ids[(size_t)q] == ids[(size_t)i]) return fail(c, MSIM_ERR_ARG, "msim_dbg_apply_batch: contig listed twice");
    }
    int rc = drain(c);                                     // nothing of these contigs in flight
    if (rc) return rc;
    c->text_kind = 0;
    for (int id : ids) c->contigs[(size_t)id].apply_stream = c->emit_stream;
    return apply_batch_device(c, ids, true);
}

// The SNP sampler's emission train (plan_gpu.hip: gpu_emit_flush's launches) over bitmaps the caller made: up to 8 jobs of
// (bitmap words, start, contig length, SNP outcomes by rank) go through ONE group's launches, train = 3 or 6; each job's record
// table comes back and, for train 3 where first[i] is given, its APPLY tile index (ceil(len / msim_dbg_apply_tile()) + 1 entries).  The kernels
// can so be run on bitmaps the sampler never produces.  Synchronous; touches no contig.
uint32_t msim_dbg_apply_tile(void) { return 1u << apply_tile_shift(); }
int msim_dbg_emit_train(msim_ctx *p, int n_jobs, const uint64_t *const *bitmaps, const uint32_t *n_words, const uint32_t *start,
                        const uint64_t *contig_len, const uint8_t *const *aux8, uint32_t d, int train, msim_record *const *recs,
                        const uint64_t *cap_recs, uint64_t *n_recs, int32_t *const *first) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    NEED_GPU(c);
    int rc = drain(c);
    if (rc) return rc;
    return gpu_dbg_emit_train(c, n_jobs, bitmaps, n_words, start, contig_len, aux8, d, train, apply_tile_shift(), recs, cap_recs,
                              n_recs, first);
}

// The SNP ti/tv transducer (plan_kernels.h section 5) over words the caller made: k_snp_maps_abs, k_snp_scan_cut_abs and the outcome
// pass in buffers of the call's own (include/msim.h).  Synchronous; touches no contig and no stream session.
int msim_dbg_snp_draws(msim_ctx *p, const uint32_t *words, uint64_t n_words, uint64_t ti_lim, uint64_t start, uint32_t K,
                       uint32_t aux_off, uint32_t *lanes, uint32_t *maps, uint64_t *end_pos, uint32_t *flags, uint8_t *aux) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    NEED_GPU(c);
    int rc = drain(c);
    if (rc) return rc;
    return gpu_dbg_snp_draws(c, words, n_words, ti_lim, start, K, aux_off, lanes, maps, end_pos, flags, aux);
}

// The sampler's tail rounds and stream cut (plan_kernels.h: k_sample_tail) over tables the caller made (include/msim.h).
// Synchronous; touches no contig and no stream session.
int msim_dbg_sample_tail(msim_ctx *p, const uint32_t *words, uint64_t n_words, const uint32_t *acc, uint64_t n_acc, uint32_t acc_first,
                         const uint32_t *blocks, uint32_t n_blocks, uint32_t raw_counts, uint32_t W, uint32_t shift, uint32_t n,
                         uint32_t k, uint32_t *bitmap, uint32_t bm_guard, msim_dbg_tail_state *state, int anchored, uint64_t win_pos,
                         uint32_t need0, uint32_t d1, uint64_t pos_limit) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    NEED_GPU(c);
    int rc = drain(c);
    if (rc) return rc;
    return gpu_dbg_sample_tail(c, words, n_words, acc, n_acc, acc_first, blocks, n_blocks, raw_counts, W, shift, n, k, bitmap, bm_guard,
                               state, anchored, win_pos, need0, d1, pos_limit);
}

// An anchored contig's whole chain (plan_kernels.h: k_chain_fused, or k_ahead_fringe / k_sample_tail / k_snp_scan_cut_abs) over
// tables the caller made (include/msim.h).  Synchronous; touches no contig and no stream session.
int msim_dbg_chain_step(msim_ctx *p, const uint32_t *words, uint64_t n_words, const uint32_t *hcnt, const uint32_t *hacc, uint64_t n_hacc,
                        const uint32_t *tail, uint64_t n_tail, const uint32_t *cnt, uint32_t *bitmap, uint32_t *win_maps,
                        msim_dbg_chain *io) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    NEED_GPU(c);
    int rc = drain(c);
    if (rc) return rc;
    return gpu_dbg_chain_step(c, words, n_words, hcnt, hacc, n_hacc, tail, n_tail, cnt, bitmap, win_maps, io);
}
int msim_dbg_chains_fused(msim_ctx *p, uint64_t *n) {
    Ctx *c = reinterpret_cast<Ctx *>(p);
    if (!c || !n) return MSIM_ERR_ARG;
    *n = gpu_plan_chains_fused(c->gpu);
    return MSIM_OK;
}

// The device halves of the SV-mix and host-chain engines over tables the caller made (plan_gpu.hip: gpu_dbg_*): the engines' own
// launch helpers in buffers of the call's own.  Synchronous; no contig, no stream session.  Each refuses with MSIM_ERR_ARG,
// before anything is launched, whatever the planners cannot produce.
//   msim_dbg_candidates: the candidate front.  bitmap given: one range (bitmap, start, d, sets[0]) through k_bitmap_count,
//     k_scan_u32, k_bitmap_expand_cand; bitmap NULL: K candidates over rt[n_draw] (four uint32: rec_base, clip, set_id, 0) and
//     sets[n_sets] (80 bytes: thr[8] u64, n u32, type[8] u8) through k_types_multi.  Then k_nsn_count, k_scan_u32, k_nsn_scatter.
//     np_words: raw (untempered) NumPy-stream words, two per candidate.
//   msim_dbg_accept_tables: k_accept_tables at p0 and k_accept_tables_ps behind k_set_pos(p0) over raw CPython-stream words;
//     (n + 1) << lg_rows entries each.  msim_dbg_accept_tables_host: the host's tables (accept_tables_host) over TEMPERED words,
//     same checks, no context.
//   msim_dbg_mixed_emit: k_stop_scatter, k_link_scatter, k_blk_reduce, k_scan_max_u32, k_keep_flags, k_scan4, k_emit_records,
//     k_pool_fill over candidates, chain verdicts and (optionally) a range table; block[] from msim_set_params.
int msim_dbg_candidates(msim_ctx *p, const uint64_t *bitmap, uint32_t n_words, uint32_t start, uint32_t d, uint32_t K,
                        const void *rt, uint32_t n_draw, const void *sets, uint32_t n_sets, const uint32_t *np_words, uint64_t n_np_words,
                        uint32_t all, uint32_t *cand_pos, uint8_t *cand_type, uint32_t *nsn_pos, uint8_t *nsn_type, uint32_t *nsn_rank,
                        uint64_t cap, uint32_t *k_out, uint32_t *n_nsn) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    NEED_GPU(c);
    int rc = drain(c);
    if (rc) return rc;
    return gpu_dbg_candidates(c, bitmap, n_words, start, d, K, rt, n_draw,
                              sets, n_sets, np_words, n_np_words, all, cand_pos, cand_type, nsn_pos,
                              nsn_type, nsn_rank, cap, k_out, n_nsn);
}

int msim_dbg_accept_tables(msim_ctx *p, const uint32_t *raw_words, uint64_t n_words, uint64_t p0, uint32_t n, const uint32_t *shift,
                           const uint32_t *width, uint32_t n_classes, uint32_t *T, uint32_t *T_ps) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    NEED_GPU(c);
    int rc = drain(c);
    if (rc) return rc;
    return gpu_dbg_accept_tables(c, raw_words, n_words, p0, n, shift, width, n_classes, T, T_ps);
}

int msim_dbg_accept_tables_host(const uint32_t *tempered, uint32_t n, const uint32_t *shift, const uint32_t *width, uint32_t n_classes,
                                uint32_t *T) {
    ChainClasses cc;
    if (!T || (n && !tempered) || n > (1u << 26) || !dbg_chain_classes(shift, width, n_classes, cc)) return MSIM_ERR_ARG;
    memset(T, 0, (((size_t)n + 1) << chain_lg_rows(cc)) * 4);
    accept_tables_host(cc, tempered, n, T);
    return MSIM_OK;
}

int msim_dbg_mixed_emit(msim_ctx *p, uint64_t L, uint32_t k, const uint32_t *cand_pos, const uint8_t *cand_type, uint32_t n_ch,
                        const uint32_t *ch_rank, const uint32_t *ch_stop, const uint32_t *ch_extra, const uint8_t *ch_aux, uint32_t n_draw,
                        const void *rt, const uint32_t *visit_from, uint32_t sn_chained, const uint32_t *np_words, uint64_t n_np_words,
                        msim_record *recs, uint32_t *rec_off, uint32_t *sn_index, uint8_t *pool, uint64_t cap_pool, uint32_t *counts,
                        int64_t *len_delta) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    NEED_GPU(c);
    int rc = drain(c);
    if (rc) return rc;
    return gpu_dbg_mixed_emit(c, L, k, cand_pos, cand_type, n_ch, ch_rank, ch_stop, ch_extra, ch_aux, n_draw,
                              rt, visit_from, sn_chained, np_words, n_np_words, recs, rec_off, sn_index,
                              pool, cap_pool, counts, len_delta);
}

// test support (tests/test_ahead_moments.py, CPU tier): the moments the anchored windows are laid out from; needs no context
int msim_dbg_stream_moments(uint64_t n, uint64_t k, uint64_t K, uint64_t ti_lim, double out[4]) {
    if (!out || !n || k >= n) return MSIM_ERR_ARG;
    const StreamMoments a = sample_words_moments(n, k), b = snp_words_moments(K, (unsigned long long)ti_lim);
    out[0] = a.e; out[1] = a.v; out[2] = b.e; out[3] = b.v;
    return MSIM_OK;
}

// test support (tests/test_stream_need_host.py, CPU tier): the stream-window arithmetic (plan_windows.h) as gpu_plan_make_room and
// the engines use it; needs no context.  out: the table's need py, np, bad; of ranges[0]: the big-sample window, the small-sample
// mean and variance bound, the least randint acceptance
int msim_dbg_stream_need(const msim_params *params, const msim_range *ranges, int n_ranges, double out[7]) {
    if (!params || !ranges || n_ranges < 1 || !out) return MSIM_ERR_ARG;
    const msim_range &r = ranges[0];
    const double n = (double)range_population(r, min_block(*params)), k = (double)r.k;
    if (n < 1) return MSIM_ERR_ARG;
    const StreamNeed need = stream_need(*params, ranges, n_ranges);
    const StreamMoments m = small_sample_moments(n, k, (double)r.setsize);
    out[0] = need.py; out[1] = need.np; out[2] = need.bad ? 1.0 : 0.0;
    out[3] = big_sample_window(n, set_path_need(n, k)); out[4] = m.e; out[5] = m.v; out[6] = randint_acceptance_min(r);
    return MSIM_OK;
}

int msim_dbg_stream_status(msim_ctx *p, int out[8]) {
    CTX_FLUSHED(c, p)
    if (!c || !out || c->host_only || !c->gpu) return MSIM_ERR_ARG;
    gpu_plan_stream_status(c, c->gpu, out);
    return MSIM_OK;
}

// test support (tests/test_gpu_waits.py): `ms` milliseconds of a one-lane kernel that does nothing, on the plan stream
// (which = 0) or the emit stream (1) -- bounded by the device's 100 MHz wall clock, so the queue always drains -- for the
// deadline of the host waits (ctx.h: wait_stream / wait_event, MSIM_WAIT_TIMEOUT_S) to be met by a wait that is really kept waiting
__global__ void k_dbg_stall(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
}
int msim_dbg_stall(msim_ctx *p, int which, uint32_t ms) {
    Ctx *c = C(p);
    if (!c || c->host_only || which < 0 || which > 1 || ms > 10000) return MSIM_ERR_ARG;
    hipLaunchKernelGGL(k_dbg_stall, dim3(1), dim3(1), 0, which ? c->emit_stream : c->stream, (unsigned long long)ms * 100000ull);
    MSIM_HIP(c, hipGetLastError());
    return MSIM_OK;
}

// test support (tools/hw_queue_probe.py): n more streams at a priority (-1 the plan stream's, 0 normal, 1 the lowest), each used
// once so that the runtime really gives it a hardware queue, kept until the process ends -- and the time of `launches` dependent
// one-lane launches on the context's plan stream (ns per launch).  What it shows: how a process's NUMBER of hardware queues
// changes the latency of every launch.
int msim_dbg_queue_probe(msim_ctx *p, int n_more, int prio, int launches, int idle_us, double *ns_per_launch) {
    Ctx *c = C(p);
    if (!c || c->host_only || n_more < 0 || n_more > 64 || launches < 1 || !ns_per_launch) return MSIM_ERR_ARG;
    int lo = 0, hi = 0;
    MSIM_HIP(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
    for (int i = 0; i < n_more; i++) {
        hipStream_t s = nullptr;                               // (deliberately never destroyed)
        MSIM_HIP(c, hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio < 0 ? hi : prio > 0 ? lo : 0));
        hipLaunchKernelGGL(k_dbg_stall, dim3(1), dim3(1), 0, s, 0ull);
        MSIM_HIP(c, wait_stream(s));
    }
    for (int w = 0; w < 64; w++) hipLaunchKernelGGL(k_dbg_stall, dim3(1), dim3(1), 0, c->stream, 0ull);
    MSIM_HIP(c, wait_stream(c->stream));
    if (idle_us > 0) {
        // a BURST of four dependent launches after the queue has idled for idle_us (what a host-chain engine does between two
        // walks): launch -> completion of the burst, averaged over `launches` bursts
        double sum = 0;
        for (int i = 0; i < launches; i++) {
            std::this_thread::sleep_for(std::chrono::microseconds(idle_us));
            const auto b0 = std::chrono::steady_clock::now();
            for (int q = 0; q < 4; q++) hipLaunchKernelGGL(k_dbg_stall, dim3(1), dim3(1), 0, c->stream, 0ull);
            MSIM_HIP(c, wait_stream(c->stream));
            sum += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - b0).count();
        }
        *ns_per_launch = sum / launches;
        return MSIM_OK;
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < launches; i++) hipLaunchKernelGGL(k_dbg_stall, dim3(1), dim3(1), 0, c->stream, 0ull);
    MSIM_HIP(c, hipGetLastError());
    MSIM_HIP(c, wait_stream(c->stream));
    *ns_per_launch = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / launches;
    return MSIM_OK;
}

int msim_stats(msim_ctx *p, msim_timing *out) {
    CTX_FLUSHED(c, p)
    if (!c || !out) return MSIM_ERR_ARG;
    {
        int rc = drain(c);
        if (rc) return rc;
    }
    *out = c->t;
    return MSIM_OK;
}

int msim_reset_stats(msim_ctx *p) {
    CTX_FLUSHED(c, p)
    if (!c) return MSIM_ERR_ARG;
    {
        int rc = drain(c);
        if (rc) return rc;
    }
    c->t = msim_timing{};
    spectrum_reset_timing(c);
    compare_reset_timing(c);
    reads_reset_timing(c);
    return MSIM_OK;
}

}  // extern "C"

// what vcf_parse.hip shares with the planners' installation path (ctx.h)
namespace msim {
int table_install(Ctx *c, Contig *g, std::vector<msim_record> &recs, std::vector<uint8_t> &pool, bool empty) {
    return ::install_host_table(c, g, recs, pool, empty);
}
int table_check(Ctx *c, uint64_t L, const msim_record *recs, uint64_t n, uint64_t pool_len, long long *delta, uint64_t *bad_index,
                const char **bad_what) {
    return ::check_record_table(c, L, recs, n, pool_len, nullptr, delta, bad_index, bad_what);
}
}  // namespace msim
