// Device text -> output files, off the calling thread.
// gfx950 (MI355X) host side.                                              SURVEY.md section 8(f) rows 1-2 (egress).
//
// The CLI's outputs are files: the mutated Fasta (about as large as the genome) and the VCF.  What the bytes are is decided
// by the kernels of text_gpu.hip (fasta_writer.py:40-58, vcf_writer.py:118-126); this file only moves them, and the moving
// is what an end-to-end run spends its time on.  Measured on the MI355X box for 1.2 GiB into a fresh file (tmpfs / overlay):
//     mmap the span + copy into it (first-touch faults) + munmap     355 / 190 ms      <- what a D2H copy into a mapping pays
//     fallocate + mmap + populate + copy + munmap                    243 / 143 ms
//     the same with 4 threads on 4 slices of one file                386 / 515 ms      <- faults on one file do not scale
//     write() in 8 MiB pieces from a resident buffer                 144 /  85 ms      <- no page tables to build and tear down
// So: a channel per output file (0 the Fasta, 1 the VCF), each with its own thread, HIP stream and a small pinned ring.  An
// entry point renders the text into one of the channel's two device buffers on the context's stream and queues a job; the
// channel's thread copies it device -> pinned ring in 8 MiB pieces (the copy of piece k + 1 runs while piece k is written)
// and pwrite()s the pieces to the file.  The calling thread goes on with the next contig's ingest / PLAN / APPLY meanwhile;
// file_wait() joins.  Writes to ONE file serialise on its inode in the kernel anyway -- one thread per file is all there is.
#include <cctype>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>

#include <fcntl.h>
#include <pthread.h>
#include <sched.h>
#include <sys/stat.h>
#include <unistd.h>

#include "bgzf.h"
#include "ctx.h"

namespace msim {

namespace {

constexpr size_t FILE_CHUNK = 8u << 20;
constexpr int FILE_SLOTS = 3;

struct FileJob {
    const uint8_t *d_src;                  // device text (a buffer of the channel) ...
    const uint8_t *h_src;                  // ... or host text the caller keeps untouched until the channel is idle
    int buf;
    uint64_t n;
    int fd;                                // a dup() of the caller's descriptor: closed when the job is done
    uint64_t offset;
    bool bgzf = false;                     // BGZF mode: the bytes are appended to the channel's uncompressed stream
    bool bgzf_close = false;               //   ... or the stream is finished: tail, EOF marker
    std::shared_ptr<std::vector<uint8_t>> owned;   // host bytes the channel holds itself (msim_bgzf_append)
};

struct FileChannel {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv_job, cv_done;
    std::deque<FileJob> q;
    bool stop = false, running = false, started = false;
    int err = 0;
    std::string err_msg;
    int device = 0;
    // the thread's own
    hipStream_t st = nullptr;
    uint8_t *pin = nullptr;
    hipEvent_t ev[FILE_SLOTS] = {};
    // text buffers (device), filled by the calling thread on the context's stream
    Scratch<uint8_t> d_buf[2];
    bool in_flight[2] = {false, false};
    hipEvent_t ready[2] = {nullptr, nullptr};
    // BGZF mode (bgzf.hip).  The calling thread's view: on, the file, the uncompressed bytes queued so far.
    bool bz = false;
    int bz_fd = -1;
    uint64_t bz_queued = 0;
    // the channel thread's: device staging of the uncompressed stream (whole blocks are compressed once it is full), the
    // bytes compressed so far and the compressed bytes written
    uint8_t *bz_stage = nullptr;
    uint64_t bz_fill = 0, bz_ulen = 0, bz_clen = 0;
    BgzfWork bz_w;
};

}  // namespace

struct FileIo { FileChannel ch[2]; };

namespace {

void set_err(FileChannel &ch, int code, const std::string &msg) {
    std::lock_guard<std::mutex> lk(ch.mu);
    if (!ch.err) { ch.err = code; ch.err_msg = msg; }
}

bool pwrite_all(int fd, const uint8_t *p, size_t n, uint64_t off, std::string &why) {
    while (n) {
        const ssize_t w = pwrite(fd, p, n, (off_t)off);
        if (w < 0) {
            if (errno == EINTR) continue;
            why = std::string("pwrite: ") + strerror(errno);
            return false;
        }
        p += w; n -= (size_t)w; off += (uint64_t)w;
    }
    return true;
}

hipError_t channel_stream(FileChannel &ch) {
    hipError_t e = hipSuccess;
    if (!ch.st) {
        e = hipSetDevice(ch.device);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&ch.st, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipHostMalloc((void **)&ch.pin, FILE_CHUNK * FILE_SLOTS, hipHostMallocDefault);
        for (int i = 0; i < FILE_SLOTS && e == hipSuccess; i++) e = hipEventCreateWithFlags(&ch.ev[i], hipEventDisableTiming);
    }
    return e;
}

constexpr uint64_t BZ_STAGE = BGZF_PIECE_BLOCKS * BGZF_BLOCK;

// Compress staging bytes [0, n) (whole blocks, or everything at the end of the stream), write the members at the channel's
// compressed offset through the pinned ring, move what is left of the staging to its front.
bool bz_flush(FileChannel &ch, uint64_t n, hipError_t &e, std::string &why) {
    uint64_t out = 0;
    e = bgzf_compress_device(ch.bz_stage, n, ch.bz_w, ch.st, &out);
    if (e != hipSuccess) return false;
    const uint64_t pieces = (out + FILE_CHUNK - 1) / FILE_CHUNK;
    auto issue = [&](uint64_t k) {
        const uint64_t off = k * FILE_CHUNK, len = out - off < FILE_CHUNK ? out - off : FILE_CHUNK;
        const int slot = (int)(k % FILE_SLOTS);
        hipError_t r = hipMemcpyAsync(ch.pin + (size_t)slot * FILE_CHUNK, ch.bz_w.d_out + off, len, hipMemcpyDeviceToHost, ch.st);
        if (r == hipSuccess) r = hipEventRecord(ch.ev[slot], ch.st);
        return r;
    };
    for (uint64_t k = 0; k < pieces && k < (uint64_t)FILE_SLOTS && e == hipSuccess; k++) e = issue(k);
    for (uint64_t k = 0; k < pieces && e == hipSuccess; k++) {
        const int slot = (int)(k % FILE_SLOTS);
        e = wait_event(ch.ev[slot]);
        if (e != hipSuccess) break;
        const uint64_t off = k * FILE_CHUNK, len = out - off < FILE_CHUNK ? out - off : FILE_CHUNK;
        if (!pwrite_all(ch.bz_fd, ch.pin + (size_t)slot * FILE_CHUNK, len, ch.bz_clen + off, why)) {
            (void)wait_stream(ch.st);
            return false;
        }
        if (k + FILE_SLOTS < pieces) e = issue(k + FILE_SLOTS);
    }
    if (e != hipSuccess) return false;
    ch.bz_clen += out;
    ch.bz_ulen += n;
    const uint64_t tail = ch.bz_fill - n;                  // (< one block, and n >= one block: no overlap)
    if (tail) e = hipMemcpyAsync(ch.bz_stage, ch.bz_stage + n, tail, hipMemcpyDeviceToDevice, ch.st);
    ch.bz_fill = tail;
    return e == hipSuccess;
}

// A job of a channel in BGZF mode: its bytes are appended to the staging (full staging: compressed and written), or the
// stream is closed (the tail, then the EOF marker).
void run_bgzf_job(FileChannel &ch, const FileJob &job) {
    {
        std::lock_guard<std::mutex> lk(ch.mu);
        if (ch.err) return;
    }
    std::string why;
    hipError_t e = channel_stream(ch);
    if (e == hipSuccess && !ch.bz_stage) e = hipMalloc((void **)&ch.bz_stage, BZ_STAGE + PAD);
    bool ok = e == hipSuccess;
    if (ok && job.bgzf_close) {
        if (ch.bz_fill) ok = bz_flush(ch, ch.bz_fill, e, why);
        if (ok) ok = pwrite_all(ch.bz_fd, BGZF_EOF, sizeof BGZF_EOF, ch.bz_clen, why);
        if (ok) ch.bz_clen += sizeof BGZF_EOF;
    } else if (ok) {
        const uint8_t *src = job.owned ? job.owned->data() : job.h_src ? job.h_src : job.d_src;
        const hipMemcpyKind kind = job.d_src && !job.owned && !job.h_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        if (kind == hipMemcpyDeviceToDevice) e = hipStreamWaitEvent(ch.st, ch.ready[job.buf], 0);   // the text is complete
        uint64_t left = job.n;
        while (ok && left && e == hipSuccess) {
            const uint64_t take = left < BZ_STAGE - ch.bz_fill ? left : BZ_STAGE - ch.bz_fill;
            e = hipMemcpyAsync(ch.bz_stage + ch.bz_fill, src, take, kind, ch.st);
            ch.bz_fill += take;
            src += take;
            left -= take;
            if (e == hipSuccess && ch.bz_fill == BZ_STAGE) ok = bz_flush(ch, BZ_STAGE, e, why);
        }
        if (ok && e == hipSuccess) e = wait_stream(ch.st);      // (the source may be reused once the channel is idle)
        ok = ok && e == hipSuccess;
    }
    if (e != hipSuccess) {
        set_err(ch, MSIM_ERR_HIP, std::string("output channel (BGZF): ") + hipGetErrorString(e));
        if (ch.st) (void)wait_stream(ch.st);
    } else if (!ok) {
        set_err(ch, MSIM_ERR_IO, why);
    }
}

void run_job(FileChannel &ch, const FileJob &job) {
    if (job.bgzf) { run_bgzf_job(ch, job); return; }
    static const bool prof = getenv("MSIM_IO_PROF") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    double wait_ms = 0, write_ms = 0;
    bool failed;
    { std::lock_guard<std::mutex> lk(ch.mu); failed = ch.err != 0; }
    hipError_t e = hipSuccess;
    if (!failed && job.h_src) {                             // host text (a batch of small contigs, framed on the host)
        const auto tb = std::chrono::steady_clock::now();
        std::string why;
        if (!pwrite_all(job.fd, job.h_src, job.n, job.offset, why)) set_err(ch, MSIM_ERR_IO, why);
        if (prof) write_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb).count();
        failed = true;                                      // (nothing left to do below)
    }
    if (!failed && !ch.st) {
        e = hipSetDevice(ch.device);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&ch.st, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipHostMalloc((void **)&ch.pin, FILE_CHUNK * FILE_SLOTS, hipHostMallocDefault);
        for (int i = 0; i < FILE_SLOTS && e == hipSuccess; i++) e = hipEventCreateWithFlags(&ch.ev[i], hipEventDisableTiming);
    }
    if (!failed && e == hipSuccess) e = hipStreamWaitEvent(ch.st, ch.ready[job.buf], 0);   // the text is complete
    if (!failed && e == hipSuccess) {
        const uint64_t pieces = (job.n + FILE_CHUNK - 1) / FILE_CHUNK;
        auto issue = [&](uint64_t k) {
            const uint64_t off = k * FILE_CHUNK, len = job.n - off < FILE_CHUNK ? job.n - off : FILE_CHUNK;
            const int slot = (int)(k % FILE_SLOTS);
            hipError_t r = hipMemcpyAsync(ch.pin + (size_t)slot * FILE_CHUNK, job.d_src + off, len, hipMemcpyDeviceToHost, ch.st);
            if (r == hipSuccess) r = hipEventRecord(ch.ev[slot], ch.st);
            return r;
        };
        for (uint64_t k = 0; k < pieces && k < (uint64_t)FILE_SLOTS && e == hipSuccess; k++) e = issue(k);
        for (uint64_t k = 0; k < pieces && e == hipSuccess; k++) {
            const int slot = (int)(k % FILE_SLOTS);
            const auto ta = std::chrono::steady_clock::now();
            e = wait_event(ch.ev[slot]);
            if (e != hipSuccess) break;
            const auto tb = std::chrono::steady_clock::now();
            const uint64_t off = k * FILE_CHUNK, len = job.n - off < FILE_CHUNK ? job.n - off : FILE_CHUNK;
            std::string why;
            const bool ok = pwrite_all(job.fd, ch.pin + (size_t)slot * FILE_CHUNK, len, job.offset + off, why);
            if (prof) {
                wait_ms += std::chrono::duration<double, std::milli>(tb - ta).count();
                write_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb).count();
            }
            if (!ok) {
                set_err(ch, MSIM_ERR_IO, why);
                (void)wait_stream(ch.st);
                break;
            }
            if (k + FILE_SLOTS < pieces) e = issue(k + FILE_SLOTS);
        }
    }
    if (e != hipSuccess) {
        set_err(ch, MSIM_ERR_HIP, std::string("output channel: ") + hipGetErrorString(e));
        if (ch.st) (void)wait_stream(ch.st);
    }
    (void)close(job.fd);
    if (prof)
        fprintf(stderr, "[msim io] t=%.4f %.1f MB at offset %llu: %.1f ms (waiting for the device copies %.1f, pwrite %.1f = %.2f GB/s)\n", std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(), job.n / 1e6,
                (unsigned long long)job.offset, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(),
                wait_ms, write_ms, write_ms > 0 ? job.n / 1e6 / write_ms : 0.0);
}

// A channel's thread runs on the CPUs of the NUMA node its GPU hangs on (sysfs: the PCI device's numa_node, the node's
// cpulist): the ring the DMA engine fills, the thread that reads it and the file pages it writes then share a socket -- on the
// two-socket hosts of the pool a CLI run pinned to the GPU's node took 0.31 s where the unpinned one took 0.40.
// MSIM_IO_CPUS overrides: a cpulist ("64-127,192-255"), or "none".
bool parse_cpulist(const char *s, cpu_set_t *set) {
    CPU_ZERO(set);
    bool any = false;
    while (*s) {
        char *end;
        long a = strtol(s, &end, 10);
        if (end == s) return false;
        long b = a;
        if (*end == '-') { s = end + 1; b = strtol(s, &end, 10); if (end == s) return false; }
        for (long q = a; q <= b && q < CPU_SETSIZE; q++) { CPU_SET((int)q, set); any = true; }
        s = end;
        while (*s == ',' || *s == ' ' || *s == '\n') s++;
    }
    return any;
}

bool read_line(const std::string &path, char *buf, size_t cap) {
    FILE *f = fopen(path.c_str(), "r");
    if (!f) return false;
    const bool ok = fgets(buf, (int)cap, f) != nullptr;
    fclose(f);
    return ok;
}

// cpulist of the NUMA node the device hangs on ("" when sysfs does not tell or the host has one node)
void gpu_node_cpulist(int device, char *buf, size_t cap) {
    buf[0] = 0;
    char bus[64] = {0}, tmp[64];
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) { (void)hipGetLastError(); return; }
    for (char *q = bus; *q; q++) *q = (char)tolower((unsigned char)*q);
    if (!read_line(std::string("/sys/bus/pci/devices/") + bus + "/numa_node", tmp, sizeof tmp)) return;
    const int node = atoi(tmp);
    if (node < 0) return;                                   // (a one-node host says -1)
    if (!read_line("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist", buf, cap)) buf[0] = 0;
    for (char *q = buf; *q; q++) if (*q == '\n') *q = 0;
}

void pin_to_gpu_node(int device) {
    cpu_set_t set;
    char buf[4096];
    if (const char *e = getenv("MSIM_IO_CPUS")) {
        if (strcmp(e, "none") != 0 && parse_cpulist(e, &set)) (void)pthread_setaffinity_np(pthread_self(), sizeof set, &set);
        return;
    }
    gpu_node_cpulist(device, buf, sizeof buf);
    if (buf[0] && parse_cpulist(buf, &set)) (void)pthread_setaffinity_np(pthread_self(), sizeof set, &set);   // (refused in a narrower cpuset: stays put)
}

void channel_main(FileChannel *chp) {
    FileChannel &ch = *chp;
    pin_to_gpu_node(ch.device);
    for (;;) {
        FileJob job;
        {
            std::unique_lock<std::mutex> lk(ch.mu);
            ch.cv_job.wait(lk, [&] { return ch.stop || !ch.q.empty(); });
            if (ch.q.empty()) break;                        // (stop: only once the queue is empty)
            job = ch.q.front();
            ch.q.pop_front();
            ch.running = true;
        }
        run_job(ch, job);
        job.owned.reset();
        {
            std::lock_guard<std::mutex> lk(ch.mu);
            ch.running = false;
            if (job.buf >= 0) ch.in_flight[job.buf] = false;
        }
        ch.cv_done.notify_all();
    }
    if (ch.st) {
        (void)wait_stream(ch.st);
        bgzf_work_free(ch.bz_w);
        if (ch.bz_stage) (void)hipFree(ch.bz_stage);
        ch.bz_stage = nullptr;
        for (auto &e : ch.ev) if (e) (void)hipEventDestroy(e);
        if (ch.pin) (void)hipHostFree(ch.pin);
        (void)hipStreamDestroy(ch.st);
        ch.st = nullptr;
    }
}

FileIo *io_get(Ctx *c) {
    if (!c->file_io) {
        c->file_io = new FileIo;
        for (auto &ch : c->file_io->ch) ch.device = c->device;
    }
    return c->file_io;
}

// queue a BGZF job (the calling thread): starts the channel's thread on first use, counts the uncompressed bytes
int bz_push(Ctx *c, FileChannel &ch, FileJob job) {
    {
        std::lock_guard<std::mutex> lk(ch.mu);
        if (!ch.started) {
            try {
                ch.th = std::thread(channel_main, &ch);
            } catch (const std::system_error &e) {
                return fail(c, MSIM_ERR_NOMEM, std::string("output channel thread: ") + e.what());
            }
            ch.started = true;
        }
        if (job.buf >= 0) ch.in_flight[job.buf] = true;
        if (!job.bgzf_close) ch.bz_queued += job.n;
        ch.q.push_back(std::move(job));
    }
    ch.cv_job.notify_one();
    return MSIM_OK;
}

}  // namespace

// BGZF mode of channel `ch_id` on `fd` (a regular file, written from offset 0): until file_bgzf_close, every job queued on
// the channel -- device text, host text, file_bgzf_append -- is appended to one uncompressed stream in queue order, and
// the offsets the *_file entry points are given must be that stream's length.
int file_bgzf_open(Ctx *c, int ch_id, int fd) {
    int rc = file_check(c, fd);
    if (rc) return rc;
    FileChannel &ch = io_get(c)->ch[ch_id];
    file_channel_idle(c, ch_id);
    if (ch.bz) return fail(c, MSIM_ERR_ARG, "output channel is in BGZF mode already");
    const int own = dup(fd);
    if (own < 0) return fail(c, MSIM_ERR_IO, std::string("dup: ") + strerror(errno));
    std::lock_guard<std::mutex> lk(ch.mu);
    ch.bz = true;
    ch.bz_fd = own;
    ch.bz_queued = 0;
    ch.bz_fill = ch.bz_ulen = ch.bz_clen = 0;
    return MSIM_OK;
}

int file_bgzf_append(Ctx *c, int ch_id, const uint8_t *src, uint64_t n) {
    FileChannel &ch = io_get(c)->ch[ch_id];
    if (!ch.bz) return fail(c, MSIM_ERR_ARG, "output channel is not in BGZF mode");
    if (!n) return MSIM_OK;
    FileJob job{nullptr, nullptr, -1, n, -1, ch.bz_queued, false, false, nullptr};
    job.bgzf = true;
    try {
        job.owned = std::make_shared<std::vector<uint8_t>>(src, src + n);
    } catch (const std::bad_alloc &) {
        return fail(c, MSIM_ERR_NOMEM, "BGZF append");
    }
    return bz_push(c, ch, std::move(job));
}

// The tail and the EOF marker go out; waits for the channel; the mode ends (the descriptor is the caller's again).
int file_bgzf_close(Ctx *c, int ch_id, uint64_t *compressed, uint64_t *uncompressed) {
    FileChannel &ch = io_get(c)->ch[ch_id];
    if (!ch.bz) return fail(c, MSIM_ERR_ARG, "output channel is not in BGZF mode");
    FileJob job{nullptr, nullptr, -1, 0, -1, ch.bz_queued, false, false, nullptr};
    job.bgzf = true;
    job.bgzf_close = true;
    int rc = bz_push(c, ch, std::move(job));
    file_channel_idle(c, ch_id);
    std::lock_guard<std::mutex> lk(ch.mu);
    if (compressed) *compressed = ch.bz_clen;
    if (uncompressed) *uncompressed = ch.bz_ulen;
    (void)close(ch.bz_fd);
    ch.bz = false;
    ch.bz_fd = -1;
    if (rc == MSIM_OK && ch.err) {
        rc = ch.err;
        fail(c, ch.err, ch.err_msg);
        ch.err = 0;
        ch.err_msg.clear();
    }
    return rc;
}

// One-shot: host bytes -> BGZF bytes (members + EOF marker) in `out` (cap >= bgzf_bound(n)), on the context's stream.
uint64_t bgzf_bound(uint64_t n) { return (n + BGZF_BLOCK - 1) / BGZF_BLOCK * (BGZF_BLOCK + 5 + 26) + sizeof BGZF_EOF; }

int bgzf_compress_host(Ctx *c, const uint8_t *src, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *written, float *device_ms) {
    if (cap < bgzf_bound(n)) return fail(c, MSIM_ERR_ARG, "BGZF output buffer smaller than msim_bgzf_bound");
    BgzfWork w;
    Scratch<uint8_t> in;                                   // (whatever ends the call frees it)
    uint64_t done = 0, pos = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    float total_ms = 0;
    hipError_t e = dev_alloc(in, BZ_STAGE + PAD);
    uint8_t *const d_in = in.p();
    for (int i = 0; i < 2 && e == hipSuccess && device_ms; i++) e = hipEventCreate(&ev[i]);
    while (e == hipSuccess && pos < n) {
        const uint64_t take = n - pos < BZ_STAGE ? n - pos : BZ_STAGE;
        uint64_t got = 0;
        e = hipMemcpyAsync(d_in, src + pos, take, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = bgzf_compress_device(d_in, take, w, c->stream, &got, ev[0], ev[1]);
        float ms = 0;
        if (e == hipSuccess && device_ms && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) total_ms += ms;
        if (e == hipSuccess) e = hipMemcpyAsync(out + done, w.d_out, got, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = wait_stream(c->stream);
        done += got;
        pos += take;
    }
    bgzf_work_free(w);
    (void)in.release();
    for (auto x : ev) if (x) (void)hipEventDestroy(x);
    if (device_ms) *device_ms = total_ms;
    if (e != hipSuccess) return fail(c, MSIM_ERR_HIP, std::string("BGZF compression: ") + hipGetErrorString(e));
    memcpy(out + done, BGZF_EOF, sizeof BGZF_EOF);
    *written = done + sizeof BGZF_EOF;
    return MSIM_OK;
}

// One-shot: a whole BGZF file (host bytes) -> its uncompressed bytes in `out`.  Pieces of at most BGZF_PIECE_BLOCKS members
// alternate between two slots, each with a stream of its own (upload -> k_bgzf_inflate -> download), so that a piece's
// copies overlap its neighbour's kernel.  `src` and `out` belong to the caller: whatever ends the call -- a member that
// fails a check, a HIP error, a wait that ran into its deadline -- both streams are drained before it returns, so no copy
// is left in flight into memory the caller may free.
int bgzf_probe_host(const uint8_t *src, uint64_t n, uint64_t *uncompressed, uint64_t *members) {
    std::string why;
    if (!bgzf_walk(src, n, uncompressed, members, nullptr, &why)) return fail(nullptr, MSIM_ERR_VALUE, "BGZF input, " + why);
    return MSIM_OK;
}

int bgzf_inflate_host(Ctx *c, const uint8_t *src, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *written, float *device_ms) {
    std::vector<BgzfMemberHost> mem;
    std::string why;
    uint64_t total = 0;
    if (!bgzf_walk(src, n, &total, nullptr, &mem, &why)) return fail(c, MSIM_ERR_VALUE, "BGZF input, " + why);
    if (cap < total) return fail(c, MSIM_ERR_ARG, "BGZF output buffer smaller than the uncompressed size msim_bgzf_probe reports");
    *written = 0;
    if (device_ms) *device_ms = 0;
    constexpr size_t P = BGZF_PIECE_BLOCKS;
    constexpr size_t IN_CAP = P * 65536, OUT_CAP = P * (size_t)BGZF_MAX_ISIZE;
    struct Slot {
        hipStream_t st = nullptr;
        hipEvent_t ev[2] = {nullptr, nullptr};
        uint8_t *d_in = nullptr, *d_out = nullptr;
        BgzfMember *d_meta = nullptr, *h_meta = nullptr;
        uint32_t *d_err = nullptr, *h_err = nullptr;
        bool busy = false;
        size_t first = 0;                      // index of the piece's first member in `mem`
    } slot[2];
    hipError_t e = hipSuccess;
    for (auto &s : slot) {
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking);
        for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipEventCreate(&s.ev[i]);
        if (e == hipSuccess) e = hipMalloc((void **)&s.d_in, IN_CAP);
        if (e == hipSuccess) e = hipMalloc((void **)&s.d_out, OUT_CAP);
        if (e == hipSuccess) e = hipMalloc((void **)&s.d_meta, P * sizeof(BgzfMember));
        if (e == hipSuccess) e = hipMalloc((void **)&s.d_err, sizeof(uint32_t));
        if (e == hipSuccess) e = hipHostMalloc((void **)&s.h_meta, P * sizeof(BgzfMember), hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void **)&s.h_err, sizeof(uint32_t), hipHostMallocDefault);
    }
    float total_ms = 0;
    int rc = MSIM_OK;
    // the piece in `s` has finished: its time, its error word
    auto collect = [&](Slot &s) {
        if (!s.busy) return;
        e = wait_stream(s.st);
        if (e != hipSuccess) return;
        s.busy = false;
        float ms = 0;
        if (device_ms && hipEventElapsedTime(&ms, s.ev[0], s.ev[1]) == hipSuccess) total_ms += ms;
        const uint32_t w = *s.h_err;
        if (w != 0xffffffffu && rc == MSIM_OK) {
            const BgzfMemberHost &m = mem[s.first + (w >> 4)];
            rc = fail(c, MSIM_ERR_VALUE, "BGZF input, member at offset " + std::to_string(m.start) + ": " + bgzf_inflate_reason(w & 15u));
        }
    };
    uint64_t out_pos = 0;
    size_t k = 0;
    int turn = 0;
    while (e == hipSuccess && rc == MSIM_OK && k < mem.size()) {
        Slot &s = slot[turn];
        collect(s);                            // (the slot's previous piece: its buffers are free again)
        if (e != hipSuccess || rc != MSIM_OK) break;
        const size_t k1 = std::min(mem.size(), k + P);
        const uint64_t in0 = mem[k].start, in1 = (uint64_t)mem[k1 - 1].payload + mem[k1 - 1].payload_len;
        if (in1 - in0 > IN_CAP) {              // (cannot happen: a member is at most 65 536 bytes and empty ones hold 28)
            size_t q = k + 1;
            while (q < k1 && (uint64_t)mem[q].payload + mem[q].payload_len - in0 <= IN_CAP) q++;
            rc = fail(c, MSIM_ERR_VALUE, "BGZF input, member at offset " + std::to_string(mem[q - 1].start) + ": too many empty members around it");
            break;
        }
        uint32_t o = 0;
        for (size_t q = k; q < k1; q++) {
            s.h_meta[q - k] = BgzfMember{(uint32_t)(mem[q].payload - in0), mem[q].payload_len, o, mem[q].isize, mem[q].crc};
            o += mem[q].isize;
        }
        s.first = k;
        s.busy = true;
        e = hipMemcpyAsync(s.d_in, src + in0, in1 - in0, hipMemcpyHostToDevice, s.st);
        if (e == hipSuccess) e = hipMemcpyAsync(s.d_meta, s.h_meta, (k1 - k) * sizeof(BgzfMember), hipMemcpyHostToDevice, s.st);
        if (e == hipSuccess) e = hipEventRecord(s.ev[0], s.st);
        if (e == hipSuccess) e = bgzf_inflate_device(s.d_in, (uint32_t)(in1 - in0), s.d_meta, (uint32_t)(k1 - k), s.d_out, s.d_err, s.st);
        if (e == hipSuccess) e = hipEventRecord(s.ev[1], s.st);
        if (e == hipSuccess) e = hipMemcpyAsync(s.h_err, s.d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, s.st);
        if (e == hipSuccess) e = hipMemcpyAsync(out + out_pos, s.d_out, o, hipMemcpyDeviceToHost, s.st);
        out_pos += o;
        k = k1;
        turn ^= 1;
    }
    for (int i = 0; i < 2 && e == hipSuccess; i++) collect(slot[turn ^ i]);   // (oldest first: the first failing member is reported)
    // nothing may stay in flight into `out` / out of `src`: after an error or a deadline this wait has no limit
    for (auto &s : slot) if (s.st) (void)hipStreamSynchronize(s.st);
    for (auto &s : slot) {
        for (void *p : {(void *)s.d_in, (void *)s.d_out, (void *)s.d_meta, (void *)s.d_err}) if (p) (void)hipFree(p);
        if (s.h_meta) (void)hipHostFree(s.h_meta);
        if (s.h_err) (void)hipHostFree(s.h_err);
        for (auto x : s.ev) if (x) (void)hipEventDestroy(x);
        if (s.st) (void)hipStreamDestroy(s.st);
    }
    if (device_ms) *device_ms = total_ms;
    if (rc != MSIM_OK) return rc;
    if (e != hipSuccess) return hip_fail(c, e, "BGZF inflate");
    *written = total;
    return MSIM_OK;
}

void device_host_cpus(int device, char *buf, size_t cap) { gpu_node_cpulist(device, buf, cap); }

// `fd` must be something pwrite() can address: a regular file.  MSIM_ERR_UNSUPPORTED otherwise (a pipe, a terminal): the
// caller fetches the text into a buffer and write()s it.
int file_check(Ctx *c, int fd) {
    struct stat sb;
    if (fstat(fd, &sb) != 0) return fail(c, MSIM_ERR_IO, std::string("fstat: ") + strerror(errno));
    if (!S_ISREG(sb.st_mode)) return fail(c, MSIM_ERR_UNSUPPORTED, "output is not a regular file: it cannot be written at an offset");
    return MSIM_OK;
}

// A device buffer of channel `ch` that no queued job reads (waits for the older of the two jobs when both are queued).
// *buf: the buffer's block (grow it with dev_reserve); *slot: for file_enqueue.
int file_text_buffer(Ctx *c, int ch_id, int *slot, DevBlock **buf) {
    FileChannel &ch = io_get(c)->ch[ch_id];
    std::unique_lock<std::mutex> lk(ch.mu);
    ch.cv_done.wait(lk, [&] { return !ch.in_flight[0] || !ch.in_flight[1]; });
    const int s = !ch.in_flight[0] ? 0 : 1;
    *slot = s;
    *buf = &ch.d_buf[s];
    return MSIM_OK;
}

// The first n bytes of the channel's buffer `slot`, complete once everything now on the context's stream has run, go to
// bytes [offset, offset + n) of `fd`.  Returns at once; file_wait() tells when and whether they got there.
int file_enqueue(Ctx *c, int ch_id, int slot, uint64_t n, int fd, uint64_t offset) {
    if (!n) return MSIM_OK;
    FileChannel &ch = io_get(c)->ch[ch_id];
    if (!ch.ready[slot]) MSIM_HIP(c, hipEventCreateWithFlags(&ch.ready[slot], hipEventDisableTiming));
    if (ch.bz) {                                            // BGZF mode: `offset` is the uncompressed stream's length
        if (offset != ch.bz_queued) return fail(c, MSIM_ERR_ARG, "BGZF channel: offset is not the end of the stream");
        MSIM_HIP(c, hipEventRecord(ch.ready[slot], c->stream));
        FileJob job{ch.d_buf[slot].p(), nullptr, slot, n, -1, offset, false, false, nullptr};
        job.bgzf = true;
        return bz_push(c, ch, job);
    }
    MSIM_HIP(c, hipEventRecord(ch.ready[slot], c->stream));
    const int own = dup(fd);
    if (own < 0) return fail(c, MSIM_ERR_IO, std::string("dup: ") + strerror(errno));
    {
        std::lock_guard<std::mutex> lk(ch.mu);
        if (!ch.started) {
            try {
                ch.th = std::thread(channel_main, &ch);
            } catch (const std::system_error &e) {
                (void)close(own);
                return fail(c, MSIM_ERR_NOMEM, std::string("output channel thread: ") + e.what());
            }
            ch.started = true;
        }
        ch.in_flight[slot] = true;
        ch.q.push_back(FileJob{ch.d_buf[slot].p(), nullptr, slot, n, own, offset, false, false, nullptr});
    }
    ch.cv_job.notify_one();
    return MSIM_OK;
}

// Host text [src, src + n) -> bytes [offset, offset + n) of `fd` on the channel's thread.  The caller leaves the text alone
// until file_channel_idle(ch) / file_wait() has returned.
int file_enqueue_host(Ctx *c, int ch_id, const uint8_t *src, uint64_t n, int fd, uint64_t offset) {
    if (!n) return MSIM_OK;
    FileChannel &ch = io_get(c)->ch[ch_id];
    if (ch.bz) {
        if (offset != ch.bz_queued) return fail(c, MSIM_ERR_ARG, "BGZF channel: offset is not the end of the stream");
        FileJob job{nullptr, src, -1, n, -1, offset, false, false, nullptr};
        job.bgzf = true;
        return bz_push(c, ch, job);
    }
    const int own = dup(fd);
    if (own < 0) return fail(c, MSIM_ERR_IO, std::string("dup: ") + strerror(errno));
    {
        std::lock_guard<std::mutex> lk(ch.mu);
        if (!ch.started) {
            try {
                ch.th = std::thread(channel_main, &ch);
            } catch (const std::system_error &e) {
                (void)close(own);
                return fail(c, MSIM_ERR_NOMEM, std::string("output channel thread: ") + e.what());
            }
            ch.started = true;
        }
        ch.q.push_back(FileJob{nullptr, src, -1, n, own, offset, false, false, nullptr});
    }
    ch.cv_job.notify_one();
    return MSIM_OK;
}

// The channel has nothing queued or running (a failure stays recorded for file_wait).
void file_channel_idle(Ctx *c, int ch_id) {
    if (!c->file_io) return;
    FileChannel &ch = c->file_io->ch[ch_id];
    std::unique_lock<std::mutex> lk(ch.mu);
    ch.cv_done.wait(lk, [&] { return ch.q.empty() && !ch.running; });
}

// Everything queued is in its file (or failed: the first failure is reported, once).
int file_wait(Ctx *c) {
    if (!c->file_io) return MSIM_OK;
    int rc = MSIM_OK;
    for (auto &ch : c->file_io->ch) {
        std::unique_lock<std::mutex> lk(ch.mu);
        ch.cv_done.wait(lk, [&] { return ch.q.empty() && !ch.running; });
        if (ch.err && rc == MSIM_OK) {
            rc = ch.err;
            fail(c, ch.err, ch.err_msg);
        }
        ch.err = 0;
        ch.err_msg.clear();
    }
    return rc;
}

void file_io_destroy(Ctx *c) {
    FileIo *io = c->file_io;
    if (!io) return;
    for (auto &ch : io->ch) {
        {
            std::lock_guard<std::mutex> lk(ch.mu);
            ch.stop = true;
        }
        ch.cv_job.notify_all();
        if (ch.th.joinable()) ch.th.join();
        if (ch.bz_fd >= 0) (void)close(ch.bz_fd);
        for (int s = 0; s < 2; s++) {
            if (ch.ready[s]) (void)hipEventDestroy(ch.ready[s]);
            (void)ch.d_buf[s].release();
        }
    }
    delete io;
    c->file_io = nullptr;
}

}  // namespace msim
