// The round trip of a counting pass's counters (compare.hip, cmp_regions.hip, cmp_phase.hip, spectrum.hip): a small block of
// 64-bit counters on the device, its pinned mirror and the event pair that times the kernels between the two calls --
//   begin     the first `words` counters zeroed on the context's stream, the timed stretch begun behind the zeroing
//   finish    the stretch ended IN FRONT of the copy (the time covers the kernels alone), the counters copied to the mirror, the
//             stream waited for, the time added to *acc
// begin() remembers its count and the copy uses it: a pass cannot zero one layout and fetch another.  A pass with more than one
// timed stretch (compare --blocks) ends `tm` itself and calls copy_wait(); its further event pairs stay with the pass.
#pragma once
#include "ctx.h"

namespace msim {

struct CounterTrip {                           // (move-only through its blocks, and never moved: a state struct holds it)
    Scratch<unsigned long long> d;
    Pinned<unsigned long long> h;              // valid behind finish() / copy_wait(): the counters begin() zeroed
    EventPair tm;
    size_t words = 0;                          // of the trip under way

    ~CounterTrip() { destroy(); }
    explicit operator bool() const { return tm.e1 != nullptr; }    // whole: create() leaves nothing behind where it fails
    hipError_t create(size_t cap_words) {
        hipError_t e = dev_alloc(d, cap_words * sizeof(unsigned long long));
        if (e == hipSuccess) e = pin_alloc(h, cap_words * sizeof(unsigned long long));
        if (e == hipSuccess) e = tm.create();
        if (e != hipSuccess) destroy();
        return e;
    }
    void destroy() { (void)d.release(); (void)h.release(); tm.destroy(); }
    int begin(Ctx *c, size_t n) {
        if (n * sizeof(unsigned long long) > d.cap) return fail(c, MSIM_ERR_HIP, "internal: a counting pass asks for more counters than its block holds");
        words = n;
        MSIM_HIP(c, hipMemsetAsync(d.p(), 0, n * sizeof(unsigned long long), c->stream));
        MSIM_HIP(c, tm.begin(c->stream));
        return MSIM_OK;
    }
    int copy_wait(Ctx *c) {
        MSIM_HIP(c, hipMemcpyAsync(h.p(), d.p(), words * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        MSIM_HIP(c, wait_stream(c->stream));
        return MSIM_OK;
    }
    int finish(Ctx *c, double *acc) {
        MSIM_HIP(c, tm.end(c->stream));
        const int rc = copy_wait(c);
        return rc ? rc : tm.add_elapsed(c, acc);
    }
};

// A pass's state, made on first use with its trip `out` of `words` counters; the slot is filled once the state is whole.
template <class State>
int lazy_state(Ctx *c, State **slot, size_t words, const char *what) {
    if (*slot) return MSIM_OK;
    State *s = new State;
    const hipError_t e = s->out.create(words);
    if (e != hipSuccess) { delete s; return hip_fail(c, e, what); }
    *slot = s;
    return MSIM_OK;
}

}  // namespace msim
