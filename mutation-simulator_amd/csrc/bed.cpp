// msim_bed_scan: BED text into intervals and runs of one name, one sequential pass (include/msim.h) -- no context, no GPU.  A
// stratification BED holds 1.5 M lines: a Python split of it would cost several times the whole compare command.
#include <cstdint>
#include <cstring>
#include <string>

#include "ctx.h"

using namespace msim;

namespace {

inline bool blank(uint8_t b) { return b == '\t' || b == ' '; }
inline bool begins(const uint8_t *p, uint64_t n, const char *word) {
    const size_t w = strlen(word);
    return n >= w && memcmp(p, word, w) == 0;
}
// decimal digits only, at most 4294967295
inline bool number(const uint8_t *p, uint64_t n, uint32_t *out) {
    if (!n) return false;
    uint64_t v = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (p[i] < '0' || p[i] > '9') return false;
        v = v * 10 + (uint64_t)(p[i] - '0');
        if (v > 0xFFFFFFFFull) return false;
    }
    *out = (uint32_t)v;
    return true;
}
int refuse(uint64_t line, const char *why) { return fail(nullptr, MSIM_ERR_VALUE, "BED line " + std::to_string(line) + ": " + why); }

}  // namespace

extern "C" int msim_bed_scan(const uint8_t *text, uint64_t n_text, uint32_t *starts, uint32_t *ends, uint64_t *lines, uint64_t *n_intervals,
                             uint64_t *run_name_off, uint32_t *run_name_len, uint64_t *run_first, uint64_t *run_count, uint64_t *n_runs) {
    if ((!text && n_text) || !n_intervals || !n_runs) return MSIM_ERR_ARG;
    const bool sizing = !starts && !ends && !lines && !run_name_off && !run_name_len && !run_first && !run_count;
    if (!sizing && (!starts || !ends || !lines || !run_name_off || !run_name_len || !run_first || !run_count)) return MSIM_ERR_ARG;
    const uint64_t cap_iv = *n_intervals, cap_run = *n_runs;
    uint64_t n_iv = 0, n_run = 0, line = 0, at = 0;
    uint64_t name_off = 0, name_len = 0;                   // the name of the run being written (none yet: n_run == 0)
    while (at < n_text) {
        const uint8_t *nl = static_cast<const uint8_t *>(memchr(text + at, '\n', (size_t)(n_text - at)));
        const uint64_t next = nl ? (uint64_t)(nl - text) + 1 : n_text;
        uint64_t end = nl ? next - 1 : n_text;
        if (nl && end > at && text[end - 1] == '\r') end--;
        const uint8_t *p = text + at;
        const uint64_t n = end - at, off = at;
        at = next;
        line++;
        if (!n || p[0] == '#' || begins(p, n, "track") || begins(p, n, "browser")) continue;
        uint64_t f_at[3], f_len[3], k = 0;
        int fields = 0;
        while (fields < 3) {
            while (k < n && blank(p[k])) k++;
            if (k == n) break;
            f_at[fields] = k;
            while (k < n && !blank(p[k])) k++;
            f_len[fields] = k - f_at[fields];
            fields++;
        }
        if (fields < 3) return refuse(line, "fewer than three fields");
        uint32_t s, e;
        if (!number(p + f_at[1], f_len[1], &s)) return refuse(line, "start is no number");
        if (!number(p + f_at[2], f_len[2], &e)) return refuse(line, "end is no number");
        if (e < s) return refuse(line, "end in front of start");
        if (e == s) continue;
        if (!n_run || f_len[0] != name_len || memcmp(text + name_off, p + f_at[0], (size_t)name_len) != 0) {
            name_off = off + f_at[0];
            name_len = f_len[0];
            if (name_len > 0xFFFFFFFFull) return refuse(line, "fewer than three fields");   // (a name of 4 GiB is no name)
            if (!sizing) {
                if (n_run >= cap_run) return fail(nullptr, MSIM_ERR_ARG, "msim_bed_scan: more runs than the arrays hold");
                run_name_off[n_run] = name_off;
                run_name_len[n_run] = (uint32_t)name_len;
                run_first[n_run] = n_iv;
                run_count[n_run] = 0;
            }
            n_run++;
        }
        if (!sizing) {
            if (n_iv >= cap_iv) return fail(nullptr, MSIM_ERR_ARG, "msim_bed_scan: more intervals than the arrays hold");
            starts[n_iv] = s;
            ends[n_iv] = e;
            lines[n_iv] = line;
            run_count[n_run - 1]++;
        }
        n_iv++;
    }
    *n_intervals = n_iv;
    *n_runs = n_run;
    return MSIM_OK;
}
