// Host arithmetic every PLAN engine shares: the sampling distance, what a range's type draw can produce, and how many words of the
// CPython stream its samples and randint draws may consume -- the engines' stream windows, hence what gpu_plan_make_room finds
// room for.  Host only: nothing of HIP in here.
#pragma once
#include <algorithm>
#include <cmath>
#include "../../include/msim.h"
#include "mt19937.h"

namespace msim {

// sampling distance d = min(mut_block.values()); population of random.sample(range(start, stop - (k - 1) d), k)  (util.py:104)
inline int64_t min_block(const msim_params &P) { return *std::min_element(P.block + 1, P.block + 8); }
inline int64_t range_population(const msim_range &r, int64_t d) { return (r.stop - (r.k - 1) * d) - r.start; }

// Can the type draw of this range produce entry j, and with which probability?  (thresholds are cumulative: entry j is drawn iff
// thr[j-1] < thr[j], with thr[-1] = 0, and only below 2^53)
inline bool type_drawable(const msim_range &r, int j) {
    const uint64_t lo = j ? r.cdf_thr[j - 1] : 0;
    return r.cdf_thr[j] > lo && lo < (1ull << 53);
}
inline double type_probability(const msim_range &r, int j) {     // (of a drawable entry)
    return (double)(std::min<uint64_t>(r.cdf_thr[j], 1ull << 53) - (j ? r.cdf_thr[j - 1] : 0)) / 9007199254740992.0;
}
// the type draw is deterministic SN: every threshold 0 or >= 2^53, and the first entry above 0 is the SNP
inline bool range_is_deterministic_sn(const msim_range &r) {
    if (r.n_types < 1 || r.n_types > 8) return false;
    int zeros = 0;
    for (int j = 0; j < r.n_types; j++) {
        if (r.cdf_thr[j] == 0) zeros++;
        else if (r.cdf_thr[j] < (1ull << 53)) return false;
    }
    return zeros < r.n_types && r.types[zeros] == MSIM_SN;
}

// _randbelow(n) accepts a getrandbits(bit_length(n)) word with probability n / 2^bits
inline double randbelow_acceptance(double n) { return n / (double)(1ull << bit_length64((uint64_t)n)); }
// Accepted draws until the set path of random.sample(range(n), k) holds k distinct values: -n ln(1 - k/n) (coupon collector),
// infinite at k == n.  _bounded is what a sum over ranges takes: n ln n < 64 n for every n below 2^64.
inline double set_path_need(double n, double k) { return -n * std::log1p(-k / n); }
inline double set_path_need_bounded(double n, double k) { return k >= n ? 64.0 * k : set_path_need(n, k); }
// Word window of one big set-path sample (a window of its own: enqueue_sample_chain, enqueue_sample_ahead): `need` accepted draws
// with a 16-sigma margin, that many over the acceptance with 16 sigma again.  The caller refuses >= 4e9 and casts.
inline double big_sample_window(double n, double need) {
    const double p_acc = randbelow_acceptance(n), target = need + 16.0 * std::sqrt(need) + 4096.0;
    return target / p_acc + 16.0 * std::sqrt(target) / p_acc + 8192.0;
}

// Mean and a variance BOUND of the words one small or pool-path sample consumes; the host-cut and host-chain engines and
// gpu_plan_make_room sum them over thousands of ranges into one window of mean + 16 sigma.  Pool path (n <= setsize): fewer than
// 2 words per draw.  Set path: the rejections' term, 4 (need - k) / p^2 for the duplicates and need / p on top.
// Not sample_words_moments (plan_gpu.h): that is the EXACT variance of one big sample, which the anchored windows need because they
// lay out an interval on both sides of the mean and diverges at k == n; here only an upper end is laid out, k may reach n and an
// over-estimate costs a few words.
struct StreamMoments { double e, v; };
inline StreamMoments small_sample_moments(double n, double k, double setsize) {
    if (n <= setsize) return StreamMoments{2.0 * k, 2.0 * k};
    const double p_acc = randbelow_acceptance(n), need = set_path_need_bounded(n, k);
    return StreamMoments{need / p_acc, need * (1.0 - p_acc) / (p_acc * p_acc) + 4.0 * (need - k) / (p_acc * p_acc) + need / p_acc};
}

// Word window of n randint draws of acceptance >= acc (the boundary pass: one per non-SNP candidate), 16 sigma
inline double randint_window(double n, double acc) { return n / acc + 16.0 * std::sqrt(n) / acc + 4096.0; }
// Least acceptance of randint(min_len, max_len) among the types this range draws a length for (TLI draws none).  A width outside
// 1 .. 2^32 - 1 is skipped: the SV-mix engine's eligibility refuses it, and so does chain_classes_add (plan_host.cpp: 1 <= w < 2^24
// for every drawable IN/DE/DU/IV/TL) for every range the host-chain engine gets from multimix_prepare.
inline double randint_acceptance_min(const msim_range &r) {
    double acc = 1.0;
    for (int j = 0; j < r.n_types; j++) {
        const int t = r.types[j];
        if (t == MSIM_SN || t == MSIM_TLI || !type_drawable(r, j)) continue;
        const int64_t w = r.max_len[t] - r.min_len[t] + 1;
        if (w >= 1 && w < (1ll << 32)) acc = std::min(acc, randbelow_acceptance((double)w));
    }
    return acc;
}

}  // namespace msim
