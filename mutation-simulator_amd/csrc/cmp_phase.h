// compare --diploid --phased ("switch and flip errors against a phased truth"): what the device kernels (cmp_phase.hip) and the
// sequential host restatement (msim_dbg_cmp_phase) share -- the rules of include/msim.h, integer arithmetic only.
//
//   informative   a truth record whose flag byte is 1, whose genotype byte is 1 or 2 and whose word is nonzero, with a partner
//                 (cmp::partner, the match's own) whose word is nonzero: a PAIR, key (truth word, calls word), orientation o
//   Scan          the monoid the device scans over the dense sequence of pairs -- per prefix the last block start, the pairs
//                 with o = 1 since it, the last pair without a raw switch bit: a block's size and Hamming distance are read at its
//                 last pair, a switch run's length at its last bit
//   tally_run     r consecutive raw switch bits: r / 2 flips, r % 2 switches
// The host restatement does not scan: it walks the pairs with a handful of counters.
#pragma once
#include "compare.h"

namespace msim {
namespace phase {

// out[MSIM_CMP_PHASE_COUNTS] of msim_cmp_phase_counts
constexpr uint32_t C_TRUTH_HETS = 0, C_CALLS_HETS = 1, C_PAIRS = 2, C_BLOCKS = 3, C_SINGLETONS = 4, C_ASSESSED = 5, C_RAW = 6,
                   C_SWITCHES = 7, C_FLIPS = 8, C_HAMMING = 9, C_PAIRS_BLOCKED = 10, COUNTS = 11;
static_assert(COUNTS == MSIM_CMP_PHASE_COUNTS, "msim.h and cmp_phase.h must agree on the counts");
// a truth record's state byte (msim_cmp_fetch_phase)
constexpr uint8_t ST_INFORMATIVE = 1, ST_SWITCH = 2, ST_ORIENTATION = 4;

MSIM_FHD inline bool het(uint32_t gt) { return gt == 1u || gt == 2u; }
// a phased het: what the two "phased hets" counters count, and the part of `informative` a record decides alone
MSIM_FHD inline bool phased_het(uint32_t gt, uint32_t word) { return het(gt) && word != 0u; }

// The state byte of truth record i before the tally (0, or ST_INFORMATIVE with its orientation); *key_b: its partner's word.
// flag: the record's flag byte of msim_cmp_counts_diploid with the same `exact`.
MSIM_FHD inline uint8_t pair_state(const uint8_t *g, uint64_t L, const cmp::Table &A, uint64_t i, const cmp::Table &B, bool exact, uint32_t flag,
                                   const uint8_t *gt_a, const uint8_t *gt_b, const uint32_t *w_a, const uint32_t *w_b, uint32_t *key_b) {
    *key_b = 0;
    const uint32_t gt = gt_a[i];
    if (flag != 1u || !phased_het(gt, w_a[i])) return 0;
    cmp::Span s;
    const int64_t j = cmp::partner(g, L, A, i, B, exact, &s);
    if (j < 0 || (uint64_t)j >= B.n) return 0;
    const uint32_t wb = w_b[j];
    if (wb == 0u) return 0;
    *key_b = wb;
    return (uint8_t)(ST_INFORMATIVE | (gt_b[j] != gt ? ST_ORIENTATION : 0));
}

// a run of r raw switch bits
MSIM_FHD inline uint64_t run_flips(uint64_t r) { return r >> 1; }
MSIM_FHD inline uint64_t run_switches(uint64_t r) { return r & 1u; }

// One prefix of the dense sequence.  Indices are stored + 1 (0: none in the prefix); fewer than 2^31 pairs exist.
struct Scan {
    uint32_t block;        // 1 + the index of the last pair that starts a block
    uint32_t ones;         // pairs with o = 1 from that pair on (none: in the whole prefix)
    uint32_t calm;         // 1 + the index of the last pair without a raw switch bit
};
// a, then b (associative; Scan{0, 0, 0} is the identity)
MSIM_FHD inline Scan join(const Scan &a, const Scan &b) {
    return Scan{b.block ? b.block : a.block, b.block ? b.ones : a.ones + b.ones, b.calm ? b.calm : a.calm};
}
// pair k of the dense sequence: starts: it starts a block; sw: it carries a raw switch bit
MSIM_FHD inline Scan element(uint32_t k, bool starts, uint32_t o, bool sw) { return Scan{starts ? k + 1u : 0u, o, sw ? 0u : k + 1u}; }

}  // namespace phase

struct Ctx;
struct PhaseState;
// compare.hip: a side's diploid table of a contig as the phase pass sees it (have: msim_cmp_join made one), and what the last
// msim_cmp_counts_diploid of the contig left (counted, with which flags)
struct DipView {
    bool have;
    cmp::Table t;
    const uint8_t *gt, *flag;
};
bool compare_dip_view(Ctx *c, int contig, int side, DipView *v, bool *counted, uint32_t *counted_flags);
// compare.hip: where the compare state keeps the phase pass's (made on first use; the compare state is made with it)
int compare_phase_slot(Ctx *c, PhaseState ***slot);
// cmp_phase.hip, called where the diploid tables go: one side's words (a new join), a contig's words and marks (contig < 0: every
// contig's), the state itself, its timing
void phase_drop_side(PhaseState *P, int contig, int side);
void phase_drop(PhaseState *P, int contig);
void phase_state_destroy(PhaseState *P);
void phase_reset_timing(PhaseState *P);

// vcf_parse.hip: the table the context's last msim_vcf_plan_contig left, where that was a consensus-grammar plan of `contig` on
// the device whose text is still loaded and whose table is still the contig's -- the text, its line starts and tab counts, the
// line (within the group) of every record
struct VcfPlanView {
    const uint8_t *text;
    const uint64_t *ls;
    const uint32_t *tabcum, *recline;
    uint64_t first, n_lines, n_rec;
    uint32_t nf0, sample;
};
bool vcf_last_plan(const Ctx *c, int contig, VcfPlanView *v);

}  // namespace msim
