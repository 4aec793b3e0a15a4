// compare --regions / --stratify ("score inside BED intervals"): what the device kernels (cmp_regions.hip) and the sequential host
// restatement (msim_dbg_cmp_counts_regions) share -- the rule of include/msim.h, integer arithmetic only.
//
//   Set        a contig's region set in normal form: n half-open intervals [starts[k], ends[k]), start < end <= L,
//              starts[k] > ends[k - 1]
//   anchor     the position a record is judged by: an IN / DE record's leftmost placement (cmp::interval's lo, the match's own
//              walk); exact, and every other type: its pos
//   inside     is the anchor inside the set: an upper-bound binary search over starts, then anchor < ends[k] of the interval in
//              front -- starts / ends are read inside [0, n) only
//   mark_of    a record's mark byte: bit s set iff its anchor is inside set s (one walk for all sets)
#pragma once
#include "compare.h"

namespace msim {
namespace rgn {

constexpr uint32_t SETS = MSIM_CMP_REGION_SETS;
static_assert(SETS == 8, "a mark is one byte: a bit per resident set");

struct Set { const uint32_t *starts, *ends; uint64_t n; };
struct Sets { Set s[SETS]; uint32_t resident; };           // resident: bit s set iff s[s] is a set (an empty one included)

MSIM_FHD inline uint32_t anchor(const uint8_t *g, uint64_t L, const cmp::Rec &r, const uint8_t *pool, uint64_t pool_len, bool exact) {
    return cmp::indel(r.type) ? cmp::interval(g, L, r, pool, pool_len, exact).lo : r.pos;
}

MSIM_FHD inline bool inside(const Set &set, uint32_t at) {
    uint64_t lo = 0, hi = set.n;                           // the first interval that starts behind `at`
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (set.starts[mid] <= at) lo = mid + 1; else hi = mid;
    }
    return lo > 0 && at < set.ends[lo - 1];
}

MSIM_FHD inline uint8_t mark_of(const uint8_t *g, uint64_t L, const cmp::Rec &r, const uint8_t *pool, uint64_t pool_len, bool exact,
                                const Sets &sets) {
    if (!cmp::known_type(r.type)) return 0;
    const uint32_t at = anchor(g, L, r, pool, pool_len, exact);
    uint32_t m = 0;
    for (uint32_t s = 0; s < SETS; s++)
        if (((sets.resident >> s) & 1u) && inside(sets.s[s], at)) m |= 1u << s;
    return (uint8_t)m;
}

// a list in normal form on a contig of L bases?
inline bool normal_form(const uint32_t *starts, const uint32_t *ends, uint64_t n, uint64_t L) {
    for (uint64_t k = 0; k < n; k++)
        if (starts[k] >= ends[k] || ends[k] > L || (k && starts[k] <= ends[k - 1])) return false;
    return true;
}

}  // namespace rgn

struct Ctx;
struct RegionState;
// compare.hip: the two tables a region call works on and what the last count call over them left -- held and current (the
// contig planned, the current table the one that was counted), or with `diploid` the two diploid tables
struct RegionTables {
    cmp::Table t[2];                           // MSIM_CMP_TRUTH, MSIM_CMP_CALLS
    const uint8_t *flag[2];                    // the flag bytes of the last count call (counted)
    bool counted;
    int outcomes;                              // of that call: 2 (msim_cmp_counts), 3 (msim_cmp_counts_blocks / _diploid)
    uint32_t counted_flags;                    // its MSIM_CMP_EXACT bit
    uint64_t table_gen;                        // the contig's table generation (held / current only)
};
// why: what is missing, for the refusal
bool compare_region_tables(Ctx *c, int contig, bool diploid, RegionTables *v, const char **why);
// compare.hip: where the compare state keeps the region state (made on first use; the compare state is made with it)
int compare_region_slot(Ctx *c, RegionState ***slot);
// cmp_regions.hip, called where the tables go: a contig's marks (a new hold or join), a contig's sets and marks (contig < 0: every
// contig's), the state itself, its timing
void regions_unmark(RegionState *R, int contig);
void regions_drop(RegionState *R, int contig);
void regions_state_destroy(RegionState *R);
void regions_reset_timing(RegionState *R);

}  // namespace msim
