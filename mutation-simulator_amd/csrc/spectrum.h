// Context-dependent SNPs ("--spectrum"): what the device kernels (spectrum.hip) and the sequential host restatements
// (msim_dbg_context_counts, msim_dbg_spectrum_plan) share.  Integer arithmetic only.
//
//   census   code(A, C, G, T) = 0..3, every other byte is invalid; site p is ELIGIBLE iff 1 <= p <= L - 2 and b[p-1], b[p],
//            b[p+1] are valid; ctx = 16 code(b[p-1]) + 4 code(b[p]) + code(b[p+1]); counts[ctx] over the eligible sites
//   draw     site p of the contig with ordinal seq: v = Philox4x32-10 (x = p >> 1, y = 0, seq, TAG_CTX) under the run's key,
//            r = the high 64 bits of v for an odd p, the low 64 for an even one -- one call serves two sites;
//            j = #{i in 0..2 : thr[3 ctx + i] <= r}; j == 3: no mutation, else the record {p, p, 0, MSIM_SN, aux = j, 0}
// The 192 thresholds are the caller's: cumulative probabilities of the three alternative bases per context, scaled by 2^64
// (mutation_simulator_amd/spectrum.py evaluates them in exact rational arithmetic).
#pragma once
#include <stdint.h>

#include "fast_math.h"

namespace msim {
namespace spectrum {

constexpr uint32_t SITES_PER_LANE = 16;                    // one 16-byte load
constexpr uint32_t TILE_LANES = 256;
constexpr uint32_t TILE = SITES_PER_LANE * TILE_LANES;     // bases of one workgroup of the sampler == MSIM_SPECTRUM_TILE
constexpr uint32_t CODE_INVALID = 4;

// A 0x41, C 0x43, G 0x47, T 0x54: bits 1 and 2 tell them apart, and the letter at the code found is the check
MSIM_FHD inline uint32_t base_code(uint32_t b) {
    const uint32_t code = ((b >> 1) ^ (b >> 2)) & 3u;
    return ((0x54474341u >> (8 * code)) & 0xffu) == b ? code : CODE_INVALID;
}

// the outcome of one site: 0..2 = the SN record's aux, 3 = no mutation.  thr: the context's three thresholds, non-decreasing
MSIM_FHD inline uint32_t outcome(const uint64_t *thr3, uint64_t r) {
    return (uint32_t)(thr3[0] <= r) + (uint32_t)(thr3[1] <= r) + (uint32_t)(thr3[2] <= r);
}

// The SBS-96 channel of an SN record in a valid context (msim_sbs_counts): substitution-major (C>A, C>G, C>T, T>A, T>C, T>G), then
// the 5' base, then the 3' base, pyrimidine-centred -- a purine centre is read off the other strand (3 - code complements).
// l, m, r: the codes of b[p-1], b[p], b[p+1]; aux 0..2: the rewrite's alternative (A>G,T,C  C>T,A,G  G>A,C,T  T>C,G,A).
// The substitution of (m, aux) sits in nibble 4 m + aux of the constant.
MSIM_FHD inline uint32_t sbs_channel(uint32_t l, uint32_t m, uint32_t r, uint32_t aux) {
    const uint32_t sub = (uint32_t)(0x0354001201020534ull >> (4 * (4 * m + aux))) & 7u;
    const bool purine = (m & 1u) == 0;
    return 16 * sub + 4 * (purine ? 3 - r : l) + (purine ? 3 - l : r);
}
constexpr uint32_t SBS_BINS = 96 + 8;                      // the channels, then msim_sbs_counts' tallies

MSIM_FHD inline uint64_t site_bits(const fastrng::U4 &v, uint64_t p) { return (p & 1) ? fastrng::hi64(v) : fastrng::lo64(v); }

}  // namespace spectrum
}  // namespace msim
