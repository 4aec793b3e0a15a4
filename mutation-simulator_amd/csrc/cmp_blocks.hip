// compare --blocks on the device (msim_cmp_counts_blocks; rule in include/msim.h, shared arithmetic in cmp_blocks.h): behind the
// match, the records of both tables are cut into blocks and every block that holds an unmatched record is replayed -- the bytes
// the rewrite writes with the truth's records of the block alone against the bytes it writes with the calls' alone.
//   scan     k_blk_scan: one lane per record of either table (the truth's first).  The lane tests whether its record starts a block
//            -- its predecessor in its own table, a binary search for its predecessor in the other -- and, on a head, walks the
//            block through the merged order: candidate or not, which stop rule ends it, its index ranges.  The head test and the
//            walk are one kernel: a head bit per record would be written by one launch and read once by the next, and the walk
//            needs no bit -- it keeps the largest footprint end and sees the next head as the record that end does not reach.
//            Blocks to replay are appended as descriptors {ia0, ia1, ib0, ib1}: one ballot a wave, its first such lane adds the
//            wave's count to the device counter, every lane stores at its rank.  Their order does not matter: a block's flag
//            stores touch its own records only, and the tallies are sums.
//   replay   k_blk_replay: one lane per descriptor, so a wave is full of working lanes whatever share of the records started a
//            block to replay.  Two cursors are stepped a byte at a time and compared; nothing is buffered.  An equal block's
//            unmatched records get flag byte 2.  Every wave also leaves the bytes its lanes compared and 64 x its longest lane's:
//            the measure of what blocks of different lengths in one wave cost (msim_dbg_cmp_blocks_split).
// Both kernels count into lane-private bins (lane_hist.h).  Every index is checked against its table's size, every base read
// against L, every pool read against the pool (cmp_blocks.h), every descriptor store against the descriptors' allocation.

#include "cmp_blocks.h"
#include "ctx.h"
#include "lane_hist.h"

namespace msim {

namespace {

constexpr int LANES = 256;
constexpr unsigned BLK_MAX_BLOCKS = 2048;
static_assert(HIST_SLOTS == 16, "cmp_blocks.h sizes the counters for 16 slots");
static_assert(blk::TALLIES <= blk::PASS_BINS, "a bin per tally");
static_assert(sizeof(blk::Desc) == sizeof(uint4), "a descriptor is one 16-byte load");

// Both tables together hold fewer than 2^32 records, so fewer than 2^24 passes; beyond BLK_MAX_BLOCKS passes the grid strides, a
// workgroup takes at most 8192 of them and a lane adds at most once per bin and pass: 16 bits hold it.
using BlkHist = LaneHist<(int)blk::PASS_BINS, LANES, 2>;
__device__ __forceinline__ unsigned long long *slot_of(unsigned long long *out) { return out + (blockIdx.x & (HIST_SLOTS - 1)) * blk::PASS_BINS; }

__global__ __launch_bounds__(LANES) void k_blk_scan(cmp::Table A, cmp::Table B, const uint8_t *__restrict__ fa, const uint8_t *__restrict__ fb,
                                                    uint32_t gap, uint64_t n_pass, blk::Desc *__restrict__ desc, uint64_t cap,
                                                    unsigned long long *__restrict__ n_desc, unsigned long long *__restrict__ out) {
    __shared__ BlkHist hist;
    hist.zero();
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t total = A.n + B.n;
    for (uint64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {     // (the same trips for every lane: the ballot below)
        const uint64_t i = pass * LANES + threadIdx.x;
        uint32_t what = blk::NOT_A_CANDIDATE;
        blk::Desc d{};
        if (i < total) {
            const bool truth = i < A.n;
            const uint64_t own = truth ? i : i - A.n;
            uint64_t other;
            if (blk::is_head(truth ? A : B, own, truth ? B : A, truth, gap, &other))
                what = blk::walk(A, B, fa, fb, truth ? own : other, truth ? other : own, gap, &d);
        }
        if (what != blk::NOT_A_CANDIDATE) {
            hist.add(blk::T_CANDIDATE, 1u);
            hist.add(what == blk::REPLAY ? blk::T_REPLAYED : what == blk::OVER_LIMIT ? blk::T_LIMIT : blk::T_TRANSLOCATION, 1u);
        }
        const unsigned long long b = __ballot(what == blk::REPLAY);
        if (b) {
            const int first = __ffsll((long long)b) - 1;
            unsigned long long base = 0;
            if ((int)lane == first) base = atomicAdd(n_desc, (unsigned long long)__popcll(b));
            base = __shfl(base, first, 64);
            const uint64_t at = base + (uint64_t)__popcll(b & ((1ull << lane) - 1));
            if (what == blk::REPLAY && at < cap) reinterpret_cast<uint4 *>(desc)[at] = make_uint4(d.ia0, d.ia1, d.ib0, d.ib1);
        }
    }
    hist.flush(slot_of(out));
}

__global__ __launch_bounds__(LANES) void k_blk_replay(const uint8_t *__restrict__ g, uint64_t L, cmp::Table A, cmp::Table B, uint8_t *__restrict__ fa,
                                                      uint8_t *__restrict__ fb, const blk::Desc *__restrict__ desc, uint64_t cap,
                                                      const unsigned long long *__restrict__ n_desc, unsigned long long *__restrict__ out,
                                                      unsigned long long *__restrict__ steps_out) {
    __shared__ BlkHist hist;
    hist.zero();
    const uint64_t appended = *n_desc, n = appended < cap ? appended : cap;
    for (uint64_t base = (uint64_t)blockIdx.x * LANES; base < n; base += (uint64_t)gridDim.x * LANES) {   // (the same trips for every lane)
        const uint64_t k = base + threadIdx.x;
        uint32_t steps = 0;
        if (k < n) {
            const uint4 w = reinterpret_cast<const uint4 *>(desc)[k];
            const blk::Desc d{w.x, w.y, w.z, w.w};
            if (blk::replay_equal(g, L, A, B, d, &steps)) {
                blk::rescue(fa, fb, d);                    // (replay_equal checked the ranges against both tables)
                hist.add(blk::T_EQUAL, 1u);
            }
        }
        // what divergence leaves of the wave: its lanes' bytes against 64 x its longest lane's, one pair of adds a wave
        unsigned long long sum = steps;
        uint32_t most = steps;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sum += __shfl_xor(sum, o, 64);
            const uint32_t m = __shfl_xor(most, o, 64);
            most = m > most ? m : most;
        }
        if ((threadIdx.x & 63) == 0 && most) {
            atomicAdd(steps_out, sum);
            atomicAdd(steps_out + 1, 64ull * most);
        }
    }
    hist.flush(slot_of(out));
}

}  // namespace

int blocks_enqueue(Ctx *c, hipStream_t stream, const uint8_t *g, uint64_t L, const cmp::Table &A, const cmp::Table &B, uint8_t *fa,
                   uint8_t *fb, uint32_t gap, blk::Desc *desc, uint64_t cap, unsigned long long *out, hipEvent_t between) {
    const uint64_t total = A.n + B.n;
    if (!total) return MSIM_OK;
    const auto [n_pass, grid] = pass_grid(total, LANES, BLK_MAX_BLOCKS);
    unsigned long long *n_desc = out + blk::PASS_COUNT_AT;
    hipLaunchKernelGGL(k_blk_scan, grid, dim3(LANES), 0, stream, A, B, (const uint8_t *)fa, (const uint8_t *)fb, gap, n_pass, desc, cap, n_desc, out);
    MSIM_HIP(c, hipGetLastError());
    if (between) MSIM_HIP(c, hipEventRecord(between, stream));
    hipLaunchKernelGGL(k_blk_replay, grid, dim3(LANES), 0, stream, g, L, A, B, fa, fb, (const blk::Desc *)desc, cap,
                       (const unsigned long long *)n_desc, out, out + blk::PASS_STEPS_AT);
    MSIM_HIP(c, hipGetLastError());
    return MSIM_OK;
}

}  // namespace msim
