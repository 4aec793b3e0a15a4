// The counting kernels' histogram (k_ctx_census, k_sbs_count, k_cmp_match<>, k_cmp_tally<>, k_region_tally<>, k_blk_scan,
// k_blk_replay): BINS 16-bit counters per LANE in LDS.
//   columns   every lane owns column threadIdx.x of `cnt`, two bins to a 32-bit word: no two lanes share a word and a wave's 64
//             adds go to 64 different banks, so an add is one conflict-free ds_add whatever the data holds -- a homopolymer
//             run or a one-channel table costs what random input costs.  A lane zeroes its own column: no barrier before its adds.
//             16 bits must hold what ONE lane adds to one bin over the workgroup's life: every kernel says at its pass loop
//             why they do (its grid cap bounds the passes a workgroup takes).
//   flush     PARTS x BINS threads sum bin b over LANES / PARTS columns each, reading them rotated by the thread index: a wave's
//             64 reads stay on 64 banks.  Then one device-scope add per non-zero bin and workgroup into `out`.
//   slots     the caller chooses `out`: HIST_SLOTS copies of the result, workgroup w adding to copy w & 15, and the host sums
//             them (hist_sum_slots) once the counters are back (counter_trip.h).  On one copy, 96 busy bins cost 96 adds to the same few lines per workgroup and the time
//             depended on the data (NOTES 21: 0.873 ms one channel, 1.095 ms a real spectrum).  The census keeps its one copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace msim {

constexpr int HIST_SLOTS = 16;

// (aligned as a __shared__ array of its own would be: without it the flush's unwrapped reads come out as eight ds_read2_b32 in
// place of four ds_read_b128, NOTES 23)
template <int BINS, int LANES, int PARTS>
struct alignas(16) LaneHist {
    static constexpr int WORDS = BINS / 2, COLS = LANES / PARTS;
    static_assert(BINS % 2 == 0, "two counters a word");
    static_assert(PARTS * BINS <= LANES, "the flush has one thread per bin and part");
    static_assert(COLS * PARTS == LANES && (COLS & (COLS - 1)) == 0, "the rotation masks a part's columns");
    uint32_t cnt[WORDS][LANES];
    uint32_t part[PARTS][BINS];

    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int w = 0; w < WORDS; w++) cnt[w][threadIdx.x] = 0;
    }
    __device__ __forceinline__ void add(uint32_t bin, uint32_t one) { atomicAdd(&cnt[bin >> 1][threadIdx.x], one << (16 * (bin & 1))); }
    __device__ __forceinline__ void flush(unsigned long long *__restrict__ out) {
        __syncthreads();
        if (threadIdx.x < PARTS * BINS) {
            const int p = (int)threadIdx.x / BINS, bn = (int)threadIdx.x - p * BINS;
            uint32_t s = 0;
#pragma unroll 8
            for (int i = 0; i < COLS; i++) s += (cnt[bn >> 1][p * COLS + ((i + (int)threadIdx.x) & (COLS - 1))] >> (16 * (bn & 1))) & 0xffffu;
            part[p][bn] = s;
        }
        __syncthreads();
        if (threadIdx.x < BINS) {
            uint32_t total = 0;
#pragma unroll
            for (int p = 0; p < PARTS; p++) total += part[p][threadIdx.x];
            if (total) atomicAdd(&out[threadIdx.x], (unsigned long long)total);
        }
    }
};

// host: bins[i] = the sum of slots[s * stride + i] over the HIST_SLOTS copies
inline void hist_sum_slots(const unsigned long long *slots, size_t stride, unsigned long long *bins, size_t n_bins) {
    for (size_t i = 0; i < n_bins; i++) bins[i] = 0;
    for (int s = 0; s < HIST_SLOTS; s++)
        for (size_t i = 0; i < n_bins; i++) bins[i] += slots[(size_t)s * stride + i];
}

// host: the grid of a kernel with a pass loop -- n records in passes of `pass`, at most `cap` workgroups, which stride beyond that
struct PassGrid { uint64_t n_pass; dim3 grid; };
inline PassGrid pass_grid(uint64_t n, uint32_t pass, unsigned cap) {
    const uint64_t n_pass = (n + pass - 1) / pass;
    return PassGrid{n_pass, dim3((unsigned)(n_pass < cap ? n_pass : cap))};
}

}  // namespace msim
