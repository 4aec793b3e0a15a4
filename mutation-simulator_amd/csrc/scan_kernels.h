// The generic u32 exclusive scan of the device engines (plan_kernels.h: the samplers' counts; haplotype.hip: the kept records
// of a haplotype's blocks).  gfx950 (MI355X) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msim {

namespace {

// ------------------------------------------------------------------ generic u32 exclusive scan
// in place over a[0..n), total to a[n]; single workgroup (these scans sit on the stream-position critical
// path, so: wave scan by shuffles, two barriers per round; a round covers 4096 items, or 16384 when more than
// one round of 4096 would be needed -- the loads of a round are independent, so the longer round costs one
// memory latency, not four)
template <int ITEMS, int WAVES = 16>
__device__ __forceinline__ void scan_rounds(uint32_t *__restrict__ a, uint32_t n, uint32_t *wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += 64 * WAVES * ITEMS) {
        const uint32_t i0 = base + threadIdx.x * ITEMS;
        uint32_t v[ITEMS];
        uint32_t mine = 0;
#pragma unroll
        for (int q = 0; q < ITEMS; q++) { v[q] = i0 + q < n ? a[i0 + q] : 0; mine += v[q]; }
        uint32_t incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t pre = carry, total = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) {
            const uint32_t t = wsum[w];
            if (w < wave) pre += t;
            total += t;
        }
        uint32_t run = pre + incl - mine;
#pragma unroll
        for (int q = 0; q < ITEMS; q++) {
            if (i0 + q < n) a[i0 + q] = run;
            run += v[q];
        }
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) a[n] = carry;
}

__global__ __launch_bounds__(1024) void k_scan_u32(uint32_t *__restrict__ a, uint32_t n) {
    __shared__ uint32_t wsum[16];
    if (n <= 4096) scan_rounds<4>(a, n, wsum);
    else scan_rounds<16>(a, n, wsum);
}

}  // namespace

}  // namespace msim
