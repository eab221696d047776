// gm_fit_reduce.hpp -- the fixed-grid fp64 reduction of the streaming least-squares kernels: k_cylfit.hip (the cylinder
// regression) and k_wall_locate.hip (the pose correction against the wall map).  A launch runs on kFitBlocks x
// kFitThreads; a block's sums go to its own partial row, and the block that takes the last ticket reduces the rows of the
// grid in a fixed order, so the order of every sum depends on neither the point count nor the launch site.
#pragma once

#include "gm_internal.hpp"

namespace gm {

constexpr int kFitThreads = 256;
constexpr int kFitCols = kFitRowLen;   // a partial row, zero padded behind a kernel's own sums
constexpr int kFitUnroll = 4;          // points per thread and trip, loads issued together

// the block's sums -> its partial row; then the ticket.  Returns true in every thread of the block that finished last,
// after the rows of the whole grid have been reduced (fixed order) into tot[0..kFitCols).  partial: [gridDim.x][kFitCols],
// gridDim.x <= kFitBlocks; ticket: 0 between launches.
template <int NACC>
__device__ inline bool fit_block_reduce(double *partial, uint32_t *ticket, const double (&acc)[NACC], double *tot)
{
    static_assert(NACC <= kFitCols, "a partial row holds kFitCols sums");
    __shared__ double red[kFitThreads / kWave][kFitCols];
    __shared__ uint32_t last;
    const int w = threadIdx.x / kWave;
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        const double r = wave_sum(acc[k]);
        if (lane_id() == 0) red[w][k] = r;
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)kFitCols) {
        double r = 0.0;
        if ((int)threadIdx.x < NACC)
#pragma unroll
            for (int j = 0; j < kFitThreads / kWave; ++j) r += red[j][threadIdx.x];
        partial[(size_t)blockIdx.x * kFitCols + threadIdx.x] = r;   // blockIdx.x < gridDim.x <= kFitBlocks rows
        __threadfence();
    }
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1u ? 1u : 0u;
    __syncthreads();
    if (!last) return false;
    __threadfence();
    // fixed-order reduction of the gridDim.x rows: thread t sums rows t, t + 256, ... (a row's columns are independent
    // loads, all in flight together: a serial chain of dependent row loads cost ~30 us per launch), then wave_sum and
    // the waves in order
    double v[kFitCols];
#pragma unroll
    for (int k = 0; k < kFitCols; ++k) v[k] = 0.0;
    for (uint32_t b = threadIdx.x; b < gridDim.x; b += kFitThreads) {
        const double *row = partial + (size_t)b * kFitCols;
#pragma unroll
        for (int k = 0; k < NACC; ++k) v[k] += row[k];
    }
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        const double r = wave_sum(v[k]);
        if (lane_id() == 0) red[w][k] = r;   // (every thread of the block is past the reads of red above)
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)kFitCols) {
        double t = 0.0;
        if ((int)threadIdx.x < NACC)
#pragma unroll
            for (int j = 0; j < kFitThreads / kWave; ++j) t += red[j][threadIdx.x];
        tot[threadIdx.x] = t;
    }
    if (threadIdx.x == 0) atomicExch(ticket, 0u);   // ready for the next launch
    __syncthreads();
    return true;
}

}  // namespace gm
