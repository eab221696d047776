// gm_point_stream.hpp -- what the kernels that bin the valid cloud share (k_surface_map, k_wall_add*, k_wall_align_bin): the
// trip loop over the points and the block's class counts.  The per-point chain itself is gm_device.hpp's.
#pragma once

#include "gm_device.hpp"

namespace gm {

// One streaming pass over pts[0 .. n) (16 B of point + 1 B of label per point; labels nullptr: every label 0) by a grid of
// kThreads-wide blocks, grid-stride in trips of kUnroll slots.  A trip first issues the loads of all its slots, then works
// them off: body(i, in, q, lab, x) once per slot whose wave still has a point (the wave's first index decides: wave-uniform,
// so the run merges inside the bodies may shuffle across the wave), in: this lane's index i is below n (q, lab are 0 past it).
// x = pre(the slot's first index in this wave) is evaluated with the slot's loads, for what a body reads per wave and slot.
template <int kThreads, int kUnroll, class Pre, class Body>
__device__ __forceinline__ void stream_points_with(const float4 *pts, const uint8_t *labels, uint32_t n, Pre pre, Body body)
{
    const int lane = lane_id();
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t w0 = (uint64_t)blockIdx.x * kThreads + (threadIdx.x & ~(uint32_t)(kWave - 1)); w0 < n; w0 += kUnroll * stride) {
        float4 q[kUnroll];
        uint32_t lab[kUnroll];
        decltype(pre(w0)) x[kUnroll];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const uint64_t i = w0 + lane + (uint64_t)k * stride;
            lab[k] = 0u;
            q[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            x[k] = pre(w0 + (uint64_t)k * stride);
            if (i < n) {
                q[k] = pts[i];
                if (labels) lab[k] = labels[i];
            }
        }
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const uint64_t i = w0 + lane + (uint64_t)k * stride;
            if (w0 + (uint64_t)k * stride >= n) break;   // (wave-uniform)
            body(i, i < n, q[k], lab[k], x[k]);
        }
    }
}
// the same without a per-slot value: body(i, in, q, lab)
template <int kThreads, int kUnroll, class Body>
__device__ __forceinline__ void stream_points(const float4 *pts, const uint8_t *labels, uint32_t n, Body body)
{
    stream_points_with<kThreads, kUnroll>(
        pts, labels, n, [](uint64_t) { return 0; }, [&](uint64_t i, bool in, const float4 &q, uint32_t lab, int) { body(i, in, q, lab); });
}

// rows[k][wave] of a block of kWaves waves -> sink(k, their sum) on thread k: one value per class and block.  Every thread
// of the block is here.
template <int kCls, int kWaves, class Sink>
__device__ __forceinline__ void block_row_sums(const uint32_t (&rows)[kCls][kWaves], Sink sink)
{
    __syncthreads();
    if (threadIdx.x < (uint32_t)kCls) {
        unsigned long long v = 0ull;
        for (int w = 0; w < kWaves; ++w) v += rows[threadIdx.x][w];
        sink(threadIdx.x, v);
    }
}
// the per-lane class counts of a kThreads-wide block: wave_sum into LDS rows, then block_row_sums
template <int kThreads, int kCls, class Sink>
__device__ __forceinline__ void block_class_counts(const uint32_t (&cls)[kCls], Sink sink)
{
    __shared__ uint32_t s_cls[kCls][kThreads / kWave];
#pragma unroll
    for (int k = 0; k < kCls; ++k) {
        const uint32_t v = wave_sum(cls[k]);
        if (lane_id() == 0) s_cls[k][threadIdx.x / kWave] = v;
    }
    block_row_sums(s_cls, sink);
}

}  // namespace gm
