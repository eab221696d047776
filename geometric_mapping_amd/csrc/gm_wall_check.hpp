// gm_wall_check.hpp -- what the kernels that check a frame against a wall map share (k_wall_check.hip's k_wall_check*,
// k_wall_check_joint.hip's k_wall_check_joint): the payload a changed point keeps in registers, the gather of its cell and
// the integer rule, the 32-byte row, the peaks and the closing atomics.  The chain head itself is gm_device.hpp's.
#pragma once

#include "gm_compact.hpp"
#include "gm_internal.hpp"

namespace gm {

static_assert(sizeof(gm_wall_check_point) == 32, "a 32-byte PointCloud2 row");
static_assert(GM_WALL_CHECK_CLS_PLANE == kChainPlane && GM_WALL_CHECK_CLS_BEYOND_GATE == kChainBeyondGate &&
                  GM_WALL_CHECK_CLS_OUTSIDE == kChainOutside, "the check's first classes are wall_chain's");

// block-shared: kWords class counts (seven per map the launch checks against), then the two peaks (magnitudes)
template <int kWords>
__device__ __forceinline__ uint32_t *wk_class_counts()
{
    __shared__ uint32_t c[kWords];
    return c;
}
__device__ __forceinline__ unsigned long long *wk_peaks()
{
    __shared__ unsigned long long p[2];
    return p;
}

// what a changed point keeps between the predicate and the emit step (8 words per item)
struct WallCheckPayload { float4 q; long long delta; float e; int cell; };

// A mapped point against its cell of T: the count first, then 8 B of sum or the two keys only for a usable cell, and the
// integer rule.  cell is j * n_sectors + k of T's own map.
__device__ __forceinline__ uint32_t wall_check_cell(const WallTable &T, int cell, uint32_t reference, uint32_t min_count, long long Tq,
                                                    float e, long long &delta)
{
    const uint32_t cn = T.cnt[cell];
    long long sum = 0;
    uint32_t lo = 0u, hi = 0u;
    if (cn >= min_count) {
        if (reference == GM_WALL_CHECK_ENVELOPE) { lo = T.lo[cell]; hi = T.hi[cell]; }
        else sum = (long long)T.sum[cell];
    }
    return wall_check_rule(reference, min_count, Tq, sum, cn, lo, hi, e, delta);
}

// the stage call's per-point delta: saturated to 32 bits
__device__ __forceinline__ int32_t wall_check_delta32(long long delta)
{
    return delta > 2147483647ll ? 2147483647 : (delta < -2147483648ll ? (int32_t)(-2147483647 - 1) : (int32_t)delta);
}

// One ballot per class over the active lanes (the lanes past the end of the input are not here), the first lane of each
// adds the wave's count to the block's word.
template <int kWords>
__device__ __forceinline__ void wall_check_count(uint32_t cls, uint32_t first_word)
{
    const int lane = lane_id();
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)GM_WALL_CHECK_N_CLS; ++k) {
        const unsigned long long m = __ballot(cls == k);
        if (m && lane == (int)__builtin_ctzll(m)) atomicAdd(&wk_class_counts<kWords>()[first_word + k], (uint32_t)__popcll(m));
    }
}

// the 32-byte row at the survivor's rank (two 16-byte stores), and this thread's integer extremes
__device__ __forceinline__ void wall_check_row(gm_wall_check_point *out, uint32_t row_is_index, uint32_t src, uint32_t dst,
                                               const WallCheckPayload &p, long long &q_pos, long long &q_neg)
{
    float4 *o = reinterpret_cast<float4 *>(out + dst);
    o[0] = make_float4(p.q.x, p.q.y, p.q.z, __fmul_rn((float)p.delta, 0x1p-20f));
    o[1] = make_float4(p.e, __int_as_float(p.cell), __uint_as_float(src), row_is_index ? __uint_as_float(src) : p.q.w);
    if (p.delta > q_pos) q_pos = p.delta;
    if (p.delta < q_neg) q_neg = p.delta;
}

template <int kWords>
__device__ __forceinline__ void wall_check_prepare()
{
    if (threadIdx.x < (uint32_t)kWords) wk_class_counts<kWords>()[threadIdx.x] = 0u;
    if (threadIdx.x < 2u) wk_peaks()[threadIdx.x] = 0ull;
}

// Every thread of the block is here (full waves): the peaks over the wave and the block, then one integer atomic per class
// word and block into cls_ctr[kWords], one atomicMax per peak and block into peak_ctr[2].
template <int kWords>
__device__ __forceinline__ void wall_check_finish(unsigned long long *cls_ctr, unsigned long long *peak_ctr, long long q_pos,
                                                  long long q_neg)
{
    unsigned long long hp = (unsigned long long)q_pos, hn = (unsigned long long)(-q_neg);
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long op = __shfl_xor(hp, o, kWave), on = __shfl_xor(hn, o, kWave);
        hp = hp > op ? hp : op;
        hn = hn > on ? hn : on;
    }
    if (lane_id() == 0) {
        if (hp) atomicMax(&wk_peaks()[0], hp);
        if (hn) atomicMax(&wk_peaks()[1], hn);
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)kWords) {
        const uint32_t c = wk_class_counts<kWords>()[threadIdx.x];
        if (c) atomicAdd(&cls_ctr[threadIdx.x], (unsigned long long)c);
    } else if (threadIdx.x < (uint32_t)kWords + 2u) {
        const unsigned long long v = wk_peaks()[threadIdx.x - kWords];
        if (v) atomicMax(&peak_ctr[threadIdx.x - kWords], v);
    }
}

}  // namespace gm
