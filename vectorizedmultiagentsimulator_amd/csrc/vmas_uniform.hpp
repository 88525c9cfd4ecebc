// vmas_uniform.hpp -- one column of PyTorch's uniform_ kernel on the device (vmas_actions.hip
// k_uniform_columns; vmas_copy.hip k_copy_draw): thread idx of torch's grid of `blocks` x 256
// threads initialises philox4x32-10 at (seed, subsequence = idx, column offset), draws 4 numbers
// per grid-stride round for elements idx + k * threads, maps them to (0, 1] and to [from, to)
// (the two float roundings fused or not: `mode`, probed against torch by the host).  uniform_at
// draws ONE element of such a call directly (vmas_spawn.hip's tries, vmas_reset.hip's masked rows).
#pragma once

#include <hip/hip_runtime.h>

#include <rocrand/rocrand_philox4x32_10.h>

#include "vmas_mi355x.h"

namespace vmas_uniform {

constexpr int kThreads = 256;

__device__ __forceinline__ float unit_float(unsigned int v, bool fused) {
    const float inv = 2.3283064e-10f;  // ROCRAND_2POW32_INV
    return fused ? __builtin_fmaf((float)v, inv, inv) : inv + (float)v * inv;
}

// Block `block` of the column's draw (blocks = torch's grid size for numel elements).  With a
// second output (col.u_out) the drawn value is also written as the action kernel applies it;
// snap != 0: that element's previous value is first stored snap bytes from it.
__device__ __forceinline__ void draw_column(const VmasUniformColumn& col, unsigned long long seed, long long numel,
                                            long long snap, int mode, int blocks, int block) {
    const long long idx = (long long)block * kThreads + threadIdx.x;
    rocrand_state_philox4x32_10 st;
    rocrand_init(seed, (unsigned long long)idx, col.offset, &st);
    const long long step = (long long)kThreads * blocks;
    const long long rounded = ((numel - 1) / (step * 4) + 1) * step * 4;
    const float from = col.from, to = col.to, range = to - from;
    const bool fused_unit = mode & 1, fused_affine = mode & 2;
    for (long long li0 = idx; li0 < rounded; li0 += step * 4) {
        const uint4 v = rocrand4(&st);
        const unsigned int vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long li = li0 + step * k;
            if (li < numel) {
                const float r = unit_float(vv[k], fused_unit);
                const float val = fused_affine ? __builtin_fmaf(r, range, from) : r * range + from;
                const float x = val == to ? from : val;  // (0, 1] -> [from, to)
                col.out[li * col.stride] = x;
                if (col.u_out) {  // apply_one's operations on the same value
                    const float u = col.u_clamp ? fminf(fmaxf(x, -col.u_range), col.u_range) : x;
                    float* uo = col.u_out + li * col.u_stride;
                    if (snap) *reinterpret_cast<float*>(reinterpret_cast<char*>(uo) + snap) = *uo;
                    *uo = u * col.u_mult;
                }
            }
        }
    }
}

struct DrawGrid {
    long long step;  // threads of torch's uniform_ grid on B elements
    unsigned long long inc;
};

// rocrand's philox4x32-10 block function (rocrand_philox4x32_10.h ten_rounds / single_round).
__device__ __forceinline__ uint4 philox10(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        // (the 64-bit products: one v_mad_u64_u32 each instead of v_mul_hi_u32 + v_mul_lo_u32, both
        // quarter rate)
        const unsigned long long p0 = (unsigned long long)c.x * 0xD2511F53u;
        const unsigned long long p1 = (unsigned long long)c.z * 0xCD9E8D57u;
        const unsigned int hi0 = (unsigned int)(p0 >> 32), lo0 = (unsigned int)p0;
        const unsigned int hi1 = (unsigned int)(p1 >> 32), lo1 = (unsigned int)p1;
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}

// Element b of torch's uniform_(lo, hi) on B floats at generator offset `off`: PyTorch's
// distribution kernel (k_uniform_columns of vmas_actions.hip, probed bit for bit against torch;
// `mode` bit 0 fused (0, 1] mapping, bit 1 fused affine transform) has thread t = b % step draw
// rocrand4 round q / 4 and take component q % 4, q = b / step, from a philox state initialised
// at (seed, subsequence t, offset off).  That state is counter (off / 4 + round, t) under key
// seed, its 4 outputs shifted by off % 4 into the next block (rocrand's interleave); computed
// here directly, one block function per draw.
__device__ __forceinline__ float uniform_at(unsigned long long seed, unsigned long long off, const DrawGrid& g, int b,
                                            float lo, float hi, int mode) {
    const int step = (int)g.step, t = b % step, q = b / step;
    const unsigned long long c = off / 4 + (unsigned long long)(q / 4);
    const uint2 key = make_uint2((unsigned int)seed, (unsigned int)(seed >> 32));
    const uint4 cur = philox10(make_uint4((unsigned int)c, (unsigned int)(c >> 32), (unsigned int)t, 0u), key);
    const int sub = (int)(off & 3ull), k = sub + q % 4;
    unsigned int u;
    if (k < 4) {
        u = k == 0 ? cur.x : k == 1 ? cur.y : k == 2 ? cur.z : cur.w;
    } else {
        const uint4 nxt = philox10(make_uint4((unsigned int)(c + 1), (unsigned int)((c + 1) >> 32), (unsigned int)t, 0u), key);
        u = k == 4 ? nxt.x : k == 5 ? nxt.y : nxt.z;
    }
    const float inv = 2.3283064e-10f;  // ROCRAND_2POW32_INV
    const float unit = (mode & 1) ? __builtin_fmaf((float)u, inv, inv) : inv + (float)u * inv;
    const float range = hi - lo;
    const float val = (mode & 2) ? __builtin_fmaf(unit, range, lo) : unit * range + lo;
    return val == hi ? lo : val;  // (0, 1] -> [lo, hi)
}

// torch's distribution-kernel grid for numel elements and the per-call philox increment
// (counter_offset, rounded up to a multiple of 4); max_blocks = CUs x (maxThreadsPerCU / 256)
inline void grid_for(long long numel, int max_blocks, int* blocks, unsigned long long* inc) {
    const long long gx = (numel + kThreads - 1) / kThreads < max_blocks ? (numel + kThreads - 1) / kThreads : max_blocks;
    *blocks = (int)gx;
    *inc = (unsigned long long)((numel - 1) / (kThreads * gx * 4) + 1) * 4;
}

}  // namespace vmas_uniform
