// vmas_reset.hip -- a scenario's reset for the rows of a mask, in ONE launch (Environment.reset_where;
// no reference counterpart: the reference resets one env per call, environment.py:229-262).
//
// k_balance_reset: balance.py:85-215 `reset_world_at(None)` after World.reset, one thread per env.
// A row outside the mask returns before it reads or writes anything but its mask byte.  A masked row
// b takes element b of the four uniform_ calls the full reset makes on [B, 1] tensors
// (vmas_uniform.hpp uniform_at: the same philox counters, so the same numbers as the full reset's
// row b), places the entities with the reference's fp32 additions (-ffp-contract=off: no FMA), and
// computes on_the_ground / global_shaping with the functions of the fused step program
// (vmas_programs.hpp), which equal the torch program bit for bit (tests/test_fused.py).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "vmas_aux.hpp"
#include "vmas_mi355x.h"
#include "vmas_programs.hpp"
#include "vmas_uniform.hpp"

using namespace vmas;

namespace {

constexpr int kResetThreads = 64;  // (one wave: the masked rows are few, more workgroups spread them)
static_assert(sizeof(VmasBalanceResetIO) + sizeof(vmas_uniform::DrawGrid) <= 4096, "kernel argument block");

__device__ __forceinline__ void put2(const VmasMutVec& v, int b, float x, float y) {
    if (!v.p) return;
    float* p = v.p + (long)b * v.s0;
    p[0] = x;
    p[v.s1] = y;
}
__device__ __forceinline__ void put1(const VmasMutVec& v, int b, float x) {
    if (v.p) v.p[(long)b * v.s0] = x;
}
// World.reset zeroes every state field; reset_world_at then sets pos (and the line's rot, to 0)
__device__ __forceinline__ void place(const VmasResetEntity& e, int b, V2 pos) {
    put2(e.pos, b, pos.x, pos.y);
    put2(e.vel, b, 0.f, 0.f);
    put1(e.rot, b, 0.f);
    put1(e.ang_vel, b, 0.f);
}

__global__ void __launch_bounds__(kResetThreads) k_balance_reset(VmasBalanceResetIO io_arg, vmas_uniform::DrawGrid g) {
    VMAS_PROGRAM_ARGS(VmasBalanceResetIO, io_arg);
    const int b = blockIdx.x * kResetThreads + threadIdx.x;
    if (b >= io.batch || io.mask[b] == 0) return;
    float u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        u[j] = vmas_uniform::uniform_at(io.seed, io.offset + g.inc * (unsigned long long)j, g, b, io.lo[j], io.hi[j],
                                        io.mode);
    const V2 goal = mk(u[0], u[1]);
    const V2 line = mk(u[2], io.line_y);
    const V2 pkg = mk(line.x + u[3], line.y + io.package_rel_y);  // line_pos + package_rel_pos
    const V2 pf = mk(io.floor_x, io.floor_y);
    for (int i = 0; i < io.n_agents; ++i) {
        const VmasResetEntity ag = io.agents[i];
        place(ag, b, mk(line.x + io.agent_dx[i], line.y + io.agent_dy));  // line_pos + offset
        const VmasMutVec f = io.force[i], t = io.torque[i];
        put2(f, b, 0.f, 0.f);
        put1(t, b, 0.f);
    }
    {
        const VmasResetEntity e = io.goal;
        place(e, b, goal);
    }
    {
        const VmasResetEntity e = io.package;
        place(e, b, pkg);
    }
    {
        const VmasResetEntity e = io.line;
        place(e, b, line);
    }
    {
        const VmasResetEntity e = io.floor;
        place(e, b, pf);
    }
    // compute_on_the_ground: is_overlapping(line, floor) + is_overlapping(package, floor), as
    // bal_side / bal_reward compute it (every rot is 0 after the reset)
    const Trig tf = xtrig(0.f);
    const float hl = io.floor_length * 0.5f, hw = io.floor_width * 0.5f;
    const Seg ln{line, mk(cosf(0.f), sinf(0.f)), io.line_length * 0.5f};
    V2 c1 = mk(INFINITY, INFINITY), c2 = mk(INFINITY, INFINITY), cp = mk(INFINITY, INFINITY);
    float bd = INFINITY, bp = INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const Seg sd = box_side(pf, tf, hl, hw, i);
        V2 q1, q2;
        xclosest_points_line_line(sd, ln, &q1, &q2);
        const float d = xnorm(q1 - q2);
        if (d < bd) {
            bd = d;
            c1 = q1;
            c2 = q2;
        }
        const V2 p = closest_point_line(sd.p, sd.dir, sd.half, pkg, true);
        const float dp = xnorm(pkg - p);
        if (dp < bp) {
            bp = dp;
            cp = p;
        }
    }
    const float dsc = xnorm(pkg - cp), dsb = xnorm(pkg - pf), dcb = xnorm(pf - cp);
    const bool og = (xnorm(c1 - c2) - kLineMinDist < 0.f) || (dsb < dcb) || (dsc < io.package_radius_lmd);
    io.on_the_ground[b] = og ? 1 : 0;
    const VmasMutVec gs = io.global_shaping;
    put1(gs, b, xnorm(pkg - goal) * io.shaping_factor);
    if (io.steps) io.steps[b] = 0.f;
}

}  // namespace

extern "C" int32_t vmas_balance_reset(int32_t device, const VmasBalanceResetIO* io, uint64_t* increment, void* stream) {
    if (!io || !increment || device < 0 || device >= 64 || io->batch <= 0 || io->n_agents < 0 ||
        io->n_agents > VMAS_SCN_MAX_AGENTS || !io->mask || !io->on_the_ground || !io->global_shaping.p || io->mode < 0 ||
        io->mode > 3)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_balance_reset: bad arguments");
    VMAS_AUX_HIP(hipSetDevice(device));
    static int max_blocks[64] = {0};
    if (!max_blocks[device]) {
        hipDeviceProp_t prop;
        VMAS_AUX_HIP(hipGetDeviceProperties(&prop, device));
        max_blocks[device] = prop.multiProcessorCount * (prop.maxThreadsPerMultiProcessor / vmas_uniform::kThreads);
        if (max_blocks[device] <= 0) return vmas_aux::fail(VMAS_E_HIP, "vmas_balance_reset: device properties");
    }
    // torch's distribution-kernel grid and per-call philox increment on B elements
    int gx_draw = 0;
    unsigned long long inc = 0;
    vmas_uniform::grid_for(io->batch, max_blocks[device], &gx_draw, &inc);
    const vmas_uniform::DrawGrid g{(long long)vmas_uniform::kThreads * gx_draw, inc};
    const int gx = (io->batch + kResetThreads - 1) / kResetThreads;
    hipLaunchKernelGGL(k_balance_reset, dim3(gx), dim3(kResetThreads), 0, (hipStream_t)stream, *io, g);
    VMAS_AUX_HIP(hipGetLastError());
    *increment = inc * 4ull;
    return VMAS_OK;
}
