// vmas_scenarios.hip -- fused observation / reward / done programs of the benchmark scenarios
// (SURVEY.md §8(f) row 4), gfx950 kernels + C ABI.
//
// The reference computes a scenario's per-step outputs as an eager tensor program: balance's
// rewards, observations and dones (balance.py:222-262) are ~37 small kernels per step, each a few
// microseconds of launch latency for a few hundred KB of traffic -- more GPU time than the physics
// step itself.  Each entry point here computes one scenario's program in ONE launch, one thread
// per environment, with the reference's fp32 operations in the reference's order (no FMA
// contraction: -ffp-contract=off as the engine; norms as torch.linalg.vector_norm of a length-2
// vector; `%` as torch.remainder; is_overlapping / get_distance as vmas_query.hpp).  The host
// side (the restated scenario) keeps every attribute the reference's program leaves behind.
#include <hip/hip_runtime.h>

#include "vmas_aux.hpp"
#include "vmas_lidar.hpp"
#include "vmas_light_programs.hpp"
#include "vmas_mi355x.h"
#include "vmas_mpe_programs.hpp"
#include "vmas_programs.hpp"
#include "vmas_query.hpp"
#include "vmas_uniform.hpp"

using namespace vmas;

namespace {

// balance.py:205-262 (restated in scenarios/balance.py): reward of the first agent (on-the-ground
// test, package-goal distance, ground / position rewards and the global shaping update), every
// agent's reward (ground_rew + pos_rew), every agent's 16-entry observation, and done
// (on_the_ground + is_overlapping(package, goal)).  Grid: x = 64-env groups, y = part, 4 waves
// per workgroup.  Part 0 is the reward / done part: the (floor, line) box-line distance of the
// on-the-ground test is split over the 4 waves, one box side each (bl_part), and wave 0 picks the
// first strict minimum over the sides in order, as closest_line_box does, then finishes.  Parts
// 1 + k are the observations of agents 4k .. 4k + 3, one per wave.  (One 64-thread workgroup per
// (group, part), the box-line distance in one chain: 11 us per step at 32 768 envs, the chain's
// latency at two waves per CU; before that 128 x 1 workgroups took 16 us.)
__global__ void __launch_bounds__(256) k_balance(VmasBalanceIO io_arg) {
    VMAS_PROGRAM_ARGS(VmasBalanceIO, io_arg);
    __shared__ float Q[kBalQRows * 64];  // the box queries' sides (vmas_programs.hpp bal_q)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * 64 + lane;
    const bool valid = b < io.batch;
    const int bb = valid ? b : io.batch - 1;
    const OutDelta od = load_out_delta(io);
    if (blockIdx.y == 0) {
        if (!(io.what & VMAS_SCN_REWARD)) {
            if (wave != 0 || !valid || !(io.what & VMAS_SCN_DONE)) return;
            bal_done(io, b, io.on_the_ground[b] != 0, od);
            return;
        }
        const BalPre pre = wave == 0 ? bal_preload(io, bb) : BalPre{0.f, mk(0.f, 0.f)};
        bal_side(io, bb, wave, lane, Q);  // side `wave` of the floor's two box queries
        __syncthreads();
        if (wave != 0 || !valid) return;
        bal_reward(io, b, lane, od, Q, pre);
        return;
    }
    // agent i's observation
    const int i = (blockIdx.y - 1) * 4 + wave;
    if (i >= io.n_agents || !valid) return;
    bal_obs(io, b, i, od);
}

// The flocking separation term sums n floats in the order of torch's .mean(-1) over a contiguous
// last dim (vmas_programs.hpp flock_mean_sq_sep, shared with the masked reset; sum_mode: the
// accumulator count the host probed, simulator/_fused.py reduce_order).

// flocking.py:149-206 (restated in scenarios/flocking.py).  Grid: x = 64-env groups, y = (policy
// agent p, part): part 0 is p's reward and the first six observation entries, part 1 + r is ray r
// of p's LIDAR (one (env, agent, ray) per thread: a thread per (env, agent) casting all 12 rays
// left the chip latency-bound at 3 waves per SIMD, 95 us per step at 32 768 envs x 8 agents).
// Positions are loaded up front with independent loads (unrolled over the static bounds).
// Part 0 of policy agent p in env b: the reward block (REWARD) and the first six observation
// entries (OBS).
struct FlockHead {
    float v[6];
};
// IO: the argument block by value, or (k_flocking_fast) read in place through the kernel
// argument segment (VMAS_PROGRAM_ARGS) -- structs copied out before use.
template <class IO>
__device__ __forceinline__ FlockHead flock_part0(IO& io, int b, int p, const OutDelta& od, bool ret = false) {
    FlockHead h{};
    constexpr int MA = VMAS_FLOCK_MAX_AGENTS;
    const int k = io.policy[p], na = io.n_all;
    const VmasShapeRef ak = io.agents[k];
    const V2 pk = ref_pos(ak, b);
    const int W = 6 + io.n_rays;
    V2 P[MA];
#pragma unroll
    for (int j = 0; j < MA; ++j) {
        const VmasShapeRef aj = io.agents[j];
        P[j] = j < na ? ref_pos(aj, b) : mk(0.f, 0.f);
    }
    if (io.what & VMAS_SCN_REWARD) {
        if (p == 0) io.t[b] = io.t[b] + 1.f;  // self.t += 1 (first policy agent's call)
        // collision rewards: pairs (i < j) of world.agents in loop order; agent k meets them
        // as j = 0 .. k-1, k+1 .. n-1 (get_distance of spheres: |p_lo - p_hi| - r_lo - r_hi)
        float cr = 0.f;  // a.collision_rew[:] = 0
        if (io.collide_reward_on) {
#pragma unroll
            for (int j = 0; j < MA; ++j) {
                if (j >= na || j == k) continue;
                const int lo = j < k ? j : k, hi = j < k ? k : j;
                const V2 plo = j < k ? P[j] : pk, phi = j < k ? pk : P[j];
                const float d = (norm(plo - phi) - io.agents[lo].radius) - io.agents[hi].radius;
                cr = cr + ((d <= io.min_collision_distance) ? io.collision_reward : 0.f);
            }
            io.collision_rew[p][b] = cr;
        } else {
            cr = io.collision_rew[p][b];
        }
        // separation: (stack(|p_k - p_j| for j != k) - desired).pow(2).mean(-1) * factor, summed
        // in torch's order (vmas_programs.hpp)
        const float shaping = flock_mean_sq_sep<MA>(
            na, k, pk, [&](int j) { return P[j]; }, io.desired_distance, io.dist_shaping_factor, io.sum_mode);
        const float dr = io.shaping_in[p][b] - shaping;
        io.shaping_out[p][b] = shaping;
        io.dist_rew[p][b] = dr;
        moved(io.rewards[p], od.rew)[b] = cr + dr;
    }
    if (io.what & VMAS_SCN_OBS) {
        const VmasVec vp = io.vel[p];
        const V2 v = ld_vec2(vp, b);
        V2 tp = mk(0.f, 0.f);
#pragma unroll
        for (int j = 0; j < MA; ++j)
            if (j == io.target) tp = P[j];
        h = FlockHead{{pk.x, pk.y, v.x, v.y, pk.x - tp.x, pk.y - tp.y}};
        if (!ret) {
            float* o = moved(io.obs[p], od.obs) + (long)b * W;
#pragma unroll
            for (int i = 0; i < 6; ++i) o[i] = h.v[i];
        }
    }
    return h;
}

// flocking.py:149-206 (restated in scenarios/flocking.py), LIDAR bit-identical to k_cast_rays
// (io.fast_lidar == 0).  Grid: x = 64-env groups, y = (policy agent p, part): part 0 is p's
// reward and the first six observation entries, part 1 + r is ray r of p's LIDAR (one (env,
// agent, ray) per thread: a thread per (env, agent) casting all 12 rays with the exact ray code
// left the chip latency-bound at 3 waves per SIMD, 95 us per step at 32 768 envs x 8 agents).
// Positions are loaded up front with independent loads (unrolled over the static bounds).
__global__ void __launch_bounds__(64) k_flocking(VmasFlockingIO io) {
    constexpr int MT = VMAS_SCN_MAX_RAY_TARGETS;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= io.batch) return;
    const int parts = (io.what & VMAS_SCN_OBS) ? 1 + io.n_rays : 1;
    const int p = blockIdx.y / parts, part = blockIdx.y - p * parts, k = io.policy[p];
    const OutDelta od = load_out_delta(io);
    if (part == 0) {
        flock_part0(io, b, p, od);
        return;
    }
    // LIDAR ray r: Lidar.measure = World.cast_rays(angles + agent rot) (cast_one)
    const V2 pk = ref_pos(io.agents[k], b);
    const int W = 6 + io.n_rays;
    const int r = part - 1, nt = io.n_ray_targets;
    V2 T[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const VmasRayTarget& x = io.ray_targets[t];
        T[t] = t < nt ? mk(x.pos[(long)b * x.pos_s0], x.pos[(long)b * x.pos_s0 + x.pos_s1]) : mk(0.f, 0.f);
    }
    const float a = io.angles[p][(long)b * io.ang_s0[p] + (long)r * io.ang_s1[p]] + ld_vec1(io.rot[p], b);
    const float dc = cosf(a), ds = sinf(a);
    float best = io.max_range;
#pragma unroll
    for (int t = 0; t < MT; ++t)  // (sphere targets: checked by the host entry point)
        if (t < nt) best = tmin(best, ray_sphere(pk, dc, ds, T[t], io.ray_targets[t].radius, io.max_range));
    io.lidar[p][(long)b * io.n_rays + r] = best;
    moved(io.obs[p], od.obs)[(long)b * W + 6 + r] = best;
}

// The same program with the fast LIDAR (io.fast_lidar, the default; RayHardware).  Grid: x = 64-env
// groups, y = groups of 4 policy agents; a wave per (64 envs, agent): its reward / head
// (flock_part0) and all of its rays (angles and targets loaded up front), the observation rows
// staged in LDS.  NR / NT > 0: the ray and target counts fixed at compile time (flocking's 12 rays;
// instantiated for 1..8 targets), the unrolled form of lidar_row with the LIDAR row split by a
// constant; otherwise its runtime form.  History (32 768 envs x 8 agents): a thread per ray of the
// exact program, 53 us; a thread per (env, agent) with ocml sincosf and per-ray angle loads, 89 us;
// waves over ray subsets with wave 0 also doing the reward, 48 us.
constexpr int kFlockFastRays = 16, kFlockFastTargets = 8, kFlockFastW = 6 + kFlockFastRays;
template <int NR, int NT>
__global__ void __launch_bounds__(256) k_flocking_fast(VmasFlockingIO io_arg) {
    constexpr int RM = NR > 0 ? NR : kFlockFastRays, TM = NT > 0 ? NT : kFlockFastTargets;
    VMAS_PROGRAM_ARGS(VmasFlockingIO, io_arg);
    __shared__ float S[4][64 * kFlockFastW];
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const int g0 = (int)blockIdx.x * 64, b = g0 + lane;
    const int p = wave_uniform((int)blockIdx.y * 4 + w);
    if (p >= io.n_policy) return;  // (wave-uniform; no workgroup barrier below)
    const bool valid = b < io.batch;
    const int nr = NR > 0 ? NR : io.n_rays, nt = NT > 0 ? NT : io.n_ray_targets, W = 6 + nr;
    const int bb = valid ? b : io.batch - 1;
    const int row = lane * W;
    const OutDelta od = load_out_delta(io);
    if (io.what & VMAS_SCN_OBS) {
        // loads first (independent): angles, rotation, position, targets
        const float* ang = io.angles[p] + (long)bb * io.ang_s0[p];
        const int as1 = io.ang_s1[p];
        float A[RM];
#pragma unroll
        for (int r = 0; r < RM; ++r) A[r] = r < nr ? ang[(long)r * as1] : 0.f;
        const VmasVec rv = io.rot[p];
        const float rot = ld_vec1(rv, bb);
        const VmasShapeRef ak = io.agents[io.policy[p]];
        const V2 pk = ref_pos(ak, bb);
        V2 T[TM];
        float R2[TM];
#pragma unroll
        for (int t = 0; t < TM; ++t) {
            const float* xp = io.ray_targets[t].pos;
            const int s0 = io.ray_targets[t].pos_s0, s1 = io.ray_targets[t].pos_s1;
            const float rad = io.ray_targets[t].radius;
            T[t] = t < nt ? mk(xp[(long)bb * s0], xp[(long)bb * s0 + s1]) - pk : mk(0.f, 0.f);
            R2[t] = t < nt ? rad * rad : 0.f;
        }
        if (valid) {
            const FlockHead h = flock_part0(io, b, p, od, true);
#pragma unroll
            for (int i = 0; i < 6; ++i) S[w][row + i] = h.v[i];
        }
        float C[TM];
#pragma unroll
        for (int t = 0; t < TM; ++t) C[t] = RayHardware::c(R2[t], T[t]);
        lidar_row<RayHardware, (NR > 0 && NT > 0), RM, 1>(
            S[w] + row + 6, nr, [&](int r) { return A[r] + rot; }, T, C, io.max_range,
            [&](int t) { return NT > 0 || t < nt; });
        const int nv = io.batch - g0 < 64 ? io.batch - g0 : 64;
        rows_out(S[w], nv, W, moved(io.obs[p], od.obs) + (long)g0 * W, lane, 64, nullptr,
                 io.lidar[p] + (long)g0 * nr, 6, nr, lane);
    } else if (valid) {
        flock_part0(io, b, p, od);
    }
}

// ---- navigation (navigation.py:199-277; restated in scenarios/navigation.py) -----------------------
// The reward block of agent k in env b is computed by the wave of (64 envs, k): every agent's
// distance to its goal (the shared pos_rew is their sum from zero in agent order, all_goal_reached
// their conjunction: each wave recomputes them rather than meeting in LDS -- n norms against a
// LIDAR's rays x targets), k's own outputs, and k's collision reward over the pairs it is part of.
// NA: the static bound of the agent loops (the agent count in the unrolled instantiations).
constexpr int kNavMA = VMAS_NAV_MAX_AGENTS;
// ws words: [0, 16) word i bit j (< i): the pair (i, j) touches in some env (World.collides' last
// test), [16, 32) it is near (distance <= min_collision_distance) in some env
constexpr int kNavWsNear = 16;
static_assert(2 * kNavMA <= VMAS_NAV_WS_WORDS && kNavMA <= 16, "navigation scratch words");

template <int NA, class IO>
__device__ __forceinline__ void nav_load(IO& io, int bb, V2* P, V2* G) {
    const int n = io.n_agents;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const VmasShapeRef aj = io.agents[j];
        const VmasVec gj = io.goal_pos[j];
        P[j] = j < n ? ref_pos(aj, bb) : mk(0.f, 0.f);
        G[j] = j < n ? ld_vec2(gj, bb) : mk(0.f, 0.f);
    }
}
template <int NA>
__device__ __forceinline__ V2 nav_sel(const V2* P, int k) {  // P[k] with static register indices
    V2 r = mk(0.f, 0.f);
#pragma unroll
    for (int j = 0; j < NA; ++j)
        if (j == k) r = P[j];
    return r;
}
// done(): every agent within its OWN radius of its goal (on_goal compares with the goal's)
template <int NA, class IO>
__device__ __forceinline__ bool nav_done(IO& io, const V2* P, const V2* G) {
    bool all = true;
#pragma unroll
    for (int j = 0; j < NA; ++j)
        if (j < io.n_agents) all = all && (xnorm(P[j] - G[j]) < io.agents[j].radius);
    return all;
}
// agent k's collision reward: a.agent_collision_rew[:] = 0, then the penalty once per pair (hi, lo <
// hi) that k is part of, World.collides(hi, lo) holds for (its static part; the batch-wide part:
// nav_pairs) and get_distance(hi, lo) = (|p_hi - p_lo| - r_hi) - r_lo
// <= min_collision_distance.  (Every addend is the same constant: the sum depends on their number
// only, not on the pairs' order.)  touch / near: the flags of the pairs (k, j < k) in this env.
template <int NA, class IO>
__device__ __forceinline__ float nav_collision(IO& io, const V2* P, V2 pk, int k, uint32_t* touch, uint32_t* near) {
    const int n = io.n_agents;
    const float radk = io.agents[k].radius;
    const uint32_t stk = io.pair_static[k];
    const double ck = io.circ[k];
    float cr = 0.f;
    uint32_t tb = 0u, nb = 0u;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        if (j >= n || j == k) continue;
        const bool lower = j < k;
        if (!((lower ? (stk >> j) : (io.pair_static[j] >> k)) & 1u)) continue;
        const float radj = io.agents[j].radius;
        const V2 ph = lower ? pk : P[j], pl = lower ? P[j] : pk;
        const float nrm = xnorm(ph - pl);
        const float d = (nrm - (lower ? radk : radj)) - (lower ? radj : radk);
        const bool nr = d <= io.min_collision_distance;
        if (nr) cr = cr + io.agent_collision_penalty;
        if (lower) {
            tb |= (nrm <= (float)(ck + io.circ[j])) ? (1u << j) : 0u;
            nb |= nr ? (1u << j) : 0u;
        }
    }
    *touch = tb;
    *near = nb;
    return cr;
}

// The batch-wide part of World.collides, after a REWARD launch (k_navigation_pairs, one workgroup):
// a pair near in some env and touching in none was penalised per env above but the reference skips
// it -- then (rare) the collision rewards and rewards of every env again, with the pairs that touch
// somewhere.  Leaves ws zero.  (A launch of its own: the kernel boundary orders it after every
// wave's outputs and flags.  Done by the last wave of the REWARD launch itself -- an agent-scope
// fence and a counter increment per wave -- that launch took 56 us at 32 768 envs x 4 agents and
// 107 us x 8, the waves queueing on the counter.)
template <class IO>
__device__ __forceinline__ void nav_pairs(IO& io, const OutDelta& od, int tid, int nthreads, uint32_t* EN) {
    const int n = io.n_agents;
    bool need = false;
    for (int i = 0; i < n; ++i) {
        const uint32_t t = io.ws[i], nr = io.ws[kNavWsNear + i];
        if (tid == 0) EN[i] = t;
        need = need || (nr & ~t) != 0u;
    }
    __syncthreads();
    if (tid < 2 * kNavMA) io.ws[tid] = 0u;
    if (!need) return;
    // (rolled: positions from memory per pair, nav_collision's operations)
    for (int b = tid; b < io.batch; b += nthreads) {
        const float s = io.pos_rew[b], fin = io.final_rew[b];
#pragma unroll 1
        for (int k = 0; k < n; ++k) {
            const VmasShapeRef ak = io.agents[k];
            const V2 pk = ref_pos(ak, b);
            float cr = 0.f;
#pragma unroll 1
            for (int j = 0; j < n; ++j) {
                const int hi = j < k ? k : j, lo = j < k ? j : k;
                if (j == k || !((io.pair_static[hi] >> lo) & (EN[hi] >> lo) & 1u)) continue;
                const VmasShapeRef aj = io.agents[j];
                const V2 pj = ref_pos(aj, b);
                const float nrm = xnorm(j < k ? pk - pj : pj - pk);
                const float d = (nrm - (j < k ? ak.radius : aj.radius)) - (j < k ? aj.radius : ak.radius);
                if (d <= io.min_collision_distance) cr = cr + io.agent_collision_penalty;
            }
            io.collision_rew[k][b] = cr;
            moved(io.rewards[k], od.rew)[b] = ((io.shared_rew ? s : io.agent_pos_rew[k][b]) + fin) + cr;
        }
    }
}

// REWARD (and DONE with it) of agent k for the wave's 64 envs; every lane of the wave calls.
template <int NA, class IO>
__device__ __forceinline__ void nav_reward(IO& io, int b, bool valid, int k, int lane, const OutDelta& od, const V2* P,
                                           const V2* G) {
    const int n = io.n_agents;
    // self.pos_rew[:] = 0; for a in agents: self.pos_rew += agent_reward(a)
    float s = 0.f, dk = 0.f, shk = 0.f, rk = 0.f;
    bool all = true, onk = false;
    const int bb = valid ? b : io.batch - 1;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        if (j >= n) continue;
        const float dist = xnorm(P[j] - G[j]);  // distance_to_goal
        const bool on = dist < io.goal_radius[j];
        const float shaping = dist * io.pos_shaping_factor;
        const float pr = io.shaping_in[j][bb] - shaping;
        s = s + pr;
        all = all && on;
        if (j == k) {
            dk = dist;
            shk = shaping;
            rk = pr;
            onk = on;
        }
    }
    const float fin = all ? io.final_reward : 0.f;  // final_rew[:] = 0; final_rew[all_goal_reached] = final_reward
    uint32_t tb, nb;
    const float cr = nav_collision<NA>(io, P, nav_sel<NA>(P, k), k, &tb, &nb);
    if (valid) {
        io.dist_to_goal[k][b] = dk;
        io.on_goal[k][b] = onk ? 1 : 0;
        io.shaping_out[k][b] = shk;
        io.agent_pos_rew[k][b] = rk;
        io.collision_rew[k][b] = cr;
        moved(io.rewards[k], od.rew)[b] = ((io.shared_rew ? s : rk) + fin) + cr;  // (pos + final_rew) + collision
        if (k == 0) {
            io.pos_rew[b] = s;
            io.final_rew[b] = fin;
            io.all_goal_reached[b] = all ? 1 : 0;
            if (io.what & VMAS_SCN_DONE) moved(io.done, od.done)[b] = nav_done<NA>(io, P, G) ? 1 : 0;
        }
    } else {
        tb = nb = 0u;
    }
    // the wave's pair flags for k_navigation_pairs (no lane near: no atomic)
    if (__ballot((tb | nb) != 0u) != 0ull) {
        uint32_t wt = 0u, wn = 0u;
#pragma unroll
        for (int j = 0; j < kNavMA; ++j) {
            wt |= __ballot((tb >> j) & 1u) != 0ull ? (1u << j) : 0u;
            wn |= __ballot((nb >> j) & 1u) != 0ull ? (1u << j) : 0u;
        }
        if (lane == 0) {
            if (wt) atomicOr(io.ws + k, wt);
            if (wn) atomicOr(io.ws + kNavWsNear + k, wn);
        }
    }
}

// the head of agent k's observation row: pos, vel, pos - goal (own, or every agent's)
template <int NA, class IO>
__device__ __forceinline__ void nav_head(IO& io, int bb, int k, const V2* P, const V2* G, float* o) {
    const V2 pk = nav_sel<NA>(P, k);
    const VmasVec vv = io.vel[k];
    const V2 v = ld_vec2(vv, bb);
    o[0] = pk.x;
    o[1] = pk.y;
    o[2] = v.x;
    o[3] = v.y;
    if (io.observe_all_goals) {
#pragma unroll
        for (int j = 0; j < NA; ++j)
            if (j < io.n_agents) {
                o[4 + 2 * j] = pk.x - G[j].x;
                o[5 + 2 * j] = pk.y - G[j].y;
            }
    } else {
        const V2 g = nav_sel<NA>(G, k);
        o[4] = pk.x - g.x;
        o[5] = pk.y - g.y;
    }
}

// The program with the LIDAR bit-identical to k_cast_rays (io.fast_lidar == 0, or a shape over the
// fast form's caps).  Grid as k_flocking: x = 64-env groups, y = (agent k, part): part 0 is k's
// reward, done (k == 0) and the observation head, part 1 + r is ray r of k's LIDAR over the other
// agents in order.
__global__ void __launch_bounds__(64) k_navigation(VmasNavigationIO io_arg) {
    constexpr int MA = kNavMA;
    VMAS_PROGRAM_ARGS(VmasNavigationIO, io_arg);
    const int lane = (int)threadIdx.x, b = (int)blockIdx.x * 64 + lane;
    const bool valid = b < io.batch;
    const int bb = valid ? b : io.batch - 1;
    const int nr = io.lidar_on ? io.n_rays : 0;
    const int parts = (io.what & VMAS_SCN_OBS) ? 1 + nr : 1;
    const int k = wave_uniform((int)blockIdx.y / parts);
    const int part = (int)blockIdx.y - k * parts;
    const int H = 4 + 2 * (io.observe_all_goals ? io.n_agents : 1), W = H + nr;
    const OutDelta od = load_out_delta(io);
    V2 P[MA], G[MA];
    nav_load<MA>(io, bb, P, G);
    if (part == 0) {
        if ((io.what & VMAS_SCN_OBS) && valid) nav_head<MA>(io, b, k, P, G, moved(io.obs[k], od.obs) + (long)b * W);
        if (io.what & VMAS_SCN_REWARD) nav_reward<MA>(io, b, valid, k, lane, od, P, G);
        else if ((io.what & VMAS_SCN_DONE) && k == 0 && valid) moved(io.done, od.done)[b] = nav_done<MA>(io, P, G) ? 1 : 0;
        return;
    }
    if (!valid) return;
    // LIDAR ray r: Lidar.measure = World.cast_rays(angles + agent rot) (cast_one)
    const int r = part - 1;
    const V2 pk = nav_sel<MA>(P, k);
    const VmasVec rv = io.rot[k];
    const float a = io.angles[k][(long)b * io.ang_s0[k] + (long)r * io.ang_s1[k]] + ld_vec1(rv, b);
    const float dc = cosf(a), ds = sinf(a);
    float best = io.max_range;
#pragma unroll
    for (int j = 0; j < MA; ++j)
        if (j < io.n_agents && j != k) best = tmin(best, ray_sphere(pk, dc, ds, P[j], io.agents[j].radius, io.max_range));
    io.lidar[k][(long)b * nr + r] = best;
    moved(io.obs[k], od.obs)[(long)b * W + H + r] = io.max_range - best;
}

__global__ void __launch_bounds__(1024) k_navigation_pairs(VmasNavigationIO io_arg) {
    VMAS_PROGRAM_ARGS(VmasNavigationIO, io_arg);
    __shared__ uint32_t EN[kNavMA];
    nav_pairs(io, load_out_delta(io), (int)threadIdx.x, (int)blockDim.x, EN);
}

// The same program with the fast LIDAR (io.fast_lidar, the default; RayPrecise), laid out as
// k_flocking_fast: grid x = 64-env groups, y = groups of 4 agents; a wave per (64 envs, agent): its
// reward, its observation head and all of its rays (angles, positions and goals loaded up front),
// the rows staged in LDS (4 x 64 x W floats, sized by the launch).  NR / NT > 0: the ray and target
// counts fixed at compile time (12 rays; 1..7 targets, i.e. 2..8 agents), the unrolled form of
// lidar_row; otherwise its runtime form.  The LIDAR's targets are the other agents in order.
constexpr int kNavFastRays = 16, kNavFastTargets = kNavMA - 1;
template <int NR, int NT>
__global__ void __launch_bounds__(256) k_navigation_fast(VmasNavigationIO io_arg) {
    constexpr int RM = NR > 0 ? NR : kNavFastRays, TM = NT > 0 ? NT : kNavFastTargets;
    constexpr int NA = NT > 0 ? NT + 1 : kNavMA;
    VMAS_PROGRAM_ARGS(VmasNavigationIO, io_arg);
    extern __shared__ float nav_lds[];
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const int g0 = (int)blockIdx.x * 64, b = g0 + lane;
    const int k = wave_uniform((int)blockIdx.y * 4 + w);
    const int n = io.n_agents;
    if (k >= n) return;  // (wave-uniform; no workgroup barrier below)
    const bool valid = b < io.batch;
    const int bb = valid ? b : io.batch - 1;
    const int nr = NR > 0 ? NR : (io.lidar_on ? io.n_rays : 0), nt = NT > 0 ? NT : n - 1;
    const int H = 4 + 2 * (io.observe_all_goals ? n : 1), W = H + nr;
    float* S = nav_lds + w * 64 * W;
    const int row = lane * W;
    const OutDelta od = load_out_delta(io);
    V2 P[NA], G[NA];
    if (!(io.what & VMAS_SCN_OBS)) {
        nav_load<NA>(io, bb, P, G);
        if (io.what & VMAS_SCN_REWARD) nav_reward<NA>(io, b, valid, k, lane, od, P, G);
        else if ((io.what & VMAS_SCN_DONE) && k == 0 && valid) moved(io.done, od.done)[b] = nav_done<NA>(io, P, G) ? 1 : 0;
        return;
    }
    // loads first (independent): angles, rotation, positions, goals
    float A[RM];
    float rot = 0.f;
    if (nr > 0) {
        const float* ang = io.angles[k] + (long)bb * io.ang_s0[k];
        const int as1 = io.ang_s1[k];
#pragma unroll
        for (int r = 0; r < RM; ++r) A[r] = r < nr ? ang[(long)r * as1] : 0.f;
        const VmasVec rv = io.rot[k];
        rot = ld_vec1(rv, bb);
    }
    nav_load<NA>(io, bb, P, G);
    const V2 pk = nav_sel<NA>(P, k);
    // target t is agent t (t < k) or t + 1: a uniform select between two static registers
    V2 T[TM];
    float C[TM];
#pragma unroll
    for (int t = 0; t < TM; ++t) {
        const V2 pt = t + 1 < NA ? (t < k ? P[t] : P[t + 1]) : P[t];
        const float rad = io.agents[t < k ? t : t + 1].radius;
        T[t] = t < nt ? pt - pk : mk(0.f, 0.f);
        C[t] = RayPrecise::c(rad * rad, T[t]);
    }
    nav_head<NA>(io, bb, k, P, G, S + row);
    if (io.what & VMAS_SCN_REWARD) nav_reward<NA>(io, b, valid, k, lane, od, P, G);
    else if ((io.what & VMAS_SCN_DONE) && k == 0 && valid) moved(io.done, od.done)[b] = nav_done<NA>(io, P, G) ? 1 : 0;
    lidar_row<RayPrecise, (NR > 0 && NT > 0), RM, 1>(
        S + row + H, nr, [&](int r) { return A[r] + rot; }, T, C, io.max_range, [&](int t) { return NT > 0 || t < nt; });
    // (the observation's LIDAR columns are max_range - the measurement)
    const int nv = io.batch - g0 < 64 ? io.batch - g0 : 64;
    rows_out(S, nv, W, moved(io.obs[k], od.obs) + (long)g0 * W, lane, 64,
             [&](int c, float v) { return c >= H ? io.max_range - v : v; }, io.lidar[k] + (long)g0 * nr, H, nr, lane);
}

// flocking's scripted target: u = stack([cos(t / period), sin(t / period)], dim=1) (the division
// by a Python scalar as torch's divide kernel computes it: t * (1 / period) in fp32).
__global__ void __launch_bounds__(256) k_flocking_target(const float* t, int batch, float inv, float* u) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    const float x = t[b] * inv;
    reinterpret_cast<float2*>(u)[b] = make_float2(cosf(x), sinf(x));
}

// transport.py:130-190 (restated in scenarios/transport.py).  Grid: x = 64-env groups, y = part:
// 0 the reward (every package) + done, 1 + i agent i's observation.  An observation part of a
// launch that also computes the reward recomputes on_goal (is_overlapping, deterministic) rather
// than reading part 0's output.
__global__ void __launch_bounds__(64) k_transport(VmasTransportIO io_arg) {
    VMAS_PROGRAM_ARGS(VmasTransportIO, io_arg);
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= io.batch) return;
    const OutDelta od = load_out_delta(io);
    if (blockIdx.y == 0) tr_reward_done(io, b, od);
    else tr_obs(io, b, blockIdx.y - 1, od);
}

// (the REWARD launch, workgroup 0) a spawn channel's armed words into the step's respawn words
// (VmasDiscoveryIO.stage_in / stage_out): one PCIe read while the reward runs, instead of a clear
// kernel of the respawn's own on the step's critical path
template <class IO>
__device__ __forceinline__ void disc_stage(IO& io) {
    if (io.stage_in && blockIdx.x == 0 && threadIdx.x < 3)
        io.stage_out[threadIdx.x] = __hip_atomic_load(io.stage_in + threadIdx.x, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_SYSTEM);
}

// The optional reductions over the targets (VmasDiscoveryIO.covered_count / done): the count of
// covered targets (an integer sum: exact) and all() of the all-time covered flags.
template <class IO>
__device__ __forceinline__ void disc_reductions(IO& io, int b, int T, int n_cov) {
    if (io.covered_count) io.covered_count[b] = (int64_t)n_cov;
    if (io.done) {
        bool all = true;
        for (int j = 0; j < T; ++j) all = all && io.all_time[(long)b * T + j] != 0;
        moved(io.done, load_out_delta(io).done)[b] = all ? 1 : 0;
    }
}

// discovery.py:146-246 (restated in scenarios/discovery.py), REWARD part: one thread per env.
__global__ void __launch_bounds__(64) k_discovery_reward(VmasDiscoveryIO io) {
    constexpr int MA = VMAS_DISC_MAX_AGENTS, MT = VMAS_DISC_MAX_TARGETS;
    disc_stage(io);
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= io.batch) return;
    const int A = io.n_agents, T = io.n_targets;
    V2 PA[MA], PT[MT];
#pragma unroll
    for (int i = 0; i < MA; ++i) PA[i] = i < A ? ld_vec2(io.pos[io.agent_entity[i]], b) : mk(0.f, 0.f);
#pragma unroll
    for (int j = 0; j < MT; ++j) PT[j] = j < T ? ld_vec2(io.pos[io.target_entity[j]], b) : mk(0.f, 0.f);
    // the stacks and the time reward
#pragma unroll
    for (int i = 0; i < MA; ++i)
        if (i < A) reinterpret_cast<float2*>(io.agents_pos)[(long)b * A + i] = make_float2(PA[i].x, PA[i].y);
#pragma unroll
    for (int j = 0; j < MT; ++j)
        if (j < T) reinterpret_cast<float2*>(io.targets_pos)[(long)b * T + j] = make_float2(PT[j].x, PT[j].y);
    if (io.time_int) reinterpret_cast<int64_t*>(io.time_rew)[b] = io.time_penalty_i;  // torch.full(int)
    else reinterpret_cast<float*>(io.time_rew)[b] = io.time_penalty;
    // torch.cdist (p = 2): sqrt(fl(fl(d0^2) + fl(d1^2))); per target the count of agents in range
    int cnt[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) cnt[j] = 0;
#pragma unroll
    for (int i = 0; i < MA; ++i) {
        if (i >= A) continue;
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            if (j >= T) continue;
            const float d0 = PA[i].x - PT[j].x, d1 = PA[i].y - PT[j].y;
            const float d = sqrtf(d0 * d0 + d1 * d1);
            io.dists[((long)b * A + i) * T + j] = d;
            cnt[j] += (d < io.covering_range) ? 1 : 0;
        }
    }
    bool cov[MT];
    int n_cov = 0;
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        cov[j] = cnt[j] >= io.agents_per_target;
        if (j < T) {
            io.per_target[(long)b * T + j] = (int64_t)cnt[j];
            io.covered[(long)b * T + j] = cov[j] ? 1 : 0;
            n_cov += cov[j] ? 1 : 0;
        }
    }
    disc_reductions(io, b, T, n_cov);
    // agent_reward: covering_reward[:] = 0; += (count of covered targets in range) * coeff;
    // shared[:] = 0; += each agent's covering reward in agent order; halved where nonzero
    float shared = 0.f;
    float covr[MA];
#pragma unroll
    for (int i = 0; i < MA; ++i) {
        covr[i] = 0.f;
        if (i >= A) continue;
        int n = 0;
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            if (j >= T) continue;
            const float d0 = PA[i].x - PT[j].x, d1 = PA[i].y - PT[j].y;
            n += (sqrtf(d0 * d0 + d1 * d1) < io.covering_range && cov[j]) ? 1 : 0;
        }
        covr[i] = 0.f + (float)n * io.covering_rew_coeff;
        io.covering[i][b] = covr[i];
        shared = shared + covr[i];
    }
    if (shared != 0.f) shared = shared / 2.f;
    io.shared[b] = shared;
#pragma unroll
    for (int i = 0; i < MA; ++i) {
        if (i >= A) continue;
        io.collision[i][b] = 0.f;  // collision_rew[:] = 0 (penalty 0: nothing added)
        const float cv = io.shared_reward ? shared : covr[i];
        moved(io.rewards[i], load_out_delta(io).rew)[b] = (0.f + cv) + io.time_penalty;  // collision_rew + covering_rew + time_rew
    }
}

// discovery.py:248-255, OBS part: one thread per (env, agent, part).
__global__ void __launch_bounds__(64) k_discovery_obs(VmasDiscoveryIO io) {
    constexpr int ME = VMAS_DISC_MAX_ENTITIES;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= io.batch) return;
    int rays = 0;
    for (int s = 0; s < io.n_lidars; ++s) rays += io.n_rays[s];
    const int parts = 1 + rays, a = blockIdx.y / parts, part = blockIdx.y - a * parts;
    const int self = io.agent_entity[a], W = 4 + rays;
    const V2 p = ld_vec2(io.pos[self], b);
    float* o = moved(io.obs[a], load_out_delta(io).obs) + (long)b * W;
    if (part == 0) {
        const V2 v = ld_vec2(io.vel[a], b);
        o[0] = p.x;
        o[1] = p.y;
        o[2] = v.x;
        o[3] = v.y;
        return;
    }
    int r = part - 1, s = 0, col = 4;
    while (s + 1 < io.n_lidars && r >= io.n_rays[s]) {
        r -= io.n_rays[s];
        col += io.n_rays[s];
        ++s;
    }
    const uint32_t mask = io.mask[s] & ~(1u << self);  // World.cast_rays skips the entity itself
    const float ang = io.angles[s][a][(long)b * io.ang_s0[s][a] + (long)r * io.ang_s1[s][a]] + ld_vec1(io.rot[a], b);
    const float dc = cosf(ang), ds = sinf(ang), mr = io.max_range[s];
    float best = mr;
#pragma unroll
    for (int e = 0; e < ME; ++e)  // (spheres: checked by the host entry point)
        if (e < io.n_entities && ((mask >> e) & 1u)) best = tmin(best, ray_sphere(p, dc, ds, ld_vec2(io.pos[e], b), io.radius[e], mr));
    io.lidar[s][a][(long)b * io.n_rays[s] + r] = best;
    o[col + r] = best;
}

// REWARD with a wave per agent (k_discovery_reward has one thread per env: 256 waves for 16 384
// envs, 31.5 us): lane = env of the workgroup's 64, wave i = agent i.  The agents' in-range bits
// meet in LDS for the per-target counts; wave 0 sums the covering rewards in agent order (the
// reference's loop order: bit-identical); the [64 x A x T] distances and the stacks are staged in
// LDS and written out as contiguous blocks.
constexpr int kDiscFastAgents = 16, kDiscFastTargets = 16;
__global__ void __launch_bounds__(1024) k_discovery_reward_fast(VmasDiscoveryIO io_arg) {
    VMAS_PROGRAM_ARGS(VmasDiscoveryIO, io_arg);
    disc_stage(io);
    constexpr int MT = kDiscFastTargets;
    __shared__ float D[64 * kDiscFastAgents * kDiscFastTargets];  // dists rows of the 64 envs (64 KiB)
    __shared__ uint32_t IN[kDiscFastAgents][64];                  // agent i's in-range target bits
    __shared__ float CR[kDiscFastAgents][64];                     // agent i's covering reward
    __shared__ float SH[64];
    const int lane = (int)(threadIdx.x & 63u);
    const int i = wave_uniform((int)(threadIdx.x >> 6));
    const int A = io.n_agents, T = io.n_targets, g0 = (int)blockIdx.x * 64, b = g0 + lane;
    const bool valid = b < io.batch;
    const int bb = valid ? b : io.batch - 1;
    const int nv = io.batch - g0 < 64 ? io.batch - g0 : 64;
    V2 PT[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        const VmasVec pv = io.pos[io.target_entity[j < T ? j : 0]];
        PT[j] = j < T ? ld_vec2(pv, bb) : mk(0.f, 0.f);
    }
    const VmasVec av = io.pos[io.agent_entity[i]];
    const V2 pa = ld_vec2(av, bb);
    // torch.cdist (p = 2): sqrt(fl(fl(d0^2) + fl(d1^2))); agent i's distances and in-range bits
    uint32_t in = 0u;
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        if (j >= T) continue;
        const float d0 = pa.x - PT[j].x, d1 = pa.y - PT[j].y;
        const float d = sqrtf(d0 * d0 + d1 * d1);
        D[(lane * A + i) * T + j] = d;
        in |= (d < io.covering_range) ? (1u << j) : 0u;
    }
    IN[i][lane] = in;
    __syncthreads();
    // per target: the count of agents in range, covered when >= agents_per_target
    uint32_t covm = 0u;
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        if (j >= T) continue;
        int cnt = 0;
        for (int k = 0; k < A; ++k) cnt += (IN[k][lane] >> j) & 1u;
        covm |= cnt >= io.agents_per_target ? (1u << j) : 0u;
        if (i == 0 && valid) {
            io.per_target[(long)b * T + j] = (int64_t)cnt;
            io.covered[(long)b * T + j] = cnt >= io.agents_per_target ? 1 : 0;
        }
    }
    if (i == 1 % A && valid) disc_reductions(io, b, T, __builtin_popcount(covm));
    // agent i's covering reward: (count of covered targets in range) * coeff
    const float covr = 0.f + (float)__builtin_popcount(in & covm) * io.covering_rew_coeff;
    CR[i][lane] = covr;
    if (valid) {
        io.covering[i][b] = covr;
        io.collision[i][b] = 0.f;  // collision_rew[:] = 0 (penalty 0: nothing added)
    }
    __syncthreads();
    if (i == 0) {  // shared[:] = 0; += each agent's covering reward in agent order; halved where nonzero
        float shared = 0.f;
        for (int k = 0; k < A; ++k) shared = shared + CR[k][lane];
        if (shared != 0.f) shared = shared / 2.f;
        SH[lane] = shared;
        if (valid) {
            io.shared[b] = shared;
            if (io.time_int) reinterpret_cast<int64_t*>(io.time_rew)[b] = io.time_penalty_i;  // torch.full(int)
            else reinterpret_cast<float*>(io.time_rew)[b] = io.time_penalty;
        }
    }
    __syncthreads();
    if (valid) {
        const float cv = io.shared_reward ? SH[lane] : covr;
        moved(io.rewards[i], load_out_delta(io).rew)[b] = (0.f + cv) + io.time_penalty;  // collision_rew + covering_rew + time_rew
    }
    // the stacks and the distances as contiguous blocks of the workgroup's envs
    const int tid = (int)threadIdx.x, nth = (int)blockDim.x;
    float* dists = io.dists + (long)g0 * A * T;
    for (int k = tid; k < nv * A * T; k += nth) dists[k] = D[k];
    float2* ap = reinterpret_cast<float2*>(io.agents_pos) + (long)g0 * A;
    float2* tp = reinterpret_cast<float2*>(io.targets_pos) + (long)g0 * T;
    for (int k = tid; k < nv * A; k += nth) {
        const int e = k / A, a = k - e * A;
        const VmasVec v = io.pos[io.agent_entity[a]];
        ap[k] = make_float2(v.p[(long)(g0 + e) * v.s0], v.p[(long)(g0 + e) * v.s0 + v.s1]);
    }
    for (int k = tid; k < nv * T; k += nth) {
        const int e = k / T, j = k - e * T;
        const VmasVec v = io.pos[io.target_entity[j]];
        tp[k] = make_float2(v.p[(long)(g0 + e) * v.s0], v.p[(long)(g0 + e) * v.s0 + v.s1]);
    }
}

// OBS with the fast LIDAR (io.fast_lidar): a wave per (64 envs, agent), every ray of its LIDARs
// from the entity positions loaded once, the direct ray-sphere form with hardware sin / cos /
// sqrt (as k_flocking_fast), the observation rows staged in LDS and written as contiguous blocks.
constexpr int kDiscFastEntities = 16, kDiscFastRays = 16;  // per LIDAR
constexpr int kDiscFastW = 4 + VMAS_DISC_MAX_LIDARS * kDiscFastRays;
__global__ void __launch_bounds__(256) k_discovery_obs_fast(VmasDiscoveryIO io_arg) {
    VMAS_PROGRAM_ARGS(VmasDiscoveryIO, io_arg);
    constexpr int ME = kDiscFastEntities, RM = kDiscFastRays;
    __shared__ float S[4][64 * kDiscFastW];
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const int a = wave_uniform((int)blockIdx.y * 4 + w);
    if (a >= io.n_agents) return;  // (wave-uniform; no workgroup barrier below)
    const int g0 = (int)blockIdx.x * 64, b = g0 + lane;
    const bool valid = b < io.batch;
    const int bb = valid ? b : io.batch - 1;
    const int nv = io.batch - g0 < 64 ? io.batch - g0 : 64;
    const int self = io.agent_entity[a], ne = io.n_entities;
    int rays = 0;
    for (int s = 0; s < io.n_lidars; ++s) rays += io.n_rays[s];
    const int W = 4 + rays, row = lane * W;
    const VmasVec sp = io.pos[self], vv = io.vel[a], rv = io.rot[a];
    const V2 p = ld_vec2(sp, bb), v = ld_vec2(vv, bb);
    const float rot = ld_vec1(rv, bb);
    V2 T[ME];
    float R2[ME];
#pragma unroll
    for (int e = 0; e < ME; ++e) {
        const VmasVec ev = io.pos[e < ne ? e : 0];
        const float rad = io.radius[e < ne ? e : 0];
        T[e] = e < ne ? ld_vec2(ev, bb) - p : mk(0.f, 0.f);
        R2[e] = rad * rad;
    }
    S[w][row + 0] = p.x;
    S[w][row + 1] = p.y;
    S[w][row + 2] = v.x;
    S[w][row + 3] = v.y;
    float C[ME];
#pragma unroll
    for (int e = 0; e < ME; ++e) C[e] = R2[e] - (T[e].x * T[e].x + T[e].y * T[e].y);
    int col = 4;
    for (int s = 0; s < io.n_lidars; ++s) {
        const uint32_t mask = io.mask[s] & ~(1u << self);  // World.cast_rays skips the entity itself
        const int nr = io.n_rays[s];
        const float* ang = io.angles[s][a] + (long)bb * io.ang_s0[s][a];
        const int as1 = io.ang_s1[s][a];
        lidar_row<RayHardware, false, RM, 2>(
            S[w] + row + col, nr, [&](int r) { return ang[(long)r * as1] + rot; }, T, C, io.max_range[s],
            [&](int e) { return e < ne && ((mask >> e) & 1u); });
        rows_out(S[w], nv, W, nullptr, 0, 0, nullptr, io.lidar[s][a] + (long)g0 * nr, col, nr, lane);
        col += nr;
    }
    rows_out(S[w], nv, W, moved(io.obs[a], load_out_delta(io).obs) + (long)g0 * W, lane, 64, nullptr, nullptr, 0, 0, lane);
}

// The same program with a wave per (64 envs, agent, LIDAR) instead of per (64 envs, agent): L
// waves of one workgroup share an agent's observation rows in LDS, each casting one LIDAR's rays
// (the same operations per ray, in the same order: bit-identical), and write the rows out together
// after one barrier.  At C4 (16 384 envs, 8 agents, 2 LIDARs) the per-agent form ran 2 048 waves,
// 2 per SIMD, too few to hide the trig / sqrt / LDS latencies; this runs 4 096.
template <int L>
__global__ void __launch_bounds__(256) k_discovery_obs_split(VmasDiscoveryIO io_arg) {
    VMAS_PROGRAM_ARGS(VmasDiscoveryIO, io_arg);
    constexpr int ME = kDiscFastEntities, RM = kDiscFastRays, AP = 4 / L;
    __shared__ float S[AP][64 * kDiscFastW];
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const int sub = w / L, s = w - sub * L;
    const int a = wave_uniform((int)blockIdx.y * AP + sub);
    const bool active = a < io.n_agents;  // (no early return: the barrier below)
    const int g0 = (int)blockIdx.x * 64, b = g0 + lane;
    const bool valid = b < io.batch;
    const int bb = valid ? b : io.batch - 1;
    const int nv = io.batch - g0 < 64 ? io.batch - g0 : 64;
    int rays = 0, col = 4;
    for (int k = 0; k < L; ++k) {
        rays += io.n_rays[k];
        if (k < s) col += io.n_rays[k];
    }
    const int W = 4 + rays, row = lane * W;
    if (active) {
        const int self = io.agent_entity[a], ne = io.n_entities;
        const VmasVec sp = io.pos[self], rv = io.rot[a];
        const V2 p = ld_vec2(sp, bb);
        const float rot = ld_vec1(rv, bb);
        if (s == 0) {
            const V2 v = ld_vec2(io.vel[a], bb);
            S[sub][row + 0] = p.x;
            S[sub][row + 1] = p.y;
            S[sub][row + 2] = v.x;
            S[sub][row + 3] = v.y;
        }
        V2 T[ME];
        float C[ME];
#pragma unroll
        for (int e = 0; e < ME; ++e) {
            const VmasVec ev = io.pos[e < ne ? e : 0];
            const float rad = io.radius[e < ne ? e : 0];
            T[e] = e < ne ? ld_vec2(ev, bb) - p : mk(0.f, 0.f);
            C[e] = rad * rad - (T[e].x * T[e].x + T[e].y * T[e].y);
        }
        const uint32_t mask = io.mask[s] & ~(1u << self);  // World.cast_rays skips the entity itself
        const int nr = io.n_rays[s];
        const float* ang = io.angles[s][a] + (long)bb * io.ang_s0[s][a];
        const int as1 = io.ang_s1[s][a];
        lidar_row<RayHardware, false, RM, 2>(
            S[sub] + row + col, nr, [&](int r) { return ang[(long)r * as1] + rot; }, T, C, io.max_range[s],
            [&](int e) { return e < ne && ((mask >> e) & 1u); });
        // (this wave's own columns: no barrier needed)
        rows_out(S[sub], nv, W, nullptr, 0, 0, nullptr, io.lidar[s][a] + (long)g0 * nr, col, nr, lane);
    }
    __syncthreads();
    if (!active) return;
    rows_out(S[sub], nv, W, moved(io.obs[a], load_out_delta(io).obs) + (long)g0 * W, lane + s * 64, 64 * L, nullptr, nullptr,
             0, 0, lane);
}

// ---- sampling (sampling.py `sample` / `reward` / `observation` / `nomrlize_pdf`; restated in
// scenarios/sampling.py) ---------------------------------------------------------------------------
// The per-(env, agent) program and the grid-point density are host / device functions: the kernels
// below and the host backend (device == -1) run the same statements.  IO is the argument block by
// reference -- on the device read in place from the kernel argument segment (VMAS_PROGRAM_ARGS).
#define VMAS_SAMP_HD __host__ __device__ __forceinline__
constexpr int kSampMA = VMAS_SAMPLING_MAX_AGENTS, kSampMG = VMAS_SAMPLING_MAX_GAUSSIANS;

// torch.clamp_(x, -m, m): NaN stays NaN
VMAS_SAMP_HD float samp_clamp(float x, float m) { return x != x ? x : fminf(fmaxf(x, -m), m); }
// torch.maximum: NaN propagates
VMAS_SAMP_HD float samp_max(float a, float b) { return (a != a) ? a : ((b != b || b > a) ? b : a); }

template <class IO>
VMAS_SAMP_HD bool samp_oob(IO& io, float x, float y) {
    return (x < -io.grid.xdim) || (x > io.grid.xdim) || (y < -io.grid.ydim) || (y > io.grid.ydim);
}
// the cell of a (clamped) point as ix * n_y + iy, or -1 when it indexes past the grid (never read
// or written: the reference raises there)
template <class IO>
VMAS_SAMP_HD int samp_cell(IO& io, float x, float y) {
    const float gs = io.grid.grid_spacing, inv = io.grid.inv_grid_spacing;
    const float fx = (io.grid.div_mode ? x * inv : x / gs) + io.grid.half_nx;
    const float fy = (io.grid.div_mode ? y * inv : y / gs) + io.grid.half_ny;
    // .to(torch.long) truncates towards zero; NaN fails every comparison
    const bool ok = fx > -1.f && fx < (float)io.grid.n_x && fy > -1.f && fy < (float)io.grid.n_y;
    return ok ? (int)fx * io.grid.n_y + (int)fy : -1;
}
// n floats summed as torch's .sum(-1) over a contiguous last dim: element j goes to accumulator
// j % acc, the accumulators are combined by an adjacent-pair tree (see flock_part0; every value is
// >= +0 or NaN, so 0 + e == e).  Static register indices only.
template <int M>
VMAS_SAMP_HD void samp_acc_add(float* y, int slot, float e) {
#pragma unroll
    for (int i = 0; i < M; ++i)
        if (i == slot) y[i] = y[i] + e;
}
template <int M>
VMAS_SAMP_HD float samp_acc_tree(float* y, int n, int acc) {
    const int m = n < acc ? n : acc;
#pragma unroll
    for (int w = 1; w < M; w *= 2)
#pragma unroll
        for (int i = 0; i + w < M; i += 2 * w)
            if (i + w < m) y[i] = y[i] + y[i + w];
    return y[0];
}
// Gaussian g's term of the density at (x, y), its location (lx, ly) given
template <class IO>
VMAS_SAMP_HD float samp_term(IO& io, int g, float x, float y, float lx, float ly) {
    const float L = io.density.scale[g];
    const float y0 = (x - lx) / L, y1 = (y - ly) / L;
    const float M = y0 * y0 + y1 * y1;
    const float lg = (-0.5f * (io.density.log_norm + M)) - io.density.half_log_det[g];
    return expf(lg);
}
// the unnormalised density of (x, y) in env b (include/vmas_mi355x.h, "sampling")
template <class IO>
VMAS_SAMP_HD float samp_density(IO& io, long b, float x, float y) {
    float acc[kSampMG];
#pragma unroll
    for (int i = 0; i < kSampMG; ++i) acc[i] = 0.f;
    const int ng = io.density.n_gaussians, am = io.density.sum_mode - 1;
#pragma unroll 1
    for (int g = 0; g < ng; ++g) {
        const float* lp = io.density.loc[g].p;
        const long s0 = io.density.loc[g].s0, s1 = io.density.loc[g].s1;
        samp_acc_add<kSampMG>(acc, g & am, samp_term(io, g, x, y, lp[b * s0], lp[b * s0 + s1]));
    }
    return samp_acc_tree<kSampMG>(acc, ng, io.density.sum_mode);
}
// The same with the env's locations by value (k_sampling_reset: drawn by this wave, held in
// registers -- the loop is unrolled so that every index is static).
struct SampLocs {
    float x[kSampMG], y[kSampMG];
};
template <class IO>
VMAS_SAMP_HD float samp_density_at(IO& io, const SampLocs& l, float x, float y) {
    float acc[kSampMG];
#pragma unroll
    for (int i = 0; i < kSampMG; ++i) acc[i] = 0.f;
    const int ng = io.density.n_gaussians, am = io.density.sum_mode - 1;
#pragma unroll
    for (int g = 0; g < kSampMG; ++g)
        if (g < ng) samp_acc_add<kSampMG>(acc, g & am, samp_term(io, g, x, y, l.x[g], l.y[g]));
    return samp_acc_tree<kSampMG>(acc, ng, io.density.sum_mode);
}
// sample(p, norm=False) of a grid point of nomrlize_pdf (the flags were cleared just before);
// density(x, y): the env's density at a clamped point
template <class IO, class D>
VMAS_SAMP_HD float samp_grid_point_of(IO& io, float x, float y, D&& density) {
    const bool oob = samp_oob(io, x, y);
    const float v = density(samp_clamp(x, io.grid.x_semidim), samp_clamp(y, io.grid.y_semidim));
    return oob ? 0.f : v;
}
template <class IO>
VMAS_SAMP_HD float samp_grid_point(IO& io, long b, float x, float y) {
    return samp_grid_point_of(io, x, y, [&](float cx, float cy) { return samp_density(io, b, cx, cy); });
}

// Agent k in env b.  REWARD (k == 0 only; the reward block of every agent): flags are read before any
// is written, an agent's sample is zero where its cell was sampled before or an earlier agent is in
// it.  OBS: row `o` ([4 + n_rays + 8]) and, when `lid` is given, the LIDAR row.  Other (env, agent)
// threads of the launch run beside this one: they read the positions this one clamps (clamping is
// idempotent) and the flags it sets (a probe is zero where the cell was sampled before OR an agent is
// in it now, whichever of the two the load returns).  Formally these cross-wave reads of `pos` and
// `sampled` beside agent 0's stores are data races; they are benign by construction: every value is
// a 4-byte (position) or 1-byte (flag) store, and either value a load can return gives the same
// result.  Known costs, not measured apart: every (env, agent) thread reloads, clamps and cells all
// NA agents (n^2 loads per env), and a lane writes its LDS row at a stride of W = 24 floats (8-way
// bank conflicts on the row writes; the copy-out reads are conflict-free).
template <int NA, class IO>
VMAS_SAMP_HD void samp_agent(IO& io, long b, int k, float* o, float* lid, long long rew_delta) {
    const int n = io.n_agents;
    const bool rew = (io.what & VMAS_SCN_REWARD) != 0;
    const float xs = io.grid.x_semidim, ys = io.grid.y_semidim;
    float CX[NA], CY[NA];
    int CELL[NA];
    bool OOB[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        CX[j] = CY[j] = 0.f;
        CELL[j] = -1;
        OOB[j] = false;
        if (j >= n) continue;
        const float* pp = io.pos[j].p;
        const long s0 = io.pos[j].s0, s1 = io.pos[j].s1;
        float x = pp[b * s0], y = pp[b * s0 + s1];
        if (rew) {
            OOB[j] = samp_oob(io, x, y);
            x = samp_clamp(x, xs);
            y = samp_clamp(y, ys);
            CELL[j] = samp_cell(io, x, y);
        }
        CX[j] = x;
        CY[j] = y;
    }
    uint8_t* flags = io.sampled + b * ((long)io.grid.n_x * io.grid.n_y);
    const float mp = io.max_pdf[b];
    if (rew && k == 0) {
        bool Z[NA], F[NA];
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            F[j] = CELL[j] >= 0 && flags[CELL[j]] != 0;
            Z[j] = OOB[j] || F[j];
#pragma unroll
            for (int i = 0; i < j; ++i) Z[j] = Z[j] || (CELL[j] >= 0 && CELL[i] == CELL[j]);
        }
        float acc[NA];
#pragma unroll
        for (int j = 0; j < NA; ++j) acc[j] = 0.f;
        float V[NA];
        const int am = io.agent_sum_mode - 1;
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            V[j] = 0.f;
            if (j >= n) continue;
            float v = samp_density(io, b, CX[j], CY[j]);
            if (io.norm) v = v / mp;
            V[j] = Z[j] ? 0.f : v;
            samp_acc_add<NA>(acc, j & am, V[j]);
            float* pp = io.pos[j].p;
            const long s0 = io.pos[j].s0, s1 = io.pos[j].s1;
            pp[b * s0] = CX[j];
            pp[b * s0 + s1] = CY[j];
            io.sample[j][b] = V[j];
            if (CELL[j] >= 0) flags[CELL[j]] = 1;
            if (io.undo) io.undo[b * n + j] = (CELL[j] >= 0 && !F[j]) ? CELL[j] : -1;
        }
        const float s = samp_acc_tree<NA>(acc, n, io.agent_sum_mode);
        io.sampling_rew[b] = s;
#pragma unroll
        for (int j = 0; j < NA; ++j)
            if (j < n) reinterpret_cast<float*>(reinterpret_cast<char*>(io.rewards[j]) + rew_delta)[b] = io.shared_rew ? s : V[j];
    }
    if (!(io.what & VMAS_SCN_OBS)) return;
    float px = 0.f, py = 0.f;
#pragma unroll
    for (int j = 0; j < NA; ++j)
        if (j == k) {
            px = CX[j];
            py = CY[j];
        }
    const float* vp = io.vel[k].p;
    const long vs0 = io.vel[k].s0, vs1 = io.vel[k].s1;
    o[0] = px;
    o[1] = py;
    o[2] = vp[b * vs0];
    o[3] = vp[b * vs0 + vs1];
    const int nr = io.lidar_on ? io.n_rays : 0;
    if (nr > 0) {
        // Lidar.measure = World.cast_rays(angles + agent rot) over the other agents, in order
        const float* ang = io.angles[k] + b * (long)io.ang_s0[k];
        const long as1 = io.ang_s1[k];
        const float rot = io.rot[k].p[b * (long)io.rot[k].s0];
        const float mr = io.max_range;
#pragma unroll 1
        for (int r = 0; r < nr; ++r) {
            const float a = ang[r * as1] + rot;
            float best = mr;
#ifdef __HIP_DEVICE_COMPILE__
            if (io.fast_lidar) {  // (the targets formed per ray, as the exact branch does)
                Ray<RayPrecise> q(a, mr);
                cast_rays<RayPrecise, NA>(
                    [&](int j, float& ux, float& uy, float& c) {
                        if (j >= n || j == k) return false;
                        const float rad = io.radius[j];
                        ux = CX[j] - px;
                        uy = CY[j] - py;
                        c = RayPrecise::c(rad * rad, mk(ux, uy));
                        return true;
                    },
                    q);
                best = q.best;
            } else
#endif
            {
                const float dc = cosf(a), ds = sinf(a);
#pragma unroll
                for (int j = 0; j < NA; ++j)
                    if (j < n && j != k) best = tmin(best, ray_sphere(mk(px, py), dc, ds, mk(CX[j], CY[j]), io.radius[j], mr));
            }
            o[4 + r] = best;
            if (lid) lid[r] = best;
        }
    }
    // the probes: sample(pos + d) with norm = True, no flag update
    const float s = io.grid.grid_spacing;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float dx = (i == 0 || i == 5 || i == 7) ? s : ((i == 1 || i == 4 || i == 6) ? -s : 0.f);
        const float dy = (i == 2 || i == 6 || i == 7) ? s : ((i == 3 || i == 4 || i == 5) ? -s : 0.f);
        float qx = px + dx, qy = py + dy;
        bool z = samp_oob(io, qx, qy);
        qx = samp_clamp(qx, xs);
        qy = samp_clamp(qy, ys);
        const int c = samp_cell(io, qx, qy);
        if (c >= 0) {
            z = z || flags[c] != 0;
#pragma unroll
            for (int j = 0; j < NA; ++j) z = z || CELL[j] == c;  // (REWARD | OBS: the cells marked by this launch)
        }
        const float v = samp_density(io, b, qx, qy) / mp;
        o[4 + nr + i] = z ? 0.f : v;
    }
}

// Grid: x = 64-env groups, y = groups of 4 agents; a wave per (64 envs, agent), the observation rows
// staged in LDS (4 x 64 x W floats, sized by the launch), as k_navigation_fast.  NA: the static bound
// of the agent loops (4, 8 or 16: the least >= n_agents).
template <int NA>
__global__ void __launch_bounds__(256) k_sampling(VmasSamplingIO io_arg) {
    VMAS_PROGRAM_ARGS(VmasSamplingIO, io_arg);
    extern __shared__ float samp_lds[];
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const int g0 = (int)blockIdx.x * 64, b = g0 + lane;
    const int k = wave_uniform((int)blockIdx.y * 4 + w);
    if (k >= io.n_agents) return;  // (wave-uniform; no workgroup barrier below)
    const bool valid = b < io.batch;
    const int nr = io.lidar_on ? io.n_rays : 0, W = 12 + nr;
    float* S = samp_lds + w * 64 * W;
    const OutDelta od = load_out_delta(io);
    if (!(io.what & VMAS_SCN_OBS)) {
        if (valid && k == 0) samp_agent<NA>(io, (long)b, 0, nullptr, nullptr, od.rew);
        return;
    }
    if (valid) samp_agent<NA>(io, (long)b, k, S + lane * W, nullptr, od.rew);
    __builtin_amdgcn_wave_barrier();
    const int nv = io.batch - g0 < 64 ? io.batch - g0 : 64;
    rows_out(S, nv, W, moved(io.obs[k], od.obs) + (long)g0 * W, lane, 64, nullptr, io.lidar[k] + (long)g0 * nr, 4, nr, lane);
}

// nomrlize_pdf: a wave per env, lanes over the grid points, then the wave's maximum (order-free).
__global__ void __launch_bounds__(256) k_sampling_max_pdf(VmasSamplingMaxPdfIO io_arg) {
    VMAS_PROGRAM_ARGS(VmasSamplingMaxPdfIO, io_arg);
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const int b = wave_uniform((int)blockIdx.x * 4 + w);
    if (b >= io.batch) return;
    if (io.mask && !io.mask[b]) return;
    const int ny = io.n_ys, P = io.n_xs * ny;
    float m = 0.f;  // (max_pdf[:] = 0 before the loop)
    for (int p = lane; p < P; p += 64) {
        const int ix = p / ny, iy = p - ix * ny;
        m = samp_max(m, samp_grid_point(io, (long)b, io.xs[ix], io.ys[iy]));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = samp_max(m, __shfl_xor(m, off, 64));
    if (lane == 0) io.max_pdf[b] = m;
}

// sampling.py `reset_world_at(None)` after World.reset for the envs of a mask (include/vmas_mi355x.h
// vmas_sampling_reset has the order).  A wave per env, as k_sampling_max_pdf; a wave whose env is
// outside the mask returns before any cross-lane operation (the test is wave-uniform) having read its
// mask byte only.  Lane l < 2 G + 2 A draws column l of the call (uniform_at: element b of the full
// reset's uniform_ call on [B, 1]); the Gaussians' locations reach every lane by readlane, never by a
// store another lane loads back -- `_locs` is written as a side effect.  Lanes then stride the grid
// points for the maximum and the flag row to clear it; the first A lanes do the agents.
__global__ void __launch_bounds__(256) k_sampling_reset(VmasSamplingResetIO io_arg, vmas_uniform::DrawGrid dg) {
    VMAS_PROGRAM_ARGS(VmasSamplingResetIO, io_arg);
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const int b = wave_uniform((int)blockIdx.x * 4 + w);
    if (b >= io.batch || io.mask[b] == 0) return;
    const int ng = io.density.n_gaussians, na = io.n_agents;
    // 1. every draw of the env: columns [0, 2 G) the locations, [2 G, 2 G + 2 A) the agents' spawns
    const bool is_loc = lane < 2 * ng, y_axis = (lane & 1) != 0;
    const float lo = is_loc ? (y_axis ? io.loc_lo[1] : io.loc_lo[0]) : (y_axis ? io.spawn_lo[1] : io.spawn_lo[0]);
    const float hi = is_loc ? (y_axis ? io.loc_hi[1] : io.loc_hi[0]) : (y_axis ? io.spawn_hi[1] : io.spawn_hi[0]);
    float u = 0.f;
    if (lane < 2 * (ng + na))
        u = vmas_uniform::uniform_at(io.seed, io.offset + dg.inc * (unsigned long long)lane, dg, b, lo, hi, io.mode);
    SampLocs L;
#pragma unroll
    for (int g = 0; g < kSampMG; ++g) {
        L.x[g] = __shfl(u, 2 * g, 64);
        L.y[g] = __shfl(u, 2 * g + 1, 64);
        if (g < ng && (lane >> 1) == g) {
            const VmasVec v = io.density.loc[g];
            const_cast<float*>(v.p)[(long)b * v.s0 + (y_axis ? v.s1 : 0)] = u;
        }
    }
    const int src = 2 * ng + 2 * (lane < na ? lane : 0);
    const float sx = __shfl(u, src, 64), sy = __shfl(u, src + 1, 64);
    // 2. nomrlize_pdf: max_pdf[b] = 0, then the maximum over the grid points (order-free)
    const int ny = io.n_ys, P = io.n_xs * ny;
    float m = 0.f;
    for (int p = lane; p < P; p += 64) {
        const int ix = p / ny, iy = p - ix * ny;
        m = samp_max(m, samp_grid_point_of(io, io.xs[ix], io.ys[iy],
                                           [&](float cx, float cy) { return samp_density_at(io, L, cx, cy); }));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = samp_max(m, __shfl_xor(m, off, 64));
    if (lane == 0) {
        io.max_pdf[b] = m;
        if (io.steps) io.steps[b] = 0.f;
    }
    // sampled[b] = False: 16 bytes per store where the rows allow it
    const long cells = (long)io.grid.n_x * io.grid.n_y;
    uint8_t* flags = io.sampled + (long)b * cells;
    if ((((unsigned long long)cells | (unsigned long long)(uintptr_t)io.sampled) & 15ull) == 0) {
        uint4* f = reinterpret_cast<uint4*>(flags);
        for (long i = lane; i < cells / 16; i += 64) f[i] = make_uint4(0u, 0u, 0u, 0u);
    } else {
        for (long i = lane; i < cells; i += 64) flags[i] = 0;
    }
    // 3. the agents: set_pos(spawn), then sample(pos, norm) -- the clamp in place, zero where the
    // drawn point is out of bounds (the cell's flag was cleared above)
    if (lane >= na) return;
    const bool oob = samp_oob(io, sx, sy);
    const float cx = samp_clamp(sx, io.grid.x_semidim), cy = samp_clamp(sy, io.grid.y_semidim);
    float v = samp_density_at(io, L, cx, cy);
    if (io.norm) v = v / m;
    const VmasResetEntity e = io.agents[lane];
    reset_place(e, b, mk(cx, cy));
    const VmasMutVec f = io.force[lane], t = io.torque[lane];
    put2(f, b, 0.f, 0.f);
    put1(t, b, 0.f);
    io.sample[lane][b] = oob ? 0.f : v;
}

const char* samp_density_error(const VmasSamplingGrid& g, const VmasSamplingDensity& d) {
    if (g.n_x <= 0 || g.n_y <= 0 || (long)g.n_x * g.n_y > (1L << 30)) return "grid size";
    if (g.div_mode != 0 && g.div_mode != 1) return "division mode";
    if (d.n_gaussians < 1 || d.n_gaussians > VMAS_SAMPLING_MAX_GAUSSIANS) return "Gaussian count";
    if (d.sum_mode < 1 || d.sum_mode > VMAS_SAMPLING_MAX_GAUSSIANS || (d.sum_mode & (d.sum_mode - 1))) return "sum mode";
    for (int i = 0; i < d.n_gaussians; ++i)
        if (!d.loc[i].p) return "null Gaussian location";
    return nullptr;
}

// ---- wheel and dispersion (vmas_light_programs.hpp has the row functions) ------------------------------
// Both programs move a few hundred bytes per env and are launch-latency-bound at every measured size,
// so the mapping is the plainest one that stores coalesced: a thread per env, a wave per 64 envs; per
// agent the wave stages its 64 observation rows in LDS (4 x 64 x W floats, sized by the launch) and
// stores them as ONE contiguous block (a lane storing its own row writes 4-byte values 4 W bytes
// apart).  One thread computes everything of its env, so the dispersion flags have one writer and no
// other thread reads them: no atomics, no ordering between threads.
__global__ void __launch_bounds__(256) k_wheel(VmasWheelIO io_arg) {
    VMAS_PROGRAM_ARGS(VmasWheelIO, io_arg);
    extern __shared__ float light_lds[];
    constexpr int W = 13;
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const int g0 = wave_uniform(((int)blockIdx.x * 4 + w) * 64), b = g0 + lane;
    if (g0 >= io.batch) return;  // (wave-uniform; no workgroup barrier below)
    const bool valid = b < io.batch;
    const OutDelta od = load_out_delta(io);
    if (valid && (io.what & VMAS_SCN_REWARD)) {
        const float r = vmas_light::wheel_rew(io, (long)b);
        io.rew[b] = r;
        for (int k = 0; k < io.n_agents; ++k) moved(io.rewards[k], od.rew)[b] = -r;
    }
    if (!(io.what & VMAS_SCN_OBS)) return;
    float* S = light_lds + w * 64 * W;
    const int nv = io.batch - g0 < 64 ? io.batch - g0 : 64;
    for (int k = 0; k < io.n_agents; ++k) {
        if (valid) vmas_light::wheel_obs_row(io, (long)b, k, S + lane * W);
        __builtin_amdgcn_wave_barrier();
        rows_out(S, nv, W, moved(io.obs[k], od.obs) + (long)g0 * W, lane, 64, nullptr, (float*)nullptr, 0, 0, lane);
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ void __launch_bounds__(256) k_dispersion(VmasDispersionIO io_arg) {
    VMAS_PROGRAM_ARGS(VmasDispersionIO, io_arg);
    extern __shared__ float light_lds[];
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const int g0 = wave_uniform(((int)blockIdx.x * 4 + w) * 64), b = g0 + lane;
    if (g0 >= io.batch) return;  // (wave-uniform; no workgroup barrier below)
    const bool valid = b < io.batch;
    const OutDelta od = load_out_delta(io);
    vmas_light::DispFlags f{0u};
    if (valid) {
        f = (io.what & VMAS_SCN_REWARD) ? vmas_light::disp_reward(io, (long)b, od.rew) : vmas_light::disp_load_flags(io, (long)b);
        if (io.what & VMAS_SCN_DONE) moved(io.done, od.done)[b] = vmas_light::disp_done(io, f) ? 1 : 0;
    }
    if (!(io.what & VMAS_SCN_OBS)) return;
    const int W = 4 + 3 * io.n_food;
    float* S = light_lds + w * 64 * W;
    const int nv = io.batch - g0 < 64 ? io.batch - g0 : 64;
    for (int k = 0; k < io.n_agents; ++k) {
        if (valid) vmas_light::disp_obs_row(io, (long)b, k, f, S + lane * W);
        __builtin_amdgcn_wave_barrier();
        rows_out(S, nv, W, moved(io.obs[k], od.obs) + (long)g0 * W, lane, 64, nullptr, (float*)nullptr, 0, 0, lane);
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- the MPE family (vmas_mpe_programs.hpp has the row functions) -----------------------------------------
// The k_wheel form: a thread per env computes the task's reward block, then per agent the wave stages its
// 64 observation rows in LDS (4 x 64 x the widest row, sized by the launch) and stores them as one
// contiguous block.  The rows' widths differ per agent (the term table), so the LDS rows are re-laid per
// agent.  A few hundred bytes per env: launch-latency-bound like its two neighbours.
__global__ void __launch_bounds__(256) k_mpe(VmasMpeIO io_arg, int w_max) {
    VMAS_PROGRAM_ARGS(VmasMpeIO, io_arg);
    extern __shared__ float light_lds[];
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const int g0 = wave_uniform(((int)blockIdx.x * 4 + w) * 64), b = g0 + lane;
    if (g0 >= io.batch) return;  // (wave-uniform; no workgroup barrier below)
    const bool valid = b < io.batch;
    const OutDelta od = load_out_delta(io);
    if (valid && (io.what & VMAS_SCN_REWARD)) {
        if (io.task == VMAS_MPE_SPREAD)
            vmas_mpe::spread_reward(io, (long)b, od.rew);
        else
            vmas_mpe::tag_reward(io, (long)b, od.rew);
    }
    if (!(io.what & VMAS_SCN_OBS)) return;
    float* S = light_lds + w * 64 * w_max;
    const int nv = io.batch - g0 < 64 ? io.batch - g0 : 64;
    for (int k = 0; k < io.n_agents; ++k) {
        const int W = 2 * io.n_terms[k];
        if (valid) vmas_mpe::obs_row(io, (long)b, k, S + lane * W);
        __builtin_amdgcn_wave_barrier();
        rows_out(S, nv, W, moved(io.obs[k], od.obs) + (long)g0 * W, lane, 64, nullptr, (float*)nullptr, 0, 0, lane);
        __builtin_amdgcn_wave_barrier();
    }
}

// Test kernel (tests/test_fused.py test_exact_math_gpu): the flag-independent division / square
// root of vmas_programs.hpp next to this translation unit's IEEE `/` and sqrtf.
__global__ void k_test_exact_math(const float* a, const float* b, float* out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = xdiv(a[i], b[i]);
    out[n + i] = a[i] / b[i];
    out[2 * n + i] = xsqrt(a[i]);
    out[3 * n + i] = sqrtf(a[i]);
}

// The fast LIDAR programs' direction instructions (v_sin_f32 / v_cos_f32 through __sinf / __cosf,
// as k_flocking_fast / k_discovery_obs_fast compute a ray's (cos, sin)): out[i] = sin, out[n + i] = cos.
__global__ void k_test_fast_trig(const float* x, float* out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = __sinf(x[i]);
    out[n + i] = __cosf(x[i]);
}

}  // namespace

extern "C" {

int32_t vmas_test_fast_trig(int32_t device, const float* x, float* out, int64_t n, void* stream) {
    if (device < 0 || !x || !out || n <= 0) return vmas_aux::fail(VMAS_E_INVALID, "vmas_test_fast_trig: bad arguments");
    VMAS_AUX_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(k_test_fast_trig, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, (long)n);
    VMAS_AUX_HIP(hipGetLastError());
    return VMAS_OK;
}

int32_t vmas_test_exact_math(int32_t device, const float* a, const float* b, float* out, int64_t n, void* stream) {
    if (device < 0 || !a || !b || !out || n <= 0) return vmas_aux::fail(VMAS_E_INVALID, "vmas_test_exact_math: bad arguments");
    VMAS_AUX_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(k_test_exact_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, out, (long)n);
    VMAS_AUX_HIP(hipGetLastError());
    return VMAS_OK;
}

int32_t vmas_balance_outputs(int32_t device, const VmasBalanceIO* io, void* stream) {
    if (!io || device < 0 || io->batch <= 0 || io->n_agents < 0 || io->n_agents > VMAS_SCN_MAX_AGENTS)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_balance_outputs: bad arguments");
    if (io->package.shape != VMAS_SPHERE || io->goal.shape != VMAS_SPHERE || io->line.shape != VMAS_LINE ||
        io->floor.shape != VMAS_BOX)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_balance_outputs: unexpected entity shapes");
    VMAS_AUX_HIP(hipSetDevice(device));
    const int parts = 1 + ((io->what & VMAS_SCN_OBS) ? (io->n_agents + 3) / 4 : 0);
    hipLaunchKernelGGL(k_balance, dim3((io->batch + 63) / 64, parts), dim3(256), 0, (hipStream_t)stream, *io);
    VMAS_AUX_HIP(hipGetLastError());
    return VMAS_OK;
}

int32_t vmas_flocking_target_action(int32_t device, const float* t, int32_t batch, float period, float* u,
                                    void* stream) {
    if (device < 0 || !t || !u || batch <= 0 || period == 0.f)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_flocking_target_action: bad arguments");
    const float inv = 1.0f / period;
    hipLaunchKernelGGL(k_flocking_target, dim3((batch + 255) / 256), dim3(256), 0, (hipStream_t)stream, t, batch, inv, u);
    VMAS_AUX_HIP(hipGetLastError());
    return VMAS_OK;
}

int32_t vmas_flocking_outputs(int32_t device, const VmasFlockingIO* io, void* stream) {
    if (!io || device < 0 || io->batch <= 0 || io->n_all < 2 || io->n_all > VMAS_FLOCK_MAX_AGENTS || io->n_policy < 1 ||
        io->n_policy > io->n_all || io->target < 0 || io->target >= io->n_all || io->n_rays < 0 ||
        io->n_ray_targets < 0 || io->n_ray_targets > VMAS_SCN_MAX_RAY_TARGETS || io->sum_mode < 1 || io->sum_mode > VMAS_FLOCK_MAX_AGENTS || (io->sum_mode & (io->sum_mode - 1)))
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_flocking_outputs: bad arguments");
    for (int i = 0; i < io->n_all; ++i)
        if (io->agents[i].shape != VMAS_SPHERE) return vmas_aux::fail(VMAS_E_INVALID, "vmas_flocking_outputs: agent %d is not a sphere", i);
    for (int t = 0; t < io->n_ray_targets; ++t)
        if (io->ray_targets[t].shape != VMAS_SPHERE)
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_flocking_outputs: LIDAR target %d is not a sphere", t);
    for (int p = 0; p < io->n_policy; ++p)
        if (io->policy[p] < 0 || io->policy[p] >= io->n_all)
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_flocking_outputs: bad policy index %d", p);
    VMAS_AUX_HIP(hipSetDevice(device));
    static_assert(sizeof(VmasFlockingIO) <= 4096, "kernel argument block");
    const int parts = (io->what & VMAS_SCN_OBS) ? 1 + io->n_rays : 1;
    if (io->fast_lidar && io->n_rays <= kFlockFastRays && io->n_ray_targets <= kFlockFastTargets) {
        const dim3 grid((io->batch + 63) / 64, (io->n_policy + 3) / 4);
        const hipStream_t st = (hipStream_t)stream;
        // flocking's 12 rays with 1..8 targets: the unrolled instantiation (other counts: runtime form)
        const int nt = io->n_rays == 12 ? io->n_ray_targets : 0;
        switch (nt) {
#define VMAS_FLOCK_CASE(k) \
    case k: hipLaunchKernelGGL((k_flocking_fast<12, k>), grid, dim3(256), 0, st, *io); break;
            VMAS_FLOCK_CASE(1) VMAS_FLOCK_CASE(2) VMAS_FLOCK_CASE(3) VMAS_FLOCK_CASE(4)
            VMAS_FLOCK_CASE(5) VMAS_FLOCK_CASE(6) VMAS_FLOCK_CASE(7) VMAS_FLOCK_CASE(8)
#undef VMAS_FLOCK_CASE
            default: hipLaunchKernelGGL((k_flocking_fast<0, 0>), grid, dim3(256), 0, st, *io); break;
        }
    } else
        hipLaunchKernelGGL(k_flocking, dim3((io->batch + 63) / 64, io->n_policy * parts), dim3(64), 0, (hipStream_t)stream,
                           *io);
    VMAS_AUX_HIP(hipGetLastError());
    return VMAS_OK;
}

int32_t vmas_navigation_outputs(int32_t device, const VmasNavigationIO* io, void* stream) {
    if (!io || device < 0 || io->batch <= 0 || io->n_agents < 1 || io->n_agents > VMAS_NAV_MAX_AGENTS || io->n_rays < 0 ||
        ((io->what & VMAS_SCN_REWARD) && !io->ws))
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_navigation_outputs: bad arguments");
    for (int i = 0; i < io->n_agents; ++i) {
        if (io->agents[i].shape != VMAS_SPHERE)
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_navigation_outputs: agent %d is not a sphere", i);
        if (io->pair_static[i] >> i)
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_navigation_outputs: pair flags of agent %d name no earlier agent", i);
    }
    VMAS_AUX_HIP(hipSetDevice(device));
    static_assert(sizeof(VmasNavigationIO) <= 4096, "kernel argument block");
    const hipStream_t st = (hipStream_t)stream;
    const int n = io->n_agents, nr = io->lidar_on ? io->n_rays : 0;
    const int W = 4 + 2 * (io->observe_all_goals ? n : 1) + nr;
    if (io->fast_lidar && nr <= kNavFastRays) {
        const dim3 grid((io->batch + 63) / 64, (n + 3) / 4);
        const size_t lds = (size_t)4 * 64 * W * sizeof(float);
        // 12 rays with 1..7 targets (2..8 agents): the unrolled instantiation (other counts: runtime form)
        switch (nr == 12 ? n - 1 : 0) {
#define VMAS_NAV_CASE(t) \
    case t: hipLaunchKernelGGL((k_navigation_fast<12, t>), grid, dim3(256), lds, st, *io); break;
            VMAS_NAV_CASE(1) VMAS_NAV_CASE(2) VMAS_NAV_CASE(3) VMAS_NAV_CASE(4)
            VMAS_NAV_CASE(5) VMAS_NAV_CASE(6) VMAS_NAV_CASE(7)
#undef VMAS_NAV_CASE
            default: hipLaunchKernelGGL((k_navigation_fast<0, 0>), grid, dim3(256), lds, st, *io); break;
        }
    } else {
        const int parts = (io->what & VMAS_SCN_OBS) ? 1 + nr : 1;
        hipLaunchKernelGGL(k_navigation, dim3((io->batch + 63) / 64, n * parts), dim3(64), 0, st, *io);
    }
    bool pairs = false;  // (no pair passes the static part of World.collides: nothing to settle)
    for (int i = 0; i < n; ++i) pairs = pairs || io->pair_static[i] != 0u;
    if ((io->what & VMAS_SCN_REWARD) && pairs) hipLaunchKernelGGL(k_navigation_pairs, dim3(1), dim3(1024), 0, st, *io);
    VMAS_AUX_HIP(hipGetLastError());
    return VMAS_OK;
}

int32_t vmas_sampling_outputs(int32_t device, const VmasSamplingIO* io, void* stream) {
    if (!io || device >= 64 || io->batch <= 0 || io->n_agents < 1 || io->n_agents > VMAS_SAMPLING_MAX_AGENTS ||
        io->n_rays < 0 || io->n_rays > VMAS_SAMPLING_MAX_RAYS || !(io->what & (VMAS_SCN_REWARD | VMAS_SCN_OBS)) ||
        io->agent_sum_mode < 1 || io->agent_sum_mode > VMAS_SAMPLING_MAX_AGENTS ||
        (io->agent_sum_mode & (io->agent_sum_mode - 1)) || !io->max_pdf || !io->sampled)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_sampling_outputs: bad arguments");
    if (const char* why = samp_density_error(io->grid, io->density))
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_sampling_outputs: bad arguments (%s)", why);
    const int n = io->n_agents, nr = io->lidar_on ? io->n_rays : 0;
    for (int i = 0; i < n; ++i) {
        bool ok = io->pos[i].p != nullptr;
        if (io->what & VMAS_SCN_REWARD) ok = ok && io->sample[i] && io->rewards[i] && io->sampling_rew;
        if (io->what & VMAS_SCN_OBS) ok = ok && io->vel[i].p && io->obs[i] && (nr == 0 || (io->rot[i].p && io->angles[i] && io->lidar[i]));
        if (!ok) return vmas_aux::fail(VMAS_E_INVALID, "vmas_sampling_outputs: null pointer (agent %d)", i);
    }
    const int W = 12 + nr;
    if (device < 0) {
        if (io->out_delta) return vmas_aux::fail(VMAS_E_INVALID, "vmas_sampling_outputs: out_delta on the host");
        for (long b = 0; b < io->batch; ++b)
            for (int k = 0; k < n; ++k) {
                const bool obs = (io->what & VMAS_SCN_OBS) != 0;
                if (!obs && k > 0) break;
                samp_agent<kSampMA>(*io, b, k, obs ? io->obs[k] + b * W : nullptr, (obs && nr > 0) ? io->lidar[k] + b * nr : nullptr, 0);
            }
        return VMAS_OK;
    }
    VMAS_AUX_HIP(hipSetDevice(device));
    static_assert(sizeof(VmasSamplingIO) <= 4096, "kernel argument block");
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((io->batch + 63) / 64, ((io->what & VMAS_SCN_OBS) ? n + 3 : 4) / 4);
    const size_t lds = (size_t)4 * 64 * W * sizeof(float);
    if (n <= 4) hipLaunchKernelGGL((k_sampling<4>), grid, dim3(256), lds, st, *io);
    else if (n <= 8) hipLaunchKernelGGL((k_sampling<8>), grid, dim3(256), lds, st, *io);
    else hipLaunchKernelGGL((k_sampling<16>), grid, dim3(256), lds, st, *io);
    VMAS_AUX_HIP(hipGetLastError());
    return VMAS_OK;
}

int32_t vmas_sampling_max_pdf(int32_t device, const VmasSamplingMaxPdfIO* io, void* stream) {
    if (!io || device >= 64 || io->batch <= 0 || io->n_xs <= 0 || io->n_ys <= 0 || (long)io->n_xs * io->n_ys > (1L << 30) ||
        !io->xs || !io->ys || !io->max_pdf)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_sampling_max_pdf: bad arguments");
    if (const char* why = samp_density_error(io->grid, io->density))
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_sampling_max_pdf: bad arguments (%s)", why);
    if (device < 0) {
        for (long b = 0; b < io->batch; ++b) {
            if (io->mask && !io->mask[b]) continue;
            float m = 0.f;
            for (int ix = 0; ix < io->n_xs; ++ix)
                for (int iy = 0; iy < io->n_ys; ++iy) m = samp_max(m, samp_grid_point(*io, b, io->xs[ix], io->ys[iy]));
            io->max_pdf[b] = m;
        }
        return VMAS_OK;
    }
    VMAS_AUX_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(k_sampling_max_pdf, dim3((io->batch + 3) / 4), dim3(256), 0, (hipStream_t)stream, *io);
    VMAS_AUX_HIP(hipGetLastError());
    return VMAS_OK;
}

int32_t vmas_sampling_reset(int32_t device, const VmasSamplingResetIO* io, uint64_t* increment, void* stream) {
    if (!io || !increment) return vmas_aux::fail(VMAS_E_INVALID, "vmas_sampling_reset: null argument block");
    if (device < 0 || device >= 64)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_sampling_reset: device %d (the draws are a device path only)", device);
    if (io->batch <= 0 || io->n_agents < 1 || io->n_agents > VMAS_SAMPLING_MAX_AGENTS || io->mode < 0 || io->mode > 3 ||
        io->n_xs <= 0 || io->n_ys <= 0 || (long)io->n_xs * io->n_ys > (1L << 30) || !io->xs || !io->ys || !io->mask ||
        !io->max_pdf || !io->sampled)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_sampling_reset: bad arguments (batch %d, %d agents)", io->batch,
                              io->n_agents);
    if (const char* why = samp_density_error(io->grid, io->density))
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_sampling_reset: bad arguments (%s)", why);
    for (int i = 0; i < io->n_agents; ++i)
        if (!io->agents[i].pos.p || !io->sample[i])
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_sampling_reset: null pointer (agent %d)", i);
    static_assert(2 * (VMAS_SAMPLING_MAX_GAUSSIANS + VMAS_SAMPLING_MAX_AGENTS) <= 64, "a lane per draw");
    static_assert(sizeof(VmasSamplingResetIO) + sizeof(vmas_uniform::DrawGrid) <= 4096, "kernel argument block");
    VMAS_AUX_HIP(hipSetDevice(device));
    static int max_blocks[64] = {0};
    if (!max_blocks[device]) {
        hipDeviceProp_t prop;
        VMAS_AUX_HIP(hipGetDeviceProperties(&prop, device));
        max_blocks[device] = prop.multiProcessorCount * (prop.maxThreadsPerMultiProcessor / vmas_uniform::kThreads);
        if (max_blocks[device] <= 0) return vmas_aux::fail(VMAS_E_HIP, "vmas_sampling_reset: device properties");
    }
    // torch's distribution-kernel grid and per-call philox increment on B elements
    int gx_draw = 0;
    unsigned long long inc = 0;
    vmas_uniform::grid_for(io->batch, max_blocks[device], &gx_draw, &inc);
    const vmas_uniform::DrawGrid g{(long long)vmas_uniform::kThreads * gx_draw, inc};
    hipLaunchKernelGGL(k_sampling_reset, dim3((io->batch + 3) / 4), dim3(256), 0, (hipStream_t)stream, *io, g);
    VMAS_AUX_HIP(hipGetLastError());
    *increment = inc * 2ull * (unsigned long long)(io->density.n_gaussians + io->n_agents);
    return VMAS_OK;
}

int32_t vmas_wheel_outputs(int32_t device, const VmasWheelIO* io, void* stream) {
    static_assert(sizeof(VmasWheelIO) <= 4096, "kernel argument block");
    if (!io || device >= 64 || io->batch <= 0 || io->n_agents < 1 || io->n_agents > VMAS_WHEEL_MAX_AGENTS ||
        !(io->what & (VMAS_SCN_REWARD | VMAS_SCN_OBS)) || !io->line_ang_vel.p)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_wheel_outputs: bad arguments");
    const bool rew = (io->what & VMAS_SCN_REWARD) != 0, obs = (io->what & VMAS_SCN_OBS) != 0;
    if ((rew && !io->rew) || (obs && (!io->line_pos.p || !io->line_rot.p)))
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_wheel_outputs: null pointer");
    const int n = io->n_agents;
    for (int i = 0; i < n; ++i)
        if ((rew && !io->rewards[i]) || (obs && (!io->pos[i].p || !io->vel[i].p || !io->obs[i])))
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_wheel_outputs: null pointer (agent %d)", i);
    constexpr int W = 13;
    if (device < 0) {
        if (io->out_delta) return vmas_aux::fail(VMAS_E_INVALID, "vmas_wheel_outputs: out_delta on the host");
        for (long b = 0; b < io->batch; ++b) {
            if (rew) {
                const float r = vmas_light::wheel_rew(*io, b);
                io->rew[b] = r;
                for (int k = 0; k < n; ++k) io->rewards[k][b] = -r;
            }
            if (obs)
                for (int k = 0; k < n; ++k) vmas_light::wheel_obs_row(*io, b, k, io->obs[k] + b * W);
        }
        return VMAS_OK;
    }
    VMAS_AUX_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(k_wheel, dim3((io->batch + 255) / 256), dim3(256), (size_t)4 * 64 * W * sizeof(float),
                       (hipStream_t)stream, *io);
    VMAS_AUX_HIP(hipGetLastError());
    return VMAS_OK;
}

int32_t vmas_dispersion_outputs(int32_t device, const VmasDispersionIO* io, void* stream) {
    static_assert(sizeof(VmasDispersionIO) <= 4096, "kernel argument block");
    static_assert(VMAS_DISP_MAX_AGENTS <= 32 && VMAS_DISP_MAX_FOOD <= 32, "a bit per agent / per food");
    if (!io || device >= 64 || io->batch <= 0 || io->n_agents < 1 || io->n_agents > VMAS_DISP_MAX_AGENTS ||
        io->n_food < 1 || io->n_food > VMAS_DISP_MAX_FOOD ||
        !(io->what & (VMAS_SCN_REWARD | VMAS_SCN_OBS | VMAS_SCN_DONE)))
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_dispersion_outputs: bad arguments");
    const bool rew = (io->what & VMAS_SCN_REWARD) != 0, obs = (io->what & VMAS_SCN_OBS) != 0;
    const bool done = (io->what & VMAS_SCN_DONE) != 0;
    const int n = io->n_agents, nf = io->n_food;
    if (done && !io->done) return vmas_aux::fail(VMAS_E_INVALID, "vmas_dispersion_outputs: null pointer (done)");
    for (int l = 0; l < nf; ++l)
        if (!io->eaten[l] || ((rew || obs) && !io->food_pos[l].p) ||
            (rew && (!io->just_eaten[l] || !io->how_many[l] || !io->anyone[l])))
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_dispersion_outputs: null pointer (food %d)", l);
    for (int i = 0; i < n; ++i)
        if (((rew || obs) && !io->pos[i].p) || (rew && !io->rewards[i]) || (obs && (!io->vel[i].p || !io->obs[i])))
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_dispersion_outputs: null pointer (agent %d)", i);
    const int W = 4 + 3 * nf;
    if (device < 0) {
        if (io->out_delta) return vmas_aux::fail(VMAS_E_INVALID, "vmas_dispersion_outputs: out_delta on the host");
        for (long b = 0; b < io->batch; ++b) {
            const vmas_light::DispFlags f = rew ? vmas_light::disp_reward(*io, b, 0) : vmas_light::disp_load_flags(*io, b);
            if (done) io->done[b] = vmas_light::disp_done(*io, f) ? 1 : 0;
            if (obs)
                for (int k = 0; k < n; ++k) vmas_light::disp_obs_row(*io, b, k, f, io->obs[k] + b * W);
        }
        return VMAS_OK;
    }
    VMAS_AUX_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(k_dispersion, dim3((io->batch + 255) / 256), dim3(256), (size_t)4 * 64 * W * sizeof(float),
                       (hipStream_t)stream, *io);
    VMAS_AUX_HIP(hipGetLastError());
    return VMAS_OK;
}

int32_t vmas_mpe_outputs(int32_t device, const VmasMpeIO* io, void* stream) {
    static_assert(sizeof(VmasMpeIO) + sizeof(int) <= 4096, "kernel argument block");
    static_assert(VMAS_MPE_MAX_AGENTS <= 8, "a bit per agent; the registers of team_sum's tree");
    if (!io || device >= 64 || io->batch <= 0 || io->n_agents < 1 || io->n_agents > VMAS_MPE_MAX_AGENTS ||
        io->n_landmarks < 0 || io->n_landmarks > VMAS_MPE_MAX_LANDMARKS || !(io->what & (VMAS_SCN_REWARD | VMAS_SCN_OBS)) ||
        (io->what & ~(VMAS_SCN_REWARD | VMAS_SCN_OBS)))
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_mpe_outputs: bad arguments");
    if (io->task != VMAS_MPE_SPREAD && io->task != VMAS_MPE_TAG)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_mpe_outputs: unknown task %d", io->task);
    const bool rew = (io->what & VMAS_SCN_REWARD) != 0, obs = (io->what & VMAS_SCN_OBS) != 0;
    const int n = io->n_agents, nl = io->n_landmarks;
    const uint32_t all = (1u << n) - 1u;
    if (rew && io->task == VMAS_MPE_SPREAD && !io->rew) return vmas_aux::fail(VMAS_E_INVALID, "vmas_mpe_outputs: null pointer (rew)");
    if (rew && io->task == VMAS_MPE_TAG) {
        if (!io->agents_rew || !io->adverary_rew)
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_mpe_outputs: null pointer (team sums)");
        if (!(io->adversary_mask & all) || !(~io->adversary_mask & all))
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_mpe_outputs: a team is empty");
        for (int m : {io->sum_mode_good, io->sum_mode_adv})
            if (m < 1 || m > VMAS_MPE_MAX_AGENTS || (m & (m - 1)))
                return vmas_aux::fail(VMAS_E_INVALID, "vmas_mpe_outputs: sum mode %d", m);
    }
    for (int l = 0; l < nl; ++l)
        if (!io->landmark_pos[l].p) return vmas_aux::fail(VMAS_E_INVALID, "vmas_mpe_outputs: null pointer (landmark %d)", l);
    int w_max = 0;
    for (int i = 0; i < n; ++i) {
        if (!io->pos[i].p || (rew && (!io->rewards[i] || (io->task == VMAS_MPE_TAG && !io->agent_rew[i]))) ||
            (obs && (!io->vel[i].p || !io->obs[i])))
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_mpe_outputs: null pointer (agent %d)", i);
        if (!obs) continue;
        const int nt = io->n_terms[i];
        if (nt < 1 || nt > VMAS_MPE_MAX_TERMS) return vmas_aux::fail(VMAS_E_INVALID, "vmas_mpe_outputs: term count (agent %d)", i);
        for (int t = 0; t < nt; ++t) {
            const VmasMpeTerm q = io->terms[i][t];
            const bool ok = q.kind == VMAS_MPE_SELF_VEL || q.kind == VMAS_MPE_SELF_POS ||
                            (q.kind == VMAS_MPE_REL_LANDMARK && q.index < nl) ||
                            ((q.kind == VMAS_MPE_REL_AGENT || q.kind == VMAS_MPE_AGENT_VEL) && q.index < n);
            if (!ok) return vmas_aux::fail(VMAS_E_INVALID, "vmas_mpe_outputs: term %d of agent %d", t, i);
        }
        w_max = 2 * nt > w_max ? 2 * nt : w_max;
    }
    if (device < 0) {
        if (io->out_delta) return vmas_aux::fail(VMAS_E_INVALID, "vmas_mpe_outputs: out_delta on the host");
        for (long b = 0; b < io->batch; ++b) {
            if (rew) {
                if (io->task == VMAS_MPE_SPREAD)
                    vmas_mpe::spread_reward(*io, b, 0);
                else
                    vmas_mpe::tag_reward(*io, b, 0);
            }
            if (obs)
                for (int k = 0; k < n; ++k) vmas_mpe::obs_row(*io, b, k, io->obs[k] + b * 2 * io->n_terms[k]);
        }
        return VMAS_OK;
    }
    VMAS_AUX_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(k_mpe, dim3((io->batch + 255) / 256), dim3(256), (size_t)4 * 64 * w_max * sizeof(float),
                       (hipStream_t)stream, *io, w_max);
    VMAS_AUX_HIP(hipGetLastError());
    return VMAS_OK;
}

int32_t vmas_transport_outputs(int32_t device, const VmasTransportIO* io, void* stream) {
    if (!io || device < 0 || io->batch <= 0 || io->n_agents < 0 || io->n_agents > VMAS_TRANSPORT_MAX_AGENTS ||
        io->n_packages < 0 || io->n_packages > VMAS_TRANSPORT_MAX_PACKAGES)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_transport_outputs: bad arguments");
    for (int i = 0; i < io->n_packages; ++i)
        if (io->package[i].shape != VMAS_BOX || io->goal[i].shape != VMAS_SPHERE)
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_transport_outputs: package %d is not (box, sphere goal)", i);
    VMAS_AUX_HIP(hipSetDevice(device));
    static_assert(sizeof(VmasTransportIO) <= 4096, "kernel argument block");
    const int parts = 1 + ((io->what & VMAS_SCN_OBS) ? io->n_agents : 0);
    hipLaunchKernelGGL(k_transport, dim3((io->batch + 63) / 64, parts), dim3(64), 0, (hipStream_t)stream, *io);
    VMAS_AUX_HIP(hipGetLastError());
    return VMAS_OK;
}

int32_t vmas_discovery_outputs(int32_t device, const VmasDiscoveryIO* io, void* stream) {
    if (!io || device < 0 || io->batch <= 0 || io->n_agents < 1 || io->n_agents > VMAS_DISC_MAX_AGENTS ||
        io->n_targets < 0 || io->n_targets > VMAS_DISC_MAX_TARGETS || io->n_entities < 1 ||
        io->n_entities > VMAS_DISC_MAX_ENTITIES || io->n_lidars < 0 || io->n_lidars > VMAS_DISC_MAX_LIDARS ||
        (io->done && !io->all_time))
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_discovery_outputs: bad arguments");
    for (int i = 0; i < io->n_agents; ++i)
        if (io->agent_entity[i] < 0 || io->agent_entity[i] >= io->n_entities)
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_discovery_outputs: bad agent index %d", i);
    for (int j = 0; j < io->n_targets; ++j)
        if (io->target_entity[j] < 0 || io->target_entity[j] >= io->n_entities)
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_discovery_outputs: bad target index %d", j);
    int rays = 0;
    for (int s = 0; s < io->n_lidars; ++s) {
        if (io->n_rays[s] < 0) return vmas_aux::fail(VMAS_E_INVALID, "vmas_discovery_outputs: bad ray count");
        rays += io->n_rays[s];
    }
    VMAS_AUX_HIP(hipSetDevice(device));
    static_assert(sizeof(VmasDiscoveryIO) <= 4096, "kernel argument block");
    const unsigned gx = (unsigned)((io->batch + 63) / 64);
    if (io->what & VMAS_SCN_REWARD) {
        if (io->n_agents <= kDiscFastAgents && io->n_targets <= kDiscFastTargets && io->n_targets >= 1)
            hipLaunchKernelGGL(k_discovery_reward_fast, dim3(gx), dim3(64 * io->n_agents), 0, (hipStream_t)stream, *io);
        else
            hipLaunchKernelGGL(k_discovery_reward, dim3(gx), dim3(64), 0, (hipStream_t)stream, *io);
    }
    if (io->what & VMAS_SCN_OBS) {
        bool fast = io->fast_lidar && io->n_entities <= kDiscFastEntities;
        for (int s = 0; s < io->n_lidars; ++s) fast = fast && io->n_rays[s] <= kDiscFastRays;
        // a wave per (64 envs, agent, LIDAR) with two LIDARs (other LIDAR counts: a wave per agent)
        if (fast && io->n_lidars == 2)
            hipLaunchKernelGGL(k_discovery_obs_split<2>, dim3(gx, (io->n_agents + 1) / 2), dim3(256), 0,
                               (hipStream_t)stream, *io);
        else if (fast)
            hipLaunchKernelGGL(k_discovery_obs_fast, dim3(gx, (io->n_agents + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                               *io);
        else
            hipLaunchKernelGGL(k_discovery_obs, dim3(gx, io->n_agents * (1 + rays)), dim3(64), 0, (hipStream_t)stream,
                               *io);
    }
    VMAS_AUX_HIP(hipGetLastError());
    return VMAS_OK;
}

}  // extern "C"
