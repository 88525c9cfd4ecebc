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
//
// k_reset_place / k_reset_commit (vmas_spawn_reset): the reset of a scenario that places its entities
// by rejection sampling (utils.py:239-319 spawn_entities_randomly / find_random_pos_for_entity), see
// the second half of this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "vmas_aux.hpp"
#include "vmas_mi355x.h"
#include "vmas_programs.hpp"
#include "vmas_uniform.hpp"

using namespace vmas;

namespace {

constexpr int kResetThreads = 64;  // (one wave: the masked rows are few, more workgroups spread them)
static_assert(sizeof(VmasBalanceResetIO) + sizeof(vmas_uniform::DrawGrid) <= 4096, "kernel argument block");

// (put1 / put2 / reset_place: vmas_programs.hpp, shared with vmas_scenarios.hip k_sampling_reset)

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
        reset_place(ag, b, mk(line.x + io.agent_dx[i], line.y + io.agent_dy));  // line_pos + offset
        const VmasMutVec f = io.force[i], t = io.torque[i];
        put2(f, b, 0.f, 0.f);
        put1(t, b, 0.f);
    }
    {
        const VmasResetEntity e = io.goal;
        reset_place(e, b, goal);
    }
    {
        const VmasResetEntity e = io.package;
        reset_place(e, b, pkg);
    }
    {
        const VmasResetEntity e = io.line;
        reset_place(e, b, line);
    }
    {
        const VmasResetEntity e = io.floor;
        reset_place(e, b, pf);
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

// ---- the spawn reset (vmas_spawn_reset) ------------------------------------------------------------
// The reference's placement loop (vmas_spawn.hip's head states it): per entity, every env keeps its
// FIRST candidate that overlaps nothing, and the loop consumes 1 try if every env accepts candidate 0,
// else (the largest accepted index over the batch) + 2.  The next entity's tries start where these end,
// so its candidates depend on a maximum over ALL envs: the hand-off between two entities is batch-wide.
// Here it is the kernel boundary -- one k_reset_place launch per entity, queued back to back by one
// call, no wait between workgroups inside a kernel and nothing that can spin.  Launch i reads the
// maxima of entities 0 .. i-1 (complete: their kernels have ended), draws its own tries with
// uniform_at (the numbers the torch uniform_ calls of the full reset produce), tests them against the
// fixed positions and the accepted candidates of the entities before it, and publishes its own
// maximum with one agent-scope atomicMax per wave.  The placement kernels write scratch and the words
// only; k_reset_commit then writes the world, for the envs of the mask, and only when every env of
// the batch found a place (else the caller redoes the reset another way: nothing was written).
struct PlaceArgs {
    int32_t batch, index, n_fixed, max_tries, mode, pad0;
    float d2_min, x_lo, x_hi, y_lo, y_hi, pad1;
    unsigned long long seed, offset;
    float* scratch;  // [slot][2][B]: slot i's x row, then its y row (a wave reads consecutive floats)
    int32_t* words;  // [0, n_place) the maxima, [VMAS_RESET_MAX_PLACE] unresolved envs
    VmasVec fixed[VMAS_RESET_MAX_FIXED];
};
static_assert(sizeof(PlaceArgs) + sizeof(vmas_uniform::DrawGrid) <= 4096, "kernel argument block");
static_assert(sizeof(VmasSpawnResetIO) <= 4096, "kernel argument block");
static_assert(VMAS_RESET_MAX_PLACE < VMAS_RESET_WORDS, "the unresolved word");
static_assert(VMAS_RESET_MAX_SEP == VMAS_FLOCK_MAX_AGENTS, "the step program's accumulators");

// torch.cdist(...) < min_dist as d2 < d2_min (vmas_spawn.hip near; vmas_aux.hpp spawn_d2_min)
__device__ __forceinline__ bool too_near(float ox, float oy, float x, float y, float d2_min) {
    const float d0 = ox - x, d1 = oy - y;
    return d0 * d0 + d1 * d1 < d2_min;
}

__global__ void __launch_bounds__(kResetThreads) k_reset_place(PlaceArgs a_arg, vmas_uniform::DrawGrid g) {
    VMAS_PROGRAM_ARGS(PlaceArgs, a_arg);
    const int B = io.batch, i = io.index;
    int32_t* W = io.words;
    // an earlier entity left an env without a place: the call is void, skip the work.  (Envs of THIS
    // launch add to the word too; a workgroup that sees them skips work that is void all the same.)
    if (__hip_atomic_load(W + VMAS_RESET_MAX_PLACE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
    const int b = blockIdx.x * kResetThreads + threadIdx.x;
    unsigned long long first = 0;  // P_i: the tries the entities before this one consumed
    for (int j = 0; j < i; ++j) {
        const int m = W[j];
        first += (unsigned long long)(m == 0 ? 1 : m + 2);
    }
    int accepted = 0, lost = 0;
    if (b < B) {
        float* S = io.scratch;
        const int lim = io.max_tries, nf = io.n_fixed, mode = io.mode;
        const float d2 = io.d2_min, x_lo = io.x_lo, x_hi = io.x_hi, y_lo = io.y_lo, y_hi = io.y_hi;
        const unsigned long long seed = io.seed, per_try = 2ull * g.inc;
        float x = 0.f, y = 0.f;
        int k = 0;
        for (;; ++k) {
            if (k >= lim) {
                lost = 1;
                break;
            }
            const unsigned long long off = io.offset + (first + (unsigned long long)k) * per_try;
            x = vmas_uniform::uniform_at(seed, off, g, b, x_lo, x_hi, mode);
            y = vmas_uniform::uniform_at(seed, off + g.inc, g, b, y_lo, y_hi, mode);
            bool hit = false;
            for (int j = 0; j < nf; ++j) {
                const VmasVec v = io.fixed[j];
                const float* p = v.p + (long)b * v.s0;
                hit = hit || too_near(p[0], p[v.s1], x, y, d2);
            }
            for (int j = 0; j < i; ++j)
                hit = hit || too_near(S[(size_t)(2 * j) * B + b], S[(size_t)(2 * j + 1) * B + b], x, y, d2);
            if (!hit) break;
        }
        if (!lost) {
            S[(size_t)(2 * i) * B + b] = x;
            S[(size_t)(2 * i + 1) * B + b] = y;
            accepted = k;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        accepted = max(accepted, __shfl_xor(accepted, off));
        lost += __shfl_xor(lost, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (accepted > 0) atomicMax(W + i, accepted);
        if (lost) atomicAdd(W + VMAS_RESET_MAX_PLACE, lost);
    }
}

__global__ void __launch_bounds__(kResetThreads) k_reset_commit(VmasSpawnResetIO io_arg) {
    VMAS_PROGRAM_ARGS(VmasSpawnResetIO, io_arg);
    const int b = blockIdx.x * kResetThreads + threadIdx.x;
    const int B = io.batch;
    if (b >= B || io.mask[b] == 0) return;
    if (io.words[VMAS_RESET_MAX_PLACE] != 0) return;  // (nothing has been written: the placement wrote scratch only)
    const float* S = io.scratch;
    auto slot = [&](int s) { return mk(S[(size_t)(2 * s) * B + b], S[(size_t)(2 * s + 1) * B + b]); };
    // a position code: a placed slot, or -1 - j for the fixed position j (validated by the host)
    auto at = [&](int s) {
        if (s >= 0) return slot(s);
        const VmasVec v = io.fixed[-1 - s];
        return ld_vec2(v, b);
    };
    for (int w = 0; w < io.n_write; ++w) {
        const VmasResetEntity e = io.write[w];
        reset_place(e, b, at(io.write_slot[w]));
    }
    for (int a = 0; a < io.n_agents; ++a) {
        const VmasMutVec f = io.force[a], t = io.torque[a];
        put2(f, b, 0.f, 0.f);
        put1(t, b, 0.f);
    }
    if (io.steps) io.steps[b] = 0.f;
    for (int d = 0; d < io.n_derived; ++d) {
        const VmasResetDerived r = io.derived[d];
        if (r.kind == VMAS_RESET_D_NORM) {
            // vector_norm(pos_a - pos_b, dim=1) * factor, as the fused programs compute it
            put1(r.out, b, xnorm(slot(r.a) - slot(r.b)) * r.factor);
        } else if (r.kind == VMAS_RESET_D_BOX_SPHERE) {
            // xoverlap_box_sphere (core.py:1932-1963) on the new positions; every rot is 0 after the reset
            const V2 pb = slot(r.a), ps = slot(r.b);
            const V2 cp = xclosest_point_box(pb, xtrig(0.f), r.length * 0.5f, r.width * 0.5f, ps);
            const float dsc = xnorm(ps - cp), dsb = xnorm(ps - pb), dcb = xnorm(pb - cp);
            r.out8[b] = ((dsb < dcb) || (dsc < r.radius_lmd)) ? 1 : 0;
        } else if (r.kind == VMAS_RESET_D_CLEAR8) {
            for (int k = 0; k < r.n; ++k) r.out8[(size_t)b * r.n + k] = 0;
        } else if (r.kind == VMAS_RESET_D_MEAN_SQ_SEP) {
            // flocking's distance_shaping from the new positions: the step program's own function
            put1(r.out, b,
                 flock_mean_sq_sep<VMAS_RESET_MAX_SEP>(
                     io.n_sep, r.a, at(io.sep_slot[r.a]), [&](int j) { return at(io.sep_slot[j]); }, io.sep_desired,
                     r.factor, io.sep_sum_mode));
        } else if (r.kind == VMAS_RESET_D_ZERO32) {
            put1(r.out, b, 0.f);
        }
    }
}

// ---- the uniform reset (vmas_uniform_reset) --------------------------------------------------------
// A reset that is a fixed list of uniform_ calls and rejects nothing (wheel.py:49-78,
// dispersion.py:51-88 `reset_world_at(None)`): one thread per env, as k_balance_reset.  Record i is call
// i of the full reset, so the generator offset of a call is a running sum over the records before it:
// a [B, 2] call advances by g2.inc (torch's grid on 2 B elements), a [B, 1] call by g1.inc.
struct UniformGrids {
    vmas_uniform::DrawGrid g2, g1;
};
static_assert(sizeof(VmasUniformResetIO) + sizeof(UniformGrids) <= 4096, "kernel argument block");

__global__ void __launch_bounds__(kResetThreads) k_uniform_reset(VmasUniformResetIO io_arg, UniformGrids g) {
    VMAS_PROGRAM_ARGS(VmasUniformResetIO, io_arg);
    const int b = blockIdx.x * kResetThreads + threadIdx.x;
    if (b >= io.batch || io.mask[b] == 0) return;
    unsigned long long off = io.offset;
    for (int i = 0; i < io.n_draws; ++i) {
        const VmasResetEntity e = io.draws[i].entity;
        const float lo = io.draws[i].lo, hi = io.draws[i].hi;
        if (io.draws[i].target == VMAS_UDRAW_POS) {
            const float x = vmas_uniform::uniform_at(io.seed, off, g.g2, 2 * b, lo, hi, io.mode);
            const float y = vmas_uniform::uniform_at(io.seed, off, g.g2, 2 * b + 1, lo, hi, io.mode);
            reset_place(e, b, mk(x, y));
            off += g.g2.inc;
        } else {
            const float r = vmas_uniform::uniform_at(io.seed, off, g.g1, b, lo, hi, io.mode);
            reset_place(e, b, mk(0.f, 0.f));
            put1(e.rot, b, r);
            off += g.g1.inc;
        }
    }
    for (int i = 0; i < io.n_fixed; ++i) {
        const VmasResetEntity e = io.fixed[i].entity;
        reset_place(e, b, mk(io.fixed[i].x, io.fixed[i].y));
    }
    for (int a = 0; a < io.n_agents; ++a) {
        const VmasMutVec f = io.force[a], t = io.torque[a];
        put2(f, b, 0.f, 0.f);
        put1(t, b, 0.f);
    }
    for (int k = 0; k < io.n_clear; ++k) io.clear[k][b] = 0;
    for (int k = 0; k < io.n_set; ++k) io.set[k][b] = 1;
    if (io.steps) io.steps[b] = 0.f;
}

std::mutex g_reset_mu;
int32_t* g_reset_host_words[64] = {nullptr};  // pinned: the words of the last call, per device

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

extern "C" int32_t vmas_spawn_reset(int32_t device, const VmasSpawnResetIO* io, uint64_t* increment, int32_t* unresolved,
                                    void* stream) {
    if (!io || !increment || !unresolved || device < 0 || device >= 64)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_spawn_reset: bad arguments");
    if (io->batch <= 0 || io->n_place < 1 || io->n_place > VMAS_RESET_MAX_PLACE || io->n_fixed < 0 ||
        io->n_fixed > VMAS_RESET_MAX_FIXED || io->n_write < 0 || io->n_write > VMAS_RESET_MAX_WRITE || io->n_agents < 0 ||
        io->n_agents > VMAS_RESET_MAX_AGENTS || io->n_derived < 0 || io->n_derived > VMAS_RESET_MAX_DERIVED || !io->mask ||
        !io->scratch || !io->words || io->mode < 0 || io->mode > 3)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_spawn_reset: bad arguments (batch %d, %d placed, %d written)",
                              io->batch, io->n_place, io->n_write);
    for (int j = 0; j < io->n_fixed; ++j)
        if (!io->fixed[j].p) return vmas_aux::fail(VMAS_E_INVALID, "vmas_spawn_reset: null fixed position %d", j);
    // a position code: a placed slot, or -1 - j for fixed[j]
    auto code_ok = [&](int32_t c) { return c >= 0 ? c < io->n_place : -1 - (long)c < (long)io->n_fixed; };
    for (int w = 0; w < io->n_write; ++w)
        if (!code_ok(io->write_slot[w]))
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_spawn_reset: entity %d reads slot %d of %d (%d fixed)", w,
                                  io->write_slot[w], io->n_place, io->n_fixed);
    if (io->n_sep < 0 || io->n_sep > VMAS_RESET_MAX_SEP)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_spawn_reset: a separation list of %d", io->n_sep);
    for (int j = 0; j < io->n_sep; ++j)
        if (!code_ok(io->sep_slot[j]))
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_spawn_reset: separation entry %d reads slot %d of %d (%d fixed)", j,
                                  io->sep_slot[j], io->n_place, io->n_fixed);
    const bool sep_ok = io->n_sep >= 2 && io->sep_sum_mode >= 1 && io->sep_sum_mode <= VMAS_RESET_MAX_SEP &&
                        !(io->sep_sum_mode & (io->sep_sum_mode - 1));
    for (int d = 0; d < io->n_derived; ++d) {
        const VmasResetDerived& r = io->derived[d];
        const bool slots = r.a >= 0 && r.a < io->n_place && r.b >= 0 && r.b < io->n_place;
        const bool ok = r.kind == VMAS_RESET_D_NORM         ? slots && r.out.p
                        : r.kind == VMAS_RESET_D_BOX_SPHERE ? slots && r.out8
                        : r.kind == VMAS_RESET_D_CLEAR8     ? r.out8 && r.n >= 0
                        : r.kind == VMAS_RESET_D_MEAN_SQ_SEP ? sep_ok && r.a >= 0 && r.a < io->n_sep && r.out.p
                        : r.kind == VMAS_RESET_D_ZERO32     ? r.out.p != nullptr
                                                            : false;
        if (!ok) return vmas_aux::fail(VMAS_E_INVALID, "vmas_spawn_reset: derived value %d (kind %d)", d, r.kind);
    }
    std::lock_guard<std::mutex> lk(g_reset_mu);
    VMAS_AUX_HIP(hipSetDevice(device));
    static int max_blocks[64] = {0};
    if (!max_blocks[device]) {
        hipDeviceProp_t prop;
        VMAS_AUX_HIP(hipGetDeviceProperties(&prop, device));
        max_blocks[device] = prop.multiProcessorCount * (prop.maxThreadsPerMultiProcessor / vmas_uniform::kThreads);
        if (max_blocks[device] <= 0) return vmas_aux::fail(VMAS_E_HIP, "vmas_spawn_reset: device properties");
    }
    if (!g_reset_host_words[device])
        VMAS_AUX_HIP(hipHostMalloc((void**)&g_reset_host_words[device], VMAS_RESET_WORDS * sizeof(int32_t),
                                   hipHostMallocDefault));
    int32_t* h = g_reset_host_words[device];
    // torch's distribution-kernel grid and per-call philox increment on B elements
    int gx_draw = 0;
    unsigned long long inc = 0;
    vmas_uniform::grid_for(io->batch, max_blocks[device], &gx_draw, &inc);
    const vmas_uniform::DrawGrid g{(long long)vmas_uniform::kThreads * gx_draw, inc};
    hipStream_t st = (hipStream_t)stream;
    const int gx = (io->batch + kResetThreads - 1) / kResetThreads;
    // (the words are zeroed by a kernel, not a memset: vmas_spawn.hip k_spawn_clear has the note)
    VMAS_AUX_HIP(vmas_aux::fill_u32_async(io->words, 0u, VMAS_RESET_WORDS, st));
    PlaceArgs a{};
    a.batch = io->batch;
    a.n_fixed = io->n_fixed;
    a.max_tries = io->max_tries > 0 ? std::min(io->max_tries, VMAS_RESET_TRIES_LIMIT) : VMAS_RESET_TRIES_LIMIT;
    a.mode = io->mode;
    a.x_lo = io->x_lo, a.x_hi = io->x_hi, a.y_lo = io->y_lo, a.y_hi = io->y_hi;
    a.seed = io->seed, a.offset = io->offset;
    a.scratch = io->scratch, a.words = io->words;
    for (int j = 0; j < io->n_fixed; ++j) a.fixed[j] = io->fixed[j];
    for (int i = 0; i < io->n_place; ++i) {
        a.index = i;
        a.d2_min = vmas_aux::spawn_d2_min(io->min_dist[i]);
        hipLaunchKernelGGL(k_reset_place, dim3(gx), dim3(kResetThreads), 0, st, a, g);
    }
    hipLaunchKernelGGL(k_reset_commit, dim3(gx), dim3(kResetThreads), 0, st, *io);
    VMAS_AUX_HIP(hipGetLastError());
    VMAS_AUX_HIP(hipMemcpyAsync(h, io->words, VMAS_RESET_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    vmas_aux::note_host_wait();
    VMAS_AUX_HIP(hipStreamSynchronize(st));  // the call's only wait
    unsigned long long tries = 0;
    for (int i = 0; i < io->n_place; ++i) tries += (unsigned long long)(h[i] == 0 ? 1 : h[i] + 2);
    *increment = tries * 2ull * inc;
    *unresolved = h[VMAS_RESET_MAX_PLACE];
    return VMAS_OK;
}

extern "C" int32_t vmas_uniform_reset(int32_t device, const VmasUniformResetIO* io, uint64_t* increment, void* stream) {
    if (!io || !increment) return vmas_aux::fail(VMAS_E_INVALID, "vmas_uniform_reset: null argument block");
    if (device < 0 || device >= 64)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_uniform_reset: device %d (the draws are a device path only)", device);
    // (element 2 b + 1 of a [B, 2] call is an int)
    if (io->batch <= 0 || io->batch > (1 << 30) - 1 || io->mode < 0 || io->mode > 3 || io->n_draws < 0 ||
        io->n_draws > VMAS_URESET_MAX_DRAWS || io->n_fixed < 0 || io->n_fixed > VMAS_URESET_MAX_FIXED || io->n_agents < 0 ||
        io->n_agents > VMAS_URESET_MAX_AGENTS || io->n_clear < 0 || io->n_clear > VMAS_URESET_MAX_CLEAR || io->n_set < 0 ||
        io->n_set > VMAS_URESET_MAX_SET || !io->mask)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_uniform_reset: bad arguments (batch %d, %d draws, %d fixed)", io->batch,
                              io->n_draws, io->n_fixed);
    int n2 = 0, n1 = 0;
    for (int i = 0; i < io->n_draws; ++i) {
        const VmasUniformDraw& d = io->draws[i];
        if (d.call != i || (d.target != VMAS_UDRAW_POS && d.target != VMAS_UDRAW_ROT))
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_uniform_reset: draw record %d (call %d, target %d)", i, d.call,
                                  d.target);
        if (d.target == VMAS_UDRAW_POS ? !d.entity.pos.p : !d.entity.rot.p)
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_uniform_reset: null destination (draw record %d)", i);
        (d.target == VMAS_UDRAW_POS ? n2 : n1) += 1;
    }
    for (int i = 0; i < io->n_fixed; ++i)
        if (!io->fixed[i].entity.pos.p)
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_uniform_reset: null destination (fixed record %d)", i);
    for (int k = 0; k < io->n_clear; ++k)
        if (!io->clear[k]) return vmas_aux::fail(VMAS_E_INVALID, "vmas_uniform_reset: null row to clear (%d)", k);
    for (int k = 0; k < io->n_set; ++k)
        if (!io->set[k]) return vmas_aux::fail(VMAS_E_INVALID, "vmas_uniform_reset: null row to set (%d)", k);
    VMAS_AUX_HIP(hipSetDevice(device));
    static int max_blocks[64] = {0};
    if (!max_blocks[device]) {
        hipDeviceProp_t prop;
        VMAS_AUX_HIP(hipGetDeviceProperties(&prop, device));
        max_blocks[device] = prop.multiProcessorCount * (prop.maxThreadsPerMultiProcessor / vmas_uniform::kThreads);
        if (max_blocks[device] <= 0) return vmas_aux::fail(VMAS_E_HIP, "vmas_uniform_reset: device properties");
    }
    // torch's distribution-kernel grid and per-call philox increment: on 2 B elements and on B elements
    int gx2 = 0, gx1 = 0;
    unsigned long long inc2 = 0, inc1 = 0;
    vmas_uniform::grid_for(2ll * io->batch, max_blocks[device], &gx2, &inc2);
    vmas_uniform::grid_for(io->batch, max_blocks[device], &gx1, &inc1);
    const UniformGrids g{{(long long)vmas_uniform::kThreads * gx2, inc2}, {(long long)vmas_uniform::kThreads * gx1, inc1}};
    const int gx = (io->batch + kResetThreads - 1) / kResetThreads;
    hipLaunchKernelGGL(k_uniform_reset, dim3(gx), dim3(kResetThreads), 0, (hipStream_t)stream, *io, g);
    VMAS_AUX_HIP(hipGetLastError());
    *increment = inc2 * (unsigned long long)n2 + inc1 * (unsigned long long)n1;
    return VMAS_OK;
}
