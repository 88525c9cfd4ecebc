// vmas_light_programs.hpp -- the per-env row functions of the wheel and dispersion step programs
// (wheel.py:80-110, dispersion.py:90-160 of the reference; restated in scenarios/wheel.py and
// scenarios/dispersion.py), as host + device templates: the gfx950 kernels k_wheel / k_dispersion
// (vmas_scenarios.hip) and the host backend (device == -1) run the same statements.  IO is the
// argument block by reference (on the device: read in place from the kernel argument segment).
//
// Every operation is fp32 and rounded on its own (-ffp-contract=off: no FMA), in the reference's
// order; `/` and sqrtf are the correctly rounded ones of the library's translation units; cosf / sinf
// are the library calls (the device library's on the GPU -- what torch's device cos / sin call --
// and libm's on the host).
#pragma once

#include <math.h>
#include <stdint.h>

#include "vmas_mi355x.h"

#define VMAS_LIGHT_HD __host__ __device__ __forceinline__

namespace vmas_light {

// torch.remainder(a, b) for floats: fmod, moved into the sign of the divisor
VMAS_LIGHT_HD float remainder(float a, float b) {
    float mod = fmodf(a, b);
    if ((mod != 0.f) && ((b < 0.f) != (mod < 0.f))) mod = mod + b;
    return mod;
}

// ---- wheel ---------------------------------------------------------------------------------------------
// | |line.ang_vel| - desired_velocity |
template <class IO>
VMAS_LIGHT_HD float wheel_rew(IO& io, long b) {
    return fabsf(fabsf(io.line_ang_vel.p[b * io.line_ang_vel.s0]) - io.desired_velocity);
}

// agent k's 13 observation columns of env b, to o[0 .. 13)
template <class IO>
VMAS_LIGHT_HD void wheel_obs_row(IO& io, long b, int k, float* o) {
    const float* pp = io.pos[k].p + b * io.pos[k].s0;
    const float* vp = io.vel[k].p + b * io.vel[k].s0;
    const float* lp = io.line_pos.p + b * io.line_pos.s0;
    const float px = pp[0], py = pp[io.pos[k].s1];
    const float rot = io.line_rot.p[b * io.line_rot.s0];
    const float av = fabsf(io.line_ang_vel.p[b * io.line_ang_vel.s0]);
    const float ex = io.half_length * cosf(rot), ey = io.half_length * sinf(rot);  // line_end_1
    o[0] = px;
    o[1] = py;
    o[2] = vp[0];
    o[3] = vp[io.vel[k].s1];
    o[4] = lp[0] - px;
    o[5] = lp[io.line_pos.s1] - py;
    o[6] = ex - px;
    o[7] = ey - py;
    o[8] = -ex - px;  // line_end_2 = -line_end_1
    o[9] = -ey - py;
    o[10] = remainder(rot, io.pi);
    o[11] = av;
    o[12] = fabsf(av - io.desired_velocity);
}

// ---- dispersion ----------------------------------------------------------------------------------------
// What one env's step leaves in registers: per food a bit of `eaten` (after the reward block, when it
// ran) -- what the observations and done read.
struct DispFlags {
    uint32_t eaten;
};

template <class IO>
VMAS_LIGHT_HD bool disp_on(IO& io, long b, int a, int l) {
    const float* pa = io.pos[a].p + b * io.pos[a].s0;
    const float* pl = io.food_pos[l].p + b * io.food_pos[l].s0;
    const float dx = pa[0] - pl[0], dy = pa[io.pos[a].s1] - pl[io.food_pos[l].s1];
    return sqrtf(dx * dx + dy * dy) < io.thr[a * VMAS_DISP_MAX_FOOD + l];
}

template <class IO>
VMAS_LIGHT_HD DispFlags disp_load_flags(IO& io, long b) {
    DispFlags f{0u};
    for (int l = 0; l < io.n_food; ++l)
        if (io.eaten[l][b]) f.eaten |= 1u << l;
    return f;
}

// The reward calls of every agent of env b, in agent order: counts, flags, rewards.  rew_delta: the
// direct-output offset of the reward rows (0: in place).  Returns the updated flags.
template <class IO>
VMAS_LIGHT_HD DispFlags disp_reward(IO& io, long b, long long rew_delta) {
    const int na = io.n_agents, nf = io.n_food;
    // bit a of on[l]: agent a stands on food l (the food loops are unrolled over the cap so that the
    // array's indices are static: registers, not scratch)
    uint32_t on[VMAS_DISP_MAX_FOOD];
    uint32_t eaten = 0u, just = 0u;
#pragma unroll
    for (int l = 0; l < VMAS_DISP_MAX_FOOD; ++l) {
        on[l] = 0u;
        if (l >= nf) continue;
        uint32_t m = 0u;
        int count = 0;
        for (int a = 0; a < na; ++a)
            if (disp_on(io, b, a, l)) {
                m |= 1u << a;
                ++count;
            }
        on[l] = m;
        if (io.eaten[l][b]) eaten |= 1u << l;
        if (io.just_eaten[l][b] || count > 0) just |= 1u << l;  // just_eaten[anyone_on_food] = True
        io.how_many[l][b] = (int64_t)count;
        io.anyone[l][b] = count > 0 ? 1 : 0;
    }
    for (int a = 0; a < na; ++a) {
        float r = 0.f;
#pragma unroll
        for (int l = 0; l < VMAS_DISP_MAX_FOOD; ++l) {
            if (l >= nf) continue;
            const bool fresh = !((eaten >> l) & 1u);
            if (io.share_reward) {
                if (((just >> l) & 1u) && fresh) r = r + 1.f;
            } else if (((on[l] >> a) & 1u) && fresh) {
                r = r + 1.f / (float)__builtin_popcount(on[l]);  // how_many.reciprocal(): on[l] != 0 here
            }
        }
        if (io.penalise_by_time && r == 0.f) r = -0.01f;
        float* out = reinterpret_cast<float*>(reinterpret_cast<char*>(io.rewards[a]) + rew_delta);
        out[b] = r;
    }
    // after the last agent's reward: eaten += just_eaten, just_eaten = False, is_rendering[eaten] = False
    eaten |= just;
    for (int l = 0; l < nf; ++l) {
        const bool e = (eaten >> l) & 1u;
        io.eaten[l][b] = e ? 1 : 0;
        io.just_eaten[l][b] = 0;
        if (e && io.is_rendering[l]) io.is_rendering[l][b] = 0;
    }
    return DispFlags{eaten};
}

// agent k's 4 + 3 n_food observation columns of env b, to o
template <class IO>
VMAS_LIGHT_HD void disp_obs_row(IO& io, long b, int k, const DispFlags& f, float* o) {
    const float* pp = io.pos[k].p + b * io.pos[k].s0;
    const float* vp = io.vel[k].p + b * io.vel[k].s0;
    const float px = pp[0], py = pp[io.pos[k].s1];
    o[0] = px;
    o[1] = py;
    o[2] = vp[0];
    o[3] = vp[io.vel[k].s1];
    for (int l = 0; l < io.n_food; ++l) {
        const float* pl = io.food_pos[l].p + b * io.food_pos[l].s0;
        o[4 + 3 * l] = pl[0] - px;
        o[5 + 3 * l] = pl[io.food_pos[l].s1] - py;
        o[6 + 3 * l] = ((f.eaten >> l) & 1u) ? 1.f : 0.f;
    }
}

template <class IO>
VMAS_LIGHT_HD bool disp_done(IO& io, const DispFlags& f) {
    return f.eaten == (io.n_food >= 32 ? 0xffffffffu : (1u << io.n_food) - 1u);
}

}  // namespace vmas_light
