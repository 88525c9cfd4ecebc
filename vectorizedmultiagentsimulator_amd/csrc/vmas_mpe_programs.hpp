// vmas_mpe_programs.hpp -- the per-env row functions of the MPE family's step program (simple_spread.py
// and simple_tag.py of the reference's scenarios/mpe; restated in scenarios/mpe/), as host + device
// templates: the gfx950 kernel k_mpe (vmas_scenarios.hip) and the host backend (device == -1) run the
// same statements.  IO is the argument block by reference (on the device: read in place from the
// kernel argument segment).
//
// Every operation is fp32 and rounded on its own (-ffp-contract=off: no FMA), in the reference's
// order; sqrtf is the correctly rounded one of the library's translation units.  Per-agent values that
// outlive a loop live in arrays indexed by the constants of loops unrolled over the caps (registers,
// not scratch); positions are re-read from memory (the cache's, after the first touch) so that the
// agent and landmark loops themselves stay rolled.
//
// A task is one reward function here plus its block of parameters in VmasMpeIO; the observation rows
// are table-driven (VmasMpeTerm) and shared by every task.
#pragma once

#include <math.h>
#include <stdint.h>

#include "vmas_mi355x.h"

#define VMAS_MPE_HD __host__ __device__ __forceinline__

namespace vmas_mpe {

constexpr int MA = VMAS_MPE_MAX_AGENTS, ML = VMAS_MPE_MAX_LANDMARKS;

struct P2 {
    float x, y;
};

template <class V>
VMAS_MPE_HD P2 ld2(const V& v, long b) {
    const float* p = v.p + b * v.s0;
    return P2{p[0], p[v.s1]};
}

// torch.linalg.vector_norm(p - q, dim=-1) of a length-2 vector
VMAS_MPE_HD float dist(P2 p, P2 q) {
    const float dx = p.x - q.x, dy = p.y - q.y;
    return sqrtf(dx * dx + dy * dy);
}

// torch.min over a stacked dim, element by element in order: the smaller value, a NaN once met
VMAS_MPE_HD float min_in_order(float m, float d) { return (d < m || d != d) ? d : m; }

template <class T>
VMAS_MPE_HD T* moved(T* p, long long delta) {
    return reinterpret_cast<T*>(reinterpret_cast<char*>(p) + delta);
}

// ---- simple_spread ---------------------------------------------------------------------------------------
// The first agent's reward call of env b: Scenario.rew and every agent's returned reward (the same value).
template <class IO>
VMAS_MPE_HD void spread_reward(IO& io, long b, long long rew_delta) {
    const int na = io.n_agents, nl = io.n_landmarks;
    float closest[ML];
#pragma unroll
    for (int l = 0; l < ML; ++l) {
        closest[l] = 0.f;
        if (l >= nl) continue;
        const P2 pl = ld2(io.landmark_pos[l], b);
        float m = dist(ld2(io.pos[0], b), pl);
        for (int a = 1; a < na; ++a) m = min_in_order(m, dist(ld2(io.pos[a], b), pl));
        closest[l] = m;
    }
    float r = 0.f;
    for (int i = 0; i < na; ++i) {
#pragma unroll
        for (int l = 0; l < ML; ++l)
            if (l < nl) r = r - closest[l];  // (once per agent: one rounding each, not a product)
        if (!((io.collide_mask >> i) & 1u)) continue;
        const P2 pi = ld2(io.pos[i], b);
        const float ri = io.radius[i];
        for (int a = 0; a < na; ++a) {
            if (a == i) continue;
            // World.is_overlapping(a, i) of two spheres: get_distance < 0
            if ((dist(ld2(io.pos[a], b), pi) - io.radius[a]) - ri < 0.f) r = r - 1.f;
        }
    }
    io.rew[b] = r;
    for (int i = 0; i < na; ++i) moved(io.rewards[i], rew_delta)[b] = r;
}

// ---- simple_tag ------------------------------------------------------------------------------------------
// stack([r_k for the team's members k in order], -1).sum(-1) in torch's order: `acc` strided accumulators
// (member k of the team goes to accumulator k % acc, each starting from the reduction's +0), combined by an
// adjacent-pair tree.  Static register indices only.
VMAS_MPE_HD float team_sum(const float (&r)[MA], uint32_t members, int acc) {
    float y[MA];
#pragma unroll
    for (int i = 0; i < MA; ++i) y[i] = 0.f;
    int n = 0;
    const int accm = acc - 1;
#pragma unroll
    for (int j = 0; j < MA; ++j) {
        if (!((members >> j) & 1u)) continue;
        const int slot = n & accm;
#pragma unroll
        for (int i = 0; i < MA; ++i)
            if (i == slot) y[i] = y[i] + r[j];
        ++n;
    }
    const int m = n < acc ? n : acc;
#pragma unroll
    for (int w = 1; w < MA; w *= 2)
#pragma unroll
        for (int i = 0; i + w < MA; i += 2 * w)
            if (i + w < m) y[i] = y[i] + y[i + w];
    return y[0];
}

// The first agent's reward call of env b: every Agent.rew, the two team sums, every returned reward.
template <class IO>
VMAS_MPE_HD void tag_reward(IO& io, long b, long long rew_delta) {
    const int na = io.n_agents;
    const uint32_t all = (1u << na) - 1u, adv = io.adversary_mask & all, good = ~io.adversary_mask & all;
    float r[MA];
#pragma unroll
    for (int i = 0; i < MA; ++i) {
        r[i] = 0.f;
        if (i >= na) continue;
        const P2 pi = ld2(io.pos[i], b);
        const bool collide = (io.collide_mask >> i) & 1u;
        float v = 0.f;
        if ((adv >> i) & 1u) {  // adversary_reward
            if (io.shape_adversary_rew) {
                float m = 0.f;
                bool first = true;
                for (int g = 0; g < na; ++g) {
                    if (!((good >> g) & 1u)) continue;
                    const float d = dist(ld2(io.pos[g], b), pi);
                    m = first ? d : min_in_order(m, d);
                    first = false;
                }
                v = v - 0.1f * m;
            }
            if (collide)
                for (int g = 0; g < na; ++g)
                    if (((good >> g) & 1u) && dist(ld2(io.pos[g], b), pi) < io.thr[g * MA + i]) v = v + 10.f;
        } else {  // agent_reward
            if (io.shape_agent_rew)
                for (int a = 0; a < na; ++a)
                    if ((adv >> a) & 1u) v = v + 0.1f * dist(pi, ld2(io.pos[a], b));
            if (collide)
                for (int a = 0; a < na; ++a)
                    if (((adv >> a) & 1u) && dist(ld2(io.pos[a], b), pi) < io.thr[a * MA + i]) v = v - 10.f;
        }
        r[i] = v;
        io.agent_rew[i][b] = v;
    }
    const float good_sum = team_sum(r, good, io.sum_mode_good), adv_sum = team_sum(r, adv, io.sum_mode_adv);
    io.agents_rew[b] = good_sum;
    io.adverary_rew[b] = adv_sum;
#pragma unroll
    for (int i = 0; i < MA; ++i) {
        if (i >= na) continue;
        const bool is_adv = (adv >> i) & 1u;
        const bool share = is_adv ? io.adversaries_share_rew != 0 : io.agents_share_rew != 0;
        moved(io.rewards[i], rew_delta)[b] = share ? (is_adv ? adv_sum : good_sum) : r[i];
    }
}

// ---- the observation rows (every task) ------------------------------------------------------------------
// agent k's 2 * n_terms[k] observation columns of env b, to o
template <class IO>
VMAS_MPE_HD void obs_row(IO& io, long b, int k, float* o) {
    const P2 pk = ld2(io.pos[k], b);
    const int nt = io.n_terms[k];
    for (int t = 0; t < nt; ++t) {
        const int kind = io.terms[k][t].kind, j = io.terms[k][t].index;
        P2 v;
        if (kind == VMAS_MPE_SELF_VEL) {
            v = ld2(io.vel[k], b);
        } else if (kind == VMAS_MPE_SELF_POS) {
            v = pk;
        } else if (kind == VMAS_MPE_REL_LANDMARK) {
            const P2 q = ld2(io.landmark_pos[j], b);
            v = P2{q.x - pk.x, q.y - pk.y};
        } else if (kind == VMAS_MPE_REL_AGENT) {
            const P2 q = ld2(io.pos[j], b);
            v = P2{q.x - pk.x, q.y - pk.y};
        } else {  // VMAS_MPE_AGENT_VEL
            v = ld2(io.vel[j], b);
        }
        o[2 * t] = v.x;
        o[2 * t + 1] = v.y;
    }
}

}  // namespace vmas_mpe
