// vmas_lidar.hpp -- the fast LIDAR of the fused scenario programs (vmas_scenarios.hip): the two ray
// methods, the caster of K rays against up to TM spheres, the driver of one LIDAR's rays into an
// observation row staged in LDS, and the copy of a wave's rows out of LDS.  Device code; the exact
// LIDAR (one ray per thread, ray_sphere, bit-identical to k_cast_rays) stays with its kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "vmas_physics.hpp"

namespace vmas {

// The index of the agent (env, ...) a whole wave works for, made wave-uniform for the compiler:
// indexing the arrays of an argument block read in place (VMAS_PROGRAM_ARGS: scalar loads from the
// kernel argument segment) with a per-lane index copies the whole block, 3.5 KiB, to every lane's
// scratch.
__device__ __forceinline__ int wave_uniform(int i) { return __builtin_amdgcn_readfirstlane(i); }

// ---- the two ray methods -------------------------------------------------------------------------------
// A method is dir(angle) -> (sin, cos), the per-target constant c(r^2, u) (u: the sphere's centre
// relative to the ray's origin) and hit(u, c, cos, sin) -> the distance, NaN on a miss (dropped by
// min_drop_nan).  Which scenario uses which:
//   RayHardware  flocking, discovery.  The cheapest pair: 6 VALU + one square root per (ray, sphere).
//   RayPrecise   navigation, sampling.  RayHardware was measured first there and missed the LIDAR
//                parity condition (below); ~20 VALU more per ray.

// __sinf / __cosf (v_sin_f32 / v_cos_f32) take the angle in revolutions: x * (1 / 2 pi) rounds to
// |x| * 2^-24 rad, i.e. 1e-6 rad at 16 rad (the LIDAR certification's turn, tests/_parity.py) and
// 1.5e-5 rad at 256.  Below this bound the fast LIDAR programs use their own direction code; above
// it ocml's range-reduced sincosf.  (Ray angles are the sensor's [0, 2 pi) plus the agent's rotation.)
constexpr float kFastTrigMaxAngle = 16.f;

// Hardware sin / cos and the ray-sphere distance in its direct form (ray_sphere_fast_nan, c = r^2 -
// |u|^2).
struct RayHardware {
    static __device__ __forceinline__ void dir(float a, float& ds, float& dc) {
        if (fabsf(a) < kFastTrigMaxAngle) {
            ds = __sinf(a);
            dc = __cosf(a);
        } else {
            sincosf(a, &ds, &dc);
        }
    }
    static __device__ __forceinline__ float c(float r2, V2 u) { return r2 - (u.x * u.x + u.y * u.y); }
    static __device__ __forceinline__ float hit(float ux, float uy, float c, float dc, float ds) {
        return ray_sphere_fast_nan(ux, uy, c, dc, ds);
    }
};

// Why navigation (and sampling, the same geometry) cannot use RayHardware: at navigation's geometry
// (centres up to 0.45 from the origin, radius 0.1, positions of magnitude 1) the direct form's r^2 -
// dn^2 = t^2 + (r^2 - |u|^2) cancels to ~5e-8 in `a`, and the hardware instructions turn the ray by
// up to ~3e-7 rad (another ~3e-8 in `a`); a grazing hit (a ~ 1e-7) then lands 6.7e-5 from the
// oracle, beyond what a certification turn reproduces (2 of 16 384 rows at 4 096 envs).  So: dn as
// the cross product u x dir (no cancellation: ~6e-9 in `a`; c = r^2), and the direction from a
// Cody-Waite reduction by pi / 2 with the Cephes sinf / cosf polynomials (angle error <= 1e-7 rad
// against double precision over +-16 rad, ~20 VALU a ray), ocml's sincosf beyond kFastTrigMaxAngle.
struct RayPrecise {
    static __device__ __forceinline__ void dir(float x, float& s, float& c) {
        if (!(fabsf(x) < kFastTrigMaxAngle)) {
            sincosf(x, &s, &c);
            return;
        }
        const float k = rintf(x * 0.636619772f);  // 2 / pi
        float r = __builtin_fmaf(-k, 1.5703125f, x);  // pi / 2 in three parts; the first product is exact
        r = __builtin_fmaf(-k, 4.837512969970703125e-4f, r);
        r = __builtin_fmaf(-k, 7.54978995489188216e-8f, r);
        const float z = r * r;
        float ps = __builtin_fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f);
        ps = __builtin_fmaf(ps, z, -1.6666654611e-1f);
        const float sr = __builtin_fmaf(r * z, ps, r);
        float pc = __builtin_fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f);
        pc = __builtin_fmaf(pc, z, 4.166664568298827e-2f);
        const float cr = __builtin_fmaf(z * z, pc, __builtin_fmaf(-0.5f, z, 1.0f));
        const int q = (int)k & 3;
        const float a = (q & 1) ? cr : sr, b = (q & 1) ? sr : cr;
        s = (q & 2) ? -a : a;
        c = ((q + 1) & 2) ? -b : b;
    }
    static __device__ __forceinline__ float c(float r2, V2) { return r2; }
    static __device__ __forceinline__ float hit(float ux, float uy, float r2, float dc, float ds) {
        const float t = __builtin_fmaf(ux, dc, uy * ds);      // the foot point's distance along the ray
        const float dn = __builtin_fmaf(ux, ds, -(uy * dc));  // the centre's distance from the ray's line
        const float a = __builtin_fmaf(-dn, dn, r2);
        return t - __builtin_amdgcn_sqrtf(__builtin_fminf(a, t * 1e30f));
    }
};

// ---- the caster ------------------------------------------------------------------------------------------
// A ray of method M: its direction, and the least hit distance so far (max_range without a hit).
template <class M>
struct Ray {
    float ds, dc, best;
    __device__ __forceinline__ Ray(float angle, float max_range) : best(max_range) { M::dir(angle, ds, dc); }
};
// The rays (one origin; their directions are computed first, by their constructors) against the
// spheres t < TM.  target(t, ux, uy, c): whether sphere t is live, and then its centre relative to
// the origin and the method's constant.  The rays' minima are updated side by side, so their
// dependent chains interleave.  The target loop is fully unrolled over the static bound with a
// guarded body and never `break`s: the callers' register arrays are only ever indexed by constants
// (a partly unrolled or early-left loop indexes them at run time, which puts them in scratch), and
// the guard is a wave-uniform branch or, where every target is live, none.  Every caller performs
// the same operations per ray in the same order, however many rays it casts at a time and whatever
// the form of its ray loop: the forms agree bit for bit.
template <class M, int TM, class Target, class... R>
__device__ __forceinline__ void cast_rays(const Target& target, R&... ray) {
#pragma unroll
    for (int t = 0; t < TM; ++t) {
        float ux, uy, c;
        if (!target(t, ux, uy, c)) continue;
        ((ray.best = min_drop_nan(ray.best, M::hit(ux, uy, c, ray.dc, ray.ds))), ...);
    }
}

// ---- one LIDAR's rays into the lane's row -------------------------------------------------------------
// slot: the LIDAR's columns of the lane's observation row in LDS; angle(r): ray r's angle (sensor +
// rotation; r < RM is a constant at every call); U: the spheres' centres relative to the origin, C:
// the method's constants, live(t): whether sphere t counts.  Leaves slot[r] = ray r's measurement,
// r < nr.
//   UNROLLED  nr == RM rays and the targets fixed at compile time: every ray unrolled with its angle
//             in a register, so all the rays' chains interleave; no per-target branch.
//   otherwise nr <= RM rays in a rolled loop (`unroll 1`), in trips of K = 1 or 2.  The angles,
//             loaded together up front, wait in the rays' own LDS slots: a register array indexed
//             at run time goes to scratch.  K = 2 where the kernel runs at 4 waves per SIMD or
//             fewer: one ray's chain (direction, then TM x (fma, fma, sqrt, min)) at a time left
//             the SIMDs waiting, two interleave.  (The fully unrolled rays x entities body is no
//             option at discovery's bounds: 16 x 16 was ~35 KiB of straight-line code, each wave
//             streaming it through the instruction cache once.)
template <class M, bool UNROLLED, int RM, int K, int TM, class Angle, class Live>
__device__ __forceinline__ void lidar_row(float* slot, int nr, const Angle& angle, const V2 (&U)[TM],
                                          const float (&C)[TM], float max_range, const Live& live) {
    static_assert(K == 1 || K == 2, "trips of one ray or two");
    auto target = [&](int t, float& ux, float& uy, float& c) {
        ux = U[t].x;
        uy = U[t].y;
        c = C[t];
        return live(t);
    };
    if constexpr (UNROLLED) {
#pragma unroll
        for (int r = 0; r < RM; ++r) {
            Ray<M> q(angle(r), max_range);
            cast_rays<M, TM>(target, q);
            slot[r] = q.best;
        }
    } else {
#pragma unroll
        for (int r = 0; r < RM; ++r)
            if (r < nr) slot[r] = angle(r);
        auto one = [&](int r) {
            Ray<M> q(slot[r], max_range);
            cast_rays<M, TM>(target, q);
            slot[r] = q.best;
        };
        if constexpr (K == 2) {
            int r = 0;
#pragma unroll 1
            for (; r + 1 < nr; r += 2) {
                Ray<M> q0(slot[r], max_range), q1(slot[r + 1], max_range);
                cast_rays<M, TM>(target, q0, q1);
                slot[r] = q0.best;
                slot[r + 1] = q1.best;
            }
            if (r < nr) one(r);  // (the odd ray)
        } else {
#pragma unroll 1
            for (int r = 0; r < nr; ++r) one(r);
        }
    }
}

// ---- a wave's rows out of LDS -----------------------------------------------------------------------------
// rows (S below): nv rows of W floats in LDS, a row per env (a lane per env writing its own row to
// memory stores 4-byte values 4 * W bytes apart: twice the output bytes reached HBM).  Written as
// contiguous blocks: obs
// [nv x W], by the lanes first, first + step, ... (one wave: lane, 64; L waves sharing the rows:
// lane + 64 s, 64 L), then lid [nv x nr] = the rows' columns [col, col + nr) by the wave's 64 lanes.
// xf: nullptr for the values as they are, or xf(column, value); that loop stays rolled (a division
// per element: unrolled, its body cost navigation 17 registers).  obs = nullptr, or nr == 0, skips
// that part.
template <class Obs, class XF>
__device__ __forceinline__ void rows_out(const float* rows, int nv, int W, Obs obs, int first, int step, const XF& xf,
                                         float* lid, int col, int nr, int lane) {
    // (the rows as an LDS pointer: through the parameter's generic one the copy loops are unrolled
    // before the compiler has found out that they read LDS, with the thresholds of flat memory)
    const auto* S = (const __attribute__((address_space(3))) float*)rows;
    if constexpr (std::is_null_pointer_v<XF> && !std::is_null_pointer_v<Obs>) {
        for (int i = first; i < nv * W; i += step) obs[i] = S[i];
    } else if constexpr (!std::is_null_pointer_v<Obs>) {
#pragma unroll 1
        for (int i = first; i < nv * W; i += step) obs[i] = xf(i - (i / W) * W, S[i]);
    }
    for (int i = lane; i < nv * nr; i += 64) {
        const int e = i / nr;
        lid[i] = S[e * W + col + (i - e * nr)];
    }
}

}  // namespace vmas
