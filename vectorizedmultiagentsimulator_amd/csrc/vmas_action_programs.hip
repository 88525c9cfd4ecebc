// vmas_action_programs.hip -- the stage between the action mapping and the physics step: the
// kinematic dynamics models (reference vmas/simulator/dynamics/diff_drive.py:33-88,
// kinematic_bicycle.py:57-112, drone.py:110-160) and the PID velocity controller
// (controllers/velocity_controller.py:78-134), each the reference's fp32 tensor program evaluated
// per env row by one thread: gfx950 kernel + host backend (device == -1) + C ABI.
//
// The reference runs an RK4 DiffDrive agent as ~60 small torch kernels, a Drone as several times
// that; here one launch covers up to 8 agents (refs in the kernel arguments, blockIdx.y = ref,
// one thread per (env, ref)), and the PID is one launch per call (one thread per element).
//
// Arithmetic: every operation is the torch program's fp32 operation in its order, rounded on its
// own (-ffp-contract=off, and the pragma below).  Python numbers reach the kernel as the fp32
// values torch makes of them (dt ** 2, dt / 6, I_yy - I_zz, l_f + l_r, 1 / T_i: evaluated in
// double by the caller, rounded once).  A division of a tensor by a Python number is a mode:
// div_mode 0 divides by the fp32 divisor, 1 multiplies by the fp32 reciprocal the caller passes
// beside it (inv_*: what a torch build does on its device, and how it rounds the reciprocal --
// 1.0f / f32(d) or f32(1.0 / d) --, is probed by the caller).  Trig is sinf / cosf / tanf /
// atan2f(x, 1.0f) (ocml on the device: the functions torch's own kernels call).
//
// Registers: states are fixed-size structs and every loop over their components is unrolled with
// constant indices, so the 12-state RK4 (five states of 12 floats live at the widest point) stays
// in VGPRs: no scratch ("Action programs").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "vmas_aux.hpp"
#include "vmas_mi355x.h"

namespace {

constexpr int kMaxRefsPerLaunch = 8;  // refs travel in the kernel arguments (8 x 256 bytes)
constexpr int kThreads = 256;

#define VMAS_HD __host__ __device__ __forceinline__

template <int N>
struct Vec {
    float v[N];
};

// tensor / python_number as the torch build evaluates it (see the file notes)
VMAS_HD float div_by(float x, float d, float inv_d, int mode) { return mode ? x * inv_d : x / d; }

// torch.clamp(x, -m, m): NaN stays NaN
VMAS_HD float clamp_sym(float x, float m) { return x != x ? x : fminf(fmaxf(x, -m), m); }

// x' = v cos(theta), y' = v sin(theta), theta' = omega (diff_drive.py:33-46)
struct DiffDriveModel {
    static constexpr int N = 3;
    float v, w;
    VMAS_HD Vec<3> f(const Vec<3>& s) const {
#pragma clang fp contract(off)
        Vec<3> o;
        o.v[0] = v * cosf(s.v[2]);
        o.v[1] = v * sinf(s.v[2]);
        o.v[2] = w;
        return o;
    }
};

// beta = atan2(tan(delta) l_r / (l_f + l_r), 1); x' = v cos(theta + beta), y' = v sin(theta + beta),
// theta' = v / (l_f + l_r) cos(beta) tan(delta) (kinematic_bicycle.py:57-70)
struct BicycleModel {
    static constexpr int N = 3;
    float steer, v, l_r, wb, inv_wb;
    int mode;
    VMAS_HD Vec<3> f(const Vec<3>& s) const {
#pragma clang fp contract(off)
        const float t = tanf(steer);
        const float beta = atan2f(div_by(t * l_r, wb, inv_wb, mode), 1.0f);
        const float a = s.v[2] + beta;
        Vec<3> o;
        o.v[0] = v * cosf(a);
        o.v[1] = v * sinf(a);
        o.v[2] = (div_by(v, wb, inv_wb, mode) * cosf(beta)) * tanf(steer);
        return o;
    }
};

// the 12-state quadrotor (drone.py:110-121); columns PHI THETA PSI P Q R VX VY VZ X Y Z
struct DroneModel {
    static constexpr int N = 12;
    float thrust, t0, t1, t2;
    float m, inv_m, g, i_yz, i_zx, i_xy, i_xx, i_yy, i_zz, inv_i_xx, inv_i_yy, inv_i_zz;
    int mode;
    VMAS_HD Vec<12> f(const Vec<12>& s) const {
#pragma clang fp contract(off)
        const float c_phi = cosf(s.v[0]), s_phi = sinf(s.v[0]);
        const float c_th = cosf(s.v[1]), s_th = sinf(s.v[1]);
        const float c_psi = cosf(s.v[2]), s_psi = sinf(s.v[2]);
        const float p = s.v[3], q = s.v[4], r = s.v[5];
        Vec<12> o;
        o.v[0] = p;
        o.v[1] = q;
        o.v[2] = r;
        o.v[3] = div_by(t0 - (i_yz * q) * r, i_xx, inv_i_xx, mode);
        o.v[4] = div_by(t1 - (i_zx * p) * r, i_yy, inv_i_yy, mode);
        o.v[5] = div_by(t2 - (i_xy * p) * q, i_zz, inv_i_zz, mode);
        o.v[6] = div_by(((c_phi * s_th) * c_psi + s_phi * s_psi) * thrust, m, inv_m, mode);
        o.v[7] = div_by(((c_phi * s_th) * s_psi - s_phi * c_psi) * thrust, m, inv_m, mode);
        o.v[8] = div_by((c_phi * c_th) * thrust, m, inv_m, mode) - g;
        o.v[9] = s.v[6];
        o.v[10] = s.v[7];
        o.v[11] = s.v[8];
        return o;
    }
};

// state + dt * k / 2 (halve) or state + dt * k, per component (_integrators.increment)
template <int N>
VMAS_HD Vec<N> stage(const Vec<N>& s, const Vec<N>& k, float dt, bool halve) {
#pragma clang fp contract(off)
    Vec<N> o;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float d = dt * k.v[i];
        o.v[i] = s.v[i] + (halve ? d * 0.5f : d);  // (/ 2 and * 0.5f are the same fp32 value)
    }
    return o;
}

// dt * f (Euler) or (dt / 6) * (k1 + 2 k2 + 2 k3 + k4) (RK4), the reference's order of additions
template <typename M>
VMAS_HD Vec<M::N> increment(const M& m, const Vec<M::N>& s, float dt, float dt_6, int rk4) {
#pragma clang fp contract(off)
    constexpr int N = M::N;
    Vec<N> o;
    const Vec<N> k1 = m.f(s);
    if (!rk4) {
#pragma unroll
        for (int i = 0; i < N; ++i) o.v[i] = dt * k1.v[i];
        return o;
    }
    const Vec<N> k2 = m.f(stage(s, k1, dt, true));
    const Vec<N> k3 = m.f(stage(s, k2, dt, true));
    const Vec<N> k4 = m.f(stage(s, k3, dt, false));
#pragma unroll
    for (int i = 0; i < N; ++i) o.v[i] = dt_6 * (((k1.v[i] + 2.0f * k2.v[i]) + 2.0f * k3.v[i]) + k4.v[i]);
    return o;
}

// One env row of one agent: the model's one-step displacement, then the force / torque that make
// the drag-free integrator follow it (_integrators.apply_displacement): a = (delta - v dt) / dt^2,
// F = m a, tau = I alpha.
VMAS_HD void program_row(const VmasActionProgramRef& r, long b) {
#pragma clang fp contract(off)
    const float vx = r.vel[b * r.vel_s0], vy = r.vel[b * r.vel_s0 + r.vel_s1], aw = r.ang_vel[b * r.ang_s0];
    const float px = r.pos[b * r.pos_s0], py = r.pos[b * r.pos_s0 + r.pos_s1], th = r.rot[b * r.rot_s0];
    float* u = r.u + b * r.u_s0;
    const int rk4 = r.integration == VMAS_INTEGRATION_RK4;
    float dx, dy, dth;
    if (r.kind == VMAS_DYNAMICS_DIFF_DRIVE) {
        const DiffDriveModel m{u[0], u[r.u_s1]};
        const Vec<3> d = increment(m, Vec<3>{{px, py, th}}, r.dt, r.dt_6, rk4);
        dx = d.v[0], dy = d.v[1], dth = d.v[2];
    } else if (r.kind == VMAS_DYNAMICS_BICYCLE) {
        const BicycleModel m{clamp_sym(u[r.u_s1], r.max_steering_angle), u[0], r.l_r, r.wheelbase, r.inv_wheelbase,
                             r.div_mode};
        const Vec<3> d = increment(m, Vec<3>{{px, py, th}}, r.dt, r.dt_6, rk4);
        dx = d.v[0], dy = d.v[1], dth = d.v[2];
    } else {
        const float thrust = u[0] + r.mass_g;  // (in place on the action, as the reference)
        u[0] = thrust;
        float* din = r.drone_in + b * 12;
        Vec<12> s;
#pragma unroll
        for (int i = 0; i < 12; ++i) s.v[i] = din[i];
        s.v[2] = th, s.v[9] = px, s.v[10] = py;
        din[2] = th, din[9] = px, din[10] = py;  // (written into the current drone_state, as the reference)
        const DroneModel m{thrust,  u[r.u_s1], u[2 * r.u_s1], u[3 * r.u_s1], r.mass, r.inv_mass, r.g,        r.i_yz,
                           r.i_zx,  r.i_xy,    r.i_xx,        r.i_yy,        r.i_zz, r.inv_i_xx, r.inv_i_yy, r.inv_i_zz,
                           r.div_mode};
        const Vec<12> d = increment(m, s, r.dt, r.dt_6, rk4);
        float* dout = r.drone_out + b * 12;
#pragma unroll
        for (int i = 0; i < 12; ++i) dout[i] = s.v[i] + d.v[i];
        dx = d.v[6], dy = d.v[7], dth = d.v[5];
    }
    const float ax = div_by(dx - vx * r.dt, r.dt2, r.inv_dt2, r.div_mode);
    const float ay = div_by(dy - vy * r.dt, r.dt2, r.inv_dt2, r.div_mode);
    const float al = div_by(dth - aw * r.dt, r.dt2, r.inv_dt2, r.div_mode);
    r.force[b * r.force_s0] = r.mass * ax;
    r.force[b * r.force_s0 + r.force_s1] = r.mass * ay;
    r.torque[b] = r.moment_of_inertia * al;
}

struct ProgramArgs {
    VmasActionProgramRef r[kMaxRefsPerLaunch];
    int B;
};

__global__ void __launch_bounds__(kThreads) k_action_programs(ProgramArgs a) {
    const long b = (long)blockIdx.x * kThreads + threadIdx.x;
    if (b < a.B) program_row(a.r[blockIdx.y], b);
}

// One element of the PID (velocity_controller.py:100-134): e = u - vel; the integral term (1 / T_i)
// * clamp(accum += dt e); the derivative term T_d (e - prev) / dt; u = (gain (e + I + D)) * mass.
VMAS_HD void pid_element(const VmasVelocityPidRef& r, long b, int c) {
#pragma clang fp contract(off)
    const long i = b * r.dim + c;
    const float err = r.u[b * r.u_s0 + c * r.u_s1] - r.vel[b * r.vel_s0 + c * r.vel_s1];
    float integ = 0.0f;  // (the reference's `err + 0` without the integrator)
    if (r.use_integrator) {
        float acc = r.accum[i] + r.dt * err;
        r.accum[i] = acc;  // (`+=`: in place, before the clamp re-binds)
        if (r.accum_clamped) {
            acc = clamp_sym(acc, r.cutoff);
            r.accum_clamped[i] = acc;
        }
        integ = r.inv_ti * acc;
    }
    const float rate = div_by(r.t_d * (err - r.prev_err[i]), r.dt, r.inv_dt, r.div_mode);
    r.err_out[i] = err;
    r.u_out[i] = (r.gain * ((err + integ) + rate)) * r.mass;
}

__global__ void __launch_bounds__(kThreads) k_velocity_pid(VmasVelocityPidRef r, long total) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i < total) pid_element(r, i / r.dim, (int)(i % r.dim));
}

const char* ref_error(const VmasActionProgramRef& r) {
    if (r.kind < VMAS_DYNAMICS_DIFF_DRIVE || r.kind > VMAS_DYNAMICS_DRONE) return "unknown kind";
    if (r.integration != VMAS_INTEGRATION_EULER && r.integration != VMAS_INTEGRATION_RK4) return "unknown integration";
    if (r.div_mode != 0 && r.div_mode != 1) return "division mode";
    if (!r.u || !r.pos || !r.vel || !r.rot || !r.ang_vel || !r.force || !r.torque) return "null pointer";
    if (r.kind == VMAS_DYNAMICS_DRONE && (!r.drone_in || !r.drone_out)) return "null drone_state";
    if (r.u_s0 < 0 || r.u_s1 < 0 || r.pos_s0 < 0 || r.pos_s1 < 0 || r.vel_s0 < 0 || r.vel_s1 < 0 || r.rot_s0 < 0 ||
        r.ang_s0 < 0 || r.force_s0 < 0 || r.force_s1 < 0)
        return "negative stride";
    return nullptr;
}

int32_t enter_device(int device) {
    int cur = -1;
    VMAS_AUX_HIP(hipGetDevice(&cur));
    if (cur != device) VMAS_AUX_HIP(hipSetDevice(device));
    return VMAS_OK;
}

}  // namespace

extern "C" {

int32_t vmas_action_programs(int32_t device, int32_t batch, const VmasActionProgramRef* refs, int32_t n_refs,
                             void* stream) {
    if (device >= 64 || batch <= 0 || n_refs <= 0 || !refs)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_action_programs: bad arguments");
    for (int i = 0; i < n_refs; ++i)
        if (const char* why = ref_error(refs[i]))
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_action_programs: bad ref %d (%s)", i, why);
    if (device < 0) {
        for (int i = 0; i < n_refs; ++i)
            for (long b = 0; b < batch; ++b) program_row(refs[i], b);
        return VMAS_OK;
    }
    if (int32_t rc = enter_device(device)) return rc;
    const unsigned gx = (unsigned)(((long)batch + kThreads - 1) / kThreads);
    for (int first = 0; first < n_refs; first += kMaxRefsPerLaunch) {
        const int n = std::min(kMaxRefsPerLaunch, n_refs - first);
        ProgramArgs a{};
        for (int i = 0; i < n; ++i) a.r[i] = refs[first + i];
        a.B = batch;
        hipLaunchKernelGGL(k_action_programs, dim3(gx, n), dim3(kThreads), 0, (hipStream_t)stream, a);
        VMAS_AUX_HIP(hipGetLastError());
    }
    return VMAS_OK;
}

int32_t vmas_velocity_pid(int32_t device, int32_t batch, const VmasVelocityPidRef* ref, void* stream) {
    if (device >= 64 || batch <= 0 || !ref) return vmas_aux::fail(VMAS_E_INVALID, "vmas_velocity_pid: bad arguments");
    const VmasVelocityPidRef& r = *ref;
    if (!r.u || !r.vel || !r.u_out || !r.err_out || !r.prev_err || (r.use_integrator && !r.accum))
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_velocity_pid: null pointer");
    if (r.u_s0 < 0 || r.u_s1 < 0 || r.vel_s0 < 0 || r.vel_s1 < 0)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_velocity_pid: negative stride");
    if (r.dim <= 0 || r.dim > 64 || (r.div_mode != 0 && r.div_mode != 1))
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_velocity_pid: bad dim or division mode");
    const long total = (long)batch * r.dim;
    if (device < 0) {
        for (long b = 0; b < batch; ++b)
            for (int c = 0; c < r.dim; ++c) pid_element(r, b, c);
        return VMAS_OK;
    }
    if (int32_t rc = enter_device(device)) return rc;
    const unsigned gx = (unsigned)((total + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_velocity_pid, dim3(gx), dim3(kThreads), 0, (hipStream_t)stream, r, total);
    VMAS_AUX_HIP(hipGetLastError());
    return VMAS_OK;
}

}  // extern "C"
