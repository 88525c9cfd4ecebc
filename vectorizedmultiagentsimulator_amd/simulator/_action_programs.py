"""Native action programs: DiffDrive / KinematicBicycle / Drone ``process_action`` and the
VelocityController's ``process_force`` as one launch each (csrc/vmas_action_programs.hip) in place
of the reference's per-agent tensor programs (~60 small kernels for an RK4 DiffDrive agent).

Selection.  A model runs natively only when
  * its type is exactly the package's class (a subclass may override ``f`` or the PID terms);
  * no autograd is involved (``world`` not ``grad_enabled``, no operand requires grad);
  * every operand is a float32 tensor of the expected shape on one device, the constants are
    Python numbers;
  * the device is ROCm (on ``cpu`` the torch program stays: its vectorised trig cannot be matched
    bit for bit; the library's host backend serves the ABI and its tests);
  * a first-use probe per (device, model, integration) found the native result equal to the torch
    program's bit for bit on a fixed 4 096-row input.
Otherwise the torch program (``process_action_torch`` / ``process_force_torch``) runs, and
``status`` gives the reason -- never an error.

Binding contract (what the reference leaves observable): ``state.force`` is written in place (same
object, version bumped), ``state.torque`` re-bound to a new [B, 1] tensor; the drone adds m g to
``u[:, 0]`` in place, writes pos / rot into columns X, Y, PSI of the current ``drone_state`` and
re-binds ``drone_state``; the PID re-binds ``agent.action.u`` and ``prev_err``, adds into
``accum_errs`` in place and re-binds it only when the windup clamp applies.

Batching.  Inside ``batch()`` (the Environment's step loops, when nothing can observe the order)
the dynamics calls are collected and issued as ONE ``vmas_action_programs`` launch at its end; a
call outside it launches at once.
"""
from __future__ import annotations

import contextlib
import types
from typing import Optional

import numpy as np
import torch

from .. import _native as N

_F32 = np.float32


def _num(x) -> bool:
    return isinstance(x, (int, float)) and not isinstance(x, bool)


# (str(device), model name, variant) -> None: native equals torch; str: why not
PROBES = {}
_DIV_MODES = {}  # str(device) -> 0 (divide), 1 (multiply by the fp32 reciprocal), None
PROBE_ROWS = 4096

_current = None  # the _Batch collecting dynamics calls, if any


def _kinds():
    from .dynamics.diff_drive import DiffDrive
    from .dynamics.drone import Drone
    from .dynamics.kinematic_bicycle import KinematicBicycle

    return {DiffDrive: N.DYNAMICS_DIFF_DRIVE, KinematicBicycle: N.DYNAMICS_BICYCLE, Drone: N.DYNAMICS_DRONE}


def _inv(x, mode: int = 1) -> np.float32:
    """The fp32 reciprocal a torch build multiplies by in place of dividing by the Python number
    ``x``: mode 1, 1.0f / f32(x) (the fp32 division); mode 2, f32(1.0 / x) (divided in double,
    rounded once).  The two differ in the last bit for e.g. 0.12 and 0.0142, agree for 0.01."""
    with np.errstate(divide="ignore"):
        return _F32(np.float64(1.0) / np.float64(x)) if mode == 2 else _F32(1) / _F32(x)


_DIV_PROBE = (0.1 ** 2, 3.0, 0.0081, 0.0142, 0.12, 0.7)  # (0.0142 and 0.12 tell modes 1 and 2 apart)


def div_mode(device) -> Optional[int]:
    """How this torch build divides a float32 tensor by a Python number on ``device``: 0 divides, 1
    and 2 multiply by a fp32 reciprocal (``_inv``), None: none of them reproduces it (probed once
    per device, as _discrete.mode probes its own division)."""
    device = torch.device(device)
    if device.type != "cuda":
        return 0
    key = str(device)
    if key not in _DIV_MODES:
        x = np.concatenate([np.linspace(0.37, 1913.0, 2048, dtype=_F32), np.linspace(-1.0, 1.0, 2048, dtype=_F32)])
        got = [(torch.from_numpy(x).to(device) / d).cpu().numpy() for d in _DIV_PROBE]
        found = None
        for md in (0, 1, 2):
            if all(np.array_equal(g, x / _F32(d) if md == 0 else x * _inv(d, md)) for g, d in zip(got, _DIV_PROBE)):
                found = md
                break
        _DIV_MODES[key] = found
    return _DIV_MODES[key]


class _Batch:
    """Dynamics refs collected for one launch; holds the tensors the refs point into."""

    def __init__(self):
        self.rows, self.keep, self.bumps = [], [], []
        self.device = None
        self.B = 0

    def flush(self) -> None:
        if not self.rows:
            return
        refs = np.concatenate(self.rows)
        idx, stream = N.launch_args(self.device)
        N.check_aux(N.action_programs(idx, self.B, refs, stream), "vmas_action_programs")
        torch.autograd.graph.increment_version(self.bumps)  # (written through raw pointers)
        self.rows, self.keep, self.bumps = [], [], []


@contextlib.contextmanager
def batch(enabled: bool = True):
    """Collect the native dynamics calls made inside into one launch at the end (``enabled``
    False: every call launches where it runs)."""
    global _current
    if not enabled:
        yield None
        return
    prev, _current = _current, _Batch()
    b = _current
    try:
        yield b
    finally:
        _current = prev
        b.flush()


def batchable(env) -> bool:
    """Nothing can observe the order of the agents' dynamics calls: the scenario's class does not
    override process_action / env_process_action (nor its instance) and no agent is scripted."""
    from .scenario import BaseScenario

    scn = env.scenario
    cls, inst = type(scn), getattr(scn, "__dict__", {})
    return (cls.process_action is BaseScenario.process_action
            and cls.env_process_action is BaseScenario.env_process_action
            and "process_action" not in inst and "env_process_action" not in inst
            and all(ag.action_script is None for ag in env.world.agents))


# ---- dynamics -----------------------------------------------------------------------------------
def _f32_2d(t, B, cols, name) -> Optional[str]:
    if not isinstance(t, torch.Tensor):
        return f"{name} is not a tensor"
    if t.dtype is not torch.float32:
        return f"{name} is {str(t.dtype).replace('torch.', '')}"
    if t.dim() != 2 or t.shape[0] != B or t.shape[1] < cols:
        return f"{name} has shape {tuple(t.shape)}"
    if t.requires_grad:
        return f"autograd ({name} requires grad)"
    return None


def _dynamics_operands(dyn, kind):
    """(operands, None) or (None, reason)."""
    ag = dyn.agent
    st = ag.state
    u = ag.action.u
    if not isinstance(u, torch.Tensor):
        return None, "no action set"
    B = u.shape[0] if u.dim() == 2 else -1
    ops = [("u", u, 4 if kind == N.DYNAMICS_DRONE else 2), ("pos", st.pos, 2), ("vel", st.vel, 2), ("rot", st.rot, 1),
           ("ang_vel", st.ang_vel, 1), ("force", st.force, 2)]
    if kind == N.DYNAMICS_DRONE:
        ops.append(("drone_state", dyn.drone_state, 12))
    for name, t, cols in ops:
        why = _f32_2d(t, B, cols, name)
        if why is None and t.device != u.device:
            why = f"{name} is on {t.device}"
        if why is not None:
            return None, why
    if kind == N.DYNAMICS_DRONE and (dyn.drone_state.shape[1] != 12 or not dyn.drone_state.is_contiguous()):
        return None, "drone_state is not a contiguous [B, 12] tensor"
    return [t for _, t, _ in ops], None


def _dynamics_constants(dyn, kind) -> Optional[tuple]:
    ag = dyn.agent
    c = (ag.mass, ag.moment_of_inertia, dyn.dt, dyn.integration)
    if kind == N.DYNAMICS_BICYCLE:
        c += (dyn.l_f, dyn.l_r, dyn.max_steering_angle)
    elif kind == N.DYNAMICS_DRONE:
        c += (dyn.I_xx, dyn.I_yy, dyn.I_zz, dyn.g)
    return c if all(_num(x) for x in c[:3] + c[4:]) and c[3] in ("euler", "rk4") else None


def _dynamics_row(kind, c, mode) -> np.ndarray:
    """The ref's scalar fields: each Python number as torch enters it -- the expression evaluated
    in double, rounded once to fp32; reciprocals as the probed mode makes them (_inv)."""
    r = np.zeros(1, dtype=N.ACTION_PROGRAM_REF_DTYPE)
    mass, moi, dt, integ = c[:4]
    r["kind"], r["integration"] = kind, (N.INTEGRATION_RK4 if integ == "rk4" else N.INTEGRATION_EULER)
    r["div_mode"] = int(mode != 0)
    r["mass"], r["moment_of_inertia"], r["dt"] = mass, moi, dt
    r["dt2"], r["inv_dt2"], r["dt_6"] = dt ** 2, _inv(dt ** 2, mode), dt / 6
    if kind == N.DYNAMICS_BICYCLE:
        l_f, l_r, ms = c[4:]
        r["l_r"], r["wheelbase"], r["inv_wheelbase"], r["max_steering_angle"] = l_r, l_f + l_r, _inv(l_f + l_r, mode), ms
    elif kind == N.DYNAMICS_DRONE:
        ixx, iyy, izz, g = c[4:]
        r["inv_mass"], r["g"], r["mass_g"] = _inv(mass, mode), g, mass * g
        r["i_yz"], r["i_zx"], r["i_xy"] = iyy - izz, izz - ixx, ixx - iyy
        r["i_xx"], r["i_yy"], r["i_zz"] = ixx, iyy, izz
        r["inv_i_xx"], r["inv_i_yy"], r["inv_i_zz"] = _inv(ixx, mode), _inv(iyy, mode), _inv(izz, mode)
    return r


_ROWS = {}  # (kind, constants, mode) -> the ref row with its scalar fields set


def dynamics_native(dyn, mode: Optional[int] = None, collect: bool = True) -> Optional[str]:
    """Run ``dyn``'s process_action natively (whatever the device: ``cpu`` tensors take the
    library's host backend), with the binding contract of the module notes.  Returns None, or the
    reason nothing was done.  No selection rule is applied here (``dynamics``).  ``collect`` False
    launches at once even inside ``batch()`` (the probe reads the result right away)."""
    kind = _kinds().get(type(dyn))
    if kind is None:
        return "not a kinematic model of the package"
    ops, why = _dynamics_operands(dyn, kind)
    if why is not None:
        return why
    c = _dynamics_constants(dyn, kind)
    if c is None:
        return "a model constant is not a Python number"
    u, pos, vel, rot, ang, force = ops[:6]
    if mode is None:
        mode = div_mode(u.device)
        if mode is None:
            return "no division mode reproduces this torch build"
    key = (kind, c, mode)
    row = _ROWS.get(key)
    if row is None:
        if len(_ROWS) > 256:
            _ROWS.clear()
        row = _ROWS[key] = _dynamics_row(kind, c, mode)
    r = row.copy()
    B = u.shape[0]
    torque = torch.empty(B, 1, dtype=torch.float32, device=u.device)
    r["u"], r["pos"], r["vel"], r["rot"] = u.data_ptr(), pos.data_ptr(), vel.data_ptr(), rot.data_ptr()
    r["ang_vel"], r["force"], r["torque"] = ang.data_ptr(), force.data_ptr(), torque.data_ptr()
    (r["u_s0"], r["u_s1"]), (r["pos_s0"], r["pos_s1"]), (r["vel_s0"], r["vel_s1"]) = u.stride(), pos.stride(), vel.stride()
    r["rot_s0"], r["ang_s0"] = rot.stride(0), ang.stride(0)
    r["force_s0"], r["force_s1"] = force.stride()
    bumps = [force]
    keep = [u, pos, vel, rot, ang, force, torque]
    if kind == N.DYNAMICS_DRONE:
        din = ops[6]
        dout = torch.empty_like(din)
        r["drone_in"], r["drone_out"] = din.data_ptr(), dout.data_ptr()
        bumps += [u, din]
        keep += [din, dout]
    b = _current if collect else None
    if b is not None and (b.device is None or (b.device == u.device and b.B == B)):
        b.device, b.B = u.device, B
        b.rows.append(r)
        b.keep += keep
        b.bumps += bumps
    else:
        idx, stream = N.launch_args(u.device)
        N.check_aux(N.action_programs(idx, B, r, stream), "vmas_action_programs")
        torch.autograd.graph.increment_version(bumps)
    dyn.agent.state.torque = torque
    if kind == N.DYNAMICS_DRONE:
        dyn.drone_state = dout
    return None


def _fake_agent(real, B, device, gen, u_cols):
    def rnd(cols, lo, hi):
        return (torch.rand(B, cols, generator=gen) * (hi - lo) + lo).to(device)

    st = types.SimpleNamespace(pos=rnd(2, -1, 1), vel=rnd(2, -1, 1), rot=rnd(1, -np.pi, np.pi), ang_vel=rnd(1, -1, 1),
                               force=torch.zeros(B, 2, device=device), torque=torch.zeros(B, 1, device=device))
    return types.SimpleNamespace(state=st, action=types.SimpleNamespace(u=rnd(u_cols, -1, 1)), mass=real.mass,
                                 moment_of_inertia=getattr(real, "moment_of_inertia", None), max_f=None, f_range=None)


def _clone_obj(obj, **attrs):
    c = object.__new__(type(obj))
    c.__dict__.update(obj.__dict__)
    c.__dict__.update(attrs)
    return c


def _clone_agent(ag):
    st = types.SimpleNamespace(**{k: v.clone() for k, v in vars(ag.state).items()})
    return types.SimpleNamespace(state=st, action=types.SimpleNamespace(u=ag.action.u.clone()), mass=ag.mass,
                                 moment_of_inertia=ag.moment_of_inertia, max_f=None, f_range=None)


def _probe_dynamics(dyn, kind, device) -> Optional[str]:
    key = (str(device), type(dyn).__name__, dyn.integration)
    if key in PROBES:
        return PROBES[key]
    if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        return "first use inside a stream capture"
    mode = div_mode(device)
    if mode is None:
        PROBES[key] = "no division mode reproduces this torch build"
        return PROBES[key]
    gen = torch.Generator().manual_seed(20240607)
    B = PROBE_ROWS
    a_t = _fake_agent(dyn.agent, B, device, gen, 4 if kind == N.DYNAMICS_DRONE else 2)
    extra = {}
    if kind == N.DYNAMICS_DRONE:
        ds = torch.rand(B, 12, generator=gen) * 2 - 1
        ds[:, :2] *= 0.3
        extra["drone_state"] = ds.to(device)
    a_n = _clone_agent(a_t)
    d_t = _clone_obj(dyn, _agent=a_t, **extra)
    d_n = _clone_obj(dyn, _agent=a_n, **{k: v.clone() for k, v in extra.items()})
    old_t, old_n = extra.get("drone_state"), d_n.__dict__.get("drone_state")
    with torch.no_grad():
        type(dyn).process_action_torch(d_t)
    why = dynamics_native(d_n, mode, collect=False)
    if why is None:
        pairs = [("force", a_t.state.force, a_n.state.force), ("torque", a_t.state.torque, a_n.state.torque),
                 ("u", a_t.action.u, a_n.action.u)]
        if kind == N.DYNAMICS_DRONE:
            pairs += [("drone_state", d_t.drone_state, d_n.drone_state), ("previous drone_state", old_t, old_n)]
        bad = [n for n, x, y in pairs if not torch.equal(x, y)]
        if bad:
            why = "the probe differs from the torch program in " + ", ".join(bad)
    PROBES[key] = why
    return why


def _dynamics_reason(dyn) -> Optional[str]:
    """None: native; "": not a kinematic model; else why the torch program runs."""
    kinds = _kinds()
    kind = kinds.get(type(dyn))
    if kind is None:
        base = next((c for c in kinds if isinstance(dyn, c)), None)
        return "" if base is None else f"{type(dyn).__name__} is a subclass of {base.__name__}"
    w = dyn.world
    if getattr(w, "_grad_enabled", False) or getattr(w, "grad_enabled", False):
        return "autograd (the world is grad_enabled)"
    ag = dyn._agent
    if ag is None:
        return "no agent"
    if isinstance(ag.action.u, torch.Tensor):
        _, why = _dynamics_operands(dyn, kind)
        if why is not None:
            return why
    if _dynamics_constants(dyn, kind) is None:
        return "a model constant is not a Python number"
    device = torch.device(w.device)
    if device.type != "cuda":
        return f"device is {device.type} (the torch program is the product there)"
    return _probe_dynamics(dyn, kind, device)


def dynamics(dyn) -> bool:
    """process_action's choice: True when the native program ran."""
    return _dynamics_reason(dyn) is None and dynamics_native(dyn) is None


def _status(reason: Optional[str]) -> str:
    return "native" if reason is None else ("none" if reason == "" else f"torch: {reason}")


def dynamics_status(dyn) -> str:
    return _status(_dynamics_reason(dyn))


# ---- the PID ------------------------------------------------------------------------------------
def _pid_constants(c) -> Optional[tuple]:
    cut = getattr(c, "integrator_windup_cutoff", None) if c.use_integrator else None
    k = (c.ctrl_gain, c.integralTs, c.derivativeTs, c.dt, c.agent.mass, bool(c.use_integrator), cut)
    return k if all(_num(x) for x in k[:5]) and (cut is None or _num(cut)) else None


def _pid_operands(c):
    ag = c.agent
    u, vel = ag.action.u, ag.state.vel
    if not isinstance(u, torch.Tensor):
        return None, "no action set"
    B = u.shape[0] if u.dim() == 2 else -1
    for name, t in (("u", u), ("vel", vel), ("accum_errs", c.accum_errs), ("prev_err", c.prev_err)):
        why = _f32_2d(t, B, 1, name)
        if why is None and (t.shape != u.shape or t.device != u.device):
            why = f"{name} has shape {tuple(t.shape)} on {t.device}"
        if why is not None:
            return None, why
    if not c.accum_errs.is_contiguous() or not c.prev_err.is_contiguous():
        return None, "accum_errs / prev_err are not contiguous"
    return (u, vel), None


def pid_native(c, mode: Optional[int] = None) -> Optional[str]:
    """``c.process_force()`` natively (``cpu`` tensors: the host backend); None or the reason
    nothing was done."""
    ops, why = _pid_operands(c)
    if why is not None:
        return why
    k = _pid_constants(c)
    if k is None:
        return "a controller parameter is not a Python number"
    u, vel = ops
    if mode is None:
        mode = div_mode(u.device)
        if mode is None:
            return "no division mode reproduces this torch build"
    gain, ti, td, dt, mass, use_i, cut = k
    B, D = u.shape
    r = np.zeros(1, dtype=N.VELOCITY_PID_REF_DTYPE)
    u_out, err = torch.empty_like(c.prev_err), torch.empty_like(c.prev_err)
    acc = c.accum_errs
    clamped = torch.empty_like(acc) if (use_i and cut is not None) else None
    r["u"], r["vel"], r["u_out"], r["err_out"], r["prev_err"] = (u.data_ptr(), vel.data_ptr(), u_out.data_ptr(),
                                                                 err.data_ptr(), c.prev_err.data_ptr())
    r["accum"] = acc.data_ptr() if use_i else 0
    r["accum_clamped"] = clamped.data_ptr() if clamped is not None else 0
    (r["u_s0"], r["u_s1"]), (r["vel_s0"], r["vel_s1"]) = u.stride(), vel.stride()
    r["dim"], r["use_integrator"], r["div_mode"] = D, int(use_i), int(mode != 0)
    r["gain"], r["t_d"], r["dt"], r["inv_dt"], r["mass"] = gain, td, dt, _inv(dt, mode), mass
    if use_i:
        r["inv_ti"] = 1.0 / ti
        if cut is not None:
            r["cutoff"] = cut
    idx, stream = N.launch_args(u.device)
    N.check_aux(N.velocity_pid(idx, B, r, stream), "vmas_velocity_pid")
    if use_i:
        torch.autograd.graph.increment_version(acc)  # (`+=`: written through a raw pointer)
        if clamped is not None:
            c.accum_errs = clamped
    c.prev_err = err
    c.agent.action.u = u_out
    return None


def _pid_variant(c):
    cut = getattr(c, "integrator_windup_cutoff", None) if c.use_integrator else None
    return "no integrator" if not c.use_integrator else ("cutoff" if cut is not None else "no cutoff")


def _probe_pid(c, device) -> Optional[str]:
    key = (str(device), "VelocityController", _pid_variant(c))
    if key in PROBES:
        return PROBES[key]
    if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        return "first use inside a stream capture"
    mode = div_mode(device)
    if mode is None:
        PROBES[key] = "no division mode reproduces this torch build"
        return PROBES[key]
    gen = torch.Generator().manual_seed(20240608)
    B, D = PROBE_ROWS, c.prev_err.shape[1]
    a_t = _fake_agent(c.agent, B, device, gen, D)
    a_t.state.vel = (torch.rand(B, D, generator=gen) * 2 - 1).to(device)
    state = {"accum_errs": ((torch.rand(B, D, generator=gen) * 2 - 1) * 0.05).to(device),
             "prev_err": (torch.rand(B, D, generator=gen) * 2 - 1).to(device)}
    a_n = _clone_agent(a_t)
    c_t = _clone_obj(c, agent=a_t, **state)
    c_n = _clone_obj(c, agent=a_n, **{k: v.clone() for k, v in state.items()})
    why = None
    for _ in range(2):  # (the second call reads what the first carried)
        with torch.no_grad():
            type(c).process_force_torch(c_t)
        why = pid_native(c_n, mode)
        if why is not None:
            break
        bad = [n for n, x, y in (("u", a_t.action.u, a_n.action.u), ("accum_errs", c_t.accum_errs, c_n.accum_errs),
                                 ("prev_err", c_t.prev_err, c_n.prev_err)) if not torch.equal(x, y)]
        if bad:
            why = "the probe differs from the torch program in " + ", ".join(bad)
            break
        u_next = (torch.rand(B, D, generator=gen) * 2 - 1).to(device)
        a_t.action.u, a_n.action.u = u_next, u_next.clone()
    PROBES[key] = why
    return why


def _pid_reason(c) -> Optional[str]:
    from .controllers.velocity_controller import VelocityController

    if not isinstance(c, VelocityController):
        return ""
    if type(c) is not VelocityController:
        return f"{type(c).__name__} is a subclass of VelocityController"
    w = c.world
    if getattr(w, "_grad_enabled", False) or getattr(w, "grad_enabled", False):
        return "autograd (the world is grad_enabled)"
    if isinstance(c.agent.action.u, torch.Tensor):
        _, why = _pid_operands(c)
        if why is not None:
            return why
    if _pid_constants(c) is None:
        return "a controller parameter is not a Python number"
    device = torch.device(w.device)
    if device.type != "cuda":
        return f"device is {device.type} (the torch program is the product there)"
    return _probe_pid(c, device)


def pid(c) -> bool:
    """process_force's choice: True when the native program ran."""
    return _pid_reason(c) is None and pid_native(c) is None


def pid_status(c) -> str:
    return _status(_pid_reason(c))


def env_status(env) -> dict:
    """Environment.action_programs."""
    out = {}
    for ag in env.world.agents:
        out[ag.name] = dynamics_status(ag.dynamics)
        c = getattr(ag, "controller", None)
        if c is not None:
            out[f"{ag.name}.controller"] = pid_status(c)
    return out
