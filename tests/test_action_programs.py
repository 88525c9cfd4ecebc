"""The native action programs on the host backend (csrc/vmas_action_programs.hip, device == -1),
driven through ``_native`` / ``simulator/_action_programs.py``: the C ABI and its argument checks,
the arithmetic of every model against the package's torch program evaluated in fp64, the PID over
consecutive calls, strided operands, and the selection rule on ``cpu`` (where the torch program
stays the product).

Tolerance of the arithmetic tests (measured, not fixed in advance): E is the largest absolute
error, per output, of the torch program in fp32 against the same program in fp64 on a 4 096-row
draw; the native result must be within 2 E of the fp64 result (two correctly behaving libm
roundings each contribute up to E).  The PID has no trig: its native result equals the fp32 torch
program bit for bit, which the test also asserts."""
import functools
import math
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd.simulator import _action_programs as AP
from vectorizedmultiagentsimulator_amd.simulator.controllers.velocity_controller import VelocityController
from vectorizedmultiagentsimulator_amd.simulator.core import Agent, World
from vectorizedmultiagentsimulator_amd.simulator.dynamics.diff_drive import DiffDrive
from vectorizedmultiagentsimulator_amd.simulator.dynamics.drone import Drone
from vectorizedmultiagentsimulator_amd.simulator.dynamics.kinematic_bicycle import KinematicBicycle

MODELS = {
    "diff_drive": lambda w, i: DiffDrive(w, integration=i),
    "bicycle": lambda w, i: KinematicBicycle(w, width=0.1, l_f=0.07, l_r=0.05, max_steering_angle=0.6, integration=i),
    "drone": lambda w, i: Drone(w, integration=i),
}
E_ROWS = 4096


def draw(model, B, seed):
    """fp32 inputs of the issue's distribution: theta in [-pi, pi], speeds and commands within +-1
    (the steering limit is 0.6, so the clamp is hit), drone roll / pitch within +-0.3, rates +-1."""
    g = torch.Generator().manual_seed(seed)

    def r(cols, scale):
        return (torch.rand(B, cols, generator=g) * 2 - 1) * scale

    d = dict(pos=r(2, 1), vel=r(2, 1), rot=r(1, math.pi), ang_vel=r(1, 1), u=r(4 if model == "drone" else 2, 1))
    if model == "drone":
        ds = r(12, 1)
        ds[:, :2] *= 0.3
        d["drone_state"] = ds
    return d


def build(model, integration, inputs, dtype=torch.float32, dyn_cls=None, device="cpu"):
    """A one-agent world holding copies of ``inputs`` in ``dtype`` on ``device``."""
    B = inputs["u"].shape[0]
    w = World(B, device)
    dyn = MODELS[model](w, integration) if dyn_cls is None else dyn_cls(w)
    a = Agent("a", dynamics=dyn, u_range=1.0)
    w.add_agent(a)
    for k in ("pos", "vel", "rot", "ang_vel"):
        setattr(a.state, k, inputs[k].to(dtype).to(device).clone())
    a.state.force = torch.zeros(B, 2, dtype=dtype, device=device)
    a.state.torque = torch.zeros(B, 1, dtype=dtype, device=device)
    a.action.u = inputs["u"].to(dtype).to(device).clone()
    if "drone_state" in inputs:
        dyn.drone_state = inputs["drone_state"].to(dtype).to(device).clone()
    return w, a


def outputs(a):
    out = {"force": a.state.force, "torque": a.state.torque}
    if isinstance(a.dynamics, Drone):
        out["drone_state"] = a.dynamics.drone_state
        out["u0"] = a.action.u[:, 0]
    return out


def run_torch(model, integration, inputs, dtype):
    _, a = build(model, integration, inputs, dtype)
    a.dynamics.process_action_torch()
    return outputs(a)


def run_native(model, integration, inputs):
    _, a = build(model, integration, inputs)
    assert AP.dynamics_native(a.dynamics) is None
    return outputs(a)


@functools.lru_cache(maxsize=None)
def torch_error(model, integration):
    """E per output over the 4 096-row draw."""
    inp = draw(model, E_ROWS, 1234)
    hi, lo = run_torch(model, integration, inp, torch.float64), run_torch(model, integration, inp, torch.float32)
    return {k: (lo[k].double() - hi[k]).abs().max().item() for k in hi}


# ---- ABI ----------------------------------------------------------------------------------------
def _ref(a, **over):
    r = np.zeros(1, dtype=N.ACTION_PROGRAM_REF_DTYPE)
    st = a.state
    torque = torch.full((a.action.u.shape[0], 1), 7.0)
    for k, t in (("u", a.action.u), ("pos", st.pos), ("vel", st.vel), ("rot", st.rot), ("ang_vel", st.ang_vel),
                 ("force", st.force), ("torque", torque)):
        r[k] = t.data_ptr()
    (r["u_s0"], r["u_s1"]), (r["pos_s0"], r["pos_s1"]), (r["vel_s0"], r["vel_s1"]) = (2, 1), (2, 1), (2, 1)
    r["rot_s0"], r["ang_s0"], r["force_s0"], r["force_s1"] = 1, 1, 2, 1
    r["kind"], r["integration"], r["mass"], r["moment_of_inertia"] = N.DYNAMICS_DIFF_DRIVE, N.INTEGRATION_RK4, 1, 1
    r["dt"], r["dt2"], r["inv_dt2"], r["dt_6"] = 0.1, 0.01, 100, 0.1 / 6
    for k, v in over.items():
        r[k] = v
    return r, torque


def test_abi_exports_and_bad_arguments():
    lib = N.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (vmas_\w+)", out))
    assert {"vmas_action_programs", "vmas_velocity_pid"} <= exported
    assert {"vmas_action_programs", "vmas_velocity_pid"} <= set(N.EXPORTED_SYMBOLS)

    _, a = build("diff_drive", "rk4", draw("diff_drive", 5, 0))
    a.state.force.fill_(7.0)
    good, good_torque = _ref(a)  # (the ref points into good_torque: kept alive to the last call)
    for over, n, word in (({"u": 0}, 1, b"null"), ({"vel_s0": -2}, 1, b"negative stride"), ({"kind": 3}, 1, b"kind"),
                          ({}, 0, b"bad arguments")):
        r, torque = _ref(a, **over)
        rc = lib.vmas_action_programs(-1, 5, r.ctypes.data, n, None)
        assert rc == -1, (over, n, rc)  # VMAS_E_INVALID
        assert word in lib.vmas_aux_last_error(), (over, lib.vmas_aux_last_error())
        assert (a.state.force == 7.0).all() and (torque == 7.0).all()  # nothing written
    # a bad ref after a good one: nothing of the good one is written either
    two = np.concatenate([good, _ref(a, integration=2)[0]])
    assert lib.vmas_action_programs(-1, 5, two.ctypes.data, 2, None) == -1
    assert (a.state.force == 7.0).all()
    assert lib.vmas_action_programs(-1, 5, good.ctypes.data, 1, None) == 0
    assert not (a.state.force == 7.0).any() and not (good_torque == 7.0).any()

    p = np.zeros(1, dtype=N.VELOCITY_PID_REF_DTYPE)
    assert lib.vmas_velocity_pid(-1, 5, p.ctypes.data, None) == -1 and b"null" in lib.vmas_aux_last_error()
    assert lib.vmas_velocity_pid(-1, 5, None, None) == -1


def test_ref_layouts_match_the_header(tmp_path):
    probe = ('#include <stdio.h>\n#include "vmas_mi355x.h"\nint main(void) { printf("%zu %zu\\n", '
             "sizeof(VmasActionProgramRef), sizeof(VmasVelocityPidRef)); return 0; }\n")
    (tmp_path / "p.c").write_text(probe)
    inc = N.LIB_PATH.parent.parent / "include"
    subprocess.run(["gcc", "-I", str(inc), str(tmp_path / "p.c"), "-o", str(tmp_path / "p")], check=True)
    sizes = list(map(int, subprocess.run([str(tmp_path / "p")], capture_output=True, text=True).stdout.split()))
    assert sizes == [N.ACTION_PROGRAM_REF_DTYPE.itemsize, N.VELOCITY_PID_REF_DTYPE.itemsize]


# ---- arithmetic ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 65, 257])
@pytest.mark.parametrize("integration", ["euler", "rk4"])
@pytest.mark.parametrize("model", list(MODELS))
def test_native_within_twice_the_fp32_error(model, integration, B):
    E = torch_error(model, integration)
    inp = draw(model, B, 100 + B)
    hi = run_torch(model, integration, inp, torch.float64)
    got = run_native(model, integration, inp)
    for k in hi:
        err = (got[k].double() - hi[k]).abs().max().item()
        print(f"{model} {integration} B={B} {k}: E={E[k]:.3e} native error={err:.3e}")
        assert err <= 2 * E[k], (k, err, E[k])


def test_more_than_eight_refs_are_chunked():
    inp = draw("diff_drive", 9, 5)
    agents = [build("diff_drive", "rk4", inp)[1] for _ in range(11)]
    want = run_native("diff_drive", "rk4", inp)
    calls = N.ACTION_PROGRAM_CALLS["vmas_action_programs"]
    with AP.batch():
        for a in agents:
            assert AP.dynamics_native(a.dynamics) is None
    assert N.ACTION_PROGRAM_CALLS["vmas_action_programs"] == calls + 1
    for a in agents:
        assert torch.equal(a.state.force, want["force"]) and torch.equal(a.state.torque, want["torque"])


# ---- PID ----------------------------------------------------------------------------------------
def _pid(B, params, form, f_range, device="cpu"):
    w = World(B, device)
    a = Agent("a", f_range=f_range)
    w.add_agent(a)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = VelocityController(a, w, params, form)
    return w, a, c


def _pid_run(native, B, params, form, f_range, dtype, us, vels):
    w, a, c = _pid(B, params, form, f_range)
    c.accum_errs, c.prev_err = c.accum_errs.to(dtype), c.prev_err.to(dtype)
    trace = []
    for step, (u, v) in enumerate(zip(us, vels)):
        if step == 2:
            c.reset(0)
        a.action.u, a.state.vel = u.to(dtype).clone(), v.to(dtype).clone()
        if native:
            assert AP.pid_native(c) is None
        else:
            c.process_force_torch()
        trace.append({"u": a.action.u.clone(), "accum_errs": c.accum_errs.clone(), "prev_err": c.prev_err.clone()})
    return trace


PID_VARIANTS = {
    "integrator off": ((1.5, 0, 0.5), 1.0),
    "cutoff": ((1.5, 2.0, 0.5), 0.05),  # (a low force limit: the windup clamp is hit)
    "no cutoff": ((1.5, 2.0, 0.5), None),  # (the warning path)
}


@pytest.mark.parametrize("variant", list(PID_VARIANTS))
@pytest.mark.parametrize("form", ["standard", "parallel"])
def test_pid_three_calls(form, variant):
    params, f_range = PID_VARIANTS[variant]
    g = torch.Generator().manual_seed(3)
    for B in (1, 65, 257):
        us = [torch.rand(B, 2, generator=g) * 2 - 1 for _ in range(3)]
        vels = [torch.rand(B, 2, generator=g) * 2 - 1 for _ in range(3)]
        hi = _pid_run(False, B, params, form, f_range, torch.float64, us, vels)
        lo = _pid_run(False, B, params, form, f_range, torch.float32, us, vels)
        got = _pid_run(True, B, params, form, f_range, torch.float32, us, vels)
        for step in range(3):
            for k in hi[step]:
                E = (lo[step][k].double() - hi[step][k]).abs().max().item()
                err = (got[step][k].double() - hi[step][k]).abs().max().item()
                print(f"pid {form} {variant} B={B} call {step} {k}: E={E:.3e} native error={err:.3e}")
                assert err <= 2 * E
                assert torch.equal(got[step][k], lo[step][k])  # (no trig: equality, as DESIGN.md records)
    if variant == "cutoff":  # (the clamp was reached)
        cut = 0.5 * f_range * (params[1] if form == "standard" else params[0] / params[1]) / (0.1 * params[0])
        assert (got[1]["accum_errs"].abs() == np.float32(cut)).any()


def test_pid_binding_contract():
    w, a, c = _pid(5, (1.5, 2.0, 0.5), "standard", 0.05)
    a.action.u, a.state.vel = torch.ones(5, 2), torch.zeros(5, 2)
    u0, acc0, prev0 = a.action.u, c.accum_errs, c.prev_err
    v = acc0._version
    assert AP.pid_native(c) is None
    assert a.action.u is not u0 and c.prev_err is not prev0 and c.accum_errs is not acc0
    assert acc0._version > v and torch.equal(acc0, torch.full((5, 2), np.float32(0.1)))  # (`+=` before the clamp)
    assert torch.equal(u0, torch.ones(5, 2)) and torch.equal(prev0, torch.zeros(5, 2))


# ---- layout -------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", list(MODELS))
def test_strided_operands_equal_contiguous(model):
    B = 65
    inp = draw(model, B, 9)
    want = run_native(model, "rk4", inp)
    _, a = build(model, "rk4", inp)
    wide = torch.full((B, 6), 99.0)
    wide[:, 1:3], wide[:, 3:5] = inp["pos"], inp["vel"]
    a.state.pos, a.state.vel = wide[:, 1:3], wide[:, 3:5]
    k = inp["u"].shape[1]
    buf = torch.full((3 * B * k,), 99.0)
    a.action.u = buf.view(3, B, k)[1]
    a.action.u.copy_(inp["u"])
    guard = torch.full((B, 4), 55.0)
    force = guard[:, 1:3]
    a.state.force = force
    assert force.stride() == (4, 1)
    assert AP.dynamics_native(a.dynamics) is None
    got = outputs(a)
    for key in want:
        assert torch.equal(got[key], want[key]), key
    assert a.state.force is force
    assert (guard[:, 0] == 55.0).all() and (guard[:, 3] == 55.0).all()
    assert (wide[:, 0] == 99.0).all() and (wide[:, 5] == 99.0).all()
    assert (buf.view(3, B, k)[0] == 99.0).all() and (buf.view(3, B, k)[2] == 99.0).all()


def test_dynamics_binding_contract():
    inp = draw("drone", 9, 2)
    _, a = build("drone", "rk4", inp)
    force, torque, ds, u = a.state.force, a.state.torque, a.dynamics.drone_state, a.action.u
    v = force._version
    assert AP.dynamics_native(a.dynamics) is None
    assert a.state.force is force and force._version > v
    assert a.state.torque is not torque and a.state.torque.shape == (9, 1)
    assert a.dynamics.drone_state is not ds and a.action.u is u
    assert torch.equal(ds[:, 9], inp["pos"][:, 0]) and torch.equal(ds[:, 10], inp["pos"][:, 1])
    assert torch.equal(ds[:, 2], inp["rot"][:, 0])
    assert torch.equal(u[:, 0], inp["u"][:, 0] + a.mass * a.dynamics.g)


# ---- selection rule -----------------------------------------------------------------------------
class D(DiffDrive):
    pass


def _selection_case(case):
    inp = draw("diff_drive", 17, 4)
    if case == "subclass":
        _, a = build("diff_drive", "rk4", inp, dyn_cls=D)
    else:
        w, a = build("diff_drive", "rk4", inp, torch.float64 if case == "float64" else torch.float32)
        if case == "grad":
            w._grad_enabled = True
    return a


@pytest.mark.parametrize("case,word", [("subclass", "D is a subclass of DiffDrive"), ("grad", "grad_enabled"),
                                       ("float64", "u is float64")])
def test_selection_keeps_torch_with_the_reason(case, word):
    a, b = _selection_case(case), _selection_case(case)
    status = AP.dynamics_status(a.dynamics)
    assert status.startswith("torch: ") and word in status, status
    calls = dict(N.ACTION_PROGRAM_CALLS)
    a.dynamics.process_action()
    b.dynamics.process_action_torch()
    assert N.ACTION_PROGRAM_CALLS == calls  # nothing native ran
    assert torch.equal(a.state.force, b.state.force) and torch.equal(a.state.torque, b.state.torque)


def test_environment_reports_action_programs_on_cpu():
    from tests._kinematic_scenario import Scenario
    from vectorizedmultiagentsimulator_amd import make_env

    env = make_env(Scenario(), num_envs=3, device="cpu", seed=0)
    env.step(env.get_random_actions())
    ap = env.action_programs
    assert set(ap) == {"diff_drive_0", "bicycle_1", "drone_2", "pid_3", "pid_3.controller"}
    assert ap["pid_3"] == "none"
    assert all(v.startswith("torch: device is cpu") for k, v in ap.items() if k != "pid_3"), ap
