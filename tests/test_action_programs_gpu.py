"""The native action programs on the device (csrc/vmas_action_programs.hip, gfx950): bit identity
with the package's torch programs, the binding contract, and whole environments -- eager and
graph mode -- against the same scenario built from trivial subclasses, which keep the torch path.

A model whose first-use probe failed ships on the torch path; the bit-identity test then fails
with the probe's reason (no tolerance is substituted)."""
import warnings

import pytest
import torch

from tests._kinematic_scenario import MixedScenario, Scenario
from tests.test_action_programs import MODELS, PID_VARIANTS, _pid, build, draw, outputs
from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd import make_env
from vectorizedmultiagentsimulator_amd.simulator import _action_programs as AP

pytestmark = pytest.mark.gpu
BATCHES = [1, 63, 64, 65, 257]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("integration", ["euler", "rk4"])
@pytest.mark.parametrize("model", list(MODELS))
def test_dynamics_bit_identity(gpu_device, model, integration, B):
    inp = draw(model, B, 300 + B)
    _, a = build(model, integration, inp, device=gpu_device)
    _, b = build(model, integration, inp, device=gpu_device)
    status = AP.dynamics_status(a.dynamics)
    assert status == "native", f"{model} {integration}: {status}"
    calls = N.ACTION_PROGRAM_CALLS["vmas_action_programs"]
    a.dynamics.process_action()
    assert N.ACTION_PROGRAM_CALLS["vmas_action_programs"] == calls + 1  # (outside an Environment: at once)
    b.dynamics.process_action_torch()
    got, want = outputs(a), outputs(b)
    for k in want:
        assert torch.equal(got[k], want[k]), (k, (got[k] - want[k]).abs().max().item())


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("variant", list(PID_VARIANTS))
@pytest.mark.parametrize("form", ["standard", "parallel"])
def test_pid_bit_identity(gpu_device, form, variant, B):
    params, f_range = PID_VARIANTS[variant]
    g = torch.Generator().manual_seed(B)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        (_, a, c), (_, b, d) = _pid(B, params, form, f_range, gpu_device), _pid(B, params, form, f_range, gpu_device)
    for step in range(3):
        if step == 2:
            c.reset(0)
            d.reset(0)
        u, v = torch.rand(B, 2, generator=g) * 2 - 1, torch.rand(B, 2, generator=g) * 2 - 1
        a.action.u, a.state.vel = u.to(gpu_device), v.to(gpu_device)
        b.action.u, b.state.vel = u.to(gpu_device), v.to(gpu_device)
        status = AP.pid_status(c)
        assert status == "native", f"pid {form} {variant}: {status}"
        prev = c.prev_err
        c.process_force()
        d.process_force_torch()
        assert c.prev_err is not prev
        for k, x, y in (("u", a.action.u, b.action.u), ("accum_errs", c.accum_errs, d.accum_errs),
                        ("prev_err", c.prev_err, d.prev_err)):
            assert torch.equal(x, y), (step, k, (x - y).abs().max().item())


def test_binding_contract(gpu_device):
    inp = draw("drone", 65, 2)
    _, a = build("drone", "rk4", inp, device=gpu_device)
    assert AP.dynamics_status(a.dynamics) == "native"
    force, torque, ds, u = a.state.force, a.state.torque, a.dynamics.drone_state, a.action.u
    v = force._version
    a.dynamics.process_action()
    assert a.state.force is force and force._version > v
    assert a.state.torque is not torque and a.state.torque.shape == (65, 1)
    assert a.dynamics.drone_state is not ds and a.action.u is u
    pos, rot = inp["pos"].to(gpu_device), inp["rot"].to(gpu_device)
    assert torch.equal(ds[:, 9], pos[:, 0]) and torch.equal(ds[:, 10], pos[:, 1]) and torch.equal(ds[:, 2], rot[:, 0])


# ---- environments -------------------------------------------------------------------------------
def _state(env):
    out = []
    for a in env.world.agents:
        out += [a.state.pos, a.state.vel, a.state.rot, a.state.ang_vel]
        if hasattr(a.dynamics, "drone_state"):
            out.append(a.dynamics.drone_state)
        c = getattr(a, "controller", None)
        if c is not None:
            out += [c.prev_err, c.accum_errs]
    return [t.clone() for t in out]


def _rollout(scenario, device, steps, graph, subclass, reset_after=None, B=257):
    """Per step (observations, rewards, state, native calls of the step)."""
    env = make_env(scenario(), num_envs=B, device=device, seed=0, graph_step=graph, subclass=subclass)
    env.action_programs  # (the first-use probes run here, outside the per-step call counts)
    g = torch.Generator().manual_seed(11)
    trace = []
    for s in range(steps):
        acts = [(torch.rand(B, env.get_agent_action_size(a), generator=g) * 2 - 1).to(device) for a in env.agents]
        c0 = dict(N.ACTION_PROGRAM_CALLS)
        obs, rew, _, _ = env.step(acts)
        calls = {k: N.ACTION_PROGRAM_CALLS[k] - c0[k] for k in c0}
        trace.append((obs, rew, _state(env), calls, env.graph_status))
        if s == reset_after:
            env.reset_where(torch.tensor([3, 100, 256]))
    return env, trace


def _assert_same(a, b):
    for s, (x, y) in enumerate(zip(a, b)):
        for part in range(3):
            for i, (p, q) in enumerate(zip(x[part], y[part])):
                assert torch.equal(p, q), (s, ("obs", "reward", "state")[part], i, (p - q).abs().max().item())


def test_eager_env_native_equals_torch_path(gpu_device):
    env_n, native = _rollout(Scenario, gpu_device, 8, False, False)
    env_t, torch_path = _rollout(Scenario, gpu_device, 8, False, True)
    ap_n, ap_t = env_n.action_programs, env_t.action_programs
    assert ap_n.pop("pid_3") == "none" and ap_t.pop("pid_3") == "none"  # (a Holonomic-family model)
    assert all(v == "native" for v in ap_n.values()), ap_n
    assert all(v.startswith("torch: ") for v in ap_t.values()), ap_t
    _assert_same(native, torch_path)
    for *_, calls, _status in native:  # the three dynamics in one launch, the PID in its own
        assert calls == {"vmas_action_programs": 1, "vmas_velocity_pid": 1}, calls
    assert all(t[3] == {"vmas_action_programs": 0, "vmas_velocity_pid": 0} for t in torch_path)


@pytest.mark.parametrize("subclass", [False, True], ids=["native", "torch-path"])
def test_graph_env_equals_eager(gpu_device, subclass):
    """A PID with integral and derivative times and a cutoff, an RK4 drone: their re-bound state
    (prev_err, accum_errs, drone_state) is carried by the replays.  Before ``_tracked_objects``
    visited dynamics and controllers such a world was captured and replayed with that state frozen
    at its capture-time tensors (measured: profiles/r14/action_programs/README.md)."""
    warm = 4
    _, eager = _rollout(Scenario, gpu_device, warm + 12, False, subclass, reset_after=warm + 5)
    env, graph = _rollout(Scenario, gpu_device, warm + 12, True, subclass, reset_after=warm + 5)
    assert [t[4] for t in graph[warm - 1:]] == ["graph"] * 13, (env.graph_status, env.graph_reason)
    _assert_same(eager, graph)
    assert all(t[3] == {"vmas_action_programs": 0, "vmas_velocity_pid": 0} for t in graph[warm:])  # (replays)


def test_mixed_order_launches_per_agent(gpu_device):
    _, native = _rollout(MixedScenario, gpu_device, 6, False, False)
    _, torch_path = _rollout(MixedScenario, gpu_device, 6, False, True)
    _assert_same(native, torch_path)
    for *_, calls, _status in native:
        assert calls == {"vmas_action_programs": 3, "vmas_velocity_pid": 1}, calls


def test_action_programs_reports_native_on_the_device(gpu_device):
    env = make_env(Scenario(), num_envs=8, device=gpu_device, seed=0, graph_step=False)
    env.step(env.get_random_actions())
    assert env.action_programs == {"diff_drive_0": "native", "bicycle_1": "native", "drone_2": "native",
                                   "pid_3": "none", "pid_3.controller": "native"}
