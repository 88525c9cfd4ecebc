"""The wheel and dispersion scenarios without a GPU: construction, the torch programs against the
restatements of tests/_wheel_spec.py / tests/_dispersion_spec.py on hand-placed envs, the resets'
draw order, reset_at / reset_where on ``cpu``, the host backend (device -1) of both step programs,
the v16 argument blocks and entry points, physics parity on the host backend and rendering."""
import ctypes
import math
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import _dispersion_spec as DS
from tests import _reset_where as R
from tests import _wheel_spec as WS
from tests._parity import step_parity
from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd import make_env

ROOT = Path(__file__).resolve().parent.parent
VMAS_E_INVALID = -1
ALL = N.VMAS_SCN_REWARD | N.VMAS_SCN_OBS | N.VMAS_SCN_DONE

DISPERSION_CONFIGS = {
    "default": dict(),
    "one_agent": dict(n_agents=1),
    "one_food": dict(n_food=1),
    "five_foods_three_agents": dict(n_food=5, n_agents=3),
    "share_reward": dict(share_reward=True),
    "penalise_by_time": dict(penalise_by_time=True),
    "share_and_penalise": dict(share_reward=True, penalise_by_time=True),
}
WHEEL_CONFIGS = {"default": dict(), "one_agent": dict(n_agents=1), "short_fast": dict(line_length=1.5, desired_velocity=0.2)}


def _placed(name, kw, B=64, seed=1, steps=2):
    env = make_env(name, num_envs=B, device="cpu", seed=seed, **kw)
    for _ in range(steps):
        env.step(env.get_random_actions())
    (WS if name == "wheel" else DS).place_cases(env)
    return env


# ---- construction ------------------------------------------------------------------------------------
def test_make_env_builds_both_and_rejects_unknown_kwargs():
    w = make_env("wheel", num_envs=3, device="cpu", n_agents=5, line_length=1.5, line_mass=20, desired_velocity=0.1)
    d = make_env("dispersion", num_envs=3, device="cpu", n_agents=3, share_reward=True, penalise_by_time=True,
                 food_radius=0.04, pos_range=0.8, n_food=6)
    assert len(w.agents) == 5 and len(d.agents) == 3 and len(d.world.landmarks) == 6
    assert d.world.x_semidim == d.world.y_semidim == 0.8
    for name in ("wheel", "dispersion"):
        # (ScenarioUtils.check_kwargs_consumed: a warning today, as in the reference)
        with pytest.warns(UserWarning, match="no_such_kwarg"):
            make_env(name, num_envs=3, device="cpu", no_such_kwarg=1)


def test_entities_and_observation_widths():
    w = make_env("wheel", num_envs=3, device="cpu")
    assert [a.name for a in w.agents] == [f"agent_{i}" for i in range(4)]
    assert all(a.u_multiplier == 0.6 and a.shape.radius == 0.03 and a.mass == 1.0 for a in w.agents)
    line, center = w.world.landmarks
    assert (line.name, center.name) == ("line", "center")
    assert line.mass == 30 and line.shape.length == 2 and line.rotatable and not line.movable and line.collide
    assert center.shape.radius == 0.02 and not center.collide
    assert w.world.x_semidim is None and w.world.y_semidim is None
    assert all(o.shape == (3, 13) for o in w.reset())
    d = make_env("dispersion", num_envs=3, device="cpu")
    assert [f.name for f in d.world.landmarks] == [f"food_{i}" for i in range(4)]
    assert all(a.shape.radius == 0.035 and not a.collide and a.u_multiplier == 1.0 for a in d.agents)
    assert all(f.shape.radius == 0.05 and not f.collide for f in d.world.landmarks)
    assert all(o.shape == (3, 4 + 3 * 4) for o in d.reset())
    d = make_env("dispersion", num_envs=3, device="cpu", n_agents=2, n_food=5)
    assert all(o.shape == (3, 19) for o in d.reset())


# ---- the torch programs against the specs ----------------------------------------------------------------
@pytest.mark.parametrize("config", list(WHEEL_CONFIGS))
def test_wheel_torch_program_equals_the_spec(config):
    env = _placed("wheel", WHEEL_CONFIGS[config])
    spec = WS.WheelSpec(env)
    exp = spec.run()
    WS.assert_cases_fired(spec, exp)
    scn = env.scenario
    rewards = [scn.reward(a) for a in env.agents]
    obs = [scn.observation(a) for a in env.agents]
    assert torch.equal(scn.rew, exp["rew"]) and scn.rew.shape == (64, 1)
    for k in range(len(env.agents)):
        assert torch.equal(rewards[k], exp["rewards"][k]) and rewards[k] is not scn.rew
        assert torch.equal(obs[k], exp["obs"][k]), (obs[k] - exp["obs"][k]).abs().max()
    assert not scn.done().any()


def _dispersion_step(env):
    scn = env.scenario
    rewards = [scn.reward(a) for a in env.agents]  # (every reward before any observation)
    obs = [scn.observation(a) for a in env.agents]
    return rewards, obs, scn.done()


def _assert_dispersion_equals(env, spec, exp, got):
    rewards, obs, done = got
    for k in range(len(env.agents)):
        assert torch.equal(rewards[k], exp["rewards"][k]), k
        assert torch.equal(obs[k], exp["obs"][k]), k
    assert torch.equal(done, exp["done"])
    for l, f in enumerate(env.world.landmarks):  # noqa: E741
        assert torch.equal(f.eaten, spec.eaten[l]) and torch.equal(f.just_eaten, spec.just_eaten[l])
        assert torch.equal(f.is_rendering, spec.is_rendering[l])
        assert f.how_many_on_food.dtype is torch.int64 and torch.equal(f.how_many_on_food, exp["how_many"][l])
        assert f.anyone_on_food.dtype is torch.bool and torch.equal(f.anyone_on_food, exp["anyone"][l])


@pytest.mark.parametrize("config", list(DISPERSION_CONFIGS))
def test_dispersion_torch_program_equals_the_spec(config):
    env = _placed("dispersion", DISPERSION_CONFIGS[config])
    spec = DS.DispersionSpec(env)
    ptrs = [f.eaten.data_ptr() for f in env.world.landmarks]
    for what in ("placed", "again"):  # (the second evaluation sees the flags the first left)
        exp = spec.run()
        if what == "placed":
            DS.assert_cases_fired(spec, exp)
        _assert_dispersion_equals(env, spec, exp, _dispersion_step(env))
    assert [f.eaten.data_ptr() for f in env.world.landmarks] == ptrs  # written in place


# ---- resets --------------------------------------------------------------------------------------------
def _host_generator():
    g = torch.Generator()
    g.set_state(R.get_rng("cpu")[0][0])
    return g


def test_full_reset_draw_order():
    B = 9
    env = make_env("wheel", num_envs=B, device="cpu", seed=4)
    g = _host_generator()
    env.reset()
    for a in env.agents:
        assert torch.equal(a.state.pos, torch.zeros(B, 2).uniform_(-1.0, 1.0, generator=g))
        assert not a.state.vel.any()
    line, center = env.world.landmarks
    assert torch.equal(line.state.rot, torch.zeros(B, 1).uniform_(-math.pi / 2, math.pi / 2, generator=g))
    assert not line.state.pos.any() and not center.state.pos.any()
    assert torch.equal(_host_generator().get_state(), g.get_state())
    env = make_env("dispersion", num_envs=B, device="cpu", seed=4, pos_range=0.7)
    for f in env.world.landmarks:
        f.eaten[:] = True
        f.is_rendering[:] = False
    g = _host_generator()
    env.reset()
    for a in env.agents:
        assert not a.state.pos.any()
    for f in env.world.landmarks:
        assert torch.equal(f.state.pos, torch.zeros(B, 2).uniform_(-0.7, 0.7, generator=g))
        assert not f.eaten.any() and not f.just_eaten.any() and f.is_rendering.all()
    assert torch.equal(_host_generator().get_state(), g.get_state())


@pytest.mark.parametrize("name", ["wheel", "dispersion"])
def test_reset_at_leaves_the_other_rows_alone(name):
    env = _placed(name, dict(), B=16)
    env.step(env.get_random_actions())
    before = R.snapshot(env)
    env.reset_at(5)
    now = R.batched_state(env)
    others = torch.arange(16) != 5
    for k in now:
        assert torch.equal(now[k][others], before[k][others]), k
    if name == "dispersion":
        for f in env.world.landmarks:
            assert not f.eaten[5] and not f.just_eaten[5] and f.is_rendering[5]
        assert not any(a.state.pos[5].any() for a in env.agents)
        assert any(f.eaten.any() for f in env.world.landmarks)  # (the placed envs ate: something to leave alone)
    else:
        assert all(a.state.pos[5].abs().max() <= 1 and not a.state.vel[5].any() for a in env.agents)
        assert not env.scenario.line.state.ang_vel[5].any()


@pytest.mark.parametrize("name", ["wheel", "dispersion"])
def test_reset_where_rows_of_a_full_reset_cpu(name):
    B = 7
    for case, arg, mask in R.mask_cases(B):
        env, twin = R.twins(name, 2, B, "cpu")
        R.check_rows_of_full_reset(env, twin, arg, mask, "cpu", return_dones=True)
        R.check_next_step_agrees(env, twin, mask, "cpu")
        assert env.scenario.native_resets == 0, case  # (the generic path serves ``cpu`` worlds)


# ---- the host backend of the step programs -----------------------------------------------------------------
@pytest.mark.parametrize("config", list(WHEEL_CONFIGS))
def test_wheel_host_backend_against_the_torch_program(config):
    env = _placed("wheel", WHEEL_CONFIGS[config])
    scn = env.scenario
    rewards = [scn._torch_reward(a) for a in env.agents]
    rew = scn.rew
    obs = [scn._torch_observation(a) for a in env.agents]
    out = scn._run_fused(N.VMAS_SCN_REWARD | N.VMAS_SCN_OBS)
    assert torch.equal(scn.rew, rew) and scn.rew is out["rew"]
    # the four line-end columns in float64 from the same states: the allowance is twice the torch CPU
    # program's own worst deviation from that value (the factor 2: a second libm)
    rot = scn.line.state.rot.double()
    end = torch.cat([torch.cos(rot), torch.sin(rot)], dim=1) * (scn.line_length / 2)
    trig, exact = [6, 7, 8, 9], [0, 1, 2, 3, 4, 5, 10, 11, 12]
    bound = worst = 0.0
    for k, a in enumerate(env.agents):
        ref64 = torch.cat([end - a.state.pos.double(), -end - a.state.pos.double()], dim=1)
        bound = max(bound, float((obs[k][:, trig].double() - ref64).abs().max()))
        worst = max(worst, float((out["obs"][k][:, trig].double() - ref64).abs().max()))
        assert torch.equal(out["rewards"][k], rewards[k])
        assert torch.equal(out["obs"][k][:, exact], obs[k][:, exact])
    print(f"wheel line-end columns against fp64: allowance {2 * bound:.3e}, worst {worst:.3e}")
    assert bound > 0 and worst <= 2 * bound


@pytest.mark.parametrize("config", list(DISPERSION_CONFIGS))
def test_dispersion_host_backend_against_the_torch_program(config):
    ref, nat = (_placed("dispersion", DISPERSION_CONFIGS[config]) for _ in range(2))
    for what in ("placed", "again"):
        exp = _dispersion_step(ref)
        out = nat.scenario._run_fused(ALL)
        for k in range(len(ref.agents)):
            assert torch.equal(out["rewards"][k], exp[0][k]) and torch.equal(out["obs"][k], exp[1][k]), (what, k)
        assert torch.equal(out["done"], exp[2])
        assert all(torch.equal(x, y) for x, y in zip(DS.landmark_attributes(ref), DS.landmark_attributes(nat))), what
        # the parts alone, on the state the whole program left
        assert torch.equal(nat.scenario._run_fused(N.VMAS_SCN_DONE)["done"], exp[2])
        again = nat.scenario._run_fused(N.VMAS_SCN_OBS)["obs"]
        assert all(torch.equal(x, y) for x, y in zip(again, exp[1]))


# ---- the ABI ---------------------------------------------------------------------------------------------
def test_abi_version_is_16_on_both_sides():
    header = (ROOT / "include" / "vmas_mi355x.h").read_text()
    version = int(re.search(r"^#define VMAS_ABI_VERSION (\d+)$", header, re.M).group(1))
    assert " * v16:" in header and "vmas_uniform_reset" in header
    assert version >= 16 and N.VMAS_ABI_VERSION == version and N.load_library().vmas_abi_version() == version
    for name in ("vmas_wheel_outputs", "vmas_dispersion_outputs", "vmas_uniform_reset"):
        assert name in N.EXPORTED_SYMBOLS and N.fn_addr(name)


def test_v16_struct_layouts_match_header_compilation():
    probe = r'''
#include <stddef.h>
#include <stdio.h>
#include "vmas_mi355x.h"
#define O(T, f) offsetof(T, f)
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(VmasWheelIO), O(VmasWheelIO, half_length), O(VmasWheelIO, line_pos),
    O(VmasWheelIO, line_ang_vel), O(VmasWheelIO, pos), O(VmasWheelIO, vel), O(VmasWheelIO, rew), O(VmasWheelIO, obs),
    O(VmasWheelIO, out_delta), VMAS_WHEEL_MAX_AGENTS);
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(VmasDispersionIO), O(VmasDispersionIO, share_reward),
    O(VmasDispersionIO, pos), O(VmasDispersionIO, food_pos), O(VmasDispersionIO, thr), O(VmasDispersionIO, eaten),
    O(VmasDispersionIO, just_eaten), O(VmasDispersionIO, is_rendering), O(VmasDispersionIO, how_many), O(VmasDispersionIO, anyone),
    O(VmasDispersionIO, rewards), O(VmasDispersionIO, done), O(VmasDispersionIO, out_delta), VMAS_DISP_MAX_AGENTS,
    VMAS_DISP_MAX_FOOD);
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(VmasUniformResetIO), sizeof(VmasUniformDraw),
    sizeof(VmasUniformFixed), O(VmasUniformDraw, target), O(VmasUniformDraw, lo), O(VmasUniformFixed, x),
    O(VmasUniformResetIO, n_agents), O(VmasUniformResetIO, seed), O(VmasUniformResetIO, mask), O(VmasUniformResetIO, steps),
    O(VmasUniformResetIO, draws), O(VmasUniformResetIO, fixed), O(VmasUniformResetIO, force), O(VmasUniformResetIO, clear),
    O(VmasUniformResetIO, set), VMAS_URESET_MAX_DRAWS, VMAS_UDRAW_ROT);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = Path(d) / "probe.c"
        src.write_text(probe)
        exe = Path(d) / "probe"
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        lines = subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines()
    c = [list(map(int, line.split())) for line in lines]
    w, d, u = N.VmasWheelIO, N.VmasDispersionIO, N.VmasUniformResetIO
    assert c[0] == [ctypes.sizeof(w), w.half_length.offset, w.line_pos.offset, w.line_ang_vel.offset, w.pos.offset,
                    w.vel.offset, w.rew.offset, w.obs.offset, w.out_delta.offset, N.VMAS_WHEEL_MAX_AGENTS]
    assert c[1] == [ctypes.sizeof(d), d.share_reward.offset, d.pos.offset, d.food_pos.offset, d.thr.offset, d.eaten.offset,
                    d.just_eaten.offset, d.is_rendering.offset, d.how_many.offset, d.anyone.offset, d.rewards.offset,
                    d.done.offset, d.out_delta.offset, N.VMAS_DISP_MAX_AGENTS, N.VMAS_DISP_MAX_FOOD]
    dr, fx = N.VmasUniformDraw, N.VmasUniformFixed
    assert c[2] == [ctypes.sizeof(u), ctypes.sizeof(dr), ctypes.sizeof(fx), dr.target.offset, dr.lo.offset, fx.x.offset,
                    u.n_agents.offset, u.seed.offset, u.mask.offset, u.steps.offset, u.draws.offset, u.fixed.offset,
                    u.force.offset, u.clear.offset, u.set.offset, N.VMAS_URESET_MAX_DRAWS, N.VMAS_UDRAW_ROT]
    # (all three travel as kernel arguments, the reset block beside its two 16-byte draw grids)
    assert ctypes.sizeof(w) <= 4096 and ctypes.sizeof(d) <= 4096 and ctypes.sizeof(u) + 32 <= 4096
    assert (N.VMAS_WHEEL_MAX_AGENTS, N.VMAS_DISP_MAX_AGENTS, N.VMAS_DISP_MAX_FOOD) == (16, 16, 16)


def _buffers(keep):
    f, u8, i64 = (ctypes.c_float * 64)(), (ctypes.c_uint8 * 64)(), (ctypes.c_int64 * 64)()
    keep += [f, u8, i64]
    return ctypes.addressof(f), ctypes.addressof(u8), ctypes.addressof(i64)


def _vec(v, p, s0=2, s1=1):
    v.p, v.s0, v.s1 = p, s0, s1


def _valid_wheel_io(keep):
    fa, _, _ = _buffers(keep)
    io = N.VmasWheelIO()
    io.batch, io.n_agents, io.what = 4, 2, N.VMAS_SCN_REWARD | N.VMAS_SCN_OBS
    for v in (io.line_pos, io.line_rot, io.line_ang_vel):
        _vec(v, fa)
    io.rew = fa
    for a in range(2):
        _vec(io.pos[a], fa), _vec(io.vel[a], fa)
        io.rewards[a], io.obs[a] = fa, fa
    return io


def _valid_dispersion_io(keep):
    fa, ua, ia = _buffers(keep)
    io = N.VmasDispersionIO()
    io.batch, io.n_agents, io.n_food, io.what = 4, 2, 2, ALL
    for k in range(2):
        _vec(io.pos[k], fa), _vec(io.vel[k], fa), _vec(io.food_pos[k], fa)
        io.eaten[k], io.just_eaten[k], io.is_rendering[k], io.how_many[k], io.anyone[k] = ua, ua, ua, ia, ua
        io.rewards[k], io.obs[k] = fa, fa
    io.done = ua
    return io


def _valid_uniform_io(keep):
    fa, ua, _ = _buffers(keep)
    io = N.VmasUniformResetIO()
    io.batch, io.mode, io.n_draws, io.n_fixed, io.n_agents, io.n_clear, io.n_set = 4, 0, 2, 1, 1, 1, 1
    io.mask = ua
    _vec(io.draws[0].entity.pos, fa)
    io.draws[0].target, io.draws[0].call = N.VMAS_UDRAW_POS, 0
    _vec(io.draws[1].entity.pos, fa), _vec(io.draws[1].entity.rot, fa, 1, 0)
    io.draws[1].target, io.draws[1].call = N.VMAS_UDRAW_ROT, 1
    _vec(io.fixed[0].entity.pos, fa)
    io.clear[0], io.set[0] = ua, ua
    return io


def test_entry_points_refuse_bad_arguments_before_any_device():
    lib = N.load_library()
    keep = []
    inc = ctypes.c_uint64(0)

    def refused(fn, io, device=0):
        args = (device, ctypes.byref(io) if io is not None else None)
        rc = (fn(*args, ctypes.byref(inc), None) if fn is lib.vmas_uniform_reset else fn(*args, None))
        return rc == VMAS_E_INVALID and fn.__name__.encode() in lib.vmas_aux_last_error()

    def edits(make, fn, changes):
        assert refused(fn, None)
        for change in changes:
            io = make(keep)
            change(io)
            assert refused(fn, io), change
            assert refused(fn, io, device=-1), change  # (refused on the host path too)

    edits(_valid_wheel_io, lib.vmas_wheel_outputs, [
        lambda io: setattr(io, "batch", 0), lambda io: setattr(io, "n_agents", 0),
        lambda io: setattr(io, "n_agents", N.VMAS_WHEEL_MAX_AGENTS + 1), lambda io: setattr(io, "what", 0),
        lambda io: setattr(io, "rew", None), lambda io: setattr(io.line_rot, "p", None),
        lambda io: setattr(io.line_ang_vel, "p", None), lambda io: io.obs.__setitem__(1, None),
        lambda io: io.rewards.__setitem__(0, None), lambda io: setattr(io.vel[1], "p", None)])
    edits(_valid_dispersion_io, lib.vmas_dispersion_outputs, [
        lambda io: setattr(io, "batch", -2), lambda io: setattr(io, "n_agents", N.VMAS_DISP_MAX_AGENTS + 1),
        lambda io: setattr(io, "n_food", 0), lambda io: setattr(io, "n_food", N.VMAS_DISP_MAX_FOOD + 1),
        lambda io: setattr(io, "what", 0), lambda io: setattr(io, "done", None),
        lambda io: io.eaten.__setitem__(1, None), lambda io: io.just_eaten.__setitem__(0, None),
        lambda io: io.how_many.__setitem__(1, None), lambda io: io.anyone.__setitem__(0, None),
        lambda io: io.rewards.__setitem__(1, None), lambda io: io.obs.__setitem__(0, None),
        lambda io: setattr(io.pos[1], "p", None), lambda io: setattr(io.food_pos[0], "p", None)])
    # (a NULL is_rendering row is allowed: the tensor need not exist)
    edits(_valid_uniform_io, lib.vmas_uniform_reset, [
        lambda io: setattr(io, "batch", 0), lambda io: setattr(io, "batch", 1 << 30), lambda io: setattr(io, "mode", 4),
        lambda io: setattr(io, "n_draws", N.VMAS_URESET_MAX_DRAWS + 1),
        lambda io: setattr(io, "n_fixed", N.VMAS_URESET_MAX_FIXED + 1),
        lambda io: setattr(io, "n_agents", N.VMAS_URESET_MAX_AGENTS + 1),
        lambda io: setattr(io, "n_clear", N.VMAS_URESET_MAX_CLEAR + 1), lambda io: setattr(io, "n_set", -1),
        lambda io: setattr(io, "mask", None), lambda io: setattr(io.draws[1], "call", 0),
        lambda io: setattr(io.draws[0], "target", 2), lambda io: setattr(io.draws[0].entity.pos, "p", None),
        lambda io: setattr(io.draws[1].entity.rot, "p", None), lambda io: setattr(io.fixed[0].entity.pos, "p", None),
        lambda io: io.clear.__setitem__(0, None), lambda io: io.set.__setitem__(0, None)])
    assert refused(lib.vmas_uniform_reset, _valid_uniform_io(keep), device=-1)  # (the draws are a device path only)
    assert inc.value == 0
    # the host path refuses direct outputs
    for make, fn in ((_valid_wheel_io, lib.vmas_wheel_outputs), (_valid_dispersion_io, lib.vmas_dispersion_outputs)):
        io = make(keep)
        io.out_delta = _buffers(keep)[2]
        assert refused(fn, io, device=-1)


# ---- physics parity on the host backend ---------------------------------------------------------------------
def place_agents_on_the_line(env):
    """In every even env: the agents within 0.05 of the line (0.04 off it, along its length), so that
    sphere-line contact against the rotate-only body occurs."""
    line = env.scenario.line
    rot = line.state.rot
    along = torch.cat([torch.cos(rot), torch.sin(rot)], dim=1)
    across = torch.cat([-torch.sin(rot), torch.cos(rot)], dim=1)
    even = (torch.arange(env.num_envs, device=rot.device) % 2 == 0).unsqueeze(-1)
    for k, a in enumerate(env.agents):
        spot = along * (-0.6 + 0.4 * k) + across * (0.04 if k % 2 == 0 else -0.04)
        a.set_pos(torch.where(even, spot, a.state.pos), batch_index=None)


@pytest.mark.parametrize("name", ["wheel", "dispersion"])
def test_step_parity_host(name):
    env = make_env(name, num_envs=48, device="cpu", seed=2)
    if name == "wheel":
        place_agents_on_the_line(env)
    reps = step_parity(env, 4)
    assert all(r["ok"] for r in reps), reps
    if name == "wheel":
        line = env.scenario.line.state
        assert line.ang_vel.abs().max() > 0 and not line.pos.any()  # (it turns, it never translates)


# ---- rendering -----------------------------------------------------------------------------------------
def test_wheel_line_is_drawn_rotated_about_the_origin():
    from tests.test_render import pixel_of, shared_bounds

    env = make_env("wheel", num_envs=2, device="cpu", seed=0)
    for a in env.agents:  # (out of the probes' way)
        a.set_pos(torch.tensor([[0.6, 0.6], [0.6, 0.6]]), batch_index=None)
    W, H = env.scenario.viewer_size
    frames = {}
    for rot in (0.0, math.pi / 2):
        env.scenario.line.set_rot(torch.full((2, 1), rot), batch_index=None)
        frames[rot] = env.render(mode="rgb_array", env_index=1)
    bounds = shared_bounds(env, 1)
    on_x, on_y = pixel_of(bounds, 0.5, 0.0, W, H), pixel_of(bounds, 0.0, 0.5, W, H)
    black, white = (38, 38, 38), (255, 255, 255)  # (Color.BLACK is 0.15 grey)
    assert not np.array_equal(frames[0.0], frames[math.pi / 2])
    assert tuple(frames[0.0][on_x]) == black and tuple(frames[0.0][on_y]) == white
    assert tuple(frames[math.pi / 2][on_x]) == white and tuple(frames[math.pi / 2][on_y]) == black


def test_an_eaten_food_is_not_drawn():
    from tests.test_render import pixel_of, shared_bounds

    env = _placed("dispersion", dict(), B=16)
    b = DS.CASE_ENVS["just_inside"]
    W, H = env.scenario.viewer_size
    food = env.world.landmarks[0]
    # food 0 lies at the origin, agent 0 covers x in [0.05, 0.12]: the probe sees the food alone
    i, j = pixel_of(shared_bounds(env, b), -0.02, 0.0, W, H)
    before = env.render(mode="rgb_array", env_index=b)
    before_batch = env.render_batch(size=(W, H))[b].numpy()
    assert tuple(before[i, j]) != (255, 255, 255) and tuple(before_batch[i, j]) != (255, 255, 255)
    _dispersion_step(env)
    assert food.eaten[b] and not food.is_rendering[b]
    after = env.render(mode="rgb_array", env_index=b)
    after_batch = env.render_batch(size=(W, H))[b].numpy()
    assert tuple(after[i, j]) == (255, 255, 255) and tuple(after_batch[i, j]) == (255, 255, 255)
