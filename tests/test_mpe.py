"""MPE simple_spread and simple_tag without a GPU: construction, the torch programs against the
restatement of tests/_mpe_spec.py on hand-placed and random envs, the resets' draw order, reset_at /
reset_where on ``cpu``, respawn_at_catch, the host backend (device -1) of the step program, the v17
argument block and entry point, physics parity on the host backend and rendering."""
import ctypes
import itertools
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import _mpe_spec as MS
from tests import _reset_where as R
from tests._parity import step_parity
from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd import make_env

ROOT = Path(__file__).resolve().parent.parent
VMAS_E_INVALID = -1
BOTH = N.VMAS_SCN_REWARD | N.VMAS_SCN_OBS

CONFIGS = {
    "spread_1": ("simple_spread", dict(n_agents=1)),
    "spread_3": ("simple_spread", dict()),
    "spread_5": ("simple_spread", dict(n_agents=5)),
    "spread_3_blind": ("simple_spread", dict(obs_agents=False)),
    "tag_default": ("simple_tag", dict()),
    "tag_two_good_flipped": ("simple_tag", dict(num_good_agents=2, agents_share_rew=True, adversaries_share_rew=False)),
    "tag_shaped": ("simple_tag", dict(num_good_agents=2, shape_agent_rew=True, shape_adversary_rew=True)),
    "tag_shaped_shared": ("simple_tag", dict(num_good_agents=2, shape_agent_rew=True, shape_adversary_rew=True,
                                             agents_share_rew=True)),
    "tag_eight_shaped": ("simple_tag", dict(num_good_agents=3, num_adversaries=5, shape_agent_rew=True,
                                            shape_adversary_rew=True, agents_share_rew=True)),
    "tag_blind": ("simple_tag", dict(num_good_agents=2, observe_same_team=False, observe_pos=False)),
}


def task_of(name):
    return "spread" if name == "simple_spread" else "tag"


def placed(config, B=64, seed=1, steps=2, device="cpu", **extra):
    """An env of the configuration after a few random steps (velocities, random rows) with the 16
    hand-placed envs written over its first rows."""
    name, kw = CONFIGS[config]
    env = make_env(name, num_envs=B, device=device, seed=seed, **kw, **extra)
    for _ in range(steps):
        env.step(env.get_random_actions())
    (MS.place_spread_cases if name == "simple_spread" else MS.place_tag_cases)(env)
    return env


def spec_of(env, config):
    task = task_of(CONFIGS[config][0])
    spec = MS.MpeSpec(env, task)
    exp = spec.run()
    (MS.assert_spread_cases_fired if task == "spread" else MS.assert_tag_cases_fired)(spec, exp)
    return task, spec, exp


# ---- construction ------------------------------------------------------------------------------------
def test_make_env_builds_both_and_rejects_unknown_kwargs():
    s = make_env("simple_spread", num_envs=3, device="cpu", n_agents=4, obs_agents=False)
    t = make_env("simple_tag", num_envs=3, device="cpu", num_good_agents=2, num_adversaries=4, num_landmarks=3,
                 shape_agent_rew=True, shape_adversary_rew=True, agents_share_rew=True, adversaries_share_rew=False,
                 observe_same_team=False, observe_pos=False, observe_vel=False, bound=1.5, respawn_at_catch=True)
    assert len(s.agents) == 4 and len(s.world.landmarks) == 4
    assert len(t.agents) == 6 and len(t.world.landmarks) == 3 and t.world.x_semidim == t.world.y_semidim == 1.5
    for name in ("simple_spread", "simple_tag"):
        # (ScenarioUtils.check_kwargs_consumed: a warning today, as in the reference)
        with pytest.warns(UserWarning, match="no_such_kwarg"):
            make_env(name, num_envs=3, device="cpu", no_such_kwarg=1)


def test_entities_world_arguments_and_observation_widths():
    s = make_env("simple_spread", num_envs=3, device="cpu")
    assert [a.name for a in s.agents] == [f"agent_{i}" for i in range(3)]
    assert [m.name for m in s.world.landmarks] == [f"landmark {i}" for i in range(3)]
    assert all(a.shape.radius == 0.15 and a.collide and a.u_multiplier == 1.0 and a.max_speed is None for a in s.agents)
    assert all(not m.collide and m.shape.radius == 0.05 for m in s.world.landmarks)
    assert s.world.x_semidim is None and s.world._substeps == 1
    for A in (1, 3, 5):
        for obs_agents in (True, False):
            e = make_env("simple_spread", num_envs=3, device="cpu", n_agents=A, obs_agents=obs_agents)
            assert all(o.shape == (3, 4 + 2 * A + (2 * (A - 1) if obs_agents else 0)) for o in e.reset())
    t = make_env("simple_tag", num_envs=3, device="cpu")
    assert [a.name for a in t.agents] == ["adversary_0", "adversary_1", "adversary_2", "agent_0"]
    assert [a.adversary for a in t.agents] == [True, True, True, False]
    for a in t.agents:
        want = (0.075, 3.0, 1.0) if a.adversary else (0.05, 4.0, 1.3)
        assert (a.shape.radius, a.u_multiplier, a.max_speed) == want and a.collide
    assert all(m.shape.radius == 0.2 and m.collide and m.name == f"landmark {i}" for i, m in enumerate(t.world.landmarks))
    w = t.world
    assert (w._substeps, w._collision_force, w.x_semidim, w.y_semidim) == (10, 500, 1.0, 1.0)
    assert [o.shape[1] for o in t.reset()] == [16, 16, 16, 14]


@pytest.mark.parametrize("vel,pos,team", list(itertools.product((True, False), repeat=3)))
def test_tag_observation_widths_for_every_flag_combination(vel, pos, team):
    G, A, L = 2, 3, 2
    env = make_env("simple_tag", num_envs=2, device="cpu", num_good_agents=G, num_adversaries=A, num_landmarks=L,
                   observe_vel=vel, observe_pos=pos, observe_same_team=team)
    own = 2 * vel + 2 * pos + 2 * L
    adv = own + 2 * G + 2 * G + (2 * (A - 1) if team else 0)           # good agents' positions and velocities
    good = own + 2 * A + ((2 + 2) * (G - 1) if team else 0)           # adversaries' positions only
    assert [o.shape[1] for o in env.reset()] == [adv] * A + [good] * G


# ---- the torch programs against the spec -------------------------------------------------------------------
def run_program(env, torch_program=True):
    scn = env.scenario
    rew, obs = (scn._torch_reward, scn._torch_observation) if torch_program else (scn.reward, scn.observation)
    rewards = [rew(a) for a in env.agents]  # (every reward before any observation, as the environment asks)
    return rewards, [obs(a) for a in env.agents]


def assert_equals_spec(env, task, exp, got, bitwise_team_sums):
    rewards, obs = got
    n = len(env.agents)
    for k in range(n):
        assert torch.equal(obs[k].cpu(), exp["obs"][k]), k
    have, want = MS.scenario_tensors(env, task), MS.expected_scenario_tensors(exp, task)
    if task == "spread":
        assert torch.equal(have[0].cpu(), want[0])
        assert all(torch.equal(r.cpu(), exp["rewards"][k]) for k, r in enumerate(rewards))
        return
    per, per_want = [t.cpu() for t in have[2:]], want[2:]
    for k in range(n):
        assert torch.equal(per[k], per_want[k]), k  # Agent.rew: bitwise
    teams = {False: [k for k, a in enumerate(env.agents) if not a.adversary],
             True: [k for k, a in enumerate(env.agents) if a.adversary]}
    for t_have, t_want, adv in ((have[0].cpu(), want[0], False), (have[1].cpu(), want[1], True)):
        if bitwise_team_sums:
            assert torch.equal(t_have, t_want), "team sum"
        for b in range(t_have.shape[0]):  # any summation order is within this bound of the exact sum
            assert MS.fsum_bound_ok(t_have[b], [per[k][b] for k in teams[adv]]), (adv, b)
    scn = env.scenario
    for k, a in enumerate(env.agents):
        share = scn.adversaries_share_rew if a.adversary else scn.agents_share_rew
        assert torch.equal(rewards[k].cpu(), (have[1] if a.adversary else have[0]).cpu() if share else per[k]), k


@pytest.mark.parametrize("config", list(CONFIGS))
def test_torch_program_equals_the_spec(config):
    env = placed(config)
    task, spec, exp = spec_of(env, config)
    shaped = task == "tag" and (spec.shape_agent_rew or spec.shape_adversary_rew)
    # unshaped tag rewards are multiples of 10: every order sums them exactly
    assert_equals_spec(env, task, exp, run_program(env), bitwise_team_sums=not shaped)


def test_two_overlapping_pairs_count_twice_each():
    env = placed("spread_5")
    b = MS.SPREAD_CASES["two_pairs"][0]
    env.scenario._torch_reward(env.agents[0])
    assert env.scenario.rew[b] == -4.0  # closest = 0 for every landmark; (0,1), (1,0), (1,2), (2,1)
    b = MS.SPREAD_CASES["tie"][0]
    assert env.scenario.rew[b] == -(5 * 5 * 0.5)


def test_torch_program_never_indexes_by_a_mask():
    """No host wait: the rewards, and the respawn of respawn_at_catch in envs that hold a catch, are
    built from whole-tensor operations -- no nonzero, no indexed write, no scalar read in the
    dispatched operations."""
    import torch.utils._python_dispatch as D

    for config, extra in (("spread_3", {}), ("tag_shaped", {}), ("tag_default", dict(respawn_at_catch=True))):
        env = placed(config, B=16, **extra)
        if extra:  # (the hand-placed catches are there for the respawn to act on)
            scn = env.scenario
            assert any(bool(scn.is_collision(scn.good_agents()[0], adv).any()) for adv in scn.adversaries())

        class NoSync(D.TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                name = str(func)
                assert "nonzero" not in name and "index_put" not in name and "_local_scalar_dense" not in name, name
                return func(*args, **(kwargs or {}))

        with NoSync():
            run_program(env)


# ---- resets --------------------------------------------------------------------------------------------
def _host_generator():
    g = torch.Generator()
    g.set_state(R.get_rng("cpu")[0][0])
    return g


@pytest.mark.parametrize("name,kw,bound", [("simple_spread", dict(n_agents=4), None), ("simple_tag", dict(bound=1.3), 1.3),
                                           ("simple_tag", dict(), 1.0)])
def test_full_reset_draw_order(name, kw, bound):
    B = 9
    env = make_env(name, num_envs=B, device="cpu", seed=4, **kw)
    g = _host_generator()
    env.reset()
    outer = 1.0 if bound is None else bound
    inner = 1.0 if bound is None else bound - 0.1  # (a Python double, as the reference computes it)
    for e in env.agents:
        assert torch.equal(e.state.pos, torch.zeros(B, 2).uniform_(-outer, outer, generator=g)), e.name
        assert not e.state.vel.any()
    for e in env.world.landmarks:
        assert torch.equal(e.state.pos, torch.zeros(B, 2).uniform_(-inner, inner, generator=g)), e.name
    assert torch.equal(_host_generator().get_state(), g.get_state())


@pytest.mark.parametrize("config", ["spread_3", "tag_default"])
def test_reset_at_leaves_the_other_rows_alone(config):
    env = placed(config, B=16)
    env.step(env.get_random_actions())
    before = R.snapshot(env)
    env.reset_at(5)
    now = R.batched_state(env)
    others = torch.arange(16) != 5
    changed = False
    for k in now:
        assert torch.equal(now[k][others], before[k][others]), k
        changed = changed or not torch.equal(now[k][5], before[k][5])
    assert changed and all(not a.state.vel[5].any() for a in env.agents)


@pytest.mark.parametrize("name", ["simple_spread", "simple_tag"])
def test_reset_where_rows_of_a_full_reset_cpu(name):
    B = 7
    for case, arg, mask in R.mask_cases(B):
        env, twin = R.twins(name, 2, B, "cpu")
        R.check_rows_of_full_reset(env, twin, arg, mask, "cpu", return_dones=True)
        R.check_next_step_agrees(env, twin, mask, "cpu")
        assert env.scenario.native_resets == 0, case  # (the generic path serves ``cpu`` worlds)


def _global_generator_twin(seed):
    """Seeds torch's global CPU generator (what a direct call of the scenario draws from) and returns a
    generator in the same state."""
    torch.manual_seed(seed)
    g = torch.Generator()
    g.set_state(torch.get_rng_state())
    return g


def test_respawn_at_catch_moves_only_the_caught_agent():
    B = 16
    env = placed("tag_default", B=B, respawn_at_catch=True)
    twin = placed("tag_default", B=B, respawn_at_catch=True)
    scn = env.scenario
    caught_env = MS.TAG_CASES["one_catch"][0]
    good = scn.good_agents()[0]
    good.state.vel[:] = 0.5
    before = {a.name: (a.state.pos.clone(), a.state.vel.clone()) for a in env.agents}
    # the catches of the hand-placed envs (one per env in which an adversary holds the good agent)
    want_caught = torch.zeros(B, dtype=torch.bool)
    for adv in scn.adversaries():
        want_caught |= scn.is_collision(good, adv)
    assert want_caught[caught_env] and not want_caught[MS.TAG_CASES["far"][0]] and not want_caught[MS.TAG_CASES["thr_at"][0]]
    g = _global_generator_twin(5)
    scn._torch_reward(env.agents[0])
    draws = [torch.zeros(B, 2).uniform_(-1.0, 1.0, generator=g) for _ in scn.adversaries()]  # a full-batch draw per pair
    assert torch.equal(torch.get_rng_state(), g.get_state())
    for a in scn.adversaries():
        assert torch.equal(a.state.pos, before[a.name][0]) and torch.equal(a.state.vel, before[a.name][1])
    moved = (good.state.pos != before[good.name][0]).any(-1)
    assert torch.equal(moved, want_caught)
    assert torch.equal(good.state.vel[~want_caught], before[good.name][1][~want_caught])
    assert not good.state.vel[want_caught].any()
    assert any(torch.equal(good.state.pos[caught_env], d[caught_env]) for d in draws)
    # nothing caught: the generator advances by the same draws
    for a in twin.scenario.adversaries():
        a.set_pos(torch.full((B, 2), 5.0), batch_index=None)
    g = _global_generator_twin(6)
    pos = twin.scenario.good_agents()[0].state.pos.clone()
    twin.scenario._torch_reward(twin.agents[0])
    for _ in twin.scenario.adversaries():
        torch.zeros(B, 2).uniform_(-1.0, 1.0, generator=g)
    assert torch.equal(torch.get_rng_state(), g.get_state())
    assert torch.equal(twin.scenario.good_agents()[0].state.pos, pos)


# ---- the host backend of the step program ------------------------------------------------------------------
# (The team sums follow the order probed for the world's device.  ATen's CPU reduction of five values is
# none of the device's forms, so the eight-agent shaped configuration is compared on the GPU only; its
# unshaped sums, multiples of 10, would be exact in any order.)
@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("config", [c for c in CONFIGS if c != "tag_eight_shaped"])
def test_host_backend_against_the_torch_program(config, B):
    ref, nat = (placed(config, B=B) for _ in range(2))
    task = task_of(CONFIGS[config][0])
    rewards, obs = run_program(ref)
    n0 = nat.scenario.native_launches
    out = nat.scenario._run_fused(BOTH)
    assert nat.scenario.native_launches == n0 + 1
    for k in range(len(ref.agents)):
        assert torch.equal(out["rewards"][k], rewards[k]), k
        assert torch.equal(out["obs"][k], obs[k]), k
    for x, y in zip(MS.scenario_tensors(ref, task), MS.scenario_tensors(nat, task)):
        assert torch.equal(x, y)
    again = nat.scenario._run_fused(N.VMAS_SCN_OBS)["obs"]  # the observation part alone
    assert all(torch.equal(x, y) for x, y in zip(again, obs))


def test_host_backend_reads_both_strides():
    ref, nat = (placed("spread_3", B=65) for _ in range(2))
    for env in (ref, nat):
        for e in env.world.entities:
            buf = torch.zeros(65, 4)
            buf[:, ::2] = e.state.pos
            e.state.pos = buf[:, ::2]
            assert not e.state.pos.is_contiguous()
    rewards, obs = run_program(ref)
    out = nat.scenario._run_fused(BOTH)
    assert all(torch.equal(x, y) for x, y in zip(out["rewards"] + out["obs"], rewards + obs))


# ---- the ABI ---------------------------------------------------------------------------------------------
def test_abi_version_is_17_on_both_sides():
    header = (ROOT / "include" / "vmas_mi355x.h").read_text()
    version = int(re.search(r"^#define VMAS_ABI_VERSION (\d+)$", header, re.M).group(1))
    assert " * v17:" in header and "vmas_mpe_outputs" in header
    assert version >= 17 and N.VMAS_ABI_VERSION == version and N.load_library().vmas_abi_version() == version
    assert "vmas_mpe_outputs" in N.EXPORTED_SYMBOLS and N.fn_addr("vmas_mpe_outputs")


def test_v17_struct_layout_matches_header_compilation():
    fields = ["task", "collide_mask", "out_delta", "pos", "vel", "landmark_pos", "n_terms", "terms", "radius",
              "adversary_mask", "shape_agent_rew", "adversaries_share_rew", "sum_mode_good", "sum_mode_adv", "thr",
              "rewards", "rew", "agent_rew", "agents_rew", "adverary_rew", "obs"]
    prints = "\n".join(f'  printf("%zu\\n", offsetof(VmasMpeIO, {f}));' for f in fields)
    probe = r'''
#include <stddef.h>
#include <stdio.h>
#include "vmas_mi355x.h"
int main(void) {
  printf("%zu %zu %zu %d %d %d\n", sizeof(VmasMpeIO), sizeof(VmasMpeTerm), offsetof(VmasMpeTerm, index),
         VMAS_MPE_MAX_AGENTS, VMAS_MPE_MAX_LANDMARKS, VMAS_MPE_MAX_TERMS);
  printf("%d %d %d %d %d %d %d\n", VMAS_MPE_SPREAD, VMAS_MPE_TAG, VMAS_MPE_SELF_VEL, VMAS_MPE_SELF_POS,
         VMAS_MPE_REL_LANDMARK, VMAS_MPE_REL_AGENT, VMAS_MPE_AGENT_VEL);
''' + prints + "\n  return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        src = Path(d) / "probe.c"
        src.write_text(probe)
        exe = Path(d) / "probe"
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        lines = subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines()
    c = [list(map(int, line.split())) for line in lines]
    io = N.VmasMpeIO
    assert c[0] == [ctypes.sizeof(io), ctypes.sizeof(N.VmasMpeTerm), N.VmasMpeTerm.index.offset, N.VMAS_MPE_MAX_AGENTS,
                    N.VMAS_MPE_MAX_LANDMARKS, N.VMAS_MPE_MAX_TERMS]
    assert c[1] == [N.VMAS_MPE_SPREAD, N.VMAS_MPE_TAG, N.VMAS_MPE_SELF_VEL, N.VMAS_MPE_SELF_POS, N.VMAS_MPE_REL_LANDMARK,
                    N.VMAS_MPE_REL_AGENT, N.VMAS_MPE_AGENT_VEL]
    assert [row[0] for row in c[2:]] == [getattr(io, f).offset for f in fields]
    assert ctypes.sizeof(io) + 8 <= 4096  # (it travels as a kernel argument, beside one int)
    assert (N.VMAS_MPE_MAX_AGENTS, N.VMAS_MPE_MAX_LANDMARKS) == (8, 8)


def _valid_io(keep, task):
    f = (ctypes.c_float * 256)()
    keep.append(f)
    fa = ctypes.addressof(f)
    io = N.VmasMpeIO()
    io.batch, io.n_agents, io.n_landmarks, io.what, io.task = 4, 2, 2, BOTH, task
    for k in range(2):
        for v in (io.pos[k], io.vel[k], io.landmark_pos[k]):
            v.p, v.s0, v.s1 = fa, 2, 1
        io.n_terms[k] = 2
        io.terms[k][0].kind, io.terms[k][1].kind, io.terms[k][1].index = N.VMAS_MPE_SELF_POS, N.VMAS_MPE_REL_AGENT, 1 - k
        io.rewards[k], io.agent_rew[k], io.obs[k] = fa, fa, fa
    io.rew, io.agents_rew, io.adverary_rew = fa, fa, fa
    io.adversary_mask, io.sum_mode_good, io.sum_mode_adv = 1, 1, 1
    return io


def test_entry_point_refuses_bad_arguments_before_any_device():
    lib = N.load_library()
    keep = []

    def refused(io, device=0):
        rc = lib.vmas_mpe_outputs(device, ctypes.byref(io) if io is not None else None, None)
        return rc == VMAS_E_INVALID and b"vmas_mpe_outputs" in lib.vmas_aux_last_error()

    assert refused(None)
    common = [
        lambda io: setattr(io, "batch", 0), lambda io: setattr(io, "n_agents", 0),
        lambda io: setattr(io, "n_agents", N.VMAS_MPE_MAX_AGENTS + 1),
        lambda io: setattr(io, "n_landmarks", N.VMAS_MPE_MAX_LANDMARKS + 1), lambda io: setattr(io, "n_landmarks", -1),
        lambda io: setattr(io, "what", 0), lambda io: setattr(io, "what", N.VMAS_SCN_DONE),
        lambda io: setattr(io, "task", 0), lambda io: setattr(io, "task", 3),
        lambda io: setattr(io.pos[1], "p", None), lambda io: setattr(io.vel[0], "p", None),
        lambda io: setattr(io.landmark_pos[1], "p", None), lambda io: io.rewards.__setitem__(1, None),
        lambda io: io.obs.__setitem__(0, None), lambda io: io.n_terms.__setitem__(0, 0),
        lambda io: io.n_terms.__setitem__(1, N.VMAS_MPE_MAX_TERMS + 1), lambda io: setattr(io.terms[0][0], "kind", 5),
        lambda io: setattr(io.terms[0][1], "index", 2),
        lambda io: (setattr(io.terms[1][0], "kind", N.VMAS_MPE_REL_LANDMARK), setattr(io.terms[1][0], "index", 2)),
    ]
    per_task = {
        N.VMAS_MPE_SPREAD: [lambda io: setattr(io, "rew", None)],
        N.VMAS_MPE_TAG: [lambda io: setattr(io, "agents_rew", None), lambda io: setattr(io, "adverary_rew", None),
                         lambda io: io.agent_rew.__setitem__(1, None), lambda io: setattr(io, "adversary_mask", 0),
                         lambda io: setattr(io, "adversary_mask", 3), lambda io: setattr(io, "sum_mode_good", 0),
                         lambda io: setattr(io, "sum_mode_adv", 3), lambda io: setattr(io, "sum_mode_adv", 16)],
    }
    for task, extra in per_task.items():
        for device in (0, -1):
            for change in common + extra:
                io = _valid_io(keep, task)
                change(io)
                assert refused(io, device), (task, device, change)
        io = _valid_io(keep, task)  # the host path refuses direct outputs
        delta = (ctypes.c_int64 * 3)()
        keep.append(delta)
        io.out_delta = ctypes.addressof(delta)
        assert refused(io, device=-1)
        assert lib.vmas_mpe_outputs(-1, ctypes.byref(_valid_io(keep, task)), None) == 0  # (the block itself is valid)


# ---- physics parity on the host backend ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["simple_spread", "simple_tag"])
def test_step_parity_host(name):
    env = make_env(name, num_envs=64, device="cpu", seed=2)
    (MS.place_spread_cases if name == "simple_spread" else MS.place_tag_cases)(env)  # (contacts from the first step)
    reps = step_parity(env, 4)
    assert all(r["ok"] for r in reps), reps


# ---- rendering -----------------------------------------------------------------------------------------
def test_tag_perimeter_is_drawn():
    from tests.test_render import pixel_of, shared_bounds

    env = make_env("simple_tag", num_envs=2, device="cpu", seed=0)
    far = torch.full((2, 2), 0.0)
    for k, e in enumerate(env.world.entities):  # (everything near the centre: out of the probes' way)
        e.set_pos(far + 0.3 * torch.tensor([np.cos(k), np.sin(k)], dtype=torch.float32), batch_index=None)
    geoms = env.scenario.extra_render(1)
    assert len(geoms) == 4
    W, H = env.scenario.viewer_size
    frame = env.render(mode="rgb_array", env_index=1)
    bounds = shared_bounds(env, 1)
    edge = 1.0 + 0.075
    black, white = (38, 38, 38), (255, 255, 255)  # (Color.BLACK is 0.15 grey)
    for x, y in ((edge, 0.5), (-edge, -0.5), (0.5, edge), (-0.5, -edge)):
        i, j = pixel_of(bounds, x, y, W, H)
        patch = frame[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2].reshape(-1, 3)
        assert any(tuple(p) == black for p in patch), (x, y)
    i, j = pixel_of(bounds, 0.8, 0.8, W, H)
    assert tuple(frame[i, j]) == white
    batch = env.render_batch(size=(W, H))
    assert batch.shape[0] == 2 and (batch[1].numpy() != 255).any()


def test_spread_frame_has_a_disc_per_agent_and_landmark():
    from tests.test_render import pixel_of, shared_bounds

    A = 3
    env = make_env("simple_spread", num_envs=2, device="cpu", seed=0)
    spots = [(-0.8 + 0.8 * k, 0.5) for k in range(A)] + [(-0.8 + 0.8 * k, -0.5) for k in range(A)]
    for e, (x, y) in zip(env.world.entities, spots):
        e.set_pos(torch.tensor([[x, y], [x, y]]), batch_index=None)
    W, H = env.scenario.viewer_size
    frame = env.render(mode="rgb_array", env_index=0)
    batch = env.render_batch(size=(W, H))[0].numpy()
    bounds = shared_bounds(env, 0)
    white = (255, 255, 255)
    colours = []
    for x, y in spots:
        i, j = pixel_of(bounds, x, y, W, H)
        assert tuple(frame[i, j]) != white and tuple(batch[i, j]) != white, (x, y)
        colours.append(tuple(frame[i, j]))
    assert len(set(colours[:A])) == 1 and len(set(colours[A:])) == 1 and colours[0] != colours[A]
    for x, y in ((-0.4, 0.0), (0.4, 0.0)):  # between the rows: background
        i, j = pixel_of(bounds, x, y, W, H)
        assert tuple(frame[i, j]) == white
