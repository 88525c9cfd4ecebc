"""The navigation scenario's fused program (csrc/vmas_scenarios.hip k_navigation /
k_navigation_fast) on gfx950: bit-identical to the scenario's torch program eagerly and replayed
from a HIP graph, the fast LIDAR within the LIDAR tolerance, the torch fallback over the agent cap,
discrete actions in graph mode, and the entry point's argument checks.  130 envs: two full waves
plus a partial one."""
import ctypes

import pytest
import torch

from tests._navigation_spec import place_cases, scenario_attributes
from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd import make_env
from vectorizedmultiagentsimulator_amd.simulator import _fused

from test_fused import _NullCtx, _Torch
from test_graph import _assert_same, _rng_load, _rng_save, _state

B = 130

CASES = {
    "default": dict(),
    "one_agent": dict(n_agents=1),
    # the runtime ray form, more than seven LIDAR targets, colours drawn by torch.randn
    "nine_agents_five_rays": dict(n_agents=9, n_lidar_rays=5),
    "shared_goals_no_lidar": dict(collisions=False, agents_with_same_goal=2),
    "all_goals_own_rewards_bounds": dict(observe_all_goals=True, shared_rew=False, enforce_bounds=True),
}


def _attrs(env):
    out = scenario_attributes(env)
    for a in env.agents:
        out += [s._last_measurement for s in (a.sensors or ())]
    return out


def _mode_envs(gpu_device, modes, num_envs, seed=3, **kw):
    """One env per mode (torch: the torch program; fused: eager; graph: replayed), the same seed
    and generator states."""
    envs = {}
    for mode in modes:
        saved = _rng_save()
        with _Torch() if mode == "torch" else _NullCtx():
            envs[mode] = make_env("navigation", num_envs=num_envs, device=gpu_device, seed=seed,
                                  graph_step=mode == "graph", **kw)
        if mode != modes[-1]:
            _rng_load(saved)
    return envs


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_fused_program_matches_torch_program_gpu(gpu_device, monkeypatch, case):
    monkeypatch.setattr(_fused, "EXACT_LIDAR", True)  # (LIDAR bit-identical to World.cast_rays)
    kw = CASES[case]
    envs = _mode_envs(gpu_device, ("torch", "fused", "graph"), B, **kw)
    ref = envs["torch"]
    for t in range(12):
        actions = ref.get_random_actions()
        outs = {}
        for mode, env in envs.items():
            s = _rng_save()
            with _Torch() if mode == "torch" else _NullCtx():
                if t == 2:
                    place_cases(env)
                if t == 5:
                    env.reset_at(7)
                if t == 9:
                    env.reset()
                outs[mode] = env.step([a.clone() for a in actions])
            if mode != "graph":
                _rng_load(s)
        for mode in ("fused", "graph"):
            _assert_same(outs["torch"], outs[mode], f"{case} {mode} outputs step {t}")
            _assert_same(_state(ref), _state(envs[mode]), f"{case} {mode} state step {t}")
            _assert_same(_attrs(ref), _attrs(envs[mode]), f"{case} {mode} attributes step {t}")
        if t == 2:  # the hand-placed envs reach the program: all goals reached, done without them
            info = outs["torch"][3]
            assert (info[0]["final_rew"] != 0).any()
            assert (outs["torch"][2] != ref.scenario.all_goal_reached).any()
    assert envs["fused"].scenario._fused_plan() is not None
    assert envs["graph"].graph_status == "graph", envs["graph"].graph_reason


def _program(env):
    return env.get_from_scenario(get_observations=True, get_rewards=True, get_infos=True, get_dones=True)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("n_agents", [2, 4, 9])
def test_program_on_hand_placed_states_gpu(gpu_device, monkeypatch, n_agents, fast):
    """The program alone, with no physics step between placing and evaluating: the hand-placed
    on-goal / overlapping / between-the-radii envs, then the batch-wide part of World.collides --
    a pair 0.003 past touching (inside min_collision_distance) in env 40 is penalised only while
    some env of the batch has that pair touching (the one-workgroup launch behind the program
    takes the penalty back otherwise: k_navigation_pairs)."""
    monkeypatch.setattr(_fused, "EXACT_LIDAR", not fast)
    envs = _mode_envs(gpu_device, ("torch", "fused"), B, seed=9, n_agents=n_agents)
    ref, fus = envs["torch"], envs["fused"]

    def both(what):
        with _Torch():
            exp = _program(ref)
        got = _program(fus)
        assert fus.scenario._fc is not None  # (the fused launch ran)
        if fast:  # (the LIDAR columns within the tolerance: test_fast_lidar_program_gpu)
            for e, g in zip(exp[0], got[0]):
                assert torch.equal(e[:, :6], g[:, :6]), what
            exp, got = exp[1:], got[1:]
        _assert_same(exp, got, f"{what} outputs")
        _assert_same(scenario_attributes(ref), scenario_attributes(fus), f"{what} attributes")
        return exp

    for env in (ref, fus):
        place_cases(env)
    exp = both("placed")
    infos = exp[-1]
    assert (infos[0]["agent_collisions"][8:16] != 0).all() and (infos[1]["agent_collisions"][8:16] != 0).all()
    assert (infos[0]["final_rew"][0:8] != 0).all()
    for touching in (False, True):
        s = _rng_save()
        with _Torch():
            ref.reset()
        _rng_load(s)
        fus.reset()
        for env in (ref, fus):
            a0, a1 = env.agents[:2]
            pos = a1.state.pos.clone()
            pos[40] = a0.state.pos[40] + torch.tensor([2 * a0.shape.radius + 0.003, 0.0], device=gpu_device)
            if touching:
                pos[129] = a0.state.pos[129] + torch.tensor([2 * a0.shape.radius - 0.01, 0.0], device=gpu_device)
            a1.set_pos(pos, batch_index=None)
        exp = both(f"near, touching={touching}")
        # (agent 0's only close neighbour in env 40 is agent 1: the spawn keeps the others 0.25 away)
        assert bool(exp[-1][0]["agent_collisions"][40] != 0) == touching
    # the scratch words are left zero for the next launch
    assert not fus.scenario._fused_plan()["ws"].any()


@pytest.mark.gpu
def test_fast_lidar_program_gpu(gpu_device):
    """The default program (fast LIDAR): every output but the LIDAR columns is bit-identical to
    the torch program; the measurements match the CPU oracle's World.cast_rays on the same state
    within the LIDAR tolerance, a ray outside it only at a hit / miss boundary (certified,
    tests/_parity.py lidar_parity)."""
    from tests._parity import lidar_parity

    envs = _mode_envs(gpu_device, ("torch", "fused"), 4096)
    ref, fus = envs["torch"], envs["fused"]
    worst = 0.0
    for t in range(8):
        actions = ref.get_random_actions()
        outs = {}
        for mode, env in envs.items():
            s = _rng_save()
            with _Torch() if mode == "torch" else _NullCtx():
                outs[mode] = env.step([a.clone() for a in actions])
            if mode == "torch":
                _rng_load(s)
        for a, ot, of in zip(fus.agents, outs["torch"][0], outs["fused"][0]):
            assert torch.equal(ot[:, :6], of[:, :6]), (t, a.name)
            # the observation holds max_range - the measurement the sensor keeps
            assert torch.equal(of[:, 6:], a.sensors[0]._max_range - a.sensors[0]._last_measurement)
        _assert_same(outs["torch"][1:], outs["fused"][1:], f"rewards / dones / infos step {t}")
        _assert_same(_state(ref), _state(fus), f"state step {t}")
        _assert_same(scenario_attributes(ref), scenario_attributes(fus), f"attributes step {t}")
        rep = lidar_parity(fus, measured=True)
        assert rep["ok"], (t, rep)
        worst = max(worst, rep["bad_rows"] / max(rep["rows"], 1))
    assert worst < 1e-3  # boundary rays are rare


@pytest.mark.gpu
def test_over_the_agent_cap_runs_the_torch_program_gpu(gpu_device):
    kw = dict(n_agents=N.VMAS_NAV_MAX_AGENTS + 1, collisions=False)
    envs = _mode_envs(gpu_device, ("torch", "fused"), B, **kw)
    ref, fus = envs["torch"], envs["fused"]
    assert _fused.enabled(fus.world) and fus.scenario._fused_plan() is None
    for t in range(3):
        actions = ref.get_random_actions()
        with _Torch():
            exp = ref.step([a.clone() for a in actions])
        got = fus.step([a.clone() for a in actions])
        _assert_same(exp, got, f"outputs step {t}")
        _assert_same(scenario_attributes(ref), scenario_attributes(fus), f"attributes step {t}")
    assert got[0][0].shape == (B, 6)


@pytest.mark.gpu
def test_discrete_actions_replay_gpu(gpu_device):
    envs = []
    for graph_step in (False, None):
        saved = _rng_save()
        envs.append(make_env("navigation", num_envs=B, device=gpu_device, seed=1, continuous_actions=False,
                             graph_step=graph_step))
        if graph_step is False:
            _rng_load(saved)
    eager, graph = envs
    for t in range(6):
        actions = eager.get_random_actions()
        out_e = eager.step([a.clone() for a in actions])
        out_g = graph.step([a.clone() for a in actions])
        _assert_same(out_e, out_g, f"outputs step {t}")
        _assert_same(_state(eager), _state(graph), f"state step {t}")
    assert graph.graph_status == "graph", graph.graph_reason


@pytest.mark.gpu
def test_default_env_replays_gpu(gpu_device):
    env = make_env("navigation", num_envs=B, device=gpu_device, seed=0)
    for _ in range(6):
        obs, rew, done, info = env.step(env.get_random_actions())
    assert env.graph_status == "graph", env.graph_reason
    # the info tensors after a replay are the scenario's
    assert torch.equal(info[0]["pos_rew"], env.scenario.pos_rew)
    assert torch.equal(info[2]["agent_collisions"], env.agents[2].agent_collision_rew)
    frames = env.render_batch([0, 129])
    assert frames.shape[0] == 2 and frames.shape[-1] == 3
    assert env.render(mode="rgb_array", env_index=129).shape == tuple(frames.shape[1:])


def test_navigation_io_layout_and_argument_checks():
    """VmasNavigationIO as Python declares it against a C compilation of the header (following
    tests/test_abi.py), under the 4 KiB of a kernel argument block; the entry point refuses a
    non-sphere agent and an agent count over the cap without touching a device."""
    import subprocess
    import tempfile
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    probe = r'''
#include <stddef.h>
#include <stdio.h>
#include "vmas_mi355x.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %d %d\n", sizeof(VmasNavigationIO), offsetof(VmasNavigationIO, agents),
    offsetof(VmasNavigationIO, circ), offsetof(VmasNavigationIO, vel), offsetof(VmasNavigationIO, shaping_in),
    offsetof(VmasNavigationIO, out_delta), VMAS_NAV_MAX_AGENTS, VMAS_NAV_WS_WORDS);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = Path(d) / "probe.c"
        src.write_text(probe)
        exe = Path(d) / "probe"
        subprocess.run(["gcc", "-I", str(root / "include"), str(src), "-o", str(exe)], check=True)
        c = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()))
    io = N.VmasNavigationIO
    assert c == [ctypes.sizeof(io), io.agents.offset, io.circ.offset, io.vel.offset, io.shaping_in.offset,
                 io.out_delta.offset, N.VMAS_NAV_MAX_AGENTS, N.VMAS_NAV_WS_WORDS]
    assert ctypes.sizeof(io) <= 4096
    lib = N.load_library()
    assert "vmas_navigation_outputs" in N.EXPORTED_SYMBOLS and N.fn_addr("vmas_navigation_outputs")
    VMAS_E_INVALID = -1
    assert lib.vmas_navigation_outputs(0, None, None) == VMAS_E_INVALID
    a = io()
    a.batch, a.n_agents, a.what = 4, 2, N.VMAS_SCN_OBS
    a.agents[0].shape = a.agents[1].shape = N.VMAS_SPHERE
    a.n_agents = N.VMAS_NAV_MAX_AGENTS + 1
    assert lib.vmas_navigation_outputs(0, ctypes.byref(a), None) == VMAS_E_INVALID
    a.n_agents = 2
    a.agents[1].shape = N.VMAS_BOX
    assert lib.vmas_navigation_outputs(0, ctypes.byref(a), None) == VMAS_E_INVALID
    assert b"not a sphere" in lib.vmas_aux_last_error()
