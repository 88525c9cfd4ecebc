"""Fused discrete-action path (Environment._apply_discrete_actions -> vmas_apply_discrete_actions,
csrc/vmas_actions.hip) against the per-agent path (_set_action, the reference's
environment.py:615-760 loop): identical u for every (n, a) of n = 2 .. 17 as multi-discrete and
flat actions in int64 / int32 / float32, identical worlds after steps, the reference's exception
and side effects when agent i's action is out of range or NaN, float actions with fractional
values, the cases the fused path declines, and the noise draws."""
import math
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd import make_env
from vectorizedmultiagentsimulator_amd.simulator.environment import Environment

from tests._action_chunks import SpecScenario, late_chunk_failure

ROOT = Path(__file__).resolve().parent.parent
DTYPES = [torch.int64, torch.int32, torch.float32]
SCALES = [(1.0, 1.0), (1.0, 0.3), (0.7, 1.0), (0.7, 0.3)]  # (u_range, u_multiplier)


MIXED = [((5, 4), 1.0, 0.5), ((3, 6, 7), 0.7, 0.3)]  # action_size 2 and 3, different nvec


def _pair(device, scenario="balance", num_envs=64, **kw):
    # (eager steps: the action paths themselves; graph mode's use of them is tests/test_step_graph_discrete.py's)
    mk = (lambda: SpecScenario()) if scenario == "spec" else (lambda: scenario)
    a = make_env(mk(), num_envs=num_envs, device=device, seed=3, graph_step=False, continuous_actions=False, **kw)
    b = make_env(mk(), num_envs=num_envs, device=device, seed=3, graph_step=False, continuous_actions=False, **kw)
    b._apply_discrete_actions = lambda actions, *args, **kw: False  # force the per-agent path
    return a, b


def _random_actions(env, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for ag in env.agents:
        nvec = ag.discrete_action_nvec
        if env.multidiscrete_actions:
            a = torch.stack([torch.randint(0, n, (env.num_envs,), generator=g) for n in nvec], dim=-1)
        else:
            a = torch.randint(0, math.prod(nvec), (env.num_envs, 1), generator=g)
        out.append(a.to(env.device))
    return out


def _fused_vs_per_agent_u(env, actions):
    """u of every agent from the fused path and from the per-agent path of the same env."""
    assert env._apply_discrete_actions([a.clone() for a in actions]) is True
    fused = [ag.action.u.clone() for ag in env.agents]
    for a, ag in zip(actions, env.agents):
        env._set_action(a.clone(), ag)
    return fused, [ag.action.u for ag in env.agents]


def _table_multi(device, dtype):
    # every (n, a), n = 2 .. 17, 0 <= a < n: two agents of 8 components per (u_range, u_multiplier)
    groups = [tuple(range(2, 10)), tuple(range(10, 18))]
    specs = [(g, r, m) for r, m in SCALES for g in groups]
    env = make_env(SpecScenario(), num_envs=17, device=device, seed=0, graph_step=False, continuous_actions=False,
                   multidiscrete_actions=True, specs=specs)
    rows = torch.arange(17).unsqueeze(1)
    actions = [torch.minimum(rows, torch.tensor(g) - 1).to(dtype).to(device) for g, _, _ in specs]
    for g, a in zip(groups, actions):  # (the table is complete)
        assert all(set(a[:, c].tolist()) == set(range(n)) for c, n in enumerate(g))
    fused, ref = _fused_vs_per_agent_u(env, actions)
    for i, (x, y) in enumerate(zip(fused, ref)):
        assert x.shape == y.shape and torch.equal(x, y), (i, specs[i], (x - y).abs().max().item())


def _table_flat(device, dtype):
    nvecs = [(7, 8), (3, 3), (2, 13, 4)]
    specs = [(v, r, m) for r, m in SCALES for v in nvecs]
    B = max(math.prod(v) for v in nvecs)
    env = make_env(SpecScenario(), num_envs=B, device=device, seed=0, graph_step=False, continuous_actions=False,
                   specs=specs)
    actions = [(torch.arange(B) % math.prod(v)).unsqueeze(1).to(dtype).to(device) for v, _, _ in specs]
    fused, ref = _fused_vs_per_agent_u(env, actions)
    for i, (x, y) in enumerate(zip(fused, ref)):
        assert x.shape == y.shape and torch.equal(x, y), (i, specs[i], (x - y).abs().max().item())


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_discrete_table_multi(dtype):
    _table_multi("cpu", dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_discrete_table_flat(dtype):
    _table_flat("cpu", dtype)


def _twin_steps(device, multi, scenario="balance", num_envs=64, **kw):
    fused, ref = _pair(device, scenario, num_envs, multidiscrete_actions=multi, **kw)
    for step in range(3):
        acts = _random_actions(fused, seed=step)
        fused.step([x.clone() for x in acts])
        ref.step([x.clone() for x in acts])
        assert fused._apply_cache is not None and fused._apply_cache.refusal is None  # (the fused path took the step)
        for x, y in zip(fused.agents, ref.agents):
            assert torch.equal(x.action.u, y.action.u)
            assert x.action.u.shape == y.action.u.shape and x.action.u.is_contiguous()
        for x, y in zip(fused.world.entities, ref.world.entities):
            assert torch.equal(x.state.pos, y.state.pos)
            assert torch.equal(x.state.vel, y.state.vel)


@pytest.mark.parametrize("multi", [False, True], ids=["flat", "multi"])
def test_discrete_steps_match_per_agent_path(multi):
    _twin_steps("cpu", multi, n_agents=3)


@pytest.mark.parametrize("num_envs", [1, 777])
@pytest.mark.parametrize("multi", [False, True], ids=["flat", "multi"])
def test_discrete_steps_match_with_mixed_action_sizes(multi, num_envs):
    _twin_steps("cpu", multi, "spec", num_envs, specs=MIXED)


def _failure(device, multi, bad, num_envs=64, n_agents=3, who=1):
    fused, ref = _pair(device, num_envs=num_envs, multidiscrete_actions=multi, n_agents=n_agents)
    for env in (fused, ref):
        env.step(_random_actions(env, seed=9))
    acts = _random_actions(fused, seed=10)
    if bad == "nan":
        acts = [a.to(torch.float32) for a in acts]
        acts[who][-1, -1] = float("nan")
    else:
        n = 3 if multi else 9  # (balance: nvec [3, 3])
        acts[who][-1, -1] = -1 if bad == "negative" else n
    msgs = []
    for env in (fused, ref):
        with pytest.raises(AssertionError) as ei:
            env.step([x.clone() for x in acts])
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[1]
    if bad != "nan":
        assert "Discrete physical actions are out of bounds, allowed int range [0,3)" in msgs[0]
    for i, (x, y) in enumerate(zip(fused.agents, ref.agents)):
        assert torch.equal(x.action.u, y.action.u), i
    good = _random_actions(fused, seed=11)  # the flags were reset: a valid step passes again
    for env in (fused, ref):
        env.step([x.clone() for x in good])
    for x, y in zip(fused.agents, ref.agents):
        assert torch.equal(x.action.u, y.action.u)
    for x, y in zip(fused.world.entities, ref.world.entities):
        assert torch.equal(x.state.pos, y.state.pos)


@pytest.mark.parametrize("bad", ["negative", "n", "nan"])
@pytest.mark.parametrize("multi", [False, True], ids=["flat", "multi"])
def test_discrete_failure_side_effects(multi, bad):
    _failure("cpu", multi, bad)


@pytest.mark.parametrize("multi", [False, True], ids=["flat", "multi"])
def test_discrete_fractional_float_actions(multi):
    """Float actions with fractional values pass the reference's range check and follow its float
    arithmetic (a fractional component keeps its fraction; a fractional flat index is floored)."""
    fused, ref = _pair("cpu", "spec", 8, multidiscrete_actions=multi, specs=MIXED)
    if multi:
        a0 = torch.tensor([[0.5, 1.5], [1.5, 0.5], [2.0, 3.0], [4.5, 0.0], [0.0, 2.5], [2.5, 3.5], [3.0, 1.0],
                           [0.25, 0.75]])
        a1 = torch.tensor([[0.5, 1.5, 2.5], [1.0, 5.5, 6.5], [2.5, 0.0, 3.0], [0.0, 4.5, 0.5], [1.5, 2.0, 3.5],
                           [2.0, 1.0, 6.0], [0.75, 3.25, 1.5], [1.25, 5.0, 5.5]])
    else:
        a0 = torch.tensor([[0.5], [1.5], [19.5], [4.0], [7.25], [12.75], [0.0], [18.0]])
        a1 = torch.tensor([[0.5], [125.5], [41.5], [42.0], [7.25], [99.75], [0.0], [125.0]])
    for env in (fused, ref):
        env.step([a0.clone(), a1.clone()])
    for x, y in zip(fused.agents, ref.agents):
        assert torch.equal(x.action.u, y.action.u)
    for x, y in zip(fused.world.entities, ref.world.entities):
        assert torch.equal(x.state.pos, y.state.pos)


@pytest.mark.parametrize("multi,bad", [(False, "nan"), (False, "range"), (True, "range")],
                         ids=["flat-nan", "flat-range", "multi-range"])
def test_discrete_failure_in_a_later_chunk(multi, bad):
    """9 agents: the failing one is past the first 8 refs (on the host backend, past the first 16
    flag bytes)."""
    late_chunk_failure("cpu", bad, continuous=False, multi=multi)


def test_discrete_path_declines():
    env = make_env("features", num_envs=8, seed=0, continuous_actions=False)
    assert env.world.dim_c > 0 and any(not a.silent for a in env.agents)
    assert env._apply_discrete_actions(env.get_random_actions()) is False
    env = make_env("balance", num_envs=8, seed=0, n_agents=2, continuous_actions=False)
    for dtype in (torch.int16, torch.float64):
        assert env._apply_discrete_actions([torch.zeros(8, 1, dtype=dtype)] * 2) is False
    assert env._apply_discrete_actions([torch.zeros(8, 1, dtype=torch.int64)] * 2) is True
    # more components than the kernel's fixed maximum
    env = make_env(SpecScenario(), num_envs=4, seed=0, continuous_actions=False, multidiscrete_actions=True,
                   specs=[((2,) * 9, 1.0, 1.0)])
    assert env._apply_discrete_actions([torch.zeros(4, 9, dtype=torch.int64)]) is False
    env.step([torch.ones(4, 9, dtype=torch.int64)])  # (the per-agent path runs)


@pytest.mark.parametrize("double,expect", [(0, "u_range / u_multiplier are not float32"),
                                           (1, "discrete_action_nvec beyond what fp32 holds exactly")])
def test_discrete_refusal_names_the_first_agent_at_fault(double, expect):
    """Two agents with one problem each (a float64 u_range, an nvec past 2^24): the checks run per
    agent, in order, so the reason is the first agent's."""
    env = make_env(SpecScenario(), num_envs=4, seed=0, continuous_actions=False, multidiscrete_actions=True,
                   specs=[((3, 3), 1.0, 1.0), ((3, 3), 1.0, 1.0)])
    env.agents[double].action._u_range_tensor = env.agents[double].action.u_range_tensor.double()
    env.agents[1 - double].discrete_action_nvec = [3, (1 << 24) + 1]
    assert env._apply_discrete_actions([torch.zeros(4, 2, dtype=torch.int64)] * 2) is False
    assert env._apply_cache.refusal == expect


def test_discrete_changed_nvec_is_picked_up():
    fused, ref = _pair("cpu", multidiscrete_actions=True, n_agents=2)
    acts = [torch.full((64, 2), 2, dtype=torch.int64) for _ in fused.agents]
    for env in (fused, ref):
        env.step([a.clone() for a in acts])
    for env in (fused, ref):
        for ag in env.agents:
            ag.discrete_action_nvec = [5, 6]  # (re-assigned after construction, a plain list)
    acts = [torch.tensor([[4, 5]]).expand(64, 2).clone() for _ in fused.agents]  # out of range for [3, 3]
    for env in (fused, ref):
        env.step([a.clone() for a in acts])
    assert fused._apply_cache is not None and fused._apply_cache.refusal is None
    for x, y in zip(fused.agents, ref.agents):
        assert torch.equal(x.action.u, y.action.u)
    fused.agents[0].discrete_action_nvec[1] = 4  # (edited in place)
    with pytest.raises(AssertionError, match=r"\[0,4\)"):
        fused.step([a.clone() for a in acts])


def test_discrete_noise_draws_match():
    fused, ref = _pair("cpu", n_agents=3)
    for env in (fused, ref):
        for ag in env.agents:
            ag.action._u_noise = 0.1
    # the simulator's RNG state is shared by all environments (class attribute, as the
    # reference): give both steps the same one
    shared = Environment.vmas_random_state
    saved = list(shared)
    for env in (fused, ref):
        shared[:] = saved
        env.step(_random_actions(env, seed=4))
    assert fused._apply_cache is not None and fused._apply_cache.refusal is None
    for x, y in zip(fused.agents, ref.agents):
        assert torch.equal(x.action.u, y.action.u)


def test_discrete_ref_layout_matches_header():
    probe = '#include <stdio.h>\n#include "vmas_mi355x.h"\nint main(void) { printf("%zu %d\\n", ' \
            'sizeof(VmasDiscreteActionRef), VMAS_DISCRETE_MAX_COMPONENTS); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        src, exe = Path(d) / "probe.c", Path(d) / "probe"
        src.write_text(probe)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        size, k = map(int, subprocess.run([str(exe)], capture_output=True, text=True).stdout.split())
    assert size == N.DISCRETE_ACTION_REF_DTYPE.itemsize and k == N.DISCRETE_MAX_COMPONENTS
    assert N.DISCRETE_ACTION_REF_DTYPE["nvec"].shape == (k,)


# ---- on the device: the table compares against torch's own kernels there, which is what validates
# the probed division mode ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_discrete_table_multi_gpu(gpu_device, dtype):
    _table_multi(gpu_device, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_discrete_table_flat_gpu(gpu_device, dtype):
    _table_flat(gpu_device, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("multi", [False, True], ids=["flat", "multi"])
def test_discrete_steps_match_per_agent_path_gpu(gpu_device, multi):
    _twin_steps(gpu_device, multi, n_agents=3)


@pytest.mark.gpu
@pytest.mark.parametrize("num_envs", [1, 777])
@pytest.mark.parametrize("multi", [False, True], ids=["flat", "multi"])
def test_discrete_steps_match_with_mixed_action_sizes_gpu(gpu_device, multi, num_envs):
    _twin_steps(gpu_device, multi, "spec", num_envs, specs=MIXED)


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["negative", "n", "nan"])
@pytest.mark.parametrize("multi", [False, True], ids=["flat", "multi"])
def test_discrete_failure_side_effects_gpu(gpu_device, multi, bad):
    _failure(gpu_device, multi, bad)


@pytest.mark.gpu
def test_discrete_failure_many_workgroups_gpu(gpu_device):
    """The bad value in the last env of the last agent of 32 768 envs: the flag crosses the
    reduction over every workgroup's slot."""
    _failure(gpu_device, False, "n", num_envs=32768, n_agents=4, who=3)


@pytest.mark.gpu
@pytest.mark.parametrize("multi,bad", [(False, "nan"), (False, "range"), (True, "range")],
                         ids=["flat-nan", "flat-range", "multi-range"])
def test_discrete_failure_in_a_later_chunk_gpu(gpu_device, multi, bad):
    """9 agents are two launches (8 + 1 refs): the flag is set in the second one."""
    late_chunk_failure(gpu_device, bad, continuous=False, multi=multi)
