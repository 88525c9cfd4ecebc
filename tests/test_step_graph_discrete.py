"""Graph mode with discrete actions (Environment._apply_discrete_actions writes the persistent
action buffer the captured step reads): a replayed step returns the same outputs and leaves the
same world as the eager step, bit for bit, through reset_at / reset; make_env's default picks the
graph step for discrete envs too; a bad action in a replaying env raises as the eager env does and
the worlds continue identically.

(The file's name sorts it after test_jit.py and test_spawn.py: every graph capture takes one of
torch's 32 pooled streams, and those two files hold CUs from a ``torch.cuda.Stream()`` that must not
share the current stream's hardware queue -- one pooled stream in four does on an MI355X with 4
queues -- so captures added before them shift which stream they get.)"""
import math

import pytest
import torch

from vectorizedmultiagentsimulator_amd import make_env
from vectorizedmultiagentsimulator_amd.simulator.environment import Environment

from tests._action_chunks import ENVS, NINE, SpecScenario


def _flat(tree, acc):
    if isinstance(tree, torch.Tensor):
        acc.append(tree)
    elif isinstance(tree, (list, tuple)):
        for x in tree:
            _flat(x, acc)
    elif isinstance(tree, dict):
        for k in sorted(tree):
            _flat(tree[k], acc)
    return acc


def _state(env):
    out = []
    for e in env.world.entities:
        s = e.state
        out += [s.pos, s.vel, s.rot, s.ang_vel]
    return out


def _rng_save():
    return ([x.clone() if isinstance(x, torch.Tensor) else x for x in Environment.vmas_random_state],
            torch.cuda.get_rng_state())


def _rng_load(saved):
    Environment.vmas_random_state[:] = [x.clone() if isinstance(x, torch.Tensor) else x for x in saved[0]]
    torch.cuda.set_rng_state(saved[1])


def _assert_same(a, b, what):
    fa, fb = _flat(a, []), _flat(b, [])
    assert len(fa) == len(fb), what
    for i, (x, y) in enumerate(zip(fa, fb)):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, i)
        assert torch.equal(x, y), (what, i, (x.float() - y.float()).abs().max().item())


def _twins(device, name, graphs, num_envs, substeps=None, **kw):
    """Envs of the same construction-time RNG state, one per graph_step value."""
    envs = []
    saved = _rng_save()
    for graph in graphs:
        _rng_load(saved)
        env = make_env(name, num_envs=num_envs, device=device, seed=1, graph_step=graph, continuous_actions=False, **kw)
        if substeps:
            env.world._substeps = substeps
            env.world._sub_dt = env.world._dt / substeps
        envs.append(env)
    return envs


def _actions(env, gen):
    out = []
    for ag in env.agents:
        nvec = ag.discrete_action_nvec
        if env.multidiscrete_actions:
            a = torch.stack([torch.randint(0, n, (env.num_envs,), generator=gen) for n in nvec], dim=-1)
        else:
            a = torch.randint(0, math.prod(nvec), (env.num_envs, 1), generator=gen)
        assert a.dtype is torch.int64
        out.append(a.to(env.device))
    return out


def _step_all(envs, actions, expect_raise=None):
    """The same step in every env, each from the same host / device RNG state."""
    outs, msgs = [], []
    s = _rng_save()
    for env in envs:
        _rng_load(s)
        if expect_raise is not None:
            with pytest.raises(AssertionError, match=expect_raise) as ei:
                env.step([a.clone() for a in actions])
            msgs.append(str(ei.value))
        else:
            outs.append(env.step([a.clone() for a in actions]))
    return msgs if expect_raise is not None else outs


@pytest.mark.gpu
@pytest.mark.parametrize("multi", [False, True], ids=["flat", "multi"])
@pytest.mark.parametrize("name,substeps", [("balance", 10), ("transport", None)])
def test_discrete_graph_replay_matches_eager_gpu(gpu_device, name, substeps, multi):
    eager, graph, auto = _twins(gpu_device, name, (False, True, None), 512, substeps, n_agents=4,
                                multidiscrete_actions=multi)
    assert auto.graph_auto and auto._graph is not None  # (the default picks the graph step)
    gen = torch.Generator().manual_seed(5)
    for t in range(14):
        actions = _actions(eager, gen)
        if t == 7:  # in-place edit between steps (reset_at -> set_pos(batch_index))
            s = _rng_save()
            for env in (eager, graph, auto):
                _rng_load(s)
                env.reset_at(3)
        if t == 10:  # full reset re-binds every state tensor
            s = _rng_save()
            for env in (eager, graph, auto):
                _rng_load(s)
                env.reset()
        out_e, out_g, out_a = _step_all((eager, graph, auto), actions)
        for what, out, env in (("graph", out_g, graph), ("default", out_a, auto)):
            _assert_same(out_e, out, f"{name} {what} outputs step {t}")
            _assert_same(_state(eager), _state(env), f"{name} {what} state step {t}")
            assert torch.equal(eager.steps, env.steps), (name, what, t)
            for x, y in zip(eager.agents, env.agents):
                assert torch.equal(x.action.u, y.action.u), (name, what, t)
    for env in (graph, auto):
        assert env.graph_status == "graph", env.graph_reason
        assert env._graph.replays >= 5
    assert eager.graph_status == "off"


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["range", "nan"])
@pytest.mark.parametrize("speculative", [False, True], ids=["wait", "speculative"])
def test_discrete_failed_action_check_leaves_world_as_eager_gpu(gpu_device, monkeypatch, bad, speculative):
    """An out-of-range (int64) or NaN (float32) discrete action in a replaying env raises the eager
    env's AssertionError and leaves the world as the eager step leaves it -- also when the replay
    was launched before the flags were known (speculative, rolled back; there every agent's u is
    the eager env's too).  The env keeps replaying, as a continuous one does after a failed check."""
    monkeypatch.setattr(Environment, "_SPECULATE", speculative)
    eager, graph = _twins(gpu_device, "balance", (False, True), 256, n_agents=4)
    gen = torch.Generator().manual_seed(6)
    for _ in range(5):
        _step_all((eager, graph), _actions(eager, gen))
    assert graph.graph_status == "graph", graph.graph_reason
    assert graph._can_speculate() == speculative
    before_u = [a.action.u.clone() for a in graph.agents]
    actions = _actions(eager, gen)
    if bad == "nan":
        actions = [a.to(torch.float32) for a in actions]
        actions[2][5, 0] = float("nan")
    else:
        actions[2][5, 0] = 9  # (balance: flat index of [3, 3])
    msgs = _step_all((eager, graph), actions, "^$" if bad == "nan" else r"allowed int range \[0,3\)")
    assert msgs[0] == msgs[1]
    _assert_same(_state(eager), _state(graph), "state after the failed step")
    for i, (ae, ag) in enumerate(zip(eager.agents, graph.agents)):
        if i < 2 or speculative:  # (without speculation the failing agent and those after it may
            # hold the rejected actions in their persistent u until the next step, as with
            # continuous actions)
            assert torch.equal(ae.action.u, ag.action.u), i
        if speculative and (i > 2 or (i == 2 and bad == "nan")):  # (a range failure zeroes agent 2's u)
            assert torch.equal(ag.action.u, before_u[i]), i
    assert torch.equal(eager.steps, graph.steps)
    for t in range(4):
        out_e, out_g = _step_all((eager, graph), _actions(eager, gen))
        _assert_same(out_e, out_g, f"outputs after the failed step {t}")
        _assert_same(_state(eager), _state(graph), f"state after the failed step {t}")
    assert graph.graph_status == "graph"


@pytest.mark.gpu
@pytest.mark.parametrize("speculative", [False, True], ids=["wait", "speculative"])
def test_discrete_fractional_flat_index_in_a_replaying_env_gpu(gpu_device, monkeypatch, speculative):
    """A float32 flat index with a fraction passes the reference's checks (it is floored); the
    kernel leaves it to the per-agent path, also after a speculative replay was rolled back for
    it: the step's results are the eager env's and the env keeps replaying."""
    monkeypatch.setattr(Environment, "_SPECULATE", speculative)
    eager, graph = _twins(gpu_device, "balance", (False, True), 256, n_agents=4)
    gen = torch.Generator().manual_seed(7)
    for _ in range(5):
        _step_all((eager, graph), _actions(eager, gen))
    assert graph.graph_status == "graph", graph.graph_reason
    for t in range(3):
        actions = [a.to(torch.float32) for a in _actions(eager, gen)]
        if t == 1:
            actions[1][7, 0] += 0.5
        out_e, out_g = _step_all((eager, graph), actions)
        _assert_same(out_e, out_g, f"outputs step {t}")
        _assert_same(_state(eager), _state(graph), f"state step {t}")
        for x, y in zip(eager.agents, graph.agents):
            assert torch.equal(x.action.u, y.action.u), t
    assert graph.graph_status == "graph" and torch.equal(eager.steps, graph.steps)


@pytest.mark.gpu
def test_discrete_graph_replay_with_nine_agents_gpu(gpu_device):
    """9 agents are more refs than one action launch carries: graph mode does not speculate (the
    blocking apply makes its two launches before every replay) and the replayed steps leave the
    eager twin's state."""
    envs, saved = [], _rng_save()
    for graph in (False, True):
        _rng_load(saved)
        envs.append(make_env(SpecScenario(), num_envs=ENVS, device=gpu_device, seed=1, graph_step=graph,
                             continuous_actions=False, specs=NINE))
    eager, graph = envs
    gen = torch.Generator().manual_seed(8)
    for _ in range(5):
        _step_all(envs, _actions(eager, gen))
    assert graph.graph_status == "graph", graph.graph_reason
    assert not graph._can_speculate()
    replays = graph._graph.replays
    for t in range(3):
        out_e, out_g = _step_all(envs, _actions(eager, gen))
        _assert_same(out_e, out_g, f"outputs step {t}")
        _assert_same(_state(eager), _state(graph), f"state step {t}")
        for x, y in zip(eager.agents, graph.agents):
            assert torch.equal(x.action.u, y.action.u), t
    assert graph._graph.replays >= replays + 3 and graph.graph_status == "graph"
