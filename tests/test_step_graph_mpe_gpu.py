"""MPE simple_spread and simple_tag in graph mode on gfx950: the default make_env call replayed from a HIP
graph against an eager twin for continuous and discrete actions (one k_mpe launch in the captured step,
nothing of the scenario carried, observations and rewards relocated directly), and reset_where between
the replays; the eager cases are in tests/test_mpe_gpu.py.

(The file's name sorts it after test_jit.py and test_spawn.py, as test_step_graph_discrete.py's does:
every graph capture takes one of torch's 32 pooled streams, and those two files hold CUs from a
``torch.cuda.Stream()`` that must not share the current stream's hardware queue, so captures added
before them shift which stream they get.)"""
import pytest
import torch

from tests import _mpe_spec as MS
from tests import _reset_where as R
from tests.test_mpe import task_of
from tests.test_reset_where_spawn_gpu import _need_mode
from vectorizedmultiagentsimulator_amd import make_env

from test_graph import _assert_same, _rng_load, _rng_save, _state


def _count_captured_launches(env):
    """Wraps the scenario's launch: [calls made during a stream capture, calls made outside one]."""
    scn = env.scenario
    counts = [0, 0]
    inner = scn._run_fused

    def counted(what):
        counts[0 if torch.cuda.is_current_stream_capturing() else 1] += 1
        return inner(what)

    scn._run_fused = counted
    return counts


@pytest.mark.gpu
@pytest.mark.parametrize("continuous", [True, False])
@pytest.mark.parametrize("name", ["simple_spread", "simple_tag"])
def test_default_make_env_call_replays_and_equals_an_eager_twin_gpu(gpu_device, name, continuous):
    B = 257
    envs = []
    for graph_step in (False, None):  # (None: the default make_env call)
        saved = _rng_save()
        envs.append(make_env(name, num_envs=B, device=gpu_device, seed=2, graph_step=graph_step, continuous_actions=continuous))
        if graph_step is False:
            _rng_load(saved)
    eager, graph = envs
    counts = _count_captured_launches(graph)
    task = task_of(name)
    replayed = 0
    for t in range(10):
        actions = eager.get_random_actions()
        was_graph = graph.graph_status == "graph"
        outside = counts[1]
        out_e = eager.step([a.clone() for a in actions])
        out_g = graph.step([a.clone() for a in actions])
        _assert_same(out_e, out_g, f"outputs step {t}")
        _assert_same(_state(eager), _state(graph), f"state step {t}")
        _assert_same(MS.scenario_tensors(eager, task), MS.scenario_tensors(graph, task), f"scenario tensors step {t}")
        if was_graph:  # a replayed step: the program ran inside the graph, nowhere else
            assert counts[1] == outside, t
            replayed += 1
    assert graph.graph_status == "graph", graph.graph_reason
    assert graph.scenario.fused_status == "native"
    assert replayed >= 5 and graph._graph.replays >= 5
    assert counts[0] == 1  # the captured step holds exactly one k_mpe launch
    # write-only trust and direct outputs: nothing of the scenario is carried, obs and rewards are relocated
    assert not any(n.startswith("Scenario.") or n.endswith(".rew") for n in graph._graph._carry_names), graph._graph._carry_names
    assert len(graph._graph._direct.enabled) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["simple_spread", "simple_tag"])
def test_reset_where_between_graph_replays_gpu(gpu_device, name):
    dev, B = gpu_device, 257
    _need_mode(dev, B)
    task = task_of(name)
    (eager, graph), _ = R.turns(dev, [False, True], lambda g: make_env(name, num_envs=B, device=dev, seed=1, graph_step=g))
    idx = torch.arange(B, device=dev)
    masks = {5: (idx % 4 == 1) | (idx == 0) | (idx == B - 1), 8: idx == B - 1}
    for t in range(11):
        actions = eager.get_random_actions()
        if t in masks:
            assert graph.graph_status == "graph", graph.graph_reason
            n0, e0 = graph.scenario.native_resets, eager.scenario.native_resets
            (o_e, o_g), (r_e, r_g) = R.turns(dev, [eager, graph], lambda env: env.reset_where(masks[t]))
            assert graph.scenario.native_resets == n0 + 1 and eager.scenario.native_resets == e0 + 1
            assert R.same_rng(r_e, r_g)
            _assert_same(o_e, o_g, f"reset_where outputs {t}")
            _assert_same(_state(eager), _state(graph), f"reset_where state {t}")
        out_e, out_g = R.turns(dev, [eager, graph], lambda e: e.step([a.clone() for a in actions]))[0]
        _assert_same(out_e, out_g, f"outputs step {t}")
        _assert_same(_state(eager), _state(graph), f"state step {t}")
        _assert_same(MS.scenario_tensors(eager, task), MS.scenario_tensors(graph, task), f"scenario tensors step {t}")
        if t >= 3:
            assert graph.graph_status == "graph", (t, graph.graph_reason)
    assert graph._graph.replays >= 7
