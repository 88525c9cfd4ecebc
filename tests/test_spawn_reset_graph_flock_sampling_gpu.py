"""reset_where between the replays of a graph-mode env, for flocking (vmas_spawn_reset) and sampling
(vmas_sampling_reset); the eager cases are in tests/test_reset_where_flock_sampling_gpu.py.

(The file's name sorts it after test_jit.py and test_spawn.py: tests/test_spawn_reset_graph_gpu.py has
the reason.)"""
import pytest
import torch

from tests import _reset_where as R
from tests.test_reset_where_spawn_gpu import _need_mode


def _state(env):
    out = []
    for e in env.world.entities:
        s = e.state
        out += [s.pos, s.vel, s.rot, s.ang_vel]
    for a in env.world.agents:
        out += [a.state.force, a.state.torque]
    sc = env.scenario
    if hasattr(sc, "sampled"):
        out += [sc.sampled, sc.max_pdf, sc._locs] + [a.sample for a in env.world.agents]
    else:
        out += [sc.t] + [a.distance_shaping for a in env.world.policy_agents]
    return out + [env.steps]


@pytest.mark.gpu
@pytest.mark.parametrize("max_steps", [None, 100])
@pytest.mark.parametrize("scenario", ["flocking", "sampling"])
def test_reset_where_between_graph_replays_gpu(gpu_device, scenario, max_steps):
    """reset_where between the steps of a graph-mode env: the native call's in-place writes reach the
    next replay by version counters, the env is still replaying afterwards, and every step's outputs
    and states equal an eager twin's."""
    dev = gpu_device
    B = 64
    _need_mode(dev, B)
    (eager, graph), _ = R.turns(dev, [False, True], lambda g: R.make_env(scenario, num_envs=B, device=dev, seed=1,
                                                                           graph_step=g, max_steps=max_steps))
    ptr = graph.scenario.sampled.data_ptr() if scenario == "sampling" else None
    masks = {5: torch.arange(B, device=dev) % 4 == 1, 9: torch.arange(B, device=dev) % 5 == 0}
    for t in range(14):
        actions = eager.get_random_actions()
        if t in masks:
            assert graph.graph_status == "graph", graph.graph_reason
            n0, e0 = graph.scenario.native_resets, eager.scenario.native_resets
            (o_e, o_g), (r_e, r_g) = R.turns(dev, [eager, graph], lambda env: env.reset_where(masks[t]))
            assert graph.scenario.native_resets == n0 + 1 and eager.scenario.native_resets == e0 + 1
            assert R.same_rng(r_e, r_g)
            for x, y in zip(R.flat(o_e), R.flat(o_g)):
                assert torch.equal(x, y), t
            for i, (x, y) in enumerate(zip(_state(eager), _state(graph))):
                assert torch.equal(x, y), (t, i)
            assert graph.graph_status == "graph", graph.graph_reason
        out_e, out_g = R.turns(dev, [eager, graph], lambda e: e.step([a.clone() for a in actions]))[0]
        fe, fg = R.flat(out_e), R.flat(out_g)
        assert len(fe) == len(fg)
        for i, (x, y) in enumerate(zip(fe, fg)):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (t, i)
        for i, (x, y) in enumerate(zip(_state(eager), _state(graph))):
            assert torch.equal(x, y), (t, i)
        if t >= 3:
            assert graph.graph_status == "graph", (t, graph.graph_reason)
    assert graph._graph.replays >= 10
    if ptr is not None:  # the flags are written in place: neither a reset nor a replay re-allocates them
        assert graph.scenario.sampled.data_ptr() == ptr
