"""The tail of a fused k_world launch (csrc/vmas_tail.hpp) read from its LDS copy, and the final
decider's way past the steal scan and the wait (csrc/vmas_jit_ops.hpp grid_next): graph-mode steps
on drawn-ahead random actions stay bit-identical to the eager twin on tiny batches -- a partial last
group, forced second passes, and one workgroup running every group (which is then every pass's
decider)."""
import pytest
import torch

from vectorizedmultiagentsimulator_amd import make_env

from tests.test_graph import _assert_same, _rng_load, _rng_save, _state

SCENARIOS = {"balance": (dict(n_agents=4), 10), "transport": (dict(n_agents=4), None)}
VARIANTS = {"default": {}, "2pass": {"VMAS_JIT_TEST_PASSES": "2"}, "cap1": {"VMAS_JIT_GRID_CAP": "1"}}


def _twins(gpu_device, name, num_envs, kw, substeps):
    envs = []
    for graph in (False, True):
        saved = _rng_save()
        env = make_env(name, num_envs=num_envs, device=gpu_device, seed=0, graph_step=graph, **kw)
        if substeps:
            env.world._substeps = substeps
            env.world._sub_dt = env.world._dt / substeps
        envs.append(env)
        if not graph:
            _rng_load(saved)
    return envs


def test_generated_kernel_reads_the_tail_from_lds(monkeypatch):
    """The generated source of a world with a tail copies Args.tail into LDS in the prologue and runs
    the tail from that copy; a module built without a tail (VMAS_JIT_TAIL=0) has neither."""
    from tests._parity import make

    kw, sub = SCENARIOS["balance"]
    src = make("balance", kw, sub, "cpu", num_envs=64, seed=0).world.engine.jit_compile_check()
    assert "__shared__ __attribute__((aligned(16))) VmasTail TL;" in src
    assert "vmas_tail::run(TL);" in src and "vmas_tail::run(a.tail)" not in src
    assert "__builtin_amdgcn_kernarg_segment_ptr()" in src
    monkeypatch.setenv("VMAS_JIT_TAIL", "0")
    src = make("balance", kw, sub, "cpu", num_envs=64, seed=0).world.engine.jit_compile_check()
    assert "VmasTail TL" not in src and "vmas_tail::run" not in src


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("num_envs", [70, 72, 192])  # (70, 72: two groups, the second partial)
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_tail_steps_match_the_eager_twin_gpu(gpu_device, monkeypatch, name, num_envs, variant):
    """8 steps of env.step(env.get_random_actions()): the drawn actions, action.u / state.force
    between the draw and the step (the snapshot), the outputs, the state and the step counter equal
    the eager twin's bit for bit, and the post-replay work ran as the launch's tail.  "2pass": a
    re-run pass after every first pass (its decider is not the final one and must still wait);
    "cap1": a one-workgroup grid, the decider of every pass.  The tail copies whole 4-byte words
    (vmas_graph_chain_launch_tail's admission), and transport carries a [B] bool: at 70 envs its
    replays keep the post-replay launch of their own (as before this file; everything else is still
    compared), so 72 envs is there as transport's partial second group with the tail."""
    from vectorizedmultiagentsimulator_amd import _native as N

    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    kw, substeps = SCENARIOS[name]
    tails0 = N.load_host().tail_launches()
    eager, graph = _twins(gpu_device, name, num_envs, kw, substeps)
    for t in range(8):
        s = _rng_save()
        a_e = eager.get_random_actions()
        _rng_load(s)
        a_g = graph.get_random_actions()
        _assert_same(a_e, a_g, f"draws step {t}")
        if t > 0:
            _assert_same([a.action.u for a in eager.agents], [a.action.u for a in graph.agents], f"u after draw {t}")
            _assert_same([a.state.force for a in eager.agents], [a.state.force for a in graph.agents],
                         f"force after draw {t}")
        s = _rng_save()
        out_e = eager.step(a_e)
        _rng_load(s)
        out_g = graph.step(a_g)
        _assert_same(out_e, out_g, f"{name} outputs step {t}")
        _assert_same(_state(eager), _state(graph), f"{name} state step {t}")
        _assert_same([a.action.u for a in eager.agents], [a.action.u for a in graph.agents], f"u step {t}")
        assert torch.equal(eager.steps, graph.steps), (name, t)
    assert graph.graph_status == "graph", graph.graph_reason
    tails = N.load_host().tail_launches() - tails0
    if name == "transport" and num_envs % 4:
        assert tails == 0
    else:
        assert tails >= 3, tails
    if variant == "2pass":
        assert graph.world.engine.last_iterations == 2
    if variant == "cap1":
        assert abs(graph.world.engine.jit_grid) == 1
