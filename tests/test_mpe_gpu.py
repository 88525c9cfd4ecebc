"""MPE simple_spread and simple_tag on gfx950: the native step program (csrc/vmas_scenarios.hip k_mpe)
bit-identical to the scenarios' torch programs and to the restatement of tests/_mpe_spec.py on the
hand-placed envs (tag's shaped team sums included: they pin the device's reduction order), the torch
fallbacks and their reasons, reset_where through vmas_uniform_reset against a twin's reset(), and
physics parity.  The graph-mode cases are in tests/test_step_graph_mpe_gpu.py.
Sizes: 1 env, 65 (a wave plus a lane), 257 (a block plus a thread), and the 16 hand-placed envs."""
import pytest
import torch

from tests import _mpe_spec as MS
from tests import _reset_where as R
from tests._parity import step_parity
from tests.test_mpe import CONFIGS, assert_equals_spec, task_of
from tests.test_reset_where_spawn_gpu import _need_mode
from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd import make_env
from vectorizedmultiagentsimulator_amd.simulator import _fused

from test_fused import _NullCtx, _Torch
from test_graph import _assert_same, _rng_load, _rng_save, _state


def _pair(gpu_device, config, B, seed=3, **extra):
    """Two eager envs of one configuration and seed in the same state, the 16 hand-placed envs written
    over their first rows: the first computes with the torch program, the second with the native one."""
    name, kw = CONFIGS[config]
    envs = []
    for mode in ("torch", "fused"):
        saved = _rng_save()
        with _Torch() if mode == "torch" else _NullCtx():
            env = make_env(name, num_envs=B, device=gpu_device, seed=seed, graph_step=False, **kw, **extra)
            for _ in range(2):
                g = torch.Generator().manual_seed(7)
                env.step([(torch.rand(B, 2, generator=g) * 2 - 1).to(gpu_device) for _ in env.agents])
        (MS.place_spread_cases if name == "simple_spread" else MS.place_tag_cases)(env)
        envs.append(env)
        if mode == "torch":
            _rng_load(saved)
    return envs


def _outputs(env, torch_program):
    with _Torch() if torch_program else _NullCtx():
        return env.get_from_scenario(get_observations=True, get_rewards=True, get_infos=False, get_dones=False)


def _compare(ref, fus, task, what):
    n0 = fus.scenario.native_launches
    exp, got = _outputs(ref, True), _outputs(fus, False)
    assert fus.scenario.native_launches == n0 + 1, what  # (one launch for every reward and observation)
    assert fus.scenario.fused_status == "native", fus.scenario.fused_status
    _assert_same(exp, got, f"{what} outputs")
    _assert_same(MS.scenario_tensors(ref, task), MS.scenario_tensors(fus, task), f"{what} scenario tensors")


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(CONFIGS))
def test_native_program_equals_torch_program_gpu(gpu_device, config):
    ref, fus = _pair(gpu_device, config, 257)
    _compare(ref, fus, task_of(CONFIGS[config][0]), config)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("config", ["spread_3", "tag_default", "tag_eight_shaped"])
def test_native_program_small_batches_gpu(gpu_device, config, B):
    ref, fus = _pair(gpu_device, config, B)
    _compare(ref, fus, task_of(CONFIGS[config][0]), f"{config} B={B}")


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["spread_3", "tag_shaped"])
def test_native_program_reads_both_strides_gpu(gpu_device, config):
    """Positions and velocities as non-contiguous views: a [B, 4] buffer sliced [:, ::2]."""
    B = 257
    ref, fus = _pair(gpu_device, config, B)
    for env in (ref, fus):
        for e in env.world.entities:
            for field in ("pos", "vel"):
                buf = torch.zeros(B, 4, device=gpu_device)
                buf[:, ::2] = getattr(e.state, field)
                setattr(e.state, field, buf[:, ::2])
                assert getattr(e.state, field).stride() == (4, 2)
    _compare(ref, fus, task_of(CONFIGS[config][0]), f"{config} strided")


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(CONFIGS))
def test_native_program_equals_the_spec_on_hand_placed_envs_gpu(gpu_device, config):
    """Bit for bit, team sums included: the spec's sum is the order the device's reduction was found to
    use (tools/probe_sum_order.py)."""
    _, fus = _pair(gpu_device, config, MS.N_CASE_ENVS)
    task = task_of(CONFIGS[config][0])
    spec = MS.MpeSpec(fus, task)
    exp = spec.run()
    (MS.assert_spread_cases_fired if task == "spread" else MS.assert_tag_cases_fired)(spec, exp)
    n0 = fus.scenario.native_launches
    scn = fus.scenario
    rewards = [scn.reward(a) for a in fus.agents]
    obs = [scn.observation(a) for a in fus.agents]
    assert scn.native_launches == n0 + 1
    assert_equals_spec(fus, task, exp, (rewards, obs), bitwise_team_sums=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", range(1, 9))
def test_team_sum_order_is_found_for_every_team_size_gpu(gpu_device, n):
    """torch's .sum(-1) over a contiguous [B, n] tensor is one of the program's orders, and the one the
    spec states: the largest power of two <= n accumulators (two values sum the same with one
    accumulator or two, and the probe reports the first count that fits)."""
    want = 1 if n <= 2 else 1 << (n.bit_length() - 1)
    assert _fused.reduce_order(torch.device(gpu_device), n, "sum", N.VMAS_MPE_MAX_AGENTS) == want


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,why", [
    ("simple_spread", dict(n_agents=9), "torch: 9 agents"),
    ("simple_tag", dict(num_landmarks=9), "torch: 9 landmarks"),
    ("simple_tag", dict(respawn_at_catch=True), "torch: respawn_at_catch"),
])
def test_declined_worlds_run_the_torch_program_gpu(gpu_device, name, kw, why):
    B = 65
    envs = []
    for mode in ("torch", "fused"):
        saved = _rng_save()
        with _Torch() if mode == "torch" else _NullCtx():
            envs.append(make_env(name, num_envs=B, device=gpu_device, seed=3, graph_step=False, **kw))
        if mode == "torch":
            _rng_load(saved)
    ref, fus = envs
    assert _fused.enabled(fus.world) and fus.scenario._fused_plan() is None
    assert fus.scenario.fused_status.startswith(why), fus.scenario.fused_status
    if "respawn" in why:
        assert fus.scenario.fused_status == "torch: respawn_at_catch"
    g = torch.Generator().manual_seed(5)
    for t in range(3):
        actions = [(torch.rand(B, 2, generator=g) * 2 - 1).to(gpu_device) for _ in ref.agents]
        s = _rng_save()
        with _Torch():
            exp = ref.step([a.clone() for a in actions])
        _rng_load(s)
        got = fus.step([a.clone() for a in actions])
        _assert_same(exp, got, f"outputs step {t}")
        _assert_same(_state(ref), _state(fus), f"state step {t}")
    assert fus.scenario.native_launches == 0  # (the launch counter did not move)


# ---- reset_where ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", [("simple_spread", dict()), ("simple_spread", dict(n_agents=5)), ("simple_tag", dict()),
                                     ("simple_tag", dict(bound=1.3, num_good_agents=2))])
def test_reset_where_rows_of_a_full_reset_gpu(gpu_device, name, kw):
    dev, B = gpu_device, 257
    _need_mode(dev, B)
    lib = N.load_library()
    idx = torch.arange(B, device=dev)
    for case, mask in (("ends", (idx == 0) | (idx == B - 1)), ("mixed", (idx % 3 == 0) | (idx == B - 1)),
                       ("none", idx < 0), ("all", idx >= 0)):
        env, twin = R.twins(name, 2, B, dev, graph_step=False, **kw)
        n0, w0 = env.scenario.native_resets, lib.vmas_host_waits()
        steps_before = env.steps.clone()
        R.check_rows_of_full_reset(env, twin, mask, mask, dev, return_dones=True)  # (rows, other rows, generator offset)
        assert env.scenario.native_resets == n0 + 1, case  # (the launch answered: no fall-back)
        assert (lib.vmas_host_waits() - w0) & 0xFFFFFFFF == 0, case
        assert torch.equal(env.steps[~mask], steps_before[~mask]) and not env.steps[mask].any()
        R.check_next_step_agrees(env, twin, mask, dev)


@pytest.mark.gpu
def test_reset_where_beyond_the_draw_table_takes_the_generic_path_gpu(gpu_device):
    """13 agents and 13 landmarks are 26 uniform_ calls: over VMAS_URESET_MAX_DRAWS."""
    dev, B = gpu_device, 65
    env, twin = R.twins("simple_spread", 2, B, dev, graph_step=False, n_agents=13)
    mask = torch.arange(B, device=dev) % 2 == 0
    R.check_rows_of_full_reset(env, twin, mask, mask, dev, return_dones=True)
    assert env.scenario.native_resets == 0


# ---- physics ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["simple_spread", "simple_tag"])
def test_step_parity_gpu(gpu_device, name):
    env = make_env(name, num_envs=257, device=gpu_device, seed=2, graph_step=False)
    (MS.place_spread_cases if name == "simple_spread" else MS.place_tag_cases)(env)  # (contacts from the first step)
    reps = step_parity(env, 4)
    assert all(r["ok"] for r in reps), reps
