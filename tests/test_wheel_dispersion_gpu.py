"""The wheel and dispersion scenarios on gfx950: the native step programs (csrc/vmas_scenarios.hip
k_wheel / k_dispersion) bit-identical to the scenarios' torch programs eagerly and replayed from a HIP
graph, the programs alone on the hand-placed states of tests/_wheel_spec.py / tests/_dispersion_spec.py,
the torch fallback over the caps, discrete actions, the roll-back of a refused step, reset_where through
vmas_uniform_reset (csrc/vmas_reset.hip k_uniform_reset) against a twin's reset(), the call on plain
tensors across a round of torch's distribution grid, and physics parity.
130 envs: two full waves plus a partial one."""
import ctypes

import pytest
import torch

from tests import _dispersion_spec as DS
from tests import _reset_where as R
from tests import _wheel_spec as WS
from tests._parity import step_parity
from tests.test_reset_where_spawn_gpu import _need_mode
from tests.test_wheel_dispersion import place_agents_on_the_line
from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd import make_env
from vectorizedmultiagentsimulator_amd.simulator import _fused
from vectorizedmultiagentsimulator_amd.simulator.environment import _uniform

from test_fused import _NullCtx, _Torch
from test_graph import _assert_same, _rng_load, _rng_save, _state

B = 130

CASES = {
    "wheel": {"default": dict(), "one_agent": dict(n_agents=1), "short_fast": dict(line_length=1.5, desired_velocity=0.2)},
    "dispersion": {"default": dict(), "one_agent": dict(n_agents=1), "one_food": dict(n_food=1),
                   "share_and_penalise": dict(share_reward=True, penalise_by_time=True)},
}
ALL_CASES = [(name, case) for name, cases in CASES.items() for case in cases]


def _spec(name):
    return WS if name == "wheel" else DS


def _attrs(name, env):
    if name == "wheel":
        return [env.scenario.rew]
    return DS.landmark_attributes(env)


def _flag_ptrs(name, env):
    if name == "wheel":
        return []
    return [t.data_ptr() for f in env.world.landmarks for t in (f.eaten, f.just_eaten)]


def _mode_envs(gpu_device, name, modes, num_envs, seed=3, **kw):
    """One env per mode (torch: the torch program; fused: eager; graph: replayed), the same seed
    and generator states."""
    envs = {}
    for mode in modes:
        saved = _rng_save()
        with _Torch() if mode == "torch" else _NullCtx():
            envs[mode] = make_env(name, num_envs=num_envs, device=gpu_device, seed=seed, graph_step=mode == "graph", **kw)
        if mode != modes[-1]:
            _rng_load(saved)
    return envs


def _twelve_steps(gpu_device, name, case, num_envs, kw):
    envs = _mode_envs(gpu_device, name, ("torch", "fused", "graph"), num_envs, **kw)
    ref = envs["torch"]
    assert envs["fused"].scenario.fused_status == "native", envs["fused"].scenario.fused_status
    eaten_any = turned = False
    ptrs = None
    for t in range(12):
        actions = ref.get_random_actions()
        outs = {}
        for mode, env in envs.items():
            s = _rng_save()
            with _Torch() if mode == "torch" else _NullCtx():
                if t == 2 and num_envs >= 16:
                    _spec(name).place_cases(env)
                    if name == "wheel":
                        place_agents_on_the_line(env)
                if t == 5:
                    env.reset_at(min(7, num_envs - 1))
                if t == 9:
                    env.reset()
                outs[mode] = env.step([a.clone() for a in actions])
            if mode != "graph":
                _rng_load(s)
        for mode in ("fused", "graph"):
            _assert_same(outs["torch"], outs[mode], f"{name} {case} {mode} outputs step {t}")
            _assert_same(_state(ref), _state(envs[mode]), f"{name} {case} {mode} state step {t}")
            _assert_same(_attrs(name, ref), _attrs(name, envs[mode]), f"{name} {case} {mode} attributes step {t}")
        if name == "dispersion":
            eaten_any = eaten_any or any(bool(f.eaten.any()) for f in ref.world.landmarks)
        else:
            turned = turned or bool(ref.scenario.line.state.ang_vel.abs().max() > 0)
        # the in-place flags keep their memory across replays (a full reset re-binds them: from then on)
        if t == 10:
            ptrs = _flag_ptrs(name, envs["graph"])
    assert envs["fused"].scenario._fused_plan() is not None
    assert envs["graph"].graph_status == "graph", envs["graph"].graph_reason
    assert _flag_ptrs(name, envs["graph"]) == ptrs
    if num_envs >= 16:
        assert eaten_any if name == "dispersion" else turned


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", ALL_CASES)
def test_native_program_matches_torch_program_gpu(gpu_device, name, case):
    _twelve_steps(gpu_device, name, case, B, CASES[name][case])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["wheel", "dispersion"])
def test_native_program_one_env_gpu(gpu_device, name):
    _twelve_steps(gpu_device, name, "one env", 1, dict())


def _program(env, done):
    return env.get_from_scenario(get_observations=True, get_rewards=True, get_infos=False, get_dones=done)


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", ALL_CASES + [("dispersion", "five_foods"), ("dispersion", "penalise")])
def test_program_on_hand_placed_states_gpu(gpu_device, name, case):
    """The program alone, with no physics step between placing and evaluating, twice in a row (the
    second evaluation sees the flags the first left), against the torch program bit for bit; the cases
    are shown to fire on the CPU restatement's own outputs."""
    kw = {"five_foods": dict(n_food=5, n_agents=3), "penalise": dict(penalise_by_time=True)}.get(case) or CASES[name][case]
    envs = _mode_envs(gpu_device, name, ("torch", "fused"), B, seed=9, **kw)
    ref, fus = envs["torch"], envs["fused"]
    for env in (ref, fus):
        _spec(name).place_cases(env)
    spec = (WS.WheelSpec if name == "wheel" else DS.DispersionSpec)(ref)
    _spec(name).assert_cases_fired(spec, spec.run())
    for what in ("placed", "again"):
        with _Torch():
            exp = _program(ref, name == "dispersion")
        got = _program(fus, name == "dispersion")
        assert fus.scenario._fc is not None  # (the native launch ran)
        _assert_same(exp, got, f"{what} outputs")
        _assert_same(_attrs(name, ref), _attrs(name, fus), f"{what} attributes")
    if name == "dispersion":  # the device's flags are the spec's after its two steps
        spec.run()
        for l, f in enumerate(fus.world.landmarks):  # noqa: E741
            assert torch.equal(f.eaten.cpu(), spec.eaten[l]) and torch.equal(f.is_rendering.cpu(), spec.is_rendering[l])


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,why", [
    ("wheel", dict(n_agents=17), "torch: 17 agents"),
    ("dispersion", dict(n_agents=17, n_food=2), "torch: 17 agents"),
    ("dispersion", dict(n_agents=2, n_food=17), "torch: 17 foods"),
])
def test_over_the_cap_runs_the_torch_program_gpu(gpu_device, name, kw, why):
    envs = _mode_envs(gpu_device, name, ("torch", "fused"), B, **kw)
    ref, fus = envs["torch"], envs["fused"]
    assert _fused.enabled(fus.world) and fus.scenario._fused_plan() is None
    assert fus.scenario.fused_status.startswith(why), fus.scenario.fused_status
    for t in range(3):
        actions = ref.get_random_actions()
        with _Torch():
            exp = ref.step([a.clone() for a in actions])
        got = fus.step([a.clone() for a in actions])
        _assert_same(exp, got, f"outputs step {t}")
        _assert_same(_attrs(name, ref), _attrs(name, fus), f"attributes step {t}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["wheel", "dispersion"])
def test_discrete_actions_replay_gpu(gpu_device, name):
    envs = []
    for graph_step in (False, None):  # (None: the default make_env call)
        saved = _rng_save()
        envs.append(make_env(name, num_envs=B, device=gpu_device, seed=2, graph_step=graph_step, continuous_actions=False))
        if graph_step is False:
            _rng_load(saved)
    eager, graph = envs
    for t in range(8):
        actions = eager.get_random_actions()
        out_e = eager.step([a.clone() for a in actions])
        out_g = graph.step([a.clone() for a in actions])
        _assert_same(out_e, out_g, f"outputs step {t}")
        _assert_same(_state(eager), _state(graph), f"state step {t}")
        _assert_same(_attrs(name, eager), _attrs(name, graph), f"attributes step {t}")
    assert graph.graph_status == "graph", graph.graph_reason
    assert graph.scenario.fused_status == "native"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["wheel", "dispersion"])
def test_default_make_env_call_reaches_the_graph_gpu(gpu_device, name):
    env = make_env(name, num_envs=B, device=gpu_device, seed=0)
    for _ in range(6):
        env.step(env.get_random_actions())
    assert env.graph_status == "graph", env.graph_reason
    assert env.scenario.fused_status == "native"


@pytest.mark.gpu
def test_refused_actions_roll_the_flags_back_gpu(gpu_device):
    """A step whose actions fail the range check is rolled back: graph mode's per-step backup of the
    in-place flag rows (3 n_food bytes per env) restores them."""
    envs = []
    for graph_step in (False, True):
        saved = _rng_save()
        envs.append(make_env("dispersion", num_envs=B, device=gpu_device, seed=2, graph_step=graph_step))
        if graph_step is False:
            _rng_load(saved)
    eager, graph = envs
    g = torch.Generator().manual_seed(4)
    for t in range(8):
        actions = [(torch.rand(B, 2, generator=g) * 2 - 1).to(gpu_device) for _ in eager.agents]
        if t == 5:
            assert graph.graph_status == "graph", graph.graph_reason
            for env in envs:  # an agent on a fresh food in env 77: the refused step would eat it
                env.agents[0].set_pos(env.world.landmarks[0].state.pos.clone(), batch_index=None)
                env.world.landmarks[0].eaten.fill_(False)
                env.world.landmarks[0].is_rendering.fill_(True)
            bad = [a.clone() for a in actions]
            bad[1][77, 0] = 3.0
            before = [t_.clone() for t_ in DS.landmark_attributes(graph)[0::5] + DS.landmark_attributes(graph)[1::5]
                      + DS.landmark_attributes(graph)[2::5]], [a.state.pos.clone() for a in graph.agents]
            for env in envs:
                with pytest.raises(AssertionError):
                    env.step([a.clone() for a in bad])
            now = DS.landmark_attributes(graph)
            assert all(torch.equal(x, y) for x, y in zip(now[0::5] + now[1::5] + now[2::5], before[0]))
            assert not graph.world.landmarks[0].eaten.any()
            assert all(torch.equal(a.state.pos, p) for a, p in zip(graph.agents, before[1]))
        out_e = eager.step([a.clone() for a in actions])
        out_g = graph.step([a.clone() for a in actions])
        _assert_same(out_e, out_g, f"outputs step {t}")
        _assert_same(_state(eager), _state(graph), f"state step {t}")
        _assert_same(_attrs("dispersion", eager), _attrs("dispersion", graph), f"attributes step {t}")
        if t == 5:
            assert graph.world.landmarks[0].eaten.all()  # (the accepted step does eat it)
    assert graph.graph_status == "graph", graph.graph_reason


# ---- reset_where ---------------------------------------------------------------------------------------
def _masks(dev):
    one = lambda *idx: torch.zeros(B, dtype=torch.bool, device=dev).index_fill_(0, torch.tensor(idx, device=dev), True)  # noqa: E731
    return [("none", torch.zeros(B, dtype=torch.bool, device=dev)), ("first", one(0)), ("last", one(B - 1)),
            ("all", torch.ones(B, dtype=torch.bool, device=dev)), ("two", one(63, 64))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", [("wheel", dict()), ("wheel", dict(n_agents=1)), ("dispersion", dict()),
                                     ("dispersion", dict(n_agents=2, n_food=5))])
def test_reset_where_rows_of_a_full_reset_gpu(gpu_device, name, kw):
    dev = gpu_device
    _need_mode(dev, B)
    lib = N.load_library()
    for case, mask in _masks(dev):
        env, twin = R.twins(name, 2, B, dev, graph_step=False, **kw)
        if name == "dispersion":  # something eaten, so that the flags have rows to reset and to keep
            for e in (env, twin):
                DS.place_cases(e)
            R.step_all(dev, [env, twin])
            assert any(bool(f.eaten.any()) for f in env.world.landmarks)
        n0, w0 = env.scenario.native_resets, lib.vmas_host_waits()
        steps_before = env.steps.clone()
        R.check_rows_of_full_reset(env, twin, mask, mask, dev, return_dones=True)
        assert env.scenario.native_resets == n0 + 1, case  # (the launch answered: no fall-back)
        assert (lib.vmas_host_waits() - w0) & 0xFFFFFFFF == 0, case
        assert torch.equal(env.steps[~mask], steps_before[~mask]) and not env.steps[mask].any()
        R.check_next_step_agrees(env, twin, mask, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["wheel", "dispersion"])
def test_reset_where_between_graph_replays_gpu(gpu_device, name):
    dev = gpu_device
    _need_mode(dev, B)
    (eager, graph), _ = R.turns(dev, [False, True], lambda g: make_env(name, num_envs=B, device=dev, seed=1, graph_step=g))
    masks = {5: torch.arange(B, device=dev) % 4 == 1, 9: torch.arange(B, device=dev) == B - 1}
    for t in range(12):
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
        _assert_same(_attrs(name, eager), _attrs(name, graph), f"attributes step {t}")
        if t >= 3:
            assert graph.graph_status == "graph", (t, graph.graph_reason)
    assert graph._graph.replays >= 8


@pytest.mark.gpu
def test_uniform_reset_on_plain_tensors_across_a_grid_round_gpu(gpu_device):
    """vmas_uniform_reset with no env: one [B, 2] call and one [B, 1] call on a batch whose 2 B elements
    pass one round of torch's distribution grid (threads x 4 elements), so that elements 2 b and 2 b + 1
    are taken from later components and from the next philox round; a handful of rows, the last included,
    against torch's own uniform_ from the same offset."""
    dev = torch.device(gpu_device)
    idx = dev.index or 0
    props = torch.cuda.get_device_properties(dev)
    max_blocks = props.multi_processor_count * (props.max_threads_per_multi_processor // 256)
    step = 256 * max_blocks  # threads of the grid once it is full
    Bq = 2 * step + 3        # 2 B = 4 step + 6: the last rows are in the second round
    _need_mode(dev, Bq)
    mode = _uniform.mode(dev, Bq)
    rows = [0, 1, step // 2 - 1, step // 2, step, 2 * step - 1, 2 * step, Bq - 1]
    mask = torch.zeros(Bq, dtype=torch.bool, device=dev)
    mask[rows] = True
    f32 = dict(device=dev, dtype=torch.float32)
    ent = [{k: torch.full((Bq, w), 7.0, **f32) for k, w in (("pos", 2), ("vel", 2), ("rot", 1), ("ang_vel", 1))}
           for _ in range(2)]
    steps = torch.full((Bq,), 5.0, **f32)
    flag = torch.ones(Bq, dtype=torch.bool, device=dev)
    io = N.VmasUniformResetIO()
    io.batch, io.mode, io.n_draws = Bq, mode, 2
    for i, (target, lo, hi) in enumerate(((N.VMAS_UDRAW_POS, -1.0, 1.0), (N.VMAS_UDRAW_ROT, -0.5, 2.0))):
        d = io.draws[i]
        d.target, d.call, d.lo, d.hi = target, i, lo, hi
        for k, t in ent[i].items():
            v = getattr(d.entity, k)
            v.p, v.s0, v.s1 = t.data_ptr(), t.stride(0), t.stride(1)
    io.n_clear, io.clear[0] = 1, flag.data_ptr()
    io.mask, io.steps = mask.data_ptr(), steps.data_ptr()
    gen = torch.cuda.default_generators[idx]
    gen.manual_seed(1234)
    off = gen.get_offset()
    io.seed, io.offset = gen.initial_seed(), off
    inc = ctypes.c_uint64(0)
    N.check_aux(N.load_library().vmas_uniform_reset(idx, ctypes.byref(io), ctypes.byref(inc), N.stream_ptr(idx)),
                "vmas_uniform_reset")
    ref_pos = torch.empty(Bq, 2, **f32).uniform_(-1.0, 1.0)
    ref_rot = torch.empty(Bq, 1, **f32).uniform_(-0.5, 2.0)
    assert gen.get_offset() - off == inc.value  # the generator advance of the two calls
    assert torch.equal(ent[0]["pos"][mask], ref_pos[mask]) and torch.equal(ent[1]["rot"][mask], ref_rot[mask])
    assert not ent[1]["pos"][mask].any() and not ent[0]["rot"][mask].any()
    for e in ent:
        assert not e["vel"][mask].any() and not e["ang_vel"][mask].any()
        for t in e.values():
            assert (t[~mask] == 7.0).all()
    assert not steps[mask].any() and (steps[~mask] == 5.0).all()
    assert not flag[mask].any() and flag[~mask].all()


# ---- physics ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["wheel", "dispersion"])
def test_step_parity_gpu(gpu_device, name):
    env = make_env(name, num_envs=B, device=gpu_device, seed=2, graph_step=False)
    if name == "wheel":
        place_agents_on_the_line(env)
    reps = step_parity(env, 4)
    assert all(r["ok"] for r in reps), reps
    if name == "wheel":
        line = env.scenario.line.state
        assert line.ang_vel.abs().max() > 0 and not line.pos.any()
