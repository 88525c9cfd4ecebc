"""The sampling scenario's native programs (csrc/vmas_scenarios.hip k_sampling /
k_sampling_max_pdf) on gfx950: bit-identical to the scenario's torch program eagerly and replayed
from a HIP graph (rewards, infos, observations, flags, positions, max_pdf), the fast LIDAR within the
LIDAR tolerance, the torch fallback over the agent cap, the normalisation against the literal loop,
reset_where in graph mode, and the torch program on the device against MultivariateNormal.
130 envs: two full waves plus a partial one."""
import pytest
import torch

from tests._sampling_spec import CASE_ENVS, SamplingSpec, assert_cases_fired, place_cases, scenario_attributes
from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd import make_env
from vectorizedmultiagentsimulator_amd.simulator import _fused

from test_fused import _NullCtx, _Torch
from test_graph import _assert_same, _rng_load, _rng_save, _state
from test_sampling import SMALL, density_tolerance

B = 130

CASES = {
    "default": dict(),
    "one_agent": dict(n_agents=1),
    "small_grid_one_gaussian": dict(n_gaussians=1, **SMALL),
    "cov_list_own_no_norm": dict(cov=[0.05, 0.1, 0.2, 0.07], n_gaussians=4, shared_rew=False, norm=False),
}


def _attrs(env):
    out = scenario_attributes(env) + list(env.scenario.locs)
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
            envs[mode] = make_env("sampling", num_envs=num_envs, device=gpu_device, seed=seed,
                                  graph_step=mode == "graph", **kw)
        if mode != modes[-1]:
            _rng_load(saved)
    return envs


def _twelve_steps(gpu_device, case, num_envs, kw):
    envs = _mode_envs(gpu_device, ("torch", "fused", "graph"), num_envs, **kw)
    ref = envs["torch"]
    assert envs["fused"].scenario.fused_status == "native", envs["fused"].scenario.fused_status
    ptr = envs["graph"].scenario.sampled.data_ptr()
    for t in range(12):
        actions = ref.get_random_actions()
        outs = {}
        for mode, env in envs.items():
            s = _rng_save()
            with _Torch() if mode == "torch" else _NullCtx():
                if t == 2 and num_envs >= 44:
                    place_cases(env)
                if t == 5:
                    env.reset_at(min(7, num_envs - 1))
                if t == 9:
                    env.reset()
                outs[mode] = env.step([a.clone() for a in actions])
            if mode != "graph":
                _rng_load(s)
        for mode in ("fused", "graph"):
            _assert_same(outs["torch"], outs[mode], f"{case} {mode} outputs step {t}")
            _assert_same(_state(ref), _state(envs[mode]), f"{case} {mode} state step {t}")
            _assert_same(_attrs(ref), _attrs(envs[mode]), f"{case} {mode} attributes step {t}")
    assert envs["fused"].scenario._fused_plan() is not None
    assert envs["graph"].graph_status == "graph", envs["graph"].graph_reason
    # the flags are written in place: a replay neither copies nor re-allocates them
    assert envs["graph"].scenario.sampled.data_ptr() == ptr
    assert ref.scenario.sampled.any()


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_native_program_matches_torch_program_gpu(gpu_device, monkeypatch, case):
    monkeypatch.setattr(_fused, "EXACT_LIDAR", True)  # (LIDAR bit-identical to World.cast_rays)
    _twelve_steps(gpu_device, case, B, CASES[case])


@pytest.mark.gpu
def test_native_program_one_env_gpu(gpu_device, monkeypatch):
    monkeypatch.setattr(_fused, "EXACT_LIDAR", True)
    _twelve_steps(gpu_device, "one env", 1, dict())


def _program(env):
    return env.get_from_scenario(get_observations=True, get_rewards=True, get_infos=True, get_dones=False)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("config", ["default", "own_rewards_five_agents", "small_grid"])
def test_program_on_hand_placed_states_gpu(gpu_device, monkeypatch, config, fast):
    """The program alone, with no physics step between placing and evaluating: the hand-placed
    shared cell, beyond-the-semidim, out-of-bounds, sampled-before, border and marked-neighbour envs
    (each shown to fire by the CPU restatement's own outputs), then once more on the state the first
    evaluation left."""
    from tests._parity import lidar_parity

    monkeypatch.setattr(_fused, "EXACT_LIDAR", not fast)
    kw = {"default": dict(), "own_rewards_five_agents": dict(shared_rew=False, n_agents=5),
          "small_grid": dict(n_gaussians=2, **SMALL)}[config]
    envs = _mode_envs(gpu_device, ("torch", "fused"), B, seed=9, **kw)
    ref, fus = envs["torch"], envs["fused"]
    for env in (ref, fus):
        place_cases(env)
    spec = SamplingSpec(ref)
    before = spec.sampled.clone()
    assert_cases_fired(spec, spec.run(), before)
    for what in ("placed", "again"):
        with _Torch():
            exp = _program(ref)
        got = _program(fus)
        assert fus.scenario._fc is not None  # (the native launch ran)
        if fast:  # (the LIDAR columns within the tolerance, certified by lidar_parity)
            for e, g in zip(exp[0], got[0]):
                assert torch.equal(e[:, :4], g[:, :4]) and torch.equal(e[:, 16:], g[:, 16:]), what
            rep = lidar_parity(fus, measured=True)
            assert rep["ok"], rep
            exp, got = exp[1:], got[1:]
        _assert_same(exp, got, f"{what} outputs")
        _assert_same(scenario_attributes(ref), scenario_attributes(fus), f"{what} attributes")
    r = list(CASE_ENVS["b_beyond_semidim"])
    assert (fus.agents[0].sample[r] == 0).all()  # (left where it was: the cell it sampled a step ago)


@pytest.mark.gpu
def test_over_the_agent_cap_runs_the_torch_program_gpu(gpu_device):
    kw = dict(n_agents=N.VMAS_SAMPLING_MAX_AGENTS + 1)
    envs = _mode_envs(gpu_device, ("torch", "fused"), B, **kw)
    ref, fus = envs["torch"], envs["fused"]
    assert _fused.enabled(fus.world) and fus.scenario._fused_plan() is None
    assert fus.scenario.fused_status.startswith("torch: 17 agents")
    for t in range(3):
        actions = ref.get_random_actions()
        with _Torch():
            exp = ref.step([a.clone() for a in actions])
        got = fus.step([a.clone() for a in actions])
        _assert_same(exp, got, f"outputs step {t}")
        _assert_same(scenario_attributes(ref), scenario_attributes(fus), f"attributes step {t}")
    assert got[0][0].shape == (B, 24)


@pytest.mark.gpu
def test_unsafe_grid_runs_the_torch_program_gpu(gpu_device):
    """agent_radius 1e-9 (the semidim rounds to the dimension): a clamped position indexes past the
    grid (the reference raises there); the native program is refused with that reason."""
    from vectorizedmultiagentsimulator_amd.scenarios import load

    scn = load("sampling.py").Scenario()
    scn.env_make_world(4, torch.device(gpu_device), agent_radius=1e-9)
    assert scn._fused_plan() is None and "index past the grid" in scn.fused_status


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["one_gaussian", "cov_list"])
def test_max_pdf_kernel_against_the_literal_loop_gpu(gpu_device, config):
    """vmas_sampling_max_pdf on the 8 x 4 grid: bit-identical to the torch program's normalisation
    and to the literal loop run on the device, with the full mask and with a partial one (the other
    rows untouched)."""
    kw = dict(n_gaussians=1, **SMALL) if config == "one_gaussian" else dict(cov=[0.05, 0.2], n_gaussians=2, **SMALL)
    envs = _mode_envs(gpu_device, ("torch", "fused"), B, **kw)
    ref, fus = envs["torch"].scenario, envs["fused"].scenario
    assert fus.fused_status == "native"
    assert torch.equal(ref.max_pdf, fus.max_pdf)
    # the literal loop, on the device, with the torch program's sample()
    loop = torch.zeros(B, device=gpu_device)
    saved = ref.sampled.clone()
    ref.sampled[:] = False
    xs, ys = ref._grid_points()
    with _Torch():
        for x in xs:
            for y in ys:
                pos = torch.stack([x, y]).repeat(B, 1)
                loop = torch.maximum(loop, ref.sample(pos, norm=False))
    ref.sampled.copy_(saved)
    assert torch.equal(loop, fus.max_pdf)
    # and the MultivariateNormal spec's loop on the CPU, within the density tolerance
    spec = SamplingSpec(envs["fused"])
    pts = torch.stack(torch.meshgrid(xs.cpu(), ys.cpu(), indexing="ij"), dim=-1).reshape(1, -1, 2).expand(B, -1, -1).clone()
    pts[..., 0].clamp_(-fus.x_semidim, fus.x_semidim)
    pts[..., 1].clamp_(-fus.y_semidim, fus.y_semidim)
    ref64, tol, ok = density_tolerance(spec.locs, fus.covs, pts)
    best = ref64.max(dim=1).values
    err = (fus.max_pdf.cpu().double() - best).abs() / best
    print(f"device max_pdf against fp64: tolerance {tol:.3e}, worst {float(err.max()):.3e}")
    assert (err <= tol).all()
    # a partial mask: one env
    want = fus.max_pdf.clone()
    fus.max_pdf[:] = -1.0
    assert fus._native_max_pdf(xs, ys, 129)
    assert fus.max_pdf[129] == want[129] and (fus.max_pdf[:129] == -1).all()
    fus.max_pdf[:] = -1.0
    assert fus._native_max_pdf(xs, ys, None)
    assert torch.equal(fus.max_pdf, want)


@pytest.mark.gpu
def test_reset_where_keeps_replaying_gpu(gpu_device, monkeypatch):
    monkeypatch.setattr(_fused, "EXACT_LIDAR", True)  # (LIDAR bit-identical to World.cast_rays)
    envs = _mode_envs(gpu_device, ("torch", "graph"), B)
    ref, graph = envs["torch"], envs["graph"]
    mask = torch.zeros(B, dtype=torch.bool, device=gpu_device)
    mask[torch.arange(B) % 3 == 1] = True
    ptr = graph.scenario.sampled.data_ptr()
    for t in range(9):
        actions = ref.get_random_actions()
        outs = []
        for mode, env in envs.items():
            s = _rng_save()
            with _Torch() if mode == "torch" else _NullCtx():
                if t == 5:
                    before = env.scenario.max_pdf.clone(), env.scenario.sampled.clone()
                    env.reset_where(mask)
                    assert torch.equal(env.scenario.max_pdf[~mask], before[0][~mask])
                    assert torch.equal(env.scenario.sampled[~mask], before[1][~mask])
                    assert not env.scenario.sampled[mask].any()
                outs.append(env.step([a.clone() for a in actions]))
            if mode != "graph":
                _rng_load(s)
        _assert_same(outs[0], outs[1], f"outputs step {t}")
        _assert_same(_state(ref), _state(graph), f"state step {t}")
        _assert_same(_attrs(ref), _attrs(graph), f"attributes step {t}")
    assert graph.graph_status == "graph", graph.graph_reason
    assert graph._graph.replays > 0 and graph.scenario.sampled.data_ptr() == ptr


@pytest.mark.gpu
def test_discrete_actions_replay_gpu(gpu_device):
    envs = []
    for graph_step in (False, None):
        saved = _rng_save()
        envs.append(make_env("sampling", num_envs=B, device=gpu_device, seed=1, continuous_actions=False,
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
    env = make_env("sampling", num_envs=B, device=gpu_device, seed=0)
    ptr = env.scenario.sampled.data_ptr()
    for _ in range(6):
        obs, rew, done, info = env.step(env.get_random_actions())
    assert env.graph_status == "graph", env.graph_reason
    assert env.scenario.fused_status == "native"
    assert env.scenario.sampled.data_ptr() == ptr and env.scenario.sampled.any()
    # the info tensors after a replay are the scenario's
    assert torch.equal(info[2]["agent_sample"], env.agents[2].sample)
    assert torch.equal(rew[0], env.scenario.sampling_rew)
    assert env.render(mode="rgb_array", env_index=129).shape[-1] == 3


@pytest.mark.gpu
def test_torch_program_on_the_device_against_multivariate_normal_gpu(gpu_device):
    """The scenario's torch program on the device against the CPU restatement with
    MultivariateNormal: flags, cells, positions and the zeros the flags require exactly; pdf values
    within the density tolerance (2 E, E the reference's own fp32 error against fp64 over the test's
    points); the LIDAR within the LIDAR tolerance."""
    import inspect

    from tests._parity import lidar_parity

    atol = inspect.signature(lidar_parity).parameters["atol"].default
    rtol = inspect.signature(lidar_parity).parameters["rtol"].default
    with _Torch():
        env = make_env("sampling", num_envs=B, device=gpu_device, seed=5, graph_step=False)
        for _ in range(3):
            env.step(env.get_random_actions())
        place_cases(env)
        spec = SamplingSpec(env)
        exp = spec.run()
        obs, rewards, infos = _program(env)
    scn = env.scenario
    assert torch.equal(scn.sampled.cpu(), spec.sampled)
    s = scn.grid_spacing
    deltas = torch.tensor([[0, 0], [s, 0], [-s, 0], [0, s], [0, -s], [-s, -s], [s, -s], [-s, s], [s, s]], dtype=torch.float32)
    mp = spec.max_pdf.double()
    worst = tol_seen = 0.0
    for j, a in enumerate(env.agents):
        pos = a.state.pos.cpu()
        assert torch.equal(pos, spec.world.agents[j].state.pos)
        pts = pos[:, None, :] + deltas[None]
        pts[..., 0].clamp_(-scn.x_semidim, scn.x_semidim)
        pts[..., 1].clamp_(-scn.y_semidim, scn.y_semidim)
        ref64, tol, ok = density_tolerance(spec.locs, scn.covs, pts)
        o, e = obs[j].cpu(), exp["obs"][j]
        assert torch.equal(o[:, :4], e[:, :4])
        assert ((o[:, 4:16] - e[:, 4:16]).abs() <= atol + rtol * e[:, 4:16].abs()).all()
        for name, got, want, r64, m in (("sample", infos[j]["agent_sample"].cpu(), exp["infos"][j]["agent_sample"],
                                         ref64[:, 0] / mp, ok[:, 0]),
                                        ("probes", o[:, 16:], e[:, 16:], ref64[:, 1:] / mp[:, None], ok[:, 1:])):
            assert torch.equal(got == 0, want == 0), name  # zeros required by the flags are exact
            live = m & (want != 0)
            err = ((got.double() - r64).abs() / r64)[live]
            worst, tol_seen = max(worst, float(err.max())), max(tol_seen, tol)
            assert (err <= tol).all(), (name, float(err.max()), tol)
    print(f"device torch program against fp64 MultivariateNormal: tolerance {tol_seen:.3e}, worst {worst:.3e}")


@pytest.mark.gpu
def test_refused_actions_roll_the_flags_back_gpu(gpu_device):
    """A replay keeps no per-step copy of ``sampled``: a step whose actions fail the range check is
    rolled back from the native program's undo log (the cells the step marked)."""
    envs = []
    for graph_step in (False, True):
        saved = _rng_save()
        envs.append(make_env("sampling", num_envs=B, device=gpu_device, seed=2, graph_step=graph_step))
        if graph_step is False:
            _rng_load(saved)
    eager, graph = envs
    g = torch.Generator().manual_seed(4)
    for t in range(8):
        actions = [(torch.rand(B, 2, generator=g) * 2 - 1).to(gpu_device) for _ in eager.agents]
        if t == 5:
            assert graph.graph_status == "graph", graph.graph_reason
            assert all(t_ is not graph.scenario.sampled for t_ in graph._graph._inplace)
            bad = [a.clone() for a in actions]
            bad[1][77, 0] = 3.0
            before = graph.scenario.sampled.clone(), [a.state.pos.clone() for a in graph.agents]
            for env in envs:
                with pytest.raises(AssertionError):
                    env.step([a.clone() for a in bad])
            assert torch.equal(graph.scenario.sampled, before[0])
            assert all(torch.equal(a.state.pos, p) for a, p in zip(graph.agents, before[1]))
        out_e = eager.step([a.clone() for a in actions])
        out_g = graph.step([a.clone() for a in actions])
        _assert_same(out_e, out_g, f"outputs step {t}")
        _assert_same(_state(eager), _state(graph), f"state step {t}")
        _assert_same(_attrs(eager), _attrs(graph), f"attributes step {t}")
    assert graph.graph_status == "graph", graph.graph_reason
