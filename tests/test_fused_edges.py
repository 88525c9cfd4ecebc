"""The fused balance / transport / discovery / flocking programs (csrc/vmas_scenarios.hip,
csrc/vmas_programs.hpp) on gfx950 where random steps at the default kwargs never take them: the
"true" side of every branch on hand-placed states (tests/_scenario_places.py), the stand-alone
k_balance / k_transport next to the world module's k_program_jit and k_world's epilogue, several
packages, discovery's options, every dispatch of the flocking and discovery LIDAR kernels, the
caps, the torch fallback over them, and batches of 1 and 64.  The reference is the scenario's own
torch program (held to the CPU oracle at the same shapes and states by
tests/test_scenario_oracle.py): outputs, scenario attributes and world state bit-identical.
130 envs: two full waves plus a partial one."""
import pytest
import torch

from tests import _scenario_places as P
from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd import make_env
from vectorizedmultiagentsimulator_amd.simulator import _fused

from test_fused import FUSED, _NullCtx, _Torch
from test_fused import _attrs as _named_attrs
from test_graph import _assert_same, _rng_load, _rng_save, _state

B = 130
_ATTRS = {c[0]: c[3] for c in FUSED}
_EPILOGUE = {"balance": N.EPILOGUE_BALANCE, "transport": N.EPILOGUE_TRANSPORT}


def _attrs(env, name, kw):
    names = list(_ATTRS[name])
    if name == "discovery":
        if not kw.get("use_agent_lidar", False):
            names.remove("agent.sensors.1._last_measurement")
        names.append("all_time_covered_targets")
    return _named_attrs(env, names)


def _mode_envs(gpu_device, name, kw, modes, num_envs=B, seed=3):
    """One env per mode (torch: the torch program; fused: eager; graph: replayed), the same seed
    and generator states."""
    envs = {}
    for mode in modes:
        saved = _rng_save()
        with _Torch() if mode == "torch" else _NullCtx():
            envs[mode] = make_env(name, num_envs=num_envs, device=gpu_device, seed=seed,
                                  graph_step=mode == "graph", **kw)
        if mode != modes[-1]:
            _rng_load(saved)
    return envs


def _each(envs, fn):
    """fn(env) in every mode's env from the same generator states (resets and respawns draw);
    returns {mode: result}."""
    out = {}
    modes = list(envs)
    for mode in modes:
        s = _rng_save()
        with _Torch() if mode == "torch" else _NullCtx():
            out[mode] = fn(envs[mode])
        if mode != modes[-1]:
            _rng_load(s)
    return out


def _assert_modes_same(envs, outs, name, kw, what):
    ref = envs["torch"]
    for mode in envs:
        if mode == "torch":
            continue
        _assert_same(outs["torch"], outs[mode], f"{what} {mode} outputs")
        _assert_same(_state(ref), _state(envs[mode]), f"{what} {mode} state")
        _assert_same(_attrs(ref, name, kw), _attrs(envs[mode], name, kw), f"{what} {mode} attributes")


def _program(env):
    return env.get_from_scenario(get_observations=True, get_rewards=True, get_infos=True, get_dones=True)


def _falls_back(env, name) -> bool:
    """The scenario's own predicate for keeping its torch program on a GPU world."""
    sc = env.scenario
    return not sc._fused_ok() if name in ("balance", "transport") else sc._fused_plan() is None


# ---- a. hand-placed states, the program alone ------------------------------------------------------
PLACED = {
    "balance": ("balance", dict(n_agents=4)),
    "transport": ("transport", dict(n_agents=4)),
    "transport_2_packages": ("transport", dict(n_agents=4, n_packages=2)),
    "discovery": ("discovery", dict(n_agents=5, use_agent_lidar=True)),
    "discovery_no_respawn": ("discovery", dict(n_agents=4, n_targets=2, targets_respawn=False)),
    "discovery_shared_time_penalty": ("discovery", dict(n_agents=5, shared_reward=True, time_penalty=-0.01)),
    "flocking": ("flocking", dict(n_agents=5)),
}
# how a balance / transport program is launched: the world module's k_program_jit (default), or
# the stand-alone k_balance / k_transport when the module holds no program or does not exist
VARIANTS = {"default": {}, "no_epilogue": {"VMAS_JIT_EPILOGUE": "0"}, "no_jit": {"VMAS_JIT": "0"}}
PLACED_RUNS = [(c, "default") for c in PLACED] + [(c, v) for c in ("balance", "transport", "transport_2_packages")
                                                  for v in ("no_epilogue", "no_jit")]


@pytest.mark.gpu
@pytest.mark.parametrize("case,variant", PLACED_RUNS, ids=[f"{c}-{v}" for c, v in PLACED_RUNS])
def test_program_on_hand_placed_states_gpu(gpu_device, monkeypatch, case, variant):
    """No step between placing and evaluating: every placed env sits where its branch fires.  (One
    random step first: the engine, and with it the world module and its k_program_jit, exists from
    the first physics step on; before it every program call is the stand-alone kernel's.)"""
    monkeypatch.setattr(_fused, "EXACT_LIDAR", True)  # (LIDAR bit-identical to World.cast_rays)
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    name, kw = PLACED[case]
    envs = _mode_envs(gpu_device, name, kw, ("torch", "fused"))
    ref, fus = envs["torch"], envs["fused"]
    actions = ref.get_random_actions()
    _each(envs, lambda env: env.step([a.clone() for a in actions]))
    masks = {mode: P.place(name, env) for mode, env in envs.items()}
    outs = _each(envs, _program)
    assert _fused.enabled(fus.world) and not _falls_back(fus, name)
    if name in _EPILOGUE:  # (which kernel ran)
        assert (fus.world.engine.jit_program(_EPILOGUE[name]) is not None) == (variant == "default")
    _assert_modes_same(envs, outs, name, kw, f"{case} {variant} placed")
    flags = P.observed(name, ref, outs["torch"])
    P.check(masks["torch"], flags, case)
    if case == "transport_2_packages":  # one package on, the other off, in the same env
        assert (flags["on_goal_0"] & ~flags["on_goal_1"]).any()
    if case == "discovery_no_respawn":  # both targets covered at some time: done
        assert outs["torch"][2][16:24].all() and not outs["torch"][2].all()
    # a second evaluation: the carried shaping / all-time flags / respawned targets of the first
    outs = _each(envs, _program)
    _assert_modes_same(envs, outs, name, kw, f"{case} {variant} placed, again")


# ---- b. hand-placed states through steps, eagerly and replayed ------------------------------------------
STEPPED = ["balance", "transport_2_packages", "discovery", "discovery_no_respawn", "flocking"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", STEPPED)
def test_placed_states_through_steps_gpu(gpu_device, monkeypatch, case):
    """8 steps, the placement at t = 2 (the step the graph env captures), reset_at(7) at t = 4,
    reset() at t = 6: k_world's epilogue through the true branches, discovery's respawn of covered
    targets inside the graph, the all-time flags carried across reset_at."""
    monkeypatch.setattr(_fused, "EXACT_LIDAR", True)
    name, kw = PLACED[case]
    envs = _mode_envs(gpu_device, name, kw, ("torch", "fused", "graph"))
    ref = envs["torch"]
    for t in range(8):
        actions = ref.get_random_actions()

        def one(env):
            if t == 2:
                P.place(name, env)
            if t == 4:
                env.reset_at(7)
            if t == 6:
                env.reset()
            return env.step([a.clone() for a in actions])

        if t == 2:
            before = ref.scenario._targets[0].state.pos.clone() if name == "discovery" else None
        outs = _each(envs, one)
        _assert_modes_same(envs, outs, name, kw, f"{case} step {t}")
        if t == 2:  # the placed envs reach the program behind a physics step
            done = outs["torch"][2]
            if case == "discovery":  # (done needs targets_respawn=False) target 0 covered, and respawned
                cov = ref.scenario.covered_targets[:, 0]
                assert cov[0:8].any() and not cov.all()
                assert ((ref.scenario._targets[0].state.pos != before).any(-1) == cov).all()
            elif case == "flocking":  # (no done) a charged collision
                hit = outs["torch"][3][0]["agent_collision_rew"] != 0
                assert hit.any() and not hit.all()
            else:
                assert done.any() and not done.all()
    assert envs["graph"].graph_status == "graph", envs["graph"].graph_reason


# ---- c. the shape matrix ----------------------------------------------------------------------------
# (scenario, kwargs, how): "graph" also replayed from a graph, "eager" not.  "no_jit": eager with
# VMAS_JIT=0 -- the cap-size worlds, one per scenario, whose world modules take 12 to 31 s to compile
# (profiles/r14/fused_edges/README.md): the generic step kernel, the programs as the stand-alone
# kernels (balance, transport) or the scenario's own launches, which is what these cases are about.
SHAPES = [
    ("balance", dict(n_agents=2), "graph"), ("balance", dict(n_agents=5), "graph"), ("balance", dict(n_agents=32), "no_jit"),
    ("transport", dict(n_agents=1, n_packages=1), "graph"), ("transport", dict(n_agents=3, n_packages=2), "graph"),
    ("transport", dict(n_agents=16, n_packages=8), "no_jit"),
    ("discovery", dict(n_agents=1, n_targets=1, agents_per_target=1), "graph"),
    ("discovery", dict(n_agents=3, n_targets=4, targets_respawn=False, shared_reward=True, time_penalty=-0.01,
                       agents_per_target=1), "graph"),
    ("discovery", dict(n_agents=3, n_targets=2, time_penalty=-1), "graph"),
    ("discovery", dict(n_agents=16, n_targets=16, use_agent_lidar=True), "no_jit"),
    ("discovery", dict(n_agents=7, n_targets=3, use_agent_lidar=True, n_lidar_rays_entities=17,
                       n_lidar_rays_agents=5), "eager"),
    ("discovery", dict(n_agents=10, n_targets=7), "eager"),  # 17 entities
    ("flocking", dict(n_agents=1, n_obstacles=0), "graph"), ("flocking", dict(n_agents=2, n_obstacles=0), "graph"),
    ("flocking", dict(n_agents=3, n_obstacles=1), "graph"), ("flocking", dict(n_agents=4, n_obstacles=8), "graph"),
    ("flocking", dict(n_agents=7, n_obstacles=9), "eager"),
    ("flocking", dict(n_agents=15, n_obstacles=16, n_lidar_rays=5), "no_jit"),
    ("flocking", dict(n_agents=4, n_obstacles=5, n_lidar_rays=17), "graph"),
    ("flocking", dict(n_agents=4, n_obstacles=5, collision_reward=0), "graph"),
]
OVER_CAP = [
    ("balance", dict(n_agents=N.VMAS_SCN_MAX_AGENTS + 1)),
    ("transport", dict(n_agents=2, n_packages=N.VMAS_TRANSPORT_MAX_PACKAGES + 1)),
    ("discovery", dict(n_agents=3, n_targets=N.VMAS_DISC_MAX_TARGETS + 1)),
    ("flocking", dict(n_agents=4, n_obstacles=N.VMAS_SCN_MAX_RAY_TARGETS + 1)),
    ("flocking", dict(n_agents=N.VMAS_FLOCK_MAX_AGENTS, n_obstacles=1)),  # 16 policy agents + the target
]


def _case_id(case):
    return case[0] + "-" + "-".join(f"{k}{v}" for k, v in case[1].items())


def _random_steps(envs, name, kw, what, steps=4, place_at=1):
    ref = envs["torch"]
    for t in range(steps):
        actions = ref.get_random_actions()

        def one(env):
            if t == place_at:
                P.place(name, env)
            return env.step([a.clone() for a in actions])

        outs = _each(envs, one)
        _assert_modes_same(envs, outs, name, kw, f"{what} step {t}")
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,how", SHAPES, ids=[_case_id(c) for c in SHAPES])
def test_shapes_and_options_match_torch_program_gpu(gpu_device, monkeypatch, name, kw, how):
    """4 random steps, the hand placement at t = 1."""
    monkeypatch.setattr(_fused, "EXACT_LIDAR", True)
    if how == "no_jit":
        monkeypatch.setenv("VMAS_JIT", "0")
    graph = how == "graph"
    envs = _mode_envs(gpu_device, name, kw, ("torch", "fused", "graph") if graph else ("torch", "fused"))
    _random_steps(envs, name, kw, _case_id((name, kw)))
    assert not _falls_back(envs["fused"], name)
    if graph:
        assert envs["graph"].graph_status == "graph", envs["graph"].graph_reason


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", OVER_CAP, ids=[_case_id(c) for c in OVER_CAP])
def test_over_the_caps_runs_the_torch_program_gpu(gpu_device, monkeypatch, name, kw):
    """One past a cap of the argument block: the scenario keeps its torch program (no launch with
    a count the entry point would refuse) and the outputs are the torch env's.  (VMAS_JIT=0: the
    fallback is the scenario's; a world module for 37 entities takes 35 s to compile.)"""
    monkeypatch.setattr(_fused, "EXACT_LIDAR", True)
    monkeypatch.setenv("VMAS_JIT", "0")
    envs = _mode_envs(gpu_device, name, kw, ("torch", "fused"))
    fus = envs["fused"]
    assert _fused.enabled(fus.world) and _falls_back(fus, name)
    outs = _random_steps(envs, name, kw, _case_id((name, kw)), steps=3)
    assert len(outs["fused"][0]) == len(fus.agents)


BATCH_EDGES = [("balance", dict(n_agents=3)), ("discovery", dict(n_agents=3, n_targets=3, use_agent_lidar=True))]


@pytest.mark.gpu
@pytest.mark.parametrize("num_envs", [1, 64])
@pytest.mark.parametrize("name,kw", BATCH_EDGES, ids=[c[0] for c in BATCH_EDGES])
def test_batch_of_one_and_of_a_full_wave_gpu(gpu_device, monkeypatch, name, kw, num_envs):
    """Batch 1 (every other lane of the wave clamps onto env 0) and exactly 64 (no partial wave),
    the program alone after a reset(); at 64 on the hand-placed state."""
    monkeypatch.setattr(_fused, "EXACT_LIDAR", True)
    envs = _mode_envs(gpu_device, name, kw, ("torch", "fused"), num_envs=num_envs)
    _each(envs, lambda env: env.reset())
    if num_envs >= 64:
        masks = {mode: P.place(name, env) for mode, env in envs.items()}
    outs = _each(envs, _program)
    assert not _falls_back(envs["fused"], name)
    _assert_modes_same(envs, outs, name, kw, f"{name} batch {num_envs}")
    assert outs["fused"][0][0].shape[0] == num_envs and outs["fused"][2].shape == (num_envs,)
    if num_envs >= 64:
        P.check(masks["torch"], P.observed(name, envs["torch"], outs["torch"]), name)


# ---- d. the fast LIDAR at the dispatches the 4096-env tests do not select -------------------------------
FAST_LIDAR = [
    ("flocking", dict(n_agents=4, n_obstacles=0)),  # k_flocking_fast<0, 0>, no target
    ("flocking", dict(n_agents=4, n_obstacles=1)),  # <12, 1>
    ("flocking", dict(n_agents=4, n_obstacles=8)),  # <12, 8>
    ("flocking", dict(n_agents=4, n_obstacles=9)),  # k_flocking (more targets than the fast form takes)
    ("flocking", dict(n_agents=4, n_obstacles=5, n_lidar_rays=5)),  # <0, 0>, the runtime ray count
    ("discovery", dict(n_agents=5, use_agent_lidar=True)),  # k_discovery_obs_split<2>, a wave pair without an agent
    ("discovery", dict(n_agents=10, n_targets=7)),  # 17 entities: k_discovery_obs
    ("discovery", dict(n_agents=4, n_targets=3, n_lidar_rays_entities=17)),  # 17 rays: k_discovery_obs
]
_LIDAR_COLS = {"flocking": 6, "discovery": 4}  # the observation's first LIDAR column


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", FAST_LIDAR, ids=[_case_id(c) for c in FAST_LIDAR])
def test_fast_lidar_dispatches_gpu(gpu_device, monkeypatch, name, kw):
    """The default (fast) LIDAR: every output but the rays bit-identical to the torch program, the
    measured rays against the CPU oracle's World.cast_rays on the same state with the LIDAR
    tolerance and certification of tests/_parity.py lidar_parity, as they are."""
    from tests._parity import lidar_parity

    monkeypatch.setattr(_fused, "EXACT_LIDAR", False)
    envs = _mode_envs(gpu_device, name, kw, ("torch", "fused"))
    ref, fus = envs["torch"], envs["fused"]
    c0 = _LIDAR_COLS[name]
    for t in range(4):
        actions = ref.get_random_actions()

        def one(env):
            if t == 1:
                P.place(name, env)
            return env.step([a.clone() for a in actions])

        outs = _each(envs, one)
        for a, ot, of in zip(fus.world.policy_agents, outs["torch"][0], outs["fused"][0]):
            assert ot.shape == of.shape and torch.equal(ot[:, :c0], of[:, :c0]), (t, a.name)
            # the observation holds the measurements the sensors keep
            assert torch.equal(of[:, c0:], torch.cat([s._last_measurement for s in a.sensors], dim=-1)), (t, a.name)
        _assert_same(outs["torch"][1:], outs["fused"][1:], f"rewards / dones / infos step {t}")
        _assert_same(_state(ref), _state(fus), f"state step {t}")
        rep = lidar_parity(fus, measured=True)
        assert rep["ok"] and rep["rows"] > 0, (t, rep)
    assert not _falls_back(fus, name)
