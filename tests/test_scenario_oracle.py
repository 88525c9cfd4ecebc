"""The step's action path and the benchmark scenarios' per-step programs against the CPU oracle
(oracle/vmas_scenario_oracle.py; VERDICT r4 "Next" #1).

The oracle restates ``Environment._set_action`` / ``Holonomic.process_action`` and each scenario's
reward / observation / done / info from the reference's files; tests/_scenario_parity.py feeds it
the product's states and actions step by step and compares u, state.force and every output.

* CPU worlds (no GPU): the product's host path (native host backend + the scenarios' torch
  programs) against the oracle -- this is what pins the restatement itself;
* GPU worlds (``-m gpu``): the fused action launch (vmas_apply_actions / the pre-applied draw) and
  the fused scenario programs (k_balance, k_transport, k_discovery_*_fast, k_flocking_fast) at the
  BASELINE configs' full sizes, in graph mode (the bench's path) and eagerly; one ``PARITY`` line
  per config.
"""
import pytest
import torch

from oracle import vmas_scenario_oracle as SO
from tests._scenario_parity import ScenarioParity
from vectorizedmultiagentsimulator_amd import make_env

CASES = [
    ("balance", dict(n_agents=4), 10),
    ("transport", dict(n_agents=4), None),
    ("discovery", dict(n_agents=5, use_agent_lidar=True), None),
    ("flocking", dict(n_agents=5), None),
]


def _make(name, kw, substeps, device, envs, seed=0, **ekw):
    env = make_env(name, num_envs=envs, device=device, seed=seed, **kw, **ekw)
    if substeps is not None:
        env.world._substeps = substeps
        env.world._sub_dt = env.world._dt / substeps
    return env


def _run(env, name, kw, steps, config, actions=None, strict=False):
    sp = ScenarioParity(env, name, kw, strict=strict)
    for t in range(steps):
        sp.step(None if actions is None else actions(env, t))
    rec = sp.record(config)
    assert sp.ok, f"{sp.failures[:6]!r} {rec!r}"
    return rec


# ---- the oracle's action path on its own (reference semantics) ---------------------------------
def test_set_action_oracle_semantics():
    a = torch.tensor([[0.5, -1.0], [1.0, 0.25]])
    u, c = SO.set_action(a, action_size=2, u_range=1.0, u_multiplier=0.7)
    assert torch.equal(u, a * torch.tensor([0.7, 0.7])) and c is None
    with pytest.raises(AssertionError):  # environment.py:653-655
        SO.set_action(a * 2, action_size=2, u_range=1.0, u_multiplier=0.7)
    u, _ = SO.set_action(a * 2, action_size=2, u_range=1.0, u_multiplier=0.7, clamp_action=True)
    assert torch.equal(u, (a * 2).clamp(-1, 1) * 0.7)
    with pytest.raises(AssertionError):  # 621-623
        SO.set_action(torch.tensor([[float("nan"), 0.0]]), action_size=2, u_range=1.0, u_multiplier=1.0)
    # comm actions: clamped into the action, but the range assert reads the unclamped view (643, 739-743)
    a3 = torch.tensor([[0.5, 0.5, 0.3]])
    u, c = SO.set_action(a3, action_size=2, u_range=1.0, u_multiplier=1.0, dim_c=1, silent=False)
    assert torch.equal(c, a3[:, 2:])
    with pytest.raises(AssertionError):
        SO.set_action(torch.tensor([[0.5, 0.5, 1.5]]), action_size=2, u_range=1.0, u_multiplier=1.0, dim_c=1,
                      silent=False, clamp_action=True)
    assert torch.equal(SO.holonomic_process_action(torch.ones(3, 4)), torch.ones(3, 2))
    assert torch.equal(SO.lidar_angles(1, 4), torch.linspace(0, 2 * torch.pi, 5)[:4].unsqueeze(0))


# ---- CPU worlds: the product's host path vs the oracle -----------------------------------------
@pytest.mark.parametrize("name,kw,substeps", CASES, ids=[c[0] for c in CASES])
def test_scenario_programs_match_oracle_cpu(name, kw, substeps):
    env = _make(name, kw, substeps, "cpu", 96, seed=1)
    _run(env, name, kw, 6, f"{name} 96 envs cpu")


@pytest.mark.parametrize("name,kw,substeps", CASES[:2], ids=[c[0] for c in CASES[:2]])
def test_clamped_actions_match_oracle_cpu(name, kw, substeps):
    """clamp_actions=True with actions up to 3x the range (environment.py:635-646)."""
    env = _make(name, kw, substeps, "cpu", 64, seed=2, clamp_actions=True)
    g = torch.Generator().manual_seed(0)
    acts = lambda env, t: [torch.rand(64, 2, generator=g) * 6 - 3 for _ in env.agents]  # noqa: E731
    _run(env, name, kw, 3, f"{name} 64 envs cpu clamp", actions=acts)


@pytest.mark.parametrize("mutation", ["shaping", "u_multiplier", "covering_range"])
def test_oracle_catches_a_misread_program_cpu(mutation):
    """The checker is not vacuous: a product program that misreads one constant of the reference
    (balance's shaping factor, an agent's u_multiplier, discovery's covering range) fails."""
    name, kw, sub = {"shaping": CASES[0], "u_multiplier": CASES[1], "covering_range": CASES[2]}[mutation]
    env = _make(name, kw, sub, "cpu", 96, seed=1)
    sp = ScenarioParity(env, name, kw)
    if mutation == "shaping":
        env.scenario.shaping_factor = 99
    elif mutation == "u_multiplier":
        # (the product's per-column tensor, not the parameter the oracle reads)
        env.agents[1].action._u_multiplier_tensor = torch.tensor([0.61, 0.6])
    else:
        env.scenario._covering_range = 0.3
    for _ in range(4):
        sp.step()
    assert not sp.ok


# ---- the scenarios' construction, independently of the product (VERDICT r5 "Next" #4) -----------
BUILD_CASES = [
    ("balance", dict(n_agents=4)), ("transport", dict(n_agents=4)),
    ("discovery", dict(n_agents=8, use_agent_lidar=True)), ("flocking", dict(n_agents=8)),
    ("balance", {}), ("transport", dict(n_agents=3, n_packages=2)), ("discovery", {}), ("flocking", {}),
]


@pytest.mark.parametrize("name,kw", BUILD_CASES, ids=[f"{c[0]}-{'-'.join(f'{k}{v}' for k, v in c[1].items())}"
                                                     for c in BUILD_CASES])
def test_make_env_world_matches_reference_construction_cpu(name, kw):
    """Every world / entity / agent / LIDAR constant a benchmark scenario's make_world sets (world
    dt, substeps, drag, collision force, gravity, semidims; each entity's shape, mass, movable /
    rotatable / collide; each agent's u_multiplier, u_range and LIDARs) equals the oracle's table,
    restated from the reference's files with their file:line (oracle/vmas_scenario_oracle.py
    scenario_construction)."""
    env = make_env(name, num_envs=4, device="cpu", seed=0, **kw)
    bad = SO.construction_mismatches(SO.scenario_construction(name, **kw), SO.world_construction(env.world))
    assert not bad, bad


def _line(env):
    return next(e for e in env.world.entities if e.name == "line")


MUTATIONS = {
    "line_length": ("balance", lambda env: setattr(_line(env).shape, "_length", 0.81)),
    "agent_radius": ("balance", lambda env: setattr(env.agents[0].shape, "_radius", 0.031)),
    "u_multiplier": ("transport", lambda env: setattr(env.agents[2].action, "_u_multiplier", 0.61)),
    "collision_force": ("discovery", lambda env: setattr(env.world, "_collision_force", 499.0)),
    "substeps": ("flocking", lambda env: setattr(env.world, "_substeps", 4)),
    "lidar_range": ("flocking", lambda env: setattr(env.agents[1].sensors[0], "_max_range", 0.21)),
    "package_mass": ("balance", lambda env: setattr(env.world.landmarks[1], "_mass", 5.5)),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_construction_pin_catches_a_misread_constant_cpu(mutation):
    """Not vacuous: one constant of a product world changed after make_world (as a misread constant
    in a product scenario would leave it) fails the comparison, naming the field."""
    name, mutate = MUTATIONS[mutation]
    kw = dict(n_agents=4)
    env = make_env(name, num_envs=4, device="cpu", seed=0, **kw)
    assert not SO.construction_mismatches(SO.scenario_construction(name, **kw), SO.world_construction(env.world))
    mutate(env)
    bad = SO.construction_mismatches(SO.scenario_construction(name, **kw), SO.world_construction(env.world))
    assert len(bad) == 1, bad


# ---- GPU worlds: fused actions + fused scenario programs vs the oracle ---------------------------
FULL = [
    ("balance", dict(n_agents=4), 10, 32768, "C2"),
    ("transport", dict(n_agents=4), None, 32768, "C3"),
    ("discovery", dict(n_agents=8, use_agent_lidar=True), None, 16384, "C4"),
    ("flocking", dict(n_agents=8), None, 32768, "C5 shard"),
    ("flocking", dict(n_agents=8), None, 262144, "C5 full"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,substeps,envs,cfg", FULL, ids=[c[4].replace(" ", "_") for c in FULL])
def test_scenario_programs_match_oracle_full_size_gpu(gpu_device, name, kw, substeps, envs, cfg):
    """The bench's path (graph mode: captured step, pre-applied random draws, fused programs with
    direct outputs) at the BASELINE config's full size: 6 steps (2 eager, capture, replays)."""
    env = _make(name, kw, substeps, gpu_device, envs, graph_step=True)
    rec = _run(env, name, kw, 6, f"{cfg} {name} {envs} envs graph: actions + scenario program vs oracle")
    assert env.graph_status == "graph", env.graph_reason
    assert rec["lidar"]["uncertified_rows"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,substeps,envs,cfg", [FULL[2], FULL[4]], ids=["C4", "C5_full"])
def test_exact_lidar_matches_oracle_without_certification_gpu(gpu_device, monkeypatch, name, kw, substeps, envs, cfg):
    """VERDICT r5 "Next" #3: the same full-size runs with the exact LIDAR (_fused.EXACT_LIDAR: library
    sin / cos, the k_cast_rays arithmetic) and every certification tier off (strict: no ray-turn,
    no scan, no band) -- 0 LIDAR rows outside the tolerance, so what the fast LIDAR's certified rows
    differ by is its hardware trig alone."""
    from vectorizedmultiagentsimulator_amd.simulator import _fused

    monkeypatch.setattr(_fused, "EXACT_LIDAR", True)
    env = _make(name, kw, substeps, gpu_device, envs, graph_step=True)
    rec = _run(env, name, kw, 6, f"{cfg} {name} {envs} envs graph, exact LIDAR, no certification: "
                                 "actions + scenario program vs oracle", strict=True)
    assert env.graph_status == "graph", env.graph_reason
    assert rec["lidar"]["bad_rows"] == 0 and rec["lidar"]["rows"] > 0, rec["lidar"]


@pytest.mark.gpu
def test_fast_trig_direction_error_is_bounded_gpu(gpu_device):
    """The fast LIDAR's ray direction (v_sin / v_cos_f32 of the fp32 angle, |a| < 16 rad) against
    float64 cos / sin of the same fp32 angle, over 2^24 evenly spread angles plus the multiples of
    pi / 4: its largest error bounds how far the scan certification may turn the oracle's ray
    (tests/_scenario_parity.py FAST_TRIG_DIR_ERR = SCAN_DELTA)."""
    import json

    from tests import _scenario_parity as P
    from vectorizedmultiagentsimulator_amd import _native as N

    n = 1 << 24
    x = torch.linspace(-16.0, 16.0, n, dtype=torch.float64)
    k = torch.arange(-20, 21, dtype=torch.float64) * (torch.pi / 4)
    x = torch.cat([x, k[k.abs() < 16]]).to(torch.float32)
    xd = x.to(gpu_device)
    out = torch.empty(2 * x.numel(), device=gpu_device)
    dev = torch.device(gpu_device).index or 0
    N.check(N.load_library().vmas_test_fast_trig(dev, xd.data_ptr(), out.data_ptr(), x.numel(),
                                                   N.stream_ptr(dev)), "vmas_test_fast_trig")
    o = out.cpu().double()
    s_hw, c_hw = o[:x.numel()], o[x.numel():]
    xs = x.double()
    err = torch.sqrt((s_hw - torch.sin(xs)) ** 2 + (c_hw - torch.cos(xs)) ** 2)
    small = xs.abs() <= 2 * torch.pi
    rec = {"probe": "fast LIDAR direction error (v_sin / v_cos_f32 vs float64)", "angles": int(x.numel()),
           "max_err_le_2pi": float(err[small].max()), "max_err_le_16": float(err.max()),
           "analytic_reduction_bound_16": 16 * 2.0 ** -23, "bound": P.FAST_TRIG_DIR_ERR}
    print("FASTTRIG " + json.dumps(rec))
    from tests import _parity

    _parity.SUMMARY.append({"config": "fast LIDAR trig bound", "envs": 0, **rec})  # (a PARITY line)
    assert float(err.max()) <= P.FAST_TRIG_DIR_ERR, rec


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,substeps", CASES, ids=[c[0] for c in CASES])
def test_scenario_programs_match_oracle_eager_gpu(gpu_device, name, kw, substeps):
    """The eager default (make_env without graph_step): the fused action launch and programs."""
    env = _make(name, kw, substeps, gpu_device, 4096, seed=4)
    _run(env, name, kw, 4, f"{name} 4096 envs eager: actions + scenario program vs oracle")


@pytest.mark.gpu
def test_clamped_actions_match_oracle_gpu(gpu_device):
    env = _make("balance", dict(n_agents=4), 10, gpu_device, 32768, seed=2, clamp_actions=True, graph_step=True)
    g = torch.Generator().manual_seed(0)
    acts = lambda env, t: [(torch.rand(32768, 2, generator=g) * 6 - 3).to(gpu_device) for _ in env.agents]  # noqa: E731
    _run(env, "balance", dict(n_agents=4), 5, "C2 balance 32768 envs graph clamp_actions: actions vs oracle",
         actions=acts)


def test_c1_plumbing_balance_128_envs_cpu():
    """BASELINE configs[0] (C1): make_env('balance', num_envs=128, n_agents=4) on CPU, 200 random
    steps -- every step's actions, observations, rewards, dones and infos against the oracle, and
    every 25th step the physics itself (teacher-forced World.step, oracle/vmas_oracle.py)."""
    from oracle import vmas_oracle as O

    env = make_env("balance", num_envs=128, device="cpu", seed=0, n_agents=4)
    sp = ScenarioParity(env, "balance", dict(n_agents=4))
    phys = []
    for t in range(200):
        sp.step()
        if t % 25 == 24:
            phys.append(O.compare_one_step(env.world))  # (an extra World.step: the shaping carried by
            # both sides is still the last reward's, as the reference's would be)
    rec = sp.record("C1 balance 128 envs cpu 200 steps: actions + scenario program + physics vs oracle")
    rec["physics_bad_envs"] = sum(r["bad_envs"] for r in phys)
    assert sp.ok, f"{sp.failures[:6]!r} {rec!r}"
    assert all(r["ok"] for r in phys), phys


def test_lidar_scan_certification_cpu():
    """tests/_scenario_parity._scan_certify runs and is not vacuous: a row moved 1e-3 off the
    oracle is not certified, the oracle's own row is."""
    from oracle import vmas_oracle as O
    from tests._scenario_parity import _scan_certify

    env = _make("flocking", dict(n_agents=5), None, "cpu", 64, seed=3)
    for _ in range(3):
        env.step(env.get_random_actions())
    snap = O.snapshot(env.world)
    prog = SO.program("flocking", env.world)
    ai = env.world.entities.index(env.world.policy_agents[0])
    ow = O.OracleWorld(env.world, snap)
    exp, rays = prog.lidar.measure(ow, ai)
    idx = torch.arange(8)
    bad = torch.zeros_like(exp, dtype=torch.bool)
    bad[:8, 0] = True
    assert _scan_certify(env.world, snap, idx, ai, rays, prog.lidar, exp, bad).all()
    off = exp.clone()
    off[:8, 0] = torch.where(exp[:8, 0] < 0.2, exp[:8, 0] + 1e-3, exp[:8, 0] - 1e-3)
    assert not _scan_certify(env.world, snap, idx, ai, rays, prog.lidar, off, bad).any()


# ---- shapes, options and branches that random steps at the default kwargs never reach ------------
# The GPU tests of the fused programs (tests/test_fused_edges.py) take the scenarios' torch programs
# as their bit-exact reference, so those programs are held to the oracle here at the same shapes
# (caps, cap + 1, one agent, several packages, both reward modes, both LIDARs, ray counts off the
# unrolled forms) and on hand-placed states that force each branch (tests/_scenario_places.py).
SHAPES = [
    ("balance", dict(n_agents=2)), ("balance", dict(n_agents=5)), ("balance", dict(n_agents=32)),
    ("balance", dict(n_agents=33)),
    ("transport", dict(n_agents=1, n_packages=1)), ("transport", dict(n_agents=3, n_packages=2)),
    ("transport", dict(n_agents=16, n_packages=8)), ("transport", dict(n_agents=2, n_packages=9)),
    ("discovery", dict(n_agents=1, n_targets=1, agents_per_target=1)),
    ("discovery", dict(n_agents=3, n_targets=4, targets_respawn=False, shared_reward=True, time_penalty=-0.01,
                       agents_per_target=1)),
    ("discovery", dict(n_agents=3, n_targets=2, time_penalty=-1)),
    ("discovery", dict(n_agents=16, n_targets=16, use_agent_lidar=True)),
    ("discovery", dict(n_agents=7, n_targets=3, use_agent_lidar=True, n_lidar_rays_entities=17,
                       n_lidar_rays_agents=5)),
    ("discovery", dict(n_agents=10, n_targets=7)),  # 17 entities
    ("flocking", dict(n_agents=1, n_obstacles=0)), ("flocking", dict(n_agents=2, n_obstacles=0)),
    ("flocking", dict(n_agents=3, n_obstacles=1)), ("flocking", dict(n_agents=4, n_obstacles=8)),
    ("flocking", dict(n_agents=7, n_obstacles=9)), ("flocking", dict(n_agents=15, n_obstacles=16, n_lidar_rays=5)),
    ("flocking", dict(n_agents=4, n_obstacles=17)), ("flocking", dict(n_agents=4, n_obstacles=5, n_lidar_rays=17)),
    ("flocking", dict(n_agents=4, n_obstacles=5, collision_reward=0)),
]


def _case_id(case):
    return case[0] + "-" + "-".join(f"{k}{v}" for k, v in case[1].items())


@pytest.mark.parametrize("name,kw", SHAPES, ids=[_case_id(c) for c in SHAPES])
def test_scenario_shapes_and_options_match_oracle_cpu(name, kw):
    env = _make(name, kw, None, "cpu", 65, seed=1)
    _run(env, name, kw, 3, f"{_case_id((name, kw))} 65 envs cpu")


PLACED = [
    ("balance", dict(n_agents=3)),
    ("transport", dict(n_agents=3, n_packages=1)), ("transport", dict(n_agents=2, n_packages=3)),
    ("discovery", dict(n_agents=4, n_targets=3)),
    ("discovery", dict(n_agents=4, n_targets=2, targets_respawn=False)),
    ("discovery", dict(n_agents=3, n_targets=4, shared_reward=True, time_penalty=-0.01, agents_per_target=1)),
    ("discovery", dict(n_agents=1, n_targets=1, agents_per_target=1)),
    ("flocking", dict(n_agents=3)), ("flocking", dict(n_agents=1, n_obstacles=2)),
    ("flocking", dict(n_agents=2, n_obstacles=0)),
]


@pytest.mark.parametrize("name,kw", PLACED, ids=[_case_id(c) for c in PLACED])
def test_programs_on_hand_placed_states_match_oracle_cpu(name, kw):
    """The "true" side of every branch: the program alone on the placed state (no step between
    placing and evaluating: a step moves the state off what was placed -- the world's bounds clamp
    balance's lowered line back above the floor, covered targets respawn), then two random steps
    from there, through discovery's respawn of the covered targets.  The placement's masks hold on
    the product's outputs, each flag true in some env and false in another."""
    from tests import _scenario_places as P

    env = _make(name, kw, None, "cpu", 65, seed=5)
    sp = ScenarioParity(env, name, kw)
    masks = P.place(name, env)
    out, exp = sp.evaluate()
    flags = P.observed(name, env, out)
    P.check(masks, flags, f"{name} program only")
    if name == "transport" and kw["n_packages"] > 1:  # one package on, another off, in the same env
        assert (flags["on_goal_0"] & ~flags["on_goal_1"]).any()
    if name == "discovery" and not kw.get("targets_respawn", True):
        assert out[2][16:24].all() and not out[2].all()  # (done: both targets covered at some time)
    assert sp.ok and sp.rec["certified_envs"] == 0, sp.rec  # (no placed env within MARGIN_TOL of a threshold)
    for _ in range(2):
        sp.step()
    rec = sp.record(f"{_case_id((name, kw))} 65 envs cpu, hand-placed")
    assert sp.ok, f"{sp.failures[:6]!r} {rec!r}"
    if name == "discovery" and kw.get("targets_respawn", True):
        assert rec["respawn"]["respawned"] >= 8 and rec["respawn"]["bad_envs"] == 0, rec


def test_program_entry_points_refuse_bad_arguments():
    """Counts over a cap, a sum mode that is no power of two and a non-sphere flocking agent are
    refused with VMAS_E_INVALID before any device call (so no GPU is needed and nothing is
    launched).  Each struct is otherwise acceptable: with the counts in range the entry point gets
    past its argument gate and names the deliberately wrong shape / index instead."""
    import ctypes

    from vectorizedmultiagentsimulator_amd import _native as N

    lib = N.load_library()
    VMAS_E_INVALID = -1

    def refused(fn, io, message):
        assert getattr(lib, fn)(0, ctypes.byref(io), None) == VMAS_E_INVALID, fn
        assert message in lib.vmas_aux_last_error(), (fn, lib.vmas_aux_last_error())

    b = N.VmasBalanceIO()
    b.batch, b.n_agents, b.what = 4, 2, N.VMAS_SCN_OBS
    refused("vmas_balance_outputs", b, b"unexpected entity shapes")  # (the gate passed)
    b.n_agents = N.VMAS_SCN_MAX_AGENTS + 1
    refused("vmas_balance_outputs", b, b"bad arguments")

    t = N.VmasTransportIO()
    t.batch, t.n_agents, t.n_packages, t.what = 4, 2, 1, N.VMAS_SCN_OBS
    t.package[0].shape = t.goal[0].shape = N.VMAS_SPHERE
    refused("vmas_transport_outputs", t, b"package 0 is not (box, sphere goal)")
    t.n_agents = N.VMAS_TRANSPORT_MAX_AGENTS + 1
    refused("vmas_transport_outputs", t, b"bad arguments")
    t.n_agents, t.n_packages = 2, N.VMAS_TRANSPORT_MAX_PACKAGES + 1
    refused("vmas_transport_outputs", t, b"bad arguments")

    d = N.VmasDiscoveryIO()
    d.batch, d.n_agents, d.n_targets, d.n_entities, d.n_lidars, d.what = 4, 1, 1, 2, 1, N.VMAS_SCN_OBS
    d.agent_entity[0] = -1
    refused("vmas_discovery_outputs", d, b"bad agent index 0")
    d.n_targets = N.VMAS_DISC_MAX_TARGETS + 1
    refused("vmas_discovery_outputs", d, b"bad arguments")

    f = N.VmasFlockingIO()
    f.batch, f.n_all, f.n_policy, f.target, f.n_rays, f.n_ray_targets, f.sum_mode = 4, 3, 2, 0, 12, 1, 2
    f.what = N.VMAS_SCN_OBS
    for i in range(3):
        f.agents[i].shape = N.VMAS_SPHERE
    f.agents[1].shape = N.VMAS_BOX
    refused("vmas_flocking_outputs", f, b"agent 1 is not a sphere")
    f.agents[1].shape = N.VMAS_SPHERE
    f.n_ray_targets = N.VMAS_SCN_MAX_RAY_TARGETS + 1
    refused("vmas_flocking_outputs", f, b"bad arguments")
    f.n_ray_targets, f.sum_mode = 1, 3
    refused("vmas_flocking_outputs", f, b"bad arguments")
    f.sum_mode = 2
    f.ray_targets[0].shape = N.VMAS_BOX  # (back past the gate: the counts above were what it refused)
    refused("vmas_flocking_outputs", f, b"LIDAR target 0 is not a sphere")
