"""Environment.reset_where(mask) of navigation, transport and discovery on a ROCm device: the native
spawn reset (vmas_spawn_reset: a k_reset_place launch per placed entity, one k_reset_commit launch).

The yardstick is ``reset()`` of a twin env at the same state and generator states
(tests/_reset_where.py), never reset_where itself.  Every case must really reject candidates -- a
reset whose envs all accept their first try would not tell a wrong generator offset from a right one
-- so the tries the twin's ``reset()`` consumed are read off the device generator and asserted.

The graph-mode test of the same call is in tests/test_spawn_reset_graph_gpu.py (its captures have to
come after test_jit.py and test_spawn.py, see there).
"""
import ctypes

import pytest
import torch

from tests import _reset_where as R
from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd.simulator import _fused
from vectorizedmultiagentsimulator_amd.simulator.environment import _uniform
from vectorizedmultiagentsimulator_amd.simulator.utils import ScenarioUtils

SKIPPED = [0]  # cases skipped because no vmas_uniform_columns mode equals torch (expected: 0)

# name -> (scenario, kwargs, E = the entities one reset places)
CONFIGS = {
    "navigation-2": ("navigation", dict(n_agents=2), 4),
    "navigation-4": ("navigation", dict(n_agents=4), 8),
    "navigation-8": ("navigation", dict(n_agents=8), 16),
    "navigation-same-goal": ("navigation", dict(n_agents=4, agents_with_same_goal=2, collisions=False), 8),
    "navigation-split-goals": ("navigation", dict(n_agents=4, agents_with_same_goal=2, split_goals=True,
                                                  collisions=False), 8),
    # 8 entities at 0.25 from each other in a 1 x 1 square: long try loops
    "navigation-tight": ("navigation", dict(n_agents=4, world_spawning_x=0.5, world_spawning_y=0.5), 8),
    "transport-1": ("transport", dict(n_packages=1), 6),
    "transport-2": ("transport", dict(n_packages=2), 7),
    "discovery": ("discovery", dict(), 12),
    "discovery-agent-lidar": ("discovery", dict(use_agent_lidar=True), 12),
}
TRIO = ([(c, B) for c in ("navigation-2", "navigation-4", "navigation-same-goal", "navigation-split-goals",
                          "transport-1", "transport-2", "discovery", "discovery-agent-lidar")
         for B in (1, 64, 65, 300)] + [("navigation-8", 65), ("navigation-tight", 300)])


def _need_mode(dev, B):
    torch.cuda.init()  # (the probe reads the device generator)
    if _uniform.mode(torch.device(dev), B) is None:
        SKIPPED[0] += 1
        print(f"reset_where spawn cases skipped: {SKIPPED[0]} (expected 0)")
        pytest.skip("no uniform mode equals torch on this device")
    print(f"reset_where spawn cases skipped: {SKIPPED[0]} (expected 0)")


def _offset(rng_state) -> int:
    """The philox offset of a device generator state (R.get_rng: seed, then offset, 8 bytes each)."""
    return int(rng_state[1][8:16].view(torch.int64).item())


def _per_try(dev, B) -> int:
    """The offset advance of one try: the x and the y draw, each one torch uniform_ call on B floats."""
    gen = torch.cuda.default_generators[torch.device(dev).index or 0]
    o0 = gen.get_offset()
    torch.empty(B, device=dev).uniform_()
    return 2 * (gen.get_offset() - o0)


def _resync(dev, envs):
    """Back to one common state: a full reset of every env from the same generator states, then
    two steps (which recompute the per-step attributes a reset leaves alone)."""
    R.turns(dev, envs, lambda e: e.reset())
    for _ in range(2):
        R.step_all(dev, envs)


@pytest.mark.gpu
@pytest.mark.parametrize("config,B", TRIO)
def test_native_spawn_rows_of_a_full_reset_gpu(gpu_device, config, B):
    """One trio of envs per world, every mask of the CPU test and the done envs: `native` resets
    through vmas_spawn_reset (native_resets counts the calls it answered), `generic` through the
    full reset and the k_masked_rows merge (the fused programs switched off for the call), `twin` is
    reset() -- all three from the same state and generator states.  native must equal the twin inside
    the mask and itself outside it, the generic path must leave the identical world, and the
    generators must end where reset() leaves them.  The single-row masks at B = 300 are the cases
    where an env outside the mask holds the batch's largest try count."""
    dev = gpu_device
    _need_mode(dev, B)
    scenario, kw, E = CONFIGS[config]
    per_try = _per_try(dev, B)
    assert per_try > 0
    native, generic, twin = envs = R.twins(scenario, 3, B, dev, max_steps=50, graph_step=False, **kw)
    cases = R.mask_cases(B) + [("none", None, None)]
    for name, arg, mask in cases:
        if arg is None:  # mask=None: the done envs -- some truncated by a forced step count
            for e in envs:
                e.steps[::3] = 50
            mask = twin.done().cpu()
            assert mask[0]
        mask_d = mask.to(dev)
        if isinstance(arg, torch.Tensor):
            arg = arg.to(dev)
        n0, g0 = native.scenario.native_resets, generic.scenario.native_resets
        f0 = native.scenario.native_reset_fallbacks
        before = R.snapshot(native)
        start = _offset(R.get_rng(dev))

        def call(i):
            if i == 0:
                return native.reset_where(arg)
            if i == 1:
                # (only the reset runs with the programs off: the observations it would return there
                # come from the torch program, whose LIDAR the fused one equals within the parity
                # tolerance, not bit for bit -- so they are asked for afterwards, as reset_where asks)
                with _fused.disabled():
                    generic.reset_where(arg, return_observations=False)
                return generic.get_from_scenario(get_observations=True, get_rewards=False, get_infos=False,
                                                 get_dones=False)[0]
            return twin.reset()

        (o_n, o_g, o_t), (r_n, r_g, r_t) = R.turns(dev, [0, 1, 2], call)
        assert native.scenario.native_resets == n0 + 1, name  # exactly one call, no silent fall-back
        assert native.scenario.native_reset_fallbacks == f0, name
        assert generic.scenario.native_resets == g0, name
        assert R.same_rng(r_n, r_t) and R.same_rng(r_g, r_t), name
        # the inputs really reject: reset() consumed more tries than one per entity
        tries = (_offset(r_t) - start) / per_try
        print(f"{config} B={B} {name}: reset() consumed {tries} tries for E={E}")
        assert tries == int(tries), name
        if B >= 64:
            assert tries > E, (name, tries)
        if config == "navigation-tight":
            assert tries >= 5 * E, (name, tries)
        s_n, s_g, s_t = R.batched_state(native), R.batched_state(generic), R.batched_state(twin)
        assert set(s_n) == set(s_g) == set(s_t) == set(before)
        for k in s_n:
            assert torch.equal(s_n[k][mask_d], s_t[k][mask_d]), (name, k, "masked rows differ from reset()")
            assert torch.equal(s_n[k][~mask_d], before[k][~mask_d]), (name, k, "rows outside the mask changed")
            assert torch.equal(s_n[k], s_g[k]), (name, k, "the generic path leaves another world")
        for x, y, z in zip(R.flat(o_n), R.flat(o_g), R.flat(o_t)):
            assert torch.equal(x, y), name
            assert torch.equal(x[mask_d], z[mask_d]), name
        a, b, c = R.step_all(dev, envs)
        rows = mask_d
        if scenario == "discovery":
            # Discovery's step respawns the targets covered in it by the same rejection sampling, whose
            # generator offsets follow the try counts of the WHOLE batch: where the twin's other envs
            # (freshly reset) differ from native's (untouched), an env that respawns a target draws other
            # positions, although its own state is the same.  Such envs are compared with the generic
            # path only (same world everywhere); every env that respawned nothing in this step must
            # equal the twin.
            respawned = ((native.scenario.covered_targets != 0).any(-1)
                         | (twin.scenario.covered_targets != 0).any(-1))
            rows = mask_d & ~respawned
            assert 2 * int(rows.sum()) >= int(mask_d.sum()), name
        for x, y, z in zip(R.flat(a), R.flat(b), R.flat(c)):
            assert torch.equal(x, y), name
            assert torch.equal(x[rows], z[rows]), name
        _resync(dev, envs)


@pytest.mark.gpu
def test_spawn_reset_falls_back_when_an_env_runs_out_of_tries_gpu(gpu_device):
    """max_tries = 1 in the tight world: some env rejects its first candidate, the launch chain
    reports it unresolved and writes nothing, and the generic path redoes the call from the same
    generator state -- the ordinary unresolved-count path."""
    dev = gpu_device
    B = 300
    _need_mode(dev, B)
    scenario, kw, E = CONFIGS["navigation-tight"]
    env, twin = R.twins(scenario, 2, B, dev, graph_step=False, **kw)
    env.scenario.spawn_max_tries = 1
    mask = torch.arange(B) % 3 == 1
    n0, f0 = env.scenario.native_resets, env.scenario.native_reset_fallbacks
    R.check_rows_of_full_reset(env, twin, mask.to(dev), mask, dev)  # (the world and the generators equal the twin's)
    assert env.scenario.native_resets == n0
    assert env.scenario.native_reset_fallbacks == f0 + 1
    # and with the limit lifted the same env resets natively again
    env.scenario.spawn_max_tries = 0
    _resync(dev, [env, twin])
    R.check_rows_of_full_reset(env, twin, mask.to(dev), mask, dev)
    assert env.scenario.native_resets == n0 + 1
    assert env.scenario.native_reset_fallbacks == f0 + 1


@pytest.mark.gpu
@pytest.mark.parametrize("B", [65, 300])
def test_fixed_positions_are_occupied_before_the_first_placement_gpu(gpu_device, B):
    """vmas_spawn_reset's fixed occupied positions (no scenario binds them yet): the placement chain
    alone, an empty mask, against spawn_entities_randomly(occupied_positions=...) from the same
    generator state -- the same positions for every env and the same generator advance."""
    dev = gpu_device
    _need_mode(dev, B)
    d = torch.device(dev)
    env = R.make_env("navigation", num_envs=B, device=dev, seed=3, n_agents=3, graph_step=False)
    w = env.world
    g = torch.Generator().manual_seed(5)
    fixed = [(torch.rand(B, 2, generator=g) - 0.5).to(dev) for _ in range(2)]
    min_dist, bounds, E = 0.3, (-0.5, 0.5), 3
    per_try = _per_try(dev, B)
    gen = torch.cuda.default_generators[d.index]
    state0 = torch.cuda.get_rng_state(d)
    off0 = gen.get_offset()
    ScenarioUtils.spawn_entities_randomly(w.agents, w, None, min_dist, bounds, bounds,
                                          occupied_positions=torch.stack(fixed, dim=1))
    want = [a.state.pos.clone() for a in w.agents]
    advance = gen.get_offset() - off0
    assert advance > E * per_try  # (candidates were rejected)
    torch.cuda.set_rng_state(state0, d)
    io = N.VmasSpawnResetIO()
    mask = torch.zeros(B, dtype=torch.bool, device=dev)
    scratch = torch.full((E, 2, B), float("nan"), device=dev)
    words = torch.zeros(N.VMAS_RESET_WORDS, dtype=torch.int32, device=dev)
    io.batch, io.mode, io.max_tries, io.n_place, io.n_fixed = B, _uniform.mode(d, B), 0, E, len(fixed)
    io.seed, io.offset = gen.initial_seed(), gen.get_offset()
    io.x_lo, io.x_hi, io.y_lo, io.y_hi = bounds[0], bounds[1], bounds[0], bounds[1]
    for i in range(E):
        io.min_dist[i] = min_dist
    for j, t in enumerate(fixed):
        io.fixed[j].p, io.fixed[j].s0, io.fixed[j].s1 = t.data_ptr(), t.stride(0), t.stride(1)
    io.mask, io.scratch, io.words = mask.data_ptr(), scratch.data_ptr(), words.data_ptr()
    inc, lost = ctypes.c_uint64(0), ctypes.c_int32(0)
    N.check_aux(N.load_library().vmas_spawn_reset(d.index, ctypes.byref(io), ctypes.byref(inc), ctypes.byref(lost),
                                                  N.stream_ptr(d.index)), "vmas_spawn_reset")
    torch.cuda.synchronize()
    assert lost.value == 0 and inc.value == advance
    for i in range(E):
        assert torch.equal(scratch[i].t(), want[i]), i
