"""The sampling scenario (scenarios/sampling.py) on CPU worlds: construction, the torch program
against the independent restatement of the reference (tests/_sampling_spec.py: MultivariateNormal,
the literal per-agent flag order, the literal normalisation loop), the reset's draw order,
reset_at / reset_where, and the library's host backend of the two native programs."""
import ctypes
import inspect

import pytest
import torch
from torch.distributions import MultivariateNormal

from tests import _reset_where as R
from tests._parity import lidar_parity
from tests._sampling_spec import CASE_ENVS, SamplingSpec, assert_cases_fired, place_cases, scenario_attributes
from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd import make_env

LIDAR_ATOL = inspect.signature(lidar_parity).parameters["atol"].default
LIDAR_RTOL = inspect.signature(lidar_parity).parameters["rtol"].default

SMALL = dict(xdim=0.5, ydim=0.25, grid_spacing=0.125)  # 8 x 4 cells: an x / y transposition shows


def density_tolerance(locs, covs, pts):
    """The density tolerance, taken from the reference computation: E = the largest relative error
    of fp32 MultivariateNormal against fp64 MultivariateNormal over ``pts`` [B, P, 2] (points whose
    fp64 density is at least 2^-100); a value passes within 2 E of fp64 (one differently rounded exp
    and division on top of the reference's own error).  Returns (fp64 density [B, P], 2 E, mask)."""
    ref64 = torch.zeros(pts.shape[:2], dtype=torch.float64)
    ref32 = torch.zeros(pts.shape[:2], dtype=torch.float32)
    for loc, cov in zip(locs, covs):
        cm = torch.tensor([[cov, 0], [0, cov]], dtype=torch.float32)
        loc = loc.detach().cpu()
        ref32 += MultivariateNormal(loc[:, None, :], covariance_matrix=cm).log_prob(pts).exp()
        ref64 += MultivariateNormal(loc.double()[:, None, :], covariance_matrix=cm.double()).log_prob(pts.double()).exp()
    ok = ref64 >= 2.0 ** -100
    E = float(((ref32.double() - ref64).abs() / ref64)[ok].max())
    return ref64, 2 * E, ok


def test_make_env_builds_sampling():
    env = make_env("sampling", num_envs=8, device="cpu", seed=0)
    scn = env.scenario
    obs = env.reset()
    assert len(obs) == 3 and all(o.shape == (8, 24) for o in obs)
    assert scn.sampled.shape == (8, 40, 40) and scn.sampled.dtype is torch.bool
    assert scn.max_pdf.shape == (8,) and (scn.max_pdf > 0).all()
    assert len(scn.locs) == 3 and all(loc.shape == (8, 2) for loc in scn.locs)
    assert env.world.x_semidim == 1 - 0.025 and env.world.y_semidim == 1 - 0.025
    for a in env.agents:
        assert a.collide and a._render_action and len(a.sensors) == 1 and a.sensors[0]._angles.shape == (8, 12)
        assert a.sensors[0]._max_range == 0.2 and a.sample.shape == (8,)
    g = scn.gaussians
    assert len(g) == 3 and all(isinstance(d, MultivariateNormal) for d in g)
    assert torch.equal(g[1].loc, scn.locs[1]) and torch.equal(g[1].covariance_matrix, scn.cov_matrices[1])
    obs, rew, done, info = env.step(env.get_random_actions())
    assert set(info[0]) == {"agent_sample"} and rew[0].shape == (8,) and not done.any()
    assert torch.equal(rew[0], scn.sampling_rew) and torch.equal(rew[1], rew[0])
    env = make_env("sampling", num_envs=4, device="cpu", seed=0, **SMALL, n_gaussians=2, cov=[0.05, 0.1])
    assert env.scenario.sampled.shape == (4, 8, 4) and env.scenario.covs == [0.05, 0.1]


def test_asserts_and_unknown_kwargs():
    with pytest.raises(AssertionError):
        make_env("sampling", num_envs=2, device="cpu", spawn_same_pos=True)  # (with collisions)
    with pytest.raises(AssertionError):
        make_env("sampling", num_envs=2, device="cpu", grid_spacing=0.3)
    with pytest.raises(AssertionError):
        make_env("sampling", num_envs=2, device="cpu", cov=[0.05, 0.05])  # (three Gaussians)
    with pytest.warns(UserWarning):
        make_env("sampling", num_envs=2, device="cpu", no_such_kwarg=1)


def test_observation_without_collisions_raises():
    with pytest.raises((IndexError, TypeError)):
        make_env("sampling", num_envs=2, device="cpu", collisions=False)


def test_density_equals_multivariate_normal_bit_for_bit():
    env = make_env("sampling", num_envs=64, device="cpu", seed=3, cov=[0.05, 0.02, 0.3])
    scn = env.scenario
    g = torch.Generator().manual_seed(1)
    for _ in range(8):
        pts = (torch.rand(64, 2, generator=g) * 2 - 1) * 1.1
        ref = torch.stack([d.log_prob(pts).exp() for d in scn.gaussians], dim=-1).sum(-1)
        assert torch.equal(scn._density(pts), ref)


CONFIGS = {
    "default": dict(),
    "one_agent": dict(n_agents=1),
    "own_rewards": dict(shared_rew=False),
    "no_norm": dict(norm=False),
    "cov_list_own_no_norm": dict(cov=[0.05, 0.1, 0.2, 0.07], n_gaussians=4, shared_rew=False, norm=False),
    "small_grid": dict(n_gaussians=1, **SMALL),
}


def _check_against_spec(env, spec, exp):
    obs, rewards, infos = env.get_from_scenario(get_observations=True, get_rewards=True, get_infos=True,
                                                get_dones=False)
    B = env.num_envs
    for r, e in zip(rewards, exp["rewards"]):
        assert torch.equal(r, e)
    for i, e in zip(infos, exp["infos"]):
        assert set(i) == set(e) and torch.equal(i["agent_sample"], e["agent_sample"])
    for k, (x, e) in enumerate(zip(scenario_attributes(env), spec.attributes())):
        assert x.dtype == e.dtype and torch.equal(x, e), k
    for o, e in zip(obs, exp["obs"]):
        assert o.shape == e.shape == (B, 24)
        assert torch.equal(o[:, :4], e[:, :4]) and torch.equal(o[:, 16:], e[:, 16:])
        lo, le = o[:, 4:16], e[:, 4:16]
        assert ((lo - le).abs() <= LIDAR_ATOL + LIDAR_RTOL * le.abs()).all()


@pytest.mark.parametrize("config", list(CONFIGS))
def test_torch_program_matches_the_spec(config):
    kw = CONFIGS[config]
    env = make_env("sampling", num_envs=64, device="cpu", seed=5, **kw)
    for _ in range(3):
        env.step(env.get_random_actions())
    # random steps first, then the hand-placed cases (each shown to fire by the spec's own outputs),
    # then once more on the state the first evaluation left (flags set, positions clamped)
    spec = SamplingSpec(env)
    exp = spec.run()
    _check_against_spec(env, spec, exp)
    place_cases(env)
    spec = SamplingSpec(env)
    before = spec.sampled.clone()
    exp = spec.run()
    assert_cases_fired(spec, exp, before)
    _check_against_spec(env, spec, exp)
    spec = SamplingSpec(env)
    exp = spec.run()
    r = list(CASE_ENVS["b_beyond_semidim"])
    assert (exp["infos"][0]["agent_sample"][r] == 0).all()  # (case d without a hand-set flag: left where it was)
    _check_against_spec(env, spec, exp)


@pytest.mark.parametrize("config", ["small_grid", "cov_list_small"])
def test_max_pdf_equals_the_literal_loop(config):
    kw = dict(n_gaussians=1, **SMALL) if config == "small_grid" else dict(cov=[0.05, 0.2], n_gaussians=2, **SMALL)
    env = make_env("sampling", num_envs=16, device="cpu", seed=2, **kw)
    scn = env.scenario
    assert torch.equal(scn.max_pdf, SamplingSpec(env).max_pdf_loop())
    env.step(env.get_random_actions())
    env.reset_at(3)  # (one env only: the same value as the loop's row, flags set elsewhere or not)
    assert torch.equal(scn.max_pdf, SamplingSpec(env).max_pdf_loop())
    assert not scn.sampled[3].any()


def test_full_reset_draw_order():
    """Per Gaussian x then y, then per agent x then y, [B, 1] each; spawn_same_pos draws all the same."""
    from vectorizedmultiagentsimulator_amd.scenarios import load

    B = 16
    # (the scenario alone: without collisions the observation of an Environment's reset raises)
    for kw in (dict(), dict(spawn_same_pos=True, collisions=False)):
        scn = load("sampling.py").Scenario()
        scn.env_make_world(B, torch.device("cpu"), **kw)
        saved = torch.random.get_rng_state()
        torch.manual_seed(7)
        scn.env_reset_world_at(None)
        got = torch.random.get_rng_state()
        torch.manual_seed(7)
        cols = [torch.zeros(B, 1).uniform_(-1, 1) for _ in range(2 * 3)]
        spawn = 0 if kw else 1
        cols += [torch.zeros(B, 1).uniform_(-spawn, spawn) for _ in range(2 * 3)]
        end = torch.random.get_rng_state()
        torch.random.set_rng_state(saved)
        assert torch.equal(end, got)  # (the generator is where these twelve draws leave it)
        for i in range(3):
            assert torch.equal(scn.locs[i], torch.cat(cols[2 * i:2 * i + 2], dim=1))
            p = torch.cat(cols[6 + 2 * i:8 + 2 * i], dim=1).clamp(-0.975, 0.975)  # (sample() clamps the spawn)
            assert torch.equal(scn.world.agents[i].state.pos, p)
            assert (p == 0).all() == bool(kw)
        assert not scn.sampled.any() and (scn.max_pdf > 0).all()


def test_reset_at_leaves_other_rows():
    env = make_env("sampling", num_envs=16, device="cpu", seed=4)
    for _ in range(2):
        env.step(env.get_random_actions())
    before = R.snapshot(env)
    env.reset_at(5)
    now = R.batched_state(env)
    keep = torch.ones(16, dtype=torch.bool)
    keep[5] = False
    changed = 0
    for k, v in now.items():
        if k.endswith(".sample"):
            continue  # (the reference re-binds agent.sample for the whole batch in reset_at: below)
        assert torch.equal(v[keep], before[k][keep]), k
        changed += int(not torch.equal(v[5], before[k][5]))
    assert changed > 0
    scn = env.scenario
    assert not scn.sampled[5].any() and scn.sampled[keep].any()
    for a in env.agents:  # every env stands on a cell it sampled in the last step, but the reset one
        assert (a.sample[keep] == 0).all() and a.sample[5] != 0


@pytest.mark.parametrize("case", [c[0] for c in R.mask_cases(16)])
def test_reset_where_rows_of_a_full_reset_cpu(case):
    env, twin = R.twins("sampling", 2, 16, "cpu")
    _, arg, mask = next(c for c in R.mask_cases(16) if c[0] == case)
    R.check_rows_of_full_reset(env, twin, arg, mask, "cpu")
    assert torch.equal(env.steps, torch.where(mask, 0.0, 3.0))
    for e in (env, twin):  # (locs are views of the batched tensor the merge wrote)
        assert all(loc.data_ptr() == e.scenario._locs[:, i].data_ptr() for i, loc in enumerate(e.scenario.locs))
    assert all(torch.equal(a[mask], b[mask]) for a, b in zip(env.scenario.locs, twin.scenario.locs))
    R.check_next_step_agrees(env, twin, mask, "cpu")


def test_extra_render_lines():
    from vectorizedmultiagentsimulator_amd.simulator import rendering

    env = make_env("sampling", num_envs=4, device="cpu", seed=0, comms_range=10)
    env.step(env.get_random_actions())
    geoms = env.scenario.extra_render(1)
    assert len(geoms) == 3 + 4 and all(isinstance(g, rendering.Geom) for g in geoms)
    env = make_env("sampling", num_envs=4, device="cpu", seed=0)
    assert len(env.scenario.extra_render(0)) == 4  # comms_range 0: the perimeter only
    frame = env.render(mode="rgb_array", env_index=1)
    assert frame.ndim == 3 and frame.shape[-1] == 3 and (frame != 255).any()


# ---- the host backend (device -1) of the two native programs ---------------------------------------
@pytest.mark.parametrize("config", ["default", "cov_list_own_no_norm", "small_grid", "one_agent"])
def test_host_backend_matches_the_torch_program(config):
    """Flags, positions, cells and required zeros exactly; pdf values within the density tolerance
    (libm's exp and torch's vectorised CPU exp need not agree); the LIDAR (exact form) within the
    LIDAR tolerance."""
    kw = CONFIGS[config]
    envs = R.twins("sampling", 2, 64, "cpu", seed=5, **kw)
    for e in envs:
        place_cases(e)
    ref, nat = envs
    scn = nat.scenario
    n = len(nat.agents)
    # the normalisation: every env, then a partial mask (the other rows untouched)
    xs, ys = scn._grid_points()
    want = scn.max_pdf.clone()
    scn.max_pdf[:] = 0
    assert scn._native_max_pdf(xs, ys, None, force=True)
    pts = torch.stack(torch.meshgrid(xs, ys, indexing="ij"), dim=-1).reshape(1, -1, 2).expand(64, -1, -1).clone()
    pts[..., 0].clamp_(-scn.x_semidim, scn.x_semidim)
    pts[..., 1].clamp_(-scn.y_semidim, scn.y_semidim)
    ref64, tol, ok = density_tolerance(scn.locs, scn.covs, pts)
    best = ref64.max(dim=1).values
    print(f"host max_pdf: tolerance {tol:.3e}, worst {float(((scn.max_pdf.double() - best).abs() / best).max()):.3e}")
    assert ((scn.max_pdf.double() - best).abs() <= tol * best).all()
    assert ((want.double() - best).abs() <= tol * best).all()
    got = scn.max_pdf.clone()
    scn.max_pdf[:] = -1.0
    assert scn._native_max_pdf(xs, ys, 7, force=True)
    assert scn.max_pdf[7] == got[7] and (scn.max_pdf[torch.arange(64) != 7] == -1).all()
    scn.max_pdf[:] = want
    # the step program
    flags_before = scn.sampled.clone()
    pos_before = [a.state.pos.clone() for a in nat.agents]
    obs, rewards, infos = ref.get_from_scenario(get_observations=True, get_rewards=True, get_infos=True, get_dones=False)
    # graph mode is offered the undo of `sampled` only for a step whose reward wrote the undo log
    assert scn._vmas_graph_restorers() == {}  # (the steps so far ran the torch program)
    out = scn._run_fused(N.VMAS_SCN_REWARD | N.VMAS_SCN_OBS)
    assert list(scn._vmas_graph_restorers()) == ["sampled"]
    assert torch.equal(scn.sampled, ref.scenario.sampled) and not torch.equal(scn.sampled, flags_before)
    B = 64
    # the tolerance over every point the program evaluates: the agents' positions and their probes
    s = scn.grid_spacing
    deltas = torch.tensor([[0, 0], [s, 0], [-s, 0], [0, s], [0, -s], [-s, -s], [s, -s], [-s, s], [s, s]], dtype=torch.float32)
    worst = widest = 0.0
    for j, (a, b) in enumerate(zip(ref.agents, nat.agents)):
        assert torch.equal(a.state.pos, b.state.pos)
        pts = a.state.pos[:, None, :] + deltas[None]
        pts[..., 0].clamp_(-scn.x_semidim, scn.x_semidim)
        pts[..., 1].clamp_(-scn.y_semidim, scn.y_semidim)
        ref64, tol, ok = density_tolerance(scn.locs, scn.covs, pts)
        mp = scn.max_pdf.double()  # (both programs divide by the same fp32 max_pdf)
        own = ref64[:, 0] / mp if scn.norm else ref64[:, 0]
        probes = ref64[:, 1:] / mp[:, None]
        o_t, o_n = obs[j], out["obs"][j]
        assert torch.equal(o_t[:, :4], o_n[:, :4])
        assert ((o_t[:, 4:16] - o_n[:, 4:16]).abs() <= LIDAR_ATOL + LIDAR_RTOL * o_t[:, 4:16].abs()).all()
        for name, t_val, n_val, r64, m in (("sample", infos[j]["agent_sample"], b.sample, own, ok[:, 0]),
                                           ("probes", o_t[:, 16:], o_n[:, 16:], probes, ok[:, 1:])):
            assert torch.equal(t_val == 0, n_val == 0), name  # zeros required by the flags are exact
            live = m & (t_val != 0)
            err = ((n_val.double() - r64).abs() / r64)[live]
            worst, widest = max(worst, float(err.max()) if err.numel() else 0.0), max(widest, tol)
            assert (err <= tol).all(), (name, float(err.max()), tol)
    print(f"host step program: tolerance (largest over the agents) {widest:.3e}, worst {worst:.3e}")
    # sampling_rew: the backend's own samples summed in fp32 in the plan's order (strided
    # accumulators, then an adjacent-pair tree), exactly
    acc = scn._fused_plan()["a_order"]
    parts = [sum((nat.agents[k].sample for k in range(i + acc, n, acc)), nat.agents[i].sample) for i in range(min(acc, n))]
    w = 1
    while w < len(parts):
        for i in range(0, len(parts) - w, 2 * w):
            parts[i] = parts[i] + parts[i + w]
        w *= 2
    assert torch.equal(scn.sampling_rew, parts[0])
    for j in range(n):
        assert torch.equal(out["rewards"][j], scn.sampling_rew if scn.shared_rew else nat.agents[j].sample)
    assert any(not torch.equal(p, a.state.pos) for p, a in zip(pos_before, nat.agents))  # (the clamp wrote)
    # the undo log: exactly the cells this step marked (graph mode's rollback clears them again)
    newly = (scn.sampled & ~flags_before).view(B, -1)
    logged = torch.zeros(B, newly.shape[1] + 1, dtype=torch.bool)
    logged.scatter_(1, torch.where(scn._undo >= 0, scn._undo, newly.shape[1]).long(), True)
    assert torch.equal(logged[:, :-1], newly)
    scn._unmark_last_step()
    assert torch.equal(scn.sampled, flags_before)


def test_sampling_io_layout_and_argument_checks():
    """The two argument blocks as Python declares them against a C compilation of the header, under
    the 4 KiB of a kernel argument block; the entry points refuse counts over the caps, a bad grid
    and null pointers without touching a device."""
    import subprocess
    import tempfile
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    probe = r'''
#include <stddef.h>
#include <stdio.h>
#include "vmas_mi355x.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\n", sizeof(VmasSamplingIO), offsetof(VmasSamplingIO, grid),
    offsetof(VmasSamplingIO, density), offsetof(VmasSamplingIO, pos), offsetof(VmasSamplingIO, angles),
    offsetof(VmasSamplingIO, sampled), offsetof(VmasSamplingIO, out_delta), sizeof(VmasSamplingMaxPdfIO),
    offsetof(VmasSamplingMaxPdfIO, max_pdf), VMAS_SAMPLING_MAX_AGENTS, VMAS_SAMPLING_MAX_GAUSSIANS,
    VMAS_SAMPLING_MAX_RAYS);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = Path(d) / "probe.c"
        src.write_text(probe)
        exe = Path(d) / "probe"
        subprocess.run(["gcc", "-I", str(root / "include"), str(src), "-o", str(exe)], check=True)
        c = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()))
    io, mio = N.VmasSamplingIO, N.VmasSamplingMaxPdfIO
    assert c == [ctypes.sizeof(io), io.grid.offset, io.density.offset, io.pos.offset, io.angles.offset,
                 io.sampled.offset, io.out_delta.offset, ctypes.sizeof(mio), mio.max_pdf.offset,
                 N.VMAS_SAMPLING_MAX_AGENTS, N.VMAS_SAMPLING_MAX_GAUSSIANS, N.VMAS_SAMPLING_MAX_RAYS]
    assert ctypes.sizeof(io) <= 4096 and ctypes.sizeof(mio) <= 4096
    lib = N.load_library()
    for name in ("vmas_sampling_outputs", "vmas_sampling_max_pdf"):
        assert name in N.EXPORTED_SYMBOLS and N.fn_addr(name)
    INVALID = -1
    assert lib.vmas_sampling_outputs(-1, None, None) == INVALID
    assert lib.vmas_sampling_max_pdf(-1, None, None) == INVALID
    buf = torch.zeros(64)
    flags = torch.zeros(4, 8, 4, dtype=torch.bool)

    def good():
        a = io()
        a.batch, a.n_agents, a.what, a.agent_sum_mode = 4, 2, N.VMAS_SCN_REWARD, 1
        a.grid.n_x, a.grid.n_y = 8, 4
        a.density.n_gaussians, a.density.sum_mode = 1, 1
        a.density.loc[0].p = buf.data_ptr()
        a.max_pdf, a.sampled = buf.data_ptr(), flags.data_ptr()
        return a

    for field, value, msg in (("n_agents", N.VMAS_SAMPLING_MAX_AGENTS + 1, b"bad arguments"),
                              ("n_rays", N.VMAS_SAMPLING_MAX_RAYS + 1, b"bad arguments"),
                              ("agent_sum_mode", 3, b"bad arguments"), ("what", 0, b"bad arguments"),
                              ("batch", 0, b"bad arguments"), ("sampled", None, b"bad arguments")):
        a = good()
        setattr(a, field, value)
        assert lib.vmas_sampling_outputs(-1, ctypes.byref(a), None) == INVALID, field
        assert msg in lib.vmas_aux_last_error()
    a = good()
    a.density.n_gaussians = N.VMAS_SAMPLING_MAX_GAUSSIANS + 1
    assert lib.vmas_sampling_outputs(-1, ctypes.byref(a), None) == INVALID
    assert b"Gaussian count" in lib.vmas_aux_last_error()
    a = good()
    a.grid.n_x = 0
    assert lib.vmas_sampling_outputs(-1, ctypes.byref(a), None) == INVALID and b"grid size" in lib.vmas_aux_last_error()
    a = good()  # (complete but for the agents' pointers)
    assert lib.vmas_sampling_outputs(-1, ctypes.byref(a), None) == INVALID
    assert b"null pointer (agent 0)" in lib.vmas_aux_last_error()
    m = mio()
    m.batch, m.n_xs, m.n_ys = 4, 8, 4
    assert lib.vmas_sampling_max_pdf(-1, ctypes.byref(m), None) == INVALID  # (no tables)
    m.xs = m.ys = m.max_pdf = buf.data_ptr()
    m.grid.n_x, m.grid.n_y = 8, 4
    assert lib.vmas_sampling_max_pdf(-1, ctypes.byref(m), None) == INVALID
    assert b"Gaussian count" in lib.vmas_aux_last_error()
