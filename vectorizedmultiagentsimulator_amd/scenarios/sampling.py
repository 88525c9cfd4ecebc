# Derived from VMAS, Copyright (c) 2022-2024 ProrokLab (https://www.proroklab.org/), licensed under
# GPL-3.0; modified for this MI355X build.  See NOTICE.md.
"""Sampling: the agents harvest a density (a sum of Gaussians) over a bounded world, cell by cell.

Restates the behaviour of vmas/scenarios/sampling.py (``Scenario``): its kwargs, attribute names,
draw order and per-step values, in this package's own structure.  Every env carries a grid of visited cells
(``sampled``); an agent's reward is the density at its position, once per cell -- the second agent
to enter a cell in the same step gets nothing.  The observation is pos, vel, a 12-ray LIDAR over the
other agents and the density at 8 probe points around the agent.

What differs from the reference, by design:

* the density is evaluated with the elementwise fp32 operations that
  ``MultivariateNormal(loc, cov I).log_prob(p).exp()`` amounts to for these covariances
  (``_density``; equal to it bit for bit on the CPU, tests/test_sampling.py), so that the native
  program has a fixed sequence of operations to equal; ``gaussians`` builds the reference's
  distributions when read;
* ``locs[i]`` are views of one batched tensor and a reset writes them in place (the reference
  re-binds the list's entries): a captured step graph keeps reading the right memory, and
  ``reset_where`` merges their rows like any other batched tensor;
* the flag mask is applied with ``torch.where`` (no boolean-mask assignment: no host wait);
* ``nomrlize_pdf`` evaluates the reference's double loop over the grid points in blocks of points
  (the same per-point operations; ``max`` does not depend on the order) or, on ROCm devices, in one
  launch (csrc/vmas_scenarios.hip k_sampling_max_pdf);
* ``extra_render`` draws the communication lines and the perimeter; the reference's density layer
  (``render_function_util`` / ``Image``) is not part of this build.
"""
import ctypes
import math
from typing import Dict, Optional

import numpy as np
import torch
from torch import Tensor
from torch.distributions import MultivariateNormal

from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd.simulator import _fused
from vectorizedmultiagentsimulator_amd.simulator.core import Agent, Sphere, World
from vectorizedmultiagentsimulator_amd.simulator.scenario import BaseScenario
from vectorizedmultiagentsimulator_amd.simulator.sensors import Lidar
from vectorizedmultiagentsimulator_amd.simulator.utils import Color, ScenarioUtils, X, Y

# (device, configuration) -> None: the native programs equal the torch program on the probe's fixed
# inputs; str: what differed (the scenario then keeps its torch program)
PROBES = {}
PROBE_ROWS = 1024
_POINT_BLOCK = 1 << 22  # elements of one block of the torch normalisation


class Scenario(BaseScenario):
    # Re-bound by the first agent's reward before anything in the step reads them (info reads
    # agent.sample after the reward): graph replays need not carry them (environment/_graph.py
    # _write_only).  sampled, max_pdf and the positions are written in place.
    _vmas_graph_write_only = frozenset({"sampling_rew"})
    _vmas_graph_write_only_agents = frozenset({"sample"})

    # kwarg -> default (the reference's names and values)
    KWARGS = {
        "n_agents": 3, "shared_rew": True, "comms_range": 0.0, "lidar_range": 0.2, "agent_radius": 0.025,
        "xdim": 1, "ydim": 1, "grid_spacing": 0.05, "n_gaussians": 3, "cov": 0.05, "collisions": True,
        "spawn_same_pos": False, "norm": True,
    }
    N_RAYS = 12
    LIDAR_START = 0.05  # the first ray's angle; the rays cover one full turn from it
    # the observation's probe points, in units of grid_spacing, in the reference's order
    PROBE_OFFSETS = ((1, 0), (-1, 0), (0, 1), (0, -1), (-1, -1), (1, -1), (-1, 1), (1, 1))

    def make_world(self, batch_dim: int, device: torch.device, **kwargs):
        self._kwargs = dict(kwargs)
        for name, default in self.KWARGS.items():
            setattr(self, name, kwargs.pop(name, default))
        ScenarioUtils.check_kwargs_consumed(kwargs)
        self.covs = list(self.cov) if isinstance(self.cov, (list, tuple)) else [self.cov] * self.n_gaussians

        assert not (self.spawn_same_pos and self.collisions)
        for dim in (self.xdim, self.ydim):
            assert (dim / self.grid_spacing) % 1 == 0
        assert len(self.covs) == self.n_gaussians

        self.visualize_semidims = False  # (extra_render draws the perimeter, at the dimensions)
        self.n_x_cells, self.n_y_cells = (int(2 * dim / self.grid_spacing) for dim in (self.xdim, self.ydim))
        self.x_semidim, self.y_semidim = self.xdim - self.agent_radius, self.ydim - self.agent_radius
        # agents spawn over the whole world, or all at the origin
        self.agent_xspawn_range, self.agent_yspawn_range = (0, 0) if self.spawn_same_pos else (self.xdim, self.ydim)

        world = World(batch_dim, device, x_semidim=self.x_semidim, y_semidim=self.y_semidim)
        for i in range(self.n_agents):
            sensors = None
            if self.collisions:
                sensors = [Lidar(world, angle_start=self.LIDAR_START, angle_end=self.LIDAR_START + 2 * torch.pi,
                                 n_rays=self.N_RAYS, max_range=self.lidar_range,
                                 entity_filter=lambda e: isinstance(e, Agent))]
            world.add_agent(Agent(name=f"agent_{i}", shape=Sphere(radius=self.agent_radius), collide=self.collisions,
                                  render_action=True, sensors=sensors))

        f32 = dict(device=device, dtype=torch.float32)
        self.max_pdf = torch.zeros(batch_dim, **f32)
        self.sampled = torch.zeros(batch_dim, self.n_x_cells, self.n_y_cells, device=device, dtype=torch.bool)
        # locs[i] is [B, 2], a view of one batched tensor (see the module notes)
        self._locs = torch.zeros(batch_dim, self.n_gaussians, world.dim_p, **f32)
        self.locs = list(self._locs.unbind(1))
        self.cov_matrices = [(cov * torch.eye(world.dim_p, **f32)).expand(batch_dim, -1, -1) for cov in self.covs]
        # MultivariateNormal's constants for cov I: L = sqrt(cov) (its Cholesky factor's diagonal),
        # half_log_det = log L + log L, and 2 log(2 pi), each as fp32 torch computes it
        self._scale = [torch.tensor(cov, **f32).sqrt() for cov in self.covs]
        self._half_log_det = [L.log() + L.log() for L in self._scale]
        self._log_norm = world.dim_p * math.log(2 * math.pi)
        self._rows = torch.arange(batch_dim, device=device)
        # the native step program's undo log: per (env, agent) the cell this step marked, or -1
        self._undo = torch.full((batch_dim, self.n_agents), -1, device=device, dtype=torch.int32)
        self._native = {"undo_live": False}  # the last reward call wrote the undo log
        return world

    @property
    def gaussians(self):
        """The reference's list of distributions, built from the current locs when read."""
        return [MultivariateNormal(loc=loc, covariance_matrix=cov_matrix)
                for loc, cov_matrix in zip(self.locs, self.cov_matrices)]

    def to(self, device: torch.device):
        super().to(device)
        self.locs = list(self._locs.unbind(1))
        for name in ("cov_matrices", "_scale", "_half_log_det"):
            setattr(self, name, [t.to(device) for t in getattr(self, name)])

    def _draw_xy(self, env_index, x_bound, y_bound, one_env_shape):
        """One uniform draw for x, then one for y, over +-bound: [B, 1] columns for a full reset,
        ``one_env_shape`` for one env (the generator advances as the reference's reset does)."""
        w = self.world
        shape = (w.batch_dim, 1) if env_index is None else one_env_shape
        cols = [torch.zeros(shape, device=w.device, dtype=torch.float32).uniform_(-b, b) for b in (x_bound, y_bound)]
        return torch.cat(cols, dim=-1)

    def reset_world_at(self, env_index: int = None):
        rows = slice(None) if env_index is None else env_index
        for loc in self.locs:  # in place: see the module notes
            loc[rows] = self._draw_xy(env_index, self.xdim, self.ydim, (1,))
        self.max_pdf[rows] = 0
        self.sampled[rows] = False
        self.nomrlize_pdf(env_index=env_index)
        for agent in self.world.agents:
            spawn = self._draw_xy(env_index, self.agent_xspawn_range, self.agent_yspawn_range, (1, 1))
            agent.set_pos(spawn, batch_index=env_index)
            agent.sample = self.sample(agent.state.pos, norm=self.norm)  # (clamps the spawn in place)

    # ---- masked reset (Environment.reset_where; csrc/vmas_scenarios.hip k_sampling_reset) --------
    # The rows of `mask` as reset_world_at(None) after World.reset leaves them, written in place by
    # ONE launch with no host wait: a wave per masked env draws the env's elements of the full reset's
    # uniform_ columns (the generator advance, 2 per Gaussian and 2 per agent, is known beforehand),
    # finds max_pdf over the grid points, clears the flag row and places the agents with their
    # samples.  _undo and _native["undo_live"] are a step's, not a reset's: untouched, as by reset().
    native_resets = 0  # launches made (a test's proof that no fall-back ran)

    def reset_world_where(self, mask):
        from vectorizedmultiagentsimulator_amd.simulator.environment import _uniform
        from vectorizedmultiagentsimulator_amd.simulator.environment._spawn_reset import _mut

        w = self.world
        env = getattr(self, "_where_env", None)
        if not _fused.enabled(w) or getattr(w, "_grad_enabled", False):
            return NotImplemented
        plan = self._fused_plan()
        if plan is None or plan["dev"].type != "cuda":
            return NotImplemented
        dev, B, agents = plan["dev"], w.batch_dim, w.agents
        mode = _uniform.mode(dev, B)
        mp, fl = self.max_pdf, self.sampled
        if (mode is None or mask.dtype is not torch.bool or mask.device != dev or not mask.is_contiguous()
                or mp.dtype is not torch.float32 or not mp.is_contiguous() or mp.device != dev or mp.shape != (B,)
                or fl.dtype is not torch.bool or not fl.is_contiguous() or fl.device != dev
                or fl.shape != (B, self.n_x_cells, self.n_y_cells)):
            return NotImplemented
        steps = env.steps if env is not None else None
        if steps is not None and (steps.dtype is not torch.float32 or steps.shape != (B,) or not steps.is_contiguous()
                                  or steps.device != dev):
            return NotImplemented
        # (graph mode) a field still bound to the persistent action buffer, whose rows the next step's
        # actions own, leaves the call to the generic path
        p_buf = getattr(getattr(env, "_u_persist", None), "buffer", None)
        p_lo = p_buf.data_ptr() if p_buf is not None else 0
        p_hi = p_lo + 4 * p_buf.numel() if p_buf is not None else 0
        io = N.VmasSamplingResetIO()
        written = [mp, fl, self._locs]
        ok = True

        def mut(t):
            nonlocal ok
            v = _mut(t, dev)
            if v is None or p_lo <= t.data_ptr() < p_hi:
                ok = False
                return N.VmasMutVec()
            written.append(t)
            return v

        for i, a in enumerate(agents):
            st, dst = a.state, io.agents[i]
            smp = getattr(a, "sample", None)
            if (st.c is not None or not isinstance(smp, Tensor) or smp.dtype is not torch.float32 or smp.device != dev
                    or smp.shape != (B,) or not smp.is_contiguous()):
                return NotImplemented  # (communication state is zeroed by World.reset, not by the launch)
            dst.pos, dst.vel, dst.rot, dst.ang_vel = mut(st.pos), mut(st.vel), mut(st.rot), mut(st.ang_vel)
            io.force[i], io.torque[i] = mut(st.__dict__.get("_force")), mut(st.__dict__.get("_torque"))
            io.sample[i] = smp.data_ptr()
            written.append(smp)
        # (one tensor bound to two fields -- a user's set_pos of a shared tensor -- cannot take two rows)
        if not ok or len({t.data_ptr() for t in written}) != len(written):
            return NotImplemented
        points = plan.get("points")
        if points is None:  # (the grid points of nomrlize_pdf, kept with the plan: two launches less per call)
            points = plan["points"] = self._grid_points()
        xpoints, ypoints = points
        keep = []
        try:
            self._fill_density(io.grid, io.density, plan, keep)
        except _NotFusable:
            return NotImplemented
        io.batch, io.n_agents, io.mode, io.norm = B, len(agents), mode, int(bool(self.norm))
        io.n_xs, io.n_ys = xpoints.numel(), ypoints.numel()
        for k, (loc, spawn) in enumerate(((self.xdim, self.agent_xspawn_range), (self.ydim, self.agent_yspawn_range))):
            io.loc_lo[k], io.loc_hi[k] = float(-loc), float(loc)  # (uniform_(-b, b) of _draw_xy)
            io.spawn_lo[k], io.spawn_hi[k] = float(-spawn), float(spawn)
        io.xs, io.ys, io.mask = xpoints.data_ptr(), ypoints.data_ptr(), mask.data_ptr()
        io.max_pdf, io.sampled = mp.data_ptr(), fl.data_ptr()
        io.steps = steps.data_ptr() if steps is not None else None
        gen = torch.cuda.default_generators[dev.index]
        off = gen.get_offset()
        io.seed, io.offset = gen.initial_seed(), off
        inc = ctypes.c_uint64(0)
        _fused.check(_fused.lib().vmas_sampling_reset(dev.index, ctypes.byref(io), ctypes.byref(inc), _fused.stream(w)),
                     "vmas_sampling_reset")
        gen.set_offset(off + inc.value)
        for t in written:
            _fused.bump_version(t)
        if steps is not None:
            _fused.bump_version(steps)
            self._where_steps_done = True
        for e in w.entities:
            e.notify_observers()
        self.native_resets += 1
        return None

    # ---- the density ----------------------------------------------------------------------------
    def _density(self, pos: Tensor, locs=None) -> Tensor:
        """sum_g exp(MultivariateNormal(loc_g, cov_g I).log_prob(pos)) for pos [..., 2] against locs
        broadcastable to it, as elementwise fp32 operations (include/vmas_mi355x.h, "sampling")."""
        vals = []
        for loc, L, hld in zip(self.locs if locs is None else locs, self._scale, self._half_log_det):
            y = (pos - loc) / L
            m = y[..., 0] * y[..., 0] + y[..., 1] * y[..., 1]
            vals.append((-0.5 * (self._log_norm + m) - hld).exp())
        return torch.stack(vals, dim=-1).sum(-1)

    def _locate(self, pos: Tensor):
        """(out of bounds [...], cell x [...], cell y [...]) of points [..., 2]; clamps ``pos`` to
        the semidims IN PLACE after the bounds test, as the reference's sample() does."""
        x, y = pos[..., X], pos[..., Y]
        outside = (x.abs() > self.xdim) | (y.abs() > self.ydim)  # strictly outside +-dim
        x.clamp_(-self.x_semidim, self.x_semidim)
        y.clamp_(-self.y_semidim, self.y_semidim)
        cells = pos / self.grid_spacing  # (a tensor by a Python number: the native code's div_mode)
        ix = (cells[..., X] + self.n_x_cells / 2).to(torch.long)
        iy = (cells[..., Y] + self.n_y_cells / 2).to(torch.long)
        return outside, ix, iy

    def sample(self, pos, update_sampled_flag: bool = False, norm: bool = True):
        """The density at pos [B, 2] (clamped in place), over max_pdf when ``norm``; zero where the
        cell is already sampled or the point lay out of bounds; marks the cell when asked to."""
        outside, ix, iy = self._locate(pos)
        value = self._density(pos)
        if norm:
            value = value / self.max_pdf
        value = torch.where(self.sampled[self._rows, ix, iy] | outside, 0.0, value)
        if update_sampled_flag:
            self.sampled[self._rows, ix, iy] = True
        return value

    def sample_single_env(self, pos, env_index, norm: bool = True):
        """sample() of points [P, 2] in one env, without flag updates (the reference expands the
        points over the whole batch and then selects the env: the same values)."""
        pos = pos.view(-1, self.world.dim_p)
        outside, ix, iy = self._locate(pos)
        value = self._density(pos, [loc[env_index] for loc in self.locs])
        if norm:
            value = value / self.max_pdf[env_index]
        return torch.where(self.sampled[env_index, ix, iy] | outside, 0.0, value)

    def _grid_points(self):
        dev = self.world.device
        return tuple(torch.arange(-dim, dim, self.grid_spacing, device=dev).to(torch.float32)
                     for dim in (self.xdim, self.ydim))

    def nomrlize_pdf(self, env_index: int = None):
        """max_pdf = the largest unnormalised sample over the grid points (flags cleared before).
        Every env, or one: the native launch on ROCm worlds, else the torch program in blocks of
        points (the reference runs sample() once per point; max does not depend on the order)."""
        xpoints, ypoints = self._grid_points()
        if self._native_max_pdf(xpoints, ypoints, env_index):
            return
        rows = slice(None) if env_index is None else slice(env_index, env_index + 1)
        locs = [loc[rows].unsqueeze(1) for loc in self.locs]  # [b, 1, 2]
        pts = torch.cartesian_prod(xpoints, ypoints)
        outside, _, _ = self._locate(pts)
        best = self.max_pdf[rows]
        block = max(1, _POINT_BLOCK // best.shape[0])
        for p0 in range(0, pts.shape[0], block):
            v = self._density(pts[p0:p0 + block].unsqueeze(0), locs)  # [b, block]
            v = torch.where(outside[p0:p0 + block].unsqueeze(0), 0.0, v)
            best = torch.maximum(best, v.max(dim=1).values)
        self.max_pdf[rows] = best

    # ---- reward / observation -------------------------------------------------------------------
    def reward(self, agent: Agent) -> Tensor:
        if _fused.enabled(self.world) and self._fused_plan() is not None:
            return self._fused_reward(agent)
        return self._torch_reward(agent)

    def _torch_reward(self, agent: Agent) -> Tensor:
        agents = self.world.agents
        if agent is agents[0]:  # every agent samples, in order: an earlier agent takes a shared cell
            self._native["undo_live"] = False
            samples = []
            for a in agents:
                a.sample = self.sample(a.state.pos, update_sampled_flag=True, norm=self.norm)
                samples.append(a.sample)
            self.sampling_rew = torch.stack(samples, dim=-1).sum(-1)
        return self.sampling_rew if self.shared_rew else agent.sample

    def observation(self, agent: Agent) -> Tensor:
        if _fused.enabled(self.world) and self._fused_plan() is not None:
            return self._fused_observation(agent)
        return self._torch_observation(agent)

    def _torch_observation(self, agent: Agent) -> Tensor:
        # (without collisions the agents have no sensor: this raises, as the reference does)
        lidar = agent.sensors[0].measure()
        pos = agent.state.pos
        probes = []
        for sx, sy in self.PROBE_OFFSETS:  # (norm=True whatever self.norm is; no flag is set)
            offset = torch.tensor([sx * self.grid_spacing, sy * self.grid_spacing], device=pos.device,
                                  dtype=torch.float32)
            probes.append(self.sample(pos + offset))
        return torch.cat([pos, agent.state.vel, lidar, torch.stack(probes, dim=-1)], dim=-1)

    def info(self, agent: Agent) -> Dict[str, Tensor]:
        return {"agent_sample": agent.sample}

    def density_for_plot(self, env_index):
        """f(points) -> the normalised, flag-masked density of one env at [P, 2] points."""
        return lambda x: self.sample_single_env(
            torch.as_tensor(x, dtype=torch.float32, device=self.world.device).clone(), env_index=env_index)

    def extra_render(self, env_index: int = 0):
        """A line between every two agents within comms_range, and the world's perimeter (the
        rectangle +-xdim x +-ydim).  (The reference's first geom, the density drawn as an image,
        is not part of this build: see the module notes; ``density_for_plot`` gives the values.)"""
        from vectorizedmultiagentsimulator_amd.simulator import rendering

        def black_line(start, end):
            line = rendering.Line(start, end, width=1)
            line.add_attr(rendering.Transform())
            line.set_color(*Color.BLACK.value)
            return line

        geoms = []
        pos = [a.state.pos[env_index] for a in self.world.agents]
        for i in range(len(pos)):
            for j in range(i + 1, len(pos)):
                if torch.linalg.vector_norm(pos[i] - pos[j]) <= self.comms_range:
                    geoms.append(black_line(pos[i], pos[j]))
        corners = [(self.xdim, self.ydim), (-self.xdim, self.ydim), (-self.xdim, -self.ydim), (self.xdim, -self.ydim)]
        for k in range(4):
            geoms.append(black_line(corners[k], corners[(k + 1) % 4]))
        return geoms

    # ---- native programs (ROCm worlds; csrc/vmas_scenarios.hip k_sampling / k_sampling_max_pdf) ----
    # The first agent's reward call runs one launch: every agent's sample(update_sampled_flag=True)
    # in agent order (the clamp of the positions, the flags, agent.sample, sampling_rew and every
    # agent's returned reward) and every agent's observation with its LIDAR and probes
    # (include/vmas_mi355x.h VmasSamplingIO).  The other calls hand out the precomputed tensors while
    # the inputs are unchanged (_fused.state_key); otherwise the call recomputes.  nomrlize_pdf is
    # one launch (VmasSamplingMaxPdfIO).  ``fused_status`` says which program runs, and why.

    def _config_key(self):
        return (self.n_agents, self.n_gaussians, tuple(float(c) for c in self.covs), float(self.xdim), float(self.ydim),
                float(self.grid_spacing), float(self.agent_radius), float(self.lidar_range), bool(self.shared_rew),
                bool(self.norm), bool(self.collisions), bool(_fused.EXACT_LIDAR))

    def _cell_bounds_ok(self, mode: int) -> bool:
        """No clamped position indexes past the grid (the operations are monotone: the two ends)."""
        from vectorizedmultiagentsimulator_amd.simulator._action_programs import _inv

        f32 = np.float32
        gs = f32(self.grid_spacing)
        inv = _inv(self.grid_spacing, mode) if mode else f32(0)
        for semidim, n in ((self.x_semidim, self.n_x_cells), (self.y_semidim, self.n_y_cells)):
            for p in (f32(semidim), -f32(semidim)):
                f = (p / gs if mode == 0 else p * inv) + f32(n / 2)
                if not (f > -1 and int(f) < n):
                    return False
        return True

    def _plan_reason(self, dev):
        """(plan, None) or (None, why the torch program runs)."""
        from vectorizedmultiagentsimulator_amd.simulator import _action_programs

        w = self.world
        agents = w.agents
        n = len(agents)
        if not 1 <= n <= N.VMAS_SAMPLING_MAX_AGENTS:
            return None, f"{n} agents (VMAS_SAMPLING_MAX_AGENTS = {N.VMAS_SAMPLING_MAX_AGENTS})"
        if not 1 <= self.n_gaussians <= N.VMAS_SAMPLING_MAX_GAUSSIANS:
            return None, f"{self.n_gaussians} Gaussians (VMAS_SAMPLING_MAX_GAUSSIANS = {N.VMAS_SAMPLING_MAX_GAUSSIANS})"
        if not all(type(a.shape).__name__ == "Sphere" for a in agents):
            return None, "an agent is not a sphere"
        if not self.collisions:
            return None, "no LIDAR (collisions=False): the observation raises, as the reference's"
        R, max_range = 0, 0.0
        for k, a in enumerate(agents):
            if not a.sensors or len(a.sensors) != 1 or type(a.sensors[0]).__name__ != "Lidar":
                return None, "an agent's sensors are not one Lidar"
            s = a.sensors[0]
            ts = [e for e in w.entities if e is not a and s.entity_filter(e)]
            if k == 0:
                R, max_range = s._angles.shape[-1], s._max_range
            if ([id(e) for e in ts] != [id(e) for e in agents if e is not a]
                    or s._angles.shape != (w.batch_dim, R) or s._max_range != max_range):
                return None, "a Lidar does not see exactly the other agents"
            for e in ts:
                assert e.collides(a) and a.collides(e), "Rays are only casted among collidables"
        if R > N.VMAS_SAMPLING_MAX_RAYS:
            return None, f"{R} rays (VMAS_SAMPLING_MAX_RAYS = {N.VMAS_SAMPLING_MAX_RAYS})"
        mode = _action_programs.div_mode(dev)
        if mode is None:
            return None, "no division mode reproduces this torch build"
        if not self._cell_bounds_ok(mode):
            return None, "a clamped position can index past the grid"
        g_order = _fused.reduce_order(dev, self.n_gaussians, "sum", N.VMAS_SAMPLING_MAX_GAUSSIANS)
        a_order = _fused.reduce_order(dev, n, "sum", N.VMAS_SAMPLING_MAX_AGENTS)
        if dev.type != "cuda":  # (the host backend: pdf values are held to a tolerance there)
            g_order, a_order = g_order or 1, a_order or 1
        if g_order is None or a_order is None:
            return None, "no summation order reproduces torch's .sum(-1)"
        return {"dev": dev, "R": R, "max_range": max_range, "mode": mode, "g_order": g_order, "a_order": a_order}, None

    def _fused_plan(self):
        w = self.world
        sig = (tuple(id(a) for a in w.agents), tuple(id(e) for e in w.entities), w.batch_dim, str(w.device),
               self._config_key())
        plan = getattr(self, "_fplan", None)
        if plan is not None and plan[0] == sig:
            return plan[1]
        dev = torch.device(w.device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        info, why = self._plan_reason(dev)
        if info is not None and dev.type == "cuda" and not getattr(self, "_is_probe", False):
            if torch.cuda.is_current_stream_capturing():
                return None  # (first use inside a stream capture: the torch program, not remembered)
            why = _probe(self, dev)
            if why is not None:
                info = None
        self._fplan = (sig, info)
        self._fwhy = why
        return info

    @property
    def fused_status(self) -> str:
        """"native", or "torch: <why>" when the scenario's torch program computes the step."""
        if not _fused.enabled(self.world):
            return "torch: the fused programs are off for this world (CPU, autograd or VMAS_FUSED_SCENARIOS=0)"
        if self._fused_plan() is not None:
            return "native"
        return f"torch: {getattr(self, '_fwhy', None) or 'first use inside a stream capture'}"

    def _fill_density(self, grid, density, plan, keep):
        from vectorizedmultiagentsimulator_amd.simulator._action_programs import _inv

        dev, mode = plan["dev"], plan["mode"]
        grid.n_x, grid.n_y, grid.div_mode = self.n_x_cells, self.n_y_cells, int(mode != 0)
        grid.xdim, grid.ydim = float(self.xdim), float(self.ydim)
        grid.x_semidim, grid.y_semidim = float(self.x_semidim), float(self.y_semidim)
        grid.grid_spacing = float(self.grid_spacing)
        grid.inv_grid_spacing = float(_inv(self.grid_spacing, mode)) if mode else 0.0
        grid.half_nx, grid.half_ny = self.n_x_cells / 2, self.n_y_cells / 2
        density.n_gaussians, density.sum_mode = self.n_gaussians, plan["g_order"]
        density.log_norm = self._log_norm
        consts = plan.get("consts")
        if consts is None:  # (read back once: the fp32 values torch computed)
            consts = plan["consts"] = ([float(t) for t in self._scale], [float(t) for t in self._half_log_det])
        for g in range(self.n_gaussians):
            loc = self.locs[g]
            if loc.dtype is not torch.float32 or loc.device != dev or loc.shape != (self.world.batch_dim, 2):
                raise _NotFusable
            density.scale[g], density.half_log_det[g] = consts[0][g], consts[1][g]
            density.loc[g] = _fused.vec(loc, keep)

    def _launch_args(self, dev):
        """(device index, stream) of a launch; a CPU world: the library's host backend (the ABI's
        device -1; reached only by direct calls of _run_fused / _native_max_pdf(force=True))."""
        return (dev.index, _fused.stream(self.world)) if dev.type == "cuda" else (-1, None)

    def _native_max_pdf(self, xpoints, ypoints, env_index, force: bool = False) -> bool:
        w = self.world
        if not (force or _fused.enabled(w)):
            return False
        plan = self._fused_plan()
        mp = self.max_pdf
        if (plan is None or mp.dtype is not torch.float32 or not mp.is_contiguous() or mp.device != plan["dev"]
                or mp.shape != (w.batch_dim,)):
            return False
        io = N.VmasSamplingMaxPdfIO()
        keep = [xpoints, ypoints]
        try:
            self._fill_density(io.grid, io.density, plan, keep)
        except _NotFusable:
            return False
        io.batch, io.n_xs, io.n_ys = w.batch_dim, xpoints.numel(), ypoints.numel()
        io.xs, io.ys, io.max_pdf = xpoints.data_ptr(), ypoints.data_ptr(), mp.data_ptr()
        mask = None
        if env_index is not None:
            mask = torch.zeros(w.batch_dim, dtype=torch.bool, device=plan["dev"])
            mask[env_index] = True
        if mask is not None:
            keep.append(mask)
            io.mask = mask.data_ptr()
        idx, stream = self._launch_args(plan["dev"])
        _fused.check(_fused.lib().vmas_sampling_max_pdf(idx, ctypes.byref(io), stream), "vmas_sampling_max_pdf")
        _fused.bump_version(mp)
        return True

    def _fused_inputs(self):
        ts = [self.sampled, self.max_pdf, self._locs]
        for a in self.world.agents:
            ts += [a.state.pos, a.state.vel, a.state.rot, a.sensors[0]._angles]
        return ts

    def _run_fused(self, what: int):
        w = self.world
        plan = self._fused_plan()
        dev, R = plan["dev"], plan["R"]
        B = w.batch_dim
        agents = w.agents
        n = len(agents)
        keep = []
        io = N.VmasSamplingIO()
        io.batch, io.n_agents, io.what, io.n_rays = B, n, what, R
        io.shared_rew, io.norm = int(bool(self.shared_rew)), int(bool(self.norm))
        io.lidar_on, io.fast_lidar = 1, 0 if _fused.EXACT_LIDAR else 1
        io.agent_sum_mode = plan["a_order"]
        io.max_range = float(plan["max_range"])
        self._fill_density(io.grid, io.density, plan, keep)
        mp, fl = self.max_pdf, self.sampled
        if (mp.dtype is not torch.float32 or not mp.is_contiguous() or mp.device != dev or mp.shape != (B,)
                or fl.dtype is not torch.bool or not fl.is_contiguous() or fl.device != dev
                or fl.shape != (B, self.n_x_cells, self.n_y_cells)):
            raise _NotFusable
        io.max_pdf, io.sampled = mp.data_ptr(), fl.data_ptr()
        W = 12 + R
        out = {}
        # (graph-mode capture: obs / rewards written straight into each replay's fresh tensors)
        io.out_delta, direct = _fused.direct_outputs(w, (
            (torch.float32, (B, W), n) if what & N.VMAS_SCN_OBS else None,
            (torch.float32, (B,), n) if what & N.VMAS_SCN_REWARD else None,
            None))
        if what & N.VMAS_SCN_REWARD:
            u = self._undo
            self._native["undo_live"] = (u.dtype is torch.int32 and u.is_contiguous() and u.device == dev
                                         and u.shape == (B, n))
            if self._native["undo_live"]:
                io.undo = u.data_ptr()
            out["sample"] = [torch.empty(B, device=dev, dtype=torch.float32) for _ in agents]
            out["sampling_rew"] = torch.empty(B, device=dev, dtype=torch.float32)
            out["rewards"] = direct[1] or [torch.empty(B, device=dev, dtype=torch.float32) for _ in agents]
            io.sampling_rew = out["sampling_rew"].data_ptr()
        if what & N.VMAS_SCN_OBS:
            out["obs"] = direct[0] or [torch.empty(B, W, device=dev, dtype=torch.float32) for _ in agents]
            out["lidar"] = [torch.empty(B, R, device=dev, dtype=torch.float32) for _ in agents]
        written = []
        for i, a in enumerate(agents):
            p = a.state.pos
            if (p.dtype is not torch.float32 or p.device != dev or p.shape != (B, 2)
                    or (B > 1 and p.stride(0) == 0) or p.requires_grad):
                raise _NotFusable
            keep.append(p)
            written.append(p)
            io.pos[i].p, io.pos[i].s0, io.pos[i].s1 = p.data_ptr(), p.stride(0), p.stride(1)
            io.radius[i] = float(a.shape.radius)
            if what & N.VMAS_SCN_REWARD:
                io.sample[i] = out["sample"][i].data_ptr()
                io.rewards[i] = out["rewards"][i].data_ptr()
            if what & N.VMAS_SCN_OBS:
                s = a.sensors[0]
                io.vel[i] = _fused.vec(_fused.f32(a.state.vel, dev), keep)
                io.rot[i] = _fused.vec(_fused.f32(a.state.rot, dev), keep)
                ang = _fused.f32(s._angles, dev)
                keep.append(ang)
                io.angles[i], io.ang_s0[i], io.ang_s1[i] = ang.data_ptr(), ang.stride(0), ang.stride(1)
                io.obs[i] = out["obs"][i].data_ptr()
                io.lidar[i] = out["lidar"][i].data_ptr()
        if len({t.data_ptr() for t in written}) != len(written):
            raise _NotFusable  # (one tensor bound to two agents: the clamp's order would show)
        idx, stream = self._launch_args(dev)
        _fused.check(_fused.lib().vmas_sampling_outputs(idx, ctypes.byref(io), stream), "vmas_sampling_outputs")
        if what & N.VMAS_SCN_REWARD:
            # the first agent's reward call: what the reference's block leaves behind
            _fused.bump_version(fl)
            self.sampling_rew = out["sampling_rew"]
            for i, a in enumerate(agents):
                _fused.bump_version(written[i])
                a.sample = out["sample"][i]
        return out

    def _vmas_graph_restorers(self):
        """Graph mode (environment/_graph.py): in-place tensors whose last step this scenario can
        undo itself, so that a replay keeps no per-step backup of them.  With the native program
        the step's writes to ``sampled`` (52 MB at 32 768 envs) are the cells of its undo log."""
        # (asked right after the step being captured ran: only if that step's reward was the native
        # launch and it wrote the log; a step that fell back to the torch program keeps its backup)
        return {"sampled": self._unmark_last_step} if self._native["undo_live"] else {}

    def _unmark_last_step(self):
        B, P = self.world.batch_dim, self.n_x_cells * self.n_y_cells
        idx = torch.where(self._undo >= 0, self._undo, P).long()
        marked = torch.zeros(B, P + 1, dtype=torch.bool, device=self.sampled.device).scatter_(1, idx, True)
        self.sampled.view(B, P).logical_and_(~marked[:, :P])
        self._undo.fill_(-1)

    def _reward_key(self, agent: Agent):
        return _fused.state_key([self.sampling_rew, agent.sample])

    def _obs_cache(self, out):
        return {i: (out["obs"][i], out["lidar"][i]) for i in range(len(self.world.agents))}

    def _fused_reward(self, agent: Agent):
        agents = self.world.agents
        i = agents.index(agent)
        if i == 0:
            try:
                out = self._run_fused(N.VMAS_SCN_REWARD | N.VMAS_SCN_OBS)
            except _NotFusable:
                self._fc = None
                return self._torch_reward(agent)
            self._fc = {
                "key": _fused.state_key(self._fused_inputs()),
                "rew": {k: (out["rewards"][k], self._reward_key(a)) for k, a in enumerate(agents)},
                "obs": self._obs_cache(out),
            }
        c = getattr(self, "_fc", None)
        if c is not None and i in c["rew"]:
            r, k = c["rew"].pop(i)
            if k == self._reward_key(agent):
                return r
        # (an operand changed under the cache: the reference's expression on the current tensors)
        return self.sampling_rew if self.shared_rew else agent.sample

    def _fused_observation(self, agent: Agent):
        i = self.world.agents.index(agent)
        c = getattr(self, "_fc", None)
        if c is None or i not in c["obs"] or c["key"] != _fused.state_key(self._fused_inputs()):
            try:
                out = self._run_fused(N.VMAS_SCN_OBS)
            except _NotFusable:
                return self._torch_observation(agent)
            c = self._fc = {"key": _fused.state_key(self._fused_inputs()), "rew": {}, "obs": self._obs_cache(out)}
        o, lid = c["obs"].pop(i)
        agent.sensors[0]._last_measurement = lid
        return o


class _NotFusable(Exception):
    """An operand the native program does not take (dtype / layout / device): the torch program runs."""


def _probe(scn: Scenario, dev) -> Optional[str]:
    """First use of a configuration on a device: the native programs against the scenario's torch
    program on fixed inputs (two steps of PROBE_ROWS envs: agents sharing cells, out of bounds and
    beyond the semidims, a third of the cells sampled; the second step reads the first one's flags).
    None when rewards, samples, flags, positions, observations (the LIDAR columns only in exact
    mode) and max_pdf are equal bit for bit."""
    key = (str(dev),) + scn._config_key()
    if key in PROBES:
        return PROBES[key]
    B = PROBE_ROWS
    gen = torch.Generator().manual_seed(20240611)

    def rnd(*shape):
        return torch.rand(*shape, generator=gen) * 2 - 1

    dims = torch.tensor([float(scn.xdim), float(scn.ydim)])
    twins = []
    for _ in range(2):
        s = type(scn)()
        s._is_probe = True
        s.env_make_world(B, dev, **scn._kwargs)
        twins.append(s)
    t, nat = twins
    locs = rnd(B, scn.n_gaussians, 2) * dims
    flags = torch.rand(B, scn.n_x_cells, scn.n_y_cells, generator=gen) < 0.33
    why = None
    with torch.no_grad():
        for s in twins:
            s._locs.copy_(locs.to(dev))
            s.sampled.copy_(flags.to(dev))
            s.max_pdf[:] = 0
        xs, ys = t._grid_points()
        with _fused.disabled():
            t.nomrlize_pdf()
        if not nat._native_max_pdf(xs, ys, None):
            why = "the normalisation program did not take the probe's operands"
        elif not torch.equal(t.max_pdf, nat.max_pdf):
            why = "the probe differs from the torch program in max_pdf"
        for step in range(2):
            if why is not None:
                break
            n = len(t.world.agents)
            pos = [rnd(B, 2) * dims * 1.08 for _ in range(n)]
            for j in range(1, n):  # (every fourth env: agent j where agent j - 1 is)
                pos[j][j % 4::4] = pos[j - 1][j % 4::4]
            for s in twins:
                for j, a in enumerate(s.world.agents):
                    a.set_pos(pos[j].to(dev), batch_index=None)
                    a.set_vel(rnd(B, 2).to(dev) if s is t else t.world.agents[j].state.vel.clone(), batch_index=None)
            with _fused.disabled():
                r_t = [t.reward(a) for a in t.world.agents]
                o_t = [t.observation(a) for a in t.world.agents]
            try:
                out = nat._run_fused(N.VMAS_SCN_REWARD | N.VMAS_SCN_OBS)
            except _NotFusable:
                why = "the step program did not take the probe's operands"
                break
            R = out["lidar"][0].shape[1]
            bad = []
            if not torch.equal(t.sampled, nat.sampled):
                bad.append("sampled")
            if not torch.equal(t.sampling_rew, nat.sampling_rew):
                bad.append("sampling_rew")
            for j, (a, b) in enumerate(zip(t.world.agents, nat.world.agents)):
                o_n = out["obs"][j]
                cols = slice(None) if _fused.EXACT_LIDAR else [c for c in range(o_n.shape[1]) if not 4 <= c < 4 + R]
                for name, x, y in (("reward", r_t[j], out["rewards"][j]), ("agent.sample", a.sample, b.sample),
                                   ("pos", a.state.pos, b.state.pos), ("observation", o_t[j][:, cols], o_n[:, cols])):
                    if not torch.equal(x, y) and name not in bad:
                        bad.append(name)
            if bad:
                why = "the probe differs from the torch program in " + ", ".join(bad)
    PROBES[key] = why
    return why
