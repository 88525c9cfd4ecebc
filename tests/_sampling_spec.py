"""The yardstick of the sampling scenario: what one step and one normalisation must compute, written
from the task's description on plain CPU tensors taken from a world snapshot (it never imports the
scenario file).

The density comes from ``torch.distributions.MultivariateNormal`` itself.  The visited-cell grid is
kept flat (``flags [B, n_x * n_y]``) and read and marked agent by agent, in agent order, so that a
later agent finds the cell an earlier one took in the same step.  ``max_pdf_loop`` visits the grid
points one at a time.  The LIDAR is the CPU oracle's ``World.cast_rays`` as
tests/_navigation_spec.py calls it.

``SamplingSpec(env)`` reads the parameters and the carried state (``sampled``, ``max_pdf``,
``locs``) from a built env; ``run()`` evaluates one step's outputs in the environment's order
(every reward, every observation, every info).  ``place_cases(env)`` overwrites a few envs by hand
so that every branch of the program occurs; ``assert_cases_fired`` checks, on the spec's own
outputs, that each did.
"""
import types

import torch
from torch.distributions import MultivariateNormal

from oracle import vmas_oracle as O
from tests._navigation_spec import _Sensor

PARAMS = ("shared_rew", "xdim", "ydim", "grid_spacing", "n_x_cells", "n_y_cells", "norm", "x_semidim", "y_semidim",
          "covs", "agent_radius")
# probe points around an agent, in units of grid_spacing, in observation order
PROBE_STEPS = [(+1, 0), (-1, 0), (0, +1), (0, -1), (-1, -1), (+1, -1), (-1, +1), (+1, +1)]


class SamplingSpec:
    def __init__(self, env):
        scn, w = env.scenario, env.world
        for k in PARAMS:
            setattr(self, k, getattr(scn, k))
        snap = O.snapshot(w)
        ow = O.OracleWorld(w, snap)
        ents = w.entities
        agents = []
        for a in w.agents:
            sa = ow.ents[ents.index(a)]
            sa.lidar = [_Sensor(ow, ents.index(a), s, snap[ents.index(a)]["rot"]) for s in (a.sensors or [])]
            agents.append(sa)
        self.world = types.SimpleNamespace(agents=agents)
        self.B = w.batch_dim
        self.flags = scn.sampled.detach().cpu().clone().reshape(self.B, -1)
        self.max_pdf = scn.max_pdf.detach().cpu().clone()
        self.locs = [loc.detach().cpu().clone() for loc in scn.locs]
        # (one covariance matrix per env, as the task builds its distributions)
        self.dists = [MultivariateNormal(loc, covariance_matrix=(cov * torch.eye(2)).expand(self.B, 2, 2))
                      for loc, cov in zip(self.locs, self.covs)]
        self.dims = torch.tensor([self.xdim, self.ydim], dtype=torch.float32)
        self.semidims = torch.tensor([self.x_semidim, self.y_semidim], dtype=torch.float32)

    @property
    def sampled(self):
        return self.flags.view(self.B, self.n_x_cells, self.n_y_cells)

    # ---- one sample ---------------------------------------------------------------------------------
    def locate(self, pts):
        """(strictly outside the dimensions [B], flat cell id [B]); ``pts`` [B, 2] is clamped to the
        semidims in place, after the bounds test and before the cell is taken."""
        outside = (pts.abs() > self.dims).any(dim=-1)
        pts.copy_(torch.clamp(pts, min=-self.semidims, max=self.semidims))
        col = torch.trunc(pts[:, 0] / self.grid_spacing + self.n_x_cells / 2).long()
        row = torch.trunc(pts[:, 1] / self.grid_spacing + self.n_y_cells / 2).long()
        assert ((0 <= col) & (col < self.n_x_cells) & (0 <= row) & (row < self.n_y_cells)).all()
        return outside, (col * self.n_y_cells + row).unsqueeze(1)

    def value(self, pts, norm, mark):
        outside, cell = self.locate(pts)
        v = torch.stack([d.log_prob(pts).exp() for d in self.dists], dim=-1).sum(-1)
        if norm:
            v = v / self.max_pdf
        v = v.masked_fill(self.flags.gather(1, cell).squeeze(1) | outside, 0.0)
        if mark:  # (an out-of-bounds point marks its clamped cell all the same)
            self.flags.scatter_(1, cell, True)
        return v

    def max_pdf_loop(self):
        """The full reset's normalisation one grid point at a time: from zero and cleared flags, the
        running maximum of the unnormalised value of the whole batch at that point (small grids)."""
        kept, self.flags = self.flags, torch.zeros_like(self.flags)
        best = torch.zeros(self.B)
        for gx in torch.arange(-self.xdim, self.xdim, self.grid_spacing).tolist():
            for gy in torch.arange(-self.ydim, self.ydim, self.grid_spacing).tolist():
                pts = torch.tensor([gx, gy], dtype=torch.float32).repeat(self.B, 1)
                best = torch.maximum(best, self.value(pts, norm=False, mark=False))
        self.flags = kept
        return best

    # ---- one step's outputs, in the environment's order ----------------------------------------------
    def run(self):
        agents = self.world.agents
        # rewards: at the first agent every agent samples where it stands, in order, marking its cell
        for a in agents:
            a.sample = self.value(a.state.pos, norm=self.norm, mark=True)
        self.sampling_rew = torch.stack([a.sample for a in agents], dim=-1).sum(-1)
        rewards = [(self.sampling_rew if self.shared_rew else a.sample).clone() for a in agents]
        # observations: pos, vel, LIDAR, then the eight probes (always normalised, never marking)
        obs = []
        for a in agents:
            cols = [a.state.pos, a.state.vel, a.lidar[0].measure()]
            for kx, ky in PROBE_STEPS:
                step = torch.tensor([kx * self.grid_spacing, ky * self.grid_spacing], dtype=torch.float32)
                cols.append(self.value(a.state.pos + step, norm=True, mark=False).unsqueeze(1))
            obs.append(torch.cat(cols, dim=1))
        infos = [{"agent_sample": a.sample.clone()} for a in agents]
        return {"obs": obs, "rewards": rewards, "infos": infos}

    def attributes(self):
        """What the program leaves behind, in a fixed order."""
        out = [self.sampling_rew, self.sampled, self.max_pdf]
        for a in self.world.agents:
            out += [a.sample, a.state.pos]
        return out


def scenario_attributes(env):
    scn = env.scenario
    out = [scn.sampling_rew, scn.sampled, scn.max_pdf]
    for a in env.world.agents:
        out += [a.sample, a.state.pos]
    return out


# ---- hand-placed cases -------------------------------------------------------------------------------
# name -> the envs in which it must fire
CASE_ENVS = {
    "a_shared_cell": range(0, 4),       # agents 0 and 1 in one unsampled cell: the second gets exactly 0
    "b_beyond_semidim": range(8, 12),   # agent 0 at 0.99 xdim: sampled (non-zero), clamped to the semidim
    "c_out_of_bounds": range(16, 20),   # agent 0 at 1.01 xdim: exactly 0, clamped, the cell marked all the same
    "d_sampled_before": range(24, 28),  # agent 0 in a cell sampled on an earlier step: exactly 0
    "e_border": range(32, 36),          # agent 0 in the last column: its outward probes are exactly 0
    "f_neighbour_marked": range(40, 44),  # agent 1 marks agent 0's (+s, +s) neighbour cell in the same step
}


def _centre(scn, ix, iy):
    s = scn.grid_spacing
    return [(ix - scn.n_x_cells / 2 + 0.5) * s, (iy - scn.n_y_cells / 2 + 0.5) * s]


def place_cases(env):
    """Overwrite positions and flags by hand (44+ envs; cases a and f need two agents)."""
    scn, w = env.scenario, env.world
    agents = w.agents
    dev = w.device
    ix, iy = scn.n_x_cells // 2 + 1, scn.n_y_cells // 2
    s = scn.grid_spacing

    def t(xy):
        return torch.tensor(xy, device=dev, dtype=torch.float32)

    def rows(name):
        r = CASE_ENVS[name]
        return slice(r.start, r.stop)

    flags = scn.sampled.clone()
    for name in CASE_ENVS:
        flags[rows(name)] = False
    flags[rows("d_sampled_before"), ix, iy] = True
    scn.sampled[:] = flags
    cx, cy = _centre(scn, ix, iy)
    p0 = agents[0].state.pos.clone()
    # (two corners of one cell: 0.8 * sqrt(2) * s apart, no contact between the spheres)
    p0[rows("a_shared_cell")] = t([cx - 0.4 * s, cy - 0.4 * s])
    p0[rows("b_beyond_semidim")] = t([0.99 * scn.xdim, cy])
    p0[rows("c_out_of_bounds")] = t([1.01 * scn.xdim, cy])
    p0[rows("d_sampled_before")] = t([cx, cy])
    p0[rows("e_border")] = t([scn.xdim - 0.8 * s, cy])
    p0[rows("f_neighbour_marked")] = t([cx, cy])
    agents[0].set_pos(p0, batch_index=None)
    if len(agents) > 1:
        p1 = agents[1].state.pos.clone()
        p1[rows("a_shared_cell")] = t([cx + 0.4 * s, cy + 0.4 * s])
        p1[rows("f_neighbour_marked")] = t(_centre(scn, ix + 1, iy + 1))
        agents[1].set_pos(p1, batch_index=None)


def assert_cases_fired(spec: SamplingSpec, exp, flags_before):
    """On the spec's own outputs (``exp = spec.run()`` after place_cases; ``flags_before``: its
    flags before the run)."""
    n = len(spec.world.agents)
    s0 = exp["infos"][0]["agent_sample"]
    pos0 = spec.world.agents[0].state.pos
    ix, iy = spec.n_x_cells // 2 + 1, spec.n_y_cells // 2
    sx = torch.tensor(spec.x_semidim, dtype=torch.float32)

    def rows(name):
        return list(CASE_ENVS[name])

    if n > 1:
        r = rows("a_shared_cell")
        s1 = exp["infos"][1]["agent_sample"]
        assert (s0[r] != 0).all() and (s1[r] == 0).all()
        if not spec.shared_rew:
            assert (exp["rewards"][1][r] == 0).all() and (exp["rewards"][0][r] != 0).all()
    r = rows("b_beyond_semidim")
    assert (s0[r] != 0).all() and (pos0[r, 0] == sx).all()
    r = rows("c_out_of_bounds")
    assert (s0[r] == 0).all() and (pos0[r, 0] == sx).all()
    assert not flags_before[r, spec.n_x_cells - 1, iy].any() and spec.sampled[r, spec.n_x_cells - 1, iy].all()
    r = rows("d_sampled_before")
    assert flags_before[r, ix, iy].all() and (s0[r] == 0).all()
    r = rows("e_border")
    probes = exp["obs"][0][:, -8:]
    assert (probes[r][:, [0, 5, 7]] == 0).all() and (probes[r][:, 1] != 0).all()
    if n > 1:
        r = rows("f_neighbour_marked")
        assert not flags_before[r, ix + 1, iy + 1].any()
        assert (probes[r][:, 7] == 0).all() and (exp["obs"][1][r][:, -8 + 4] == 0).all()
        assert (s0[r] != 0).all() and (exp["infos"][1]["agent_sample"][r] != 0).all()
