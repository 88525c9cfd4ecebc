# Derived from VMAS, Copyright (c) 2022-2024 ProrokLab (https://www.proroklab.org/), licensed under
# GPL-3.0; modified for this MI355X build.  See NOTICE.md.
"""MPE simple_tag: slower adversaries chase faster good agents around obstacles in a bounded world.

Restates vmas/scenarios/mpe/simple_tag.py:13-275 (``Scenario``; the reference's
``render_interactively`` is not part of this build).  Two teams (``Agent(adversary=True)``): a good
agent loses 10 per adversary touching it, an adversary gains 10 per good agent it touches; either can
be shaped by distance.  ``Agent.rew`` holds each agent's own value, ``agents_rew`` / ``adverary_rew``
(the reference's spelling) the teams' sums, and a team that shares its reward returns the sum.
Observation rows differ in width per agent: an adversary sees the good agents' velocities, a good
agent does not see the adversaries'.

What differs from the reference, by design: its mask-indexed ``rew[collision] -= 10`` / ``+= 10`` --
a host wait per agent pair per step on a device -- and the mask-indexed respawn of
``respawn_at_catch`` are written as ``torch.where`` on whole tensors (the same values, no host wait;
the respawn keeps the reference's full-batch draw per pair, so the generator ends where the
reference's does).
"""
import numpy as np
import torch
from torch import Tensor

from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd.simulator import _fused
from vectorizedmultiagentsimulator_amd.simulator._mpe import MpeProgram, NotFusable, norm2
from vectorizedmultiagentsimulator_amd.simulator.core import Agent, Landmark, Line, Sphere, World
from vectorizedmultiagentsimulator_amd.simulator.scenario import BaseScenario
from vectorizedmultiagentsimulator_amd.simulator.utils import Color, ScenarioUtils


class Scenario(MpeProgram, BaseScenario):
    # Re-bound by the first agent's reward before anything in the step reads them: graph replays need
    # not carry them (environment/_graph.py _write_only).
    _vmas_graph_write_only = frozenset({"agents_rew", "adverary_rew"})
    _vmas_graph_write_only_agents = frozenset({"rew"})

    def make_world(self, batch_dim: int, device: torch.device, **kwargs):
        num_good_agents = kwargs.pop("num_good_agents", 1)
        num_adversaries = kwargs.pop("num_adversaries", 3)
        num_landmarks = kwargs.pop("num_landmarks", 2)
        self.shape_agent_rew = kwargs.pop("shape_agent_rew", False)
        self.shape_adversary_rew = kwargs.pop("shape_adversary_rew", False)
        self.agents_share_rew = kwargs.pop("agents_share_rew", False)
        self.adversaries_share_rew = kwargs.pop("adversaries_share_rew", True)
        self.observe_same_team = kwargs.pop("observe_same_team", True)
        self.observe_pos = kwargs.pop("observe_pos", True)
        self.observe_vel = kwargs.pop("observe_vel", True)
        self.bound = kwargs.pop("bound", 1.0)
        self.respawn_at_catch = kwargs.pop("respawn_at_catch", False)
        ScenarioUtils.check_kwargs_consumed(kwargs)

        self.visualize_semidims = False  # (extra_render draws the perimeter)
        self.adversary_radius = 0.075

        world = World(batch_dim=batch_dim, device=device, x_semidim=self.bound, y_semidim=self.bound, substeps=10,
                      collision_force=500)
        for i in range(num_adversaries + num_good_agents):
            adversary = i < num_adversaries
            world.add_agent(Agent(
                name=f"adversary_{i}" if adversary else f"agent_{i - num_adversaries}",
                collide=True,
                shape=Sphere(radius=self.adversary_radius if adversary else 0.05),
                u_multiplier=3.0 if adversary else 4.0,
                max_speed=1.0 if adversary else 1.3,
                color=Color.RED if adversary else Color.GREEN,
                adversary=adversary,
            ))
        for i in range(num_landmarks):
            world.add_landmark(Landmark(name=f"landmark {i}", collide=True, shape=Sphere(radius=0.2), color=Color.BLACK))
        return world

    def _draws(self):
        """(entity, lo, hi) per uniform_ call of a full reset, in call order: the agents over +-bound,
        then the landmarks over +-(bound - 0.1) (Python doubles, rounded by uniform_ itself)."""
        w = self.world
        inner = self.bound - 0.1
        return [(a, -self.bound, self.bound) for a in w.agents] + [(m, -inner, inner) for m in w.landmarks]

    def reset_world_at(self, env_index: int = None):
        w = self.world
        rows = 1 if env_index is not None else w.batch_dim
        for entity, lo, hi in self._draws():
            spot = torch.zeros((rows, w.dim_p), device=w.device, dtype=torch.float32).uniform_(lo, hi)
            entity.set_pos(spot, batch_index=env_index)

    # ---- masked reset (Environment.reset_where; csrc/vmas_reset.hip k_uniform_reset) --------------
    # The rows of `mask` as reset_world_at(None) after World.reset leaves them, in place, in ONE
    # launch with no host wait (simulator/environment/_uniform_reset.py).
    native_resets = 0  # launches made (a test's proof that no fall-back ran)

    def reset_world_where(self, mask):
        from vectorizedmultiagentsimulator_amd.simulator.environment._uniform_reset import uniform_reset_where

        return uniform_reset_where(self, mask, [(e, "pos", lo, hi) for e, lo, hi in self._draws()])

    # ---- teams ------------------------------------------------------------------------------------
    def good_agents(self):
        return [a for a in self.world.agents if not a.adversary]

    def adversaries(self):
        return [a for a in self.world.agents if a.adversary]

    def is_collision(self, agent1: Agent, agent2: Agent) -> Tensor:
        dist = norm2(agent1.state.pos - agent2.state.pos)
        return dist < agent1.shape.radius + agent2.shape.radius  # (the sum in double, compared as fp32)

    # ---- reward / observation: the torch program (the definition) ----------------------------------
    def _torch_reward(self, agent: Agent):
        w = self.world
        if agent is w.agents[0]:
            for a in w.agents:
                a.rew = self.adversary_reward(a) if a.adversary else self.agent_reward(a)
            self.agents_rew = torch.stack([a.rew for a in self.good_agents()], dim=-1).sum(-1)
            self.adverary_rew = torch.stack([a.rew for a in self.adversaries()], dim=-1).sum(-1)
            if self.respawn_at_catch:
                for a in self.good_agents():
                    for adv in self.adversaries():
                        caught = self.is_collision(a, adv).unsqueeze(-1)
                        spot = torch.zeros((w.batch_dim, w.dim_p), device=w.device,
                                           dtype=torch.float32).uniform_(-self.bound, self.bound)
                        a.state.pos = torch.where(caught, spot, a.state.pos)
                        a.state.vel = torch.where(caught, 0.0, a.state.vel)
        if agent.adversary:
            return self.adverary_rew if self.adversaries_share_rew else agent.rew
        return self.agents_rew if self.agents_share_rew else agent.rew

    def agent_reward(self, agent: Agent) -> Tensor:
        """A good agent: minus 10 per adversary touching it; shaped: plus 0.1 x its distance to each."""
        rew = torch.zeros(self.world.batch_dim, device=self.world.device, dtype=torch.float32)
        adversaries = self.adversaries()
        if self.shape_agent_rew:
            for adv in adversaries:
                rew = rew + 0.1 * norm2(agent.state.pos - adv.state.pos)
        if agent.collide:
            for adv in adversaries:
                rew = torch.where(self.is_collision(adv, agent), rew - 10, rew)
        return rew

    def adversary_reward(self, agent: Agent) -> Tensor:
        """An adversary: plus 10 per good agent it touches; shaped: minus 0.1 x its distance to the nearest."""
        rew = torch.zeros(self.world.batch_dim, device=self.world.device, dtype=torch.float32)
        agents = self.good_agents()
        if self.shape_adversary_rew:
            rew = rew - 0.1 * torch.min(
                torch.stack([norm2(a.state.pos - agent.state.pos) for a in agents], dim=-1),
                dim=-1)[0]
        if agent.collide:
            for a in agents:
                rew = torch.where(self.is_collision(a, agent), rew + 10, rew)
        return rew

    def _others(self, agent: Agent):
        """(other, its index, whether its velocity is observed too) per other agent `agent` observes."""
        seen = []
        for j, other in enumerate(self.world.agents):
            if other is agent:
                continue
            if other.adversary == agent.adversary and not self.observe_same_team:
                continue
            seen.append((other, j, not other.adversary))  # (nobody sees an adversary's velocity)
        return seen

    def _torch_observation(self, agent: Agent):
        pos = agent.state.pos
        seen = self._others(agent)
        cols = ([agent.state.vel] if self.observe_vel else []) + ([pos] if self.observe_pos else [])
        cols += [mark.state.pos - pos for mark in self.world.landmarks]
        cols += [other.state.pos - pos for other, _, _ in seen]
        cols += [other.state.vel for other, _, with_vel in seen if with_vel]
        return torch.cat(cols, dim=-1)

    def extra_render(self, env_index: int = 0):
        """The perimeter the agents' rims can reach: four lines at +-(bound + adversary_radius)."""
        from vectorizedmultiagentsimulator_amd.simulator import rendering

        geoms = []
        edge = self.bound + self.adversary_radius
        length = 2 * ((self.bound - self.adversary_radius) + self.adversary_radius * 2)
        for i in range(4):
            geom = Line(length=length).get_geometry()
            xform = rendering.Transform()
            geom.add_attr(xform)
            if i % 2:  # a horizontal line at y = +-edge
                xform.set_translation(0.0, edge if i == 1 else -edge)
                xform.set_rotation(0.0)
            else:  # a vertical line at x = +-edge
                xform.set_translation(edge if i == 0 else -edge, 0.0)
                xform.set_rotation(torch.pi / 2)
            geom.set_color(*Color.BLACK.value)
            geoms.append(geom)
        return geoms

    # ---- the native program's task (simulator/_mpe.py; csrc/vmas_mpe_programs.hpp tag_reward) -------
    _mpe_task = N.VMAS_MPE_TAG

    def _mpe_decline(self):
        if self.respawn_at_catch:
            return "respawn_at_catch"
        if not self.good_agents() or not self.adversaries():
            return "a team is empty"
        return None

    def _mpe_terms(self, agent: Agent):
        seen = self._others(agent)
        terms = ([(N.VMAS_MPE_SELF_VEL, 0)] if self.observe_vel else []) + ([(N.VMAS_MPE_SELF_POS, 0)] if self.observe_pos else [])
        terms += [(N.VMAS_MPE_REL_LANDMARK, j) for j in range(len(self.world.landmarks))]
        terms += [(N.VMAS_MPE_REL_AGENT, j) for _, j, _ in seen]
        terms += [(N.VMAS_MPE_AGENT_VEL, j) for _, j, with_vel in seen if with_vel]
        return terms

    def _mpe_fill(self, io, dev):
        agents = self.world.agents
        io.adversary_mask = sum(1 << i for i, a in enumerate(agents) if a.adversary)
        io.shape_agent_rew, io.shape_adversary_rew = int(bool(self.shape_agent_rew)), int(bool(self.shape_adversary_rew))
        io.agents_share_rew, io.adversaries_share_rew = int(bool(self.agents_share_rew)), int(bool(self.adversaries_share_rew))
        for i, a in enumerate(agents):
            for j, b in enumerate(agents):
                io.thr[i * N.VMAS_MPE_MAX_AGENTS + j] = float(np.float32(a.shape.radius + b.shape.radius))
        # the team sums in the order of torch's .sum(-1) on this device (probed once per device and n)
        modes = [_fused.reduce_order(dev, len(team), "sum", N.VMAS_MPE_MAX_AGENTS)
                 for team in (self.good_agents(), self.adversaries())]
        if None in modes:
            raise NotFusable("no summation order reproduces torch's .sum(-1) on this device")
        io.sum_mode_good, io.sum_mode_adv = modes

    def _mpe_scenario_outputs(self, io, B, dev):
        f32 = dict(device=dev, dtype=torch.float32)
        out = {"agents_rew": torch.empty(B, **f32), "adverary_rew": torch.empty(B, **f32),
               "rew": [torch.empty(B, **f32) for _ in self.world.agents]}
        io.agents_rew, io.adverary_rew = out["agents_rew"].data_ptr(), out["adverary_rew"].data_ptr()
        for i, t in enumerate(out["rew"]):
            io.agent_rew[i] = t.data_ptr()
        return out

    def _mpe_bind(self, out):
        self.agents_rew, self.adverary_rew = out["agents_rew"], out["adverary_rew"]
        for a, t in zip(self.world.agents, out["rew"]):
            a.rew = t

    def _mpe_bound(self):
        return [self.agents_rew, self.adverary_rew] + [a.rew for a in self.world.agents]
