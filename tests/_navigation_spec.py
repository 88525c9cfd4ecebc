# Derived from VMAS, Copyright (c) 2022-2024 ProrokLab (https://www.proroklab.org/), licensed under
# GPL-3.0; modified for this MI355X build.  See NOTICE.md.
"""The yardstick of the navigation scenario's per-step program: a literal transcription of the
reference's ``reward`` / ``agent_reward`` / ``observation`` / ``done`` / ``info``
(vmas/scenarios/navigation.py:199-284) on plain CPU tensors taken from a world snapshot.

The reference cannot be run on this Python, so there are no recorded
vectors; as tests/_render_spec.py does for rendering, this module restates what the reference
computes, independently of the scenario under test (it never imports the scenario file): boolean
masks and in-place ``[:] = 0`` exactly as written there, ``World.collides`` and the distance
query through the CPU oracle, the LIDAR from ``OracleWorld.cast_rays`` as
tests/golden/make_golden.py calls it.

``NavigationSpec(env)`` reads the parameters and the carried ``pos_shaping`` from a built env,
``run()`` evaluates one step's outputs in the environment's order (every reward, every
observation, every info, done).
"""
from typing import Dict

import torch
from torch import Tensor

from oracle import vmas_oracle as O

PARAMS = ("shared_rew", "observe_all_goals", "collisions", "pos_shaping_factor", "final_reward",
          "agent_collision_penalty", "min_collision_distance")


class _World:
    """The three World members the reference's program touches, over the oracle's stand-ins."""

    def __init__(self, ow, agents):
        self.ow = ow
        self.agents = agents
        self._collidable_pairs = ow._collidable_pairs

    def collides(self, a, b) -> bool:  # core.py:2787-2802
        if (not a.e.collides(b.e)) or (not b.e.collides(a.e)) or a is b:
            return False
        a_shape = a.shape
        b_shape = b.shape
        if not a.movable and not a.rotatable and not b.movable and not b.rotatable:
            return False
        if not {a_shape.__class__, b_shape.__class__} in self._collidable_pairs:
            return False
        if not (
            torch.linalg.vector_norm(a.state.pos - b.state.pos, dim=-1)
            <= a.shape.circumscribed_radius() + b.shape.circumscribed_radius()
        ).any():
            return False
        return True

    def get_distance(self, a, b):
        return self.ow.get_distance(a, b)


class _Sensor:
    """Lidar.measure (sensors.py:107-128) through the oracle's World.cast_rays."""

    def __init__(self, ow, entity_index, sensor, rot):
        self.ow, self.i, self.sensor, self.rot = ow, entity_index, sensor, rot
        self._max_range = sensor._max_range
        self._last_measurement = None

    def measure(self):
        angles = self.sensor._angles.detach().cpu() + self.rot
        self._last_measurement = self.ow.cast_rays(self.i, angles, self._max_range, self.sensor.entity_filter)
        return self._last_measurement


class NavigationSpec:
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
            sa.goal = ow.ents[ents.index(a.goal)]
            sa.pos_shaping = a.pos_shaping.detach().cpu().clone()
            sa.pos_rew = a.pos_rew.detach().cpu().clone()
            sa.agent_collision_rew = a.agent_collision_rew.detach().cpu().clone()
            sa.sensors = [_Sensor(ow, ents.index(a), s, snap[ents.index(a)]["rot"]) for s in (a.sensors or [])]
            agents.append(sa)
        self.world = _World(ow, agents)
        self.pos_rew = scn.pos_rew.detach().cpu().clone()
        self.final_rew = scn.final_rew.detach().cpu().clone()

    # ---- navigation.py:199-284, as written ----------------------------------------------------
    def reward(self, agent):
        is_first = agent == self.world.agents[0]

        if is_first:
            self.pos_rew[:] = 0
            self.final_rew[:] = 0

            for a in self.world.agents:
                self.pos_rew += self.agent_reward(a)
                a.agent_collision_rew[:] = 0

            self.all_goal_reached = torch.all(
                torch.stack([a.on_goal for a in self.world.agents], dim=-1),
                dim=-1,
            )

            self.final_rew[self.all_goal_reached] = self.final_reward

            for i, a in enumerate(self.world.agents):
                for j, b in enumerate(self.world.agents):
                    if i <= j:
                        continue
                    if self.world.collides(a, b):
                        distance = self.world.get_distance(a, b)
                        a.agent_collision_rew[
                            distance <= self.min_collision_distance
                        ] += self.agent_collision_penalty
                        b.agent_collision_rew[
                            distance <= self.min_collision_distance
                        ] += self.agent_collision_penalty

        pos_reward = self.pos_rew if self.shared_rew else agent.pos_rew
        return pos_reward + self.final_rew + agent.agent_collision_rew

    def agent_reward(self, agent):
        agent.distance_to_goal = torch.linalg.vector_norm(
            agent.state.pos - agent.goal.state.pos,
            dim=-1,
        )
        agent.on_goal = agent.distance_to_goal < agent.goal.shape.radius

        pos_shaping = agent.distance_to_goal * self.pos_shaping_factor
        agent.pos_rew = agent.pos_shaping - pos_shaping
        agent.pos_shaping = pos_shaping
        return agent.pos_rew

    def observation(self, agent):
        goal_poses = []
        if self.observe_all_goals:
            for a in self.world.agents:
                goal_poses.append(agent.state.pos - a.goal.state.pos)
        else:
            goal_poses.append(agent.state.pos - agent.goal.state.pos)
        return torch.cat(
            [
                agent.state.pos,
                agent.state.vel,
            ]
            + goal_poses
            + (
                [agent.sensors[0]._max_range - agent.sensors[0].measure()]
                if self.collisions
                else []
            ),
            dim=-1,
        )

    def done(self):
        return torch.stack(
            [
                torch.linalg.vector_norm(
                    agent.state.pos - agent.goal.state.pos,
                    dim=-1,
                )
                < agent.shape.radius
                for agent in self.world.agents
            ],
            dim=-1,
        ).all(-1)

    def info(self, agent) -> Dict[str, Tensor]:
        return {
            "pos_rew": self.pos_rew if self.shared_rew else agent.pos_rew,
            "final_rew": self.final_rew,
            "agent_collisions": agent.agent_collision_rew,
        }

    # ---- one step's outputs, in the environment's order (environment.py:260-330) ---------------
    def run(self):
        agents = self.world.agents
        rewards = [self.reward(a).clone() for a in agents]
        obs = [self.observation(a) for a in agents]
        infos = [{k: v.clone() for k, v in self.info(a).items()} for a in agents]
        return {"obs": obs, "rewards": rewards, "infos": infos, "done": self.done()}

    def attributes(self):
        """The scenario attributes the program leaves behind, in a fixed order."""
        out = [self.pos_rew, self.final_rew, self.all_goal_reached]
        for a in self.world.agents:
            out += [a.distance_to_goal, a.on_goal, a.pos_rew, a.pos_shaping, a.agent_collision_rew]
        return out


def scenario_attributes(env):
    """The same attributes of a built env, in the spec's order."""
    scn = env.scenario
    out = [scn.pos_rew, scn.final_rew, scn.all_goal_reached]
    for a in env.world.agents:
        out += [a.distance_to_goal, a.on_goal, a.pos_rew, a.pos_shaping, a.agent_collision_rew]
    return out


def place_cases(env):
    """Overwrite positions by hand so that every branch of the program occurs (64+ envs):
    envs 0-7 every agent within 0.5 * goal.shape.radius of its goal; envs 8-15 agents 0 and 1 with
    centres 2 * agent_radius - 0.01 apart (needs two agents); envs 16-23 agent 0 inside
    agent.shape.radius but outside goal.shape.radius of its goal, the others on theirs."""
    w = env.world
    agents = w.agents
    dev = w.device
    for a in agents:
        pos, goal = a.state.pos.clone(), a.goal.state.pos
        pos[0:8] = goal[0:8] + torch.tensor([0.5 * a.goal.shape.radius, 0.0], device=dev)
        pos[16:24] = goal[16:24] + torch.tensor([0.0, 0.25 * a.goal.shape.radius], device=dev)
        a.set_pos(pos, batch_index=None)
    a0 = agents[0]
    between = 0.5 * (a0.shape.radius + a0.goal.shape.radius)
    assert a0.goal.shape.radius < between < a0.shape.radius
    pos = a0.state.pos.clone()
    pos[16:24] = a0.goal.state.pos[16:24] + torch.tensor([between, 0.0], device=dev)
    a0.set_pos(pos, batch_index=None)
    if len(agents) > 1:
        a1 = agents[1]
        pos = a1.state.pos.clone()
        pos[8:16] = a0.state.pos[8:16] + torch.tensor([2 * a0.shape.radius - 0.01, 0.0], device=dev)
        a1.set_pos(pos, batch_index=None)
