# Derived from VMAS, Copyright (c) 2022-2024 ProrokLab (https://www.proroklab.org/), licensed under
# GPL-3.0; modified for this MI355X build.  See NOTICE.md.
"""Navigation: every agent drives to its own goal, seeing the other agents through a LIDAR.

Restates vmas/scenarios/navigation.py:21-311 (``Scenario``; the reference's cvxpy ``HeuristicPolicy``
and ``render_interactively`` are not part of this build).  Each agent is a sphere with one LIDAR
that sees agents only (present only when ``collisions``), and owns a non-colliding goal landmark.
"""
import ctypes
from typing import Dict

import torch
from torch import Tensor

from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd.simulator import _fused
from vectorizedmultiagentsimulator_amd.simulator.core import Agent, Landmark, Sphere, World
from vectorizedmultiagentsimulator_amd.simulator.scenario import BaseScenario
from vectorizedmultiagentsimulator_amd.simulator.sensors import Lidar
from vectorizedmultiagentsimulator_amd.simulator.utils import Color, ScenarioUtils


class Scenario(BaseScenario):
    # Re-bound by the first agent's reward before anything in the step reads them (info and done
    # read them after the reward): graph replays need not carry them (environment/_graph.py
    # _write_only).  agent.pos_shaping is read by the reward and stays carried; self.pos_rew /
    # self.final_rew / agent.agent_collision_rew are written in place.
    _vmas_graph_write_only = frozenset({"all_goal_reached"})
    _vmas_graph_write_only_agents = frozenset({"distance_to_goal", "on_goal", "pos_rew"})

    def make_world(self, batch_dim: int, device: torch.device, **kwargs):
        self.plot_grid = False
        self.n_agents = kwargs.pop("n_agents", 4)
        self.collisions = kwargs.pop("collisions", True)
        self.world_spawning_x = kwargs.pop("world_spawning_x", 1)  # X-coordinate limit for entities spawning
        self.world_spawning_y = kwargs.pop("world_spawning_y", 1)  # Y-coordinate limit for entities spawning
        # If False, the world is unlimited; else, constrained by world_spawning_x and world_spawning_y.
        self.enforce_bounds = kwargs.pop("enforce_bounds", False)
        self.agents_with_same_goal = kwargs.pop("agents_with_same_goal", 1)
        self.split_goals = kwargs.pop("split_goals", False)
        self.observe_all_goals = kwargs.pop("observe_all_goals", False)
        self.lidar_range = kwargs.pop("lidar_range", 0.35)
        self.agent_radius = kwargs.pop("agent_radius", 0.1)
        self.comms_range = kwargs.pop("comms_range", 0)
        self.n_lidar_rays = kwargs.pop("n_lidar_rays", 12)
        self.shared_rew = kwargs.pop("shared_rew", True)
        self.pos_shaping_factor = kwargs.pop("pos_shaping_factor", 1)
        self.final_reward = kwargs.pop("final_reward", 0.01)
        self.agent_collision_penalty = kwargs.pop("agent_collision_penalty", -1)
        ScenarioUtils.check_kwargs_consumed(kwargs)

        self.min_distance_between_entities = self.agent_radius * 2 + 0.05
        self.min_collision_distance = 0.005

        if self.enforce_bounds:
            self.x_semidim = self.world_spawning_x
            self.y_semidim = self.world_spawning_y
        else:
            self.x_semidim = None
            self.y_semidim = None

        assert 1 <= self.agents_with_same_goal <= self.n_agents
        if self.agents_with_same_goal > 1:
            assert not self.collisions, "If agents share goals they cannot be collidables"
        # agents_with_same_goal == n_agents: all agent same goal
        # agents_with_same_goal = x: the first x agents share the goal
        # agents_with_same_goal = 1: all independent goals
        if self.split_goals:
            assert self.n_agents % 2 == 0 and self.agents_with_same_goal == self.n_agents // 2, (
                "Splitting the goals is allowed when the agents are even and half the team has the same goal"
            )

        world = World(batch_dim, device, substeps=2, x_semidim=self.x_semidim, y_semidim=self.y_semidim)

        known_colors = [
            (0.22, 0.49, 0.72),
            (1.00, 0.50, 0),
            (0.30, 0.69, 0.29),
            (0.97, 0.51, 0.75),
            (0.60, 0.31, 0.64),
            (0.89, 0.10, 0.11),
            (0.87, 0.87, 0),
        ]
        colors = torch.randn((max(self.n_agents - len(known_colors), 0), 3), device=device)

        def entity_filter_agents(e):
            return isinstance(e, Agent)

        for i in range(self.n_agents):
            color = known_colors[i] if i < len(known_colors) else colors[i - len(known_colors)]
            # Constraint: all agents have same action range and multiplier
            agent = Agent(
                name=f"agent_{i}",
                collide=self.collisions,
                color=color,
                shape=Sphere(radius=self.agent_radius),
                render_action=True,
                sensors=(
                    [Lidar(world, n_rays=self.n_lidar_rays, max_range=self.lidar_range,
                           entity_filter=entity_filter_agents)]
                    if self.collisions
                    else None
                ),
            )
            agent.pos_rew = torch.zeros(batch_dim, device=device)
            agent.agent_collision_rew = agent.pos_rew.clone()
            world.add_agent(agent)

            goal = Landmark(name=f"goal {i}", collide=False, color=color)
            world.add_landmark(goal)
            agent.goal = goal

        self.pos_rew = torch.zeros(batch_dim, device=device)
        self.final_rew = self.pos_rew.clone()
        return world

    def reset_world_at(self, env_index: int = None):
        w = self.world
        x_bounds = (-self.world_spawning_x, self.world_spawning_x)
        y_bounds = (-self.world_spawning_y, self.world_spawning_y)
        ScenarioUtils.spawn_entities_randomly(
            w.agents, w, env_index, self.min_distance_between_entities, x_bounds, y_bounds,
        )
        occupied_positions = torch.stack([agent.state.pos for agent in w.agents], dim=1)
        if env_index is not None:
            occupied_positions = occupied_positions[env_index].unsqueeze(0)

        goal_poses = []
        for _ in w.agents:
            position = ScenarioUtils.find_random_pos_for_entity(
                occupied_positions=occupied_positions,
                env_index=env_index,
                world=w,
                min_dist_between_entities=self.min_distance_between_entities,
                x_bounds=x_bounds,
                y_bounds=y_bounds,
            )
            goal_poses.append(position.squeeze(1))
            occupied_positions = torch.cat([occupied_positions, position], dim=1)

        for i, agent in enumerate(w.agents):
            if self.split_goals:
                goal_index = int(i // self.agents_with_same_goal)
            else:
                goal_index = 0 if i < self.agents_with_same_goal else i
            agent.goal.set_pos(goal_poses[goal_index], batch_index=env_index)
            if env_index is None:
                agent.pos_shaping = (
                    torch.linalg.vector_norm(agent.state.pos - agent.goal.state.pos, dim=1) * self.pos_shaping_factor
                )
            else:
                agent.pos_shaping[env_index] = (
                    torch.linalg.vector_norm(agent.state.pos[env_index] - agent.goal.state.pos[env_index])
                    * self.pos_shaping_factor
                )

    # ---- masked reset (Environment.reset_where; csrc/vmas_reset.hip vmas_spawn_reset) -----------
    # The rows of `mask` as reset_world_at(None) after World.reset leaves them, in place: the agents
    # and then one goal position per agent placed by the reference's loop on the device, every
    # agent's goal at the position its goal index names, pos_shaping from the new positions.
    native_resets = 0           # calls the launch chain answered (a test's proof that no fall-back ran)
    native_reset_fallbacks = 0  # calls handed to the generic path because an env passed spawn_max_tries
    spawn_max_tries = 0         # tries per entity before that happens (0: the kernel's limit)

    def reset_world_where(self, mask):
        from vectorizedmultiagentsimulator_amd.simulator.environment._spawn_reset import spawn_reset_where

        agents = self.world.agents
        if any(not isinstance(getattr(a, "pos_shaping", None), Tensor) for a in agents):
            return NotImplemented
        writes, derived = [], []
        for i, a in enumerate(agents):
            if self.split_goals:
                goal_index = int(i // self.agents_with_same_goal)
            else:
                goal_index = 0 if i < self.agents_with_same_goal else i
            writes += [(a, ("agent", i)), (a.goal, ("goal", goal_index))]
            derived.append(("norm", ("agent", i), ("goal", goal_index), self.pos_shaping_factor, a.pos_shaping))
        n = len(agents)
        keys = [("agent", i) for i in range(n)] + [("goal", i) for i in range(n)]
        return spawn_reset_where(
            self, mask, [(keys, self.min_distance_between_entities)], writes,
            (-self.world_spawning_x, self.world_spawning_x), (-self.world_spawning_y, self.world_spawning_y),
            derived=derived, max_tries=self.spawn_max_tries)

    def reward(self, agent: Agent):
        if _fused.enabled(self.world) and self._fused_plan() is not None:
            return self._fused_reward(agent)
        return self._torch_reward(agent)

    def _torch_reward(self, agent: Agent):
        w = self.world
        is_first = agent == w.agents[0]
        if is_first:
            self.pos_rew[:] = 0
            self.final_rew[:] = 0
            for a in w.agents:
                self.pos_rew += self.agent_reward(a)
                a.agent_collision_rew[:] = 0
            self.all_goal_reached = torch.all(torch.stack([a.on_goal for a in w.agents], dim=-1), dim=-1)
            # final_rew[all_goal_reached] = final_reward, without a boolean-mask host sync
            self.final_rew[:] = torch.where(self.all_goal_reached, float(self.final_reward), 0.0)
            for i, a in enumerate(w.agents):
                for j, b in enumerate(w.agents):
                    if i <= j:
                        continue
                    if w.collides(a, b):
                        distance = w.get_distance(a, b)
                        # rew[distance <= min] += penalty, for both agents, as torch.where
                        add = torch.where(distance <= self.min_collision_distance,
                                          float(self.agent_collision_penalty), 0.0)
                        a.agent_collision_rew += add
                        b.agent_collision_rew += add
        pos_reward = self.pos_rew if self.shared_rew else agent.pos_rew
        return pos_reward + self.final_rew + agent.agent_collision_rew

    def agent_reward(self, agent: Agent):
        agent.distance_to_goal = torch.linalg.vector_norm(agent.state.pos - agent.goal.state.pos, dim=-1)
        agent.on_goal = agent.distance_to_goal < agent.goal.shape.radius
        pos_shaping = agent.distance_to_goal * self.pos_shaping_factor
        agent.pos_rew = agent.pos_shaping - pos_shaping
        agent.pos_shaping = pos_shaping
        return agent.pos_rew

    def observation(self, agent: Agent):
        if _fused.enabled(self.world) and self._fused_plan() is not None:
            return self._fused_observation(agent)
        return self._torch_observation(agent)

    def _torch_observation(self, agent: Agent):
        goal_poses = []
        if self.observe_all_goals:
            for a in self.world.agents:
                goal_poses.append(agent.state.pos - a.goal.state.pos)
        else:
            goal_poses.append(agent.state.pos - agent.goal.state.pos)
        return torch.cat(
            [agent.state.pos, agent.state.vel]
            + goal_poses
            + ([agent.sensors[0]._max_range - agent.sensors[0].measure()] if self.collisions else []),
            dim=-1,
        )

    def done(self):
        if _fused.enabled(self.world) and self._fused_plan() is not None:
            return self._fused_done()
        return self._torch_done()

    def _torch_done(self):
        return torch.stack(
            [
                torch.linalg.vector_norm(agent.state.pos - agent.goal.state.pos, dim=-1) < agent.shape.radius
                for agent in self.world.agents
            ],
            dim=-1,
        ).all(-1)

    def info(self, agent: Agent) -> Dict[str, Tensor]:
        return {
            "pos_rew": self.pos_rew if self.shared_rew else agent.pos_rew,
            "final_rew": self.final_rew,
            "agent_collisions": agent.agent_collision_rew,
        }

    def extra_render(self, env_index: int = 0):
        """navigation.py:286-311: a line between each pair of agents within comms_range."""
        from vectorizedmultiagentsimulator_amd.simulator import rendering

        geoms = []
        agents = self.world.agents
        for i, agent1 in enumerate(agents):
            for j, agent2 in enumerate(agents):
                if j <= i:
                    continue
                agent_dist = torch.linalg.vector_norm(agent1.state.pos - agent2.state.pos, dim=-1)
                if agent_dist[env_index] <= self.comms_range:
                    color = Color.BLACK.value
                    line = rendering.Line(agent1.state.pos[env_index], agent2.state.pos[env_index], width=1)
                    xform = rendering.Transform()
                    line.add_attr(xform)
                    line.set_color(*color)
                    geoms.append(line)
        return geoms

    # ---- fused program (GPU worlds; csrc/vmas_scenarios.hip k_navigation) ----------------------
    # The first agent's reward call runs one launch: the reward block above for every agent
    # (distance_to_goal, on_goal, the re-bound pos_shaping, pos_rew, the shared pos_rew / final_rew
    # / all_goal_reached, the pairwise collision penalties and every agent's returned reward),
    # every agent's observation with its LIDAR, and done() -- followed, in worlds with collisions, by
    # a one-workgroup launch that settles World.collides' batch-wide test (include/vmas_mi355x.h
    # VmasNavigationIO).  The other reward calls return their
    # precomputed reward, observation / done calls hand out the precomputed tensors -- while the
    # inputs are unchanged (_fused.state_key); otherwise the call recomputes, as the reference
    # does on every call.

    def _fused_plan(self):
        w = self.world
        agents = w.agents
        sig = (tuple(id(a) for a in agents), tuple(id(e) for e in w.entities), w.batch_dim, bool(self.collisions),
               tuple(id(a.goal) for a in agents))
        plan = getattr(self, "_fplan", None)
        if plan is not None and plan[0] == sig:
            return plan[1]
        info = None
        dev = torch.device(w.device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        ok = (1 <= len(agents) <= N.VMAS_NAV_MAX_AGENTS
              and all(type(a.shape).__name__ == "Sphere" and type(a.goal.shape).__name__ == "Sphere" for a in agents))
        R, max_range = 0, 0.0
        if ok and self.collisions:
            for k, a in enumerate(agents):
                if not a.sensors or len(a.sensors) != 1 or type(a.sensors[0]).__name__ != "Lidar":
                    ok = False
                    break
                s = a.sensors[0]
                ts = [e for e in w.entities if e is not a and s.entity_filter(e)]
                if k == 0:
                    R, max_range = s._angles.shape[-1], s._max_range
                # the program's LIDAR targets are the other agents, in order
                if ([id(e) for e in ts] != [id(e) for e in agents if e is not a]
                        or s._angles.shape != (w.batch_dim, R) or s._max_range != max_range):
                    ok = False
                    break
                for e in ts:
                    assert e.collides(a) and a.collides(e), "Rays are only casted among collidables"
        if ok:
            # (the launch's scratch words: pair flags of World.collides' batch-wide test, left zero)
            info = {"dev": dev, "R": R, "max_range": max_range,
                    "ws": torch.zeros(N.VMAS_NAV_WS_WORDS, device=dev, dtype=torch.int32)}
        self._fplan = (sig, info)
        return info

    def _fused_inputs(self):
        ts = []
        for a in self.world.agents:
            ts += [a.state.pos, a.state.vel, a.goal.state.pos]
            if self.collisions:
                ts += [a.state.rot, a.sensors[0]._angles]
        return ts

    def _obs_width(self, R: int) -> int:
        return 4 + 2 * (len(self.world.agents) if self.observe_all_goals else 1) + (R if self.collisions else 0)

    def _run_fused(self, what: int):
        w = self.world
        plan = self._fused_plan()
        dev, R = plan["dev"], plan["R"]
        B = w.batch_dim
        agents = w.agents
        n = len(agents)
        keep = []
        io = N.VmasNavigationIO()
        io.batch, io.n_agents, io.what, io.n_rays = B, n, what, R
        io.shared_rew = 1 if self.shared_rew else 0
        io.observe_all_goals = 1 if self.observe_all_goals else 0
        io.lidar_on = 1 if self.collisions else 0
        io.fast_lidar = 0 if _fused.EXACT_LIDAR else 1
        io.pos_shaping_factor = float(self.pos_shaping_factor)
        io.final_reward = float(self.final_reward)
        io.agent_collision_penalty = float(self.agent_collision_penalty)
        io.min_collision_distance = float(self.min_collision_distance)
        io.max_range = float(plan["max_range"])
        io.ws = plan["ws"].data_ptr()
        W = self._obs_width(R)
        for i, a in enumerate(agents):
            io.agents[i] = _fused.ref(w, a, keep, 0)
            io.goal_pos[i] = _fused.vec(_fused.f32(a.goal.state.pos, dev), keep)
            io.goal_radius[i] = float(a.goal.shape.radius)
            io.circ[i] = float(a.shape.circumscribed_radius())
            # World.collides' static part for the pairs (i, j < i) of the reward's loop
            io.pair_static[i] = sum(1 << j for j in range(i) if w._collides_static(a, agents[j]))
        out = {}
        # (graph-mode capture: obs / rewards / done written straight into each replay's fresh tensors)
        io.out_delta, direct = _fused.direct_outputs(w, (
            (torch.float32, (B, W), n) if what & N.VMAS_SCN_OBS else None,
            (torch.float32, (B,), n) if what & N.VMAS_SCN_REWARD else None,
            (torch.bool, (B,), 1) if what & N.VMAS_SCN_DONE else None))
        if what & N.VMAS_SCN_REWARD:
            for x in (self.pos_rew, self.final_rew):
                if x.dtype is not torch.float32 or not x.is_contiguous() or x.shape != (B,) or x.device != dev:
                    raise _NotFusable
            io.pos_rew, io.final_rew = self.pos_rew.data_ptr(), self.final_rew.data_ptr()
            for k in ("dist", "shaping", "pos_rew"):
                out[k] = [torch.empty(B, device=dev, dtype=torch.float32) for _ in agents]
            out["on_goal"] = [torch.empty(B, device=dev, dtype=torch.bool) for _ in agents]
            out["all_goal"] = torch.empty(B, device=dev, dtype=torch.bool)
            out["rewards"] = direct[1] or [torch.empty(B, device=dev, dtype=torch.float32) for _ in agents]
            io.all_goal_reached = out["all_goal"].data_ptr()
        if what & N.VMAS_SCN_OBS:
            out["obs"] = direct[0] or [torch.empty(B, W, device=dev, dtype=torch.float32) for _ in agents]
            if self.collisions:
                out["lidar"] = [torch.empty(B, R, device=dev, dtype=torch.float32) for _ in agents]
        if what & N.VMAS_SCN_DONE:
            out["done"] = direct[2][0] if direct[2] else torch.empty(B, device=dev, dtype=torch.bool)
            io.done = out["done"].data_ptr()
        for i, a in enumerate(agents):
            if what & N.VMAS_SCN_REWARD:
                sh, cr = a.pos_shaping, a.agent_collision_rew
                for x in (sh, cr):
                    if x.dtype is not torch.float32 or not x.is_contiguous() or x.shape != (B,) or x.device != dev:
                        raise _NotFusable
                keep.append(sh)
                io.shaping_in[i], io.collision_rew[i] = sh.data_ptr(), cr.data_ptr()
                io.shaping_out[i] = out["shaping"][i].data_ptr()
                io.dist_to_goal[i] = out["dist"][i].data_ptr()
                io.on_goal[i] = out["on_goal"][i].data_ptr()
                io.agent_pos_rew[i] = out["pos_rew"][i].data_ptr()
                io.rewards[i] = out["rewards"][i].data_ptr()
            if what & N.VMAS_SCN_OBS:
                io.vel[i] = _fused.vec(_fused.f32(a.state.vel, dev), keep)
                io.obs[i] = out["obs"][i].data_ptr()
                if self.collisions:
                    s = a.sensors[0]
                    io.rot[i] = _fused.vec(_fused.f32(a.state.rot, dev), keep)
                    ang = _fused.f32(s._angles, dev)
                    keep.append(ang)
                    io.angles[i], io.ang_s0[i], io.ang_s1[i] = ang.data_ptr(), ang.stride(0), ang.stride(1)
                    io.lidar[i] = out["lidar"][i].data_ptr()
        _fused.check(_fused.lib().vmas_navigation_outputs(dev.index, ctypes.byref(io), _fused.stream(w)),
                     "vmas_navigation_outputs")
        if what & N.VMAS_SCN_REWARD:
            # the first agent's reward call: every attribute the reference's block leaves behind
            _fused.bump_version(self.pos_rew)
            _fused.bump_version(self.final_rew)
            self.all_goal_reached = out["all_goal"]
            for i, a in enumerate(agents):
                _fused.bump_version(a.agent_collision_rew)
                a.distance_to_goal = out["dist"][i]
                a.on_goal = out["on_goal"][i]
                a.pos_rew = out["pos_rew"][i]
                a.pos_shaping = out["shaping"][i]
        return out

    def _reward_key(self, agent: Agent):
        return _fused.state_key([self.pos_rew, self.final_rew, agent.pos_rew, agent.agent_collision_rew])

    def _obs_cache(self, out):
        n = len(self.world.agents)
        lid = out.get("lidar") or [None] * n
        return {i: (out["obs"][i], lid[i]) for i in range(n)}

    def _fused_reward(self, agent: Agent):
        agents = self.world.agents
        i = agents.index(agent)
        if i == 0:
            try:
                out = self._run_fused(N.VMAS_SCN_REWARD | N.VMAS_SCN_OBS | N.VMAS_SCN_DONE)
            except _NotFusable:
                self._fc = None
                return self._torch_reward(agent)
            self._fc = {
                "key": _fused.state_key(self._fused_inputs()),
                "rew": {k: (out["rewards"][k], self._reward_key(a)) for k, a in enumerate(agents)},
                "obs": self._obs_cache(out),
                "done": out["done"],
            }
        c = getattr(self, "_fc", None)
        if c is not None and i in c["rew"]:
            r, k = c["rew"].pop(i)
            if k == self._reward_key(agent):
                return r
        # (an operand changed under the cache: the reference's expression on the current tensors)
        pos_reward = self.pos_rew if self.shared_rew else agent.pos_rew
        return pos_reward + self.final_rew + agent.agent_collision_rew

    def _fused_observation(self, agent: Agent):
        i = self.world.agents.index(agent)
        c = getattr(self, "_fc", None)
        if c is None or i not in c["obs"] or c["key"] != _fused.state_key(self._fused_inputs()):
            try:
                out = self._run_fused(N.VMAS_SCN_OBS)
            except _NotFusable:
                return self._torch_observation(agent)
            c = self._fc = {"key": _fused.state_key(self._fused_inputs()), "rew": {}, "obs": self._obs_cache(out),
                            "done": None}
        o, lid = c["obs"].pop(i)
        if lid is not None:
            agent.sensors[0]._last_measurement = lid
        return o

    def _fused_done(self):
        c = getattr(self, "_fc", None)
        if c is not None and c["done"] is not None and c["key"] == _fused.state_key(self._fused_inputs()):
            d, c["done"] = c["done"], None
            return d
        try:
            return self._run_fused(N.VMAS_SCN_DONE)["done"]
        except _NotFusable:
            return self._torch_done()


class _NotFusable(Exception):
    """An operand the fused kernel does not take (dtype / layout / device): the torch program runs."""
