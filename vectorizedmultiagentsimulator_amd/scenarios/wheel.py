# Derived from VMAS, Copyright (c) 2022-2024 ProrokLab (https://www.proroklab.org/), licensed under
# GPL-3.0; modified for this MI355X build.  See NOTICE.md.
"""Wheel: the agents push a heavy line, pinned at the origin, so that it turns at a wanted speed.

Restates vmas/scenarios/wheel.py:14-110 (``Scenario``; the reference's ``HeuristicPolicy`` and
``render_interactively`` are not part of this build).  The line is the one collidable body that
rotates but never translates (``movable=False, rotatable=True``); every agent's reward is minus the
distance of the line's angular speed from ``desired_velocity``, and an observation holds the agent's
state, the line's centre and two ends relative to the agent, the line's angle modulo pi and its speed.
"""
import ctypes
import math

import torch
from torch import Tensor

from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd.simulator import _fused
from vectorizedmultiagentsimulator_amd.simulator.core import Agent, Landmark, Line, Sphere, World
from vectorizedmultiagentsimulator_amd.simulator.scenario import BaseScenario
from vectorizedmultiagentsimulator_amd.simulator.utils import Color, ScenarioUtils

OBS_WIDTH = 13


class Scenario(BaseScenario):
    # Re-bound by the first agent's reward before anything in the step reads it: graph replays need
    # not carry it (environment/_graph.py _write_only).
    _vmas_graph_write_only = frozenset({"rew"})

    def make_world(self, batch_dim: int, device: torch.device, **kwargs):
        n_agents = kwargs.pop("n_agents", 4)
        self.line_length = kwargs.pop("line_length", 2)
        line_mass = kwargs.pop("line_mass", 30)
        self.desired_velocity = kwargs.pop("desired_velocity", 0.05)
        ScenarioUtils.check_kwargs_consumed(kwargs)

        world = World(batch_dim, device)
        for i in range(n_agents):
            # Constraint: all agents have same action range and multiplier
            world.add_agent(Agent(name=f"agent_{i}", u_multiplier=0.6, shape=Sphere(0.03)))
        self.line = Landmark(name="line", collide=True, rotatable=True, shape=Line(length=self.line_length),
                             mass=line_mass, color=Color.BLACK)
        world.add_landmark(self.line)
        world.add_landmark(Landmark(name="center", shape=Sphere(radius=0.02), collide=False, color=Color.BLACK))
        return world

    def reset_world_at(self, env_index: int = None):
        w = self.world
        rows = 1 if env_index is not None else w.batch_dim
        for agent in w.agents:  # one [rows, 2] draw over [-1, 1) per agent, in agent order
            spawn = torch.zeros((rows, w.dim_p), device=w.device, dtype=torch.float32).uniform_(-1.0, 1.0)
            agent.set_pos(spawn, batch_index=env_index)
        angle = torch.zeros((rows, 1), device=w.device, dtype=torch.float32).uniform_(-torch.pi / 2, torch.pi / 2)
        self.line.set_rot(angle, batch_index=env_index)

    # ---- masked reset (Environment.reset_where; csrc/vmas_reset.hip k_uniform_reset) --------------
    # The rows of `mask` as reset_world_at(None) after World.reset leaves them, in place, in ONE
    # launch with no host wait: the full reset is a fixed list of uniform_ calls, so the generator
    # advance is known before the call (simulator/environment/_uniform_reset.py).
    native_resets = 0  # launches made (a test's proof that no fall-back ran)

    def reset_world_where(self, mask):
        from vectorizedmultiagentsimulator_amd.simulator.environment._uniform_reset import uniform_reset_where

        w = self.world
        center = [e for e in w.landmarks if e is not self.line]
        draws = [(a, "pos", -1.0, 1.0) for a in w.agents] + [(self.line, "rot", -torch.pi / 2, torch.pi / 2)]
        return uniform_reset_where(self, mask, draws, fixed=[(e, 0.0, 0.0) for e in center])

    # ---- reward / observation ---------------------------------------------------------------------
    def reward(self, agent: Agent):
        if _fused.enabled(self.world) and self._fused_plan() is not None:
            return self._fused_reward(agent)
        return self._torch_reward(agent)

    def _speed_error(self) -> Tensor:
        return (self.line.state.ang_vel.abs() - self.desired_velocity).abs()

    def _torch_reward(self, agent: Agent):
        if agent is self.world.agents[0]:
            self.rew = self._speed_error()
        return -self.rew

    def observation(self, agent: Agent):
        if _fused.enabled(self.world) and self._fused_plan() is not None:
            return self._fused_observation(agent)
        return self._torch_observation(agent)

    def _torch_observation(self, agent: Agent):
        line, pos = self.line.state, agent.state.pos
        half = self.line_length / 2
        end = torch.cat([half * torch.cos(line.rot), half * torch.sin(line.rot)], dim=1)
        return torch.cat(
            [pos, agent.state.vel, line.pos - pos, end - pos, -end - pos, line.rot % torch.pi, line.ang_vel.abs(),
             self._speed_error()],
            dim=-1,
        )

    # ---- fused program (GPU worlds; csrc/vmas_scenarios.hip k_wheel) -------------------------------
    # The first agent's reward call runs one launch: ``rew``, every agent's reward and every agent's
    # observation (include/vmas_mi355x.h VmasWheelIO).  The other calls hand out the precomputed
    # tensors while the inputs are unchanged (_fused.state_key); otherwise the call recomputes.

    def _plan_reason(self):
        agents = self.world.agents
        if not 1 <= len(agents) <= N.VMAS_WHEEL_MAX_AGENTS:
            return f"{len(agents)} agents (VMAS_WHEEL_MAX_AGENTS = {N.VMAS_WHEEL_MAX_AGENTS})"
        if not all(type(a.shape).__name__ == "Sphere" for a in agents):
            return "an agent is not a sphere"
        if type(self.line.shape).__name__ != "Line":
            return "the line is not a Line"
        return None

    def _fused_plan(self):
        w = self.world
        sig = (tuple(id(a) for a in w.agents), id(self.line), w.batch_dim, str(w.device))
        plan = getattr(self, "_fplan", None)
        if plan is not None and plan[0] == sig:
            return plan[1]
        dev = torch.device(w.device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        why = self._plan_reason()
        info = {"dev": dev} if why is None else None
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
        return f"torch: {self._fwhy}"

    def _fused_inputs(self):
        line = self.line.state
        ts = [line.pos, line.rot, line.ang_vel]
        for a in self.world.agents:
            ts += [a.state.pos, a.state.vel]
        return ts

    def _launch_args(self, dev):
        """(device index, stream) of a launch; a CPU world: the library's host backend (the ABI's
        device -1; reached only by direct calls of _run_fused)."""
        return (dev.index, _fused.stream(self.world)) if dev.type == "cuda" else (-1, None)

    def _run_fused(self, what: int):
        w = self.world
        dev = self._fused_plan()["dev"]
        B, agents = w.batch_dim, w.agents
        n = len(agents)
        keep = []
        io = N.VmasWheelIO()
        io.batch, io.n_agents, io.what = B, n, what
        io.half_length, io.desired_velocity, io.pi = self.line_length / 2, float(self.desired_velocity), math.pi
        for t, shape in ((self.line.state.pos, (B, 2)), (self.line.state.rot, (B, 1)), (self.line.state.ang_vel, (B, 1))):
            if t.shape != shape or t.requires_grad:
                raise _NotFusable
        for a in agents:
            if a.state.pos.shape != (B, 2) or a.state.vel.shape != (B, 2):
                raise _NotFusable
        line = self.line.state
        io.line_pos = _fused.vec(_fused.f32(line.pos, dev), keep)
        io.line_rot = _fused.vec(_fused.f32(line.rot, dev), keep)
        io.line_ang_vel = _fused.vec(_fused.f32(line.ang_vel, dev), keep)
        out = {}
        # (graph-mode capture: obs / rewards written straight into each replay's fresh tensors)
        io.out_delta, direct = _fused.direct_outputs(w, (
            (torch.float32, (B, OBS_WIDTH), n) if what & N.VMAS_SCN_OBS else None,
            (torch.float32, (B, 1), n) if what & N.VMAS_SCN_REWARD else None,
            None))
        if what & N.VMAS_SCN_REWARD:
            out["rew"] = torch.empty(B, 1, device=dev, dtype=torch.float32)
            out["rewards"] = direct[1] or [torch.empty(B, 1, device=dev, dtype=torch.float32) for _ in agents]
            io.rew = out["rew"].data_ptr()
        if what & N.VMAS_SCN_OBS:
            out["obs"] = direct[0] or [torch.empty(B, OBS_WIDTH, device=dev, dtype=torch.float32) for _ in agents]
        for i, a in enumerate(agents):
            io.pos[i] = _fused.vec(_fused.f32(a.state.pos, dev), keep)
            io.vel[i] = _fused.vec(_fused.f32(a.state.vel, dev), keep)
            if what & N.VMAS_SCN_REWARD:
                io.rewards[i] = out["rewards"][i].data_ptr()
            if what & N.VMAS_SCN_OBS:
                io.obs[i] = out["obs"][i].data_ptr()
        idx, stream = self._launch_args(dev)
        _fused.check(_fused.lib().vmas_wheel_outputs(idx, ctypes.byref(io), stream), "vmas_wheel_outputs")
        if what & N.VMAS_SCN_REWARD:
            self.rew = out["rew"]  # the first agent's reward call re-binds it
        return out

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
                "rew": {k: (out["rewards"][k], _fused.state_key([self.rew])) for k in range(len(agents))},
                "obs": dict(enumerate(out["obs"])),
            }
        c = getattr(self, "_fc", None)
        if c is not None and i in c["rew"]:
            r, k = c["rew"].pop(i)
            if k == _fused.state_key([self.rew]):
                return r
        # (an operand changed under the cache: the reference's expression on the current tensor)
        return -self.rew

    def _fused_observation(self, agent: Agent):
        i = self.world.agents.index(agent)
        c = getattr(self, "_fc", None)
        if c is None or i not in c["obs"] or c["key"] != _fused.state_key(self._fused_inputs()):
            try:
                out = self._run_fused(N.VMAS_SCN_OBS)
            except _NotFusable:
                return self._torch_observation(agent)
            c = self._fc = {"key": _fused.state_key(self._fused_inputs()), "rew": {}, "obs": dict(enumerate(out["obs"]))}
        return c["obs"].pop(i)


class _NotFusable(Exception):
    """An operand the fused kernel does not take (dtype / layout / device): the torch program runs."""
