"""Host side of the MPE family's step program (csrc/vmas_scenarios.hip k_mpe, include/vmas_mi355x.h
VmasMpeIO): what ``scenarios/mpe/simple_spread.py`` and ``scenarios/mpe/simple_tag.py`` share.

A scenario of the family mixes :class:`MpeProgram` in and provides

* ``_mpe_task``: ``N.VMAS_MPE_SPREAD`` / ``N.VMAS_MPE_TAG``;
* ``_mpe_terms(agent)``: that agent's observation row as ``(kind, index)`` pairs, two columns each;
* ``_mpe_decline()``: why its options keep the torch program, or None;
* ``_mpe_fill(io, dev)``: its task's parameters into the argument block;
* ``_mpe_scenario_outputs(io, B, dev)``: the scenario-level tensors its reward leaves bound, as
  ``{name: tensor}``, their pointers stored into the block, ``_mpe_bind(out)`` binding them and
  ``_mpe_bound()`` listing the tensors bound now;
* ``_torch_reward`` / ``_torch_observation``: the definition, which runs wherever the program does not.

The first agent's reward call runs ONE launch: every reward, the scenario tensors and every agent's
observation.  The later calls hand the precomputed tensors out while the inputs are unchanged
(``_fused.state_key``); otherwise the call recomputes.
"""
from __future__ import annotations

import ctypes
import weakref

import torch

from .. import _native as N
from . import _fused


def norm2(d: torch.Tensor) -> torch.Tensor:
    """|d| per row of a [B, 2] tensor with one rounding per operation: sqrt(dx * dx + dy * dy), the
    square root correctly rounded.

    On a device that is ``torch.linalg.vector_norm(d, dim=-1)`` bit for bit, in one kernel.  ATen's
    CPU kernels are not held to that: the norm accumulates the squares with a fused multiply-add
    where the hardware has one (one rounding fewer), and the vectorised fp32 square root of some
    instruction sets is an ulp off in under 1 % of its results.  So on ``cpu`` the operations are
    spelled out and the root is taken in fp64 and rounded once more (for a square root that is the
    correctly rounded fp32 result): the same bits on every backend, which is what the scenarios'
    programs, the library's host backend and their restatement are held to."""
    if d.device.type != "cpu":
        return torch.linalg.vector_norm(d, dim=-1)
    dx, dy = d[:, 0], d[:, 1]
    return (dx * dx + dy * dy).double().sqrt().float()


_LAUNCHES = weakref.WeakKeyDictionary()  # scenario -> launches made (MpeProgram.native_launches)


class NotFusable(Exception):
    """An operand the fused kernel does not take (dtype / layout / device): the torch program runs."""


class MpeProgram:
    def reward(self, agent):
        if _fused.enabled(self.world) and self._fused_plan() is not None:
            return self._fused_reward(agent)
        return self._torch_reward(agent)

    def observation(self, agent):
        if _fused.enabled(self.world) and self._fused_plan() is not None:
            return self._fused_observation(agent)
        return self._torch_observation(agent)

    # ---- the plan ---------------------------------------------------------------------------------------
    def _plan_reason(self):
        agents, marks = self.world.agents, self.world.landmarks
        if not 1 <= len(agents) <= N.VMAS_MPE_MAX_AGENTS:
            return f"{len(agents)} agents (VMAS_MPE_MAX_AGENTS = {N.VMAS_MPE_MAX_AGENTS})"
        if len(marks) > N.VMAS_MPE_MAX_LANDMARKS:
            return f"{len(marks)} landmarks (VMAS_MPE_MAX_LANDMARKS = {N.VMAS_MPE_MAX_LANDMARKS})"
        if not all(type(e.shape).__name__ == "Sphere" for e in agents + marks):
            return "an agent or a landmark is not a sphere"
        return self._mpe_decline()

    def _fused_plan(self):
        w = self.world
        sig = (tuple(id(e) for e in w.agents), tuple(id(e) for e in w.landmarks), w.batch_dim, str(w.device))
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
        if self._fused_plan() is None:
            return f"torch: {self._fwhy}"
        declined = getattr(self, "_fdeclined", None)  # (what the last launch attempt met)
        return "native" if declined is None else f"torch: {declined}"

    def _fused_inputs(self):
        ts = []
        for a in self.world.agents:
            ts += [a.state.pos, a.state.vel]
        return ts + [m.state.pos for m in self.world.landmarks]

    def _launch_args(self, dev):
        """(device index, stream) of a launch; a CPU world: the library's host backend (the ABI's
        device -1; reached only by direct calls of _run_fused)."""
        return (dev.index, _fused.stream(self.world)) if dev.type == "cuda" else (-1, None)

    # ---- the launch -------------------------------------------------------------------------------------
    @property
    def native_launches(self) -> int:
        """vmas_mpe_outputs calls this scenario made (a test's proof of which program ran).  Counted
        beside the scenario, not on it: graph mode would see a step that changes Python-side state."""
        return _LAUNCHES.get(self, 0)

    def _run_fused(self, what: int):
        w = self.world
        dev = self._fused_plan()["dev"]
        B, agents, marks = w.batch_dim, w.agents, w.landmarks
        n = len(agents)
        keep = []
        io = N.VmasMpeIO()
        io.batch, io.n_agents, io.n_landmarks, io.what, io.task = B, n, len(marks), what, self._mpe_task

        def operand(t):
            if not isinstance(t, torch.Tensor) or t.shape != (B, 2) or t.device != dev:
                raise NotFusable("an operand is not a [B, 2] tensor on the world's device")
            if t.dtype is not torch.float32:
                raise NotFusable("an operand is not float32")
            if t.requires_grad:
                raise NotFusable("an operand requires grad")
            return _fused.vec(t, keep)

        io.collide_mask = sum(1 << i for i, a in enumerate(agents) if a.collide)
        widths = []
        for i, a in enumerate(agents):
            io.pos[i] = operand(a.state.pos)
            if what & N.VMAS_SCN_OBS:
                io.vel[i] = operand(a.state.vel)
            terms = self._mpe_terms(a)
            if not 1 <= len(terms) <= N.VMAS_MPE_MAX_TERMS:
                raise NotFusable(f"an observation row of {len(terms)} terms")
            io.n_terms[i] = len(terms)
            for t, (kind, index) in enumerate(terms):
                io.terms[i][t].kind, io.terms[i][t].index = kind, index
            widths.append(2 * len(terms))
        for j, m in enumerate(marks):
            io.landmark_pos[j] = operand(m.state.pos)
        self._mpe_fill(io, dev)
        out = {}
        # (graph-mode capture: obs / rewards written straight into each replay's fresh tensors; the
        # rows' widths may differ per agent)
        io.out_delta, direct = _fused.direct_outputs(w, (
            (torch.float32, [(B, wd) for wd in widths], None) if what & N.VMAS_SCN_OBS else None,
            (torch.float32, (B,), n) if what & N.VMAS_SCN_REWARD else None,
            None))
        f32 = dict(device=dev, dtype=torch.float32)
        if what & N.VMAS_SCN_REWARD:
            out["rewards"] = direct[1] or [torch.empty(B, **f32) for _ in agents]
            out["scenario"] = self._mpe_scenario_outputs(io, B, dev)
        if what & N.VMAS_SCN_OBS:
            out["obs"] = direct[0] or [torch.empty(B, wd, **f32) for wd in widths]
        for i in range(n):
            if what & N.VMAS_SCN_REWARD:
                io.rewards[i] = out["rewards"][i].data_ptr()
            if what & N.VMAS_SCN_OBS:
                io.obs[i] = out["obs"][i].data_ptr()
        idx, stream = self._launch_args(dev)
        _fused.check(_fused.lib().vmas_mpe_outputs(idx, ctypes.byref(io), stream), "vmas_mpe_outputs")
        _LAUNCHES[self] = _LAUNCHES.get(self, 0) + 1
        self._fdeclined = None
        if what & N.VMAS_SCN_REWARD:
            self._mpe_bind(out["scenario"])  # the first agent's reward call re-binds them
        return out

    def _fused_reward(self, agent):
        agents = self.world.agents
        i = agents.index(agent)
        if i == 0:
            try:
                out = self._run_fused(N.VMAS_SCN_REWARD | N.VMAS_SCN_OBS)
            except NotFusable as e:
                self._fc, self._fdeclined = None, str(e)
                return self._torch_reward(agent)
            self._fc = {
                "key": _fused.state_key(self._fused_inputs()),
                "bound": _fused.state_key(self._mpe_bound()),
                "rew": dict(enumerate(out["rewards"])),
                "obs": dict(enumerate(out["obs"])),
            }
        c = getattr(self, "_fc", None)
        if c is not None and i in c["rew"] and c["bound"] == _fused.state_key(self._mpe_bound()):
            return c["rew"].pop(i)
        # (a scenario tensor changed under the cache, or the first agent's call ran the torch program:
        # the reference's expression on the current tensors)
        return self._torch_reward(agent)

    def _fused_observation(self, agent):
        i = self.world.agents.index(agent)
        c = getattr(self, "_fc", None)
        if c is None or i not in c["obs"] or c["key"] != _fused.state_key(self._fused_inputs()):
            try:
                out = self._run_fused(N.VMAS_SCN_OBS)
            except NotFusable as e:
                self._fdeclined = str(e)
                return self._torch_observation(agent)
            c = self._fc = {"key": _fused.state_key(self._fused_inputs()), "bound": None, "rew": {},
                            "obs": dict(enumerate(out["obs"]))}
        return c["obs"].pop(i)
