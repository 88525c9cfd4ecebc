"""_set_action of every agent in one native call (csrc/vmas_actions.hip), for continuous and for
discrete actions without communication and without autograd: one launch and no stream
synchronisation in place of the reference's per-agent torch ops and host waits
(environment.py:615-709).  ``apply`` is the one body of both kinds; a kind (``Continuous`` /
``Discrete``) supplies only what differs: the action dtypes it takes, the plan's key and refs, the
per-step fill of the refs' action fields, the library's entry points and what a set flag means."""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from ... import _native as N
from . import _discrete

COMMUNICATION = "communication actions (dim_c > 0, non-silent agents) take the per-agent action path"


class ActionPlan:
    """What the action launches of one env configuration share (Environment._apply_cache), the
    speculative launch and the blocking apply alike.  A plan with a ``refusal`` holds the key and
    the reason alone: that configuration keeps the per-agent path."""

    __slots__ = ("key", "refusal", "refs", "refs_addr", "fields", "flags", "flags_addr", "words", "tensors", "sizes",
                 "total", "idx", "mode")

    def __init__(self, key, refusal: Optional[str] = None):
        self.key, self.refusal = key, refusal
        self.mode = None  # (discrete: the probed division mode, an argument of its entry points)


# Graph mode's action buffer (Environment._u_persist): every step of ``plan`` writes ``buffer`` and
# binds the agents' u to the same ``views`` of it (None until the first apply), which the captured step reads
PersistentActions = namedtuple("PersistentActions", "plan buffer views")

NOT_FLOAT32 = "u_range / u_multiplier are not float32"


def _float32(ag) -> bool:
    return ag.action.u_range_tensor.dtype is torch.float32 and ag.action.u_multiplier_tensor.dtype is torch.float32


def _build(env, key, ref_dtype, step_fields) -> ActionPlan:
    """The plan of ``key``: one ref per agent with what both kinds share set (range / multiplier
    tensors, output offset and width); ``step_fields`` name the columns the per-step fill writes."""
    agents, B = env.agents, env.num_envs
    if not all(_float32(ag) for ag in agents):
        return ActionPlan(key, NOT_FLOAT32)
    tensors = [(ag.action.u_range_tensor, ag.action.u_multiplier_tensor) for ag in agents]
    plan = ActionPlan(key)
    plan.refs = refs = np.zeros(len(agents), dtype=ref_dtype)
    plan.tensors, plan.sizes = tensors, [ag.action_size for ag in agents]
    plan.total = sum(plan.sizes)
    refs["u_range"], refs["u_mult"] = [r.data_ptr() for r, _ in tensors], [m.data_ptr() for _, m in tensors]
    refs["out_offset"], refs["n_phys"] = np.cumsum([0] + plan.sizes[:-1]) * B, plan.sizes
    plan.fields = tuple(refs[f] for f in step_fields)
    plan.flags = np.zeros(max(16, (2 * len(agents) + 7) // 8 * 8), dtype=np.uint8)  # (whole uint64 words)
    plan.words = plan.flags.view(np.uint64)
    # the arrays' addresses once (ndarray.ctypes builds a helper object per access: ~1.6 us)
    plan.refs_addr, plan.flags_addr = refs.ctypes.data, plan.flags.ctypes.data
    plan.idx = N.launch_args(env.device)[0]
    return plan


def _bind(env, ag, u) -> None:
    ag.action.u = u
    if ag.action.u_noise > 0:
        noise = torch.randn(*ag.action.u.shape, device=env.device, dtype=torch.float32) * ag.u_noise
        ag.action.u += noise


class Continuous:
    """fp32 actions: the NaN / range checks, the clamp and u = physical * u_multiplier."""

    DTYPES = (torch.float32,)  # other action dtypes take the per-agent path
    RUN, LAUNCH = "vmas_apply_actions", "vmas_apply_actions_launch"
    field = None  # no per-step check: apply() writes the action's column count itself (no call per agent)

    @staticmethod
    def key(env):
        return (tuple(env.agents), bool(env.clamp_action), env.num_envs, env.world.dim_c, str(env.device))

    @staticmethod
    def plan(env, key) -> ActionPlan:
        plan = _build(env, key, N.ACTION_APPLY_REF_DTYPE, ("u", "s0", "s1", "n_cols"))
        if plan.refusal is None:
            plan.refs["clamp"] = int(bool(env.clamp_action))
        return plan

    @staticmethod
    def finish(env, plan, actions, us, persistent) -> bool:
        """Agents in order, exactly as the reference loop: agent i raises before its u is
        assigned; the agents before it keep their new u and noise."""
        flags = plan.flags
        for i, ag in enumerate(env.agents):
            if flags[2 * i]:
                print()  # the reference prints an empty line before this assert (environment.py:621-622)
                assert not flags[2 * i]
            assert not flags[2 * i + 1], f"Physical actions of agent {ag.name} are out of its range {ag.u_range}"
            _bind(env, ag, us[i])
        return True


class Discrete:
    """Flat-index or multi-discrete actions (int64, int32 or float32): the flat decode, the range
    checks, the odd-n swap and u = ((a / (n - 1)) * 2 u_max - u_max) * u_multiplier of
    environment.py:667-709."""

    DTYPES = _discrete.DTYPE_CODES
    RUN, LAUNCH = "vmas_apply_discrete_actions", "vmas_apply_discrete_actions_launch"

    @staticmethod
    def key(env):
        # (nvec is a plain list the caller may re-assign or edit: compared by value every call)
        nvecs = tuple(tuple(ag.discrete_action_nvec) for ag in env.agents)
        return ("discrete", tuple(env.agents), bool(env.multidiscrete_actions), nvecs, env.num_envs, env.world.dim_c,
                str(env.device))

    @staticmethod
    def plan(env, key) -> ActionPlan:
        multi, nvecs, K = key[2], key[3], N.DISCRETE_MAX_COMPONENTS
        for ag, nvec in zip(env.agents, nvecs):
            if not 1 <= len(nvec) <= K or ag.action_size > K:
                return ActionPlan(key, f"more than {K} discrete action components take the per-agent action path")
            if len(nvec) > ag.action_size or (multi and len(nvec) != ag.action_size):
                return ActionPlan(key, "discrete_action_nvec does not match action_size")
            if (not all(isinstance(n, (int, np.integer)) and 2 <= n <= 1 << 24 for n in nvec)
                    or (not multi and math.prod(nvec) > 1 << 24)):
                return ActionPlan(key, "discrete_action_nvec beyond what fp32 holds exactly")
            if not _float32(ag):  # (per agent, between the nvec checks: the first agent at fault gives the reason)
                return ActionPlan(key, NOT_FLOAT32)
        plan =_build(env, key, N.DISCRETE_ACTION_REF_DTYPE, ("a", "s0", "s1", "dtype"))
        mode = _discrete.mode(env.device)
        if mode is None:
            return ActionPlan(key, "no division mode of the discrete action kernel reproduces this torch build")
        plan.mode = mode
        plan.refs["flat"], plan.refs["n_comp"] = int(not multi), [len(v) for v in nvecs]
        for i, v in enumerate(nvecs):
            plan.refs["nvec"][i, : len(v)] = v
        return plan

    @staticmethod
    def field(plan, env, i, a):  # the dtype code; None: the per-agent path raises the reference's shape assertion
        n = plan.sizes[i] if env.multidiscrete_actions else 1
        ok = a.dim() == 2 and a.shape[0] == env.num_envs and a.shape[1] == n
        return _discrete.DTYPE_CODES[a.dtype] if ok else None

    @staticmethod
    def finish(env, plan, actions, us, persistent) -> bool:
        """A set flag -- a NaN, a value out of range, a float32 flat index that is not a whole
        number -- hands the step to the reference's own loop: it raises at the failing agent (the
        agents before it keep their new u, its own u is what the reference leaves) or, for values
        the reference accepts, computes u with the reference's float arithmetic."""
        agents = env.agents
        if plan.flags[: 2 * len(agents)].any():
            for i, ag in enumerate(agents):
                env._set_action(actions[i], ag)
            if persistent:  # (the captured step reads the persistent views)
                for i, ag in enumerate(agents):
                    us[i].copy_(ag.action.u)
                    ag.action.u = us[i]
            return True
        for i, ag in enumerate(agents):
            _bind(env, ag, us[i])
        return True


def apply(env, kind, actions, persistent: bool = False, speculative: bool = False):
    """Every agent's u from ``actions`` in one native call.  Returns False when the case does not
    apply (the per-agent path runs), else True.  persistent (graph mode): every step writes the
    same buffer and binds the same u views.  speculative (graph mode, no action noise, at most 8
    agents): the kernel is only launched and the agents' u are bound to the persistent buffer;
    returns the launch's sequence number (or False) and the caller checks the flags later
    (Environment._speculative_flags_ok)."""
    agents = env.agents
    n = len(agents)
    # the persistent buffer is rewritten: a draw's applied values are stale, and so is a draw
    # made ahead into it (_take_spec would hand out actions whose applied values are gone)
    env._drawn = env._spec = None
    env._ushadow.disarm()
    if n == 0:
        return False
    dtypes = kind.DTYPES
    for a in actions:
        if a.dtype not in dtypes or (env.grad_enabled and a.requires_grad):
            return False
    key = kind.key(env)
    plan = env._apply_cache
    if plan is None or plan.key != key:
        comm = env.world.dim_c > 0 and any(not ag.silent for ag in agents)
        plan = env._apply_cache = ActionPlan(key, COMMUNICATION) if comm else kind.plan(env, key)
    if plan.refusal is not None:
        return False
    tensors = plan.tensors
    for i, ag in enumerate(agents):  # range / multiplier tensors are cached by the Action
        if ag.action._u_range_tensor is not tensors[i][0] or ag.action._u_multiplier_tensor is not tensors[i][1]:
            env._apply_cache = None
            return apply(env, kind, actions, persistent, speculative)
    idx = plan.idx
    if speculative and (idx < 0 or n > 8 or any(ag.action.u_noise > 0 for ag in agents)):
        return False
    dev, B, keep = env.device, env.num_envs, []
    (f_ptr, f_s0, f_s1, f_kind), field = plan.fields, kind.field
    for i, a in enumerate(actions):
        if a.device != dev:
            a = a.to(dev)
        # the ref's fourth per-step field: the column count (continuous), or the kind's own (discrete: the
        # dtype code, None where the shape is not the expected one)
        x = a.shape[1] if field is None else field(plan, env, i, a)
        if x is None:
            return False
        keep.append(a)
        s = a.stride()
        f_ptr[i], f_s0[i], f_s1[i], f_kind[i] = a.data_ptr(), s[0], s[1], x
    pc = None
    if persistent:  # graph mode: every step writes the same buffer / the same u views
        pc = env._u_persist
        if pc is None or pc.plan is not plan:
            g = env._graph
            if g is not None and g.graph is not None:
                g.drop("action parameters changed")  # the captured step reads the previous buffer's views
                if speculative:
                    return False
            pc = env._u_persist = PersistentActions(
                plan, torch.empty(B * plan.total, device=dev, dtype=torch.float32), None)
        out = pc.buffer
    else:
        out = torch.empty(B * plan.total, device=dev, dtype=torch.float32)
    stream = N.stream_ptr(idx) if idx >= 0 else None
    lib, mode = N.load_library(), (() if plan.mode is None else (plan.mode,))
    if speculative:
        seq = ctypes.c_uint32(0)
        N.check_aux(getattr(lib, kind.LAUNCH)(idx, B, plan.refs_addr, n, out.data_ptr(), *mode, ctypes.byref(seq),
                                              stream), kind.LAUNCH)
        env._spec_keep = keep  # the kernel reads them: alive until the flags are in
    else:
        N.check_aux(getattr(lib, kind.RUN)(idx, B, plan.refs_addr, n, out.data_ptr(), *mode, plan.flags_addr, stream),
                    kind.RUN)
    del keep
    if pc is not None and pc.views is not None:
        us = pc.views
    else:
        sizes = plan.sizes
        if all(sz == sizes[0] for sz in sizes):
            us = out.view(n, B, sizes[0]).unbind(0)
        else:
            us = [out.narrow(0, int(o), B * sz).view(B, sz) for o, sz in zip(plan.refs["out_offset"], sizes)]
        if pc is not None:
            env._u_persist = pc._replace(views=us)
    if speculative:
        for i, ag in enumerate(agents):
            ag.action.u = us[i]
        return seq.value
    return kind.finish(env, plan, actions, us, persistent)
