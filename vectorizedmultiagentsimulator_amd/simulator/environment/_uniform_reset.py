"""``reset_world_where`` of a scenario whose full reset is a fixed list of ``uniform_`` calls.

wheel and dispersion reset with plain ``uniform_`` calls and reject nothing, so what the full reset
advances the generator by is known before the call, and the rows of a mask are ONE native launch
with no host wait (``vmas_uniform_reset``, csrc/vmas_reset.hip k_uniform_reset).  The scenario lists

* ``draws``: ``(entity, "pos" | "rot", lo, hi)`` per ``uniform_`` call of its ``reset_world_at(None)``,
  in call order -- a ``[B, 2]`` call for a position, a ``[B, 1]`` call for a rotation;
* ``fixed``: ``(entity, x, y)`` for an entity the reset puts at a given position;
* ``clear`` / ``set_``: bool rows ``[B]`` the reset leaves False / True.

Every entity of the world must be in one of the two lists (``World.reset`` zeroes all of them).
``uniform_reset_where`` returns ``NotImplemented`` wherever the launch cannot stand in for the full
reset -- a CPU world, a tensor that is not where the kernel expects it -- and the caller leaves the
call to the generic path (environment/_masked.py), as balance's ``reset_world_where`` does.
"""
from __future__ import annotations

import ctypes

import torch

from ... import _native as N
from .. import _fused
from ._spawn_reset import _bool_rows, _mut


def uniform_reset_where(scenario, mask, draws, fixed=(), clear=(), set_=()):
    from . import _uniform

    w = scenario.world
    env = getattr(scenario, "_where_env", None)
    if not _fused.enabled(w) or getattr(w, "_grad_enabled", False):
        return NotImplemented
    if (len(draws) > N.VMAS_URESET_MAX_DRAWS or len(fixed) > N.VMAS_URESET_MAX_FIXED
            or len(w.agents) > N.VMAS_URESET_MAX_AGENTS or len(clear) > N.VMAS_URESET_MAX_CLEAR
            or len(set_) > N.VMAS_URESET_MAX_SET):
        return NotImplemented
    listed = [d[0] for d in draws] + [f[0] for f in fixed]
    if sorted(id(e) for e in listed) != sorted(id(e) for e in w.entities):
        return NotImplemented  # (World.reset zeroes every entity: each is written exactly once)
    dev = torch.device(w.device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    B = w.batch_dim
    mode = _uniform.mode(dev, B)
    if mode is None or mask.dtype is not torch.bool or mask.device != dev or not mask.is_contiguous():
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
    io = N.VmasUniformResetIO()
    written = []
    ok = True

    def mut(t):
        nonlocal ok
        v = _mut(t, dev)
        if v is None or p_lo <= t.data_ptr() < p_hi:
            ok = False
            return N.VmasMutVec()
        written.append(t)
        return v

    def entity(dst, e):
        st = e.state
        dst.pos, dst.vel, dst.rot, dst.ang_vel = mut(st.pos), mut(st.vel), mut(st.rot), mut(st.ang_vel)

    for i, (e, target, lo, hi) in enumerate(draws):
        d = io.draws[i]
        entity(d.entity, e)
        d.target = N.VMAS_UDRAW_POS if target == "pos" else N.VMAS_UDRAW_ROT
        d.call, d.lo, d.hi = i, float(lo), float(hi)
    for i, (e, x, y) in enumerate(fixed):
        entity(io.fixed[i].entity, e)
        io.fixed[i].x, io.fixed[i].y = float(x), float(y)
    for i, a in enumerate(w.agents):
        if a.state.c is not None:
            return NotImplemented  # (communication state: zeroed by World.reset, not by the launch)
        io.force[i], io.torque[i] = mut(a.state.__dict__.get("_force")), mut(a.state.__dict__.get("_torque"))
    for rows, dst in ((clear, io.clear), (set_, io.set)):
        for i, t in enumerate(rows):
            if not _bool_rows(t, dev, (B,)):
                return NotImplemented
            dst[i] = t.data_ptr()
            written.append(t)
    # (one tensor bound to two fields -- a user's set_pos of a shared tensor -- cannot take two rows)
    if not ok or len({t.data_ptr() for t in written}) != len(written):
        return NotImplemented
    io.batch, io.mode, io.n_draws, io.n_fixed = B, mode, len(draws), len(fixed)
    io.n_agents, io.n_clear, io.n_set = len(w.agents), len(clear), len(set_)
    io.mask = mask.data_ptr()
    io.steps = steps.data_ptr() if steps is not None else None
    gen = torch.cuda.default_generators[dev.index]
    off = gen.get_offset()
    io.seed, io.offset = gen.initial_seed(), off
    inc = ctypes.c_uint64(0)
    _fused.check(_fused.lib().vmas_uniform_reset(dev.index, ctypes.byref(io), ctypes.byref(inc), _fused.stream(w)),
                 "vmas_uniform_reset")
    gen.set_offset(off + inc.value)
    for t in written:
        _fused.bump_version(t)
    if steps is not None:
        _fused.bump_version(steps)
        scenario._where_steps_done = True
    for e in w.entities:
        e.notify_observers()
    scenario.native_resets += 1
    return None
