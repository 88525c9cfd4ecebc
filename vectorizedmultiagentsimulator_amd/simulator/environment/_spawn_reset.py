"""The native path of ``Environment.reset_where(mask)`` for scenarios whose reset places entities by
rejection sampling (``ScenarioUtils.spawn_entities_randomly`` / ``find_random_pos_for_entity``):
navigation, transport, discovery, flocking.

One ``vmas_spawn_reset`` call (csrc/vmas_reset.hip): a ``k_reset_place`` launch per placed entity --
the reference's placement loop for EVERY env, since an env outside the mask can hold the batch's
largest try count and with it the next entity's generator offset -- then one ``k_reset_commit`` launch
that writes the rows of the mask in place, and one host wait for the try counts.  The full reset
makes a stream synchronisation per placed entity instead (simulator/utils.py
``_find_random_pos_native``), and the generic ``reset_where`` (``_masked.py``) adds a snapshot and a
merge around it.

A scenario describes its reset as

  * ``stages``: ``[(keys, min_dist), ...]`` in placement order -- one entry per spawn call, ``keys``
    one hashable per placed position (an entity, or any token for a position that no entity or
    several entities take); a key's scratch slot is its place in that order;
  * ``writes``: ``[(entity, key), ...]`` -- every entity of the world with the key whose position it
    gets (vel / rot / ang_vel are zeroed as ``World.reset`` zeroes them); ``Fixed(j)`` in place of a
    key: the entity is set to ``fixed[j]``, a given position, and not placed (flocking's target);
  * ``derived``: the values ``reset_world_at`` computes from the new positions: ``("norm", key_a,
    key_b, factor, out)``, ``("box_sphere", box, sphere, key_box, key_sphere, out)``, ``("clear", out)``
    (bool rows), ``("zero", out)`` (a float row), ``("mean_sq_sep", i, factor, out)``: flocking's
    separation term of entry ``i`` of ``sep``'s list;
  * ``sep``: ``(positions, desired_distance)`` -- the key or ``Fixed(j)`` of every agent of
    ``world.agents``, in order (one list per call).

``spawn_reset_where`` returns ``NotImplemented`` wherever the launch cannot stand in for the full
reset (the caller then leaves the call to the generic path), as balance's ``reset_world_where`` does.
"""
from __future__ import annotations

import ctypes
import weakref

import torch

from ... import _native as N
from .. import _fused


# per scenario: (batch, placed, device), the candidates' scratch [placed][2][B], the call's words
_BUFFERS = weakref.WeakKeyDictionary()


def _mut(t, dev):
    """A [B, 2] / [B, 1] / [B] fp32 device tensor as a VmasMutVec, or None if it is not one."""
    if (t is None or t.dtype is not torch.float32 or t.device != dev or t.dim() not in (1, 2)
            or (t.dim() == 2 and t.shape[1] not in (1, 2)) or (t.shape[0] > 1 and t.stride(0) == 0)):
        return None
    v = N.VmasMutVec()
    v.p, v.s0, v.s1 = t.data_ptr(), t.stride(0), (t.stride(1) if t.dim() > 1 else 0)
    return v


def _bool_rows(t, dev, shape) -> bool:
    return (isinstance(t, torch.Tensor) and t.dtype is torch.bool and t.device == dev and tuple(t.shape) == shape
            and t.is_contiguous())


class Fixed:
    """In place of a key: the position ``fixed[j]``."""

    def __init__(self, j: int):
        self.j = int(j)


def spawn_reset_where(scenario, mask, stages, writes, x_bounds, y_bounds, derived=(), fixed=(), max_tries=0, sep=None):
    """The rows of ``mask`` as the scenario's full reset leaves them, in place (see the module's
    head); ``None`` when done, ``NotImplemented`` when the generic path has to run.  Counts
    ``scenario.native_resets`` (launched and committed) and ``scenario.native_reset_fallbacks`` (an
    env found no place within ``max_tries``: nothing written, the generators untouched)."""
    from . import _uniform

    w = scenario.world
    env = getattr(scenario, "_where_env", None)
    if not _fused.enabled(w) or getattr(w, "_grad_enabled", False):
        return NotImplemented
    keys = [k for ks, _ in stages for k in ks]
    slot_of = {k: i for i, k in enumerate(keys)}
    if (not keys or len(keys) > N.VMAS_RESET_MAX_PLACE or len(slot_of) != len(keys)
            or len(writes) > N.VMAS_RESET_MAX_WRITE or len(w.agents) > N.VMAS_RESET_MAX_AGENTS
            or len(derived) > N.VMAS_RESET_MAX_DERIVED or len(fixed) > N.VMAS_RESET_MAX_FIXED):
        return NotImplemented
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

    def code(key):
        """The ABI's position code: a placed slot, or -1 - j for ``fixed[j]``."""
        if isinstance(key, Fixed):
            assert 0 <= key.j < len(fixed), key.j
            return -1 - key.j
        return slot_of[key]

    # (graph mode) a field still bound to the persistent action buffer, whose rows the next step's
    # actions own, leaves the call to the generic path
    p_buf = getattr(getattr(env, "_u_persist", None), "buffer", None)
    p_lo = p_buf.data_ptr() if p_buf is not None else 0
    p_hi = p_lo + 4 * p_buf.numel() if p_buf is not None else 0
    io = N.VmasSpawnResetIO()
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

    if {id(e) for e, _ in writes} != {id(e) for e in w.entities}:
        return NotImplemented  # (World.reset zeroes every entity: each needs its position's key)
    pos_slot = {}  # id(pos tensor) -> the slot it takes
    for i, (e, key) in enumerate(writes):
        st, dst = e.state, io.write[i]
        io.write_slot[i] = code(key)
        # (the full reset binds ONE tensor as the pos of every entity set to the same position --
        # navigation's shared goals: it takes its slot once; another slot would need two rows)
        if pos_slot.setdefault(id(st.pos), code(key)) != code(key):
            return NotImplemented
        first = not any(t is st.pos for t in written)
        dst.pos = mut(st.pos) if first else N.VmasMutVec()
        dst.vel, dst.rot, dst.ang_vel = mut(st.vel), mut(st.rot), mut(st.ang_vel)
    for i, a in enumerate(w.agents):
        if a.state.c is not None:
            return NotImplemented  # (communication state: zeroed by World.reset, not by the launch)
        io.force[i], io.torque[i] = mut(a.state.__dict__.get("_force")), mut(a.state.__dict__.get("_torque"))
    keep = []
    if sep is not None:
        positions, desired = sep
        order = _fused.reduce_order(dev, len(positions) - 1) if 2 <= len(positions) <= N.VMAS_RESET_MAX_SEP else None
        if order is None:
            return NotImplemented  # (no summation order reproduces torch's .mean(-1), or too long a list)
        io.n_sep, io.sep_sum_mode, io.sep_desired = len(positions), order, float(desired)
        for i, key in enumerate(positions):
            io.sep_slot[i] = code(key)
    for i, d in enumerate(derived):
        r = io.derived[i]
        if d[0] == "norm":
            _, ka, kb, factor, out = d
            if not isinstance(out, torch.Tensor) or out.shape != (B,):
                return NotImplemented
            r.kind, r.a, r.b, r.factor, r.out = N.VMAS_RESET_D_NORM, slot_of[ka], slot_of[kb], float(factor), mut(out)
        elif d[0] == "box_sphere":
            _, box, sphere, ka, kb, out = d
            if (type(box.shape).__name__ != "Box" or type(sphere.shape).__name__ != "Sphere"
                    or not _bool_rows(out, dev, (B,))):
                return NotImplemented
            rb, rs = _fused.ref(w, box, keep, 0), _fused.ref(w, sphere, keep, 0)
            r.kind, r.a, r.b = N.VMAS_RESET_D_BOX_SPHERE, slot_of[ka], slot_of[kb]
            r.length, r.width, r.radius_lmd = rb.length, rb.width, rs.radius_lmd
            r.out8 = out.data_ptr()
            written.append(out)
        elif d[0] == "mean_sq_sep":
            _, index, factor, out = d
            if sep is None or not isinstance(out, torch.Tensor) or out.shape != (B,):
                return NotImplemented
            r.kind, r.a, r.factor, r.out = N.VMAS_RESET_D_MEAN_SQ_SEP, int(index), float(factor), mut(out)
        elif d[0] == "zero":
            out = d[1]
            if not isinstance(out, torch.Tensor) or out.shape != (B,):
                return NotImplemented
            r.kind, r.out = N.VMAS_RESET_D_ZERO32, mut(out)
        else:
            out = d[1]
            if not (isinstance(out, torch.Tensor) and out.dim() == 2 and _bool_rows(out, dev, (B, out.shape[1]))):
                return NotImplemented
            r.kind, r.n, r.out8 = N.VMAS_RESET_D_CLEAR8, out.shape[1], out.data_ptr()
            written.append(out)
    for i, t in enumerate(fixed):
        if t.dtype is not torch.float32 or t.device != dev or tuple(t.shape) != (B, 2):
            return NotImplemented
        io.fixed[i] = _fused.vec(t, keep)
    # (one tensor bound to two fields -- a user's set_pos of a shared tensor -- cannot take two rows)
    if not ok or len({t.data_ptr() for t in written}) != len(written):
        return NotImplemented
    i = 0
    for ks, min_dist in stages:
        for _ in ks:
            io.min_dist[i] = float(min_dist)
            i += 1
    buf = _BUFFERS.get(scenario)
    if buf is None or buf[0] != (B, len(keys), dev):
        buf = _BUFFERS[scenario] = ((B, len(keys), dev),
                                    torch.empty(len(keys) * 2 * B, dtype=torch.float32, device=dev),
                                    torch.zeros(N.VMAS_RESET_WORDS, dtype=torch.int32, device=dev))
    io.batch, io.mode, io.max_tries, io.n_place = B, mode, int(max_tries), len(keys)
    io.n_fixed, io.n_write, io.n_agents, io.n_derived = len(fixed), len(writes), len(w.agents), len(derived)
    io.x_lo, io.x_hi, io.y_lo, io.y_hi = float(x_bounds[0]), float(x_bounds[1]), float(y_bounds[0]), float(y_bounds[1])
    io.mask, io.scratch, io.words = mask.data_ptr(), buf[1].data_ptr(), buf[2].data_ptr()
    io.steps = steps.data_ptr() if steps is not None else None
    gen = torch.cuda.default_generators[dev.index]
    off = gen.get_offset()
    io.seed, io.offset = gen.initial_seed(), off
    inc, lost = ctypes.c_uint64(0), ctypes.c_int32(0)
    _fused.check(_fused.lib().vmas_spawn_reset(dev.index, ctypes.byref(io), ctypes.byref(inc), ctypes.byref(lost),
                                               _fused.stream(w)), "vmas_spawn_reset")
    if lost.value:
        # an env found no place within max_tries: the commit wrote nothing and the generator stands
        # where it stood, so the generic path redoes the call with the reference's loop
        scenario.native_reset_fallbacks += 1
        return NotImplemented
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
