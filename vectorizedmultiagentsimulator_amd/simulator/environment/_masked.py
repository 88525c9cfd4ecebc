"""The generic path of ``Environment.reset_where(mask)``: rows of a full reset.

``reset_where`` leaves, in every env of the mask, the row a full ``reset()`` made at the same
generator states would leave, and in every other env the row it held before -- for every batched
tensor of the simulation state.  A scenario without a ``reset_world_where`` of its own gets that
from its ordinary full reset:

  1. walk the tracked objects (graph mode's ``_tracked_objects``: every entity's dynamics and
     controller included) and record each attribute that is a tensor with leading dimension ``batch_dim``,
     with its version counter and a copy of its values (the full reset may write it in place);
  2. run the full reset (``env_reset_world_at(None)``, ``steps = zeros``);
  3. merge: a tensor the reset re-bound still has its old object as the snapshot, one it wrote in
     place (same object, another version) has the copy; the rows OUTSIDE the mask are copied old ->
     new by one ``vmas_masked_rows`` launch (the host loop on ``cpu``), and the attribute keeps the
     reset's tensor.  A tensor the reset did not touch is left alone.

Python-side state of the tracked objects (what graph mode's ``_plain_attrs`` / ``_fingerprint``
report: numbers, strings, for a scenario outside the package also the contents of containers)
cannot be merged per row: if the full reset changed any, ``RuntimeError`` names the attribute.  The
generators advance exactly as ``reset()`` advances them, whatever the mask.
"""
from __future__ import annotations

from typing import Any, List

import torch
from torch import Tensor

from ... import _native as N


def tracked_objects(scenario, env=None) -> List[Any]:
    from ._graph import _tracked_objects

    if env is not None:
        objs = _tracked_objects(env)
    else:  # (a scenario driven without an Environment: the same walk from the scenario down)
        class _Shim:
            pass

        shim = _Shim()
        shim.world, shim.scenario = scenario.world, scenario
        objs = _tracked_objects(shim)[1:]
    return objs


def as_mask(mask, batch_dim: int, device) -> Tensor:
    """``mask`` as a contiguous bool tensor [batch_dim] on ``device``: a bool tensor of that shape,
    an integer index tensor (scattered on the device, no host read) or a sequence of ints (checked
    on the host as ``_check_batch_index`` checks one index)."""
    if isinstance(mask, Tensor):
        if mask.dtype is torch.bool:
            assert mask.shape == (batch_dim,), f"Mask must have shape ({batch_dim},), got {tuple(mask.shape)}"
            return mask.to(device).contiguous()
        assert not mask.dtype.is_floating_point and not mask.dtype.is_complex and mask.dim() <= 1, (
            f"Index must be a bool mask [{batch_dim}] or a 1-d integer tensor, got {mask.dtype} {tuple(mask.shape)}"
        )
        idx = mask.to(device=device, dtype=torch.long).reshape(-1)
        if idx.device.type == "cpu":
            assert idx.numel() == 0 or (0 <= int(idx.min()) and int(idx.max()) < batch_dim), (
                f"Index must be between 0 and {batch_dim}, got {idx.tolist()}"
            )
            out = torch.zeros(batch_dim, dtype=torch.bool)
            out[idx] = True
            return out
        # (a device index: counted into the mask with no host read; one outside the batch counts nowhere)
        valid = (idx >= 0) & (idx < batch_dim)
        hits = torch.zeros(batch_dim, dtype=torch.int32, device=device)
        hits.index_add_(0, idx.clamp(0, batch_dim - 1), valid.to(torch.int32))
        return hits > 0
    idx = [mask] if isinstance(mask, int) else list(mask)
    for i in idx:
        assert isinstance(i, int) and not isinstance(i, bool), f"Index must be an int, got {i!r}"
        assert 0 <= i < batch_dim, f"Index must be between 0 and {batch_dim}, got {i}"
    out = torch.zeros(batch_dim, dtype=torch.bool)
    if idx:
        out[idx] = True
    return out.to(device)


def _batched(v, batch_dim: int) -> bool:
    return isinstance(v, Tensor) and v.ndim >= 1 and v.size(0) == batch_dim


def _rows_ok(t: Tensor) -> bool:
    """Each row t[b] is one contiguous run of bytes and the rows do not overlap."""
    if t.numel() == 0 or t.is_contiguous():
        return True
    return t[0].is_contiguous() and (t.shape[0] == 1 or t.stride(0) >= t[0].numel())


def _row_view(t: Tensor) -> Tensor:
    """``t`` itself when the launch can address its rows, else a contiguous copy."""
    return t if _rows_ok(t) else t.contiguous()


class _Snapshot:
    """The values of tensors before the full reset, for those it turns out to have written in
    place.  On a ROCm device the contiguous ones go into ONE buffer with one vmas_copy_spans launch
    (a clone each was most of the call's host time at C2: ~50 launches); anything else is cloned."""

    def __init__(self, tensors, device):
        self.clones, self.slots, self.buf = {}, {}, None
        device = torch.device(device)
        spans, off = [], 0
        for i, t in enumerate(tensors):
            nb = t.numel() * t.element_size()
            if device.type == "cuda" and nb and t.is_contiguous() and t.device.type == "cuda":
                self.slots[i] = (off, nb)
                spans.append((t.data_ptr(), off, nb))
                off += (nb + 15) & ~15
            else:
                self.clones[i] = t.clone()
        if spans:
            self.buf = torch.empty(off, dtype=torch.uint8, device=tensors[0].device if device.index is None else device)
            base = self.buf.data_ptr()
            idx, stream = N.launch_args(self.buf.device)
            N.copy_raw(idx, [(src, base + o, nb) for src, o, nb in spans], stream)

    def get(self, i: int, like: Tensor) -> Tensor:
        c = self.clones.get(i)
        if c is not None:
            return c
        off, nb = self.slots[i]
        return self.buf[off:off + nb].view(like.dtype).view(like.shape)


def generic_reset_where(scenario, mask: Tensor, env=None) -> None:
    from ._graph import _package_scenario_class, _plain_attrs

    world = scenario.world
    B = world.batch_dim
    objs = tracked_objects(scenario, env)
    shadow = getattr(env, "_ushadow", None)
    before = []
    with torch.no_grad():
        for o in objs:
            for k, v in o.__dict__.items():
                if isinstance(v, Tensor) and _batched(v, B):
                    # (graph mode, between a random-action draw and its step: the persistent action
                    # buffer already holds the next actions; the values to keep are the snapshot's)
                    old = shadow.view(v) if shadow is not None and shadow.active else v
                    before.append((o, k, v, v._version, old))
        snap = _Snapshot([b[4] for b in before], world.device)
    strict = not _package_scenario_class(scenario)
    plain0 = _plain_attrs(objs, strict)

    scenario.env_reset_world_at(None)
    if env is not None:
        env.steps = torch.zeros(env.num_envs, device=env.device)

    plain1 = _plain_attrs(objs, strict)
    changed = sorted((k for k in set(plain0) | set(plain1) if plain0.get(k) != plain1.get(k)), key=lambda k: k[1])
    if changed:
        names = {id(o): type(o).__name__ for o in objs}
        raise RuntimeError(
            "reset_where: the full reset changed Python-side state that cannot be merged per env: "
            + ", ".join(f"{names.get(i, '?')}.{k}" for i, k in changed[:4])
            + ".  The world is now fully reset (every env, as reset()).  Give the scenario a "
            "reset_world_where(mask) of its own."
        )

    spans, written, keep = [], [], []
    claimed = {}  # id(new tensor) -> id of the old tensor merged into it (two attributes may share one)
    with torch.no_grad():
        for i, (o, k, v, ver, shown) in enumerate(before):
            new = o.__dict__.get(k)
            if not _batched(new, B):
                continue  # (the reset dropped or reshaped the attribute: nothing to merge row by row)
            if new is v and new._version == ver:
                continue  # untouched
            # re-bound and never written: the old object is its own snapshot; written in place
            # (before a re-bind too), or shown through the action shadow: the clone
            old = v if (new is not v and v._version == ver and shown is v) else snap.get(i, shown)
            if old.shape != new.shape or old.dtype != new.dtype or old.device != new.device:
                continue  # (another layout: the attribute is the reset's alone)
            prev = claimed.get(id(new))
            if prev == id(shown):
                continue  # (the same pair of tensors through a second attribute)
            if prev is not None or not _rows_ok(new):
                # one tensor bound to two attributes with different histories, or an expanded /
                # transposed one: this attribute gets a tensor of its own
                new = new.clone() if _rows_ok(new) else new.contiguous()
                o.__dict__[k] = new
            claimed[id(new)] = id(shown)
            es = new.element_size()
            nb = new.numel() * es
            if nb == 0:
                continue
            # (the common case first: both contiguous, one row after the other)
            row = nb // B
            src = old if old.is_contiguous() else _row_view(old)
            spans.append((new.data_ptr(), src.data_ptr(), row,
                          row if (B == 1 or new.is_contiguous()) else new.stride(0) * es,
                          row if (B == 1 or src.is_contiguous()) else src.stride(0) * es))
            written.append(new)
            keep.append(src)
        idx, stream = N.launch_args(torch.device(world.device))
        N.masked_rows(idx, spans, mask.data_ptr(), B, False, stream)
        if written:  # (the launch wrote them through raw pointers)
            torch.autograd.graph.increment_version(written)
    del keep, snap
