"""rgb_array rendering on the native rasteriser (csrc/vmas_render.hip).

``render_frame`` is ``Environment.render``: it collects the geoms the reference's viewer would draw
(boundary, grid, ``extra_render``, every entity's ``render``, ``top_layer_render``), lowers them on
the host to the primitive table of ``vmas_render_frames`` (frame function: include/vmas_mi355x.h)
and rasterises one frame.  ``render_batch`` is ``Environment.render_batch``: ``vmas_render_scene``
builds the entity layer of many environments' tables on the device and ``vmas_render_frames``
rasterises them, with no Python per environment and no host synchronisation.
"""
from __future__ import annotations

import ctypes
import math
import weakref
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from .. import _native as N
from . import rendering
from .utils import Color

MARGIN = 2.0  # pixels around a primitive's outline in its bounding box (coverage ends at d = 0.5, a border at 1.5)

# ------------------------------------------------------------------------------------------------
# one device-to-host copy per frame
_SNAP: Optional["HostState"] = None


class HostState:
    """What Environment.render reads of ONE environment, fetched with one device-to-host copy:
    every entity's position, rotation, is_rendering flag and tensor colour, the action-line forces
    and the LIDARs' angles and last measurements."""

    def __init__(self, world, env_index: int):
        self.env_index = env_index
        self.index = {}
        parts: List[Tensor] = []
        off = 0

        def add(obj, name, t):
            nonlocal off
            t = t.detach().reshape(-1).to(torch.float32)
            self.index[(id(obj), name)] = (off, off + t.numel())
            off += t.numel()
            parts.append(t)

        for e in world.entities:
            add(e, "pos", e.state.pos[env_index])
            add(e, "rot", e.state.rot[env_index])
            add(e, "mask", e.is_rendering[env_index])
            c = e.color
            if isinstance(c, Tensor):
                add(e, "color", c[env_index] if c.dim() > 1 else c)
            if getattr(e, "_render_action", False) and e.state.force is not None:
                add(e, "force", e.state.force[env_index])
            for s in getattr(e, "_sensors", None) or ():
                if getattr(s, "_last_measurement", None) is not None and hasattr(s, "_angles"):
                    add(s, "angles", s._angles[env_index])
                    add(s, "dist", s._last_measurement[env_index])
        self.values = torch.cat(parts).cpu().tolist() if parts else []

    def get(self, obj, name):
        span = self.index.get((id(obj), name))
        return None if span is None else self.values[span[0]:span[1]]


def host_value(obj, name: str, env_index: int, read) -> list:
    """Floats of one environment's value: from the frame's snapshot when there is one for this
    environment, else read from the tensor (a copy of its own)."""
    s = _SNAP
    if s is not None and s.env_index == env_index:
        v = s.get(obj, name)
        if v is not None:
            return v
    v = read()
    if isinstance(v, Tensor):
        return v.detach().reshape(-1).to(torch.float32).cpu().tolist()
    return [float(x) for x in np.asarray(v, dtype=np.float64).reshape(-1)]


# ------------------------------------------------------------------------------------------------
# camera and boundary (reference environment.py:851-903, 941-997)
def camera_range(scenario):
    if scenario.viewer_zoom <= 0:
        raise ValueError("Scenario viewer zoom must be > 0")
    zoom = np.float32(scenario.viewer_zoom)
    aspect = scenario.viewer_size[0] / scenario.viewer_size[1]
    if aspect < 1:
        return zoom, np.float32(scenario.viewer_zoom / aspect)
    return np.float32(scenario.viewer_zoom * aspect), zoom


def camera_bounds(env, agent_pos: Sequence[Sequence[float]], focus_pos=None):
    """(left, right, bottom, top) in fp32, as vmas_render_scene computes them."""
    scn = env.scenario
    cam_x, cam_y = camera_range(scn)
    f32 = np.float32
    if focus_pos is not None:
        px, py = f32(focus_pos[0]), f32(focus_pos[1])
        return px - cam_x, px + cam_x, py - cam_y, py + cam_y
    ox, oy = f32(scn.render_origin[0]), f32(scn.render_origin[1])
    zoom = f32(scn.viewer_zoom)
    max_r = f32(max(a.shape.circumscribed_radius() for a in env.world.agents))
    mx = max(abs(f32(p[0]) - ox) for p in agent_pos)
    my = max(abs(f32(p[1]) - oy) for p in agent_pos)
    fx, fy = mx + f32(2) * max_r, my + f32(2) * max_r
    vs = max(max(fx / cam_x, zoom), max(fy / cam_y, zoom))
    cx, cy = cam_x * vs, cam_y * vs
    return -cx + ox, cx + ox, -cy + oy, cy + oy


def boundary_segments(world) -> list:
    xs, ys = world.x_semidim, world.y_semidim
    if xs is None and ys is None:
        return []
    big = 100
    x, y = (xs if xs is not None else big), (ys if ys is not None else big)
    if ys is not None:
        pts = [(-x, y), (x, y), (x, -y), (-x, -y)]
    else:
        pts = [(-x, y), (-x, -y), (x, y), (x, -y)]
    step = 1 if xs is not None and ys is not None else 2
    return [(pts[i], pts[(i + 1) % 4]) for i in range(0, 4, step)]


# ------------------------------------------------------------------------------------------------
# lowering geoms to the primitive table
def _matrix(t: rendering.Transform) -> np.ndarray:
    c, s = math.cos(t.rotation), math.sin(t.rotation)
    sx, sy = t.scale
    return np.array([[c * sx, -s * sy, t.translation[0]], [s * sx, c * sy, t.translation[1]], [0.0, 0.0, 1.0]])


class _Table:
    def __init__(self):
        self.rows = []
        self.verts = []

    def row(self, kind, rgba, p, bbox, flags=0, v0=0, nv=0):
        self.rows.append((kind, flags, tuple(rgba), tuple(p) + (0.0,) * (6 - len(p)), v0, nv, tuple(bbox)))

    def seg(self, a, b, w, rgba):
        m = 0.5 * max(float(w), 1.0) + MARGIN
        self.row(N.VMAS_PRIM_SEG, rgba, (a[0], a[1], b[0], b[1], float(w)),
                 (min(a[0], b[0]) - m, min(a[1], b[1]) - m, max(a[0], b[0]) + m, max(a[1], b[1]) + m))

    def poly(self, pts, rgba, border):
        v0 = len(self.verts)
        self.verts.extend(pts)
        xs, ys = [q[0] for q in pts], [q[1] for q in pts]
        self.row(N.VMAS_PRIM_POLY, rgba, (), (min(xs) - MARGIN, min(ys) - MARGIN, max(xs) + MARGIN, max(ys) + MARGIN),
                 flags=N.VMAS_PRIM_BORDER if border else 0, v0=v0, nv=len(pts))

    def emit(self, geom, parent: np.ndarray, inherited):
        if isinstance(geom, rendering.TextLine):
            return
        m = np.eye(3)
        color, width = None, None
        for a in geom.attrs:  # the attribute added last is outermost
            if isinstance(a, rendering.Transform):
                m = _matrix(a) @ m
            elif isinstance(a, rendering.Color) and color is None:
                color = a.vec4
            elif isinstance(a, rendering.LineWidth) and width is None:
                width = a.stroke
        m = parent @ m
        rgba = tuple(float(x) for x in (color if color is not None else inherited))
        if len(rgba) == 3:
            rgba += (1.0,)
        width = 1.0 if width is None else float(width)

        def at(q):
            return (m[0, 0] * q[0] + m[0, 1] * q[1] + m[0, 2], m[1, 0] * q[0] + m[1, 1] * q[1] + m[1, 2])

        s1, s2 = math.hypot(m[0, 0], m[1, 0]), math.hypot(m[0, 1], m[1, 1])
        similar = abs(s1 - s2) <= 1e-6 * max(s1, s2) and abs(m[0, 0] * m[0, 1] + m[1, 0] * m[1, 1]) <= 1e-6 * s1 * s2
        if isinstance(geom, rendering.Compound):
            for g in geom.gs:
                self.emit(g, m, rgba)
        elif isinstance(geom, rendering.Line):
            self.seg(at(geom.start), at(geom.end), width, rgba)
        elif isinstance(geom, rendering.PolyLine):
            pts = [at(q) for q in geom.v]
            for k in range(len(pts) - 1):
                self.seg(pts[k], pts[k + 1], width, rgba)
            if geom.close and len(pts) > 2:
                self.seg(pts[-1], pts[0], width, rgba)
        elif isinstance(geom, rendering.FilledPolygon):
            if len(geom.v) >= 3:
                self.poly([at(q) for q in geom.v], rgba, bool(geom.draw_border))
        elif isinstance(geom, rendering.Circle):
            if not similar:  # an ellipse after a non-uniform scale: its outline as a polygon / polyline
                pts = [at((geom.radius * math.cos(2 * math.pi * k / 64), geom.radius * math.sin(2 * math.pi * k / 64)))
                       for k in range(64)]
                if geom.filled:
                    self.poly(pts, rgba, bool(geom.draw_border))
                else:
                    for k in range(64):
                        self.seg(pts[k], pts[(k + 1) % 64], width, rgba)
                return
            c, r = at((0.0, 0.0)), geom.radius * s1
            if geom.filled:
                e = r + MARGIN
                self.row(N.VMAS_PRIM_DISC, rgba, (c[0], c[1], r), (c[0] - e, c[1] - e, c[0] + e, c[1] + e),
                         flags=N.VMAS_PRIM_BORDER if geom.draw_border else 0)
            else:
                e = r + 0.5 * max(width, 1.0) + MARGIN
                self.row(N.VMAS_PRIM_RING, rgba, (c[0], c[1], r, width), (c[0] - e, c[1] - e, c[0] + e, c[1] + e))
        elif isinstance(geom, rendering.Grid):
            n = int(math.ceil(geom.length / geom.spacing))
            half = geom.length / 2
            if similar and abs(m[0, 1]) <= 1e-9 * s1 and m[0, 0] > 0:
                o, e = at((0.0, 0.0)), half * s1 + MARGIN
                sp, hp = geom.spacing * s1, half * s1
                k0 = math.floor(hp / sp + 0.5)  # the line nearest the grid's origin
                self.row(N.VMAS_PRIM_GRID, rgba, (o[0], o[1], sp, hp, width, k0 * sp - hp),
                         (o[0] - e, o[1] - e, o[0] + e, o[1] + e), v0=-k0, nv=n - 1 - k0)
            else:  # a rotated grid: its lines one by one
                for k in range(n):
                    u = -half + k * geom.spacing
                    self.seg(at((u, -half)), at((u, half)), width, rgba)
                    self.seg(at((-half, u)), at((half, u)), width, rgba)
        else:
            raise TypeError(f"rgb_array rendering cannot draw a {type(geom).__name__}")


def lower(geoms, bounds, width: int, height: int):
    """The primitive table ([P] of N.RENDER_PRIM_DTYPE, pixel space) and vertex pool ([V, 2] fp32) of
    a list of geoms seen through bounds = (left, right, bottom, top)."""
    left, right, bottom, top = (float(b) for b in bounds)
    sx, sy = width / (right - left), height / (top - bottom)
    view = np.array([[sx, 0.0, -left * sx], [0.0, sy, -bottom * sy], [0.0, 0.0, 1.0]])
    t = _Table()
    for g in geoms:
        t.emit(g, view, (0.0, 0.0, 0.0, 1.0))
    prims = np.zeros(len(t.rows), dtype=N.RENDER_PRIM_DTYPE)
    for k, (kind, flags, rgba, p, v0, nv, bbox) in enumerate(t.rows):
        prims[k] = (kind, flags, rgba, p, v0, nv, bbox)
    verts = np.asarray(t.verts, dtype=np.float32).reshape(-1, 2)
    return prims, verts


# ------------------------------------------------------------------------------------------------
def rasterise(device: torch.device, prims: np.ndarray, verts: np.ndarray, n_frames: int, height: int, width: int):
    """vmas_render_frames over a host-built table [n_frames * P]: a NumPy [E, H, W, 3] uint8."""
    lib = N.load_library()
    prims = np.ascontiguousarray(prims)
    verts = np.ascontiguousarray(verts, dtype=np.float32)
    n_prims = prims.size // max(n_frames, 1)
    if device.type != "cuda":
        out = np.empty((n_frames, height, width, 3), dtype=np.uint8)
        N.check_aux(lib.vmas_render_frames(-1, n_frames, height, width, prims.ctypes.data if prims.size else None, n_prims,
                                           verts.ctypes.data if verts.size else None, verts.size // 2,
                                           out.ctypes.data, None), "vmas_render_frames")
        return out
    idx, stream = N.launch_args(device)
    d_prims = torch.from_numpy(prims.view(np.uint8).reshape(-1)).to(device) if prims.size else None
    d_verts = torch.from_numpy(verts.reshape(-1)).to(device) if verts.size else None
    out = torch.empty((n_frames, height, width, 3), dtype=torch.uint8, device=device)
    N.check_aux(lib.vmas_render_frames(idx, n_frames, height, width, d_prims.data_ptr() if d_prims is not None else None,
                                       n_prims, d_verts.data_ptr() if d_verts is not None else None, verts.size // 2,
                                       out.data_ptr(), stream), "vmas_render_frames")
    return out.cpu().numpy()


def collect_geoms(env, env_index: int) -> list:
    """The geoms of one frame in the reference's draw order (environment.py:905-939)."""
    scn = env.scenario
    geoms = []
    if scn.visualize_semidims:
        for a, b in boundary_segments(env.world):
            line = rendering.Line(a, b, width=0.7)
            line.set_color(*Color.GRAY.value)
            geoms.append(line)
    if scn.plot_grid:
        grid = rendering.Grid(spacing=scn.grid_spacing)
        grid.set_color(*Color.BLACK.value, alpha=0.3)
        geoms.append(grid)
    geoms += scn.extra_render(env_index)
    for entity in env.world.entities:
        geoms += entity.render(env_index=env_index)
    geoms += scn.top_layer_render(env_index)
    return geoms


def render_frame(env, mode, env_index, agent_index_focus, visualize_when_rgb, plot_position_function):
    global _SNAP
    env._check_batch_index(env_index)
    assert mode in env.metadata["render.modes"], (
        f"Invalid mode {mode} received, allowed modes: {env.metadata['render.modes']}"
    )
    if agent_index_focus is not None:
        assert 0 <= agent_index_focus < env.n_agents, (
            f"Agent focus in rendering should be a valid agent index between 0 and {env.n_agents},"
            f" got {agent_index_focus}"
        )
    if mode != "rgb_array" or visualize_when_rgb:
        raise NotImplementedError("only headless mode=\"rgb_array\" rendering is part of the MI355X engine "
                                  "(no window: mode=\"human\" and visualize_when_rgb are not)")
    if plot_position_function is not None:
        raise NotImplementedError("plot_position_function is not drawn by the rgb_array renderer of the MI355X engine")
    camera_range(env.scenario)  # (viewer_zoom <= 0 raises before anything is read)
    width, height = (int(v) for v in env.scenario.viewer_size)
    snap = HostState(env.world, env_index)
    if agent_index_focus is None:
        bounds = camera_bounds(env, [snap.get(a, "pos") for a in env.world.agents])
    else:
        bounds = camera_bounds(env, None, focus_pos=snap.get(env.agents[agent_index_focus], "pos"))
    _SNAP = snap
    try:
        geoms = collect_geoms(env, env_index)
    finally:
        _SNAP = None
    prims, verts = lower(geoms, bounds, width, height)
    return rasterise(env.device, prims, verts, 1, height, width)[0]


# ------------------------------------------------------------------------------------------------
# the batch path
def _f32(t: Tensor) -> Tensor:
    t = t.detach()
    if t.dtype is not torch.float32:
        t = t.to(torch.float32)
    if t.dim() > 1 and t.stride(-1) != 1:
        t = t.contiguous()
    return t


# per environment: the small constant device tensors the scene launch reads (colours, index lists)
_CONSTS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def _check_plain_render(world):
    from .core import Agent, Entity
    from .sensors import Lidar

    for e in world.entities:
        own = Agent.render if isinstance(e, Agent) else Entity.render
        if type(e).render is not own:
            raise NotImplementedError(
                f"render_batch draws shapes, LIDAR rays and action lines on the device; entity {e.name!r} "
                f"({type(e).__name__}) overrides render(): use render(mode=\"rgb_array\") for it")
        for s in getattr(e, "_sensors", None) or ():
            if type(s).render is not Lidar.render:
                raise NotImplementedError(
                    f"render_batch cannot draw sensor {type(s).__name__} of {e.name!r}: use render(mode=\"rgb_array\")")


def render_batch(env, env_indices=None, size=None, agent_index_focus=None, with_bounds: bool = False):
    """Environment.render_batch; with_bounds: also the cameras' [E, 4] (left, right, bottom, top)."""
    from .core import Agent, Box, Line, Sphere

    world, scn, dev = env.world, env.scenario, env.device
    _check_plain_render(world)
    if agent_index_focus is not None:
        assert 0 <= agent_index_focus < env.n_agents, (
            f"Agent focus in rendering should be a valid agent index between 0 and {env.n_agents},"
            f" got {agent_index_focus}"
        )
    camera_range(scn)
    width, height = (int(v) for v in (size if size is not None else scn.viewer_size))
    if width <= 0 or height <= 0:
        raise ValueError(f"render_batch: bad frame size {(width, height)}")
    B = env.num_envs
    keep = []  # tensors the launches read
    cache = _CONSTS.setdefault(env, {})

    def const(values) -> Tensor:
        key = (tuple(float(v) for v in values), str(dev))
        t = cache.get(key)
        if t is None:
            t = cache[key] = torch.tensor(key[0], dtype=torch.float32, device=dev)
        return t

    if env_indices is None:
        n_frames, idx_ptr = B, None
    else:
        if isinstance(env_indices, Tensor):
            idx = env_indices.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        else:
            idx_list = [int(i) for i in env_indices]
            for i in idx_list:
                env._check_batch_index(i)
            key = ("idx", tuple(idx_list), str(dev))
            idx = cache.get(key)
            if idx is None:
                idx = cache[key] = torch.tensor(idx_list, dtype=torch.int64, device=dev)
        keep.append(idx)
        n_frames, idx_ptr = idx.numel(), idx.data_ptr()

    segs = boundary_segments(world) if scn.visualize_semidims else []
    n_fixed = len(segs) + (1 if scn.plot_grid else 0)
    ents, lidars = [], []
    slot, n_boxes, focus = n_fixed, 0, -1
    for k, e in enumerate(world.entities):
        d = N.VmasRenderEntity()
        pos, rot = _f32(e.state.pos), _f32(e.state.rot)
        color = e.color
        color = _f32(color.to(dev)) if isinstance(color, Tensor) else const(color)
        mask = e.is_rendering
        if mask.dtype is not torch.bool or mask.stride(0) != 1:
            mask = mask.to(torch.bool).contiguous()
        keep += [pos, rot, color, mask]
        d.pos, d.rot, d.color, d.mask = pos.data_ptr(), rot.data_ptr(), color.data_ptr(), mask.data_ptr()
        d.pos_s0, d.rot_s0 = pos.stride(0), rot.stride(0)
        d.color_s0 = color.stride(0) if color.dim() > 1 else 0
        shape = e.shape
        if isinstance(shape, Sphere):
            d.shape, d.radius = N.VMAS_SPHERE, shape.radius
        elif isinstance(shape, Box):
            d.shape, d.length, d.width, d.vert_slot = N.VMAS_BOX, shape.length, shape.width, n_boxes
            n_boxes += 1
        elif isinstance(shape, Line):
            d.shape, d.length, d.width = N.VMAS_LINE, shape.length, shape.width
        else:
            raise NotImplementedError(f"render_batch cannot draw shape {type(shape).__name__} of {e.name!r}")
        is_agent = isinstance(e, Agent)
        d.alpha = float(e._alpha) if is_agent else 1.0
        d.slot = slot
        slot += 1
        if is_agent:
            d.flags |= N.VMAS_RENDER_AGENT
            if agent_index_focus is not None and e is env.agents[agent_index_focus]:
                focus = k
            for s in e._sensors or ():
                meas = s._last_measurement
                if not s._render or meas is None:
                    continue
                li = N.VmasRenderLidar()
                ang, meas = _f32(s._angles), _f32(meas)
                keep += [ang, meas]
                li.pos, li.rot, li.angles, li.dist, li.mask = d.pos, d.rot, ang.data_ptr(), meas.data_ptr(), d.mask
                li.pos_s0, li.rot_s0, li.angles_s0, li.dist_s0 = d.pos_s0, d.rot_s0, ang.stride(0), meas.stride(0)
                li.n_rays, li.slot, li.alpha = meas.shape[1], slot, float(s.alpha)
                li.rgb[:] = [float(c) for c in s.render_color][:3]
                slot += 2 * li.n_rays
                lidars.append(li)
            force = e.state.force if e._render_action else None
            if force is not None:
                force = _f32(force)
                keep.append(force)
                d.flags |= N.VMAS_RENDER_ACTION
                d.force, d.force_s0 = force.data_ptr(), force.stride(0)
                d.action_scale = 10 * shape.circumscribed_radius()
                d.action_slot = slot
                slot += 1
        ents.append(d)
    sc = N.VmasRenderScene()
    sc.width, sc.height, sc.focus, sc.n_boundary = width, height, focus, len(segs)
    for k, (a, b) in enumerate(segs):
        sc.boundary[k][:] = [a[0], a[1], b[0], b[1]]
    sc.plot_grid, sc.grid_spacing = int(bool(scn.plot_grid)), float(scn.grid_spacing)
    sc.origin[:] = [float(scn.render_origin[0]), float(scn.render_origin[1])]
    sc.zoom = float(scn.viewer_zoom)
    sc.max_agent_radius = max(a.shape.circumscribed_radius() for a in world.agents)
    sc.n_boxes, sc.n_prims, sc.batch = n_boxes, slot, B
    e_arr = (N.VmasRenderEntity * len(ents))(*ents)
    l_arr = (N.VmasRenderLidar * len(lidars))(*lidars) if lidars else None
    lib = N.load_library()
    idx_dev, stream = N.launch_args(dev)
    prims = torch.empty(n_frames * slot * N.RENDER_PRIM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    verts = torch.empty((n_frames, max(n_boxes, 1), 4, 2), dtype=torch.float32, device=dev)
    bounds = torch.empty((n_frames, 4), dtype=torch.float32, device=dev)
    out = torch.empty((n_frames, height, width, 3), dtype=torch.uint8, device=dev)
    N.check_aux(lib.vmas_render_scene(idx_dev, n_frames, idx_ptr, e_arr, len(ents), l_arr, len(lidars), ctypes.byref(sc),
                                      prims.data_ptr(), verts.data_ptr(), bounds.data_ptr(), stream), "vmas_render_scene")
    N.check_aux(lib.vmas_render_frames(idx_dev, n_frames, height, width, prims.data_ptr(), slot, verts.data_ptr(),
                                       n_frames * max(n_boxes, 1) * 4, out.data_ptr(), stream), "vmas_render_frames")
    del keep
    return (out, bounds) if with_bounds else out
