"""The frame function of rgb_array rendering, restated in NumPy float64 from its definition (the
comment above VmasRenderPrim in include/vmas_mi355x.h), independently of csrc/vmas_render.hip, and
the seeded random scenes the render tests share.

A scene is a list of primitives in WORLD units seen through bounds = (left, right, bottom, top):
    ("disc", (cx, cy), r, rgba, border)        ("poly", [(x, y), ...], rgba, border)
    ("seg", (ax, ay), (bx, by), w, rgba)       ("ring", (cx, cy), r, w, rgba)
    ("grid", spacing, length, w, rgba)
Line widths w are in pixels.  ``to_pixels`` applies the world -> pixel map (the bounds must have the
frame's aspect: lengths scale by W / (right - left)); ``frame`` composites pixel-space primitives.

TOLERANCE wherever two implementations are compared: no channel value differs by more than 1 level,
and at most 0.1 % of the channel values differ at all.
"""
import math

import numpy as np

MAX_LEVELS = 1
MAX_FRACTION = 1e-3


def assert_frames_close(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == np.uint8 and b.dtype == np.uint8, (a.shape, b.shape, a.dtype, b.dtype)
    d = np.abs(a.astype(np.int16) - b.astype(np.int16))
    worst, frac = int(d.max(initial=0)), float((d > 0).mean()) if d.size else 0.0
    print(f"frames {what}: max |diff| {worst} levels, {frac:.2e} of the values differ")
    assert worst <= MAX_LEVELS, (what, worst)
    assert frac <= MAX_FRACTION, (what, frac)


def to_pixels(scene, bounds, W, H):
    left, right, bottom, top = bounds
    sx, sy = W / (right - left), H / (top - bottom)

    def pt(q):
        return ((q[0] - left) * sx, (q[1] - bottom) * sy)

    out = []
    for pr in scene:
        k = pr[0]
        if k == "disc":
            out.append(("disc", pt(pr[1]), pr[2] * sx, pr[3], pr[4]))
        elif k == "poly":
            out.append(("poly", [pt(q) for q in pr[1]], pr[2], pr[3]))
        elif k == "seg":
            out.append(("seg", pt(pr[1]), pt(pr[2]), pr[3], pr[4]))
        elif k == "ring":
            out.append(("ring", pt(pr[1]), pr[2] * sx, pr[3], pr[4]))
        elif k == "grid":
            out.append(("grid", pt((0.0, 0.0)), pr[1] * sx, pr[2] / 2 * sx, pr[3], int(math.ceil(pr[2] / pr[1])), pr[4]))
        else:
            raise ValueError(k)
    return out


def _seg_dist(qx, qy, a, b):
    ex, ey = b[0] - a[0], b[1] - a[1]
    px, py = qx - a[0], qy - a[1]
    ee = ex * ex + ey * ey
    t = np.clip((px * ex + py * ey) / ee, 0.0, 1.0) if ee > 0 else np.zeros_like(qx)
    return np.hypot(px - t * ex, py - t * ey)


def _distance(pr, qx, qy):
    k = pr[0]
    if k == "disc":
        return np.hypot(qx - pr[1][0], qy - pr[1][1]) - pr[2]
    if k == "ring":
        return np.abs(np.hypot(qx - pr[1][0], qy - pr[1][1]) - pr[2]) - max(pr[3], 1.0) / 2
    if k == "seg":
        return _seg_dist(qx, qy, pr[1], pr[2]) - max(pr[3], 1.0) / 2
    if k == "poly":
        v = pr[1]
        best = np.full(qx.shape, np.inf)
        inside = np.zeros(qx.shape, dtype=bool)
        for i in range(len(v)):
            a, b = v[i - 1], v[i]
            best = np.minimum(best, _seg_dist(qx, qy, a, b))
            if a[1] != b[1]:
                crosses = (b[1] > qy) != (a[1] > qy)
                xc = (a[0] - b[0]) * (qy - b[1]) / (a[1] - b[1]) + b[0]
                inside ^= crosses & (qx < xc)
        return np.where(inside, -best, best)
    if k == "grid":
        _, o, sp, half, w, n, _ = pr
        ux, uy = qx - o[0], qy - o[1]

        def axis(u):
            kk = np.clip(np.floor((u + half) / sp + 0.5), 0, n - 1)
            return np.abs(u - (kk * sp - half))

        d = np.minimum(axis(ux), axis(uy)) - max(w, 1.0) / 2
        return np.where((np.abs(ux) > half) | (np.abs(uy) > half), np.inf, d)
    raise ValueError(k)


def frame(H, W, prims, floats=False):
    """Composite pixel-space primitives: [H, W, 3] uint8 (floats=True: the float64 colours)."""
    j, i = np.meshgrid(np.arange(W), np.arange(H))
    qx, qy = j + 0.5, H - i - 0.5
    out = np.ones((H, W, 3))

    def blend(rgb, alpha, d):
        nonlocal out
        cov = np.clip(0.5 - d, 0.0, 1.0)[..., None] * alpha
        out = out * (1 - cov) + np.asarray(rgb, dtype=np.float64) * cov

    for pr in prims:
        d = _distance(pr, qx, qy)
        rgba = pr[-2] if pr[0] in ("disc", "poly") else pr[-1]
        blend(rgba[:3], rgba[3], d)
        if pr[0] in ("disc", "poly") and pr[-1]:
            blend([0.5 * c for c in rgba[:3]], 0.5 * rgba[3], np.abs(d) - 1)
    return out if floats else np.floor(255 * out + 0.5).astype(np.uint8)


# ------------------------------------------------------------------------------------------------
# packing a pixel-space list into the native table
MARGIN = 2.0


def pack(prims, n_rows=None, v_base=0):
    """(table [P] of RENDER_PRIM_DTYPE, vertices [V, 2] fp32) of a pixel-space list; padded with
    VMAS_PRIM_NONE records to n_rows; POLY vertex indices start at v_base."""
    from vectorizedmultiagentsimulator_amd import _native as N

    rows = np.zeros(len(prims) if n_rows is None else n_rows, dtype=N.RENDER_PRIM_DTYPE)
    verts = []
    for r, pr in zip(rows, prims):
        k = pr[0]
        if k == "disc":
            e = pr[2] + MARGIN
            r["kind"], r["flags"], r["rgba"], r["p"][:3] = N.VMAS_PRIM_DISC, int(pr[4]), pr[3], (*pr[1], pr[2])
            r["bbox"] = (pr[1][0] - e, pr[1][1] - e, pr[1][0] + e, pr[1][1] + e)
        elif k == "ring":
            e = pr[2] + max(pr[3], 1.0) / 2 + MARGIN
            r["kind"], r["rgba"], r["p"][:4] = N.VMAS_PRIM_RING, pr[4], (*pr[1], pr[2], pr[3])
            r["bbox"] = (pr[1][0] - e, pr[1][1] - e, pr[1][0] + e, pr[1][1] + e)
        elif k == "seg":
            e = max(pr[3], 1.0) / 2 + MARGIN
            r["kind"], r["rgba"], r["p"][:5] = N.VMAS_PRIM_SEG, pr[4], (*pr[1], *pr[2], pr[3])
            r["bbox"] = (min(pr[1][0], pr[2][0]) - e, min(pr[1][1], pr[2][1]) - e,
                         max(pr[1][0], pr[2][0]) + e, max(pr[1][1], pr[2][1]) + e)
        elif k == "poly":
            xs, ys = [q[0] for q in pr[1]], [q[1] for q in pr[1]]
            r["kind"], r["flags"], r["rgba"] = N.VMAS_PRIM_POLY, int(pr[3]), pr[2]
            r["v0"], r["nv"] = v_base + len(verts), len(pr[1])
            r["bbox"] = (min(xs) - MARGIN, min(ys) - MARGIN, max(xs) + MARGIN, max(ys) + MARGIN)
            verts += pr[1]
        elif k == "grid":
            _, o, sp, half, w, n, rgba = pr
            e = half + MARGIN
            k0 = math.floor(half / sp + 0.5)  # the record counts lines from the one nearest the origin
            r["kind"], r["rgba"], r["p"] = N.VMAS_PRIM_GRID, rgba, (o[0], o[1], sp, half, w, k0 * sp - half)
            r["v0"], r["nv"] = -k0, n - 1 - k0
            r["bbox"] = (o[0] - e, o[1] - e, o[0] + e, o[1] + e)
    return rows, np.asarray(verts, dtype=np.float32).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------
# seeded random scenes: all kinds, in world units around the origin
def random_scene(rng, n, extent=1.0):
    scene = []
    for _ in range(n):
        kind = rng.choice(["disc", "poly", "box", "seg", "ring", "grid"], p=[0.25, 0.15, 0.2, 0.25, 0.1, 0.05])
        rgba = tuple(rng.uniform(0, 1, 3)) + (float(rng.choice([1.0, 1.0, rng.uniform(0.2, 0.9)])),)
        c = rng.uniform(-extent, extent, 2)
        border = bool(rng.integers(2))
        if kind == "disc":
            scene.append(("disc", tuple(c), float(rng.uniform(0.01, 0.3) * extent), rgba, border))
        elif kind == "ring":
            scene.append(("ring", tuple(c), float(rng.uniform(0.05, 0.4) * extent), float(rng.uniform(0.3, 4)), rgba))
        elif kind == "seg":
            d = rng.uniform(-0.6, 0.6, 2) * extent
            scene.append(("seg", tuple(c), tuple(c + d), float(rng.uniform(0.05, 5)), rgba))
        elif kind == "box":
            hl, hw, th = rng.uniform(0.02, 0.4) * extent, rng.uniform(0.02, 0.2) * extent, rng.uniform(0, 2 * math.pi)
            cs, sn = math.cos(th), math.sin(th)
            corners = [(-hl, -hw), (-hl, hw), (hl, hw), (hl, -hw)]
            scene.append(("poly", [(c[0] + x * cs - y * sn, c[1] + x * sn + y * cs) for x, y in corners], rgba, border))
        elif kind == "poly":  # a star-shaped simple polygon (convex or not) of 3..9 vertices
            m = int(rng.integers(3, 10))
            ang = np.sort(rng.uniform(0, 2 * math.pi, m)) + np.arange(m) * 1e-3
            rad = rng.uniform(0.05, 0.35, m) * extent
            scene.append(("poly", [(c[0] + r * math.cos(a), c[1] + r * math.sin(a)) for a, r in zip(ang, rad)], rgba, border))
        else:
            scene.append(("grid", float(rng.uniform(0.08, 0.3) * extent), 50.0, float(rng.uniform(0.3, 2)), rgba))
    return scene


# (frame (H, W), P, bounds of the E = 3 frames scaled by the frame's aspect)
CASES = [((37, 53), 0), ((37, 53), 7), ((64, 64), 40), ((53, 37), 300), ((64, 64), 300), ((700, 700), 13),
         ((700, 700), 60)]


def case_frames(H, W, P, seed):
    """The three frames of a case: [(bounds, pixel-space list)] with different bounds each."""
    rng = np.random.default_rng(seed)
    aspect = W / H
    frames = []
    for zoom, (ox, oy) in ((1.0, (0.0, 0.0)), (1.7, (0.3, -0.2)), (0.6, (-0.25, 0.4))):
        half_x, half_y = (zoom * aspect, zoom) if aspect >= 1 else (zoom, zoom / aspect)
        bounds = (ox - half_x, ox + half_x, oy - half_y, oy + half_y)
        frames.append((bounds, to_pixels(random_scene(rng, P), bounds, W, H)))
    return frames


def native_frames(device_index, frames, H, W, stream=None, torch_device=None):
    """vmas_render_frames over case_frames' output: [E, H, W, 3] uint8 (NumPy).  device_index < 0:
    the host backend; else the tables go to torch_device and the launch to its current stream."""
    from vectorizedmultiagentsimulator_amd import _native as N

    P = max((len(f[1]) for f in frames), default=0)
    tables, verts, v_base = [], [], 0
    for _, prims in frames:
        t, v = pack(prims, n_rows=P, v_base=v_base)
        tables.append(t)
        verts.append(v)
        v_base += len(v)
    table = np.concatenate(tables) if P else np.zeros(0, dtype=N.RENDER_PRIM_DTYPE)
    verts = np.concatenate(verts) if verts else np.zeros((0, 2), dtype=np.float32)
    lib = N.load_library()
    E = len(frames)
    if device_index < 0:
        out = np.empty((E, H, W, 3), dtype=np.uint8)
        rc = lib.vmas_render_frames(-1, E, H, W, table.ctypes.data if table.size else None, P,
                                    verts.ctypes.data if verts.size else None, len(verts), out.ctypes.data, None)
        assert rc == 0, N.load_library().vmas_aux_last_error()
        return out
    import torch

    d_table = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(torch_device)
    d_verts = torch.from_numpy(verts.reshape(-1).copy()).to(torch_device)
    out = torch.full((E, H, W, 3), 7, dtype=torch.uint8, device=torch_device)
    rc = lib.vmas_render_frames(device_index, E, H, W, d_table.data_ptr() if table.size else None, P,
                                d_verts.data_ptr() if verts.size else None, len(verts), out.data_ptr(), stream)
    assert rc == 0, N.load_library().vmas_aux_last_error()
    return out.cpu().numpy()
