"""vmas_render_frames on the host backend (device = -1): known answers of the frame function with
explicit bounds, seeded random scenes against the float64 restatement (tests/_render_spec.py), and
bad arguments to both render entry points."""
import ctypes
import math

import numpy as np
import pytest

from tests import _render_spec as S
from vectorizedmultiagentsimulator_amd import _native as N

GRAY = (0.25, 0.25, 0.25, 1.0)


def host(prims, H, W):
    return S.native_frames(-1, [(None, prims)], H, W)[0]


def test_gray_disc_centre_and_outside():
    H = W = 41
    f = host([("disc", (20.5, 20.5), 8.0, GRAY, True)], H, W)
    assert tuple(f[20, 20]) == (64, 64, 64)  # floor(255 * 0.25 + 0.5)
    assert tuple(f[20, 20 + 11]) == (255, 255, 255)  # 3 px outside the radius
    assert tuple(f[20 - 11, 20]) == (255, 255, 255)


@pytest.mark.parametrize("r", [2.0, 2.1, 3.7, 10.25, 25.0])
def test_disc_coverage_sums_to_its_area(r):
    # an alpha-1 borderless black disc: 1 - out is the coverage
    H = W = 64
    f = S.frame(H, W, [("disc", (32.3, 31.6), r, (0, 0, 0, 1.0), False)], floats=True)
    n = host([("disc", (32.3, 31.6), r, (0, 0, 0, 1.0), False)], H, W)
    bound = 0.1 * 2 * math.pi * r
    spec_area, native_area = float((1 - f[..., 0]).sum()), float((255 - n[..., 0].astype(np.float64)).sum() / 255)
    print(f"r = {r}: pi r^2 = {math.pi * r * r:.3f}, spec {spec_area:.3f}, native {native_area:.3f}, bound {bound:.3f}")
    assert abs(spec_area - math.pi * r * r) <= bound
    assert abs(native_area - math.pi * r * r) <= bound


def test_rotated_box_centre_and_half_turn_symmetry():
    H = W = 60
    cs, sn = math.cos(0.7), math.sin(0.7)
    corners = [(30 + x * cs - y * sn, 30 + x * sn + y * cs) for x, y in ((-18, -7), (-18, 7), (18, 7), (18, -7))]
    red = (0.75, 0.25, 0.25, 1.0)
    f = host([("poly", corners, red, True)], H, W)
    # the centre pixels are deep inside: the fill colour, no border (|d| - 1 > 0.5)
    assert tuple(f[29, 29]) == tuple(f[30, 30]) == (191, 64, 64)
    assert tuple(f[2, 2]) == (255, 255, 255)
    S.assert_frames_close(f, f[::-1, ::-1], "box vs its 180 degree flip")
    # a point along the box's long axis is inside, the same distance along the short axis is not
    assert tuple(f[H - 1 - int(30 + 14 * sn), int(30 + 14 * cs)]) == (191, 64, 64)
    assert tuple(f[H - 1 - int(30 + 14 * cs), int(30 - 14 * sn)]) == (255, 255, 255)


def test_alpha_blend_of_overlapping_discs():
    H = W = 40
    a = ("disc", (16.0, 20.0), 9.0, (0.75, 0.25, 0.25, 1.0), False)
    b = ("disc", (24.0, 20.0), 9.0, (0.25, 0.25, 0.75, 0.5), False)
    f = host([a, b], H, W)
    # the overlap's centre (20, 20): A over white, then B at alpha 0.5
    want = [math.floor(255 * (ca * 0.5 + cb * 0.5) + 0.5) for ca, cb in zip(a[3][:3], b[3][:3])]
    assert list(f[20, 20]) == list(f[19, 19]) == want
    assert list(f[20, 10]) == [191, 64, 64]  # A alone
    assert list(f[20, 30]) == [math.floor(255 * (0.5 + 0.5 * c) + 0.5) for c in b[3][:3]]  # B over white


def test_plus_y_is_up():
    H, W = 50, 30
    f = host([("disc", (15.0, 40.0), 4.0, GRAY, False)], H, W)  # pixel-space y = 40 of 50: near the top
    dark = np.argwhere(f[..., 0] < 128)
    assert len(dark) and dark[:, 0].max() < H // 2
    assert tuple(f[H - 40, 15]) == (64, 64, 64)


def test_line_width_below_one_is_drawn_as_one_and_kinds():
    H = W = 32
    thin = host([("seg", (4.0, 16.0), (28.0, 16.0), 0.05, (0, 0, 0, 1.0))], H, W)
    one = host([("seg", (4.0, 16.0), (28.0, 16.0), 1.0, (0, 0, 0, 1.0))], H, W)
    assert np.array_equal(thin, one)
    # the line y = 16 lies between two pixel rows: each gets half coverage
    assert thin[15, 16, 0] == thin[16, 16, 0] == 128 and thin[13, 16, 0] == 255
    ring = host([("ring", (16.0, 16.0), 10.0, 2.0, (0, 0, 0, 1.0))], H, W)
    assert ring[16, 16, 0] == 255 and ring[15, 26, 0] < 40 and ring[15, 5, 0] < 40
    grid = host([("grid", (16.0, 16.0), 8.0, 96.0, 1.0, 24, (0, 0, 0, 1.0))], H, W)
    assert grid[15, 20, 0] == 128 and grid[20, 16, 0] == 128 and grid[20, 20, 0] == 255  # lines through (16, 16), period 8
    assert grid[20, 24, 0] == 128 and grid[20, 23, 0] == 128


@pytest.mark.parametrize("shape,P", S.CASES)
def test_random_scenes_match_the_spec(shape, P):
    H, W = shape
    frames = S.case_frames(H, W, P, seed=1000 + P + H)
    got = S.native_frames(-1, frames, H, W)
    assert got.shape == (3, H, W, 3) and got.dtype == np.uint8
    for e, (_, prims) in enumerate(frames):
        S.assert_frames_close(got[e], S.frame(H, W, prims), f"{H}x{W} P={P} frame {e}")
    if P == 0:
        assert (got == 255).all()
    else:
        assert not np.array_equal(got[0], got[1])


def test_struct_layouts_match_the_header(tmp_path):
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    src = tmp_path / "probe.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "vmas_mi355x.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(VmasRenderPrim), sizeof(VmasRenderEntity), sizeof(VmasRenderLidar),
         sizeof(VmasRenderScene), offsetof(VmasRenderPrim, bbox), offsetof(VmasRenderEntity, vert_slot),
         offsetof(VmasRenderLidar, rgb), offsetof(VmasRenderScene, grid_spacing), offsetof(VmasRenderScene, batch));
  return 0; }
''')
    subprocess.run(["gcc", "-I", str(root / "include"), str(src), "-o", str(tmp_path / "probe")], check=True)
    sizes = list(map(int, subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True).stdout.split()))
    assert sizes == [N.RENDER_PRIM_DTYPE.itemsize, ctypes.sizeof(N.VmasRenderEntity), ctypes.sizeof(N.VmasRenderLidar),
                     ctypes.sizeof(N.VmasRenderScene), N.RENDER_PRIM_DTYPE.fields["bbox"][1],
                     N.VmasRenderEntity.vert_slot.offset, N.VmasRenderLidar.rgb.offset,
                     N.VmasRenderScene.grid_spacing.offset, N.VmasRenderScene.batch.offset]


def test_bad_arguments_return_errors():
    lib = N.load_library()
    out = np.zeros((1, 8, 8, 3), dtype=np.uint8)
    prims, verts = S.pack([("poly", [(1, 1), (6, 1), (3, 6)], GRAY, False)])
    ok = lib.vmas_render_frames(-1, 1, 8, 8, prims.ctypes.data, 1, verts.ctypes.data, 3, out.ctypes.data, None)
    assert ok == 0 and out.min() < 255
    assert lib.vmas_render_frames(-1, 1, 8, 8, prims.ctypes.data, 1, verts.ctypes.data, 3, None, None) == -1
    assert b"vmas_render_frames" in lib.vmas_aux_last_error()
    assert lib.vmas_render_frames(-1, 1, 0, 8, prims.ctypes.data, 1, verts.ctypes.data, 3, out.ctypes.data, None) == -1
    assert lib.vmas_render_frames(-1, 1, 8, 8, None, 1, verts.ctypes.data, 3, out.ctypes.data, None) == -1
    assert lib.vmas_render_frames(-1, -1, 8, 8, prims.ctypes.data, 1, verts.ctypes.data, 3, out.ctypes.data, None) == -1
    # a polygon that indexes past the vertex pool, and an unknown kind
    assert lib.vmas_render_frames(-1, 1, 8, 8, prims.ctypes.data, 1, verts.ctypes.data, 2, out.ctypes.data, None) == -1
    prims["kind"] = 9
    assert lib.vmas_render_frames(-1, 1, 8, 8, prims.ctypes.data, 1, verts.ctypes.data, 3, out.ctypes.data, None) == -1

    sc = N.VmasRenderScene()
    assert lib.vmas_render_scene(-1, 1, None, None, 0, None, 0, ctypes.byref(sc), None, None, None, None) == -1
    assert b"vmas_render_scene" in lib.vmas_aux_last_error()
    ent = N.VmasRenderEntity()
    table = np.zeros(4, dtype=N.RENDER_PRIM_DTYPE)
    bounds = np.zeros(4, dtype=np.float32)
    pos, rot, col = np.zeros((1, 2), np.float32), np.zeros((1, 1), np.float32), np.zeros(3, np.float32)
    ent.pos, ent.rot, ent.color, ent.pos_s0, ent.rot_s0 = pos.ctypes.data, rot.ctypes.data, col.ctypes.data, 2, 1
    ent.shape, ent.flags, ent.radius, ent.alpha, ent.slot = N.VMAS_SPHERE, N.VMAS_RENDER_AGENT, 0.1, 1.0, 0
    sc.width, sc.height, sc.focus, sc.zoom, sc.n_prims, sc.batch = 16, 16, -1, 1.0, 1, 1

    def scene():
        return lib.vmas_render_scene(-1, 1, None, ctypes.byref(ent), 1, None, 0, ctypes.byref(sc), table.ctypes.data, None,
                                     bounds.ctypes.data, None)

    assert scene() == 0 and table[0]["kind"] == N.VMAS_PRIM_DISC and list(bounds) == [-1, 1, -1, 1]
    sc.zoom = 0.0
    assert scene() == -1
    sc.zoom, ent.slot = 1.0, 1  # a slot outside the table
    assert scene() == -1
    ent.slot, ent.shape = 0, 7
    assert scene() == -1
    ent.shape, sc.focus = N.VMAS_SPHERE, 3
    assert scene() == -1
    sc.focus, sc.batch = -1, 0
    assert scene() == -1
