"""Analytic known-answer tests of the queries and of the step's gradient: ray casts, distance
queries, overlap tests and the vector-Jacobian product, each against a closed form written out in
the test (float64 ``math``; neither the oracle nor the package produces an expected value), on
the oracle and on the engine for every target of tests/_kat.py."""
import math
import os

import pytest
import torch

from oracle import vmas_oracle as O
from vectorizedmultiagentsimulator_amd.simulator.core import Agent, Box, Landmark, Line, Sphere
from vectorizedmultiagentsimulator_amd.simulator.sensors import Lidar

from _kat import C, DT, GPU_BATCH, K, LMD, Target, allclose, deviation, set_state, tgt, world_with  # noqa: F401

AGENT_POS = (0.1, -0.2)
MAX_RANGE = 1.0
SQ2 = math.sqrt(2)

# (id, target shape, placement relative to the agent, target rot, ray angle, expected distance)
RAY_CASES = [
    ("sphere-oblique", lambda: Sphere(0.1), (0.3, 0.4), 0.0, math.atan2(4, 3), 0.4),  # 0.5 - r along (3, 4) / 5
    ("line-diagonal", lambda: Line(0.4), (0.5, 0.0), math.pi / 4, 0.0, 0.5),  # through the line's centre
    ("line-oblique-ray", lambda: Line(0.4), (0.5, 0.0), math.pi / 2, 0.1, 0.5 / math.cos(0.1)),
    ("box-rotated", lambda: Box(length=0.4, width=0.2), (0.5, 0.1), math.pi / 2, 0.0, 0.4),  # near face x = 0.5 - 0.1
    ("box-vertex", lambda: Box(length=0.2, width=0.2), (0.5, 0.0), math.pi / 4, 0.0, 0.5 - 0.1 * SQ2),
    ("behind", lambda: Sphere(0.1), (-0.5, 0.0), 0.0, 0.0, MAX_RANGE),
    ("in-front-ray-backwards", lambda: Sphere(0.1), (0.5, 0.0), 0.0, math.pi, MAX_RANGE),
    ("box-behind", lambda: Box(length=0.2, width=0.2), (-0.5, 0.0), 0.0, 0.0, MAX_RANGE),
    ("line-behind", lambda: Line(0.4), (-0.5, 0.0), math.pi / 2, 0.0, MAX_RANGE),
]


def near(pair, want, tgt, label=None):
    """Both results of an (oracle, engine) pair equal the closed form ``want`` within abs 1e-6 in
    every env; prints each deviation before it asserts."""
    label = label or os.environ.get("PYTEST_CURRENT_TEST", "").split("::")[-1].split(" ")[0]
    for who, res in zip(("oracle", tgt.name), pair):
        dev = deviation(res.reshape(res.shape[0], -1), want)
        print(f"KAT {label} [{who}]: |dev| {dev:.3g} tol 1e-06")
        assert dev <= 1e-6, (label, who, dev)


def _rays_both(w, ag, angles, entity_filter):
    """(oracle, engine) ray distances of ``ag`` for absolute ``angles``."""
    got = w.cast_rays(ag, angles, max_range=MAX_RANGE, entity_filter=entity_filter)
    ow = O.OracleWorld(w, O.snapshot(w))
    exp = ow.cast_rays(w.entities.index(ag), angles.cpu(), MAX_RANGE, entity_filter)
    return exp, got


@pytest.mark.parametrize("shape,rel,rot,angle,expected", [c[1:] for c in RAY_CASES], ids=[c[0] for c in RAY_CASES])
def test_ray_cast_from_offset_agent(tgt, shape, rel, rot, angle, expected):
    ag = Agent("ag", shape=Sphere(0.01))
    target = Landmark("t", shape=shape())
    w = world_with(ag, target, tgt=tgt)
    set_state(ag, AGENT_POS, tgt=tgt)
    set_state(target, (AGENT_POS[0] + rel[0], AGENT_POS[1] + rel[1]), rot=rot, tgt=tgt)
    angles = torch.full((tgt.batch, 1), angle, device=tgt.device)
    near(_rays_both(w, ag, angles, lambda e: e is target), [expected], tgt)


def test_ray_nearer_of_two_targets_wins(tgt):
    ag = Agent("ag", shape=Sphere(0.01))
    front = Landmark("front", shape=Sphere(0.1))
    far = Landmark("far", shape=Box(length=0.2, width=0.2))
    hidden = Landmark("hidden", shape=Line(0.4))  # nearer still, but filtered out
    w = world_with(ag, far, front, hidden, tgt=tgt)
    set_state(ag, AGENT_POS, tgt=tgt)
    set_state(front, (AGENT_POS[0] + 0.5, AGENT_POS[1]), tgt=tgt)
    set_state(far, (AGENT_POS[0] + 0.8, AGENT_POS[1]), tgt=tgt)
    set_state(hidden, (AGENT_POS[0] + 0.2, AGENT_POS[1]), rot=math.pi / 2, tgt=tgt)
    angles = torch.zeros(tgt.batch, 1, device=tgt.device)
    near(_rays_both(w, ag, angles, lambda e: e is front or e is far), [0.4], tgt)
    near(_rays_both(w, ag, angles, lambda e: e is far), [0.7], tgt)
    near(_rays_both(w, ag, angles, lambda e: e is not ag), [0.2], tgt)


def test_lidar_angle_row_and_agent_rot(tgt):
    """A 12-ray Lidar spaces its rays 2 pi / 12 apart from angle 0 and adds the agent's rot.  One
    sphere (r = 0.1, 0.5 away) sits 0.05 rad off ray 2: that ray travels D cos(a) - sqrt(r^2 -
    D^2 sin(a)^2), every other ray misses (the neighbours pass D sin(pi / 6 -+ 0.05) > r away)."""
    n, rot, off, D, r = 12, 0.3, 0.05, 0.5, 0.1
    ag = Agent("ag", shape=Sphere(0.01))
    target = Landmark("t", shape=Sphere(r))
    w = world_with(ag, target, tgt=tgt)
    lidar = Lidar(w, n_rays=n, max_range=MAX_RANGE, entity_filter=lambda e: e is target)
    ag.add_sensor(lidar)
    set_state(ag, AGENT_POS, rot=rot, tgt=tgt)
    phi = rot + 2 * 2 * math.pi / n + off
    set_state(target, (AGENT_POS[0] + D * math.cos(phi), AGENT_POS[1] + D * math.sin(phi)), tgt=tgt)
    row = [2 * math.pi * i / n for i in range(n)]
    assert allclose(lidar._angles, row, abs_=1e-6) and lidar._angles.shape == (tgt.batch, n)
    hit = D * math.cos(off) - math.sqrt(r * r - (D * math.sin(off)) ** 2)
    want = [MAX_RANGE] * n
    want[2] = hit
    assert D * math.sin(2 * math.pi / n - off) > r
    got = lidar.measure()
    ow = O.OracleWorld(w, O.snapshot(w))
    exp = ow.cast_rays(w.entities.index(ag), (lidar._angles + ag.state.rot).cpu(), MAX_RANGE, lambda e: e is target)
    near((exp, got), want, tgt)
    assert abs(hit - (D - r)) > 50e-6  # the off-centre hit differs from a central one


# ---- distance queries ---------------------------------------------------------------------------
def _dist_both(w, a, b):
    ow = O.OracleWorld(w, O.snapshot(w))
    return ow.get_distance(ow.ents[w.entities.index(a)], ow.ents[w.entities.index(b)]), w.get_distance(a, b)


def _overlap_both(w, a, b):
    ow = O.OracleWorld(w, O.snapshot(w))
    return ow.is_overlapping(ow.ents[w.entities.index(a)], ow.ents[w.entities.index(b)]), w.is_overlapping(a, b)


def _point_both(w, e, point, tgt):
    p = torch.tensor([point] * tgt.batch, dtype=torch.float32, device=tgt.device)
    ow = O.OracleWorld(w, O.snapshot(w))
    return ow.get_distance_from_point(ow.ents[w.entities.index(e)], p.cpu()), w.get_distance_from_point(e, p)


def test_distance_line_line_end_to_interior(tgt):
    l1 = Landmark("l1", shape=Line(1.0))
    l2 = Landmark("l2", shape=Line(0.4))
    w = world_with(l1, l2, tgt=tgt)
    set_state(l1, (0.0, 0.0), tgt=tgt)
    set_state(l2, (0.3, 0.5), rot=math.pi / 2, tgt=tgt)  # its lower end at (0.3, 0.3)
    near(_dist_both(w, l1, l2), [0.3 - LMD], tgt)
    for res in _overlap_both(w, l1, l2):
        assert not bool(res.any())


def test_distance_box_box_vertex_to_face(tgt):
    a = Landmark("a", shape=Box(length=1.0, width=0.5))
    b = Landmark("b", shape=Box(length=0.2, width=0.2))
    w = world_with(a, b, tgt=tgt)
    set_state(a, (0.0, 0.0), tgt=tgt)
    set_state(b, (0.5 + 0.2 + 0.1 * SQ2, 0.15), rot=math.pi / 4, tgt=tgt)  # vertex 0.2 off the right face
    near(_dist_both(w, a, b), [0.2 - LMD], tgt)


def test_distance_sphere_line(tgt):
    s = Landmark("s", shape=Sphere(0.1))
    line = Landmark("line", shape=Line(1.0))
    w = world_with(s, line, tgt=tgt)
    set_state(s, (0.2, 0.0), tgt=tgt)
    set_state(line, (0.0, 2.0), tgt=tgt)
    near(_dist_both(w, s, line), [2 - 0.1 - LMD], tgt)


def test_distance_from_point(tgt):
    s = Landmark("s", shape=Sphere(0.1))
    box = Landmark("box", shape=Box(length=1.0, width=0.5))
    line = Landmark("line", shape=Line(1.0))
    w = world_with(s, box, line, tgt=tgt)
    set_state(s, (1.0, 0.0), tgt=tgt)
    set_state(box, (0.0, 0.0), tgt=tgt)
    set_state(line, (0.0, 2.0), tgt=tgt)
    # sphere: |(0.3, 0.4)| - r; box: above the interior of the top face; line: below its interior
    for e, point, want in ((s, (1.3, 0.4), 0.4), (box, (0.2, 1.0), 0.75 - LMD), (line, (0.1, 1.5), 0.5 - LMD)):
        near(_point_both(w, e, point, tgt), [want], tgt)


@pytest.mark.parametrize("kind", ["sphere-sphere", "sphere-line"])
def test_is_overlapping_both_sides_of_zero(tgt, kind):
    """The overlap test flips where the closed-form distance crosses zero (1e-4 either side)."""
    a = Landmark("a", shape=Sphere(0.05))
    b = Landmark("b", shape=Sphere(0.05) if kind == "sphere-sphere" else Line(1.0))
    w = world_with(a, b, tgt=tgt)
    touch = 0.1 if kind == "sphere-sphere" else 0.05 + LMD
    set_state(b, (0.0, 0.0), tgt=tgt)
    for gap in (1e-4, -1e-4):
        set_state(a, (0.2, touch + gap) if kind == "sphere-line" else (touch + gap, 0.0), tgt=tgt)
        near(_dist_both(w, a, b), [gap], tgt)
        for res in _overlap_both(w, a, b):
            assert bool(res.all()) == (gap < 0) and bool(res.any()) == (gap < 0)


# ---- the step's gradient ------------------------------------------------------------------------
GRAD_TARGETS = [
    pytest.param(("cpu", 1), id="cpu"),
    pytest.param(("cuda:0", GPU_BATCH), id="gpu", marks=pytest.mark.gpu),
]


@pytest.mark.parametrize("target", GRAD_TARGETS)
def test_step_vjp_closed_form(target):
    """Sphere-sphere contact, mass 2, drag 0.25, sphere at (0.09, 0) moving (0.2, 0.1):
    vx' = 0.75 vx + c pen(0.1 - px) dt / m and px' = px + vx' dt, and d pen(x) / dx =
    sigmoid(x / k), so with s = sigmoid(10):
        d vx'/d px = -c s dt / m,  d vx'/d vx = 0.75,  d px'/d px = 1 - c s dt^2 / m,
        d px'/d vx = 0.075,  and x does not depend on y at py = 0 (cross terms 0).
    Checked on the engine's native VJP and on autograd of the oracle, rel 1e-4."""
    device, batch = target
    if device != "cpu" and not torch.cuda.is_available():
        pytest.skip("no ROCm GPU visible")
    t = Target(device, batch, None)
    m = 2.0
    s = 1.0 / (1.0 + math.exp(-(0.1 - 0.09) / K))
    want = {
        "vel": {"pos": [-C * s * DT / m, 0.0], "vel": [0.75, 0.0]},
        "pos": {"pos": [1.0 - C * s * DT * DT / m, 0.0], "vel": [0.075, 0.0]},
    }
    for out in ("vel", "pos"):
        a = Landmark("a", shape=Sphere(0.05), movable=True, mass=m)
        b = Landmark("b", shape=Sphere(0.05))
        w = world_with(a, b, drag=0.25, tgt=t)
        set_state(a, (0.09, 0.0), vel=(0.2, 0.1), tgt=t)
        set_state(b, (0.0, 0.0), tgt=t)
        snap = O.snapshot(w)
        ora = {i: {k: v.clone().requires_grad_(True) for k, v in d.items()} for i, d in snap.items()}
        pos = a.state.pos.clone().requires_grad_(True)
        vel = a.state.vel.clone().requires_grad_(True)
        a.state.pos, a.state.vel = pos, vel
        w.step()
        getattr(a.state, out)[:, 0].sum().backward()  # d (x component of out) / d inputs, per env
        ow = O.OracleWorld(w, ora)
        ow.step()
        ow.result()[0][out][:, 0].sum().backward()
        for wrt, got, exp in (("pos", pos.grad, ora[0]["pos"].grad), ("vel", vel.grad, ora[0]["vel"].grad)):
            for who, g in (("oracle", exp), ("engine", got)):
                dev = deviation(g, want[out][wrt])
                print(f"KAT vjp d{out}.x/d{wrt} [{who}/{device}]: |dev| {dev:.3g}")
                assert allclose(g, want[out][wrt], rel=1e-4, abs_=1e-7), (out, wrt, who, g[0].tolist())
    # non-vacuity: without the softplus' slope (a hard contact, s = 1) the stiffness term moves
    # by (1 - s) = 4.5e-5 relative only, so the pin on s is the pen KATs'; a dropped 1 / m doubles it
    assert abs(want["vel"]["pos"][0] - (-C * s * DT)) > 50 * 1e-4 * abs(want["vel"]["pos"][0])
