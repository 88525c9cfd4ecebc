"""Seeded random-structure worlds and contact-seeking states for tests/test_world_fuzz.py.

``build(seed, batch, device)`` makes a bare ``World`` (no scenario, as tests/_kat.py:world_with)
whose structure -- world parameters, entity kinds / shapes / flags / limits, collision filters,
joints -- is drawn from ``random.Random(seed)`` alone, so that it is the same on every device.
``state(world, seed)`` draws a snapshot from a torch CPU generator; ``install`` writes it.

Placement seeks contact without deep overlap: every entity sits next to a randomly chosen earlier
one (its ``parent``), in a random direction per env, at the centre distance where their surfaces
are a per-env gap in [-0.005, +0.02] from touching (bisection on the oracle's own distance query,
started from the circumscribed radii); of N_CANDIDATES (direction, rotation) candidates each env
takes the one that keeps the entity clear of the other entities.  The later entity of a joint is
instead placed so that the two anchors are ``dist`` (+ up to 5 mm) apart and a fixed rotation is
met within 0.03 rad.  Uniform placement would put ~13 % of the envs on crossing segments, whose
distance is exactly 0 -- on the ``dist < 1e-6`` cut-off, where an env certifies itself and tests
nothing.

What the generator does not draw, and why (conditions on the inputs; none is a limit of the
engine or of the specialiser, which refused no world):
  * no entity is the later end of two joints, and two joints on one entity take its two ends (a
    joint left stretched, or three bodies folded onto one hinge, fly through each other);
  * a collidable joint only between spheres or non-colliding entities (its landmark's ends lie on
    the anchors: on a Line or Box that is distance 0, the cut-off, in every env);
  * a sphere's anchor stays inside the unit circle (outside it the reference's
    Sphere.get_delta_from_anchor puts the anchor ~1 / radius metres away);
  * velocities, forces and torques are a few mm of motion per step (VEL ...): faster thin shapes
    pass through each other within the step.  The speed / force / torque limits are drawn
    around the same scales, so that they bite in part of the envs;
  * <= 7 entities + <= 2 joint landmarks; dt = 0.1; contact_margin, joint_force and
    torque_constraint_force at the package defaults.
"""
from __future__ import annotations

import functools
import math
import random
from types import SimpleNamespace

import torch

from oracle import vmas_oracle as O
from vectorizedmultiagentsimulator_amd.simulator.core import Agent, Box, Landmark, Line, Sphere, World
from vectorizedmultiagentsimulator_amd.simulator.dynamics.holonomic import Holonomic
from vectorizedmultiagentsimulator_amd.simulator.dynamics.holonomic_with_rot import HolonomicWithRotation
from vectorizedmultiagentsimulator_amd.simulator.joints import Joint

# the smallest count from 24 up that meets test_fuzz_seed_set_is_not_vacuous
SEEDS = list(range(26))
BATCHES = [1, 2, 63, 64, 65, 70, 129]  # one env, two, a wave - 1, a wave, a wave + 1, + 6, two groups + 1
N_CANDIDATES = 16  # placements (direction, rotation) tried per env
# Scales of the random state.  A contact of a few mm depth pushes back with c * depth ~ 1 N; what
# moves an entity further than that in one step (0.1 s) drives thin shapes (lines, hollow boxes)
# straight through each other, onto the dist == 0 cut-off.  The clamps of build() are drawn around
# these scales, so that they bite in part of the envs.
VEL, ANG_VEL, FORCE, TORQUE = 0.05, 0.2, 0.3, 0.003


def batch_of(seed: int) -> int:
    return BATCHES[SEEDS.index(seed) % len(BATCHES)]


def _maybe(rng, p, draw):
    return draw() if rng.random() < p else None


def _shape(rng):
    kind = rng.choice(["sphere", "sphere", "box", "hollow", "line"])
    if kind == "sphere":
        return Sphere(radius=round(rng.uniform(0.03, 0.1), 3))
    if kind == "line":
        return Line(length=round(rng.uniform(0.1, 0.4), 3))
    return Box(length=round(rng.uniform(0.1, 0.3), 3), width=round(rng.uniform(0.05, 0.2), 3),
               hollow=kind == "hollow")


def build(seed: int, batch: int, device) -> World:
    rng = random.Random(seed)
    n = rng.randint(1, 7)
    n_joints = rng.randint(1, 2) if (n >= 2 and rng.random() < 0.4) else 0
    substeps = rng.randint(2 if n_joints else 1, 5)  # (World.add_joint: joints need substeps > 1)
    w = World(
        batch, device, dt=0.1, substeps=substeps,
        drag=rng.choice([0.0, 0.1, 0.25, 0.4]),
        linear_friction=rng.choice([0.0, 0.0, 0.05, 0.3]),
        angular_friction=rng.choice([0.0, 0.0, 0.02, 0.2]),
        x_semidim=_maybe(rng, 0.4, lambda: round(rng.uniform(0.15, 0.6), 2)),
        y_semidim=_maybe(rng, 0.4, lambda: round(rng.uniform(0.15, 0.6), 2)),
        collision_force=float(rng.randint(100, 500)),
        gravity=rng.choice([(0.0, 0.0), (0.0, 0.0), (0.0, -0.5), (0.3, -0.2)]),
    )
    w.export_forces = rng.random() < 0.5
    names = [f"e{i}" for i in range(n)]
    gen = torch.Generator().manual_seed(1000 + seed)  # values of [B, 2] gravities only

    # joints (pairs of entity indices), drawn before the entities so that each can be added as
    # soon as both its entities exist: the joint landmark then lands in the middle of the list
    joint_specs = []
    taken, end = set(), {}
    for _ in range(n_joints):
        # each joint is satisfied by where its later entity is put, so no entity is the later one
        # of two joints (a joint left stretched pulls with joint_force x metres: bodies would
        # fly through each other within a substep)
        a, b = rng.sample(range(n), 2)
        if max(a, b) in taken:
            continue
        taken.add(max(a, b))
        dist = rng.choice([0.0, 0.15, 0.3])
        rot_a, rot_b = rng.random() < 0.5, rng.random() < 0.5
        fix_a = round(rng.uniform(-1.0, 1.0), 2) if (not rot_a and rng.random() < 0.5) else None
        fix_b = round(rng.uniform(-1.0, 1.0), 2) if (not rot_b and rng.random() < 0.5) else None
        if dist == 0:
            # (Joint: with dist 0 there is one constraint and no landmark to latch a rotation
            # from: it rotates when both ends do, else it needs the one fixed rotation both share)
            if rot_a and rot_b:
                fix_a = fix_b = None
            else:
                rot_a = rot_b = False
                fix_a = fix_b = fix_a if fix_a is not None else round(rng.uniform(-1.0, 1.0), 2)
        joint_specs.append(dict(
            a=a, b=b, dist=dist, rotate_a=rot_a, rotate_b=rot_b, fixed_rotation_a=fix_a, fixed_rotation_b=fix_b,
            anchor_a=_anchor(rng, end, a), anchor_b=_anchor(rng, end, b),
            collidable=dist > 0 and rng.random() < 0.5,  # (Joint: collidable needs dist > 0)
        ))

    ents, parent, filters, moving_static = [], [], {}, []
    joints = []
    for i in range(n):
        is_agent = i == 0 or rng.random() < 0.5
        movable, rotatable, collide = rng.random() < 0.7, rng.random() < 0.6, rng.random() < 0.8
        grav_kind = rng.choice(["none", "none", "vec", "tensor"])
        gravity = None
        if grav_kind == "vec":
            gravity = [round(rng.uniform(-0.5, 0.5), 2), round(rng.uniform(-0.5, 0.5), 2)]
        elif grav_kind == "tensor":
            gravity = (torch.rand(batch, 2, generator=gen) - 0.5).to(device)
        kw = dict(
            shape=_shape(rng), movable=movable, rotatable=rotatable, collide=collide,
            mass=round(rng.uniform(0.5, 5.0), 2),
            drag=_maybe(rng, 0.3, lambda: round(rng.uniform(0.0, 0.5), 2)),
            linear_friction=_maybe(rng, 0.3, lambda: round(rng.uniform(0.0, 0.5), 2)),
            angular_friction=_maybe(rng, 0.3, lambda: round(rng.uniform(0.0, 0.3), 2)),
            max_speed=_maybe(rng, 0.3, lambda: round(rng.uniform(0.02, 0.12), 3)),
            v_range=_maybe(rng, 0.3, lambda: round(rng.uniform(0.02, 0.12), 3)),
            gravity=gravity,
        )
        if i > 0 and rng.random() < 0.2:
            # a filter that excludes one named entity: mostly the one it will be placed against
            other = rng.randrange(i)
            filters[i] = names[other]
            kw["collision_filter"] = functools.partial(_not_named, names[other])
        if is_agent:
            # drawn independently of movable / rotatable: a clamp on an agent that cannot move
            kw.update(
                max_f=_maybe(rng, 0.35, lambda: round(rng.uniform(0.1, 0.5), 2)),
                f_range=_maybe(rng, 0.35, lambda: round(rng.uniform(0.1, 0.5), 2)),
                max_t=_maybe(rng, 0.35, lambda: round(rng.uniform(0.0005, 0.004), 4)),
                t_range=_maybe(rng, 0.35, lambda: round(rng.uniform(0.0005, 0.004), 4)),
                dynamics=HolonomicWithRotation() if rotatable else Holonomic(),
            )
            e = Agent(names[i], **kw)
            w.add_agent(e)
        else:
            e = Landmark(names[i], **kw)
            w.add_landmark(e)
        ents.append(e)
        parent.append(_parent_of(rng, i, filters, names))
        # an entity that cannot move may still hold a velocity (friction acts on it)
        moving_static.append(rng.random() < 0.3)
        for js in joint_specs:
            if max(js["a"], js["b"]) == i:
                # A collidable joint landmark is a Line whose ends sit on the two anchors.  On a
                # sphere that is an ordinary (deep) contact; on a Line or Box the end lies on or
                # across the entity's own segments, where the distance is exactly 0 -- the
                # dist < 1e-6 cut-off in every env.  So: collidable only between spheres and
                # entities that do not collide.
                touchable = all(isinstance(ents[k].shape, Sphere) or not ents[k].collide for k in (js["a"], js["b"]))
                for end_, k in (("anchor_a", js["a"]), ("anchor_b", js["b"])):
                    if isinstance(ents[k].shape, Sphere):
                        # keep a sphere's anchor inside the unit circle: outside it the reference
                        # (Sphere.get_delta_from_anchor) divides by norm x radius and puts the
                        # anchor ~1 / radius metres away, a lever that overflows within a step
                        x, y = js[end_]
                        js[end_] = (x, round(math.copysign(min(abs(y), 0.95 * math.sqrt(max(1 - x * x, 0.0))), y), 3))
                js["collidable"] = js["collidable"] and touchable
                j = Joint(ents[js["a"]], ents[js["b"]], anchor_a=js["anchor_a"], anchor_b=js["anchor_b"],
                          rotate_a=js["rotate_a"], rotate_b=js["rotate_b"], dist=js["dist"],
                          collidable=js["collidable"], fixed_rotation_a=js["fixed_rotation_a"],
                          fixed_rotation_b=js["fixed_rotation_b"], mass=round(rng.uniform(0.5, 2.0), 2))
                w.add_joint(j)
                joints.append((js, j))
    w._fuzz = SimpleNamespace(seed=seed, ents=ents, parent=parent, filters=filters, joints=joints,
                              moving_static=moving_static)
    return w


def _anchor(rng, end, i):
    """An off-centre anchor near one end of entity i's long axis: two bodies hinged there can
    point away from each other; hinged near their centres they could only lie across each other.
    A second joint on the same entity takes the other end, so that a chain stretches out instead
    of folding three bodies onto one point."""
    sign = -end[i] if i in end else rng.choice([-1, 1])
    end[i] = sign
    return (sign * round(rng.uniform(0.85, 1.0), 2), round(rng.uniform(-0.9, 0.9), 2))


def _not_named(name, e):
    return e.name != name


def _parent_of(rng, i, filters, names):
    """The earlier entity that entity i is placed against (None for the first)."""
    if i == 0:
        return None
    if i in filters and rng.random() < 0.7:
        return names.index(filters[i])
    return rng.randrange(i)


# ---- placement ----------------------------------------------------------------------------------
_QUERY = O.OracleWorld.__new__(O.OracleWorld)  # the distance queries read nothing of the world


def _gap(shape_a, pos_a, rot_a, shape_b, pos_b, rot_b):
    """Surface distance of two shapes minus what 'touching' means to the contact force (the
    oracle's get_distance: < 0 exactly where the contact force is on)."""
    a = SimpleNamespace(shape=shape_a, state=SimpleNamespace(pos=pos_a, rot=rot_a))
    b = SimpleNamespace(shape=shape_b, state=SimpleNamespace(pos=pos_b, rot=rot_b))
    if {type(shape_a), type(shape_b)} == {Box, Sphere}:
        # (get_distance reports every touching box-sphere pair as -1: no gradient to bisect on;
        # the signed surface distance instead, -1 only for a centre inside the box)
        box, sph = (a, b) if isinstance(shape_a, Box) else (b, a)
        cp = O.get_closest_point_box(box.state.pos, box.state.rot, box.shape.width, box.shape.length, sph.state.pos)
        d_sc = torch.linalg.vector_norm(sph.state.pos - cp, dim=-1)
        d_sb = torch.linalg.vector_norm(sph.state.pos - box.state.pos, dim=-1)
        d_cb = torch.linalg.vector_norm(box.state.pos - cp, dim=-1)
        return torch.where(d_sb < d_cb, -1.0, d_sc - O.LINE_MIN_DIST - sph.shape.radius)
    return _QUERY.get_distance(a, b).clone()


def _unit(theta):
    return torch.cat([theta.cos(), theta.sin()], dim=-1)


def _place_next_to(shape, rot, p_shape, p_pos, p_rot, theta, target):
    """Centre of ``shape`` in direction ``theta`` from the parent, at the distance where their gap
    crosses ``target`` ([B]): bisection from the circumscribed radii inward."""
    B = rot.shape[0]
    hi = torch.full((B, 1), p_shape.circumscribed_radius() + shape.circumscribed_radius() + 0.03)
    lo = torch.zeros(B, 1)
    u = _unit(theta)
    for _ in range(14):  # (to 0.5 m / 2^14 = 0.03 mm)
        mid = (lo + hi) / 2
        above = (_gap(shape, p_pos + mid * u, rot, p_shape, p_pos, p_rot) > target).unsqueeze(-1)
        hi = torch.where(above, mid, hi)
        lo = torch.where(above, lo, mid)
    return p_pos + hi * u


def state(world, seed: int):
    """A snapshot (O.snapshot's layout) of ``world``; the same for every device."""
    fz = world._fuzz
    g = torch.Generator().manual_seed(seed)
    B = world.batch_dim
    uni = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g)  # noqa: E731
    pos, rot = {}, {}
    joint_of = {}  # later entity index -> (spec, joint) of its first joint
    for js, j in fz.joints:
        joint_of.setdefault(max(js["a"], js["b"]), (js, j))
    # A fixed rotation is met where the state is drawn (a constraint torque grows as exp(|error|)
    # and overflows within a step from a random angle).  Joint.notify points a joint landmark
    # along atan2, in (-pi, pi]: the earlier entity of a joint with a fixed rotation at its end
    # draws its rotation so that rot + fixed stays inside that range (``shift``).
    shift = {}
    for js, j in fz.joints:
        if js["dist"] > 0:
            o_end = "a" if js["a"] < js["b"] else "b"
            if js["fixed_rotation_" + o_end] is not None:
                shift[js[o_end]] = js["fixed_rotation_" + o_end]
    free_rot = lambda k: uni(-math.pi + 0.1, math.pi - 0.1, B, 1) - shift.get(k, 0.0)  # noqa: E731
    wrap = lambda a: torch.atan2(a.sin(), a.cos())  # noqa: E731
    jit = lambda: uni(-0.03, 0.03, B, 1)  # noqa: E731
    for i, e in enumerate(fz.ents):
        if i == 0:
            pos[i], rot[i] = uni(-0.05, 0.05, B, 2), free_rot(i)
            continue
        p = fz.parent[i]
        target = uni(-0.005, 0.02, B)
        if i in joint_of:
            js, j = joint_of[i]
            i_end, o_end = ("b", "a") if js["b"] == i else ("a", "b")
            o = js[o_end]
            ks = j.joint_constraints
            d_i = torch.tensor((ks[-1] if i_end == "b" else ks[0]).delta_anchor(e), dtype=torch.float32)
            d_o = torch.tensor((ks[0] if i_end == "b" else ks[-1]).delta_anchor(fz.ents[o]), dtype=torch.float32)
            anchor_o = pos[o] + O.rotate_vector(d_o.expand(B, 2), rot[o])
            skip = o if js["dist"] == 0 else None  # (a dist-0 joint's pair is not a contact pair)
            fix_i, fix_o = js["fixed_rotation_" + i_end], js["fixed_rotation_" + o_end]
        else:
            skip = p
        best_pos = best_rot = best_score = None
        for _ in range(N_CANDIDATES * (3 if i in joint_of else 1)):
            c_rot = free_rot(i)
            if i in joint_of:
                # the two anchors dist (+ up to 5 mm) apart, in a random direction
                sep = js["dist"] + uni(0.0, 0.005, B, 1)
                phi = uni(-math.pi, math.pi, B, 1)  # direction from anchor a to anchor b
                if js["dist"] == 0:
                    if fix_i is not None:  # rot_a = rot_b + fixed
                        c_rot = rot[o] + (fix_i if i_end == "a" else -fix_i) + jit()
                else:
                    if fix_o is not None:  # the landmark's rotation (phi) = rot_o + fixed_o
                        phi = rot[o] + fix_o + jit()
                    if fix_i is not None:
                        c_rot = wrap(phi) - fix_i + jit()
                anchor_i = anchor_o + (sep if i_end == "b" else -sep) * _unit(phi)
                c_pos = anchor_i - O.rotate_vector(d_i.expand(B, 2), c_rot)
            else:
                c_pos = _place_next_to(e.shape, c_rot, fz.ents[p].shape, pos[p], rot[p],
                                       uni(-math.pi, math.pi, B, 1), target)
            clear = torch.full((B,), float("inf"))
            for k in range(i):
                if k != skip:
                    clear = torch.minimum(clear, _gap(e.shape, c_pos, c_rot, fz.ents[k].shape, pos[k], rot[k]))
            score = clear.clamp(max=0.004)  # clear of the others by 4 mm is as good as any
            if best_pos is None:
                best_pos, best_rot, best_score = c_pos, c_rot, score
            else:
                better = (score > best_score).unsqueeze(-1)
                best_pos = torch.where(better, c_pos, best_pos)
                best_rot = torch.where(better, c_rot, best_rot)
                best_score = torch.maximum(score, best_score)
        pos[i], rot[i] = best_pos, best_rot
    index = {id(e): i for i, e in enumerate(fz.ents)}
    snap = {}
    for wi, e in enumerate(world.entities):
        if id(e) in index:
            i = index[id(e)]
            moves = e.movable or fz.moving_static[i]
            turns = e.rotatable or fz.moving_static[i]
            d = {"pos": pos[i], "rot": rot[i],
                 "vel": VEL * torch.randn(B, 2, generator=g) if moves else torch.zeros(B, 2),
                 "ang_vel": ANG_VEL * torch.randn(B, 1, generator=g) if turns else torch.zeros(B, 1)}
            if isinstance(e, Agent):
                d["force"] = FORCE * torch.randn(B, 2, generator=g)
                d["torque"] = TORQUE * torch.randn(B, 1, generator=g)
        else:
            # a joint landmark: between its two anchors (as Joint.notify centres it), a few mm off
            js, j = next((js, j) for js, j in fz.joints if j.landmark is e)
            ia, ib = js["a"], js["b"]
            da = torch.tensor(j.joint_constraints[0].delta_anchor(j.entity_a), dtype=torch.float32)
            db = torch.tensor(j.joint_constraints[1].delta_anchor(j.entity_b), dtype=torch.float32)
            pa = pos[ia] + O.rotate_vector(da.expand(B, 2), rot[ia])
            pb = pos[ib] + O.rotate_vector(db.expand(B, 2), rot[ib])
            d = {"pos": (pa + pb) / 2 + uni(-0.003, 0.003, B, 2),
                 "rot": torch.atan2(pb[:, 1] - pa[:, 1], pb[:, 0] - pa[:, 0]).unsqueeze(-1) + uni(-0.02, 0.02, B, 1),
                 "vel": VEL * torch.randn(B, 2, generator=g), "ang_vel": ANG_VEL * torch.randn(B, 1, generator=g)}
        snap[wi] = {k: v.to(torch.float32).contiguous() for k, v in d.items()}
    return snap


def install(world, snap) -> None:
    """Write ``snap`` into the world (O.load_snapshot), then let every joint that latches a
    rotation do so: an end with rotate_* = False and no fixed rotation takes its fixed rotation
    from the state in Joint.notify, which a reset runs through set_rot -- load_snapshot's direct
    writes do not, and the engine refuses a constraint whose fixed_rotation is still None.  The
    notify also re-centres the joint landmark; its snapshot row is written again afterwards."""
    O.load_snapshot(world, snap)
    latched = False
    for js, j in world._fuzz.joints:
        if j.landmark is None:
            continue
        for e, rotate, fixed in ((j.entity_a, j.rotate_a, j.fixed_rotation_a),
                                 (j.entity_b, j.rotate_b, j.fixed_rotation_b)):
            if not rotate and fixed is None:
                e.set_rot(e.state.rot.clone(), batch_index=None)
                latched = True
    if latched:
        O.load_snapshot(world, snap)


@functools.lru_cache(maxsize=None)
def _cpu_case(seed: int):
    w = build(seed, batch_of(seed), "cpu")
    return w, state(w, seed)


def case(seed: int, device="cpu"):
    """(world on ``device`` with its state installed, the snapshot).  The snapshot of a seed is
    computed once and shared: treat it as read-only."""
    w0, snap = _cpu_case(seed)
    w = build(seed, batch_of(seed), device)
    install(w, snap)
    return w, snap
