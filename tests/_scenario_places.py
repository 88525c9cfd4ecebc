"""Hand-placed states for the balance / transport / discovery / flocking programs, as
tests/_navigation_spec.py place_cases does for navigation: random steps never reach the "true" side
of their branches (a fallen package, a package on its goal, a covered target, a collision), so a
test overwrites positions in fixed env ranges and names the envs where each flag must fire.

``place(name, env)`` needs 64+ envs, is called identically on every env under comparison and
returns ``{flag: mask}``: ``flag`` must be true in the envs of ``mask``; a key ``not_<flag>`` names
envs where it must be false.  ``observed(name, env, out)`` reads the same flags from one
evaluation's outputs (obs, rewards, dones, infos) and the scenario attributes the program leaves
behind; ``check(masks, flags)`` asserts them and that every flag is true in some env and false in
another, so a test on them cannot pass vacuously.  Every offset comes from the entities' own shape
attributes and the scenario's parameters.
"""
import math

import torch

from vectorizedmultiagentsimulator_amd.simulator.utils import LINE_MIN_DIST


def _mask(B, dev, *ranges):
    m = torch.zeros(B, dtype=torch.bool, device=dev)
    for lo, hi in ranges:
        m[lo:hi] = True
    return m


def _put(entity, rows, pos):
    """entity.state.pos[rows] = pos (re-bound through set_pos, as a user's edit would be)."""
    p = entity.state.pos.clone()
    p[rows] = pos
    entity.set_pos(p, batch_index=None)


def _xy(dev, x, y):
    return torch.tensor([x, y], device=dev, dtype=torch.float32)


def place_balance(env):
    """Envs 0-7 the package within 0.2 * goal.radius of its goal (done, not on the ground); 8-15
    the package centre half its radius above the floor's top face (the sphere-closest-point side of
    the box-sphere overlap); 16-23 the package centre inside the floor box (the centre-distance
    side); 24-31 the line, with the agents under it, 0.003 above the top face (inside the line's
    contact shell: the line-box distance); 32+ untouched."""
    w, sc = env.world, env.scenario
    B, dev = w.batch_dim, w.device
    assert B >= 64
    pk, goal, line, floor = sc.package, sc.package.goal, sc.line, sc.floor
    r = pk.shape.radius
    top = floor.state.pos[:, 1] + floor.shape.width / 2
    assert 0.25 * floor.shape.width > r + LINE_MIN_DIST and 0.003 < LINE_MIN_DIST
    a, b, c, d = slice(0, 8), slice(8, 16), slice(16, 24), slice(24, 32)
    pos = pk.state.pos.clone()
    pos[a] = goal.state.pos[a] + _xy(dev, 0.2 * goal.shape.radius, 0.0)
    pos[b, 1] = top[b] + 0.5 * r
    pos[c, 1] = top[c] - 0.25 * floor.shape.width
    pk.set_pos(pos, batch_index=None)
    drop = line.state.pos[d, 1] - (top[d] + 0.003)
    for e in [line] + list(w.agents):
        p = e.state.pos.clone()
        p[d, 1] -= drop
        e.set_pos(p, batch_index=None)
    return {"on_the_ground": _mask(B, dev, (8, 32)), "not_on_the_ground": _mask(B, dev, (0, 8)),
            "done": _mask(B, dev, (0, 32))}


def place_transport(env):
    """Package 0: envs 0-15 the goal centre inside the box; 16-23 outside it, half a goal radius
    from a side; 24-31 goal.radius + 0.02 from that side (off).  Envs 0-7: every other package on
    the goal too (done), so with 2+ packages envs 8-23 have one package on and the others as the
    reset left them."""
    w, sc = env.world, env.scenario
    B, dev = w.batch_dim, w.device
    assert B >= 64
    pks = sc.packages
    p0, goal = pks[0], pks[0].goal
    L, R = p0.shape.length, goal.shape.radius
    assert 0.02 > LINE_MIN_DIST  # (the overlap test's threshold is radius + LINE_MIN_DIST)
    g = goal.state.pos
    pos = p0.state.pos.clone()
    pos[0:16] = g[0:16] + _xy(dev, 0.25 * L, 0.0)
    pos[16:24] = g[16:24] + _xy(dev, L / 2 + 0.5 * R, 0.0)
    pos[24:32] = g[24:32] + _xy(dev, L / 2 + R + 0.02, 0.0)
    p0.set_pos(pos, batch_index=None)
    n = len(pks)
    for k, p in enumerate(pks[1:], start=1):  # distinct spots, the goal centre inside every box
        rad = 0.25 * min(p.shape.length, p.shape.width)
        th = 2 * math.pi * k / n
        _put(p, slice(0, 8), g[0:8] + _xy(dev, rad * math.cos(th), rad * math.sin(th)))
    return {"on_goal_0": _mask(B, dev, (0, 24)), "not_on_goal_0": _mask(B, dev, (24, 32)),
            "done": _mask(B, dev, (0, 8)), "not_done": _mask(B, dev, (24, 32))}


def place_discovery(env):
    """Around target 0, with c the covering range and k = agents_per_target: envs 0-7 agents
    0..k-1 at 0.6 c (covered); 8-15 agents 0..k-2 there and every other agent on a ring at
    c + 0.01 (one short); 16-23 (more than k agents) target 1 moved to 1.2 c from target 0 and
    agents 0..k side by side between the two (the count exceeds the threshold; each of them is in
    range of two covered targets)."""
    w, sc = env.world, env.scenario
    B, dev = w.batch_dim, w.device
    assert B >= 64
    agents, targets = w.agents, sc._targets
    A, T = len(agents), len(targets)
    c, k = sc._covering_range, sc._agents_per_target
    r = agents[0].shape.radius
    assert 1 <= k <= A and 0.6 * c > r + targets[0].shape.radius
    t0 = targets[0].state.pos
    masks = {"covered_0": _mask(B, dev, (0, 8)), "not_covered_0": _mask(B, dev, (8, 16))}
    for i, a in enumerate(agents):
        pos = a.state.pos.clone()
        th = 2 * math.pi * i / k + 0.3
        if i < k:
            pos[0:8] = t0[0:8] + _xy(dev, 0.6 * c * math.cos(th), 0.6 * c * math.sin(th))
        if i < k - 1:
            pos[8:16] = t0[8:16] + _xy(dev, 0.6 * c * math.cos(th), 0.6 * c * math.sin(th))
        else:
            th = 2 * math.pi * i / A + 0.3
            pos[8:16] = t0[8:16] + _xy(dev, (c + 0.01) * math.cos(th), (c + 0.01) * math.sin(th))
        a.set_pos(pos, batch_index=None)
    if A > k:
        s = slice(16, 24)
        # towards the middle of the arena, so that nothing lands outside the world's bounds
        sign = torch.where(t0[s, 0] > 0, -1.0, 1.0).unsqueeze(-1)
        if T >= 2:
            _put(targets[1], s, t0[s] + sign * _xy(dev, 1.2 * c, 0.0))
        gap = min(0.5 * c, 1.4 * c / k)
        assert k * gap / 2 < 0.8 * c
        for i in range(k + 1):
            _put(agents[i], s, t0[s] + sign * _xy(dev, 0.6 * c, 0.0) + _xy(dev, 0.0, (i - k / 2) * gap))
        masks["covered_0"] = _mask(B, dev, (0, 8), (16, 24))
        masks["over_threshold_0"] = _mask(B, dev, (16, 24))
        if T >= 2:
            masks["covered_1"] = _mask(B, dev, (16, 24))
            masks["two_targets_agent_0"] = _mask(B, dev, (16, 24))
    return masks


def place_flocking(env):
    """Envs 0-7 policy agents 0 and 1 with surfaces 0.004 apart (inside min_collision_distance);
    8-15 the same pair 0.006 apart (outside); 16-23 policy agent 0 0.004 from the scripted target;
    24-31 (with obstacles) policy agent 0 at 0.5 * max_range from obstacle 0's surface along its
    ray 0, the other obstacles lined up behind obstacle 0: that ray reads 0.5 * max_range."""
    w, sc = env.world, env.scenario
    B, dev = w.batch_dim, w.device
    assert B >= 64
    pol, tgt, obst = w.policy_agents, sc._target, sc.obstacles
    a0 = pol[0]
    m = sc.min_collision_distance
    assert 0.004 < m < 0.006
    masks = {}
    charged = sc.collision_reward != 0
    if len(pol) > 1:
        a1 = pol[1]
        both = a0.shape.radius + a1.shape.radius
        pos = a1.state.pos.clone()
        pos[0:8] = a0.state.pos[0:8] + _xy(dev, both + 0.004, 0.0)
        pos[8:16] = a0.state.pos[8:16] + _xy(dev, both + 0.006, 0.0)
        a1.set_pos(pos, batch_index=None)
    # on the side the target's script moves it to first (u = (cos 0, sin 0))
    _put(a0, slice(16, 24), tgt.state.pos[16:24] + _xy(dev, tgt.shape.radius + a0.shape.radius + 0.004, 0.0))
    if charged:
        masks["collision_0"] = _mask(B, dev, (16, 24)) | (_mask(B, dev, (0, 8)) if len(pol) > 1 else False)
        if len(pol) > 1:
            masks["not_collision_0"] = _mask(B, dev, (8, 16))
            masks["collision_1"] = _mask(B, dev, (0, 8))
    if obst:
        s = slice(24, 32)
        sensor = a0.sensors[0]
        ang = sensor._angles[s, 0:1] + a0.state.rot[s]
        u = torch.cat([torch.cos(ang), torch.sin(ang)], dim=-1)
        o0 = obst[0].state.pos
        _put(a0, s, o0[s] - u * (obst[0].shape.radius + 0.5 * sensor._max_range))
        for j, o in enumerate(obst[1:], start=1):
            _put(o, s, o0[s] + u * (j * 2.2 * o.shape.radius))
        masks["ray_0_half_range"] = _mask(B, dev, (24, 32))
    return masks


PLACE = {"balance": place_balance, "transport": place_transport, "discovery": place_discovery,
         "flocking": place_flocking}


def place(name, env):
    return PLACE[name](env)


def observed(name, env, out):
    """The flags ``place`` names, read from one evaluation of the program: ``out`` = (obs, rewards,
    dones, infos) of ``env``, plus the attributes its scenario holds afterwards."""
    obs, rews, dones, infos = out[0], out[1], out[2], out[-1]
    sc, w = env.scenario, env.world
    if name == "balance":
        return {"on_the_ground": sc.on_the_ground.clone(), "done": dones.clone(),
                "fell": infos[0]["ground_rew"] == sc.fall_reward}
    if name == "transport":
        f = {f"on_goal_{k}": obs[0][:, 4 + 7 * k + 6] != 0 for k in range(len(sc.packages))}
        f["done"] = dones.clone()
        return f
    if name == "discovery":
        c, k = sc._covering_range, sc._agents_per_target
        cov = sc.covered_targets
        f = {"covered_0": cov[:, 0].clone(), "over_threshold_0": sc.agents_per_target[:, 0] > k}
        if cov.shape[1] > 1:
            f["covered_1"] = cov[:, 1].clone()
            f["two_targets_agent_0"] = w.agents[0].covering_reward >= 2 * sc.covering_rew_coeff
        return f
    if name == "flocking":
        pol = w.policy_agents
        f = {f"collision_{p}": infos[p]["agent_collision_rew"] != 0 for p in range(min(2, len(pol)))}
        s = pol[0].sensors[0]
        half = 0.5 * s._max_range
        f["ray_0_half_range"] = (obs[0][:, 6] - half).abs() <= RAY_ATOL + RAY_RTOL * half
        return f
    raise KeyError(name)


# the LIDAR parity tolerance (tests/_parity.py lidar_parity): the closed form 0.5 * max_range is
# what the oracle's ray-circle intersection gives up to fp32 rounding of the placed positions
RAY_ATOL, RAY_RTOL = 2e-5, 2e-5


def check(masks, flags, what=""):
    for key, mask in masks.items():
        mask = mask.to(torch.bool)
        if key.startswith("not_"):
            f = flags[key[4:]].to(mask.device)
            assert not f[mask].any(), (what, key, f[mask].tolist())
        else:
            f = flags[key].to(mask.device)
            assert f[mask].all(), (what, key, f[mask].tolist())
            assert mask.any() and not f.all(), (what, key, "the flag never turned out false")
