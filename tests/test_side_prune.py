"""k_world's side pruning (csrc/vmas_physics.hpp side_bounds, csrc/vmas_jit.hip side_prune: a box-line
pair as one task over the box sides that can hold the closest point) changes no bit: from the same
state, the kernel generated with VMAS_JIT_SIDE_PRUNE=1 (the default) and the one with =0 (the pair
split into per-side parts, full scans) produce torch.equal states, step after step, in the default math
mode and with VMAS_JIT_MATH=exact; with exact math both also equal the generic k_step (VMAS_JIT=0),
which never prunes.  200 envs: three full 64-env groups plus one of 8 lanes."""
import math

import pytest
import torch

from oracle import vmas_oracle as O
from tests._parity import make

WORLDS = {
    "balance": (dict(n_agents=4), 10),                      # split box-line (floor / line), 5 box-sphere
    "transport": (dict(n_agents=4), None),                  # box-sphere against movable packages
    "pollock": (dict(n_agents=4, n_lines=3, n_boxes=3), None),  # box-sphere, box-line, box-box
    "waterfall": (dict(), None),                            # joints (always exact), box-line, box-box
}


def _worlds(monkeypatch, device, name, num_envs, math_mode, seed=3):
    """The same world three ways (the knobs are read when the kernel is built): pruned, unpruned,
    and -- exact math only -- the generic k_step."""
    kw, sub = WORLDS[name]
    if math_mode == "exact":
        monkeypatch.setenv("VMAS_JIT_MATH", "exact")
    else:
        monkeypatch.delenv("VMAS_JIT_MATH", raising=False)
    envs = {}
    for key, var, val in (("pruned", "VMAS_JIT_SIDE_PRUNE", "1"), ("full", "VMAS_JIT_SIDE_PRUNE", "0"),
                          ("k_step", "VMAS_JIT", "0")):
        if key == "k_step" and math_mode != "exact":
            continue
        monkeypatch.setenv(var, val)
        envs[key] = make(name, kw, sub, device, num_envs=num_envs, seed=seed)
        envs[key].world.engine._ensure()
    monkeypatch.delenv("VMAS_JIT", raising=False)
    src = {k: e.world.engine.jit_source() for k, e in envs.items() if k != "k_step"}
    if name == "transport":  # no box-line pair: the same kernel either way
        assert src["pruned"] == src["full"]
    else:
        assert "pair_bl_pruned(" in src["pruned"] and "bl_part(" not in src["pruned"]
        assert "bl_part(" in src["full"] or "pair_bl(" in src["full"]  # (split, or a plan without splits)
    assert "pruned" not in src["full"]
    return envs


def _same(a, b, nan_equal=False):
    if nan_equal:
        return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))
    return torch.equal(a, b)


def _step_all_and_compare(envs, snap, what, nan_equal=False):
    """One world.step() of every variant from `snap`; every state field equal to the pruned one's."""
    out = {}
    for key, env in envs.items():
        O.load_snapshot(env.world, snap)
        env.world.step()
        out[key] = O.snapshot(env.world)
        assert env.world.engine.kernel_name == ("k_step" if key == "k_step" else "k_world"), env.world.engine.jit_error
    for key in out:
        if key == "pruned":
            continue
        for i in out["pruned"]:
            for k in out["pruned"][i]:
                assert _same(out["pruned"][i][k], out[key][i][k], nan_equal), (what, key, envs["pruned"].world.entities[i].name, k)
    return out["pruned"]


@pytest.mark.gpu
@pytest.mark.parametrize("math_mode", ["default", "exact"])
@pytest.mark.parametrize("name", list(WORLDS))
def test_pruned_steps_equal_full_steps_gpu(gpu_device, monkeypatch, name, math_mode):
    envs = _worlds(monkeypatch, gpu_device, name, 200, math_mode)
    lead = envs["pruned"]
    for t in range(8):
        lead.step(lead.get_random_actions())  # (free run: fresh random agent forces every step)
        snap = O.snapshot(lead.world)
        _step_all_and_compare(envs, snap, (name, math_mode, t))


def _crafted_balance(env):
    """128 envs.  Group 0 (envs 0-63): the line well above mid-floor in every lane -- ends and
    underside of the floor prune for the whole wave.  Group 1 (64-127): even lanes with the line
    overhanging the floor's end at x = 5 or standing on end, odd lanes with it resting on the
    floor -- the wave's vote fails and the full scan runs."""
    sc, w = env.scenario, env.world
    B, dev = 128, w.device
    g = torch.Generator().manual_seed(11)
    top = float(sc.floor.state.pos[0, 1]) + sc.floor.shape.width / 2  # the floor's upper face
    lp = torch.zeros(B, 2)
    lr = torch.zeros(B, 1)
    lp[:64, 0] = torch.rand(64, generator=g) * 2 - 1
    lp[:64, 1] = 0.2 + 0.6 * torch.rand(64, generator=g)
    lr[:64, 0] = (torch.rand(64, generator=g) * 2 - 1) * 0.5
    # The world clamps the line's centre to y >= -1, 0.03 above the floor's face: a line touches
    # the floor with an end (or its flank on the floor's corner), never lying flat.
    rest = top + 0.004  # inside the line's contact shell (LINE_MIN_DIST = 0.0067)
    half = sc.line_length / 2
    for b in range(64, 128):
        lane = b - 64
        x = float(torch.rand(1, generator=g)) * 2 - 1
        if lane % 2:  # resting on the floor: centre at the clamp, one end down on the face
            lp[b] = torch.tensor([x, -1.0])
            lr[b, 0] = math.asin((-1.0 - rest) / half) * (1 if lane % 4 == 1 else -1)
        elif lane % 4 == 0:  # overhanging the end at x = 5: the flank passes just above the corner
            lp[b] = torch.tensor([4.9, -1.0])
            lr[b, 0] = -math.atan((-1.0 - rest) / 0.1)
        else:  # standing on end
            lp[b] = torch.tensor([x, rest + half])
            lr[b, 0] = math.pi / 2
    zeros2, zeros1 = torch.zeros(B, 2, device=dev), torch.zeros(B, 1, device=dev)
    lp, lr = lp.to(dev), lr.to(dev)
    sc.line.set_pos(lp, batch_index=None)
    sc.line.set_rot(lr, batch_index=None)
    along = torch.cat([torch.cos(lr), torch.sin(lr)], dim=1)
    up = torch.cat([-torch.sin(lr), torch.cos(lr)], dim=1)  # the line's normal
    # the package on the line; in the resting lanes over the low end, whose weight keeps it down
    off = torch.zeros(B, 1, device=dev)
    off[65:128:4] = -0.3
    off[67:128:4] = 0.3
    sc.package.set_pos(lp + along * off + up * (sc.package.shape.radius + 0.005), batch_index=None)
    for i, a in enumerate(w.agents):  # above the line, clear of it and of each other
        a.set_pos(lp + torch.tensor([-0.3 + 0.2 * i, 0.9], device=dev), batch_index=None)
    for e in [sc.line, sc.package, *w.agents]:
        e.set_vel(zeros2, batch_index=None)
    sc.line.state.ang_vel = zeros1.clone()


@pytest.mark.gpu
@pytest.mark.parametrize("math_mode", ["default", "exact"])
def test_crafted_balance_vote_passes_and_fails_gpu(gpu_device, monkeypatch, math_mode):
    envs = _worlds(monkeypatch, gpu_device, "balance", 128, math_mode)
    lead = envs["pruned"]
    _crafted_balance(lead)
    snap = O.snapshot(lead.world)
    for t in range(4):
        snap = _step_all_and_compare(envs, snap, ("crafted", math_mode, t))
    O.load_snapshot(lead.world, snap)
    sc = lead.scenario
    d = lead.world.get_distance(sc.line, sc.floor)
    assert bool((d[64:] <= 0.0).all()), d[64:]  # group 1: the line within its contact distance of the floor
    assert bool((d[:64] > 0.5).all())


@pytest.mark.gpu
@pytest.mark.parametrize("math_mode", ["default", "exact"])
def test_nan_line_position_gpu(gpu_device, monkeypatch, math_mode):
    """A NaN in one env's line position: its wave's votes fail (nothing pruned there), the other
    waves prune; the NaN pattern and every other value are the full scan's."""
    envs = _worlds(monkeypatch, gpu_device, "balance", 200, math_mode)
    lead = envs["pruned"]
    for _ in range(2):
        lead.step(lead.get_random_actions())
    snap = O.snapshot(lead.world)
    li = lead.world.entities.index(lead.scenario.line)
    snap[li]["pos"][70, 0] = float("nan")
    for t in range(3):
        snap = _step_all_and_compare(envs, snap, ("nan", math_mode, t), nan_equal=True)
    assert bool(torch.isnan(snap[li]["pos"][70]).any())
    assert not bool(torch.isnan(snap[li]["pos"][:64]).any())
