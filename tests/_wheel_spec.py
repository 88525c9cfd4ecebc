"""The wheel scenario's per-step values, restated on plain CPU tensors (the yardstick of
tests/test_wheel_dispersion*.py; written from the scenario's description, never importing it).

For env b, line L, agent a:  rew = | |L.ang_vel| - desired_velocity |, every agent's reward is -rew;
the observation's 13 columns are a.pos, a.vel, L.pos - a.pos, e1 - a.pos, -e1 - a.pos,
remainder(L.rot, pi), |L.ang_vel|, rew -- with e1 = f32(line_length / 2) * (cos L.rot, sin L.rot).
Every operation is fp32 (numpy float32 scalars, one rounding each); cos / sin are taken once over the
whole [B, 1] rotation tensor with torch, as any torch program takes them."""
import math

import numpy as np
import torch

F = np.float32
PI32 = F(math.pi)


def remainder(a, b):
    """torch.remainder for floats: fmod, moved into the divisor's sign."""
    m = np.fmod(F(a), F(b))
    if m != 0 and ((b < 0) != (m < 0)):
        m = F(m + F(b))
    return F(m)


class WheelSpec:
    def __init__(self, env):
        scn, w = env.scenario, env.world
        cpu = lambda t: t.detach().cpu().clone()  # noqa: E731
        self.B = w.batch_dim
        self.line_length, self.desired_velocity = scn.line_length, scn.desired_velocity
        line = next(e for e in w.landmarks if e.name == "line")
        self.line_pos, self.line_rot, self.line_ang_vel = cpu(line.state.pos), cpu(line.state.rot), cpu(line.state.ang_vel)
        self.pos = [cpu(a.state.pos) for a in w.agents]
        self.vel = [cpu(a.state.vel) for a in w.agents]

    def run(self):
        B, n = self.B, len(self.pos)
        half, dv = F(self.line_length / 2), F(self.desired_velocity)
        cos, sin = torch.cos(self.line_rot).numpy(), torch.sin(self.line_rot).numpy()
        rew = np.zeros((B, 1), dtype=F)
        obs = [np.zeros((B, 13), dtype=F) for _ in range(n)]
        for b in range(B):
            av = np.abs(self.line_ang_vel[b, 0].numpy())
            rew[b, 0] = np.abs(F(av - dv))
            ex, ey = F(half * cos[b, 0]), F(half * sin[b, 0])
            lx, ly = self.line_pos[b].numpy()
            for k in range(n):
                px, py = self.pos[k][b].numpy()
                vx, vy = self.vel[k][b].numpy()
                obs[k][b] = [px, py, vx, vy, F(lx - px), F(ly - py), F(ex - px), F(ey - py), F(F(-ex) - px),
                             F(F(-ey) - py), remainder(self.line_rot[b, 0].numpy(), PI32), av, rew[b, 0]]
        rew = torch.from_numpy(rew)
        return {"rew": rew, "rewards": [-rew for _ in range(n)], "obs": [torch.from_numpy(o) for o in obs]}


# ---- hand-placed cases -------------------------------------------------------------------------------
ROTS = {"rot_0": 0.0, "rot_half_pi": math.pi / 2, "rot_minus_half_pi": -math.pi / 2, "rot_minus_0.3": -0.3,
        "rot_3pi_0.1": 3 * math.pi + 0.1, "rot_pi32": float(PI32), "rot_minus_pi32": -float(PI32)}
ANG_VELS = {"av_0": 0.0, "av_desired": None, "av_minus_desired": None, "av_minus_0.7": -0.7, "av_2": 2.0}
# name -> the env in which it must fire (rotation cases, then angular velocity cases)
CASE_ENVS = {name: i for i, name in enumerate(list(ROTS) + list(ANG_VELS))}


def _ang_vel(name, dv):
    return {"av_desired": dv, "av_minus_desired": -dv}.get(name, ANG_VELS[name])


def place_cases(env):
    """Overwrite the line's rotation / angular velocity by hand (12+ envs)."""
    scn = env.scenario
    line = scn.line
    rot, av = line.state.rot.clone(), line.state.ang_vel.clone()
    for name, value in ROTS.items():
        rot[CASE_ENVS[name], 0] = value
    for name in ANG_VELS:
        av[CASE_ENVS[name], 0] = _ang_vel(name, scn.desired_velocity)
    line.set_rot(rot, batch_index=None)
    line.set_ang_vel(av, batch_index=None)


def assert_cases_fired(spec: WheelSpec, exp):
    """On the spec's own outputs (``exp = spec.run()`` after place_cases): the known answers."""
    half, dv = F(spec.line_length / 2), F(spec.desired_velocity)
    o, rew = exp["obs"][0].numpy(), exp["rew"].numpy()
    px, py = spec.pos[0].numpy().T

    def env(name):
        return CASE_ENVS[name]

    b = env("rot_0")
    assert o[b, 10] == 0 and o[b, 6] == F(half - px[b]) and o[b, 7] == F(F(0) - py[b]) and o[b, 8] == F(-half - px[b])
    # +-pi/2 both end up at pi/2 (the negative one moved into the divisor's sign)
    assert o[env("rot_half_pi"), 10] == F(math.pi / 2)
    assert o[env("rot_minus_half_pi"), 10] == F(F(-math.pi / 2) + PI32) and abs(o[env("rot_minus_half_pi"), 10] - math.pi / 2) < 1e-6
    assert o[env("rot_minus_0.3"), 10] == F(F(-0.3) + PI32)
    assert abs(float(o[env("rot_3pi_0.1"), 10]) - 0.1) < 2e-6 and o[env("rot_3pi_0.1"), 10] == np.fmod(F(3 * math.pi + 0.1), PI32)
    assert o[env("rot_pi32"), 10] == 0 and o[env("rot_minus_pi32"), 10] == 0
    assert (o[:, 10] >= 0).all() and (o[:, 10] < PI32).all()
    assert rew[env("av_0"), 0] == dv and o[env("av_0"), 11] == 0
    for name in ("av_desired", "av_minus_desired"):
        assert rew[env(name), 0] == 0 and o[env(name), 11] == dv and o[env(name), 12] == 0
    assert rew[env("av_minus_0.7"), 0] == F(F(0.7) - dv) and o[env("av_minus_0.7"), 11] == F(0.7)
    assert rew[env("av_2"), 0] == F(F(2) - dv)
    for r in exp["rewards"]:
        assert torch.equal(r, -exp["rew"])
