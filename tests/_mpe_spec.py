"""MPE simple_spread and simple_tag, per-step values restated on NumPy float32 scalars (the yardstick of
tests/test_mpe*.py; written from the tasks' description, never importing the scenario files).

Every operation is one fp32 rounding, env by env, agent by agent.  |p - q| = sqrt(dx*dx + dy*dy).

spread: closest[l] = min over agents of |a - l|.  rew = 0; per agent i in order: per landmark in order
rew -= closest[l]; then per other agent a in order rew -= 1 where (|a - i| - f32(r_a)) - f32(r_i) < 0.
Everybody's reward is rew.  Observation: pos, vel, landmarks - pos, (obs_agents) others - pos.

tag: hit(i, j) = |i - j| < f32(double(r_i) + double(r_j)).  Good agent: 0, (shaped) + f32(0.1) * |g - adv| per
adversary in order, - 10 per adversary hitting it in order.  Adversary: 0, (shaped) - f32(0.1) * min over
good agents of |g - adv|, + 10 per good agent it hits in order.  Team sums: stack(...).sum(-1) -- the order
of torch's device reduction for n <= 8 (tools/probe_sum_order.py): with k the largest power of
two <= n, k strided accumulators (element i to accumulator i % k, each from 0), combined by an
adjacent-pair tree.  A sharing team returns its sum.  Observation: (observe_vel) vel, (observe_pos) pos,
landmarks - pos, seen others - pos, seen good others' vel; same-team others are seen with
observe_same_team only."""
import math

import numpy as np
import torch

F = np.float32
N_CASE_ENVS = 16


def dist(p, q):
    dx, dy = F(p[0] - q[0]), F(p[1] - q[1])
    return np.sqrt(F(F(dx * dx) + F(dy * dy)))


def team_sum(values):
    """The device order of stack(values, -1).sum(-1) for 1 <= n <= 8 (see the module notes)."""
    n = len(values)
    k = 1 << (n.bit_length() - 1)
    acc = [F(0)] * k
    for i, v in enumerate(values):
        acc[i % k] = F(acc[i % k] + v)
    w = 1
    while w < k:
        for i in range(0, k - w, 2 * w):
            acc[i] = F(acc[i] + acc[i + w])
        w *= 2
    return acc[0]


class MpeSpec:
    def __init__(self, env, task):
        scn, w = env.scenario, env.world
        cpu = lambda t: t.detach().cpu().numpy().copy()  # noqa: E731
        self.task, self.B = task, w.batch_dim
        self.pos = [cpu(a.state.pos) for a in w.agents]
        self.vel = [cpu(a.state.vel) for a in w.agents]
        self.marks = [cpu(m.state.pos) for m in w.landmarks]
        self.radius = [a.shape.radius for a in w.agents]
        self.collide = [bool(a.collide) for a in w.agents]
        self.adversary = [bool(a.adversary) for a in w.agents]
        if task == "spread":
            self.obs_agents = bool(scn.obs_agents)
        else:
            for k in ("shape_agent_rew", "shape_adversary_rew", "agents_share_rew", "adversaries_share_rew",
                      "observe_same_team", "observe_pos", "observe_vel"):
                setattr(self, k, bool(getattr(scn, k)))

    # ---- spread ------------------------------------------------------------------------------------------
    def spread_reward(self, b):
        n = len(self.pos)
        closest = [min(dist(self.pos[a][b], m[b]) for a in range(n)) for m in self.marks]
        rew = F(0)
        for i in range(n):
            for c in closest:
                rew = F(rew - c)
            if not self.collide[i]:
                continue
            for a in range(n):
                if a != i and F(F(dist(self.pos[a][b], self.pos[i][b]) - F(self.radius[a])) - F(self.radius[i])) < 0:
                    rew = F(rew - F(1))
        return rew

    def spread_obs(self, b, k):
        p = self.pos[k][b]
        row = [p[0], p[1], *self.vel[k][b]]
        for m in self.marks:
            row += [F(m[b][0] - p[0]), F(m[b][1] - p[1])]
        if self.obs_agents:
            for j in range(len(self.pos)):
                if j != k:
                    row += [F(self.pos[j][b][0] - p[0]), F(self.pos[j][b][1] - p[1])]
        return row

    # ---- tag ---------------------------------------------------------------------------------------------
    def hit(self, b, i, j):
        return bool(dist(self.pos[i][b], self.pos[j][b]) < F(self.radius[i] + self.radius[j]))

    def tag_agent_rewards(self, b):
        n = len(self.pos)
        advs = [i for i in range(n) if self.adversary[i]]
        good = [i for i in range(n) if not self.adversary[i]]
        out = []
        for i in range(n):
            r = F(0)
            if self.adversary[i]:
                if self.shape_adversary_rew:
                    r = F(r - F(F(0.1) * min(dist(self.pos[g][b], self.pos[i][b]) for g in good)))
                if self.collide[i]:
                    for g in good:
                        if self.hit(b, g, i):
                            r = F(r + F(10))
            else:
                if self.shape_agent_rew:
                    for a in advs:
                        r = F(r + F(F(0.1) * dist(self.pos[i][b], self.pos[a][b])))
                if self.collide[i]:
                    for a in advs:
                        if self.hit(b, a, i):
                            r = F(r - F(10))
            out.append(r)
        return out, good, advs

    def tag_obs(self, b, k):
        p = self.pos[k][b]
        row = ([*self.vel[k][b]] if self.observe_vel else []) + ([p[0], p[1]] if self.observe_pos else [])
        for m in self.marks:
            row += [F(m[b][0] - p[0]), F(m[b][1] - p[1])]
        seen = [j for j in range(len(self.pos))
                if j != k and (self.adversary[j] != self.adversary[k] or self.observe_same_team)]
        for j in seen:
            row += [F(self.pos[j][b][0] - p[0]), F(self.pos[j][b][1] - p[1])]
        for j in seen:
            if not self.adversary[j]:
                row += [*self.vel[j][b]]
        return row

    # ---- a step ------------------------------------------------------------------------------------------
    def run(self):
        B, n = self.B, len(self.pos)
        rewards = [np.zeros(B, dtype=F) for _ in range(n)]
        obs = [[] for _ in range(n)]
        scenario = {}
        if self.task == "spread":
            scenario["rew"] = np.zeros(B, dtype=F)
        else:
            scenario.update(agents_rew=np.zeros(B, dtype=F), adverary_rew=np.zeros(B, dtype=F),
                            rew=[np.zeros(B, dtype=F) for _ in range(n)])
        for b in range(B):
            if self.task == "spread":
                r = self.spread_reward(b)
                scenario["rew"][b] = r
                for k in range(n):
                    rewards[k][b] = r
                    obs[k].append(self.spread_obs(b, k))
            else:
                per, good, advs = self.tag_agent_rewards(b)
                gs, as_ = team_sum([per[i] for i in good]), team_sum([per[i] for i in advs])
                scenario["agents_rew"][b], scenario["adverary_rew"][b] = gs, as_
                for k in range(n):
                    scenario["rew"][k][b] = per[k]
                    share = self.adversaries_share_rew if self.adversary[k] else self.agents_share_rew
                    rewards[k][b] = (as_ if self.adversary[k] else gs) if share else per[k]
                    obs[k].append(self.tag_obs(b, k))
        t = lambda a: torch.from_numpy(np.asarray(a, dtype=F))  # noqa: E731
        scenario = {k: ([t(x) for x in v] if isinstance(v, list) else t(v)) for k, v in scenario.items()}
        return {"rewards": [t(r) for r in rewards], "obs": [t(o) for o in obs], "scenario": scenario}


def scenario_tensors(env, task):
    scn = env.scenario
    if task == "spread":
        return [scn.rew]
    return [scn.agents_rew, scn.adverary_rew] + [a.rew for a in env.agents]


def expected_scenario_tensors(exp, task):
    s = exp["scenario"]
    return [s["rew"]] if task == "spread" else [s["agents_rew"], s["adverary_rew"]] + s["rew"]


def fsum_bound_ok(team_value, members):
    """|team sum - fsum(members)| <= (n - 1) 2^-24 sum |x_i|: the bound of any summation order."""
    xs = [float(x) for x in members]
    return abs(float(team_value) - math.fsum(xs)) <= (len(xs) - 1) * 2.0 ** -24 * math.fsum(abs(x) for x in xs)


# ---- hand-placed cases -------------------------------------------------------------------------------
# Agents and landmarks a case does not name stand on a far grid (apart by 0.6: nothing touches).
R_SPREAD = F(0.3)    # f32(0.15) + f32(0.15), exactly 2 f32(0.15): the overlap boundary
R_TAG = F(0.125)     # f32(0.075 + 0.05): adversary against good agent


def around(x):
    return [np.nextafter(F(x), F(0)), F(x), np.nextafter(F(x), F(1))]


SPREAD_CASES = {  # name -> (env, agents needed)
    "far": (0, 1), "tie": (1, 2), "one_pair": (2, 2), "two_pairs": (3, 3), "thr_below": (4, 2), "thr_at": (5, 2),
    "thr_above": (6, 2), "exact_sum": (7, 1), "last_closest": (8, 2), "diagonal_pair": (9, 2), "coincident": (10, 2),
    "pair_last": (11, 3), "all_on_one": (12, 3), "landmark_far": (13, 1), "pair_12": (14, 3), "touching_apart": (15, 2),
}
TAG_CASES = {  # name -> (env, good agents needed, adversaries needed)
    "far": (0, 1, 1), "one_catch": (1, 1, 1), "two_catch": (2, 1, 2), "all_catch": (3, 1, 1), "thr_below": (4, 1, 1),
    "thr_at": (5, 1, 1), "thr_above": (6, 1, 1), "second_good": (7, 2, 1), "both_good": (8, 2, 1), "shaped_exact": (9, 1, 1),
    "adv_on_adv": (10, 1, 2), "good_on_landmark": (11, 1, 1), "last_adv": (12, 1, 2), "diagonal_catch": (13, 1, 1),
    "diagonal_miss": (14, 1, 1), "coincident": (15, 1, 1),
}


def _far(pos, marks, b):
    for i, p in enumerate(pos):
        p[b, 0], p[b, 1] = -3.0 + 0.75 * i, 2.5
    for j, m in enumerate(marks):
        m[b, 0], m[b, 1] = -3.0 + 0.75 * j, -2.5


def _put(t, b, x, y=0.0):
    t[b, 0], t[b, 1] = float(x), float(y)


def _write(env, pos, marks):
    for a, p in zip(env.agents, pos):
        a.set_pos(p, batch_index=None)
    for m, p in zip(env.world.landmarks, marks):
        m.set_pos(p, batch_index=None)


def place_spread_cases(env):
    """Envs 0 .. 15 by hand (points on the x axis or 3-4-5 triangles: the norms are exact)."""
    pos = [a.state.pos.clone() for a in env.agents]
    marks = [m.state.pos.clone() for m in env.world.landmarks]
    n = len(pos)
    lo, at, hi = around(R_SPREAD)
    for name, (b, need) in SPREAD_CASES.items():
        if b >= pos[0].shape[0]:
            continue
        _far(pos, marks, b)
        if n < need or name == "far":
            continue
        if name == "landmark_far":
            continue
        for m in marks:  # every landmark under agent 0, at the origin: closest = 0
            _put(m, b, 0.0)
        _put(pos[0], b, 0.0)
        if name == "tie":  # agents 0 and 1 at 0.5 on either side of every landmark
            _put(pos[0], b, 0.5), _put(pos[1], b, -0.5)
        if name == "one_pair":
            _put(pos[1], b, 0.25)
        if name == "two_pairs":  # 0-1 and 1-2 overlap, 0-2 does not
            _put(pos[1], b, 0.25), _put(pos[2], b, 0.5)
        if name in ("thr_below", "thr_at", "thr_above"):
            _put(pos[1], b, {"thr_below": lo, "thr_at": at, "thr_above": hi}[name])
        if name == "exact_sum":  # agent i at 0.5 i, landmark l at 0.5 l + 0.25: every closest is 0.25
            for i in range(n):
                _put(pos[i], b, 0.5 * i)
            for j in range(len(marks)):
                _put(marks[j], b, 0.5 * j + 0.25)
        if name == "last_closest":  # the last agent stands on the landmarks, agent 0 at 1.0
            _put(pos[0], b, 1.0), _put(pos[n - 1], b, 0.0)
        if name == "diagonal_pair":  # a 3-4-5 triangle scaled to 0.25: overlapping off the axes
            _put(pos[1], b, 0.15, 0.2)
        if name == "coincident":
            _put(pos[1], b, 0.0)
        if name == "pair_last":
            _put(pos[n - 1], b, 0.0, 0.25)
        if name == "all_on_one":  # agents 0, 1, 2 in one spot: three pairs, six counts
            _put(pos[1], b, 0.0), _put(pos[2], b, 0.0)
        if name == "pair_12":  # agents 1 and 2 overlap far from agent 0
            _put(pos[1], b, 1.0, 1.0), _put(pos[2], b, 1.0, 1.25)
        if name == "touching_apart":  # a 3-4-5 triangle of hypotenuse 0.5: apart
            _put(pos[1], b, 0.3, 0.4)
    _write(env, pos, marks)


def assert_spread_cases_fired(spec: MpeSpec, exp):
    n, nl = len(spec.pos), len(spec.marks)
    rew = exp["scenario"]["rew"].numpy()
    lo, at, hi = around(R_SPREAD)
    assert lo < R_SPREAD == at < hi
    # the three floats around the boundary fall on both sides of it
    sides = [bool(F(F(d - F(0.15)) - F(0.15)) < 0) for d in (lo, at, hi)]
    assert sides == [True, False, False]

    def val(name):
        b, need = SPREAD_CASES[name]
        return rew[b] if n >= need and b < spec.B else None

    def check(name, want):
        got = val(name)
        assert got is None or got == F(want), (name, got, want)

    check("tie", -(n * nl * 0.5))  # (multiples of 0.5: every partial sum is exact)
    assert n < 2 or spec.B < 2 or dist(spec.pos[0][1], spec.marks[0][1]) == dist(spec.pos[1][1], spec.marks[0][1]) == F(0.5)
    check("one_pair", -2)
    check("two_pairs", -4)  # two overlapping pairs, each counted from both sides: 4 x -1 on closest = 0
    check("thr_below", -2), check("thr_at", 0), check("thr_above", 0)
    check("exact_sum", -(n * nl * 0.25))
    check("last_closest", 0)
    check("diagonal_pair", -2), check("coincident", -2), check("pair_last", -2), check("all_on_one", -6)
    check("pair_12", -2), check("touching_apart", 0)
    assert val("far") is not None and val("far") < -1  # (far: no overlap, large distances)
    for k in range(n):
        assert torch.equal(exp["rewards"][k], exp["scenario"]["rew"])
        assert exp["obs"][k].shape == (spec.B, 4 + 2 * nl + (2 * (n - 1) if spec.obs_agents else 0))


def place_tag_cases(env):
    pos = [a.state.pos.clone() for a in env.agents]
    marks = [m.state.pos.clone() for m in env.world.landmarks]
    advs = [i for i, a in enumerate(env.agents) if a.adversary]
    good = [i for i, a in enumerate(env.agents) if not a.adversary]
    lo, at, hi = around(R_TAG)
    for name, (b, need_g, need_a) in TAG_CASES.items():
        if b >= pos[0].shape[0]:
            continue
        _far(pos, marks, b)
        if len(good) < need_g or len(advs) < need_a or name == "far":
            continue
        g0, a0 = good[0], advs[0]
        _put(pos[g0], b, 0.0)
        if name in ("one_catch", "second_good", "both_good", "coincident"):
            _put(pos[a0], b, 0.0 if name == "coincident" else 0.0625)
        if name == "second_good":  # adversary 0 on good agent 1, good agent 0 elsewhere
            _put(pos[good[1]], b, 0.0), _put(pos[g0], b, 1.0, 1.0)
        if name == "both_good":
            _put(pos[good[1]], b, 0.0, 0.0625)
        if name == "two_catch":
            _put(pos[a0], b, 0.0625), _put(pos[advs[1]], b, -0.0625)
        if name == "all_catch":
            for k, a in enumerate(advs):
                _put(pos[a], b, 0.0, 0.015625 * (k + 1))
        if name in ("thr_below", "thr_at", "thr_above"):
            _put(pos[a0], b, {"thr_below": lo, "thr_at": at, "thr_above": hi}[name])
        if name == "shaped_exact":  # adversary k at distance 0.5, 1, 0.25, ... of good agent 0, on the axes
            for k, a in enumerate(advs):
                d = [0.5, 1.0, 0.25, 2.0, 0.75, 1.5, 1.25][k]
                _put(pos[a], b, d if k % 2 == 0 else 0.0, 0.0 if k % 2 == 0 else d)
        if name == "adv_on_adv":
            _put(pos[a0], b, 1.0), _put(pos[advs[1]], b, 1.0, 0.0625)
        if name == "good_on_landmark" and marks:
            _put(marks[0], b, 0.0)
        if name == "last_adv":
            _put(pos[advs[-1]], b, 0.0, -0.0625)
        if name == "diagonal_catch":  # 3-4-5 scaled to 0.1 < 0.125
            _put(pos[a0], b, 0.06, 0.08)
        if name == "diagonal_miss":  # 3-4-5 scaled to 0.15 > 0.125
            _put(pos[a0], b, 0.09, 0.12)
    _write(env, pos, marks)


def assert_tag_cases_fired(spec: MpeSpec, exp):
    n = len(spec.pos)
    advs = [i for i in range(n) if spec.adversary[i]]
    good = [i for i in range(n) if not spec.adversary[i]]
    lo, at, hi = around(R_TAG)
    assert R_TAG == F(0.075 + 0.05) and [bool(d < R_TAG) for d in (lo, at, hi)] == [True, False, False]
    per = [r.numpy() for r in exp["scenario"]["rew"]]
    g0, a0 = good[0], advs[0]
    shaped = spec.shape_agent_rew or spec.shape_adversary_rew

    def env_of(name):
        b, need_g, need_a = TAG_CASES[name]
        return b if len(good) >= need_g and len(advs) >= need_a and b < spec.B else None

    def catches(name, want_good, want_adv0):
        """Unshaped: the exact multiples of 10; shaped: the sign and the size of the catch term."""
        b = env_of(name)
        if b is None:
            return
        if not shaped:
            assert per[g0][b] == F(want_good) and per[a0][b] == F(want_adv0), (name, per[g0][b], per[a0][b])
        else:
            assert abs(per[g0][b] - F(want_good)) < 3 and abs(per[a0][b] - F(want_adv0)) < 3, name

    catches("far", 0, 0), catches("one_catch", -10, 10), catches("coincident", -10, 10)
    catches("two_catch", -20, 10), catches("all_catch", -10 * len(advs), 10)
    catches("thr_below", -10, 10), catches("thr_at", 0, 0), catches("thr_above", 0, 0)
    catches("second_good", 0, 10), catches("both_good", -10, 20)
    catches("adv_on_adv", 0, 0), catches("good_on_landmark", 0, 0)
    catches("diagonal_catch", -10, 10), catches("diagonal_miss", 0, 0)
    b = env_of("last_adv")
    if b is not None and not shaped:
        assert per[advs[-1]][b] == 10 and per[a0][b] == 0 and per[g0][b] == -10
    b = env_of("shaped_exact")
    if b is not None and spec.shape_agent_rew:
        want = F(0)
        for k in range(len(advs)):
            want = F(want + F(F(0.1) * F([0.5, 1.0, 0.25, 2.0, 0.75, 1.5, 1.25][k])))
        assert per[g0][b] == want
    if b is not None and spec.shape_adversary_rew and len(good) == 1:
        assert per[a0][b] == F(F(0) - F(F(0.1) * F(0.5)))
    # the team sums and what a sharing team returns
    for b in range(min(spec.B, N_CASE_ENVS)):
        assert fsum_bound_ok(exp["scenario"]["agents_rew"][b], [per[i][b] for i in good])
        assert fsum_bound_ok(exp["scenario"]["adverary_rew"][b], [per[i][b] for i in advs])
    for k in range(n):
        team = exp["scenario"]["adverary_rew" if spec.adversary[k] else "agents_rew"]
        share = spec.adversaries_share_rew if spec.adversary[k] else spec.agents_share_rew
        assert torch.equal(exp["rewards"][k], team if share else exp["scenario"]["rew"][k])
