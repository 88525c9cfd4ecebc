"""The dispersion scenario's per-step values, restated on plain CPU tensors (the yardstick of
tests/test_wheel_dispersion*.py; written from the scenario's description, never importing it).

For env b, agents a, foods l in world.landmarks order:  on[a, l] = |a.pos - l.pos| < thr (strict), thr =
f32(double(a.radius) + double(l.radius)).  The first agent's reward call counts how_many_on_food[l] (int64),
anyone_on_food = how_many > 0 and ORs it into just_eaten.  An agent's reward starts at fp32 0 and adds,
in food order, 1 per food with just_eaten & ~eaten (share_reward) or fp32 1 / how_many per food with
on[a, l] & ~eaten[l]; a reward that is exactly 0 becomes f32(-0.01) with penalise_by_time.  After the
last agent's reward eaten |= just_eaten, just_eaten = False, is_rendering &= ~eaten.  Every observation is
taken after every reward: a.pos, a.vel, per food l.pos - a.pos and eaten as 0.0 / 1.0.  done = all
foods eaten.  A per-env, per-agent Python loop over numpy float32 scalars, one rounding per operation."""
import numpy as np
import torch

F = np.float32


class DispersionSpec:
    def __init__(self, env):
        scn, w = env.scenario, env.world
        cpu = lambda t: t.detach().cpu().clone()  # noqa: E731
        self.B = w.batch_dim
        self.share_reward, self.penalise_by_time = bool(scn.share_reward), bool(scn.penalise_by_time)
        self.pos = [cpu(a.state.pos) for a in w.agents]
        self.vel = [cpu(a.state.vel) for a in w.agents]
        self.food = [cpu(f.state.pos) for f in w.landmarks]
        self.eaten = [cpu(f.eaten) for f in w.landmarks]
        self.just_eaten = [cpu(f.just_eaten) for f in w.landmarks]
        self.is_rendering = [cpu(f.is_rendering) for f in w.landmarks]
        self.thr = [[F(a.shape.radius + f.shape.radius) for f in w.landmarks] for a in w.agents]

    def on(self, b, a, l):  # noqa: E741
        dx, dy = (self.pos[a][b] - self.food[l][b]).numpy()
        return bool(np.sqrt(F(F(dx * dx) + F(dy * dy))) < self.thr[a][l])

    def run(self):
        """One step's program, updating the spec's flags in place; returns its outputs."""
        B, n, nf = self.B, len(self.pos), len(self.food)
        how_many = [torch.zeros(B, dtype=torch.int64) for _ in range(nf)]
        rewards = [np.zeros(B, dtype=F) for _ in range(n)]
        obs = [np.zeros((B, 4 + 3 * nf), dtype=F) for _ in range(n)]
        done = torch.zeros(B, dtype=torch.bool)
        eaten_before = [e.clone() for e in self.eaten]
        for b in range(B):
            on = [[self.on(b, a, l) for l in range(nf)] for a in range(n)]  # noqa: E741
            for l in range(nf):  # noqa: E741
                how_many[l][b] = sum(on[a][l] for a in range(n))
                if how_many[l][b] > 0:
                    self.just_eaten[l][b] = True
            for a in range(n):
                r = F(0)
                for l in range(nf):  # noqa: E741
                    if self.eaten[l][b]:
                        continue
                    if self.share_reward:
                        if self.just_eaten[l][b]:
                            r = F(r + F(1))
                    elif on[a][l]:
                        r = F(r + F(F(1) / F(int(how_many[l][b]))))
                if self.penalise_by_time and r == 0:
                    r = F(-0.01)
                rewards[a][b] = r
            for l in range(nf):  # noqa: E741
                self.eaten[l][b] = bool(self.eaten[l][b]) or bool(self.just_eaten[l][b])
                self.just_eaten[l][b] = False
                if self.eaten[l][b]:
                    self.is_rendering[l][b] = False
            done[b] = all(bool(e[b]) for e in self.eaten)
            for a in range(n):
                px, py = self.pos[a][b].numpy()
                row = [px, py, *self.vel[a][b].numpy()]
                for l in range(nf):  # noqa: E741
                    fx, fy = self.food[l][b].numpy()
                    row += [F(fx - px), F(fy - py), F(1) if self.eaten[l][b] else F(0)]
                obs[a][b] = row
        return {"how_many": how_many, "anyone": [h > 0 for h in how_many], "done": done, "on_eaten_before": eaten_before,
                "rewards": [torch.from_numpy(r) for r in rewards], "obs": [torch.from_numpy(o) for o in obs]}


def landmark_attributes(env):
    out = []
    for f in env.world.landmarks:
        out += [f.eaten, f.just_eaten, f.is_rendering, f.how_many_on_food, f.anyone_on_food]
    return out


# ---- hand-placed cases -------------------------------------------------------------------------------
# name -> the env in which it must fire; (min agents, min foods) it needs
CASE_ENVS = {
    "nobody": 0,            # nobody on food: reward 0 (-0.01 with penalise_by_time)
    "one_on_one": 1,        # agent 0 alone on food 0: reward 1, eaten, obs flag 1, not rendered
    "two_on_one": 2,        # agents 0, 1 on food 0: 1/2 each
    "three_on_one": 3,      # agents 0, 1, 2 on food 0: fp32 1/3 each
    # agent 0 on foods 0, 1, 2 shared with 2, 3 and 3 agents: (1/2 + 1/3) + 1/3 in fp32, three roundings.
    # (For these three terms every order of the additions rounds to the same float, 1.1666667: the case
    # pins the value and the counts, not the order.)
    "three_foods": 4,
    "on_eaten": 5,          # agent 0 on food 0 eaten before: no reward (shared or not), counted, stays eaten
    "eats_other_zero": 6,   # agent 0 eats food 0, agent 1 far away gets exactly 0 (non-shared)
    "two_new": 7,           # agent 0 on food 0, agent 1 on food 1: shared reward 2 for everybody
    "all_eaten": 8,         # every food but food 0 eaten before, agent 0 on food 0: done
    "all_but_one": 9,       # every food but food 0 eaten before, nobody on it: not done
    "exactly_thr": 10,      # agent 0 at distance exactly thr of food 0: NOT on food (strict <)
    "just_inside": 11,      # agent 0 at nextafter(thr, 0): on food
}
NEEDS = {"two_on_one": (2, 1), "three_on_one": (3, 1), "three_foods": (3, 3), "eats_other_zero": (2, 1), "two_new": (2, 2)}
N_CASE_ENVS = 12


def active(name, n, nf):
    need = NEEDS.get(name, (1, 1))
    return n >= need[0] and nf >= need[1]


def place_cases(env):
    """Overwrite positions and flags by hand in envs 0 .. 11 (foods at the origin or on the x axis: the
    norms are exact).  Agents and foods a case does not name stand far from everything."""
    w = env.world
    agents, foods = w.agents, w.landmarks
    n, nf = len(agents), len(foods)
    thr = float(F(agents[0].shape.radius + foods[0].shape.radius))
    pos = [a.state.pos.clone() for a in agents]
    fpos = [f.state.pos.clone() for f in foods]
    eaten = [f.eaten.clone() for f in foods]
    for b in range(N_CASE_ENVS):
        for a in range(n):
            pos[a][b, 0], pos[a][b, 1] = -0.5, -0.9 + 0.1 * a
        for l in range(nf):  # noqa: E741
            fpos[l][b, 0], fpos[l][b, 1] = 0.6, -0.9 + 0.1 * l
            eaten[l][b] = False

    def put(t, b, x, y=0.0):
        t[b, 0], t[b, 1] = x, y

    for name, b in CASE_ENVS.items():
        if not active(name, n, nf) or name == "nobody":
            continue
        put(fpos[0], b, 0.0)
        if name in ("one_on_one", "on_eaten", "eats_other_zero", "all_eaten"):
            put(pos[0], b, 0.0)
        if name in ("two_on_one", "three_on_one"):
            for a in range(2 if name == "two_on_one" else 3):
                put(pos[a], b, 0.0)
        if name == "three_foods":  # food 0 at 0, foods 1 and 2 at 0.08; agents at 0.04, 0.08, 0.12
            put(fpos[1], b, 0.08), put(fpos[2], b, 0.08)
            put(pos[0], b, 0.04), put(pos[1], b, 0.08), put(pos[2], b, 0.12)
        if name == "on_eaten":
            eaten[0][b] = True
        if name == "two_new":
            put(fpos[1], b, 0.5), put(pos[0], b, 0.0), put(pos[1], b, 0.5)
        if name in ("all_eaten", "all_but_one"):
            for l in range(1, nf):  # noqa: E741
                eaten[l][b] = True
        if name == "exactly_thr":
            put(pos[0], b, thr)
        if name == "just_inside":
            put(pos[0], b, float(np.nextafter(F(thr), F(0))))
    for a, p in zip(agents, pos):
        a.set_pos(p, batch_index=None)
    for f, p, e in zip(foods, fpos, eaten):
        f.set_pos(p, batch_index=None)
        f.eaten.copy_(e)  # (in place, as the scenario writes it)
        f.just_eaten.fill_(False)
        shown = f.is_rendering.clone()
        shown[:N_CASE_ENVS] = ~e[:N_CASE_ENVS]
        f.is_rendering.copy_(shown)


def assert_cases_fired(spec: DispersionSpec, exp):
    """On the spec's own outputs (``exp = spec.run()`` right after place_cases): the known answers."""
    n, nf = len(spec.pos), len(spec.food)
    share, zero = spec.share_reward, F(-0.01) if spec.penalise_by_time else F(0)
    rew = [r.numpy() for r in exp["rewards"]]
    third = F(F(1) / F(3))

    def env(name):
        return CASE_ENVS[name]

    def fired(name):
        return active(name, n, nf)

    b = env("nobody")
    assert all(r[b] == zero for r in rew) and not any(h[b] for h in exp["how_many"]) and not spec.eaten[0][b]
    b = env("one_on_one")
    assert rew[0][b] == 1 and exp["how_many"][0][b] == 1 and spec.eaten[0][b] and not spec.is_rendering[0][b]
    assert exp["obs"][0][b, 6] == 1 and not spec.just_eaten[0][b]
    if fired("two_on_one"):
        b = env("two_on_one")
        assert exp["how_many"][0][b] == 2 and rew[0][b] == rew[1][b] == (F(1) if share else F(0.5))
    if fired("three_on_one"):
        b = env("three_on_one")
        assert exp["how_many"][0][b] == 3 and rew[0][b] == rew[1][b] == rew[2][b] == (F(1) if share else third)
    if fired("three_foods"):
        b = env("three_foods")
        assert [int(exp["how_many"][l][b]) for l in range(3)] == [2, 3, 3]
        if not share:
            assert rew[0][b] == F(F(F(0.5) + third) + third)  # in food order
            assert rew[2][b] == F(third + third)
    b = env("on_eaten")
    assert exp["on_eaten_before"][0][b] and exp["how_many"][0][b] == 1 and spec.eaten[0][b]
    assert all(r[b] == zero for r in rew)  # (shared reward on an eaten food: 0 too)
    if fired("eats_other_zero") and not share:
        b = env("eats_other_zero")
        assert rew[0][b] == 1 and rew[1][b] == zero
    if fired("two_new"):
        b = env("two_new")
        assert all(r[b] == (2 if share else (1 if a < 2 else zero)) for a, r in enumerate(rew))
    assert exp["done"][env("all_eaten")] and not exp["done"][env("all_but_one")]
    b = env("exactly_thr")
    assert exp["how_many"][0][b] == 0 and rew[0][b] == zero and not spec.eaten[0][b]
    b = env("just_inside")
    assert exp["how_many"][0][b] == 1 and rew[0][b] == 1 and spec.eaten[0][b]
