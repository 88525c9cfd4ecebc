"""Random-structure world fuzz of the step kernels (tests/_fuzz_world.py) and state-layout edges.

Every seed of ``F.SEEDS`` is one bare World the fixed scenarios do not have (Box / Line agents,
rotatable-not-movable entities, non-colliding entities in the middle of the list, collision
filters, clamps on agents that cannot move, joints between arbitrary shapes, one semidim, 1-5
substeps), at a batch from ``F.BATCHES``, with a contact-seeking random state.  Each is held
against the oracle on the host backend, the world-specialised k_world (relaxed and exact math)
and the generic k_step, at the project's stated tolerance (the defaults of O.compare) with 0
uncertified envs; exact k_world and k_step must be bit-identical.  The distance queries and ray
casts run on the same worlds.  The layout tests hand the engine the same state through strided,
stride-0, 4-byte-aligned and float64 tensors: the step must be bit-identical to the contiguous one
and must write nothing into the tensors it was given.

The measured deviations and the coverage table are recorded in DESIGN.md (c).
"""
import math
from collections import Counter
from types import SimpleNamespace

import pytest
import torch

from oracle import vmas_oracle as O
from tests import _fuzz_world as F
from tests._parity import _RAY_CERT_DELTAS, distance_parity
from tests.test_force_dicts import _check as check_force_dicts
from vectorizedmultiagentsimulator_amd.simulator.core import Agent, Box, Line

CLASSES = ("ss", "ls", "ll", "bs", "bl", "bb")


# ---- non-vacuity ----------------------------------------------------------------------------------
def _coverage(seed):
    """What one seed covers (oracle alone): a set of tags, and (cut-off envs, envs)."""
    w, snap = F.case(seed)
    fz = w._fuzz
    out, ow = O.oracle_step(w, snap)
    # a condition on the inputs: no world of the set overflows in the oracle itself
    assert all(bool(torch.isfinite(v).all()) for d in out.values() for v in d.values()), seed
    tags = {c for sub in ow.active_log for c, _, _ in sub}
    if w._joints:
        tags.add("joint")
        if any(js["dist"] == 0 for js, _ in fz.joints):
            tags.add("joint dist 0")
        if any(js["fixed_rotation_a"] is not None or js["fixed_rotation_b"] is not None for js, _ in fz.joints):
            tags.add("joint fixed rotation")
    ents = w.entities
    for i, e in enumerate(ents):
        if isinstance(e, Agent) and isinstance(e.shape, Box):
            tags.add("Box agent")
        if isinstance(e, Agent) and isinstance(e.shape, Line):
            tags.add("Line agent")
        if e.rotatable and not e.movable:
            tags.add("rotatable, not movable")
        if e.movable and not e.rotatable and isinstance(e.shape, (Box, Line)):
            tags.add("movable, not rotatable Box/Line")
        if not e.collide and 0 < i < len(ents) - 1:
            tags.add("collide=False mid-list")
        if isinstance(e.gravity, torch.Tensor) and e.gravity.dim() == 2:
            tags.add("[B,2] gravity")
        if isinstance(e, Agent) and e.max_f is not None and not e.movable:
            tags.add("max_f, not movable")
        if isinstance(e, Agent) and e.max_t is not None and not e.rotatable:
            tags.add("max_t, not rotatable")
    for i, name in fz.filters.items():
        a, b = fz.ents[i], next(x for x in fz.ents if x.name == name)
        dynamic = a.movable or a.rotatable or b.movable or b.rotatable
        joined = frozenset({a.name, b.name}) in w._joints and w._joints[frozenset({a.name, b.name})].dist == 0
        if a.collide and b.collide and dynamic and not joined and b.collides(a):
            ia, ib = ents.index(a), ents.index(b)
            gap = F._gap(a.shape, snap[ia]["pos"], snap[ia]["rot"], b.shape, snap[ib]["pos"], snap[ib]["rot"])
            if bool((gap < 0).any()):
                tags.add("filter removes a touching pair")
    if (w._x_semidim is None) != (w._y_semidim is None):
        tags.add("one semidim")
    if w._substeps == 1:
        tags.add("substeps 1")
    if w.export_forces:
        tags.add("export_forces")
    return tags, int((ow.cutoff_margin <= O.CUTOFF_TOL).sum()), w.batch_dim


REQUIRED = {**{c: 3 for c in CLASSES}, "joint": 4, "joint dist 0": 1, "joint fixed rotation": 1,
            **{k: 2 for k in (
                "Box agent", "Line agent", "rotatable, not movable", "movable, not rotatable Box/Line",
                "collide=False mid-list", "filter removes a touching pair", "[B,2] gravity",
                "max_f, not movable", "max_t, not rotatable", "one semidim", "substeps 1", "export_forces")}}


def test_fuzz_seed_set_is_not_vacuous():
    assert 24 <= len(F.SEEDS) <= 48
    count, cut, envs = Counter(), 0, 0
    for seed in F.SEEDS:
        tags, c, n = _coverage(seed)
        count.update(tags)
        cut, envs = cut + c, envs + n
    print(f"FUZZ coverage over {len(F.SEEDS)} seeds (seeds that have it / required):")
    for k, need in REQUIRED.items():
        print(f"FUZZ   {k:34s} {count[k]:3d} / {need}")
    print(f"FUZZ   envs on a contact cut-off after the oracle's step: {cut} of {envs} ({100.0 * cut / envs:.2f} %)")
    for k, need in REQUIRED.items():
        assert count[k] >= need, (k, count[k], need)
    assert cut <= 0.02 * envs, (cut, envs)


# ---- step parity ----------------------------------------------------------------------------------
DEVIATION = {}  # target -> field -> largest |engine - oracle| over the seed set (printed per test)


def _note(target, reps):
    d = DEVIATION.setdefault(target, {})
    for r in reps:
        for k, v in r["max_abs"].items():
            d[k] = max(d.get(k, 0.0), v)
    print(f"FUZZ deviation [{target}] so far:", {k: float(f"{v:.3g}") for k, v in d.items()})


def _two_steps(w, target, **kw):
    reps = []
    for _ in range(2):
        rep = O.compare_one_step(w, broadphase="batch", **kw)
        print(f"FUZZ [{target}] seed {w._fuzz.seed} B {w.batch_dim}: bad {rep['bad_envs']} certified "
              f"{rep['certified_envs']} uncertified {rep['uncertified_envs']} max_abs {rep['max_abs']}")
        assert rep["ok"] and rep["uncertified_envs"] == 0, rep
        reps.append(rep)
    _note(target, reps)
    return reps


def _forces(w):
    """World.forces_dict / torques_dict against the oracle's last-substep totals, when the world
    exports them and some entity can receive a force."""
    if w.export_forces and any(e.movable or e.rotatable for e in w.entities):
        check_force_dicts(w, steps=1)


@pytest.mark.parametrize("seed", F.SEEDS)
def test_fuzz_host(seed):
    w, _ = F.case(seed)
    reps = _two_steps(w, "host")
    rep = O.compare_one_step(w, broadphase="env")
    assert rep["ok"] and rep["uncertified_envs"] == 0, rep
    _note("host", reps + [rep])
    w.broadphase = "batch"
    _forces(w)


@pytest.mark.parametrize("seed", F.SEEDS)
def test_fuzz_world_kernel_compiles(seed):
    w, _ = F.case(seed)
    src = w.engine.jit_compile_check()
    assert "k_world" in src


@pytest.mark.gpu
@pytest.mark.parametrize("seed", F.SEEDS)
def test_fuzz_relaxed_gpu(gpu_device, monkeypatch, seed):
    monkeypatch.delenv("VMAS_JIT", raising=False)
    monkeypatch.delenv("VMAS_JIT_MATH", raising=False)
    w, _ = F.case(seed, gpu_device)
    _two_steps(w, "k_world relaxed")
    assert w.engine.kernel_name == "k_world", w.engine.jit_error
    # (a world with joints compiles in exact math whatever the mode: csrc/vmas_jit.hip relaxed_math)
    assert ("VMAS_PHYS_RELAXED" in w.engine.jit_source()) == (not w._joints)
    _forces(w)
    assert w.engine.kernel_name == "k_world"


def _assert_same(a, b, what):
    for i in a:
        for k in a[i]:
            assert torch.equal(a[i][k], b[i][k]), (what, i, k, float((a[i][k] - b[i][k]).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", F.SEEDS)
def test_fuzz_exact_and_generic_gpu(gpu_device, monkeypatch, seed):
    monkeypatch.delenv("VMAS_JIT", raising=False)
    monkeypatch.setenv("VMAS_JIT_MATH", "exact")
    w, snap = F.case(seed, gpu_device)
    # strict parity: no certification on the envs the oracle does not put on a cut-off
    expected, ow = O.oracle_step(w, snap)
    band = O.sensitivity_band(w, snap, expected)
    w.step()
    assert w.engine.kernel_name == "k_world", w.engine.jit_error
    assert "VMAS_PHYS_RELAXED" not in w.engine.jit_source()
    got = O.snapshot(w)
    on_cut = ow.cutoff_margin <= O.CUTOFF_TOL
    pick = lambda d, m: {i: {k: v[m] for k, v in f.items()} for i, f in d.items()}  # noqa: E731
    for mask, certify in ((~on_cut, False), (on_cut, True)):
        if not bool(mask.any()):
            continue
        rep = O.compare(pick(got, mask), pick(expected, mask), w, band=pick(band, mask),
                        cutoff=ow.cutoff_margin[mask] if certify else None)
        if rep["uncertified_envs"]:
            more = O.sensitivity_band(w, snap, expected, n=O.BAND_RETRY_N, seed=98765)
            wide = {i: {k: torch.maximum(band[i][k], more[i][k]) for k in band[i]} for i in band}
            rep = O.compare(pick(got, mask), pick(expected, mask), w, band=pick(wide, mask),
                            cutoff=ow.cutoff_margin[mask] if certify else None)
        print(f"FUZZ [k_world exact] seed {seed} certify {certify}: envs {rep['n_envs']} bad {rep['bad_envs']} "
              f"max_abs {rep['max_abs']}")
        assert rep["ok"] and rep["uncertified_envs"] == 0, (certify, rep)
        _note("k_world exact", [rep])
    # the generic kernel on the same snapshot: bit-identical, in both broadphase modes
    monkeypatch.setenv("VMAS_JIT", "0")
    ref, _ = F.case(seed, gpu_device)
    for bp in ("batch", "env"):
        F.install(w, snap)
        F.install(ref, snap)
        w.broadphase = ref.broadphase = bp
        w.step()
        ref.step()
        assert w.engine.kernel_name == "k_world" and ref.engine.kernel_name == "k_step"
        _assert_same(O.snapshot(w), O.snapshot(ref), bp)
        if w.export_forces:
            for x, y in zip(w.entities, ref.entities):
                assert torch.equal(w.forces_dict[x], ref.forces_dict[y]), (bp, x.name)
                assert torch.equal(w.torques_dict[x], ref.torques_dict[y]), (bp, x.name)


# ---- queries --------------------------------------------------------------------------------------
def _queries(w, snap, target, atol=2e-5, rtol=2e-5):
    rep = distance_parity(SimpleNamespace(world=w))
    print(f"FUZZ [{target}] seed {w._fuzz.seed} distance: {rep}")
    assert rep["ok"], rep
    ow = O.OracleWorld(w, snap)
    base = torch.linspace(0, 2 * math.pi, 17)[:16]
    worst = n_unc = n_rows = 0
    for agent in w.agents:
        if not agent.collide:
            continue
        # every entity the reference lets a ray be cast at ("Rays are only casted among collidables")
        filt = lambda e, a=agent: e.collides(a) and a.collides(e)  # noqa: E731
        ai = w.entities.index(agent)
        angles = base.unsqueeze(0) + snap[ai]["rot"]
        got = w.cast_rays(agent, angles.to(w.device), 0.5, filt).detach().cpu()
        exp = ow.cast_rays(ai, angles, 0.5, filt)
        diff = (got - exp).abs()
        bad = diff > atol + rtol * exp.abs()
        worst = max(worst, float(diff.max()))
        if bad.any():
            cert = torch.zeros_like(bad)
            for d in _RAY_CERT_DELTAS:
                e2 = ow.cast_rays(ai, angles + d, 0.5, filt)
                cert |= (got - e2).abs() <= atol + rtol * e2.abs()
            n_unc += int((bad & ~cert).any(-1).sum())
        n_rows += got.shape[0]
    print(f"FUZZ [{target}] seed {w._fuzz.seed} rays: rows {n_rows} max_abs {worst:.3g} uncertified {n_unc}")
    assert n_unc == 0


@pytest.mark.parametrize("seed", F.SEEDS)
def test_fuzz_queries_host(seed):
    w, snap = F.case(seed)
    _queries(w, snap, "host")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", F.SEEDS)
def test_fuzz_queries_gpu(gpu_device, seed):
    w, snap = F.case(seed, gpu_device)
    _queries(w, snap, "gpu")


# ---- state-layout edges ---------------------------------------------------------------------------
def _layout_seeds():
    """The first 7 seeds plus the first later seed with a joint (or 8 when one of them has one)."""
    has_joint = lambda s: bool(F.build(s, 1, "cpu")._joints)  # noqa: E731  (the structure alone: cheap)
    seeds = list(F.SEEDS[:8])
    if not any(has_joint(s) for s in seeds):
        seeds[-1] = next(s for s in F.SEEDS[8:] if has_joint(s))
    return seeds


LAYOUT_SEEDS = _layout_seeds()
SENTINEL = -12345.0


def _present(w, snap):
    """Assign every state tensor of ``w`` as a non-contiguous / widened view holding ``snap``'s
    values.  Returns [(buffer, its clone at assignment)] of everything the engine was handed."""
    dev, B = w.device, w.batch_dim
    held = []

    def wide(v, cols, at):
        buf = torch.full((B, cols), SENTINEL, device=dev)
        buf[:, at:at + v.shape[1]] = v.to(dev)
        held.append(buf)
        return buf[:, at:at + v.shape[1]]

    static = next((i for i, e in enumerate(w.entities) if not e.movable), None)
    f64 = next((i for i, e in enumerate(w.entities) if e.movable), None)
    for i, e in enumerate(w.entities):
        s, st = snap[i], e.state
        if i == f64:  # one movable entity's whole state in float64
            for k, v in s.items():
                setattr(st, k, v.to(dev, torch.float64))
                held.append(getattr(st, k))
            continue
        if i == static:  # stride 0: one row for every env
            row = s["pos"][:1].to(dev).clone()
            held.append(row)
            st.pos = row.expand(B, 2)
        else:  # columns 1:3 of [B, 5]: stride (5, 1), 4-byte aligned
            st.pos = wide(s["pos"], 5, 1)
        vt = s["vel"].to(dev).t().contiguous()  # [2, B].t(): stride (1, B)
        held.append(vt)
        st.vel = vt.t()
        st.rot = wide(s["rot"], 3, 2)  # column 2 of [B, 3]
        st.ang_vel = wide(s["ang_vel"], 3, 2)
        if "force" in s:
            st.force = wide(s["force"], 5, 1)
            st.torque = wide(s["torque"], 3, 2)
        if B > 1:  # (the strides of a size-1 dimension are arbitrary)
            assert st.pos.stride(0) in (0, 5) and st.vel.stride() == (1, B) and st.rot.stride(0) == 3
    return [(b, b.clone()) for b in held]


def _layout(seed, device, kernel):
    w, snap = F.case(seed, device)
    snap = {i: dict(d) for i, d in snap.items()}
    static = next((i for i, e in enumerate(w.entities) if not e.movable), None)
    if static is not None:  # the stride-0 form needs the same position in every env
        snap[static]["pos"] = snap[static]["pos"][:1].repeat(w.batch_dim, 1)
    F.install(w, snap)
    w.step()  # whatever the engine folds at build time is folded now
    assert kernel is None or w.engine.kernel_name == kernel
    F.install(w, snap)
    w.step()
    want = O.snapshot(w)
    F.install(w, snap)
    held = _present(w, snap)
    assigned = [(e, {k: getattr(e.state, k) for k in snap[i]}) for i, e in enumerate(w.entities)]
    w.step()
    _assert_same(O.snapshot(w), want, ("layout", seed))
    for buf, before in held:  # padding keeps its sentinel, the assigned values are untouched
        assert torch.equal(buf, before)
    for e, fields in assigned:  # fresh tensors after the step (eager mode): none of ours
        for k, t in fields.items():
            if (k in ("pos", "vel") and e.movable) or (k in ("rot", "ang_vel") and e.rotatable):
                assert getattr(e.state, k) is not t, (e.name, k)


@pytest.mark.parametrize("seed", LAYOUT_SEEDS)
def test_layout_host(seed):
    _layout(seed, "cpu", None)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["relaxed", "exact", "generic"])
@pytest.mark.parametrize("seed", LAYOUT_SEEDS)
def test_layout_gpu(gpu_device, monkeypatch, seed, mode):
    if mode == "generic":
        monkeypatch.setenv("VMAS_JIT", "0")
        monkeypatch.delenv("VMAS_JIT_MATH", raising=False)
    else:
        monkeypatch.delenv("VMAS_JIT", raising=False)
        monkeypatch.setenv("VMAS_JIT_MATH", mode)
    _layout(seed, gpu_device, "k_step" if mode == "generic" else "k_world")
