"""Shared helpers of the analytic known-answer tests (test_oracle_kat.py, test_kat_queries.py).

Every expected value of a KAT is computed in the test, in float64 Python ``math``, from geometry
written out in the test; neither the oracle nor the package produces one.  Each case is then held
against the oracle AND the native engine on four targets:
  * ``cpu``: the library's host backend, one env;
  * ``gpu-relaxed``: the gfx950 world kernel k_world in its default relaxed fp32 math (hardware
    rcp / sqrt / exp / log / sin / cos -- the kernel bench.py times);
  * ``gpu-exact``: the same with VMAS_JIT_MATH=exact (IEEE div / sqrt, ocml transcendentals);
  * ``gpu-generic``: VMAS_JIT=0, the generic k_step every world falls back to when the
    world-specialised kernel does not apply.
The GPU targets replicate the case over 70 envs: one full wavefront plus a partial one; every env
must give the closed-form answer.

Tolerance of the step cases (``tol``): one rule,

    |d vel| <= (dt / m) * c * 16 * eps32 * L  +  4 * eps32 * |vel|

A contact (or joint) force's slope in the distance is at most ``c`` (``joint_force`` for a joint),
and the distance carries a few ulp of ``L``, the larger of the distance and dist_min that the
case's constraint compares (each case states its L).  16 ulp is what the sphere-sphere KAT's
rel=1e-5 amounts to (L = 0.1, F ~ 1).  ``ang_vel`` gets the same rule with lever / I in place of
1 / m, and ``pos`` / ``rot`` get the rule x dt.  Cases without a contact have L = 0: only the
4-ulp term is left.  The deviations measured on every target are tabulated in DESIGN.md (c).
"""
import math
from dataclasses import dataclass

import pytest
import torch

from oracle import vmas_oracle as O
from vectorizedmultiagentsimulator_amd.simulator.core import Agent, World

K = 1e-3  # contact_margin
DT = 0.1
C = 100.0  # collision_force
LMD = 4 / 600  # LINE_MIN_DIST
EPS32 = 2.0**-23
GPU_BATCH = 70  # one full wavefront + a partial one


@dataclass
class Target:
    device: str
    batch: int
    math: str | None
    name: str = "cpu"


TARGETS = [
    pytest.param(("cpu", 1, None), id="cpu"),
    pytest.param(("cuda", GPU_BATCH, "relaxed"), id="gpu-relaxed", marks=pytest.mark.gpu),
    pytest.param(("cuda", GPU_BATCH, "exact"), id="gpu-exact", marks=pytest.mark.gpu),
    pytest.param(("cuda", GPU_BATCH, "generic"), id="gpu-generic", marks=pytest.mark.gpu),
]


@pytest.fixture(params=TARGETS)
def tgt(request, monkeypatch):
    dev, batch, mode = request.param
    if dev == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no ROCm GPU visible")
        # both are read when the engine builds its kernels for a world
        if mode == "generic":
            monkeypatch.setenv("VMAS_JIT", "0")
            monkeypatch.delenv("VMAS_JIT_MATH", raising=False)
        else:
            monkeypatch.delenv("VMAS_JIT", raising=False)
            monkeypatch.setenv("VMAS_JIT_MATH", mode)
        dev = "cuda:0"
    return Target(dev, batch, mode, f"gpu-{mode}" if mode else "cpu")


def softplus_pen(x):
    return K * (max(0.0, x / K) + math.log1p(math.exp(-abs(x / K))))


pen = softplus_pen


def world_with(*entities, tgt=None, **kw):
    tgt = tgt or Target("cpu", 1, None)
    w = World(tgt.batch, tgt.device, **kw)
    for e in entities:
        (w.add_agent if isinstance(e, Agent) else w.add_landmark)(e)
    w._kat_target = tgt
    return w


def set_state(e, pos, vel=(0.0, 0.0), rot=0.0, ang=0.0, tgt=None):
    tgt = tgt or Target("cpu", 1, None)
    rep = lambda v: torch.tensor([v] * tgt.batch, dtype=torch.float32, device=tgt.device)  # noqa: E731
    e.state.pos = rep(pos)
    e.state.vel = rep(vel)
    e.state.rot = rep([rot])
    e.state.ang_vel = rep([ang])


def assert_kernel(w):
    """The engine of a GPU target runs the kernel the target names."""
    t = w._kat_target
    if t.device == "cpu":
        return
    if t.math == "generic":
        assert w.engine.kernel_name == "k_step", "gpu-generic KATs run the generic step kernel"
    else:
        assert w.engine.kernel_name == "k_world", "GPU KATs run the world-specialised kernel"
        # (a world with joints compiles in exact math whatever the mode: csrc/vmas_jit.hip relaxed_math)
        assert ("VMAS_PHYS_RELAXED" in w.engine.jit_source()) == (t.math == "relaxed" and not w._joints)


def step_both(w):
    """(oracle result, engine result) of one step from the current state (CPU tensors)."""
    expected, _ = O.oracle_step(w)
    w.step()
    assert_kernel(w)
    return expected, O.snapshot(w)


def allclose(t, value, rel=0.0, abs_=0.0):
    """Every env of a [B, k] result equals the closed-form value (pytest.approx semantics)."""
    t = t.detach().cpu().reshape(t.shape[0], -1)
    want = torch.tensor(value, dtype=torch.float64).reshape(1, -1)
    err = (t.double() - want).abs()
    return bool((err <= torch.maximum(rel * want.abs(), torch.tensor(abs_, dtype=torch.float64))).all())


def tol(L=0.0, mag=0.0, inv_m=1.0, c=C, dt=DT):
    """The step cases' tolerance rule (module docstring) for a velocity of magnitude ``mag``;
    ``inv_m`` is 1 / m for ``vel`` and lever / I for ``ang_vel``.  x DT for ``pos`` / ``rot``."""
    return dt * inv_m * c * 16 * EPS32 * L + 4 * EPS32 * abs(mag)


def deviation(t, want):
    """Largest |t - want| over every env and component; ``want`` is [k] (every env the same) or
    [B, k] (one closed-form row per env)."""
    t = t.detach().cpu().reshape(t.shape[0], -1).double()
    want = torch.tensor(want, dtype=torch.float64)
    want = want.reshape(1, -1) if want.dim() < 2 else want
    assert want.shape[0] in (1, t.shape[0]) and want.shape[1] == t.shape[1], (t.shape, want.shape)
    assert torch.isfinite(t).all()
    return float((t - want).abs().max())


def expect(w, results, ent, field, want, tolerance, label="", cols=None):
    """``field`` of entity index ``ent`` equals the closed-form ``want`` within ``tolerance`` in
    every env, in the oracle's result and in the engine's (``results`` = step_both's pair).  The
    oracle additionally stays within rel 1e-4 of the closed form's magnitude.  Prints each
    deviation before it asserts (the measurements of DESIGN.md (c))."""
    mag = max((abs(x) for row in ([want] if not isinstance(want[0], (list, tuple)) else want) for x in row),
              default=0.0)
    for who, res in zip(("oracle", "engine"), results):
        t = res[ent][field]
        t = t if cols is None else t[:, cols]
        dev = deviation(t, want)
        name = "oracle" if who == "oracle" else w._kat_target.name
        print(f"KAT {label or field} [{name}] {field}: |dev| {dev:.3g} (rel {dev / mag if mag else 0.0:.3g}) "
              f"tol {tolerance:.3g}")
        assert dev <= tolerance, (label, who, field, dev, tolerance)
        if who == "oracle" and mag:
            assert dev <= 1e-4 * mag, (label, field, dev)


def distinguishes(want, wrong, tolerance):
    """Non-vacuity: a plausible wrong answer lies more than 50 tolerances from the right one."""
    gap = max(abs(a - b) for a, b in zip(want, wrong))
    assert gap > 50 * tolerance, (want, wrong, tolerance)
