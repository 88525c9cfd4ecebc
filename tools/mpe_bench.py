#!/usr/bin/env python3
"""Step and reset times of MPE simple_spread and simple_tag on one MI355X (bench.py measures the balance
flagship and has no switch for them), at 32 768 envs with the default kwargs, and the reference's
published VMAS-against-MPE protocol for simple_spread.

Step: ``env.step(actions)`` on a fixed list of pre-drawn random actions, HIP events around the timed steps:

  a  default make_env (graph mode, the native program k_mpe)
  b  graph_step=False, the native program
  c  the torch program (VMAS_FUSED_SCENARIOS off), eager
  d  what a user had before the scenarios shipped: this tree's Scenario class, its native path off,
     handed as a user scenario to the make_env of another tree (--package-root: a built checkout of
     the commit before), default graph_step

Reset (configuration r, this tree): ``reset()``, and ``reset_where`` at 1 %, 10 % and 100 % of the envs
through the native launch (k_uniform_reset) and through the generic path.

Published protocol (configuration p, simple_spread only): 30 000 envs, ``reset()``, then 100 steps with
``continuous_actions=False``, every agent's action a fresh [B, 1] tensor of 2s built inside the loop as
the reference's harness builds it; wall clock with one device synchronise before the clock stops.  The
loop runs twice in the process: the first pass, as published, holds the graph capture and every kernel's
first launch; the second is the same loop warm.  The two published figures are printed beside it as
context, not as a ratio: the hardware differs and the reference's clock stops without a synchronise.

Every (configuration, scenario) run is a child process of its own under its own timeout, the
configurations alternate, and the whole list is gone through --repeats times.  Prints one JSON line per
run and a closing summary line with the range of every configuration.

    python tools/mpe_bench.py [--configs abcrp] [--package-root DIR] [--repeats 3] [--out FILE]
    python tools/mpe_bench.py --one a --scenario simple_tag        (one run, in this process)
"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "vectorizedmultiagentsimulator_amd"
PUBLISHED = {"protocol": "simple_spread, 30 000 envs, 100 steps, discrete actions (BASELINE.md section 1)",
             "vmas_rtx_2080_ti_s": 10.15, "vmas_xeon_6248r_s": 193.12,
             "note": "context only: other hardware, and a clock that stops without a device synchronise"}


def _timed(torch, fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3  # ms per call, host wall clock to device idle


def run_resets(args, vmas, torch) -> dict:
    env = vmas.make_env(args.scenario, num_envs=args.envs, device=args.device, seed=0)
    scn = env.scenario
    for _ in range(3):
        env.step(env.get_random_actions())
    env.reset()
    rec = {"config": "r", "scenario": args.scenario, "envs": args.envs, "fused_status": scn.fused_status}
    rec["reset_ms"] = round(_timed(torch, env.reset, 10), 3)
    native = type(scn).reset_world_where
    for frac, name in ((0.01, "1pct"), (0.1, "10pct"), (1.0, "100pct")):
        mask = torch.zeros(args.envs, dtype=torch.bool, device=args.device)
        mask[: max(1, int(args.envs * frac))] = True
        n0 = scn.native_resets
        env.reset_where(mask)
        rec[f"reset_where_{name}_ms"] = round(_timed(torch, lambda: env.reset_where(mask), 10), 3)
        rec[f"native_calls_{name}"] = scn.native_resets - n0
        type(scn).reset_world_where = lambda self, mask: NotImplemented  # the generic path
        try:
            env.reset_where(mask)
            rec[f"reset_where_generic_{name}_ms"] = round(_timed(torch, lambda: env.reset_where(mask), 5), 3)
        finally:
            type(scn).reset_world_where = native
    env.step(env.get_random_actions())
    rec["graph_status"] = getattr(env, "graph_status", "off")
    return rec


def run_published(args, vmas, torch) -> dict:
    B, steps = 30000, 100
    env = vmas.make_env("simple_spread", num_envs=B, device=args.device, seed=0, continuous_actions=False)
    n_agents = len(env.agents)

    def protocol():
        env.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            # (the harness's own expression: a one-element tensor made on the device from a Python list,
            # repeated over the envs -- a small host-to-device copy per agent and step included)
            actions = [torch.tensor([2], device=args.device).repeat(B, 1) for _ in range(n_agents)]
            env.step(actions)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    # the protocol as published has no warm-up: the first pass holds the graph capture and every kernel's
    # first launch; the second pass is the same loop on the warm process
    first, second = protocol(), protocol()
    return {"config": "p", "scenario": "simple_spread", "envs": B, "steps": steps,
            "first_pass_wall_s": round(first, 4), "second_pass_wall_s": round(second, 4),
            "first_pass_env_steps_per_s": round(B * steps / first), "second_pass_env_steps_per_s": round(B * steps / second),
            "graph_status": getattr(env, "graph_status", "off"), "fused_status": env.scenario.fused_status,
            "published_for_context": PUBLISHED}


# include/vmas_mi355x.h's names for the family, for a package built before they existed (configuration d)
MPE_CONSTANTS = dict(VMAS_MPE_MAX_AGENTS=8, VMAS_MPE_MAX_LANDMARKS=8, VMAS_MPE_MAX_TERMS=24, VMAS_MPE_SPREAD=1,
                     VMAS_MPE_TAG=2, VMAS_MPE_SELF_VEL=0, VMAS_MPE_SELF_POS=1, VMAS_MPE_REL_LANDMARK=2,
                     VMAS_MPE_REL_AGENT=3, VMAS_MPE_AGENT_VEL=4)


def _user_scenario(name, vmas):
    """This tree's Scenario class for another tree's package: its file and the family's host module
    loaded by path, the family's constants lent to that package's binding module (its native path is
    off: they only have to exist)."""
    native = sys.modules[vmas.__name__ + "._native"]
    for k, v in MPE_CONSTANTS.items():
        if not hasattr(native, k):
            setattr(native, k, v)
    helper = vmas.__name__ + ".simulator._mpe"
    if helper not in sys.modules:
        spec = importlib.util.spec_from_file_location(helper, PKG / "simulator" / "_mpe.py")
        mod = importlib.util.module_from_spec(spec)
        sys.modules[helper] = mod
        spec.loader.exec_module(mod)
    spec = importlib.util.spec_from_file_location(f"user_{name}", PKG / "scenarios" / "mpe" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Scenario()


def run_one(args) -> dict:
    cfg = args.one
    if cfg in ("c", "d"):
        os.environ["VMAS_FUSED_SCENARIOS"] = "0"  # (read when the package is imported)
    pkg_root = Path(args.package_root).resolve() if cfg == "d" else ROOT
    sys.path.insert(0, str(pkg_root))
    import torch

    import vectorizedmultiagentsimulator_amd as vmas

    assert Path(vmas.__file__).resolve().parent.parent == pkg_root, vmas.__file__
    if cfg == "r":
        return run_resets(args, vmas, torch)
    if cfg == "p":
        return run_published(args, vmas, torch)
    scenario = _user_scenario(args.scenario, vmas) if cfg == "d" else args.scenario
    graph = False if cfg in ("b", "c") else None
    env = vmas.make_env(scenario, num_envs=args.envs, device=args.device, seed=0, graph_step=graph)
    n_agents = len(env.agents)
    g = torch.Generator(device="cpu").manual_seed(1)
    actions = [[(torch.rand(args.envs, 2, generator=g) * 2 - 1).to(args.device) for _ in range(n_agents)]
               for _ in range(8)]
    for t in range(args.warmup):
        env.step([a.clone() for a in actions[t % 8]])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for t in range(args.steps):
        out = env.step([a.clone() for a in actions[t % 8]])
    e1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    dev = e0.elapsed_time(e1) * 1e-3
    assert all(bool(torch.isfinite(o).all()) for o in out[0])
    graph_obj = getattr(env, "_graph", None)
    chain = getattr(graph_obj, "_chain", None)
    return {
        "config": cfg, "scenario": args.scenario, "n_agents": n_agents, "envs": args.envs, "steps": args.steps,
        "step_us": round(dev / args.steps * 1e6, 2),
        "wall_step_us": round(wall / args.steps * 1e6, 2),
        "env_steps_per_s": round(args.envs * args.steps / dev),
        "graph_status": getattr(env, "graph_status", "off"),
        "graph_reason": getattr(env, "graph_reason", ""),
        "fused_status": getattr(env.scenario, "fused_status", ""),
        # launches of one replayed step: the chain's kernels (the post-replay launch comes on top)
        "chain_launches": getattr(chain, "n_nodes", None),
        "chain_why": getattr(graph_obj, "chain_why", ""),
        "carried": len(getattr(graph_obj, "_carry_names", []) or []),
        "direct_categories": len(getattr(getattr(graph_obj, "_direct", None), "enabled", []) or []),
        "package": "this tree" if pkg_root == ROOT else "--package-root",
    }


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--steps", type=int, default=300)
    p.add_argument("--warmup", type=int, default=30)
    p.add_argument("--envs", type=int, default=32768)
    p.add_argument("--scenario", default="simple_spread", choices=["simple_spread", "simple_tag"])
    p.add_argument("--scenarios", default="simple_spread,simple_tag")
    p.add_argument("--configs", default="abcrp")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--package-root", default="", help="config d: a built tree of the commit before")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--one", default="", choices=["", "a", "b", "c", "d", "r", "p"])
    p.add_argument("--out", default="")
    p.add_argument("--run-timeout", type=int, default=240)
    args = p.parse_args()
    if "d" in (args.one or args.configs) and not args.package_root:
        sys.exit("config d needs --package-root")
    if args.one:
        import torch

        if not torch.cuda.is_available():
            sys.exit("mpe_bench.py needs a ROCm GPU")
        print(json.dumps(run_one(args)), flush=True)
        return
    runs = []
    for rep in range(args.repeats):
        for name in args.scenarios.split(","):
            for cfg in args.configs:
                if cfg == "p" and name != "simple_spread":
                    continue
                cmd = [sys.executable, __file__, "--one", cfg, "--scenario", name, "--envs", str(args.envs),
                       "--steps", str(args.steps), "--warmup", str(args.warmup), "--device", args.device]
                if args.package_root:
                    cmd += ["--package-root", args.package_root]
                # (a child that fails or runs out of time ends the whole run: nothing more is started)
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.run_timeout)
                if r.returncode != 0:
                    sys.exit(f"run {cfg} {name} failed rc={r.returncode}:\n{r.stderr[-2000:]}")
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                rec["repeat"] = rep
                runs.append(rec)
                print(json.dumps(rec), flush=True)
    summary = {"bench": "mpe", "envs": args.envs, "steps": args.steps, "warmup": args.warmup, "ranges": {}}
    for rec in runs:
        s = summary["ranges"].setdefault(f"{rec['config']}/{rec['scenario']}", {})
        for name, v in rec.items():
            if name.endswith(("_us", "_ms", "_per_s", "_s")) and isinstance(v, (int, float)):
                s.setdefault(name, []).append(v)
        s["graph_status"] = rec.get("graph_status", "")
    print(json.dumps(summary), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in runs + [summary]) + "\n")


if __name__ == "__main__":
    main()
