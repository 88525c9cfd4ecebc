#!/usr/bin/env python3
"""Time per call of the ways to reset some envs of a batch on one MI355X: balance at C2 size
(32 768 envs, 4 agents, 10 substeps) and transport at C3 size (32 768 envs, 4 agents), masks of
1 %, 10 % and 100 % of the envs.

Per (scenario, density), each between two device events with a synchronise before reading, after
warm-up steps (the graph is captured) and one untimed call of the method:
  reset          ``env.reset()`` (the mask does not matter)
  reset_at_loop  ``for i in mask.nonzero(): env.reset_at(i)`` over at most ``--cap`` indices, the
                 time scaled to the whole mask (``indices_timed``, ``indices`` and ``scaled`` say so)
  where_generic  ``env.reset_where(mask)`` through the full reset + the k_masked_rows merge (for
                 balance: with the scenario's own reset_world_where declining for the call)
  where_native   ``env.reset_where(mask)`` through k_balance_reset (balance only)
``*_with_step_us`` is the same call followed by one ``env.step(env.get_random_actions())`` (what
graph mode copies back before the next replay is in there); ``step_us`` is that step alone.
A tree without ``reset_where`` (the parent commit) times only reset and reset_at_loop.

    python tools/reset_bench.py [--reps 20] [--cap 200] [--label NAME] [--only balance|transport]
                                [--methods reset,reset_at_loop,where_generic,where_native]

Writes profiles/r12/masked_reset/<label>.json and prints the same JSON line.

``--scenario NAME[,NAME...]`` (balance, navigation, transport, discovery, flocking, sampling) times
those scenarios instead, ``where_native`` for every one whose class has a ``reset_world_where`` of its
own (navigation, transport, discovery, flocking: vmas_spawn_reset; sampling: vmas_sampling_reset), and
writes under profiles/r16/spawn_reset -- or, when flocking (32 768 envs, 8 agents: the C5 per-GPU shard)
or sampling (32 768 envs, 3 agents, as tools/sampling_bench.py) is among them, under
profiles/r17/flock_sampling_reset.
``--package-root DIR`` imports the package from DIR, a built checkout of another commit (the parent:
its ``reset_where`` is the generic path, ``where_generic``), so that the two trees can be run
alternately on the same calls:

    python tools/reset_bench.py --scenario navigation,transport,discovery --methods reset,where_generic,where_native
    python tools/reset_bench.py --scenario navigation,transport,discovery --methods reset,where_generic \
                                --package-root ../parent --label parent
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WORKLOADS = {
    "balance": dict(envs=32768, kw=dict(n_agents=4), substeps=10),   # C2
    "transport": dict(envs=32768, kw=dict(n_agents=4), substeps=0),  # C3
}
# --scenario: the scenarios with a native reset_where, at the sizes of their step benchmarks
SCENARIOS = {
    "balance": WORKLOADS["balance"],
    "navigation": dict(envs=32768, kw=dict(n_agents=4), substeps=0),
    "transport": WORKLOADS["transport"],
    "discovery": dict(envs=16384, kw=dict(), substeps=0),  # C4
    "flocking": dict(envs=32768, kw=dict(n_agents=8), substeps=0),  # the C5 per-GPU shard
    "sampling": dict(envs=32768, kw=dict(n_agents=3), substeps=0),  # as tools/sampling_bench.py
}
DENSITIES = (0.01, 0.1, 1.0)


def timed(torch, fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps, (time.perf_counter() - t0) * 1e6 / reps


def run(args, name):
    import torch

    from vectorizedmultiagentsimulator_amd import make_env

    wl = SCENARIOS[name] if args.scenario else WORKLOADS[name]
    B = wl["envs"]
    env = make_env(name, num_envs=B, device=args.device, seed=0, **wl["kw"])
    if wl["substeps"]:
        env.world._substeps = wl["substeps"]
        env.world._sub_dt = env.world._dt / wl["substeps"]
    step = lambda: env.step(env.get_random_actions())  # noqa: E731
    for _ in range(args.warmup):
        step()
    has_where = hasattr(env, "reset_where")
    from vectorizedmultiagentsimulator_amd.simulator.scenario import BaseScenario

    # the scenario resets the rows of a mask itself (k_balance_reset, vmas_spawn_reset)
    own = getattr(type(env.scenario), "reset_world_where", None) is not getattr(BaseScenario, "reset_world_where", None)
    out = {"envs": B, "graph_status": getattr(env, "graph_status", "off"), "has_reset_where": has_where}
    out["step_us"] = round(timed(torch, step, args.reps)[0], 2)
    g = torch.Generator(device="cpu").manual_seed(0)
    perm = torch.randperm(B, generator=g)
    for dens in DENSITIES:
        n = max(1, int(round(B * dens)))
        mask = torch.zeros(B, dtype=torch.bool)
        mask[perm[:n]] = True
        idx = mask.nonzero().flatten().tolist()
        mask = mask.to(args.device)
        rec = {"indices": n}
        methods = {}
        if "reset" in args.methods:
            methods["reset"] = (lambda: env.reset(), 1.0)
        if "reset_at_loop" in args.methods:
            sub = idx[:args.cap]
            rec["indices_timed"], rec["scaled"] = len(sub), round(n / len(sub), 3)

            def loop():
                for i in sub:
                    env.reset_at(i)

            methods["reset_at_loop"] = (loop, n / len(sub))
        if has_where and "where_generic" in args.methods:
            def generic():
                if own:  # (the scenario's own reset declines for the call: an instance attribute)
                    env.scenario.reset_world_where = lambda m: NotImplemented
                try:
                    env.reset_where(mask)
                finally:
                    env.scenario.__dict__.pop("reset_world_where", None)

            methods["where_generic"] = (generic, 1.0)
        if has_where and own and (name == "balance" or args.scenario) and "where_native" in args.methods:
            methods["where_native"] = (lambda: env.reset_where(mask), 1.0)
        for m, (fn, scale) in methods.items():
            reps = 2 if m == "reset_at_loop" else args.reps
            fn()
            step()
            n0 = getattr(env.scenario, "native_resets", 0)
            dev_us, wall_us = timed(torch, fn, reps)
            rec[m + "_us"] = round(dev_us * scale, 2)
            rec[m + "_wall_us"] = round(wall_us * scale, 2)
            if m == "where_native":
                assert env.scenario.native_resets == n0 + reps, "the native reset fell back"
            if m != "reset_at_loop":
                rec[m + "_with_step_us"] = round(timed(torch, lambda: (fn(), step()), reps)[0], 2)
        out[f"{dens:g}"] = rec
    out["graph_status_end"] = getattr(env, "graph_status", "off")
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--cap", type=int, default=200, help="most indices the reset_at loop is timed over")
    p.add_argument("--only", default=None, choices=list(WORKLOADS))
    p.add_argument("--scenario", default=None, help="comma-separated: " + ", ".join(SCENARIOS))
    p.add_argument("--package-root", default="", help="a built tree of another commit to import the package from")
    p.add_argument("--methods", default="reset,reset_at_loop,where_generic,where_native")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--label", default="run")
    p.add_argument("--out", default=None, help="directory of the JSON (default profiles/r12/masked_reset)")
    args = p.parse_args()
    args.methods = args.methods.split(",")
    if args.scenario:
        args.scenario = args.scenario.split(",")
        for name in args.scenario:
            if name not in SCENARIOS:
                p.error(f"--scenario {name}: one of {', '.join(SCENARIOS)}")
    if args.package_root:
        sys.path.insert(0, str(Path(args.package_root).resolve()))
    import torch

    if not torch.cuda.is_available():
        sys.exit("reset_bench.py needs a ROCm GPU")
    out = {"bench": "masked_reset", "label": args.label, "reps": args.reps, "warmup": args.warmup,
           "reset_at_cap": args.cap,
           "note": f"reset_at_loop: timed over at most {args.cap} indices and scaled to the mask's count"}
    if args.package_root:
        out["package_root"] = args.package_root
    for name in (args.scenario or ([args.only] if args.only else list(WORKLOADS))):
        out[name] = run(args, name)
    sub = ("r12", "masked_reset")
    if args.scenario:
        sub = ("r17", "flock_sampling_reset") if {"flocking", "sampling"} & set(args.scenario) else ("r16", "spawn_reset")
    d = Path(args.out) if args.out else ROOT / "profiles" / sub[0] / sub[1]
    d.mkdir(parents=True, exist_ok=True)
    (d / f"{args.label}.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
