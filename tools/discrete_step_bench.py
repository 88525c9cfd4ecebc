#!/usr/bin/env python3
"""Step rate of a discrete-action env on one MI355X: balance (32 768 envs, 4 agents, 10 substeps)
in the loop ``env.step(env.get_random_actions())`` with flat and with multi-discrete actions
(bench.py measures the continuous flagship and has no discrete switch).  Per mode: warm-up steps
(they include the graph capture), then the timed steps between two device events, with a final
synchronise.  Prints one JSON line.

    python tools/discrete_step_bench.py [--steps 300] [--warmup 30] [--graph auto|on|off]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def run(args, multi: bool) -> dict:
    import torch

    from vectorizedmultiagentsimulator_amd import make_env

    graph = {"auto": None, "on": True, "off": False}[args.graph]
    env = make_env("balance", num_envs=args.envs, device=args.device, seed=0, graph_step=graph, n_agents=args.n_agents,
                   continuous_actions=False, multidiscrete_actions=multi)
    env.world._substeps = args.substeps
    env.world._sub_dt = env.world._dt / args.substeps
    for _ in range(args.warmup):
        env.step(env.get_random_actions())
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(args.steps):
        out = env.step(env.get_random_actions())
    e1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    dev = e0.elapsed_time(e1) * 1e-3
    assert all(bool(torch.isfinite(o).all()) for o in out[0])
    return {
        "step_us": round(dev / args.steps * 1e6, 2),
        "wall_step_us": round(wall / args.steps * 1e6, 2),
        "env_steps_per_s": round(args.envs * args.steps / dev),
        "graph_status": getattr(env, "graph_status", "off"),
        "graph_reason": getattr(env, "graph_reason", ""),
        "fused_actions": getattr(getattr(env, "_apply_cache", None), "refusal", "") is None,
    }


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--steps", type=int, default=300)
    p.add_argument("--warmup", type=int, default=30)
    p.add_argument("--envs", type=int, default=32768)
    p.add_argument("--n-agents", type=int, default=4)
    p.add_argument("--substeps", type=int, default=10)
    p.add_argument("--graph", default="auto", choices=["auto", "on", "off"])
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--label", default="")
    args = p.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("discrete_step_bench.py needs a ROCm GPU")
    out = {"bench": "discrete_step", "label": args.label,
           "workload": f"balance {args.envs} envs, n_agents={args.n_agents}, substeps={args.substeps}, "
                       f"env.step(env.get_random_actions()), graph={args.graph}",
           "steps": args.steps, "warmup": args.warmup}
    for name, multi in (("flat", False), ("multi", True)):
        out[name] = run(args, multi)
    try:
        from vectorizedmultiagentsimulator_amd.simulator.environment import _discrete

        out["division_mode"] = _discrete.MODES.get(str(torch.device(args.device)))
    except ImportError:  # (a tree without the fused discrete path)
        out["division_mode"] = None
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
