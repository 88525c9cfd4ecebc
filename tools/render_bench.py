#!/usr/bin/env python3
"""rgb_array rendering on one MI355X: ``render_batch`` on balance (4 agents) for 1 024 environments
at 64 x 64, and one ``render`` at 700 x 700.  Per measurement: warm-up calls, then the timed calls
between two device events, with a final synchronise.  The batch's output rate is E * H * W * 3 bytes
per call over the device time, stated against the HBM write rate.  Prints one JSON line.

    python tools/render_bench.py [--calls 200] [--warmup 20]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_TBPS = 6.29  # measured float4-copy rate of an MI355X (8.0 TB/s by its specification)


def timed(torch, fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls, (time.perf_counter() - t0) / calls, out


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--calls", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--envs", type=int, default=1024)
    p.add_argument("--size", type=int, default=64)
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--label", default="")
    args = p.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("render_bench.py needs a ROCm GPU")
    from vectorizedmultiagentsimulator_amd import make_env

    env = make_env("balance", num_envs=args.envs, device=args.device, seed=0, n_agents=4)
    for _ in range(5):
        env.step(env.get_random_actions())
    size = (args.size, args.size)
    dev, wall, frames = timed(torch, lambda: env.render_batch(size=size), args.calls, args.warmup)
    nbytes = args.envs * args.size * args.size * 3
    assert frames.shape == (args.envs, args.size, args.size, 3) and bool((frames < 255).any())
    batch = {
        "call_us": round(dev * 1e6, 2), "wall_call_us": round(wall * 1e6, 2), "frames_per_s": round(args.envs / dev),
        "output_bytes": nbytes, "output_gb_per_s": round(nbytes / dev / 1e9, 2),
        "store_bound_us": round(nbytes / (HBM_TBPS * 1e12) * 1e6, 3),
        "share_of_hbm_write_rate": round(nbytes / dev / (HBM_TBPS * 1e12), 5),
    }
    single_calls = max(args.calls // 10, 5)
    dev1, wall1, frame = timed(torch, lambda: env.render(mode="rgb_array", env_index=0), single_calls, 3)
    assert frame.shape == (700, 700, 3)
    out = {"bench": "render", "label": args.label,
           "workload": f"balance n_agents=4: render_batch {args.envs} envs at {args.size}x{args.size}; "
                       f"render(mode='rgb_array') at 700x700",
           "calls": args.calls, "warmup": args.warmup, "hbm_write_tb_per_s": HBM_TBPS,
           "render_batch": batch,
           "render": {"calls": single_calls, "device_call_us": round(dev1 * 1e6, 2), "wall_call_us": round(wall1 * 1e6, 2)},
           "graph_status": getattr(env, "graph_status", "off")}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
