"""Which summation order torch's ``stack([B] * n, -1).sum(-1)`` uses on this device for 1 <= n <= 8
(simple_tag's team sums; the sibling of tools/probe_mean_order.py, which asked the same of flocking's
mean).  Per n it prints every candidate order that reproduces torch bit for bit on 4096 rows of
mixed-magnitude, mixed-sign values -- as a stacked tensor, as the scenario builds it -- and the
accumulator count ``simulator/_fused.reduce_order`` settles on.

    python tools/probe_sum_order.py [--device cuda:0]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def strided(v, s):
    """s accumulators: accumulator i sums elements i, i + s, ... in order."""
    acc = []
    for i in range(min(s, len(v))):
        a = v[i]
        for j in range(i + s, len(v), s):
            a = a + v[j]
        acc.append(a)
    return acc


def seq(v):
    s = v[0]
    for t in v[1:]:
        s = s + t
    return s


def tree(v):
    """Adjacent pairs: ((v0 + v1) + (v2 + v3)) + ..."""
    v = list(v)
    w = 1
    while w < len(v):
        for i in range(0, len(v) - w, 2 * w):
            v[i] = v[i] + v[i + w]
        w *= 2
    return v[0]


def candidates(cols):
    out = {"seq": seq(cols), "rev": seq(cols[::-1]), "tree": tree(cols)}
    for s in (2, 4, 8):
        if s <= len(cols):
            acc = strided(cols, s)
            out[f"str{s}_seq"] = seq(acc)
            out[f"str{s}_tree"] = tree(acc)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    dev = torch.device(args.device)
    from vectorizedmultiagentsimulator_amd import _native as N
    from vectorizedmultiagentsimulator_amd.simulator import _fused

    for n in range(1, 9):
        g = torch.Generator(device="cpu").manual_seed(4321 + n)
        x = torch.rand(4096, n, generator=g) * torch.exp2(torch.randint(-12, 12, (4096, n), generator=g).float())
        x = (x * (torch.randint(0, 2, (4096, n), generator=g).float() * 2 - 1)).to(dev)
        cols = [x[:, i].contiguous() for i in range(n)]
        ref = torch.stack(cols, dim=-1).sum(-1)
        hits = [k for k, v in candidates(cols).items() if torch.equal(v, ref)]
        print(json.dumps({"n": n, "device": str(dev), "orders_equal_to_torch": hits,
                          "reduce_order": _fused.reduce_order(dev, n, "sum", N.VMAS_MPE_MAX_AGENTS)}), flush=True)


if __name__ == "__main__":
    main()
