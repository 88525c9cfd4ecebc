"""Digest of the generated k_world source of a fixed list of worlds, without a GPU: one line per
world with its name, the source length and the sha256 of the source (what the bench's PMC records
are keyed on, kernel_source_sha256).  Equal digests before and after a change of the generator
mean the shipped kernels' text is unchanged.  The source does not cover the headers it includes:
--isa adds the sha256 of the gfx950 device assembly (tools/kworld_isa.py device_asm) of the whole
module and of each kernel in it.
usage: python tools/kworld_source_digest.py [--isa] [world ...]      (no VMAS_* variable set)
To compare two commits, run this file and tools/kworld_isa.py of the newer one in both trees.
"""
import argparse
import hashlib
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from kworld_isa import PRESET, device_asm, kernel_body, preset_source  # noqa: E402  (tools/, the script's directory)

N_FUZZ = 5


def worlds():
    """(name, function returning the generated source), in a fixed order."""
    from tests import _fuzz_world as F
    from tests._parity import SCENARIOS, make

    def parity(name, kw, sub):
        return lambda: make(name, kw, sub, "cpu", num_envs=8, seed=0).world.engine.jit_compile_check()

    out = [(f"parity/{name}", parity(name, kw, sub)) for name, kw, sub in SCENARIOS]
    # tests/test_jit.py test_jit_oversized_world_keeps_its_rows_in_global_memory
    out.append(("oversized/pollock", parity("pollock", dict(n_agents=8, n_lines=10, n_boxes=10), None)))
    out += [(f"bench/{name}", lambda name=name: preset_source(name, num_envs=8)) for name in PRESET]
    out += [(f"fuzz/{seed}", lambda seed=seed: F.case(seed)[0].engine.jit_compile_check())
            for seed in F.SEEDS[:N_FUZZ]]
    return out


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--isa", action="store_true", help="also hash the gfx950 device assembly")
    p.add_argument("only", nargs="*", help="world names (default: all)")
    args = p.parse_args()
    for name, source in worlds():
        if args.only and name not in args.only:
            continue
        src = source()
        line = f"{name:20s} {len(src):7d} {sha(src)}"
        if args.isa:
            asm = device_asm(src)
            line += f" isa {sha(asm)}"
            for kernel in ("k_world", "k_program_jit"):
                body = kernel_body(asm, kernel)
                if body:
                    line += f" {kernel} {sha(body)}"
        print(line, flush=True)


if __name__ == "__main__":
    main()
