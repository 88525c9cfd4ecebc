"""The side-pruning bounds of csrc/vmas_physics.hpp (side_bounds; k_world's box narrowphases) on
the host: tests/side_prune_host.hip is compiled host-only into a stand-alone program, where
vote_all is the per-env predicate -- every sample decides for itself, stricter than the wave vote.

Per family (10^5 samples each, fixed seeds) and per class (box-sphere, box-line, box-box): the
pruned closest points are bitwise the unpruned ones and no scan has all four sides pruned.
Families: (a) balance's floor with its line / spheres, (b) small boxes at any rotation, (c)
targets inside or crossing the box, (d3 / d4) family (b) scaled by 10^3 / 10^4, (e) degenerate
inputs (zero-length line, zero half extents, NaN / +-Inf coordinates and rotations, rotations of
1e6 rad).  Non-vacuity: in family (a) exactly three sides are pruned in every sample -- a weaker
bound (a bounding circle, say) does not reach that."""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vectorizedmultiagentsimulator_amd" / "csrc"
SAMPLES = 100_000
FAMILIES = ["a", "b", "c", "d3", "d4", "e"]
CLASSES = ["bs", "bl", "bb"]


@pytest.fixture(scope="module")
def tallies(tmp_path_factory):
    exe = tmp_path_factory.mktemp("side_prune") / "side_prune_host"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "-I", str(CSRC), "-I", str(ROOT / "include"), "-o", str(exe),
                    str(ROOT / "tests" / "side_prune_host.hip")], check=True)
    out = subprocess.run([str(exe), str(SAMPLES)], check=True, capture_output=True, text=True).stdout
    rec = {}
    for line in out.splitlines():
        fam, cls, *fields = line.split()
        rec[fam, cls] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    return rec


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("fam", FAMILIES)
def test_pruned_scan_is_bitwise_the_full_scan(tallies, fam, cls):
    t = tallies[fam, cls]
    print(fam, cls, t)
    assert t["samples"] >= 100_000
    assert t["mismatch"] == 0
    assert t["all_pruned"] == 0


@pytest.mark.parametrize("cls", ["bs", "bl"])
def test_balance_prunes_exactly_three_sides(tallies, cls):
    t = tallies["a", cls]
    print(cls, t)
    assert t["samples"] >= 100_000 and t["not3"] == 0


@pytest.mark.parametrize("fam", ["b", "c", "d3", "d4"])
def test_bounds_prune_beyond_balance(tallies, fam):
    """The generic families prune too (some samples reach three sides), and scaling the geometry
    leaves the pruned fraction where it was: the margin scales with the operands."""
    t, b = tallies[fam, "bs"], tallies["b", "bs"]
    assert t["not3"] < t["samples"]
    if fam in ("d3", "d4"):
        assert abs(t["not3"] - b["not3"]) < 0.02 * t["samples"]
