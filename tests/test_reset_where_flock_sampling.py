"""The masked resets of flocking and sampling without a GPU: vmas_sampling_reset (csrc/vmas_scenarios.hip)
and the v15 vocabulary of vmas_spawn_reset (csrc/vmas_reset.hip: fixed-source writes, the separation
record, the float-row zero) refuse bad arguments before they touch a device, their argument blocks are
laid out as the header declares them, and on ``cpu`` both scenarios still reset through the generic
path (rows of the twin's ``reset()``, tests/_reset_where.py), their native counters untouched."""
import ctypes
import re
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

from tests import _reset_where as R
from tests.test_reset_where_spawn import VMAS_E_INVALID, _valid_io
from vectorizedmultiagentsimulator_amd import _native as N

ROOT = Path(__file__).resolve().parent.parent


def test_abi_version_is_15_on_both_sides():
    """The header, the binding and the library agree, at the version that brought these calls (15) or
    a later one, and the header's changelog has the line."""
    header = (ROOT / "include" / "vmas_mi355x.h").read_text()
    version = int(re.search(r"^#define VMAS_ABI_VERSION (\d+)$", header, re.M).group(1))
    assert " * v15:" in header and "vmas_sampling_reset" in header
    assert version >= 15 and N.VMAS_ABI_VERSION == version and N.load_library().vmas_abi_version() == version


def _valid_sampling_io(keep):
    """An argument block that passes every check (host buffers: no call below reaches a launch)."""
    io = N.VmasSamplingResetIO()
    f = (ctypes.c_float * 64)()
    u8 = (ctypes.c_uint8 * 64)()
    keep += [f, u8]
    fa, ua = ctypes.addressof(f), ctypes.addressof(u8)
    io.batch, io.n_agents, io.mode, io.norm, io.n_xs, io.n_ys = 4, 2, 0, 1, 4, 4
    io.grid.n_x, io.grid.n_y = 4, 4
    io.density.n_gaussians, io.density.sum_mode = 2, 2
    for g in range(2):
        io.density.loc[g].p, io.density.loc[g].s0, io.density.loc[g].s1 = fa, 2, 1
    io.xs, io.ys, io.mask, io.max_pdf, io.sampled = fa, fa, ua, fa, ua
    for a in range(2):
        io.agents[a].pos.p, io.agents[a].pos.s0, io.agents[a].pos.s1 = fa, 2, 1
        io.sample[a] = fa
    return io


def test_sampling_reset_refuses_bad_arguments_before_any_device():
    assert "vmas_sampling_reset" in N.EXPORTED_SYMBOLS and N.fn_addr("vmas_sampling_reset")
    lib = N.load_library()
    inc = ctypes.c_uint64(0)

    def refused(io, device=0):
        rc = lib.vmas_sampling_reset(device, ctypes.byref(io) if io is not None else None, ctypes.byref(inc), None)
        return rc == VMAS_E_INVALID and b"vmas_sampling_reset" in lib.vmas_aux_last_error()

    keep = []
    assert refused(None)  # a null block
    for batch in (0, -3):
        io = _valid_sampling_io(keep)
        io.batch = batch
        assert refused(io)
    io = _valid_sampling_io(keep)
    io.mask = None  # a null mask
    assert refused(io)
    io = _valid_sampling_io(keep)
    io.n_agents = N.VMAS_SAMPLING_MAX_AGENTS + 1
    assert refused(io)
    io = _valid_sampling_io(keep)
    io.density.n_gaussians = N.VMAS_SAMPLING_MAX_GAUSSIANS + 1
    assert refused(io)
    io = _valid_sampling_io(keep)
    io.sample[1] = None  # an agent without its sample row
    assert refused(io)
    assert refused(_valid_sampling_io(keep), device=-1)  # (the draws are a device path only)
    assert inc.value == 0


def test_spawn_reset_refuses_malformed_v15_records_before_any_device():
    lib = N.load_library()
    inc, lost = ctypes.c_uint64(0), ctypes.c_int32(0)
    keep = []
    out = (ctypes.c_float * 4)()
    fixed = (ctypes.c_float * 8)()

    def call(io):
        return lib.vmas_spawn_reset(0, ctypes.byref(io), ctypes.byref(inc), ctypes.byref(lost), None)

    def refused(io):
        return call(io) == VMAS_E_INVALID and b"vmas_spawn_reset" in lib.vmas_aux_last_error()

    def with_fixed():
        io = _valid_io(keep)  # (n_place = 2)
        io.n_fixed = 1
        io.fixed[0].p, io.fixed[0].s0, io.fixed[0].s1 = ctypes.addressof(fixed), 2, 1
        return io

    def with_sep():
        io = with_fixed()
        io.n_sep, io.sep_sum_mode = 3, 2
        io.sep_slot[0], io.sep_slot[1], io.sep_slot[2] = -1, 0, 1
        io.n_derived = 1
        r = io.derived[0]
        r.kind, r.a, r.factor = N.VMAS_RESET_D_MEAN_SQ_SEP, 1, 1.0
        r.out.p, r.out.s0 = ctypes.addressof(out), 1
        return io

    # a fixed-source write: fixed[0] exists, fixed[1] does not; without fixed positions none does
    io = with_fixed()
    io.n_write, io.write_slot[0] = 1, -2
    assert refused(io)
    io = _valid_io(keep)
    io.n_write, io.write_slot[0] = 1, -1
    assert refused(io)
    io = with_fixed()
    io.n_write, io.write_slot[0] = 1, -(2 ** 31)
    assert refused(io)
    # the separation record: every way it can be malformed
    for spoil in ("entry", "no_list", "one_entry", "too_long", "order_0", "order_3", "order_32", "slot", "fixed_slot",
                  "null_out"):
        io = with_sep()
        r = io.derived[0]
        if spoil == "entry":
            r.a = 3
        elif spoil == "no_list":
            io.n_sep = 0
        elif spoil == "one_entry":
            io.n_sep, r.a = 1, 0
        elif spoil == "too_long":
            io.n_sep = N.VMAS_RESET_MAX_SEP + 1
        elif spoil.startswith("order_"):
            io.sep_sum_mode = int(spoil[6:])
        elif spoil == "slot":
            io.sep_slot[2] = 2
        elif spoil == "fixed_slot":
            io.sep_slot[0] = -2
        else:
            r.out.p = None
        assert refused(io), spoil
    # the float-row zero without its row
    io = _valid_io(keep)
    io.n_derived = 1
    io.derived[0].kind = N.VMAS_RESET_D_ZERO32
    assert refused(io)
    assert inc.value == 0 and lost.value == 0
    # (the well-formed blocks -- with_sep(), a write of -1 with one fixed position -- reach a launch:
    # tests/test_reset_where_flock_sampling_gpu.py)


def test_v15_struct_layouts_match_header_compilation():
    probe = r'''
#include <stddef.h>
#include <stdio.h>
#include "vmas_mi355x.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d\n", sizeof(VmasSpawnResetIO), sizeof(VmasResetDerived),
    offsetof(VmasSpawnResetIO, derived), offsetof(VmasSpawnResetIO, n_sep), offsetof(VmasSpawnResetIO, sep_sum_mode),
    offsetof(VmasSpawnResetIO, sep_desired), offsetof(VmasSpawnResetIO, sep_slot), VMAS_RESET_MAX_SEP,
    VMAS_RESET_D_MEAN_SQ_SEP, VMAS_RESET_D_ZERO32);
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(VmasSamplingResetIO),
    offsetof(VmasSamplingResetIO, n_xs), offsetof(VmasSamplingResetIO, loc_lo), offsetof(VmasSamplingResetIO, spawn_hi),
    offsetof(VmasSamplingResetIO, seed), offsetof(VmasSamplingResetIO, offset), offsetof(VmasSamplingResetIO, grid),
    offsetof(VmasSamplingResetIO, density), offsetof(VmasSamplingResetIO, xs), offsetof(VmasSamplingResetIO, mask),
    offsetof(VmasSamplingResetIO, steps), offsetof(VmasSamplingResetIO, agents), offsetof(VmasSamplingResetIO, torque),
    offsetof(VmasSamplingResetIO, sample));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = Path(d) / "probe.c"
        src.write_text(probe)
        exe = Path(d) / "probe"
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        lines = subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines()
    c = [list(map(int, line.split())) for line in lines]
    sp, sa = N.VmasSpawnResetIO, N.VmasSamplingResetIO
    assert c[0] == [ctypes.sizeof(sp), ctypes.sizeof(N.VmasResetDerived), sp.derived.offset, sp.n_sep.offset,
                    sp.sep_sum_mode.offset, sp.sep_desired.offset, sp.sep_slot.offset, N.VMAS_RESET_MAX_SEP,
                    N.VMAS_RESET_D_MEAN_SQ_SEP, N.VMAS_RESET_D_ZERO32]
    assert c[1] == [ctypes.sizeof(sa), sa.n_xs.offset, sa.loc_lo.offset, sa.spawn_hi.offset, sa.seed.offset,
                    sa.offset.offset, sa.grid.offset, sa.density.offset, sa.xs.offset, sa.mask.offset, sa.steps.offset,
                    sa.agents.offset, sa.torque.offset, sa.sample.offset]
    # (both travel as kernel arguments, the sampling block beside the 16-byte draw grid)
    assert ctypes.sizeof(sp) <= 4096 and ctypes.sizeof(sa) + 16 <= 4096
    assert N.VMAS_RESET_MAX_SEP == N.VMAS_FLOCK_MAX_AGENTS  # (the step program's accumulators)


@pytest.mark.parametrize("scenario,kw", [("flocking", {}), ("flocking", {"n_agents": 1, "n_obstacles": 0}),
                                         ("sampling", {}), ("sampling", {"n_agents": 1, "norm": False})])
def test_cpu_worlds_take_the_generic_path(scenario, kw):
    B = 7
    env, twin = R.twins(scenario, 2, B, "cpu", **kw)
    assert env.scenario.native_resets == 0
    if scenario == "flocking":
        assert env.scenario.native_reset_fallbacks == 0 and env.scenario.spawn_max_tries == 0
    mask = torch.arange(B) % 3 == 1
    R.check_rows_of_full_reset(env, twin, mask, mask, "cpu", return_info=True)
    assert env.scenario.native_resets == 0
    assert getattr(env.scenario, "native_reset_fallbacks", 0) == 0
