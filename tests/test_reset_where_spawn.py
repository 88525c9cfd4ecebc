"""The spawn reset without a GPU: vmas_spawn_reset (csrc/vmas_reset.hip) refuses bad arguments before
it touches a device, its argument block is laid out as the header declares it, and on ``cpu``
navigation, transport and discovery still reset through the generic path (rows of the twin's
``reset()``, tests/_reset_where.py), their native counters untouched."""
import ctypes
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

from tests import _reset_where as R
from vectorizedmultiagentsimulator_amd import _native as N

ROOT = Path(__file__).resolve().parent.parent
VMAS_E_INVALID = -1  # (include/vmas_mi355x.h)


def _valid_io(keep):
    """An argument block that passes every check (host buffers: no call below reaches a launch)."""
    io = N.VmasSpawnResetIO()
    buf = (ctypes.c_float * 64)()
    words = (ctypes.c_int32 * N.VMAS_RESET_WORDS)()
    mask = (ctypes.c_uint8 * 4)()
    keep += [buf, words, mask]
    io.batch, io.mode, io.max_tries, io.n_place = 4, 0, 0, 2
    io.x_lo, io.x_hi, io.y_lo, io.y_hi = -1.0, 1.0, -1.0, 1.0
    io.mask = ctypes.addressof(mask)
    io.scratch = ctypes.addressof(buf)
    io.words = ctypes.addressof(words)
    return io


def test_spawn_reset_refuses_bad_arguments_before_any_device():
    assert "vmas_spawn_reset" in N.EXPORTED_SYMBOLS and N.fn_addr("vmas_spawn_reset")
    lib = N.load_library()
    inc, lost = ctypes.c_uint64(0), ctypes.c_int32(0)

    def call(io, device=0):
        return lib.vmas_spawn_reset(device, ctypes.byref(io) if io is not None else None, ctypes.byref(inc),
                                    ctypes.byref(lost), None)

    keep = []
    assert call(None) == VMAS_E_INVALID  # a null io
    assert b"vmas_spawn_reset" in lib.vmas_aux_last_error()
    for batch in (0, -3):
        io = _valid_io(keep)
        io.batch = batch
        assert call(io) == VMAS_E_INVALID
    io = _valid_io(keep)
    io.n_place = N.VMAS_RESET_MAX_PLACE + 1  # more entities than the cap
    assert call(io) == VMAS_E_INVALID
    io = _valid_io(keep)
    io.n_write = N.VMAS_RESET_MAX_WRITE + 1
    assert call(io) == VMAS_E_INVALID
    io = _valid_io(keep)
    io.mask = None  # a null mask
    assert call(io) == VMAS_E_INVALID
    io = _valid_io(keep)
    io.n_write, io.write_slot[0] = 1, 2  # an entity reading a slot that is not placed
    assert call(io) == VMAS_E_INVALID
    io = _valid_io(keep)
    io.n_derived = 1  # (kind 0)
    assert call(io) == VMAS_E_INVALID
    assert call(_valid_io(keep), device=-1) == VMAS_E_INVALID  # (a device path only)
    assert inc.value == 0 and lost.value == 0


def test_spawn_reset_struct_layout_matches_header_compilation():
    probe = r'''
#include <stddef.h>
#include <stdio.h>
#include "vmas_mi355x.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d\n", sizeof(VmasSpawnResetIO), sizeof(VmasResetDerived),
    offsetof(VmasSpawnResetIO, seed), offsetof(VmasSpawnResetIO, min_dist), offsetof(VmasSpawnResetIO, mask),
    offsetof(VmasSpawnResetIO, fixed), offsetof(VmasSpawnResetIO, write), offsetof(VmasSpawnResetIO, torque),
    offsetof(VmasSpawnResetIO, derived), VMAS_RESET_MAX_PLACE, VMAS_RESET_MAX_WRITE, VMAS_RESET_MAX_AGENTS,
    VMAS_RESET_MAX_FIXED, VMAS_RESET_MAX_DERIVED, VMAS_RESET_WORDS);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = Path(d) / "probe.c"
        src.write_text(probe)
        exe = Path(d) / "probe"
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        c = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()))
    io = N.VmasSpawnResetIO
    py = [ctypes.sizeof(io), ctypes.sizeof(N.VmasResetDerived), io.seed.offset, io.min_dist.offset, io.mask.offset,
          io.fixed.offset, io.write.offset, io.torque.offset, io.derived.offset, N.VMAS_RESET_MAX_PLACE,
          N.VMAS_RESET_MAX_WRITE, N.VMAS_RESET_MAX_AGENTS, N.VMAS_RESET_MAX_FIXED, N.VMAS_RESET_MAX_DERIVED,
          N.VMAS_RESET_WORDS]
    assert c == py
    assert ctypes.sizeof(io) <= 4096  # (it travels as a kernel argument)
    # navigation with 8 agents places 16 entities
    assert N.VMAS_RESET_MAX_PLACE >= 16 and N.VMAS_RESET_MAX_WRITE >= 16


@pytest.mark.parametrize("scenario,kw", [("navigation", {}), ("transport", {"n_packages": 2}), ("discovery", {})])
def test_cpu_worlds_take_the_generic_path(scenario, kw):
    B = 7
    env, twin = R.twins(scenario, 2, B, "cpu", **kw)
    assert env.scenario.native_resets == 0 and env.scenario.native_reset_fallbacks == 0
    assert env.scenario.spawn_max_tries == 0
    mask = torch.arange(B) % 3 == 1
    R.check_rows_of_full_reset(env, twin, mask, mask, "cpu")
    assert env.scenario.native_resets == 0 and env.scenario.native_reset_fallbacks == 0
