"""The masked-reset structs (VmasMaskedSpan, VmasMutVec, VmasResetEntity, VmasBalanceResetIO) as
Python declares them against a C compilation of the header, following tests/test_abi.py; the two
entry points are exported and refuse bad arguments without a device."""
import ctypes
import subprocess
import tempfile
from pathlib import Path

from vectorizedmultiagentsimulator_amd import _native as N

ROOT = Path(__file__).resolve().parent.parent


def test_reset_struct_sizes_and_offsets_match_header_compilation():
    probe = r'''
#include <stddef.h>
#include <stdio.h>
#include "vmas_mi355x.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(VmasMaskedSpan), sizeof(VmasMutVec), sizeof(VmasResetEntity),
    sizeof(VmasBalanceResetIO), offsetof(VmasBalanceResetIO, mask), offsetof(VmasBalanceResetIO, agent_dx),
    offsetof(VmasBalanceResetIO, agents), offsetof(VmasBalanceResetIO, force), offsetof(VmasBalanceResetIO, steps),
    VMAS_MASKED_MAX_SPANS);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = Path(d) / "probe.c"
        src.write_text(probe)
        exe = Path(d) / "probe"
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        c = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()))
    io = N.VmasBalanceResetIO
    py = [ctypes.sizeof(N.VmasMaskedSpan), ctypes.sizeof(N.VmasMutVec), ctypes.sizeof(N.VmasResetEntity),
          ctypes.sizeof(io), io.mask.offset, io.agent_dx.offset, io.agents.offset, io.force.offset, io.steps.offset,
          N.VMAS_MASKED_MAX_SPANS]
    assert c == py
    assert N.MASKED_SPAN_DTYPE.itemsize == ctypes.sizeof(N.VmasMaskedSpan)
    # the spans and the reset's argument block travel as kernel arguments (4 KiB)
    assert N.VMAS_MASKED_MAX_SPANS * N.MASKED_SPAN_DTYPE.itemsize + 24 <= 4096
    assert ctypes.sizeof(io) + 16 <= 4096


def test_reset_entry_points_exported_and_checked():
    assert "vmas_masked_rows" in N.EXPORTED_SYMBOLS and "vmas_balance_reset" in N.EXPORTED_SYMBOLS
    lib = N.load_library()
    assert N.fn_addr("vmas_masked_rows") and N.fn_addr("vmas_balance_reset")
    assert lib.vmas_masked_rows(-1, None, 1, None, 4, 0, None) == -1  # spans NULL
    assert lib.vmas_masked_rows(-1, None, 0, None, 0, 0, None) == 0   # nothing to do
    inc = ctypes.c_uint64(0)
    assert lib.vmas_balance_reset(-1, None, ctypes.byref(inc), None) == -1  # (a device path only)
    io = N.VmasBalanceResetIO()
    assert lib.vmas_balance_reset(-1, ctypes.byref(io), ctypes.byref(inc), None) == -1
