"""Which division the discrete-action kernel (``vmas_apply_discrete_actions``) has to use.

The reference maps a discrete action ``a`` of ``n`` values to ``(a / (n - 1)) * (2 * u_max) - u_max``
(environment.py:693-703), four torch kernels and so four fp32 roundings.  On the CPU torch divides;
on a GPU its division by a Python scalar may be evaluated as a multiplication by the fp32
reciprocal.  The two differ in the last bit for about a fifth of the ``(n, a)`` pairs -- first at
(7, 5), (8, 3), (8, 6) -- and agree for the default ``nvec = [3, 3]``, so the library has a mode for
each and ``mode()`` probes, once per device, which one equals torch bit for bit on the whole
``(n, a)`` table of ``n = 2 .. 17``, or returns None (the env then keeps the per-agent path).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

# action dtypes the kernel reads (VMAS_DISCRETE_INT64 / _INT32 / _FLOAT32); others take the per-agent path
DTYPE_CODES = {torch.int64: 0, torch.int32: 1, torch.float32: 2}

MODES: Dict[str, Optional[int]] = {}  # str(device) -> 0 (divide), 1 (multiply by the reciprocal), None

_PROBE_N = list(range(2, 18))  # two refs of 8 components
# (f32 values whose products round: 1.0 alone would hide a contracted multiply-subtract)
_PROBE_RANGE = [0.7, 1.0, 0.3, 0.55, 1.3, 0.9, 0.1, 2.0]
_PROBE_MULT = [0.3, 1.0, 0.5, 0.7, 1.1, 0.45, 3.0, 0.9]


def _native():
    from ... import _native as N

    return N


def reference_u(a: torch.Tensor, nvec, u_range: torch.Tensor, u_mult: torch.Tensor) -> torch.Tensor:
    """u of a [B, len(nvec)] multi-discrete action with the reference's own torch expressions."""
    a = a.clone()
    u = torch.zeros(a.shape[0], len(nvec), device=a.device, dtype=torch.float32)
    for c, n in enumerate(nvec):
        pa = a[:, c]
        u_max = u_range[c]
        if n % 2 != 0:
            stay = pa == 0
            decrement = (pa > 0) & (pa <= n // 2)
            pa[stay] = n // 2
            pa[decrement] -= 1
        u[:, c] = (pa / (n - 1)) * (2 * u_max) - u_max
    u *= u_mult
    return u


def mode(device: torch.device) -> Optional[int]:
    key = str(device)
    if key in MODES:
        return MODES[key]
    N = _native()
    idx, stream = N.launch_args(device)
    B, K = max(_PROBE_N), N.DISCRETE_MAX_COMPONENTS
    rows = torch.arange(B, dtype=torch.int64).unsqueeze(1)
    r = torch.tensor(_PROBE_RANGE, dtype=torch.float32, device=device)
    m = torch.tensor(_PROBE_MULT, dtype=torch.float32, device=device)
    groups = [_PROBE_N[i:i + K] for i in range(0, len(_PROBE_N), K)]
    acts = [torch.minimum(rows, torch.tensor(g, dtype=torch.int64) - 1).to(device) for g in groups]
    want = [reference_u(a, g, r, m) for a, g in zip(acts, groups)]
    refs = np.zeros(len(groups), dtype=N.DISCRETE_ACTION_REF_DTYPE)
    for i, (a, g) in enumerate(zip(acts, groups)):
        refs[i] = (a.data_ptr(), r.data_ptr(), m.data_ptr(), i * B * K, a.stride(0), a.stride(1),
                   DTYPE_CODES[torch.int64], 0, K, K, g)
    flags = np.zeros(2 * len(groups), dtype=np.uint8)
    found = None
    for md in (0, 1):
        out = torch.zeros(len(groups) * B * K, dtype=torch.float32, device=device)
        N.check_aux(N.load_library().vmas_apply_discrete_actions(idx, B, refs.ctypes.data, len(groups), out.data_ptr(),
                                                                 md, flags.ctypes.data, stream),
                    "vmas_apply_discrete_actions")
        got = out.view(len(groups), B, K)
        if not flags.any() and all(torch.equal(got[i], w) for i, w in enumerate(want)):
            found = md
            break
    MODES[key] = found
    return found
