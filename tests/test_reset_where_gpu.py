"""Environment.reset_where(mask) on a ROCm device: balance's native reset (one k_balance_reset
launch), the generic path's merge (one k_masked_rows launch), graph mode, and k_masked_rows alone.

The yardstick is ``reset()`` of a twin env at the same state and generator states
(tests/_reset_where.py), never reset_where itself.
"""
import pytest
import torch

from tests import _reset_where as R
from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd.simulator import _fused
from vectorizedmultiagentsimulator_amd.simulator.environment import _uniform

SKIPPED = [0]  # cases skipped because no vmas_uniform_columns mode equals torch (expected: 0)

BALANCE = [(B, A, True) for B in (1, 64, 65, 300) for A in (2, 4)] + [(65, 4, False)]


def _resync(dev, envs):
    """Back to one common state: a full reset of every env from the same generator states, then
    two steps (which recompute the per-step attributes a reset leaves alone)."""
    R.turns(dev, envs, lambda e: e.reset())
    for _ in range(2):
        R.step_all(dev, envs)


@pytest.mark.gpu
@pytest.mark.parametrize("B,A,random_pkg", BALANCE)
def test_native_balance_rows_of_a_full_reset_gpu(gpu_device, B, A, random_pkg):
    """Every mask of the CPU test, on one trio of envs per world: `native` resets through
    k_balance_reset (native_resets counts the launches), `generic` through the full reset and the
    k_masked_rows merge (the fused programs switched off for the call), `twin` is reset() -- all
    three from the same state and generator states.  native must equal the twin inside the mask
    and itself outside it, and the generic path must leave the identical world."""
    dev = gpu_device
    torch.cuda.init()  # (the probe reads the device generator)
    if _uniform.mode(torch.device(dev), B) is None:
        SKIPPED[0] += 1
        print(f"reset_where native cases skipped: {SKIPPED[0]} (expected 0)")
        pytest.skip("no uniform mode equals torch on this device")
    print(f"reset_where native cases skipped: {SKIPPED[0]} (expected 0)")
    kw = dict(n_agents=A, random_package_pos_on_line=random_pkg, max_steps=50, graph_step=False)
    native, generic, twin = envs = R.twins("balance", 3, B, dev, **kw)
    cases = R.mask_cases(B) + [("none", None, None)]
    for name, arg, mask in cases:
        if arg is None:  # mask=None: the done envs -- some truncated by a forced step count
            for e in envs:
                e.steps[::3] = 50
            mask = twin.done().cpu()
            assert mask[0]
        mask_d = mask.to(dev)
        if isinstance(arg, torch.Tensor):
            arg = arg.to(dev)
        n0, g0 = native.scenario.native_resets, generic.scenario.native_resets
        before = R.snapshot(native)

        def call(i):
            if i == 0:
                return native.reset_where(arg)
            if i == 1:
                with _fused.disabled():
                    return generic.reset_where(arg)
            return twin.reset()

        (o_n, o_g, o_t), (r_n, r_g, r_t) = R.turns(dev, [0, 1, 2], call)
        assert native.scenario.native_resets == n0 + 1, name  # no silent fall-back
        assert generic.scenario.native_resets == g0, name
        assert R.same_rng(r_n, r_t) and R.same_rng(r_g, r_t), name
        s_n, s_g, s_t = R.batched_state(native), R.batched_state(generic), R.batched_state(twin)
        assert set(s_n) == set(s_g) == set(s_t) == set(before)
        for k in s_n:
            assert torch.equal(s_n[k][mask_d], s_t[k][mask_d]), (name, k, "masked rows differ from reset()")
            assert torch.equal(s_n[k][~mask_d], before[k][~mask_d]), (name, k, "rows outside the mask changed")
            assert torch.equal(s_n[k], s_g[k]), (name, k, "the generic path leaves another world")
        for x, y, z in zip(R.flat(o_n), R.flat(o_g), R.flat(o_t)):
            assert torch.equal(x, y), name
            assert torch.equal(x[mask_d], z[mask_d]), name
        a, b, c = R.step_all(dev, envs)
        for x, y, z in zip(R.flat(a), R.flat(b), R.flat(c)):
            assert torch.equal(x, y), name
            assert torch.equal(x[mask_d], z[mask_d]), name
        _resync(dev, envs)


def _state(env):
    out = []
    for e in env.world.entities:
        s = e.state
        out += [s.pos, s.vel, s.rot, s.ang_vel]
    for a in env.world.agents:
        out += [a.state.force, a.state.torque]
    out += [env.scenario.global_shaping, env.scenario.on_the_ground, env.steps]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("max_steps", [None, 100])
@pytest.mark.parametrize("path", ["native", "generic"])
def test_reset_where_between_graph_replays_gpu(gpu_device, path, max_steps):
    """reset_where between the steps of a graph-mode env: still replaying afterwards, and every
    step's outputs and states equal to an eager twin's.  native: in-place writes, seen by version
    counters; generic: re-binds, copied into the captured tensors; max_steps: the step counter
    stays in the graph, without it the folded increment must follow env.steps."""
    dev = gpu_device
    B = 64
    kw = dict(n_agents=4, max_steps=max_steps)
    (eager, graph), _ = R.turns(dev, [False, True], lambda g: R.make_env("balance", num_envs=B, device=dev, seed=1,
                                                                           graph_step=g, **kw))
    for env in (eager, graph):
        env.world._substeps = 10
        env.world._sub_dt = env.world._dt / 10
    masks = {5: torch.arange(B, device=dev) % 4 == 1, 9: torch.arange(B, device=dev) % 5 == 0}
    for t in range(14):
        actions = eager.get_random_actions()
        if t in masks:
            assert graph.graph_status == "graph", graph.graph_reason
            n0 = graph.scenario.native_resets

            def call(env):
                if path == "native":
                    return env.reset_where(masks[t])
                with _fused.disabled():
                    return env.reset_where(masks[t])

            (o_e, o_g), (r_e, r_g) = R.turns(dev, [eager, graph], call)
            assert graph.scenario.native_resets == n0 + (1 if path == "native" else 0)
            assert R.same_rng(r_e, r_g)
            for x, y in zip(R.flat(o_e), R.flat(o_g)):
                assert torch.equal(x, y), t
            for x, y in zip(_state(eager), _state(graph)):
                assert torch.equal(x, y), t
            assert graph.graph_status == "graph", graph.graph_reason
        out_e, out_g = R.turns(dev, [eager, graph], lambda e: e.step([a.clone() for a in actions]))[0]
        fe, fg = R.flat(out_e), R.flat(out_g)
        assert len(fe) == len(fg)
        for i, (x, y) in enumerate(zip(fe, fg)):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (t, i)
        for i, (x, y) in enumerate(zip(_state(eager), _state(graph))):
            assert torch.equal(x, y), (t, i)
        if t >= 3:
            assert graph.graph_status == "graph", (t, graph.graph_reason)
    assert graph._graph.replays >= 10
    assert graph._graph._steps_folded == (max_steps is None)


def _masked_case(device, B, seed):
    """Spans of 4-, 8- and 64-byte rows (contiguous, and with a stride longer than the row), an
    odd 6-byte row and a 1-byte row; (spans, dst tensors, expected tensors)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    mask = torch.rand(B, generator=g) < 0.4
    if B > 1:
        mask[0], mask[B - 1] = True, False
    spans, dsts, want, keep = [], [], [], []
    for dtype, cols, pad in ((torch.float32, 1, 0), (torch.float32, 2, 0), (torch.float32, 16, 0),
                             (torch.float32, 2, 3), (torch.float32, 1, 1), (torch.int16, 3, 0), (torch.bool, 1, 0),
                             (torch.float32, 16, 4)):
        def rnd():
            t = torch.randint(0, 200, (B, cols + pad), generator=g).to(dtype)
            return t.to(device)

        dst_full, src_full = rnd(), rnd()
        dst, src = dst_full[:, :cols], src_full[:, :cols]  # (pad > 0: rows strided, not contiguous)
        m = mask.to(device).unsqueeze(1)
        ref_full = dst_full.clone()
        ref_full[:, :cols] = torch.where(m, dst, src)  # rows outside the mask come from src
        es = dst.element_size()
        spans.append((dst.data_ptr(), src.data_ptr(), cols * es, dst.stride(0) * es, src.stride(0) * es))
        dsts.append(dst_full)
        want.append(ref_full)
        keep.append(src_full)
    return mask.to(device), spans, dsts, want, keep


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1000])
def test_masked_rows_match_torch_where_gpu(gpu_device, B):
    mask, spans, dsts, want, keep = _masked_case(gpu_device, B, B)
    N.masked_rows(0, spans, mask.data_ptr(), B, False, N.stream_ptr(0))
    torch.cuda.synchronize()
    for i, (d, w) in enumerate(zip(dsts, want)):
        assert torch.equal(d, w), (B, i)


@pytest.mark.gpu
def test_masked_rows_more_spans_than_one_launch_gpu(gpu_device):
    B = 65
    mask = (torch.arange(B) % 2 == 0).to(gpu_device)
    n = N.VMAS_MASKED_MAX_SPANS + 5
    dst = torch.zeros(n, B, 2, device=gpu_device)
    src = torch.arange(n * B * 2, dtype=torch.float32, device=gpu_device).reshape(n, B, 2)
    spans = [(dst[i].data_ptr(), src[i].data_ptr(), 8, 8, 8) for i in range(n)]
    N.masked_rows(0, spans, mask.data_ptr(), B, True, N.stream_ptr(0))  # (the other direction: rows of the mask)
    torch.cuda.synchronize()
    assert torch.equal(dst, torch.where(mask.view(1, B, 1), src, torch.zeros_like(src)))


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1000])
def test_masked_rows_host_backend(B):
    mask, spans, dsts, want, keep = _masked_case("cpu", B, B)
    N.masked_rows(-1, spans, mask.data_ptr(), B, False, None)
    for i, (d, w) in enumerate(zip(dsts, want)):
        assert torch.equal(d, w), (B, i)


def test_masked_rows_refuse_overlapping_rows():
    t = torch.zeros(8, 2)
    m = torch.ones(8, dtype=torch.bool)
    with pytest.raises(N.NativeLibraryError):
        N.masked_rows(-1, [(t.data_ptr(), t.data_ptr(), 8, 4, 8)], m.data_ptr(), 8, False, None)
