"""The post-replay stage's address arithmetic and tree shaping (simulator/environment/_post.py) on
CPU tensors: tables are built, nothing is launched.

The expected rows follow the rules as ``StepGraph._post_spans`` / ``_post_table`` stated them
before they moved here.  When they moved, the cases below were also run once through the old
methods (on a stand-in object carrying the attributes they read) and gave rows identical to the
new functions'.
"""
from types import SimpleNamespace

import numpy as np
import torch

from vectorizedmultiagentsimulator_amd import _native as N
from vectorizedmultiagentsimulator_amd.simulator.environment._post import (
    PostStage, _clone_plan, _post_spans, _post_table, _steps_current)

U8 = torch.uint8


def out_tree():
    t0 = torch.zeros(4, 3)
    t1 = torch.zeros(4)
    t2 = torch.zeros(3, 4).t()  # (the non-contiguous member, shape (4, 3))
    t3 = torch.zeros(4, dtype=torch.bool)
    t4 = torch.zeros(4, 2, dtype=torch.bool)
    t5 = t0  # (the same tensor twice: two fresh copies)
    ka, kb, kk, kn = "a", "b", "k", "n"
    tree = [{ka: t0, kb: (t1, t2)}, [t3], {kk: {kn: t4}}, t5]
    return tree, [t0, t1, t2, t3, t4, t5]


def carry_pair():
    """One carry pair: X and Y are the first 192 bytes of two 256-byte buffers (so that a tensor
    can straddle X's end)."""
    bx, by = torch.zeros(256, dtype=U8), torch.zeros(256, dtype=U8)
    return bx, by, bx[:192], by[:192]


def table(outs=(), bk_src=(), bk_dst=(), direct=(), state_idx=None, steps=None, wb=False, pair=None):
    _, _, x, y = pair or carry_pair()
    outs = list(outs)
    _, group_srcs, _ = _clone_plan(outs, outs, list(direct))
    return _post_table(group_srcs, [x], [y], [], list(bk_src), list(bk_dst), list(direct), state_idx, steps, wb)


def rows(t, lo=0, hi=None):
    return [(int(r["src"]), int(r["dst"]), int(r["nbytes"])) for r in t.tbl[lo:hi]]


def test_tree_rebuild():
    tree, ts = out_tree()
    groups, group_srcs, (fn, consts) = _clone_plan(ts, tree, [])
    # by (dtype, shape), the same dtypes adjacent (ordered by the dtype's name)
    assert groups == [(torch.bool, (4,), 1), (torch.bool, (4, 2), 1), (torch.float32, (4, 3), 3),
                      (torch.float32, (4,), 1)]
    assert [(a, b) for a, b, _ in group_srcs] == [(0, 1), (1, 2), (2, 5), (5, 6)]
    order = [ts[3], ts[4], ts[0], ts[2], ts[5], ts[1]]  # the sources in plan order
    assert all(a is b for a, b in zip([x for _, _, srcs in group_srcs for x in srcs], order))
    # sentinel views in plan order: each names the output position its source came from
    at = {3: 0, 4: 1, 0: 2, 2: 3, 5: 4, 1: 5}  # output index -> view index
    views = [None] * 6
    for i, p in at.items():
        views[p] = ("view", i)
    out = fn(views, consts)
    assert out == [{"a": ("view", 0), "b": (("view", 1), ("view", 2))}, [("view", 3)], {"k": {"n": ("view", 4)}},
                   ("view", 5)]
    assert type(out[0]["b"]) is tuple and type(out[1]) is list
    for new, old in ((out[0], tree[0]), (out[2], tree[2]), (out[2]["k"], tree[2]["k"])):
        assert all(a is b for a, b in zip(new, old))  # dict keys by identity
    # non-tensor leaves by identity
    marker = object()
    _, _, (fn2, c2) = _clone_plan([ts[0]], [ts[0], {"x": marker}, None], [])
    out2 = fn2(["v"], c2)
    assert out2[0] == "v" and out2[1]["x"] is marker and out2[2] is None
    # the non-contiguous member: in loose (by view index), no output row
    t = _post_table(group_srcs, [], [], [], [], [], [], None, None)
    assert len(t.loose) == 1 and t.loose[0][0] == 3 and t.loose[0][1] is ts[2]
    assert t.contig == [[True], [True], [True, False, True], [True]]
    assert t.n_out == t.n_all == 5 and not t.plain
    assert rows(t) == [(x.data_ptr(), 0, x.numel() * x.element_size()) for x in order if x.is_contiguous()]
    assert ts[2].data_ptr() not in {r[0] for r in rows(t)}


def test_spans_backup_sources():
    bx, by, x, y = carry_pair()
    X, Y = x.data_ptr(), y.data_ptr()
    inside, outside = bx[16:48].view(torch.float32), torch.zeros(8)
    d_in, d_out = torch.empty_like(inside), torch.empty_like(outside)
    carry, bk, n = _post_spans([x], [y], [inside, outside], [d_in, d_out], None)
    assert carry == [(Y, X, 192)] and n == 2
    assert bk[0] == (Y + 16, d_in.data_ptr(), 32)  # (a) inside X: read from Y + (lo - X)
    assert bk[1] == (outside.data_ptr(), d_out.data_ptr(), 32)  # (b) outside X: its own address
    t = table(bk_src=[inside, outside], bk_dst=[d_in, d_out], pair=(bx, by, x, y))
    assert not t.plain and t.n_bk == 2 and t.n_out == 0 and rows(t) == carry + bk
    for bad in (bx[160:224], bx[0:64:2]):  # (c) straddling X's end; (d) not contiguous
        d = torch.empty(bad.shape, dtype=U8)
        assert _post_spans([x], [y], [bad], [d], None) == (carry, None, 0)
        out = torch.zeros(4)
        t = table(outs=[out], bk_src=[bad], bk_dst=[d], pair=(bx, by, x, y))
        assert t.plain and t.n_bk == 0 and t.n_all == t.n_out == 1
        assert rows(t) == [(out.data_ptr(), 0, 16)]  # no carry or backup rows


def test_spans_clash_and_writeback():
    pair = carry_pair()
    bx, _, x, _ = pair
    assert table(outs=[bx[8:24].view(torch.float32)], pair=pair).clash  # (e) an output that is a slice of X
    assert not table(outs=[torch.zeros(4)], pair=pair).clash
    assert not table(outs=[bx[192:256]], pair=pair).clash  # (the same buffer, past X's end)
    X = x.data_ptr()
    for state_idx, wb, n in ((0, False, 1), (0, True, 0), (None, True, 1)):  # (f)
        t = table(outs=[torch.zeros(4)], state_idx=state_idx, wb=wb, pair=pair)
        assert sum(1 for r in rows(t) if r[1] == X) == n, (state_idx, wb)
        assert t.n_all - t.n_out == n and not t.plain


def test_steps_row_and_direct_words():
    pair = carry_pair()
    out, steps = torch.zeros(4), torch.zeros(5)
    member = torch.zeros(4)
    word = torch.zeros(2, dtype=torch.int64)
    direct = [{"members": [member], "word": word.data_ptr() + 8}]
    t = table(outs=[out, member], direct=direct, steps=steps, pair=pair)
    # (h) a store row per direct region, at the region's word; its members have no copy row
    assert t.direct_rows == [1] and rows(t, 1, 2) == [(0, word.data_ptr() + 8, N.VMAS_COPY_STORE64)]
    assert member.data_ptr() not in {r[0] for r in rows(t)}
    # (g) the folded steps row: the last output row
    assert t.steps_row == t.n_out - 1 == 2 and t.steps is steps
    assert rows(t, 2, 3) == [(0, steps.data_ptr(), steps.numel() * 4)]
    before = t.tbl.copy()
    _steps_current(t, steps)
    assert np.array_equal(t.tbl, before)
    rebound = torch.zeros(7)
    _steps_current(t, rebound)
    assert t.steps is rebound and rows(t, 2, 3) == [(0, rebound.data_ptr(), 28)]
    keep = np.arange(len(before)) != t.steps_row
    assert np.array_equal(t.tbl[keep], before[keep])  # that row only
    assert table(outs=[out], pair=pair).steps_row is None


def _stage(**kw):
    _, _, x, y = carry_pair()
    out, steps = torch.zeros(4), torch.zeros(3)
    return PostStage(env=SimpleNamespace(steps=steps), dev_index=0, out_tree=[out], out_tensors=[out],
                     carry_dst=[x], carry_src=[y], carry_other=[], carry_ys=[y], inplace=[], state_idx=0,
                     direct=[], steps_folded=True, **kw)


def test_table_cache():
    st = _stage()
    assert st.tbl is None and st.tbl_wb is None
    t = st.table()
    assert st.table() is t and st.tbl is t and st.tbl_wb is None  # the same inputs: the same table
    twb = st.table(True)
    assert twb is not t and st.table(True) is twb and st.table() is t  # cached independently
    assert twb.n_all == twb.n_out and t.n_all == t.n_out + 1  # (only the plain one carries the state)
    src = [torch.zeros(4)]
    dst = [torch.empty(4)]
    st.set_backups(src, dst)  # the backup lists replaced
    t2 = st.table()
    assert t2 is not t and t2.n_bk == 1 and st.table() is t2
    assert st.table(True) is not twb
    src.append(torch.zeros(2))  # their length changed
    dst.append(torch.empty(2))
    t3 = st.table()
    assert t3 is not t2 and t3.n_bk == 2 and st.table() is t3
    # invalidate() clears the covered record, not the tables
    st.covered = ("carry", "bk", 0)
    t3wb = st.table(True)
    st.invalidate()
    assert st.covered is None and st.table() is t3 and st.table(True) is t3wb
    assert not st.carry_current() and not st.backup_current(0)
