"""The post-replay stage of a graph-mode step (``_graph.py`` captures and replays).

After a replay, ONE native launch (vmas_copy_spans) makes the fresh copies of the step's outputs,
carries the re-bound state to the next step (Y -> X) and takes the next step's rollback backups.
What it moves is a span table (``PostTable``), built once per (capture, backup buffers) by pure
functions of addresses, sizes and contiguity (``_clone_plan``, ``_post_spans``, ``_post_table``:
they run on CPU tensors, tests/test_post_stage.py); a step only writes its fresh outputs'
addresses into it.  ``PostStage`` is what a StepGraph holds per capture: the clone plan, the two
tables (with and without the carry of the engine's state buffer, which k_world's write-back
replaces) and the record of what the last launch covered, which the StepGraph invalidates
wherever it writes a carried or backed-up tensor itself.
"""
from __future__ import annotations

import operator
from typing import Any, Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from ... import _native as N

_VERSION = operator.attrgetter("_version")  # a tensor's version counter (map() without a Python frame)


class PostTable:
    """One span table and what belongs to it."""

    __slots__ = (
        "tbl", "addr",  # the N.COPY_SPAN_DTYPE rows and their address (ndarray.ctypes.data, taken once)
        "n_out", "n_all",  # rows [0, n_out): outputs, direct words, the step counter; [n_out, n_all): carry, backups
        "plain",  # a non-contiguous carry or a straddling backup: outputs only, the rest stays with its callers
        "clash",  # an output lies in a carry destination: the outputs are launched before the carry
        "n_bk",  # backup tensors covered
        "steps_row", "steps",  # the folded `steps += 1` row (or None) and the tensor it points at
        "direct_rows",  # the row of each direct region's store word
        "contig",  # per clone group: which members are contiguous (have an output row)
        "bk_dst", "bk_lens",  # the backup lists it was built for (PostStage.table's validity check)
        "loose",  # the non-contiguous outputs as (view index, source): no row, a torch copy each
        "host",  # the OutputAlloc (csrc/vmas_host.cpp; None until the table is first used)
        "tail_ok",  # whether its items may ride the fused launch's tail (None: not judged yet)
    )


class Covered(NamedTuple):
    """What the last post-replay launch covered: the version counters of the carried Y tensors and
    of the in-place tensors as it saw them, and how many backups it took."""

    carry_ver: tuple
    bk_ver: tuple
    bk_n: int


def _clone_plan(out_tensors: List[Tensor], out_tree, direct: List[dict]):
    """Outputs grouped by (dtype, shape): per group one allocation [n, *shape] whose unbind gives
    the n fresh tensors, all filled by the post-replay copy launch; the result tree rebuilt by a
    function generated for its structure.  Built once per capture (the replay's output tensors
    are fixed), so a step makes a handful of host calls instead of several per output.
    Returns (groups [(dtype, shape, n)], group_srcs [(start, end, sources)], (fn, consts))."""
    ts = out_tensors
    dmember = {id(m): (ri, mi) for ri, r in enumerate(direct) for mi, m in enumerate(r["members"])}
    by_key: Dict[Tuple[torch.dtype, Tuple[int, ...]], List[int]] = {}
    for i, t in enumerate(ts):
        if id(t) not in dmember:  # (directly written: views of the replay's fresh buffer)
            by_key.setdefault((t.dtype, tuple(t.shape)), []).append(i)
    plan = sorted(by_key.items(), key=lambda kv: str(kv[0][0]))  # same dtypes adjacent
    groups = [(dt, shape, len(idx)) for (dt, shape), idx in plan]
    order = [i for _, idx in plan for i in idx]  # position in the concatenated views -> output
    pos = {i: p for p, i in enumerate(order)}
    # the direct categories' members follow the groups' views (OutputAlloc.alloc's order)
    base, at = [], len(order)
    for r in direct:
        base.append(at)
        at += len(r["members"])
    for i, t in enumerate(ts):
        if id(t) in dmember:
            ri, mi = dmember[id(t)]
            pos[i] = base[ri] + mi
    # per (dtype, shape) group, in view order: its sources
    group_srcs, start = [], 0
    for _, idx in plan:
        group_srcs.append((start, start + len(idx), [ts[i] for i in idx]))
        start += len(idx)
    consts: List[Any] = []
    counter = [0]

    def expr(t):
        if isinstance(t, Tensor):
            counter[0] += 1
            return f"v[{pos[counter[0] - 1]}]"
        if isinstance(t, list):
            return "[" + ", ".join(expr(x) for x in t) + "]"
        if isinstance(t, tuple):
            return "(" + "".join(expr(x) + ", " for x in t) + ")"
        if isinstance(t, dict):
            items = []
            for k, x in t.items():
                consts.append(k)
                items.append(f"c[{len(consts) - 1}]: {expr(x)}")
            return "{" + ", ".join(items) + "}"
        consts.append(t)
        return f"c[{len(consts) - 1}]"

    fn = eval("lambda v, c: " + expr(out_tree))  # noqa: S307 -- generated from the output tree's structure only
    return groups, group_srcs, (fn, consts)


def _post_spans(carry_dst, carry_src, bk_src, bk_dst, state_idx: Optional[int], wb: bool = False):
    """Per capture: the carry spans (Y -> X, contiguous byte views) and the backup spans of
    the next step (in-place tensors and the action buffer -> their backups; a backup whose
    tensor lies inside a carry destination X is taken from the matching bytes of Y, which
    is what X holds once the carry has run).  None if a backup straddles a carry destination
    or is not contiguous (then the backups stay in StepGraph.backup())."""
    carry = [(y.data_ptr(), x.data_ptr(), x.numel()) for i, (x, y) in enumerate(zip(carry_dst, carry_src))
             if not (wb and i == state_idx)]  # (wb: k_world wrote the state back itself)
    bk = []
    n = len(bk_src) if bk_dst else 0
    for t, d in zip(bk_src[:n], bk_dst[:n]):
        if not (t.is_contiguous() and d.is_contiguous()):
            return carry, None, 0
        lo, nb = t.data_ptr(), t.numel() * t.element_size()
        src = lo
        for y, x, cn in carry:
            if lo < x + cn and x < lo + nb:  # overlaps carry destination X
                if not (x <= lo and lo + nb <= x + cn):
                    return carry, None, 0
                src = y + (lo - x)
        bk.append((src, d.data_ptr(), nb))
    return carry, bk, n


def _post_table(group_srcs, carry_dst, carry_src, carry_other, bk_src, bk_dst, direct: List[dict],
                state_idx: Optional[int], steps: Optional[Tensor], wb: bool = False) -> PostTable:
    """The post-replay span table: the contiguous outputs (their destinations are filled per step
    by OutputAlloc), a store word per direct region, the folded step counter (steps: the tensor,
    or None), then the carry and backup spans."""
    out_rows = [(x.data_ptr(), 0, x.numel() * x.element_size()) for _, _, srcs in group_srcs
                for x in srcs if x.is_contiguous()]
    direct_rows = []
    for r in direct:  # (the next replay's buffer offset: written by OutputAlloc.alloc)
        direct_rows.append(len(out_rows))
        out_rows.append((0, r["word"], N.VMAS_COPY_STORE64))
    steps_row = None
    if steps is not None:  # (last output row: the launch of the outputs always covers it)
        steps_row = len(out_rows)
        out_rows.append((0, steps.data_ptr(), steps.numel() * 4))
    carry, bk, n_bk = _post_spans(carry_dst, carry_src, bk_src, bk_dst, state_idx, wb)
    plain = bool(carry_other) or bk is None
    extra = [] if plain else carry + bk
    tbl = np.zeros(len(out_rows) + len(extra), dtype=N.COPY_SPAN_DTYPE)
    for i, row in enumerate(out_rows + extra):
        tbl[i] = row
    t = PostTable()
    t.tbl, t.addr = tbl, tbl.ctypes.data
    t.n_out, t.n_all = len(out_rows), len(tbl)
    t.plain, t.n_bk = plain, n_bk
    t.clash = any(lo < x + cn and x < lo + nb for lo, _, nb in out_rows if nb > 0 for _, x, cn in carry)
    t.steps_row, t.steps = steps_row, steps
    t.direct_rows = direct_rows
    t.contig = [[x.is_contiguous() for x in srcs] for _, _, srcs in group_srcs]
    t.loose = [(start + k, x) for start, _, srcs in group_srcs for k, x in enumerate(srcs) if not x.is_contiguous()]
    t.bk_dst, t.bk_lens = bk_dst, (len(bk_dst), len(bk_src))
    t.host = t.tail_ok = None
    return t


def _steps_current(t: PostTable, st: Tensor) -> None:
    """Point the table's increment row at Environment.steps as bound now (reset() re-binds it;
    before_actions checked it: fp32, contiguous, on the device)."""
    if t.steps is not st:
        row = t.tbl[t.steps_row]
        row["dst"] = st.data_ptr()
        row["nbytes"] = st.numel() * 4
        t.steps = st


def _ahead_offset_word(deferred):
    """Where a draw made ahead in the post-replay launch reads its generator offset: 0 (the
    host passes it) without deferred launches; with one spawn channel (discovery's respawn,
    whose host side advances the generator only after this launch is queued) the device word
    the respawn launch leaves it in (VMAS_SPAWN_OFF_END_WORD); None: no draw ahead."""
    if len(deferred) != 1:
        return None if deferred else 0
    mx = getattr(getattr(deferred[0], "chan", None), "mx", None)
    return None if mx is None else mx.data_ptr() + 4 * N.VMAS_SPAWN_OFF_END_WORD


class PostStage:
    """The post-replay stage of one capture (see the module notes)."""

    def __init__(self, *, env, dev_index: int, out_tree, out_tensors, carry_dst, carry_src, carry_other,
                 carry_ys, inplace, state_idx: Optional[int], direct: List[dict], steps_folded: bool,
                 deferred=(), tail: bool = False):
        self.env, self.dev = env, dev_index
        self.carry_dst, self.carry_src, self.carry_other = carry_dst, carry_src, carry_other
        self.carry_ys, self.inplace = carry_ys, inplace  # (their version counters: the covered record)
        self.state_idx, self.steps_folded = state_idx, steps_folded
        self.direct = direct  # (DirectOutputs.enabled: the regions the replays relocate)
        self.off_dev = _ahead_offset_word(deferred)
        self.tail = tail  # (VMAS_GRAPH_TAIL and a trusted scenario: _tail_admit)
        self.bk_src, self.bk_dst = [], []  # (the rollback backups' tensors and buffers: set_backups)
        self.clone_groups, self.clone_group_srcs, self.clone_build = _clone_plan(out_tensors, out_tree, direct)
        self.tbl: Optional[PostTable] = None  # with every carry
        self.tbl_wb: Optional[PostTable] = None  # without the state carry (the write-back)
        self.covered: Optional[Covered] = None
        self._fns = None  # (entry points handed to _vmas_host: resolved with the first OutputAlloc)

    # ---- what the StepGraph tells it ------------------------------------------------------------
    def invalidate(self) -> None:
        """A carried or backed-up tensor was written outside the post-replay launch."""
        self.covered = None

    def set_backups(self, src: List[Tensor], dst: List[Tensor]) -> None:
        self.bk_src, self.bk_dst = src, dst
        self.covered = None

    def carry_current(self) -> bool:
        """The last post-replay launch carried Y -> X and no Y was modified since (version
        counters: a native replay bumps none, a caller's in-place edit or the re-bind copy of
        before_actions bumps them)."""
        c = self.covered
        return c is not None and c.carry_ver == tuple(map(_VERSION, self.carry_ys))

    def backup_current(self, n: int) -> bool:
        c = self.covered
        return (c is not None and c.bk_n >= n and self.carry_current()
                and c.bk_ver == tuple(map(_VERSION, self.inplace)))

    # ---- tables ---------------------------------------------------------------------------------
    def table(self, wb: bool = False) -> PostTable:
        """The table with (wb False) or without the state carry, rebuilt when the backup lists
        it was built for were replaced or changed length."""
        t = self.tbl_wb if wb else self.tbl
        bk_dst = self.bk_dst
        if t is not None and t.bk_dst is bk_dst and t.bk_lens == (len(bk_dst), len(self.bk_src)):
            return t
        t = _post_table(self.clone_group_srcs, self.carry_dst, self.carry_src, self.carry_other, self.bk_src, bk_dst,
                        self.direct, self.state_idx, self.env.steps if self.steps_folded else None, wb)
        if wb:
            self.tbl_wb = t
        else:
            self.tbl = t
        return t

    def _ready(self, t: PostTable) -> PostTable:
        """Before any use of a table: its steps row at the bound tensor, its OutputAlloc made."""
        if t.steps_row is not None:
            _steps_current(t, self.env.steps)
        if t.host is None:
            self._host_alloc(t)
        return t

    def _host_alloc(self, t: PostTable) -> None:
        """The table's OutputAlloc (csrc/vmas_host.cpp).  Its alloc() makes per (dtype, shape) group
        one [n, *shape] allocation, unbinds it into the group's fresh tensors, writes the contiguous
        members' addresses into the table's output rows and each direct region's next buffer offset
        into its store row; it returns the views in the plan's order."""
        groups, row = [], 0
        for (dt, shape, n), (_, _, srcs), contig in zip(self.clone_groups, self.clone_group_srcs, t.contig):
            ks = [k for k, c in enumerate(contig) if c]
            groups.append((srcs[0], list(shape), n, row, ks))
            row += len(ks)
        regions = [(r["buf"], r["box"], r["members"][0], row,
                    [(list(m.shape), list(m.stride()), m.storage_offset()) for m in r["members"]])
                   for r, row in zip(self.direct, t.direct_rows)]
        t.host = N.load_host().OutputAlloc(self.dev, groups, t.tbl, t.addr, N.fn_addr("vmas_copy_spans"),
                                           N.fn_addr("vmas_aux_last_error"), regions)
        if self._fns is None:
            self._fns = (N.fn_addr("vmas_graph_chain_launch"), N.fn_addr("vmas_graph_chain_launch_wb"),
                         N.fn_addr("vmas_graph_chain_launch_tail"), N.fn_addr("vmas_copy_spans_draw"))

    # The post-replay launch's items as the tail of the replay's one fused k_world launch
    # (csrc/vmas_tail.hpp, vmas_graph_chain_launch_tail): one launch per step instead of two.  A copy
    # then runs inside the launch that wrote its source, possibly on another XCD, so it is admitted
    # only when that source is written through: k_world's state outputs (stored sc1) and the
    # tensors a trusted scenario's program writes through (`_vmas_tail_sources()`: balance's global
    # shaping, position and ground rewards; transport's per-package distance, on-goal flag, colour and
    # shaping).  Store words and the step counter need nothing.
    def _tail_admit(self, t: PostTable, ch) -> bool:
        srcs = getattr(self.env.scenario, "_vmas_tail_sources", None)
        if not self.tail or ch.n_nodes != 1 or not ch.fused or srcs is None or t.plain:
            return False
        ranges = []
        try:
            tensors = list(srcs())
        except Exception:  # noqa: BLE001 -- (an attribute the declaration names is not bound: no tail)
            return False
        for v in tensors:
            if not isinstance(v, Tensor) or not v.is_contiguous() or v.device.type != "cuda":
                return False
            ranges.append((v.data_ptr(), v.data_ptr() + v.numel() * v.element_size()))
        if self.state_idx is not None:  # (the engine's output buffer: k_world's sc1 stores)
            y = self.carry_src[self.state_idx]
            ranges.append((y.data_ptr(), y.data_ptr() + y.numel()))
        for r in t.tbl:
            n, src = int(r["nbytes"]), int(r["src"])
            if n == N.VMAS_COPY_STORE64 or src == 0 or n == 0:
                continue
            if not any(lo <= src and src + n <= hi for lo, hi in ranges):
                return False
        return True

    # ---- the stage ------------------------------------------------------------------------------
    def prepare(self):
        """The host half of run(): (table, fresh output views); nothing is launched."""
        t = self._ready(self.table())
        return t, t.host.alloc()

    def _copy(self, t: PostTable, views, hi: int):
        """Rows [0, hi) launched from here: fresh outputs (unless prepared), the launch(es)."""
        if views is None:
            views = t.host.alloc()
        dev, st, lo = self.dev, N.stream_ptr(self.dev), 0
        if t.clash and hi > t.n_out:  # (the outputs are copied out before the carry overwrites them)
            N.copy_table_at(dev, t.addr, 0, t.n_out, st)
            lo = t.n_out
        N.copy_table_at(dev, t.addr, lo, hi, st)
        t.host.commit()
        return views

    def _finish(self, t: PostTable, views):
        """The non-contiguous outputs (a torch copy each), then the step's result tree over the views."""
        for k, s in t.loose:
            views[k].copy_(s)
        fn, consts = self.clone_build
        return fn(views, consts)

    def run(self, prep=None, chain=None, wb: bool = False):
        """After a replay, in ONE native launch (vmas_copy_spans): the fresh copies of the
        outputs, the carry of the re-bound state to the next step (Y -> X, which before_actions
        then skips while no Y changes) and the next step's backups (which backup() then skips
        while no in-place tensor changes).  The outputs are copied before the carry when one
        of them lies in a carry destination (two launches).  prep: what prepare() returned;
        chain: the replay's kernel chain, not launched yet; wb: k_world wrote the state back."""
        t, views = prep if prep is not None else (self.table(wb), None)
        if chain is not None and (t.plain or t.host is None or views is not None):
            chain.launch(wb, N.stream_ptr(self.dev))  # (it cannot ride the C++ call: now, before anything else)
            chain = None
        self._ready(t)
        if views is not None or t.plain:  # prepared, or plain (outputs only): launched from here
            views = self._copy(t, views, t.n_all)
        else:
            # the common case in one C++ call (csrc/vmas_host.cpp OutputAlloc.post): the replay's
            # kernel chain (chain: not launched yet), fresh outputs, their addresses into the table,
            # the launch(es)
            host, fns = t.host, self._fns
            ch = (chain.addr, fns[1 if wb else 0]) if chain is not None else (0, 0)
            mid, hi = (t.n_out if t.clash else 0), t.n_all
            # (with a deferred launch -- discovery's respawn, whose host side advances the generator
            # after this -- the draw reads its offset where the respawn launch leaves it)
            off_dev, env = self.off_dev, self.env
            ahead = env._draw_ahead_plan() if (hi - mid <= 96 and not t.n_bk and off_dev is not None) else None
            if ahead is not None:  # (+ the next step's random actions in the same launch)
                st, drawer, P = ahead
                tail = 0
                if ch[0] and not mid:  # (a single fused launch: these items as its tail, _tail_admit)
                    ok = t.tail_ok
                    if ok is None:
                        ok = t.tail_ok = self._tail_admit(t, chain)
                    if ok:
                        tail = fns[2]
                views, acts, snap, seed, off, inc = N.load_host().post_draw(
                    host, drawer, mid, hi, P.data_ptr(), P.numel(), fns[3], off_dev, *ch, tail, int(wb))
                env._drew_ahead(st, acts, snap, seed, off, inc)
            else:
                views = host.post(mid, hi, *ch)
        self.covered = None if t.plain else Covered(tuple(map(_VERSION, self.carry_ys)),
                                                    tuple(map(_VERSION, self.inplace)), t.n_bk)
        return self._finish(t, views)

    def clone_outputs(self):
        """Fresh copies of the replay's outputs alone (a segmented capture ran the step itself)."""
        t = self._ready(self.table())
        return self._finish(t, self._copy(t, None, t.n_out))
