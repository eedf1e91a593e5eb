"""The decode section of `mhla_amd/ops.py` (CausalState ... mhla_causal_commit) run on CPU tensors against a recording stand-in for
the library (tools/fake_decode_lib.py): every library call with every argument, every public call's effect on the state's host
mirror, every exception's type and message, and the signature and docstring hash of every public name of the section.  Plain
states, views of a dense pool, of a pool of fp32 pages and of one of h16 pages (after every call on a view: the pool's mirror, its
free pages and its table, host and device), a slot map on the device, the pack prefill `into=` a view, the pools' own methods, and
packed new tokens (`cu_seqlens=`) as one chain and cut by each of the three limits.  Two trees whose logs are byte-identical make the
same calls in the same order and refuse the same things with the same words: the check of a refactor of that section
(profiles/decode_host_refactor.md, profiles/decode_host_refactor_pools.md).

    python tools/record_decode_calls.py [--tree DIR] [-o LOG]     the log (sha256 on stderr); DIR: another checkout to import
    python tools/record_decode_calls.py --raises                  also list the `raise` lines of the section no scenario reached
    python tools/record_decode_calls.py --counts                  Python function calls per public call (cProfile), no log
"""
import argparse
import contextlib
import cProfile
import hashlib
import inspect
import itertools
import os
import pstats
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.join(HERE, ".."))
ap.add_argument("-o", "--output")
ap.add_argument("--raises", action="store_true")
ap.add_argument("--counts", action="store_true")
opt = ap.parse_args()
sys.path.insert(0, os.path.abspath(opt.tree))

import torch  # noqa: E402

import mhla_amd  # noqa: E402
from mhla_amd import CausalState, PagedCausalState, _lib, ops  # noqa: E402
from mhla_amd import build as _build  # noqa: E402
from fake_decode_lib import Session  # noqa: E402

_build.build(verbose=False)
B, K, V, CAP = 3, 16, 24, 5
PUBLIC = ("CausalState", "CausalState.empty", "CausalState.to_ragged", "CausalState.sync", "CausalState.clone", "CausalState.cat",
          "mhla_causal_prefill", "mhla_causal_state", "mhla_causal_step", "mhla_causal_step_dev", "mhla_causal_extend", "CausalDraft",
          "mhla_causal_verify", "mhla_causal_commit",
          "CausalState.at", "CausalState.reset", "CausalState.fork", "CausalStateView", "CausalStateView.compact", "CausalStateView.sync",
          "PagedCausalState", "PagedCausalState.empty", "PagedCausalState.at", "PagedCausalState.to_ragged", "PagedCausalState.clone",
          "PagedCausalState.reserve", "PagedCausalState.trim", "PagedCausalState.reset", "PagedCausalState.fork", "PagedCausalState.sync",
          "PagedStateView", "PagedStateView.compact", "PoolExhausted")
# a pool of N_SLOTS slots, of which a view takes SLOTS in that order (slots 1 and 3 belong to others and must keep every bit)
SLOTS, N_SLOTS, N_PAGES, OTHERS = (4, 0, 2), 5, 16, {1: 70, 3: 1}


def rand(*shape, dtype=torch.float32, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def tokens(dtype, H, Hk, T, k_dim=K):
    return (rand(B, T, H, k_dim, dtype=dtype, seed=1), rand(B, T, Hk, k_dim, dtype=dtype, seed=2), rand(B, T, Hk, V, dtype=dtype, seed=3),
            rand(B, T, H, V, dtype=dtype, seed=4))


def new_state(Hk, lengths=None, seen=0, k_dim=K, batch=B):
    e = CausalState.empty(batch, Hk, k_dim, V, CAP, device="cpu")
    if lengths is None:
        e.seen = seen
        return e
    return CausalState(e.S, e.P, e.Cur, 0, 64, lengths=lengths)


def name_all(s, state=None, **tensors):
    s.name(**tensors)
    if state is not None:
        s.name(S=state.S, P=state.P, Cur=state.Cur, pos=state.pos, full=state._full)


def new_pool(kind, Hk, lengths=(6, 133, 127), slots=SLOTS, k_dim=K, n_pages=N_PAGES):
    """(pool, pool.at(slots)) of one kind -- "dense", "paged" (fp32 pages) or "h16" --: the view's sequences hold `lengths`, the
    slots of `OTHERS` theirs, every chunk that holds a token has its page.  slots: a tuple, or an int32 tensor (a map on the device)."""
    host = [OTHERS.get(i, 0) for i in range(N_SLOTS)]
    for i, n in zip(SLOTS, lengths):
        host[i] = n
    if kind == "dense":
        e = CausalState.empty(N_SLOTS, Hk, k_dim, V, CAP, device="cpu")
        pool = CausalState(e.S, e.P, e.Cur, 0, 64, lengths=host)
    else:
        pool = PagedCausalState.empty(N_SLOTS, Hk, k_dim, V, CAP, n_pages, "cpu", page_format="fp32" if kind == "paged" else "h16")
        pool.reserve(range(N_SLOTS), host)
        pool._set_lengths(range(N_SLOTS), host)
        pool.pos.copy_(torch.tensor(host, dtype=torch.int32))
    return pool, pool.at(slots)


def name_pool(s, pool, view=None):
    s.name(S=pool._chunks, P=pool.P, Cur=pool.Cur, pos=pool.pos, full=pool._full, slot=view.map if view is not None else None,
           table=getattr(pool, "table_dev", None), mult=pool.page_mult)


def pool_line(s, pool):
    """The pool behind a view after a call: its host mirror and -- paged -- the free pages and the table, host and device."""
    if pool is None:
        return
    pos = None if pool.pos is None else pool.pos.tolist()
    line = f"  pool: seen={pool.seen} lengths={pool.lengths} stale={pool.stale} pos={pos} full={None if pool._full is None else pool._full.tolist()}"
    if pool.pages is not None:
        line += f" pages_free={pool.pages_free} free={sorted(pool.free)} refs={pool.refs} have={pool.have} table={pool.table} table_dev={pool.table_dev.tolist()}"
    s.lines.append(line)


@contextlib.contextmanager
def lowered(**limits):
    """Module globals of `ops` (the limits a call is cut by) set for the block."""
    saved = {n: getattr(ops, n) for n in limits}
    for n, x in limits.items():
        setattr(ops, n, x)
    try:
        yield
    finally:
        for n, x in saved.items():
            setattr(ops, n, x)


def pool_scenarios(s, tag, dtype, H, Hk):
    """Views of pools (dense, fp32 pages, h16 pages), the pack prefill `into=` them, and packed new tokens, in one configuration."""
    mix, w = torch.rand(CAP, CAP, generator=torch.Generator().manual_seed(9)), torch.rand(V, generator=torch.Generator().manual_seed(8)) + 0.5
    lengths = (6, 133, 127)

    def run(label, fn, q, k, v, pool, view, **kw):
        name_pool(s, pool, view)
        s.name(mix=mix, w=w, q=q, k=k, v=v, gate=kw.get("gate"))
        got = s.call(f"{tag} {label}", fn, q, k, v, mix, view, state=view, **kw)
        pool_line(s, pool)
        return got

    def commit(label, draft, pool, st, accept):
        got = s.call(f"{tag} {label}", mhla_amd.mhla_causal_commit, draft, mix, st, accept, state=st)
        pool_line(s, pool)
        return got

    q, k, v, g = tokens(dtype, H, Hk, 1)
    q5, k5, v5, g5 = tokens(dtype, H, Hk, 5)
    for kind in ("dense", "paged", "h16"):
        for at in (lengths, (63, 133, 127), (64, 133, 127)):   # (the last: the step opens a chunk, a paged pool gives it a page)
            run(f"{kind} view: step at {at}", mhla_amd.mhla_causal_step, q, k, v, *new_pool(kind, Hk, at), gate=g, norm_weight=w)
        pool, view = new_pool(kind, Hk)
        pool.full
        run(f"{kind} view: step_dev", mhla_amd.mhla_causal_step_dev, q, k, v, pool, view)
        run(f"{kind} view: step after step_dev (stale)", mhla_amd.mhla_causal_step, q, k, v, pool, view)
        s.call(f"{tag} {kind} view: sync", view.sync, state=view)
        pool_line(s, pool)
        if kind == "h16":
            continue
        run(f"{kind} view: extend T=5", mhla_amd.mhla_causal_extend, q5, k5, v5, *new_pool(kind, Hk), gate=g5)
        run(f"{kind} view: extend T=1", mhla_amd.mhla_causal_extend, q, k, v, *new_pool(kind, Hk))
        for counts, left in (((3, 0, 5), False), ((3, 0, 5), True), ((0, 0, 0), False)):
            run(f"{kind} view: extend counts={counts} left_padded={left}", mhla_amd.mhla_causal_extend, q5, k5, v5, *new_pool(kind, Hk, (60, 133, 127)),
                counts=counts, left_padded=left, norm_weight=w)
        for counts, left, accept in (((3, 0, 5), False, (2, 0, 0)), ((3, 0, 5), True, (3, 0, 5)), (None, False, (0, 0, 0)), (None, False, torch.tensor([5, 1, 0]))):
            pool, view = new_pool(kind, Hk, (60, 133, 127))
            got = run(f"{kind} view: verify counts={counts} left_padded={left}", mhla_amd.mhla_causal_verify, q5, k5, v5, pool, view, counts=counts,
                      left_padded=left, gate=g5)
            commit(f"{kind} view: commit accept={accept}", got[1], pool, view, accept)
    pool, _ = new_pool("dense", Hk)
    dmap = torch.tensor([4, -1, 2], dtype=torch.int32)   # (an entry outside the pool: that row is inactive)
    pool.full
    run("dense view, slot map on the device: step_dev", mhla_amd.mhla_causal_step_dev, q, k, v, pool, pool.at(dmap), gate=g)

    # ---- the pack prefill into a view
    kp, vp = rand(1, 109, Hk, K, dtype=dtype, seed=5), rand(1, 109, Hk, V, dtype=dtype, seed=6)
    for kind in ("dense", "paged", "h16"):
        for label, k_, v_, cu in (("pack", kp, vp, [0, 6, 76, 109]), ("pack with an empty sequence", kp, vp, [0, 6, 6, 109]),
                                  ("all-empty pack", kp[:, :0], vp[:, :0], [0, 0, 0, 0])):
            pool, view = new_pool(kind, Hk)
            pool.full
            name_pool(s, pool, view)
            s.name(k=kp, v=vp, mix=mix)
            s.call(f"{tag} {kind} view: state {label} into=", mhla_amd.mhla_causal_state, k_, v_, mix, cu_seqlens=cu, into=view, state=view)
            pool_line(s, pool)

    # ---- packed new tokens
    dt = ops._DTYPES[dtype]
    packs = (((0, 3, 3, 73), (2, 0, 30)), ((0, 0, 0, 70), (0, 0, 70)))   # (cu, accept); sequence 1 is empty; of the second, the first two
    ws = _lib.load().mhla_causal_extend_packed_ws_bytes(3, 73, H, Hk, K, V, ops._ragged_plan(lengths, (3, 0, 70), CAP)[1], dt)
    cuts = (("one chain", {}), ("cut by _PACK_MAX_TOKENS", dict(_PACK_MAX_TOKENS=70)), ("cut by _MAX_GRID_BH", dict(_MAX_GRID_BH=2 * H)),
            ("cut by EXTEND_WS_CAP_BYTES", dict(EXTEND_WS_CAP_BYTES=ws - 1)))
    for kind in ("plain", "dense", "paged"):
        fresh = lambda: (None, new_state(Hk, lengths)) if kind == "plain" else new_pool(kind, Hk)

        def packed(label, fn, cu, pool, st, **kw):
            n = cu[-1]
            qn, kn, vn, gn = (rand(1, n, h, d, dtype=dtype, seed=20 + i) for i, (h, d) in enumerate(((H, K), (Hk, K), (Hk, V), (H, V))))
            if pool is None:
                name_all(s, st)
            else:
                name_pool(s, pool, st)
            s.name(mix=mix, w=w, q=qn, k=kn, v=vn, gate=gn)
            got = s.call(f"{tag} {kind}: {label} cu={cu}", fn, qn, kn, vn, mix, st, state=st, cu_seqlens=cu, gate=gn, **kw)
            pool_line(s, pool)
            return got

        for what, limits in cuts:
            for cu, accept in packs:
                with lowered(**limits):
                    packed(f"packed extend, {what}", mhla_amd.mhla_causal_extend, cu, *fresh(), norm_weight=w)
                    pool, st = fresh()
                    got = packed(f"packed verify, {what}", mhla_amd.mhla_causal_verify, cu, pool, st)
                    if got is not None:
                        commit(f"{kind}: packed commit accept={accept}, {what}", got[1], pool, st, accept)
        packed("packed extend, all-empty pack", mhla_amd.mhla_causal_extend, (0, 0, 0, 0), *fresh())
        pool, st = fresh()
        got = packed("packed verify, all-empty pack", mhla_amd.mhla_causal_verify, (0, 0, 0, 0), pool, st)
        commit(f"{kind}: packed commit of nothing", got[1], pool, st, (0, 0, 0))
        pool, st = fresh()
        got = packed("packed verify, every draft rejected", mhla_amd.mhla_causal_verify, packs[0][0], pool, st)
        commit(f"{kind}: packed commit accept all zero", got[1], pool, st, (0, 0, 0))


def pool_methods(s):
    """The methods of the pools themselves, the free pages, the table and the host mirror after each."""
    Hk = 2

    def call(pool, label, fn, *a, **kw):
        got = s.call(f"pool methods: {label}", fn, *a, **kw)
        pool_line(s, pool)
        return got

    for kind in ("dense", "paged", "h16"):
        pool, view = new_pool(kind, Hk, (70, 133, 127))
        pool.full
        name_pool(s, pool, view)
        if kind != "dense":
            call(pool, f"{kind} reserve", pool.reserve, (1, 3), 200)
            call(pool, f"{kind} reserve per slot", pool.reserve, [4, 2], torch.tensor([320, 0]))
            call(pool, f"{kind} trim", pool.trim, (1, 4))
        call(pool, f"{kind} fork", pool.fork, 0, 3)
        call(pool, f"{kind} fork onto a longer slot", pool.fork, 3, 1)
        call(pool, f"{kind} reset", pool.reset, [0, 2])
        if kind != "dense":
            call(pool, f"{kind} trim after the reset", pool.trim, range(N_SLOTS))
        for name in ("compact", "clone"):
            got = call(pool, f"{kind} view.{name}", getattr(view, name))
            s.lines.append(f"  {name}: S {tuple(got.S.shape)} {got.S.dtype} pos={got.pos.tolist()} full={got._full.tolist()}")
        pool._full[1] = 1
        pool.stale = True
        call(pool, f"{kind} sync with a full flag", pool.sync)
        call(pool, f"{kind} to_ragged is the pool", lambda: pool.to_ragged() is pool)
        call(pool, f"{kind} view.to_ragged is the view", lambda: view.to_ragged() is view)
        s.lines.append(f"  nbytes={pool.nbytes} dims={pool.dims} capacity_chunks={pool.capacity_chunks} view: rows={view.rows} dims={view.dims} "
                       f"capacity_chunks={view.capacity_chunks} {view!r}")
    st = new_state(Hk, (6, 133, 127))
    dense, dview = new_pool("dense", Hk)
    paged, pview = new_pool("paged", Hk)
    call(None, "cat of a state and two views", lambda: _named_state(s, CausalState.cat([st, dview, pview])))


def scenarios(s, tag, dtype, H, Hk):
    """Every scenario of one (heads, dtype, grid limit) configuration; every call on a fresh state."""
    mix, w = torch.rand(CAP, CAP, generator=torch.Generator().manual_seed(9)), torch.rand(V, generator=torch.Generator().manual_seed(8)) + 0.5
    ws64 = _lib.load().mhla_causal_extend_ragged_gqa_ws_bytes(B, 64, H, Hk, K, V, 1, 0)

    def run(label, fn, q, k, v, state, *, names=None, **kw):
        name_all(s, state, mix=mix, w=w, **(names or dict(q=q, k=k, v=v)), gate=kw.get("gate"))
        return s.call(f"{tag} {label}", fn, q, k, v, mix, state, state=state, **kw)

    # ---- mhla_causal_state
    _, k70, v70, _ = tokens(dtype, H, Hk, 70)
    for label, kw in (("uniform", {}), ("lengths", dict(lengths=(6, 70, 33))), ("lengths left-padded", dict(lengths=[6, 70, 33], left_padded=True)),
                      ("lengths tensor with zero", dict(lengths=torch.tensor([0, 70, 70]))), ("capacity 3", dict(capacity_chunks=3))):
        s.name(k=k70, v=v70, mix=mix)
        s.call(f"{tag} state {label}", lambda **kw: _named_state(s, mhla_amd.mhla_causal_state(k70, v70, mix, **kw)), **kw)
    s.call(f"{tag} state T=0", mhla_amd.mhla_causal_state, k70[:, :0], v70[:, :0], mix)
    kp, vp = rand(1, 109, Hk, K, dtype=dtype, seed=5), rand(1, 109, Hk, V, dtype=dtype, seed=6)
    s.name(k=kp, v=vp, mix=mix)
    s.call(f"{tag} state cu_seqlens", lambda: _named_state(s, mhla_amd.mhla_causal_state(kp, vp, mix, cu_seqlens=[0, 6, 76, 76, 109])))

    # ---- mhla_causal_step
    q, k, v, g = tokens(dtype, H, Hk, 1)
    for pos in (5, 63):
        run(f"step uniform at {pos}", mhla_amd.mhla_causal_step, q, k, v, new_state(Hk, seen=pos))
    run("step ragged", mhla_amd.mhla_causal_step, q, k, v, new_state(Hk, (6, 133, 127)))
    packed = rand(B, 1, H * K + Hk * K + Hk * V, dtype=dtype, seed=7)
    qs, ks, vs = (t.unflatten(2, (h, -1)) for t, h in zip(packed.split((H * K, Hk * K, Hk * V), dim=2), (H, Hk, Hk)))
    for lengths in (None, (6, 133, 127)):
        run(f"step strided views lengths={lengths}", mhla_amd.mhla_causal_step, qs, ks, vs, new_state(Hk, lengths, seen=5), names=dict(qkv=packed))
    wide = rand(B, 1, H, K + 1, dtype=dtype, seed=10)
    for lengths in (None, (6, 133, 127)):
        run(f"step copied view lengths={lengths}", mhla_amd.mhla_causal_step, wide[..., :K], k, v, new_state(Hk, lengths, seen=5), names=dict(qwide=wide, k=k, v=v))
    for gate, nw, epi in itertools.product((None, g), (None, w), (None, True, False)):
        for lengths in (None, (6, 133, 127)):
            run(f"step gate={gate is not None} norm_weight={nw is not None} epilogue={epi} lengths={lengths}", mhla_amd.mhla_causal_step, q, k, v,
                new_state(Hk, lengths, seen=5), gate=gate, norm_weight=nw, epilogue=epi, norm_eps=1e-6, scale=0.5)
    run("step bf16 norm weight", mhla_amd.mhla_causal_step, q, k, v, new_state(Hk, (6, 133, 127)), norm_weight=w.to(torch.bfloat16))

    # ---- mhla_causal_step_dev
    ang = torch.outer(torch.arange(64 * CAP, dtype=torch.float32), 1.0 / (10000 ** (torch.arange(0, K, 2, dtype=torch.float32) / K)))
    rot = (torch.cos(ang).to(dtype), torch.sin(ang).to(dtype))
    both = torch.stack((torch.cos(ang), torch.sin(ang)), dim=2).to(dtype)   # (interleaved tables: made contiguous by the call)
    for label, kw in (("bare", {}), ("feature_map", dict(feature_map="relu")), ("rotary", dict(rotary=rot)),
                      ("feature_map and rotary", dict(feature_map="elu", rotary=rot, gate=g, norm_weight=w)),
                      ("rotary interleaved", dict(rotary=(both[..., 0], both[..., 1])))):
        st = new_state(Hk, (6, 133, 127))
        st.full
        s.name(cos=rot[0], sin=rot[1], both=both)
        run(f"step_dev {label}", mhla_amd.mhla_causal_step_dev, q, k, v, st, **kw)
    run("step after step_dev (stale)", mhla_amd.mhla_causal_step, q, k, v, st)
    s.call(f"{tag} sync", st.sync, state=st)

    # ---- mhla_causal_extend
    for T in (1, 2, 70):
        qT, kT, vT, gT = tokens(dtype, H, Hk, T)
        run(f"extend T={T} uniform", mhla_amd.mhla_causal_extend, qT, kT, vT, new_state(Hk, seen=5))
        run(f"extend T={T} ragged equal", mhla_amd.mhla_causal_extend, qT, kT, vT, new_state(Hk, (6, 6, 6)), gate=gT)
        run(f"extend T={T} ragged equal pairs", mhla_amd.mhla_causal_extend, qT, kT, vT, new_state(Hk, (6, 6, 70)))
        run(f"extend T={T} ragged unequal", mhla_amd.mhla_causal_extend, qT, kT, vT, new_state(Hk, (6, 133, 127)), norm_weight=w)
    for counts, left in (((3, 0, 70), False), ((3, 0, 70), True), (torch.tensor([0, 0, 0]), False), ((0, 0, 64), True)):
        run(f"extend counts={counts} left_padded={left}", mhla_amd.mhla_causal_extend, qT, kT, vT, new_state(Hk, (6, 133, 127)), counts=counts,
            left_padded=left, gate=gT)
    q2, k2, v2, g2 = tokens(dtype, H, Hk, 200)
    for cap, what in ((1, "cap 1"), (ws64, "cap of a 64-token window")):
        saved, ops.EXTEND_WS_CAP_BYTES = ops.EXTEND_WS_CAP_BYTES, cap
        try:
            run(f"extend T=200 uniform, {what}", mhla_amd.mhla_causal_extend, q2, k2, v2, new_state(Hk, seen=5), gate=g2)
            run(f"extend T=200 ragged equal pairs, {what}", mhla_amd.mhla_causal_extend, q2, k2, v2, new_state(Hk, (6, 6, 70)))
            run(f"extend T=70 ragged unequal, {what}", mhla_amd.mhla_causal_extend, qT, kT, vT, new_state(Hk, (6, 133, 127)), gate=gT)
            for left in (False, True):
                run(f"extend counts left_padded={left}, {what}", mhla_amd.mhla_causal_extend, qT, kT, vT, new_state(Hk, (6, 133, 127)),
                    counts=(3, 0, 70), left_padded=left, gate=gT, norm_weight=w)
                run(f"extend T=200 counts left_padded={left}, {what}", mhla_amd.mhla_causal_extend, q2, k2, v2, new_state(Hk, (6, 100, 0)),
                    counts=(3, 0, 200), left_padded=left)
            run(f"verify, {what}", mhla_amd.mhla_causal_verify, qT, kT, vT, new_state(Hk, (6, 133, 127)))
        finally:
            ops.EXTEND_WS_CAP_BYTES = saved

    # ---- mhla_causal_verify, mhla_causal_commit
    q5, k5, v5, g5 = tokens(dtype, H, Hk, 5)
    for counts, left, accepts in (((3, 0, 5), False, ((2, 0, 0), (0, 0, 0), (3, 0, 5))), ((3, 0, 5), True, ((0, 0, 5), torch.tensor([3, 0, 1]))),
                                  (None, False, ((5, 5, 5),)), ((0, 0, 0), False, ((0, 0, 0),))):
        for accept in accepts:
            st = new_state(Hk, (60, 133, 127))
            got = run(f"verify counts={counts} left_padded={left}", mhla_amd.mhla_causal_verify, q5, k5, v5, st, counts=counts, left_padded=left,
                      gate=g5, norm_weight=w)
            s.call(f"{tag} commit accept={accept}", mhla_amd.mhla_causal_commit, got[1], mix, st, accept, state=st)
    st = new_state(Hk, (60, 133, 127))
    got = run("verify copied view", mhla_amd.mhla_causal_verify, rand(B, 5, H, K + 1, dtype=dtype, seed=11)[..., :K], rand(B, 5, Hk, K + 1, dtype=dtype, seed=12)[..., :K],
              v5, st, names=dict(v=v5))
    s.name(draft_k=got[1].k)
    s.call(f"{tag} commit of the copies",mhla_amd.mhla_causal_commit, got[1], mix, st, (1, 2, 3), state=st)


def _named_state(s, state):
    s.name(S=state.S, P=state.P, Cur=state.Cur, pos=state.pos)
    return state


def refusals(s):
    """Every `raise` of the section, once at least (H = 4, Hkv = 2, fp32 unless the refusal is about something else)."""
    H, Hk = 4, 2
    mix, w = torch.rand(CAP, CAP), torch.rand(V)
    meta = torch.device("meta")
    q, k, v, g = tokens(torch.float32, H, Hk, 1)
    q5, k5, v5, g5 = tokens(torch.float32, H, Hk, 5)
    rag = lambda *a, **kw: new_state(Hk, (6, 133, 127), *a, **kw)
    call = lambda label, fn, *a, **kw: s.call(f"refusal: {label}", fn, *a, **kw)
    e = CausalState.empty(B, Hk, K, V, CAP, device="cpu")
    # CausalState
    call("pos dtype", CausalState, e.S, e.P, e.Cur, lengths=(1, 2, 3), pos=torch.zeros(3))
    call("pos shape", CausalState, e.S, e.P, e.Cur, lengths=(1, 2, 3), pos=torch.zeros(2, dtype=torch.int32))
    call("pos without lengths", CausalState, e.S, e.P, e.Cur, pos=torch.zeros(3, dtype=torch.int32))
    call("lengths count", CausalState, e.S, e.P, e.Cur, lengths=(1, 2))
    call("lengths negative", CausalState, e.S, e.P, e.Cur, lengths=torch.tensor([1, -2, 3]))
    call("empty size", CausalState.empty, B, 0, K, V, CAP, "cpu")
    st = rag()
    st._full = torch.tensor([0, 1, 1], dtype=torch.int32)
    call("sync over capacity", st.sync, state=st)
    call("cat of nothing", CausalState.cat, [])
    call("cat of another thing", CausalState.cat, [e, 3])
    call("cat of differing states", CausalState.cat, [e, CausalState.empty(B, Hk, K, V, CAP + 1, device="cpu")])
    st = rag()
    st.stale = True
    call("cat of a stale state", CausalState.cat, [e, st])
    for fn, T in ((mhla_amd.mhla_causal_step, 1), (mhla_amd.mhla_causal_extend, 5), (mhla_amd.mhla_causal_verify, 5)):
        call(f"stale state, {fn.__name__}", fn, *tokens(torch.float32, H, Hk, T)[:3], mix, st, state=st)
    call("stale state, commit", mhla_amd.mhla_causal_commit, ops.CausalDraft(k5, v5, (5, 5, 5), False, st.lengths), mix, st, (1, 1, 1), state=st)
    # prefill, state
    call("prefill rank", mhla_amd.mhla_causal_prefill, q[0], k, v, mix)
    call("prefill chunk size", mhla_amd.mhla_causal_prefill, q, k, v, mix, 32)
    call("prefill lengths", mhla_amd.mhla_causal_prefill, q5, k5, v5, mix, lengths=(1, 2, 9))
    k70, v70 = tokens(torch.float32, H, Hk, 70)[1:3]
    kp, vp = k70[:1], v70[:1]
    call("pack rank", mhla_amd.mhla_causal_state, kp[0], vp, mix, cu_seqlens=[0, 70])
    call("pack with lengths", mhla_amd.mhla_causal_state, kp, vp, mix, cu_seqlens=[0, 70], lengths=(70,))
    call("pack left-padded", mhla_amd.mhla_causal_state, kp, vp, mix, cu_seqlens=[0, 70], left_padded=True)
    call("pack v shape", mhla_amd.mhla_causal_state, kp, vp[:, :5], mix, cu_seqlens=[0, 70])
    call("pack capacity 0", mhla_amd.mhla_causal_state, kp, vp, mix, cu_seqlens=[0, 70], capacity_chunks=0)
    call("pack of no sequence", mhla_amd.mhla_causal_state, kp[:, :0], vp[:, :0], mix, cu_seqlens=[0])
    saved, ops._MAX_GRID_BH = ops._MAX_GRID_BH, Hk
    call("pack beyond the grid", mhla_amd.mhla_causal_state, kp, vp, mix, cu_seqlens=[0, 6, 70])
    ops._MAX_GRID_BH = saved
    call("pack beyond the capacity", mhla_amd.mhla_causal_state, kp, vp, mix, cu_seqlens=[0, 1, 70], capacity_chunks=1)
    call("pack narrow matrix", mhla_amd.mhla_causal_state, kp, vp, torch.rand(CAP, 1), cu_seqlens=[0, 6, 70])
    call("pack matrix elsewhere", mhla_amd.mhla_causal_state, kp, vp, torch.rand(CAP, CAP, device=meta), cu_seqlens=[0, 6, 70])
    call("state rank", mhla_amd.mhla_causal_state, k70[0], v70, mix)
    call("state v shape", mhla_amd.mhla_causal_state, k70, v70[:, :5], mix)
    call("state v dtype", mhla_amd.mhla_causal_state, k70, v70.double(), mix)
    call("state lengths count", mhla_amd.mhla_causal_state, k70, v70, mix, lengths=(1, 2))
    call("state lengths beyond T", mhla_amd.mhla_causal_state, k70, v70, mix, lengths=(1, 2, 71))
    call("state capacity 6", mhla_amd.mhla_causal_state, k70, v70, mix, capacity_chunks=6)
    call("state beyond the capacity", mhla_amd.mhla_causal_state, k70, v70, mix, capacity_chunks=1)
    call("state narrow matrix", mhla_amd.mhla_causal_state, k70, v70, torch.rand(CAP, 1))
    call("state matrix elsewhere", mhla_amd.mhla_causal_state, k70, v70, torch.rand(CAP, CAP, device=meta))
    call("state dtype", mhla_amd.mhla_causal_state, k70.double(), v70.double(), mix)
    # the entry check, for each of the four
    for fn, T in ((mhla_amd.mhla_causal_step, 1), (mhla_amd.mhla_causal_step_dev, 1), (mhla_amd.mhla_causal_extend, 5), (mhla_amd.mhla_causal_verify, 5)):
        qT, kT, vT, _ = tokens(torch.float32, H, Hk, T)
        call(f"{fn.__name__} state type", fn, qT, kT, vT, mix, (1, 2))
        call(f"{fn.__name__} rank", fn, qT, kT[0], vT, mix, rag())
        call(f"{fn.__name__} T=2 or 0", fn, *tokens(torch.float32, H, Hk, 2 if T == 1 else 0)[:3], mix, rag())
    # _decode_prepare, through each of the four (the order of refusals is the order of these calls)
    for fn, T in ((mhla_amd.mhla_causal_step, 1), (mhla_amd.mhla_causal_step_dev, 1), (mhla_amd.mhla_causal_extend, 5), (mhla_amd.mhla_causal_verify, 5)):
        qT, kT, vT, gT = tokens(torch.float32, H, Hk, T)
        n = fn.__name__
        call(f"{n} heads", fn, qT, tokens(torch.float32, H, 3, T)[1], vT, mix, new_state(3, (6, 133, 127)))
        call(f"{n} too many heads per k/v head", fn, rand(B, T, 9, K), rand(B, T, 1, K), rand(B, T, 1, V), mix, new_state(1, (6, 133, 127)))
        call(f"{n} v shape", fn, qT, kT, rand(B, T, H, V), mix, rag())
        call(f"{n} gate shape", fn, qT, kT, vT, mix, rag(), gate=gT[:, :, :Hk])
        call(f"{n} k dtype", fn, qT, kT.to(torch.bfloat16), vT, mix, rag())
        call(f"{n} k elsewhere", fn, qT, kT.to(meta), vT, mix, rag())
        call(f"{n} dtype", fn, qT.double(), kT.double(), vT.double(), mix, rag())
        call(f"{n} state shape", fn, qT, kT, vT, mix, new_state(H, (6, 133, 127)))
        call(f"{n} uniform state shape", fn, qT, kT, vT, mix, new_state(H, seen=5))
        call(f"{n} matrix elsewhere", fn, qT, kT, vT, torch.rand(CAP, CAP, device=meta), rag())
        call(f"{n} norm weight elsewhere", fn, qT, kT, vT, mix, rag(), norm_weight=w.to(meta))
        st = rag()
        st.P = st.P.to(meta)
        call(f"{n} state.P elsewhere", fn, qT, kT, vT, mix, st)
        call(f"{n} norm weight size", fn, qT, kT, vT, mix, rag(), norm_weight=torch.rand(V + 1))
        call(f"{n} requires grad", fn, qT, kT.clone().requires_grad_(), vT, mix, rag())
        call(f"{n} matrix rank", fn, qT, kT, vT, torch.rand(CAP), rag())
        call(f"{n} matrix narrower than its rows", fn, qT, kT, vT, torch.rand(CAP, 2), rag())
        st = rag()
        st.chunk_size = 32
        call(f"{n} chunk size", fn, qT, kT, vT, mix, st)
        call(f"{n} matrix rows", fn, qT, kT, vT, torch.rand(2, 2), rag())
        call(f"{n} uniform matrix rows", fn, qT, kT, vT, torch.rand(2, 2), new_state(Hk, seen=130))
        call(f"{n} capacity", fn, qT, kT, vT, torch.rand(8, 8), new_state(Hk, (6, 133, 320)))
        call(f"{n} uniform capacity", fn, qT, kT, vT, torch.rand(8, 8), new_state(Hk, seen=320))
        call(f"{n} epilogue=False with a gate", fn, qT, kT, vT, mix, rag(), gate=gT, epilogue=False)
        z = torch.zeros(B, Hk, CAP, V, K).transpose(3, 4)
        call(f"{n} state contiguity", fn, qT, kT, vT, mix, CausalState(z, e.P, e.Cur, 0, 64, lengths=(6, 133, 127)))
        st = rag()
        st.pos = st.pos.to(torch.int64)
        call(f"{n} pos dtype", fn, qT, kT, vT, mix, st)
    # the step's own row test against _ragged_slices': lengths (63, 100) ask the step for row 2 and the plan for row 1
    two = torch.rand(2, 2)
    call("step closes a chunk beyond the matrix", mhla_amd.mhla_causal_step, q, k, v, two, new_state(Hk, (63, 100, 5)))
    call("extend counts of one on the same state", mhla_amd.mhla_causal_extend, q, k, v, two, new_state(Hk, (63, 100, 5)), counts=(1, 1, 1))
    call("extend counts beyond the matrix columns", mhla_amd.mhla_causal_extend, *tokens(torch.float32, H, Hk, 28)[:3], torch.rand(3, 2), new_state(Hk, (63, 100, 5)),
         counts=(1, 28, 0))
    # mhla_causal_step_dev
    dev = mhla_amd.mhla_causal_step_dev
    call("step_dev uniform state", dev, q, k, v, mix, new_state(Hk, seen=5))
    call("step_dev matrix below the capacity", dev, q, k, v, torch.rand(CAP - 1, CAP), rag())
    good = torch.zeros(64 * CAP, K // 2)
    for label, t in (("rows", good[:-1]), ("rank", good[0]), ("dtype", good.double()), ("elsewhere", good.to(meta)), ("columns", good[:, :-1])):
        call(f"step_dev rotary cos {label}", dev, q, k, v, mix, rag(), rotary=(t, good))
        call(f"step_dev rotary sin {label}", dev, q, k, v, mix, rag(), rotary=(good, t))
    q12, k12, v12, _ = tokens(torch.float32, H, Hk, 1, k_dim=12)
    call("step_dev K % 8 with a feature map", dev, q12, k12, v12, mix, new_state(Hk, (6, 133, 127), k_dim=12), feature_map="relu")
    call("step_dev K % 8 with rotary", dev, q12, k12, v12, mix, new_state(Hk, (6, 133, 127), k_dim=12), rotary=(torch.zeros(64 * CAP, 6), torch.zeros(64 * CAP, 6)))
    call("step_dev feature map", dev, q, k, v, mix, rag(), feature_map="gelu")
    capturing, torch.cuda.is_current_stream_capturing = torch.cuda.is_current_stream_capturing, lambda: True
    call("step_dev state.full under capture", dev, q, k, v, mix, rag())
    torch.cuda.is_current_stream_capturing = capturing
    # counts
    for fn in (mhla_amd.mhla_causal_extend, mhla_amd.mhla_causal_verify):
        n = fn.__name__
        call(f"{n} counts count", fn, q5, k5, v5, mix, rag(), counts=(1, 2))
        call(f"{n} counts beyond T", fn, q5, k5, v5, mix, rag(), counts=torch.tensor([1, 6, 0]))
        call(f"{n} counts negative", fn, q5, k5, v5, mix, rag(), counts=(1, -1, 0))
        call(f"{n} counts on a uniform state", fn, q5, k5, v5, mix, new_state(Hk, seen=5), counts=(1, 2, 3))
        call(f"{n} counts, state of another batch", fn, q5, k5, v5, mix, new_state(Hk, (6, 133), batch=2), counts=(1, 2, 3))
        call(f"{n} counts matrix rank", fn, q5, k5, v5, torch.rand(CAP), rag(), counts=(1, 2, 3))
        call(f"{n} counts matrix rows", fn, q5, k5, v5, torch.rand(2, 2), rag(), counts=(1, 2, 3))
        call(f"{n} counts capacity", fn, q5, k5, v5, torch.rand(8, 8), new_state(Hk, (6, 133, 318)), counts=(1, 0, 3))
    # commit
    commit = mhla_amd.mhla_causal_commit
    st = rag()
    draft = ops.CausalDraft(k5, v5, (3, 0, 5), False, st.lengths)
    call("commit draft type", commit, (k5, v5), mix, st, (1, 0, 1))
    call("commit state type", commit, draft, mix, None, (1, 0, 1))
    call("commit uniform state", commit, draft, mix, new_state(Hk, seen=5), (1, 0, 1))
    call("commit accept count", commit, draft, mix, st, (1, 0))
    call("commit accept beyond the counts", commit, draft, mix, st, (1, 1, 1))
    call("commit accept negative", commit, draft, mix, st, torch.tensor([1, 0, -1]))
    call("commit state moved", commit, draft, mix, new_state(Hk, (6, 133, 128)), (1, 0, 1))
    call("commit state shape", commit, draft, mix, new_state(H, (6, 133, 127)), (1, 0, 1))
    call("commit matrix rank", commit, draft, torch.rand(CAP), st, (1, 0, 1))
    call("commit matrix elsewhere", commit, draft, torch.rand(CAP, CAP, device=meta), st, (1, 0, 1))
    call("commit matrix columns", commit, ops.CausalDraft(k5, v5, (3, 0, 5), False, (6, 133, 127)), torch.rand(CAP, 2), st, (1, 0, 3))
    call("commit matrix rows", commit, ops.CausalDraft(k5, v5, (3, 0, 5), False, (6, 133, 127)), torch.rand(2, CAP), st, (1, 0, 3))
    call("commit dtype", commit, ops.CausalDraft(k5.double(), v5.double(), (3, 0, 5), False, (6, 133, 127)), mix, st, (1, 0, 3))
    pool_refusals(s, call, H, Hk, mix)


def pool_refusals(s, call, H, Hk, mix):
    """The refusals of the pools, their views, the pack prefill `into=` and packed new tokens; after each on a paged view, the pool."""
    q, k, v, g = tokens(torch.float32, H, Hk, 1)
    q5, k5, v5, g5 = tokens(torch.float32, H, Hk, 5)
    step, dev, extend, verify, commit = (mhla_amd.mhla_causal_step, mhla_amd.mhla_causal_step_dev, mhla_amd.mhla_causal_extend,
                                         mhla_amd.mhla_causal_verify, mhla_amd.mhla_causal_commit)
    draft5 = lambda lengths, view=None, cu=None: ops.CausalDraft(k5, v5, (3, 0, 5), False, lengths, view, cu)
    # slots
    dense, dview = new_pool("dense", Hk)
    for label, slots in (("a bool", [0, True]), ("a float", [0, 1.0]), ("none", []), ("outside", [0, 5, -1]), ("twice", [1, 0, 1, 0])):
        call(f"at: slots {label}", dense.at, slots)
    call("at on a uniform state", new_state(Hk, seen=5).at, [0])
    call("reset on a uniform state", new_state(Hk, seen=5).reset, [0])
    call("fork on a stale pool", _stale(new_pool("dense", Hk)[0]).fork, 0, 1)
    call("fork: slot outside", dense.fork, 0, 9)
    call("a view of a view", ops.CausalStateView, dview, [0])
    call("view.at", dview.at, [0])
    call("view.reset", dview.reset, [0])
    call("view.fork", dview.fork, 0, 1)
    for label, t in (("int64", torch.tensor([0, 1])), ("rank", torch.zeros(1, 2, dtype=torch.int32)), ("empty", torch.zeros(0, dtype=torch.int32)),
                     ("elsewhere", torch.zeros(2, dtype=torch.int32, device="meta")), ("strided", torch.zeros(4, dtype=torch.int32)[::2])):
        call(f"at: a device map, {label}", dense.at, t)
    # a slot map on the device goes to step_dev alone
    for kind in ("dense", "paged"):
        pool, _ = new_pool(kind, Hk)
        onDev = pool.at(torch.tensor([4, 0, 2], dtype=torch.int32))
        call(f"{kind} device map, step", step, q, k, v, mix, onDev, state=onDev)
        call(f"{kind} device map, extend", extend, q5, k5, v5, mix, onDev, state=onDev)
        call(f"{kind} device map, extend cu_seqlens", extend, q5[:1], k5[:1], v5[:1], mix, onDev, state=onDev, cu_seqlens=(0, 2, 2, 5))
        call(f"{kind} device map, verify", verify, q5, k5, v5, mix, onDev, state=onDev)
        call(f"{kind} device map, commit", commit, draft5((6, 133, 127), onDev), mix, onDev, (1, 0, 1), state=onDev)
        call(f"{kind} device map, compact", onDev.compact)
        call(f"{kind} device map, state into=", mhla_amd.mhla_causal_state, k5[:1], v5[:1], mix, cu_seqlens=(0, 2, 2, 5), into=onDev)
        call(f"{kind} device map, cat", CausalState.cat, [onDev])
        pool_line(s, pool)
    # the paged pool's constructor
    P_ = PagedCausalState
    pg, sl, tab = (lambda n=4: torch.zeros(n, Hk, K, V)), (lambda n=2: torch.zeros(n, Hk, K, V)), [[-1] * CAP, [-1] * CAP]
    call("paged: pages rank", P_, pg()[0], sl(), sl(), tab)
    call("paged: P against pages", P_, pg(), torch.zeros(2, Hk, K, V + 1), sl(), tab)
    call("paged: P against Cur", P_, pg(), sl(), sl(3), tab)
    call("paged: dtype", P_, pg().double(), sl(), sl(), tab)
    call("paged: contiguity", P_, pg(), torch.zeros(2, Hk, V, K).transpose(2, 3), torch.zeros(2, Hk, V, K).transpose(2, 3), tab)
    call("paged: elsewhere", P_, pg(), sl().to("meta"), sl().to("meta"), tab)
    call("paged: no slot", P_, pg(), sl(0), sl(0), [])
    call("paged: no page", P_, pg(0), sl(), sl(), tab)
    call("paged: table rows", P_, pg(), sl(), sl(), tab[:1])
    call("paged: table of no entries", P_, pg(), sl(), sl(), [[], []])
    call("paged: table rows of differing lengths", P_, pg(), sl(), sl(), torch.full((2, CAP), -1).tolist()[:1] + [[-1] * (CAP - 1)])
    call("paged: table entries not ints", P_, pg(), sl(), sl(), [[0.5, True, -1, -1, -1], [-1] * CAP])
    call("paged: table entries outside", P_, pg(), sl(), sl(), torch.tensor([[4, -2, -1, -1, -1], [0, -1, -1, -1, -1]]))
    call("paged: a page twice in a slot", P_, pg(), sl(), sl(), [[1, 1, -1, 2, 2], [1, -1, -1, -1, -1]])
    call("paged: lengths count", P_, pg(), sl(), sl(), tab, lengths=(1,))
    call("paged: lengths beyond the capacity", P_, pg(), sl(), sl(), tab, lengths=(64 * CAP + 1, 0))
    call("paged: tokens without a page", P_, pg(), sl(), sl(), [[0, -1, 1, -1, -1], [-1] * CAP], lengths=(130, 1))
    h16, mult = (lambda kk=K: torch.zeros(4, Hk, kk, V, dtype=torch.float16)), torch.zeros(4, Hk, K * V // 64)
    call("paged h16: K V % 64", P_, h16(3), torch.zeros(2, Hk, 3, V), torch.zeros(2, Hk, 3, V), tab, page_mult=mult)
    call("paged h16: no page_mult", P_, h16(), sl(), sl(), tab)
    call("paged h16: fp32 pages with a page_mult", P_, pg(), sl(), sl(), tab, page_mult=mult)
    call("paged h16: page_mult dtype", P_, h16(), sl(), sl(), tab, page_mult=mult.double())
    call("paged h16: page_mult shape", P_, h16(), sl(), sl(), tab, page_mult=mult[:, :, :-1])
    call("paged h16: page_mult strided", P_, h16(), sl(), sl(), tab, page_mult=torch.zeros(4, Hk, K * V // 32)[..., ::2])
    call("paged h16: page_mult elsewhere", P_, h16(), sl(), sl(), tab, page_mult=mult.to("meta"))
    call("paged h16: P dtype", P_, h16(), sl().double(), sl().double(), tab, page_mult=mult)
    call("paged.empty: size", P_.empty, 2, Hk, K, V, CAP, 0, "cpu")
    call("paged.empty: page format", P_.empty, 2, Hk, K, V, CAP, 4, "cpu", page_format="bf16")
    call("paged.empty: h16 K V % 64", P_.empty, 2, Hk, 3, V, CAP, 4, "cpu", page_format="h16")
    # the paged pool's methods
    paged, pview = new_pool("paged", Hk, n_pages=9)   # (every page is taken: 3 + 2 + 2 + 1 + 1)
    call("paged.clone", paged.clone)
    call("paged.reserve: slots", paged.reserve, [0, 0], 5)
    call("paged.reserve: tokens count", paged.reserve, [0, 1], [5])
    call("paged.reserve: tokens negative", paged.reserve, [0, 1], [5, -1])
    call("paged.reserve: beyond the capacity", paged.reserve, [0, 1], 64 * CAP + 1)
    call("paged.reserve: pool exhausted", paged.reserve, [4, 1], [64, 129])
    pool_line(s, paged)
    call("paged.trim on a stale pool", _stale(new_pool("paged", Hk)[0]).trim, [0])
    call("paged.reset: slot outside", paged.reset, [5])
    call("paged view.S", lambda: pview.S)
    # a paged pool where a state is expected, and a full one
    for label, fn, a in (("step", step, (q, k, v)), ("step_dev", dev, (q, k, v)), ("extend", extend, (q5, k5, v5)), ("verify", verify, (q5, k5, v5))):
        call(f"the paged pool itself, {label}", fn, *a, mix, paged)
    call("the paged pool itself, commit", commit, draft5(paged.lengths), mix, paged, (1, 0, 1))
    call("the paged pool itself, cat", CausalState.cat, [paged])
    full, fview = new_pool("paged", Hk, (64, 133, 127), n_pages=9)
    call("pool exhausted, step", step, q, k, v, mix, fview, state=fview)
    pool_line(s, full)
    call("pool exhausted, extend", extend, q5, k5, v5, mix, fview, state=fview)
    call("pool exhausted, extend counts", extend, q5, k5, v5, mix, fview, state=fview, counts=(1, 0, 2))
    call("pool exhausted, extend cu_seqlens", extend, q5[:1], k5[:1], v5[:1], mix, fview, state=fview, cu_seqlens=(0, 2, 2, 5))
    call("pool exhausted, verify", verify, q5, k5, v5, mix, fview, state=fview)
    call("pool exhausted, verify cu_seqlens", verify, q5[:1], k5[:1], v5[:1], mix, fview, state=fview, cu_seqlens=(0, 2, 2, 5))
    call("pool exhausted, commit", commit, draft5(fview.lengths, fview), mix, fview, (1, 0, 1), state=fview)
    call("pool exhausted, commit of a pack", commit, draft5(fview.lengths, fview, (0, 3, 3, 8)), mix, fview, (1, 0, 1), state=fview)
    k70, v70 = tokens(torch.float32, H, Hk, 70)[1:3]
    call("pool exhausted, state into=", mhla_amd.mhla_causal_state, k70[:1], v70[:1], mix, cu_seqlens=(0, 1, 2, 70), into=full.at((1, 3, 4)))
    pool_line(s, full)
    # h16 pages: extend, verify and commit
    hpool, hview = new_pool("h16", Hk)
    call("h16 pages, extend", extend, q5, k5, v5, mix, hview, state=hview)
    call("h16 pages, extend counts", extend, q5, k5, v5, mix, hview, state=hview, counts=(1, 0, 2))
    call("h16 pages, extend cu_seqlens", extend, q5[:1], k5[:1], v5[:1], mix, hview, state=hview, cu_seqlens=(0, 2, 2, 5))
    call("h16 pages, verify", verify, q5, k5, v5, mix, hview, state=hview)
    call("h16 pages, verify cu_seqlens", verify, q5[:1], k5[:1], v5[:1], mix, hview, state=hview, cu_seqlens=(0, 2, 2, 5))
    call("h16 pages, commit", commit, draft5(hview.lengths, hview), mix, hview, (1, 0, 1), state=hview)
    pool_line(s, hpool)
    # the pack prefill into a view
    kp, vp, cu = k70[:1], v70[:1], (0, 6, 6, 70)
    state_, prefill = mhla_amd.mhla_causal_state, mhla_amd.mhla_causal_prefill
    call("state into= without a pack", state_, k70, v70, mix, into=dview)
    call("prefill into= without a pack", prefill, tokens(torch.float32, H, Hk, 70)[0], k70, v70, mix, into=dview)
    call("state into= a state", state_, kp, vp, mix, cu_seqlens=cu, into=new_state(Hk, (6, 133, 127)))
    call("state into= the paged pool", state_, kp, vp, mix, cu_seqlens=cu, into=paged)
    call("state into= a stale pool", state_, kp, vp, mix, cu_seqlens=cu, into=_stale(new_pool("dense", Hk)[0]).at(SLOTS))
    call("state into= with a capacity", state_, kp, vp, mix, cu_seqlens=cu, into=dview, capacity_chunks=CAP)
    call("state into= sequences against slots", state_, kp, vp, mix, cu_seqlens=(0, 6, 70), into=dview)
    call("state into= heads", state_, kp, vp, mix, cu_seqlens=cu, into=new_pool("dense", H)[1])
    call("state into= K", state_, kp, vp, mix, cu_seqlens=cu, into=new_pool("paged", Hk, k_dim=8)[1])
    call("state into= beyond the capacity", state_, kp, vp, torch.rand(1, 1), cu_seqlens=cu, into=dview)
    call("prefill into= sequences against slots", prefill, tokens(torch.float32, H, Hk, 70)[0][:1], kp, vp, mix, cu_seqlens=(0, 6, 70), into=dview)
    # packed new tokens
    qp, kp5, vp5 = q5[:1], k5[:1], v5[:1]
    cu5 = (0, 2, 2, 5)
    rag = lambda: new_state(Hk, (6, 133, 127))
    for fn in (extend, verify):
        n = fn.__name__
        call(f"{n} cu_seqlens with counts", fn, qp, kp5, vp5, mix, rag(), cu_seqlens=cu5, counts=(2, 0, 3))
        call(f"{n} cu_seqlens left-padded", fn, qp, kp5, vp5, mix, rag(), cu_seqlens=cu5, left_padded=True)
        call(f"{n} cu_seqlens with B = 3", fn, q5, k5, v5, mix, rag(), cu_seqlens=cu5)
        call(f"{n} cu_seqlens not from 0", fn, qp, kp5, vp5, mix, rag(), cu_seqlens=(1, 2, 2, 5))
        call(f"{n} cu_seqlens decreasing", fn, qp, kp5, vp5, mix, rag(), cu_seqlens=torch.tensor([0, 3, 2, 5]))
        call(f"{n} cu_seqlens rank", fn, qp, kp5, vp5, mix, rag(), cu_seqlens=torch.tensor([cu5]))
        call(f"{n} cu_seqlens end", fn, qp, kp5, vp5, mix, rag(), cu_seqlens=(0, 2, 2, 4))
        call(f"{n} cu_seqlens on a uniform state", fn, qp, kp5, vp5, mix, new_state(Hk, seen=5), cu_seqlens=cu5)
        call(f"{n} cu_seqlens sequences", fn, qp, kp5, vp5, mix, rag(), cu_seqlens=(0, 2, 5))
        call(f"{n} cu_seqlens on a view, sequences", fn, qp, kp5, vp5, mix, dview, cu_seqlens=(0, 2, 5))
        call(f"{n} cu_seqlens matrix rank", fn, qp, kp5, vp5, torch.rand(CAP), rag(), cu_seqlens=cu5)
        call(f"{n} cu_seqlens matrix rows", fn, qp, kp5, vp5, torch.rand(2, 2), rag(), cu_seqlens=cu5)
        call(f"{n} cu_seqlens capacity", fn, qp, kp5, vp5, torch.rand(8, 8), new_state(Hk, (6, 133, 318)), cu_seqlens=cu5)
        call(f"{n} cu_seqlens k shape", fn, qp, kp5[:, :4], vp5, mix, rag(), cu_seqlens=cu5)
        call(f"{n} cu_seqlens T = 0 with tokens in cu", fn, qp[:, :0], kp5[:, :0], vp5[:, :0], mix, rag(), cu_seqlens=cu5)
        call(f"{n} cu_seqlens matrix columns", fn, qp[:, :2], kp5[:, :2], vp5[:, :2], torch.rand(2, 2), new_state(Hk, (63, 127, 5)), cu_seqlens=(0, 1, 2, 2))
        with lowered(_PACK_MAX_TOKENS=2):
            call(f"{n} cu_seqlens: a sequence beyond the token bound", fn, qp, kp5, vp5, mix, rag(), cu_seqlens=cu5)
        with lowered(EXTEND_WS_CAP_BYTES=1):
            call(f"{n} cu_seqlens: a sequence beyond the workspace cap", fn, qp, kp5, vp5, mix, rag(), cu_seqlens=cu5)
        with lowered(_MAX_GRID_BH=H - 1):
            call(f"{n} cu_seqlens: a grid of less than one sequence", fn, qp, kp5, vp5, mix, rag(), cu_seqlens=cu5)
    # a view has no sequential fallback (equal head counts: grouped heads fall back to windows of tokens first)
    eq = tokens(torch.float32, H, H, 5)
    with lowered(EXTEND_WS_CAP_BYTES=1):
        for kind in ("dense", "paged"):
            pool, view = new_pool(kind, H)
            call(f"{kind} view: extend beyond the workspace cap", extend, *eq[:3], mix, view, state=view)
            call(f"{kind} view: extend counts beyond the workspace cap", extend, *eq[:3], mix, view, state=view, counts=(3, 0, 5))
            call(f"{kind} view: verify beyond the workspace cap", verify, *eq[:3], mix, view, state=view)
            pool_line(s, pool)
        gq = tokens(torch.float32, H, Hk, 5)
        call("grouped heads: extend beyond the workspace cap", extend, *gq[:3], mix, rag(), counts=(3, 0, 5))
    # the commit: a draft of another view, packed drafts
    other, oview = new_pool("dense", Hk)
    got = s.call("refusal: verify on a view", verify, q5, k5, v5, mix, dview, state=dview)
    for label, st in (("the same slots of another pool", oview), ("other slots of the pool", dense.at((0, 4, 2))), ("a state of its own", rag()),
                      ("the pool itself", dense)):
        call(f"commit to {label}", commit, got[1], mix, st, (1, 0, 1))
    call("commit of a state's draft to a view", commit, draft5((6, 133, 127)), mix, dview, (1, 0, 1))
    call("commit to an equal view of the pool", commit, got[1], mix, dense.at(SLOTS), (1, 0, 1))
    st = rag()
    pack = lambda k_=k5[:1], v_=v5[:1]: ops.CausalDraft(torch.cat((k_, k_[:, :3]), 1), torch.cat((v_, v_[:, :3]), 1), (3, 0, 5), False, st.lengths, None, (0, 3, 3, 8))
    call("commit of a pack: accept beyond the counts", commit, pack(), mix, st, (1, 1, 1))
    call("commit of a pack: matrix columns", commit, pack(), torch.rand(CAP, 2), st, (1, 0, 3))
    call("commit of a pack: matrix rows", commit, pack(), torch.rand(2, CAP), st, (1, 0, 3))
    call("commit of a pack: state shape", commit, pack(), mix, new_state(H, (6, 133, 127)), (1, 0, 1))
    with lowered(_PACK_MAX_TOKENS=4):
        call("commit of a pack: a sequence beyond the token bound", commit, pack(), mix, st, (1, 0, 3))


def _stale(pool):
    pool.stale = True
    return pool


def record():
    lines = []
    for name in PUBLIC:
        obj = ops
        for part in name.split("."):
            obj = getattr(obj, part)
        doc = hashlib.sha256((obj.__doc__ or "").encode()).hexdigest()
        try:
            sig = inspect.signature(obj)
        except ValueError:   # (an exception class that takes what its base takes)
            sig = f"({', '.join(c.__name__ for c in obj.__mro__[1:])})"
        lines.append(f"{name}{sig} doc {doc}")
    with Session(ops, _lib) as s:
        for (H, Hk), dtype, limit in itertools.product(((4, 4), (4, 2)), (torch.float32, torch.bfloat16), (None, 2)):
            saved = ops._MAX_GRID_BH
            if limit:
                ops._MAX_GRID_BH = limit * H
            try:
                tag = f"[H={H} Hkv={Hk} {dtype} grid={'default' if limit is None else f'{limit}H'}]"
                scenarios(s, tag, dtype, H, Hk)
                pool_scenarios(s, tag, dtype, H, Hk)
            finally:
                ops._MAX_GRID_BH = saved
        pool_methods(s)
        refusals(s)
    return lines + s.lines


def raise_lines():
    src = open(ops.__file__).read().split("\n")
    lo = next(i for i, ln in enumerate(src) if ln.startswith("class CausalState"))
    hi = next(i for i, ln in enumerate(src) if ln.startswith("# per-head RMSNorm x swish gate"))
    return {i + 1 for i in range(lo, hi) if src[i].lstrip().startswith("raise ")}, src


def count_calls():
    """Python function calls (cProfile, builtins included) of one public call, caches warm; the count does not depend on the machine."""
    H = 4
    mix = torch.rand(CAP, CAP)
    out = []
    with Session(ops, _lib) as s:
        def measure(label, fn, make_args):
            fn(*make_args()[0], **make_args()[1])   # (warm: the cached workspace sizes)
            args, kw = make_args()
            prof = cProfile.Profile()
            prof.enable()
            fn(*args, **kw)
            prof.disable()
            out.append(f"{label}: {pstats.Stats(prof).total_calls}")

        for Hk in (4, 2):
            q, k, v, g = tokens(torch.float32, H, Hk, 1)
            q5, k5, v5, g5 = tokens(torch.float32, H, Hk, 5)
            tag = f"Hkv={Hk}"
            measure(f"mhla_causal_step uniform {tag}", mhla_amd.mhla_causal_step, lambda: ((q, k, v, mix, new_state(Hk, seen=5)), {}))
            measure(f"mhla_causal_step ragged, one chain {tag}", mhla_amd.mhla_causal_step, lambda: ((q, k, v, mix, new_state(Hk, (6, 133, 127))), {}))

            def dev_args():
                st = new_state(Hk, (6, 133, 127))
                st.full
                return (q, k, v, mix, st), {}
            measure(f"mhla_causal_step_dev {tag}", mhla_amd.mhla_causal_step_dev, dev_args)
            measure(f"mhla_causal_step_dev gate, norm weight {tag}", mhla_amd.mhla_causal_step_dev,
                    lambda: (dev_args()[0], dict(gate=g, norm_weight=torch.ones(V))))
            measure(f"mhla_causal_extend T=5 uniform {tag}", mhla_amd.mhla_causal_extend, lambda: ((q5, k5, v5, mix, new_state(Hk, seen=5)), {}))
            measure(f"mhla_causal_extend T=5 ragged {tag}", mhla_amd.mhla_causal_extend, lambda: ((q5, k5, v5, mix, new_state(Hk, (6, 133, 127))), {}))
            measure(f"mhla_causal_extend counts {tag}", mhla_amd.mhla_causal_extend,
                    lambda: ((q5, k5, v5, mix, new_state(Hk, (6, 133, 127))), dict(counts=(3, 0, 5))))
            measure(f"mhla_causal_verify {tag}", mhla_amd.mhla_causal_verify, lambda: ((q5, k5, v5, mix, new_state(Hk, (6, 133, 127))), dict(counts=(3, 0, 5))))

            def commit_args():
                st = new_state(Hk, (6, 133, 127))
                return (ops.CausalDraft(k5, v5, (3, 0, 5), False, st.lengths), mix, st, (1, 0, 3)), {}
            measure(f"mhla_causal_commit {tag}", mhla_amd.mhla_causal_commit, commit_args)

            # views of pools: the ragged step and the device-positioned step
            for kind in ("dense", "paged", "h16"):
                def view_args():
                    pool, view = new_pool(kind, Hk)
                    pool.full, view.map, view.lengths
                    return (q, k, v, mix, view), {}
                measure(f"mhla_causal_step {kind} view {tag}", mhla_amd.mhla_causal_step, view_args)
                measure(f"mhla_causal_step_dev {kind} view {tag}", mhla_amd.mhla_causal_step_dev, view_args)

            # packed new tokens
            cu = (0, 3, 3, 8)
            qp, kp, vp = (torch.cat((t[:1], t[:1, :3]), 1) for t in (q5, k5, v5))
            for kind in ("plain", "dense"):
                def state_():
                    if kind == "plain":
                        return new_state(Hk, (6, 133, 127))
                    view = new_pool(kind, Hk)[1]
                    view.map, view.lengths
                    return view

                def packed_commit_args():
                    st = state_()
                    return (ops.CausalDraft(kp, vp, (3, 0, 5), False, st.lengths, None if kind == "plain" else st, cu), mix, st, (1, 0, 3)), {}
                measure(f"mhla_causal_extend cu_seqlens {kind} {tag}", mhla_amd.mhla_causal_extend, lambda: ((qp, kp, vp, mix, state_()), dict(cu_seqlens=cu)))
                measure(f"mhla_causal_verify cu_seqlens {kind} {tag}", mhla_amd.mhla_causal_verify, lambda: ((qp, kp, vp, mix, state_()), dict(cu_seqlens=cu)))
                measure(f"mhla_causal_commit of a pack {kind} {tag}", mhla_amd.mhla_causal_commit, packed_commit_args)
    return out


if __name__ == "__main__":
    if opt.counts:
        print("\n".join(count_calls()))
        sys.exit(0)
    seen = set()
    if opt.raises:
        path = ops.__file__

        def tracer(frame, event, arg):
            if frame.f_code.co_filename != path:
                return None
            if event == "line":
                seen.add(frame.f_lineno)
            return tracer
        sys.settrace(tracer)
    log = "\n".join(record()) + "\n"
    sys.settrace(None)
    if opt.output:
        open(opt.output, "w").write(log)
    else:
        sys.stdout.write(log)
    print(f"sha256 {hashlib.sha256(log.encode()).hexdigest()}  {log.count(chr(10))} lines", file=sys.stderr)
    if opt.raises:
        want, src = raise_lines()
        for n in sorted(want - seen):
            print(f"never raised: {n}: {src[n - 1].strip()[:120]}", file=sys.stderr)
        print(f"{len(want & seen)} of {len(want)} raise statements of the section were reached", file=sys.stderr)
