"""Packed new tokens (`cu_seqlens=`) of mhla_causal_extend / mhla_causal_verify / mhla_causal_commit, host side, no GPU: every refusal
before any library call, assigned page or change of the host mirror; the library calls recorded by tools/fake_decode_lib.py on CPU
tensors -- the packed entry point, its offsets and token count, the vouching values of `_ragged_plan`, views with a zero batch
stride, slot map and page table present or null for the three kinds of state, Hkv -- and one chain per slice when the token bound,
the (b, h) grid range or `EXTEND_WS_CAP_BYTES` cuts the pack between sequences."""
import os
import re
import sys

import pytest
import torch

import mhla_amd
from mhla_amd import CausalState, PagedCausalState, PoolExhausted, _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fake_decode_lib import Session, batch_of  # noqa: E402

H, HKV, K, V, CAP, L = 4, 2, 8, 12, 4, 5
LENGTHS = (60, 0, 63, 64, 5)
COUNTS = (10, 0, 1, 130, 3)
CU = (0, 10, 10, 11, 141, 144)
N = CU[-1]
NAMES = ("mhla_causal_extend_packed", "mhla_causal_verify_packed", "mhla_causal_commit_packed")
# positions of the recorded arguments (the workspace and its size are one entry)
X = dict(q=0, k=1, v=2, mix=3, ldmix=4, S=5, n_pages=6, table=7, cap=8, P=9, Cur=10, pos=11, slot=12, n_slots=13, off=14, n_tokens=15, max_end=16,
         max_later=17, any_close=18, out=19, gate=20, y=23, ws=24, B=25, H=26, Hkv=27, K=28, V=29)
XC = dict(k=0, v=1, S=4, n_pages=5, table=6, cap=7, pos=10, slot=11, n_slots=12, off=13, acc=14, n_tokens=15, max_end=16, max_later=17,
          any_close=18, ws=19, B=20, Hkv=21)


def z(*s):
    return torch.zeros(s)


def toks(n=N, vdim=V, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, n, H, K, generator=g), torch.randn(1, n, HKV, K, generator=g), torch.randn(1, n, HKV, vdim, generator=g),
            torch.rand(L, L, generator=g))


def plain(lengths=LENGTHS, hkv=HKV, cap=CAP):
    B = len(lengths)
    return CausalState(z(B, hkv, cap, K, V), z(B, hkv, K, V), z(B, hkv, K, V), 0, 64, lengths=lengths)


SLOTS = [5, 2, 0, 4, 1]   # (slot 3 unused)


def dense_view(lengths=LENGTHS):
    host = [0] * 6
    for s, n in zip(SLOTS, lengths):
        host[s] = n
    pool = CausalState(z(6, HKV, CAP, K, V), z(6, HKV, K, V), z(6, HKV, K, V), 0, 64, lengths=host)
    return pool, pool.at(SLOTS)


def paged_view(lengths=LENGTHS, n_pages=12, page_format="fp32", vdim=V):
    pool = PagedCausalState.empty(6, HKV, K, vdim, CAP, n_pages, "cpu", page_format=page_format)
    pool.reserve(SLOTS, list(lengths))
    pool._set_lengths(SLOTS, lengths)
    pool.pos.copy_(torch.tensor(pool.lengths, dtype=torch.int32))
    return pool, pool.at(SLOTS)


def mirror(state):
    pool = getattr(state, "pool", state)
    return (pool.lengths, pool.seen, None if pool.pos is None else pool.pos.tolist(), [list(r) for r in pool.table] if pool.pages is not None else None)


@pytest.fixture
def offsets(monkeypatch):
    """The host values of every `_packed_offsets` copy the call makes."""
    seen, real = [], ops._packed_offsets

    def spy(*a, **kw):
        t, at = real(*a, **kw)
        seen.append((t.tolist(), at))
        return t, at
    monkeypatch.setattr(ops, "_packed_offsets", spy)
    return seen


def refused(exc, match, fn, *args, state, **kw):
    before = mirror(state)
    with Session(ops, _lib) as s:
        with pytest.raises(exc, match=match):
            s.call("refused", fn, *args, catch=False, **kw)
    assert s.calls == [], "refused after a library call"
    assert mirror(state) == before, "a refused call changed the host mirror or assigned a page"


@pytest.mark.parametrize("fn", [mhla_amd.mhla_causal_extend, mhla_amd.mhla_causal_verify], ids=["extend", "verify"])
def test_every_refusal_comes_first(fn):
    from mhla_amd import build
    build.build(verbose=False)
    q, k, v, mix = toks()
    st = plain()
    refused(ValueError, "excludes counts and left_padded", fn, q, k, v, mix, st, state=st, cu_seqlens=CU, counts=COUNTS)
    refused(ValueError, "excludes counts and left_padded", fn, q, k, v, mix, st, state=st, cu_seqlens=CU, left_padded=True)
    refused(ValueError, "must start at 0", fn, q, k, v, mix, st, state=st, cu_seqlens=(1, 10, 10, 11, 141, 144))
    refused(ValueError, "non-decreasing", fn, q, k, v, mix, st, state=st, cu_seqlens=(0, 10, 9, 11, 141, 144))
    refused(ValueError, r"ends at 143, the pack has N = 144", fn, q, k, v, mix, st, state=st, cu_seqlens=(0, 10, 10, 11, 141, 143))
    refused(ValueError, r"holds 5 sequences, cu_seqlens has 5 entries \(4 sequences\)", fn, q, k, v, mix, st, state=st, cu_seqlens=(0, 10, 11, 141, 144))
    refused(ValueError, "1-D integer tensor", fn, q, k, v, mix, st, state=st, cu_seqlens=torch.tensor([CU]))
    two = tuple(t.expand(2, -1, -1, -1) for t in (q, k, v))
    refused(ValueError, r"one packed row \(B = 1\), got B = 2", fn, *two, mix, st, state=st, cu_seqlens=CU)
    uniform = CausalState(z(5, HKV, CAP, K, V), z(5, HKV, K, V), z(5, HKV, K, V), 5, 64)
    refused(ValueError, "needs a ragged state and this one is uniform", fn, q, k, v, mix, uniform, state=uniform, cu_seqlens=CU)
    stale = plain()
    stale.stale = True
    refused(ValueError, "stale", fn, q, k, v, mix, stale, state=stale, cu_seqlens=CU)
    stale.stale = False
    # IndexErrors name the sequences: sequence 3 ends at 194 tokens, 4 chunks
    refused(IndexError, r"sequences \[3\] \(lengths \(64,\) \+ counts \(130,\)\) need up to 4 chunks but mixing_matrix has only 3 rows",
            fn, q, k, v, mix[:3, :3], st, state=st, cu_seqlens=CU)
    small = plain(cap=3)
    refused(IndexError, r"sequences \[3\].*need up to 4 chunks but the state holds only 3", fn, q, k, v, mix, small, state=small, cu_seqlens=CU)
    # the page rule, all or nothing: the view needs 2 + 0 + 1 + 4 + 1 = 8 pages and holds 4 of the pool's 6
    pool, view = paged_view(n_pages=6)
    refused(PoolExhausted, r"need 4 more pages, the pool has 2 free", fn, q, k, v, mix, view, state=view, cu_seqlens=CU)
    pool, view = paged_view(page_format="h16", vdim=16)   # (h16 pages: K V a multiple of 64)
    refused(NotImplementedError, "h16", fn, *toks(vdim=16), view, state=view, cu_seqlens=CU)


def check_views(call, names, n_tokens, first=0):
    for name in names:
        kind, base, at, sb, sn, sh = call.args[X[name]]
        heads, width = (H, K) if name == "q" else (HKV, K) if name == "k" else (HKV, V) if name == "v" else (H, V)
        assert kind == "view" and sb == 0 and sn == heads * width and sh == width and at == first * heads * width, (name, call.args[X[name]])
    assert call.args[X["n_tokens"]] == n_tokens


@pytest.mark.parametrize("kind", ["state", "dense view", "paged view"])
@pytest.mark.parametrize("verify", [False, True], ids=["extend", "verify"])
def test_what_one_packed_call_records(kind, verify, offsets):
    q, k, v, mix = toks()
    pool, st = (None, plain()) if kind == "state" else dense_view() if kind == "dense view" else paged_view()
    fn = mhla_amd.mhla_causal_verify if verify else mhla_amd.mhla_causal_extend
    with Session(ops, _lib) as s:
        own = pool if pool is not None else st
        s.name(q=q, k=k, v=v, mix=mix, S=own._chunks, P=own.P, Cur=own.Cur, pos=own.pos)
        if kind != "state":
            s.name(slot=st.map)
        if kind == "paged view":
            s.name(table=pool.table_dev)
        res = s.call("packed", fn, q, k, v, mix, st, cu_seqlens=CU, catch=False)
    o = res[0] if verify else res
    assert tuple(o.shape) == (1, N, H, V)
    (c,) = s.calls
    assert c.name == NAMES[1 if verify else 0]
    a = c.args
    assert offsets == [(list(CU), [0])], "one small copy: the offsets"
    assert a[X["off"]][0] == "ptr" and a[X["off"]][2] == 0
    check_views(c, ("q", "k", "v", "out"), N)
    assert a[X["gate"]] == ("null",) and a[X["y"]] == ("null",)
    max_end, max_later, any_close, _ = ops._ragged_plan(LENGTHS, COUNTS, CAP)
    assert (a[X["max_end"]], a[X["max_later"]], a[X["any_close"]]) == (max_end, max_later, int(any_close)) == (194, 2, 1)
    assert (batch_of(c), a[X["H"]], a[X["Hkv"]], a[X["K"]], a[X["V"]], a[X["cap"]]) == (5, H, HKV, K, V, CAP)
    assert a[X["mix"]] == ("ptr", "mix", 0) and a[X["ldmix"]] == L and a[X["S"]] == ("ptr", "S", 0) and a[X["pos"]] == ("ptr", "pos", 0)
    if kind == "state":
        assert a[X["slot"]] == ("null",) and a[X["n_slots"]] == 0 and a[X["table"]] == ("null",) and a[X["n_pages"]] == 0
    else:
        assert a[X["slot"]] == ("ptr", "slot", 0) and a[X["n_slots"]] == 6
        assert (a[X["table"]], a[X["n_pages"]]) == ((("ptr", "table", 0), 12) if kind == "paged view" else (("null",), 0))
    need = _lib.load().mhla_causal_extend_packed_ws_bytes(5, N, H, HKV, K, V, 2, 0)
    al4 = lambda n: (n + 3) // 4 * 4
    assert a[X["ws"]][1] >= need == 4 * (al4(5 * HKV * 2 * K * V) + al4(H * N * V) + al4(5))
    own = pool if pool is not None else st
    after = tuple(p + n for p, n in zip(LENGTHS, COUNTS))
    assert st.lengths == (LENGTHS if verify else after) and st.seen == max(st.lengths)
    if kind == "paged view":
        assert all(pool.table[s][j] >= 0 for s, n in zip(SLOTS, after) for j in range(-(-n // 64))), "the page rule ran for the pack's ends"
    if verify:
        draft = res[1]
        assert draft.cu == CU and draft.counts == COUNTS and draft.lengths == LENGTHS and not draft.left_padded
        assert draft.view is (st if kind != "state" else None)


def test_the_epilogue_goes_through_y():
    q, k, v, mix = toks()
    gate, w = torch.randn(1, N, H, V), torch.rand(V)
    with Session(ops, _lib) as s:
        s.name(gate=gate)
        s.call("y", mhla_amd.mhla_causal_extend, q, k, v, mix, plain(), cu_seqlens=CU, gate=gate, norm_weight=w, catch=False)
    (c,) = s.calls
    assert c.args[X["out"]] == ("null",) and c.args[X["y"]][0] == "view" and c.args[X["y"]][3] == 0
    assert c.args[X["gate"]] == ("view", "gate", 0, 0, H * V, V)


def test_an_all_empty_pack_launches_nothing():
    q, k, v, mix = toks(0)
    st = plain()
    with Session(ops, _lib) as s:
        o = s.call("extend", mhla_amd.mhla_causal_extend, q, k, v, mix, st, cu_seqlens=(0,) * 6, catch=False)
        o2, draft = s.call("verify", mhla_amd.mhla_causal_verify, q, k, v, mix, st, cu_seqlens=(0,) * 6, catch=False)
        assert s.call("commit", mhla_amd.mhla_causal_commit, draft, mix, st, (0,) * 5, catch=False) is st
    assert s.calls == [] and st.lengths == LENGTHS
    assert tuple(o.shape) == tuple(o2.shape) == (1, 0, H, V) and draft.cu == (0,) * 6
    # idle sequences beside one that has tokens: one chain, their offsets equal
    q, k, v, mix = toks(3)
    st = plain((5, 64, 7))
    with Session(ops, _lib) as s:
        o = s.call("some", mhla_amd.mhla_causal_extend, q, k, v, mix, st, cu_seqlens=(0, 0, 3, 3), catch=False)
    assert len(s.calls) == 1 and batch_of(s.calls[0]) == 3 and st.lengths == (5, 67, 7) and tuple(o.shape) == (1, 3, H, V)


@pytest.mark.parametrize("limit", ["tokens", "grid", "workspace"])
def test_one_chain_per_slice(limit, monkeypatch, offsets):
    q, k, v, mix = toks()
    st = plain()
    lib = _lib.load()
    ws = lambda i, j: lib.mhla_causal_extend_packed_ws_bytes(j - i, CU[j] - CU[i], H, HKV, K, V, ops._ragged_plan(LENGTHS[i:j], COUNTS[i:j], CAP)[1], 0)
    if limit == "tokens":
        monkeypatch.setattr(ops, "_PACK_MAX_TOKENS", 133)
        want = [(0, 3), (3, 5)]
    elif limit == "grid":
        monkeypatch.setattr(ops, "_MAX_GRID_BH", 2 * H)
        want = [(0, 2), (2, 4), (4, 5)]
    else:
        assert ws(0, 4) > ws(0, 3) and ws(3, 5) <= ws(0, 4) - 1
        monkeypatch.setattr(ops, "EXTEND_WS_CAP_BYTES", ws(0, 4) - 1)
        want = [(0, 3), (3, 5)]
    with Session(ops, _lib) as s:
        s.name(q=q, k=k, v=v, pos=st.pos, S=st.S)
        s.call("cut", mhla_amd.mhla_causal_extend, q, k, v, mix, st, cu_seqlens=CU, catch=False)
    assert len(s.calls) == len(want) and len(offsets) == 1, "one chain per slice, one copy for all of them"
    host, at = offsets[0]
    for c, (i, j), a0 in zip(s.calls, want, at):
        assert c.name == NAMES[0] and batch_of(c) == j - i
        assert host[a0:a0 + j - i + 1] == [x - CU[i] for x in CU[i:j + 1]], "offsets from the chain's first token"
        check_views(c, ("q", "k", "v", "out"), CU[j] - CU[i], CU[i])
        assert c.args[X["off"]][2] == 4 * a0
        plan = ops._ragged_plan(LENGTHS[i:j], COUNTS[i:j], CAP)
        assert (c.args[X["max_end"]], c.args[X["max_later"]], c.args[X["any_close"]]) == (plan[0], plan[1], int(plan[2]))
        assert c.args[X["pos"]] == ("ptr", "pos", 4 * i) and c.args[X["S"]] == ("ptr", "S", 4 * i * HKV * CAP * K * V)
    assert st.lengths == tuple(p + n for p, n in zip(LENGTHS, COUNTS))


def test_a_single_sequence_over_a_limit_is_refused(monkeypatch):
    q, k, v, mix = toks()
    st = plain()
    need = _lib.load().mhla_causal_extend_packed_ws_bytes(1, 130, H, HKV, K, V, 2, 0)
    monkeypatch.setattr(ops, "EXTEND_WS_CAP_BYTES", need - 1)
    for fn in (mhla_amd.mhla_causal_extend, mhla_amd.mhla_causal_verify):
        refused(ValueError, r"sequence 3 alone brings 130 new tokens.*cut between sequences", fn, q, k, v, mix, st, state=st, cu_seqlens=CU)
    monkeypatch.setattr(ops, "EXTEND_WS_CAP_BYTES", 256 << 20)
    monkeypatch.setattr(ops, "_PACK_MAX_TOKENS", 129)
    refused(ValueError, r"sequence 3 alone brings 130 new tokens", mhla_amd.mhla_causal_extend, q, k, v, mix, st, state=st, cu_seqlens=CU)


@pytest.mark.parametrize("kind", ["state", "paged view"])
def test_the_commit_reads_the_pack_from_the_draft(kind, offsets):
    q, k, v, mix = toks()
    pool, st = (None, plain()) if kind == "state" else paged_view()
    accept = (4, 0, 1, 70, 0)
    with Session(ops, _lib) as s:
        own = pool if pool is not None else st
        s.name(k=k, v=v, mix=mix, S=own._chunks, P=own.P, Cur=own.Cur, pos=own.pos)
        _, draft = s.call("verify", mhla_amd.mhla_causal_verify, q, k, v, mix, st, cu_seqlens=CU, catch=False)
        with pytest.raises(ValueError, match=r"accept=.* must be in 0 \.\. counts"):
            s.call("over", mhla_amd.mhla_causal_commit, draft, mix, st, (11, 0, 1, 70, 0), catch=False)
        assert len(s.calls) == 1 and st.lengths == LENGTHS
        assert s.call("commit", mhla_amd.mhla_causal_commit, draft, mix, st, accept, catch=False) is st
    c = s.calls[1]
    a = c.args
    assert c.name == NAMES[2] and len(s.calls) == 2
    assert offsets[1] == (list(CU) + list(accept), [0]), "one small copy: the offsets, then accept"
    assert a[XC["off"]][0] == "ptr" and a[XC["acc"]] == ("ptr", a[XC["off"]][1], 4 * 6)
    for name, width in (("k", K), ("v", V)):
        assert a[XC[name]] == ("view", name, 0, 0, HKV * width, width)
    plan = ops._ragged_plan(LENGTHS, accept, CAP)
    assert (a[XC["n_tokens"]], a[XC["max_end"]], a[XC["max_later"]], a[XC["any_close"]]) == (N, plan[0], plan[1], int(plan[2])) == (N, 134, 1, 1)
    assert (batch_of(c), a[XC["Hkv"]], a[XC["cap"]]) == (5, HKV, CAP)
    assert (a[XC["slot"]] == ("null",)) == (kind == "state") and (a[XC["table"]] == ("null",)) == (kind == "state")
    assert a[XC["n_pages"]] == (0 if kind == "state" else 12) and a[XC["n_slots"]] == (0 if kind == "state" else 6)
    assert st.lengths == tuple(p + n for p, n in zip(LENGTHS, accept))
    # every draft rejected: nothing is launched
    st2 = plain()
    with Session(ops, _lib) as s:
        _, d2 = s.call("verify", mhla_amd.mhla_causal_verify, q, k, v, mix, st2, cu_seqlens=CU, catch=False)
        s.call("none", mhla_amd.mhla_causal_commit, d2, mix, st2, (0,) * 5, catch=False)
    assert len(s.calls) == 1 and st2.lengths == LENGTHS


def test_the_draft_keeps_its_positional_form():
    k, v = z(2, 3, HKV, K), z(2, 3, HKV, V)
    d = ops.CausalDraft(k, v, (3, 1), True, (5, 6))
    assert d.cu is None and d.view is None and d.left_padded and "packed" not in repr(d)
    d = ops.CausalDraft(k, v, (3, 1), False, (5, 6), None, [0, 3, 4])
    assert d.cu == (0, 3, 4) and ops.CausalDraft.__slots__[-1] == "cu" and "packed" in repr(d)


def test_padded_calls_keep_their_entry_points():
    """`counts=` still goes through mhla_causal_extend_ragged / mhla_causal_verify_ragged with the padded width (the golden call logs of
    test_decode_calls_cpu.py hold every argument)."""
    g = torch.Generator().manual_seed(1)
    q, k, v = torch.randn(5, 130, H, K, generator=g), torch.randn(5, 130, HKV, K, generator=g), torch.randn(5, 130, HKV, V, generator=g)
    mix = torch.rand(L, L, generator=g)
    with Session(ops, _lib) as s:
        s.call("extend", mhla_amd.mhla_causal_extend, q, k, v, mix, plain(), counts=COUNTS, catch=False)
        _, d = s.call("verify", mhla_amd.mhla_causal_verify, q, k, v, mix, plain(), counts=COUNTS, catch=False)
    assert [c.name for c in s.calls] == ["mhla_causal_extend_ragged_gqa", "mhla_causal_verify_ragged_gqa"] and d.cu is None
    assert all(c.args[0][3] == 130 * H * K for c in s.calls), "the padded views keep their batch stride"


def test_the_entry_points_are_declared_exported_and_bound():
    from mhla_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mhla_hip.h")).read()
    for name in NAMES + ("mhla_causal_extend_packed_ws_bytes",):
        assert re.search(r"\b(int|size_t) " + name + r"\(", header), f"{name} is not declared in include/mhla_hip.h"
        assert name in _lib.SIGNATURES and callable(getattr(lib, name))
    assert _lib.ABI_VERSION == 9 == lib.mhla_abi_version()
    assert lib.mhla_causal_extend_packed_ws_bytes(0, 1, H, HKV, K, V, 0, 0) == lib.mhla_causal_extend_packed_ws_bytes(1, 1, H, 3, K, V, 0, 0) == 0
