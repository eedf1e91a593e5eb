"""`featmap_rotary_decode` / `mhla_featmap_rotary_decode`, host side, no GPU: the one library call the op records under
tools/fake_decode_lib.py for each token layout -- the slot map and slot count of a view or nulls, `off_dev` against `ntok_dev`, the
views of a pack with a zero batch stride --, every ValueError before any library call, and every MHLA_EINVAL of the real entry point,
which returns before a launch (addresses are plain integers here)."""
import os
import re
import sys

import pytest
import torch

import mhla_amd
from mhla_amd import CausalState, PagedCausalState, _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fake_decode_lib import Session  # noqa: E402

NAME = "mhla_featmap_rotary_decode"
H, HKV, K, V, CAP, ROWS = 4, 2, 16, 8, 4, 256
# positions of the recorded arguments
X = dict(q=0, k=1, cos=2, sin=3, ld_tab=4, tab_rows=5, pos=6, slot=7, n_slots=8, ntok=9, off=10, T=11, left=12, yq=13, yk=14, B=15, H=16, Hkv=17,
         K=18, fmap=19, dtype=20)


def z(*s):
    return torch.zeros(s)


def toks(B, T, seed=3, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, H, K, generator=g).to(dtype), torch.randn(B, T, HKV, K, generator=g).to(dtype)


def tables(dtype=torch.float32):
    g = torch.Generator().manual_seed(1)
    return torch.rand(ROWS, K // 2, generator=g).to(dtype), torch.rand(ROWS, K // 2, generator=g).to(dtype)


def plain(lengths):
    B = len(lengths)
    return CausalState(z(B, HKV, CAP, K, V), z(B, HKV, K, V), z(B, HKV, K, V), 0, 64, lengths=lengths)


def record(q, k, state, pool=None, **kw):
    cos, sin = tables(q.dtype)
    with Session(ops, _lib) as s:
        own = pool if pool is not None else state
        s.name(q=q, k=k, cos=cos, sin=sin, pos=own.pos)
        if pool is not None:
            s.name(slot=state.map)
        if kw.get("off_dev") is not None:
            s.name(off=kw["off_dev"])
        out = s.call("prologue", mhla_amd.featmap_rotary_decode, q, k, cos, sin, state, catch=False, **kw)
    (c,) = s.calls
    assert c.name == NAME
    a = c.args
    assert a[X["cos"]] == ("ptr", "cos", 0) and a[X["sin"]] == ("ptr", "sin", 0) and a[X["ld_tab"]] == K // 2 and a[X["tab_rows"]] == ROWS
    assert a[X["pos"]] == ("ptr", "pos", 0)
    assert (a[X["H"]], a[X["Hkv"]], a[X["K"]], a[X["dtype"]]) == (H, HKV, K, _lib.F32)
    return out, a


def test_padded_with_counts():
    q, k = toks(3, 5)
    (yq, yk), a = record(q, k, plain((7, 0, 63)), counts=(5, 2, 0), feature_map="relu")
    assert tuple(yq.shape) == (3, 5, H, K) and tuple(yk.shape) == (3, 5, HKV, K)
    assert a[X["q"]] == ("view", "q", 0, 5 * H * K, H * K, K) and a[X["k"]] == ("view", "k", 0, 5 * HKV * K, HKV * K, K)
    assert a[X["yq"]][0] == "view" and a[X["yq"]][1] not in ("q", "k") and a[X["yk"]][1] not in ("q", "k"), "out of place"
    assert a[X["ntok"]][0] == "ptr" and a[X["off"]] == ("null",), "the counts, no offsets"
    assert a[X["slot"]] == ("null",) and a[X["n_slots"]] == 0, "a state of its own has no slot map"
    assert (a[X["T"]], a[X["left"]], a[X["B"]], a[X["fmap"]]) == (5, 0, 3, 1)


def test_left_padded_and_no_counts():
    q, k = toks(3, 5)
    _, a = record(q, k, plain((7, 0, 63)), counts=[5, 2, 0], left_padded=True, feature_map="elu")
    assert a[X["ntok"]][0] == "ptr" and a[X["off"]] == ("null",) and (a[X["T"]], a[X["left"]], a[X["fmap"]]) == (5, 1, 2)
    _, a = record(q, k, plain((7, 0, 63)))
    assert a[X["ntok"]] == ("null",) and a[X["off"]] == ("null",) and (a[X["T"]], a[X["left"]], a[X["B"]], a[X["fmap"]]) == (5, 0, 3, 0)


def test_packed_with_host_cu_seqlens(monkeypatch):
    copies, real = [], torch.tensor
    q, k = toks(1, 9)
    st, cu = plain((7, 0, 63)), torch.tensor([0, 4, 4, 9])
    monkeypatch.setattr(ops.torch, "tensor", lambda data, *a, **kw: (copies.append(list(data)), real(data, *a, **kw))[1])
    (yq, yk), a = record(q, k, st, cu_seqlens=cu)
    assert copies == [[0, 4, 4, 9]], "one small copy: the offsets"
    assert tuple(yq.shape) == (1, 9, H, K)
    assert a[X["off"]][0] == "ptr" and a[X["ntok"]] == ("null",) and (a[X["T"]], a[X["left"]], a[X["B"]]) == (9, 0, 3)
    assert a[X["q"]] == ("view", "q", 0, 0, H * K, K) and a[X["k"]] == ("view", "k", 0, 0, HKV * K, K), "a pack's views have no batch stride"
    assert a[X["slot"]] == ("null",) and a[X["n_slots"]] == 0


@pytest.mark.parametrize("page_format", ["fp32", "h16"])
def test_packed_with_off_dev_on_a_view_of_a_pool(page_format, monkeypatch):
    pool = PagedCausalState.empty(6, HKV, K, V, CAP, 12, "cpu", page_format=page_format)
    view = pool.at([4, 1, 5])
    view.map   # (the view's own small copy, made on first use: not the call's)
    pool.stale = True   # a stale host mirror is fine: the positions are read on the device
    off = torch.tensor([0, 4, 4, 9], dtype=torch.int32)
    qk = torch.randn(1, 9, (H + HKV) * K)
    q, k = qk[..., :H * K].view(1, 9, H, K), qk[..., H * K:].view(1, 9, HKV, K)   # slices of one fused projection
    monkeypatch.setattr(ops.torch, "tensor", lambda *a, **kw: pytest.fail("off_dev: no host read and no copy"))
    cos, sin = tables()
    with Session(ops, _lib) as s:
        s.name(qk=qk, pos=pool.pos, slot=view.map, off=off)
        yq, yk = s.call("prologue", mhla_amd.featmap_rotary_decode, q, k, cos, sin, view, off_dev=off, inplace=True, catch=False)
    (c,) = s.calls
    a = c.args
    assert yq is q and yk is k
    ld = (H + HKV) * K
    assert a[X["q"]] == a[X["yq"]] == ("view", "qk", 0, 0, ld, K) and a[X["k"]] == a[X["yk"]] == ("view", "qk", H * K, 0, ld, K), "in place, strided"
    assert a[X["off"]] == ("ptr", "off", 0) and a[X["ntok"]] == ("null",)
    assert a[X["slot"]] == ("ptr", "slot", 0) and a[X["n_slots"]] == 6 and a[X["pos"]] == ("ptr", "pos", 0), "the pool's positions through the slot map"
    assert (a[X["T"]], a[X["left"]], a[X["B"]]) == (9, 0, 3)


def refused(match, q, k, state, cos=None, sin=None, exc=ValueError, **kw):
    c, s_ = tables(q.dtype)
    with Session(ops, _lib) as s:
        with pytest.raises(exc, match=match):
            s.call("refused", mhla_amd.featmap_rotary_decode, q, k, c if cos is None else cos, s_ if sin is None else sin, state, catch=False, **kw)
    assert s.calls == [], "refused after a library call"


def test_every_value_error_comes_before_the_call():
    q, k = toks(3, 5)
    st = plain((7, 0, 63))
    uniform = CausalState(z(3, HKV, CAP, K, V), z(3, HKV, K, V), z(3, HKV, K, V), 5, 64)
    refused(r"uniform.*to_ragged\(\)", q, k, uniform)
    refused("counts has 2 entries", q, k, st, counts=(1, 2))
    refused(r"counts=\(1, 6, 0\) must be in 0 \.\. T=5", q, k, st, counts=(1, 6, 0))
    refused(r"counts=\(1, -1, 0\)", q, k, st, counts=(1, -1, 0))
    refused("holds 3 sequences, the tokens 2", q[:2], k[:2], st)
    pq, pk = toks(1, 9)
    refused("excludes counts and left_padded", pq, pk, st, cu_seqlens=(0, 4, 4, 9), counts=(4, 0, 5))
    refused("excludes counts and left_padded", pq, pk, st, cu_seqlens=(0, 4, 4, 9), left_padded=True)
    refused("must start at 0", pq, pk, st, cu_seqlens=(1, 4, 4, 9))
    refused("non-decreasing", pq, pk, st, cu_seqlens=(0, 4, 3, 9))
    refused("ends at 8, the pack has N = 9", pq, pk, st, cu_seqlens=(0, 4, 4, 8))
    refused(r"one packed row \(B = 1\), got B = 3", q, k, st, cu_seqlens=(0, 4, 4, 5))
    refused("holds 3 sequences, the tokens 2", pq, pk, st, cu_seqlens=(0, 4, 9))
    off = torch.tensor([0, 4, 4, 9], dtype=torch.int32)
    refused("off_dev .* excludes counts, cu_seqlens and left_padded", pq, pk, st, off_dev=off, cu_seqlens=(0, 4, 4, 9))
    refused("off_dev .* excludes counts, cu_seqlens and left_padded", pq, pk, st, off_dev=off, counts=(4, 0, 5))
    refused("off_dev .* excludes counts, cu_seqlens and left_padded", pq, pk, st, off_dev=off, left_padded=True)
    refused(r"contiguous int32 \[sequences \+ 1\]", pq, pk, st, off_dev=off.long())
    refused(r"contiguous int32 \[sequences \+ 1\]", pq, pk, st, off_dev=[0, 4, 4, 9])
    refused(r"one packed row \(B = 1\), got B = 3", q, k, st, off_dev=off)
    refused("holds 3 sequences, the tokens 2", pq, pk, st, off_dev=off[:3])
    # inference only
    g = q.clone().requires_grad_(True)
    refused("inference only", g, k, st)
    with torch.no_grad():
        record(g, k, st)
    # tables in the dtype of q, [tab_rows, K/2]
    cos, sin = tables()
    refused(r"cos/sin: \[tab_rows, K/2 = 8\]", q, k, st, cos=cos.half(), sin=sin.half())
    refused(r"cos/sin: \[tab_rows, K/2 = 8\]", q, k, st, cos=cos[:, :4], sin=sin[:, :4])
    refused(r"cos/sin: \[tab_rows, K/2 = 8\]", q, k, st, cos=cos, sin=sin[:5])
    # shapes, feature map, state
    refused("K % 8 == 0", q[..., :12], k[..., :12], st)
    refused("Hkv dividing H=4", q, torch.randn(3, 5, 3, K), st)
    refused("like q", q, k.half(), st)
    refused("feature_map 'gelu'", q, k, st, feature_map="gelu")
    refused("state must be a CausalState", q, k, None, exc=TypeError)
    pool = PagedCausalState.empty(3, HKV, K, V, CAP, 4, "cpu")
    refused("is a pool, not a state", q, k, pool, exc=TypeError)
    wide = torch.randn(3, 5, H, K + 1)
    refused("inplace needs q and k addressable in place", wide[..., 1:], k, st, inplace=True)


def test_an_empty_pack_launches_nothing():
    q, k = toks(1, 0)
    cos, sin = tables()
    with Session(ops, _lib) as s:
        yq, yk = s.call("empty", mhla_amd.featmap_rotary_decode, q, k, cos, sin, plain((7, 0, 63)), cu_seqlens=(0, 0, 0, 0), catch=False)
    assert s.calls == [] and tuple(yq.shape) == (1, 0, H, K) and tuple(yk.shape) == (1, 0, HKV, K)


def test_the_entry_point_is_declared_exported_and_bound():
    from mhla_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mhla_hip.h")).read()
    assert re.search(r"\bint " + NAME + r"\(", header), f"{NAME} is not declared in include/mhla_hip.h"
    assert NAME in _lib.SIGNATURES and callable(getattr(lib, NAME))
    assert _lib.ABI_VERSION == 9 == lib.mhla_abi_version()
    assert "featmap_rotary_decode" in mhla_amd.__all__


def test_every_einval_of_the_library_returns_before_a_launch():
    """The real entry point on addresses that are plain integers: every call below must fail a check and return MHLA_EINVAL; none
    reaches a launch (there is no device here, and the addresses are not memory)."""
    from mhla_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    Vw = _lib.View
    fn = getattr(lib, NAME)
    A = 1 << 20   # an aligned address
    ok = dict(q=Vw(A, 5 * H * K, H * K, K), k=Vw(A, 5 * HKV * K, HKV * K, K), cos=A, sin=A, ld_tab=K // 2, tab_rows=ROWS, pos=A, slot=None,
              n_slots=0, ntok=None, off=None, T=5, left=0, yq=Vw(A, 5 * H * K, H * K, K), yk=Vw(A, 5 * HKV * K, HKV * K, K), B=3, H=H, Hkv=HKV,
              K=K, fmap=0, dtype=_lib.F32, stream=None)

    def einval(message, **change):
        args = dict(ok, **change)
        rc = fn(*args.values())
        assert rc == -22 and message in lib.mhla_last_error(), (change, rc, lib.mhla_last_error())

    for size in ("B", "H", "Hkv", "K"):
        einval(b"need positive sizes and K % 8 == 0", **{size: 0})
    einval(b"need positive sizes and K % 8 == 0", K=12)
    einval(b"H=4 is not a multiple of Hkv=3", Hkv=3)
    for T in (0, -1, 65536):
        einval(b"1 .. 65535 token rows", T=T)
    einval(b"feature_map 3", fmap=3)
    einval(b"feature_map -1", fmap=-1)
    einval(b"unknown dtype 3", dtype=3)
    einval(b"unknown dtype -1", dtype=-1)
    for name in ("q", "k", "yq", "yk"):
        einval(name.encode() + b": null pointer", **{name: Vw(None, 0, 0, 0)})
        einval(name.encode() + b": pointer not 16-byte aligned", **{name: Vw(A + 8, 5 * H * K, H * K, K)})
        einval(name.encode() + b": strides", **{name: Vw(A, 5 * H * K, H * K + 2, K)})
    einval(b"q: pointer not 8-byte aligned", q=Vw(A + 4, 5 * H * K, H * K, K), dtype=_lib.BF16)
    einval(b"cos/sin tables", cos=None)
    einval(b"cos/sin tables", sin=None)
    einval(b"cos/sin tables", sin=A + 4)
    einval(b"ld_tab=4 < K/2 = 8", ld_tab=4)
    einval(b"ld_tab=10", ld_tab=10)
    einval(b"tab_rows=0", tab_rows=0)
    einval(b"tab_rows=-5", tab_rows=-5)
    einval(b"pos_dev: null or not 4-byte aligned", pos=None)
    einval(b"pos_dev: null or not 4-byte aligned", pos=A + 2)
    for name in ("slot", "ntok", "off"):
        einval(b"slot_dev / ntok_dev / off_dev: not 4-byte aligned", **{name: A + 2, "n_slots": 6})
    einval(b"n_slots=0 with a slot map", slot=A, n_slots=0)
    einval(b"n_slots=-1 with a slot map", slot=A, n_slots=-1)
    einval(b"off_dev (packed tokens) excludes ntok_dev and left_padded", off=A, ntok=A)
    einval(b"off_dev (packed tokens) excludes ntok_dev and left_padded", off=A, left=1)
