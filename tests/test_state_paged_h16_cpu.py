"""h16 pages of a paged state pool (`PagedCausalState.empty(..., page_format="h16")`), host side, no GPU.
  * The REFERENCE CODEC (tests/pool_util.py: `encode`, `decode`): a torch restatement of the one encode / decode of causal_step.hpp
    (the exponent field through an int32 view, as h16_mult_from_max reads it; the rounding is `.half()`), which
    tests/test_gpu_state_paged_h16.py holds the kernels to bit for bit.
  * The host layer on tools/fake_decode_lib.py: what is allocated, that the page rule / fork / trim / reset give the tables of the
    fp32 pool for the same calls, that compact() decodes, the three refusals, K V % 64, and the `_h16` entry points with the
    arguments the header names.  The pool (`pool_util.host_pool`) is the one tests/test_state_swap_cpu.py uses.
  * The INPUT CHECK of the GPU row-parity test: with that test's very inputs (`pool_util.tokens(..., device="cpu")`: the one generator,
    without the copy to the device), decoding is emulated in fp64 with every finished chunk
    replaced by decode(encode(fp32(S_j))) and held to the exact fp64 operator chunk by chunk, at the part of the row bound that is
    left after the final rounding of a row (1e-3 of the chunk's maximum): what the page format itself costs, with nothing of the
    kernels in it.  Observed: profiles/causal_state_h16.md."""
import os
import re
import sys

import pytest
import torch

import mhla_amd
from mhla_amd import CausalState, PagedCausalState, PagedStateView, PoolExhausted, _lib, ops
from pool_util import (CAP, CASES, GROUP, HOST_DIMS, HOST_LENGTHS, HOST_ROWS, IDS, N_SLOTS, ROW_EXTRA, decode, encode, gate_norm, host_pool,
                       host_state, rows_fp64, sequence)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fake_decode_lib import Session  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------------
# the reference codec
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_codec_keeps_eleven_bits_of_each_groups_maximum():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3, 2, 40, 72, generator=g) * torch.exp2(torch.randint(-40, 40, (3, 2, 1, 1), generator=g).float())
    x[0, 0, :8] *= 1e-6                       # groups far below their neighbours
    x[1, 1].view(-1)[:GROUP] = 0.0            # an all-zero group
    x[2, 0].view(-1)[5] = 3.0e38              # near the top of fp32
    pay, mult = encode(x)
    assert pay.dtype == torch.float16 and pay.shape == x.shape and mult.dtype == torch.float32 and tuple(mult.shape) == (3, 2, 45)
    back = decode(pay, mult)
    assert bool(torch.isfinite(pay.float()).all())
    gmax = x.reshape(3, 2, 45, GROUP).abs().amax(-1, keepdim=True).double()
    err = (back.double() - x.double()).abs().reshape(3, 2, 45, GROUP)
    assert bool((err <= 2.0 ** -11 * gmax).all()), "decode(encode(x)) within 2^-11 of each group's maximum"
    assert float(pay[1, 1].view(-1)[:GROUP].abs().max()) == 0.0 and float(back[1, 1].view(-1)[:GROUP].abs().max()) == 0.0
    bits = mult.view(torch.int32)
    assert bool(((bits & 0x807FFFFF) == 0).all()) and bool(((bits >> 23) >= 1).all()) and bool(((bits >> 23) <= 240).all()), "powers of two"
    # the largest element of a group lands in [2^14, 2^15): the payload's own range
    top = pay.float().reshape(3, 2, 45, GROUP).abs().amax(-1)
    live = gmax.squeeze(-1) > 2.0 ** -100
    assert bool((top[live] >= 2.0 ** 14).all()) and bool((top[live] <= 2.0 ** 15).all())
    # decoding is exact: a second round trip changes nothing
    pay2, mult2 = encode(back)
    assert torch.equal(pay2.view(torch.int16), pay.view(torch.int16)) and torch.equal(mult2[live], mult[live])


# ---------------------------------------------------------------------------------------------------------------------------
# the host layer
# ---------------------------------------------------------------------------------------------------------------------------
(H, K, V, N_PAGES), LENGTHS, ROWS = HOST_DIMS, HOST_LENGTHS, HOST_ROWS   # (5, 0, 0, 63, 130) through [[4, ..], [], [], [6, ..], [7, 5, 2, -1]]
E = K * V
NAMES = ("mhla_causal_step_paged_h16", "mhla_causal_step_dev_paged_h16", "mhla_causal_varlen_state_init_paged_h16")


def toks(B, T=1):
    g = torch.Generator().manual_seed(5)
    return torch.randn(B, T, H, K, generator=g), torch.randn(B, T, H, K, generator=g), torch.randn(B, T, H, V, generator=g), torch.rand(CAP, CAP, generator=g)


@pytest.fixture
def no_library(monkeypatch):
    def load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", load)


def test_an_empty_h16_pool_and_what_it_allocates(no_library):
    pool = PagedCausalState.empty(N_SLOTS, H, K, V, CAP, N_PAGES, "cpu", page_format="h16")
    assert pool.page_format == "h16" and pool.pages.dtype == torch.float16 and tuple(pool.pages.shape) == (N_PAGES, H, K, V)
    assert pool.page_mult.dtype == torch.float32 and tuple(pool.page_mult.shape) == (N_PAGES, H, E // GROUP)
    assert pool.P.dtype == pool.Cur.dtype == torch.float32 and pool.S is None and pool.dims == (N_SLOTS, H, CAP, K, V)
    dense = 4 * (2 * N_SLOTS * H * E + N_SLOTS + N_SLOTS * CAP)
    assert pool.nbytes == N_PAGES * H * (2 * E + 4 * E // GROUP) + dense
    pool.full
    assert pool.nbytes == N_PAGES * H * (2 * E + 4 * E // GROUP) + dense + 4 * N_SLOTS
    fp32 = PagedCausalState.empty(N_SLOTS, H, K, V, CAP, N_PAGES, "cpu")
    assert fp32.page_format == "fp32" and fp32.page_mult is None and fp32.pages.dtype == torch.float32
    assert fp32.nbytes == 4 * N_PAGES * H * E + dense
    view = pool.at([3, 0])
    assert isinstance(view, PagedStateView) and view.pages is pool.pages and view.page_mult is pool.page_mult
    assert CausalState.empty(1, H, K, V, CAP, "cpu").page_mult is None
    assert "page_format=h16" in repr(pool) and "page_format" not in repr(fp32)
    with pytest.raises(ValueError, match="'fp32' or 'h16'"):
        PagedCausalState.empty(N_SLOTS, H, K, V, CAP, N_PAGES, "cpu", page_format="bf16")


def test_a_chunk_that_is_no_whole_number_of_groups_is_refused(no_library):
    with pytest.raises(ValueError, match=r"K V % 64 == 0"):
        PagedCausalState.empty(N_SLOTS, H, 8, 12, CAP, N_PAGES, "cpu", page_format="h16")
    z = lambda *s: torch.zeros(s)
    with pytest.raises(ValueError, match=r"K V % 64 == 0"):
        PagedCausalState(z(N_PAGES, H, 8, 12).half(), z(N_SLOTS, H, 8, 12), z(N_SLOTS, H, 8, 12), ROWS, page_mult=z(N_PAGES, H, 1))
    assert PagedCausalState.empty(N_SLOTS, H, 8, 12, CAP, N_PAGES, "cpu").page_format == "fp32", "the fp32 pool takes the shape as ever"
    # a payload without multipliers, multipliers of another shape or dtype, multipliers beside fp32 pages
    for pages, mult in ((z(N_PAGES, H, K, V).half(), None), (z(N_PAGES, H, K, V).half(), z(N_PAGES, H, E // GROUP + 1)),
                        (z(N_PAGES, H, K, V).half(), z(N_PAGES, H, E // GROUP).double()), (z(N_PAGES, H, K, V), z(N_PAGES, H, E // GROUP))):
        with pytest.raises(ValueError, match="h16 pages are a float16 `pages`"):
            PagedCausalState(pages, z(N_SLOTS, H, K, V), z(N_SLOTS, H, K, V), ROWS, page_mult=mult)
    with pytest.raises(ValueError, match="contiguous float32"):
        PagedCausalState(z(N_PAGES, H, K, V).half(), z(N_SLOTS, H, K, V).half(), z(N_SLOTS, H, K, V).half(), ROWS, page_mult=z(N_PAGES, H, E // GROUP))


def test_compact_decodes_the_pages(no_library):
    pool = host_pool()
    g = torch.Generator().manual_seed(1)
    chunks = torch.randn(N_PAGES, H, K, V, generator=g) * torch.exp2(torch.arange(N_PAGES).float() - 4)[:, None, None, None]
    pay, mult = encode(chunks)
    pool.pages.copy_(pay)
    pool.page_mult.copy_(mult)
    for t in (pool.P, pool.Cur):
        t.copy_(torch.randn(t.shape, generator=g))
    c = pool.at([4, 0]).compact()
    assert type(c) is CausalState and c.S.dtype == torch.float32 and c.lengths == (130, 5) and tuple(c.S.shape) == (2, H, CAP, K, V)
    want = decode(pay, mult)
    for j, p in enumerate((7, 5, 2)):
        assert torch.equal(c.S[0, :, j], want[p])
    assert torch.equal(c.S[1, :, 0], want[4]) and float(c.S[0, :, 3].abs().max()) == float(c.S[1, :, 1:].abs().max()) == 0.0
    assert torch.equal(c.P, pool.P[[4, 0]]) and torch.equal(c.Cur, pool.Cur[[4, 0]])


def _build():
    from mhla_amd import build
    build.build(verbose=False)


def test_the_refusals_come_before_any_page_is_assigned():
    _build()
    pool = host_pool()
    view = pool.at([3, 0, 4])
    q, k, v, mix = toks(3, 70)
    before = host_state(pool)
    with Session(ops, _lib) as s:
        for fn in (mhla_amd.mhla_causal_extend, mhla_amd.mhla_causal_verify):
            with pytest.raises(NotImplementedError, match="h16"):
                s.call(fn.__name__, fn, q, k, v, mix, view, counts=(3, 2, 70), catch=False)
            with pytest.raises(NotImplementedError, match="h16"):
                s.call(fn.__name__, fn, q, k, v, mix, view, catch=False)
        draft = ops.CausalDraft(k, v, (3, 2, 70), False, view.lengths, view)
        with pytest.raises(NotImplementedError, match="h16"):
            s.call("commit", mhla_amd.mhla_causal_commit, draft, mix, view, (1, 2, 1), catch=False)
    assert s.calls == [] and host_state(pool) == before and not pool.stale, "nothing launched, no page assigned, nothing moved"
    # the same calls on the fp32 pool are what they were
    fp32 = host_pool("fp32")
    with Session(ops, _lib) as s:
        s.call("extend", mhla_amd.mhla_causal_extend, q, k, v, mix, fp32.at([3, 0, 4]), counts=(3, 2, 70), catch=False)
    assert [c.name for c in s.calls] == ["mhla_causal_extend_paged"]


def test_the_page_rule_and_the_counts_do_not_depend_on_the_format():
    """The same calls on an fp32 and on an h16 pool: tables, reference counts, free lists, lengths and positions agree after each."""
    _build()
    pools = {fmt: host_pool(fmt) for fmt in ("fp32", "h16")}
    q, k, v, mix = toks(3)
    _, pk, pv, _ = toks(1, 134)
    dev_map = torch.tensor([3, -1, 4], dtype=torch.int32)

    def both(what, fn):
        out = {}
        for fmt, pool in pools.items():
            with Session(ops, _lib) as s:
                fn(pool, s)
            out[fmt] = (host_state(pool), pool.stale, [len(c.args) for c in s.calls])
        assert out["fp32"][:2] == out["h16"][:2], f"{what}: the pools disagree"
        return out["h16"][0]

    t = both("step", lambda p, s: s.call("step", mhla_amd.mhla_causal_step, q, k, v, mix, p.at([3, 0, 4]), catch=False))
    assert t[3] == (6, 0, 0, 64, 131) and t[0] == [list(r) for r in ROWS]
    t = both("prefill", lambda p, s: s.call("prefill", mhla_amd.mhla_causal_state, pk, pv, mix, cu_seqlens=[0, 64, 134], into=p.at([4, 1]), catch=False))
    assert t[0][4] == [0, -1, -1, -1] and t[0][1] == [1, 2, -1, -1] and t[3] == (6, 70, 0, 64, 64)
    t = both("reserve", lambda p, s: p.reserve([3, 2], [65, 130]))
    assert t[0][3] == [6, 3, -1, -1] and t[0][2] == [5, 7, 8, -1]
    both("step_dev", lambda p, s: (p.full, s.call("step_dev", mhla_amd.mhla_causal_step_dev, q, k, v, mix, p.at(dev_map), catch=False)))
    for p in pools.values():
        assert p.stale
        p.stale = False
    t = both("fork", lambda p, s: p.fork(1, 0))
    assert t[0][0] == [1, -1, -1, -1] and t[1][1] == 2 and 4 in t[2], "slot 0 shares slot 1's finished chunk and gave its own page back"
    t = both("trim", lambda p, s: p.trim([3, 2]))
    assert t[0][3] == [6, -1, -1, -1] and t[0][2] == [-1] * 4
    t = both("reset", lambda p, s: p.reset([1]))
    assert t[1][1] == 1 and t[3][1] == 0
    with pytest.raises(PoolExhausted, match=r"need 11 more pages, the pool has 6 free"):
        pools["h16"].reserve([1, 2, 3], [256, 256, 256])


def _pointers(call):
    out = {}
    for a in call.args:
        if isinstance(a, tuple) and a[0] == "ptr":
            out.setdefault(a[1], []).append(a[2])
    return out


@pytest.mark.parametrize("entry", ["step", "step_dev"])
def test_a_view_of_an_h16_pool_makes_the_h16_call(entry, monkeypatch):
    _build()
    monkeypatch.setattr(ops, "_MAX_GRID_BH", 2 * H)   # (two slices: the map is cut with the tokens, the pool passes whole)
    pool = host_pool()
    view = pool.at(torch.tensor([3, 0, 4], dtype=torch.int32) if entry == "step_dev" else [3, 0, 4])
    q, k, v, mix = toks(3)
    fn = mhla_amd.mhla_causal_step if entry == "step" else mhla_amd.mhla_causal_step_dev
    with Session(ops, _lib) as s:
        s.name(q=q, k=k, v=v, mix=mix, pages=pool.pages, mult=pool.page_mult, table=pool.table_dev, P=pool.P, Cur=pool.Cur, pos=pool.pos,
               full=pool.full, map=view.map)
        s.call(entry, fn, q, k, v, mix, view, catch=False)
    assert [c.name for c in s.calls] == [f"mhla_causal_{entry}_paged_h16"] * 2
    for c, first in zip(s.calls, (0, 2)):
        ptr = _pointers(c)
        assert ptr["map"] == [4 * first] and all(ptr[n] == [0] for n in ("mix", "pages", "mult", "table", "P", "Cur", "pos"))
        args = c.args
        i = args.index(("ptr", "pages", 0))
        assert args[i - 1] == CAP and args[i - 2] == ("ptr", "mix", 0), "mix, ldmix, then the pool"
        assert args[i + 1:i + 6] == (("ptr", "mult", 0), N_PAGES, ("ptr", "table", 0), CAP, ("ptr", "P", 0)), \
            "pages_h16, page_mult, n_pages, table_dev, cap_chunks, P"
        i = args.index(("ptr", "map", 4 * first))
        assert args[i - 1] == ("ptr", "pos", 0) and args[i + 1] == N_SLOTS
        assert len(args) == len([a for a in _lib.SIGNATURES[c.name][1]]) - 1, "(the workspace and its size are one recorded argument)"


def test_a_pack_prefill_into_an_h16_view_is_one_h16_call_with_a_workspace(monkeypatch):
    _build()
    pool = host_pool()
    view = pool.at([4, 1])
    _, k, v, mix = toks(1, 134)
    lib = _lib.load()
    one = lib.mhla_causal_varlen_state_init_paged_h16_ws_bytes(1, H, K, V, 0)
    assert one == 4 * H * E and lib.mhla_causal_varlen_state_init_paged_h16_ws_bytes(3, H, K, V, 0) == 3 * one
    assert lib.mhla_causal_varlen_state_init_paged_h16_ws_bytes(0, H, K, V, 0) == 0

    def prefill():
        with Session(ops, _lib) as s:
            s.name(k=k, v=v, mix=mix, pages=pool.pages, mult=pool.page_mult, table=pool.table_dev, P=pool.P, Cur=pool.Cur, pos=pool.pos, map=view.map)
            assert s.call("prefill", mhla_amd.mhla_causal_state, k, v, mix, cu_seqlens=[0, 64, 134], into=view, catch=False) is view
        assert [c.name for c in s.calls] == ["mhla_causal_varlen_state_init_paged_h16"]
        return s.calls[0].args

    args = prefill()
    i = args.index(("ptr", "pages", 0))
    assert args[i + 1:i + 6] == (("ptr", "mult", 0), N_PAGES, ("ptr", "table", 0), CAP, ("ptr", "P", 0))
    i = args.index(("ptr", "map", 0))
    assert args[i - 2] == 2 and args[i - 1][1].startswith("new") and args[i + 1] == N_SLOTS
    ws = [a for a in args if isinstance(a, tuple) and a[0] == "ws"]
    assert len(ws) == 1 and 3 * one <= ws[0][1] < 3 * one + 64 and args[-3] == ws[0], "the three chunks' staging, ahead of dtype and stream"
    assert pool.lengths == (5, 70, 0, 63, 64) and pool.table[4] == [0, -1, -1, -1] and pool.table[1] == [1, 2, -1, -1]
    # beyond the cap the workspace stays at the cap (the library then works through the chunk list in slices); never below one chunk
    monkeypatch.setattr(ops, "EXTEND_WS_CAP_BYTES", 2 * one)
    assert 2 * one <= [a for a in prefill() if isinstance(a, tuple) and a[0] == "ws"][0][1] < 2 * one + 64
    monkeypatch.setattr(ops, "EXTEND_WS_CAP_BYTES", 16)
    assert one <= [a for a in prefill() if isinstance(a, tuple) and a[0] == "ws"][0][1] < one + 64


def test_the_entry_points_are_declared_exported_bound_and_check_their_pool():
    _build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mhla_hip.h")).read()
    for name in NAMES:
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl, f"{name} is not declared in include/mhla_hip.h"
        decl = " ".join(decl.group(1).split())
        paged = _lib.SIGNATURES[name[:-len("_h16")]][1]
        args = _lib.SIGNATURES[name][1]
        at = paged.index(_lib.c_int) + 1
        want = paged[:at] + [_lib.c_void_p, _lib.c_void_p] + paged[at + 1:]
        if "state_init" in name:
            want = want[:-2] + [_lib.c_void_p, _lib.c_size_t] + want[-2:]
            assert "void* ws, size_t ws_bytes, int dtype, void* stream" in decl
        assert args == want and len(decl.split(",")) == len(args) and callable(getattr(lib, name))
        assert "void* pages_h16, float* page_mult, int n_pages, const int32_t* table_dev, int cap_chunks" in decl
    assert re.search(r"\bsize_t mhla_causal_varlen_state_init_paged_h16_ws_bytes\(", header)
    assert lib.mhla_abi_version() == _lib.ABI_VERSION == 9
    # the host checks of the pool come first and need no device
    null = _lib.NULL_VIEW
    buf = (_lib.ctypes.c_float * 8)()
    addr = (_lib.ctypes.addressof(buf) + 15) // 16 * 16

    def prefill(pages, mult, Kc=8, Vc=16, table=addr):
        return lib.mhla_causal_varlen_state_init_paged_h16(null, null, None, 0, pages, mult, 9, table, 4, None, None, 1, None, None, 5, 0, 1, 2,
                                                           Kc, Vc, 64, 1, None, None, None, 0, 0, None)

    for args, what in (((None, addr), b"pages_h16 or page_mult null"), ((addr, None), b"pages_h16 or page_mult null"),
                       ((addr + 8, addr), b"16-byte aligned and page_mult 4-byte aligned"), ((addr, addr + 2), b"page_mult 4-byte aligned"),
                       ((addr, addr, 8, 12), b"K*V % 64 == 0"), ((addr, addr, 8, 16, None), b"table_dev null"), ((addr, addr), b"slot_dev null")):
        assert prefill(*args) != 0, what
        assert what in lib.mhla_last_error(), (what, lib.mhla_last_error())


# ---------------------------------------------------------------------------------------------------------------------------
# the input check of the row parity, on the inputs of the GPU tests (pool_util: tokens, sequence, rows_fp64, gate_norm)
# ---------------------------------------------------------------------------------------------------------------------------
def through_h16(S):
    return decode(*encode(S.float())).double()


def row_chunks(m, n):
    """The rows [m, m + n) of a sequence by its own chunks, as decode_util.check_step_rows cuts them: up to the next boundary, then whole chunks."""
    first = min(n, 64 - m % 64)
    return [slice(0, first)] + [slice(t, min(n, t + 64)) for t in range(first, n, 64)]


def worst_chunk(got, want, m):
    return max(float((got[:, c] - want[:, c]).abs().max() / want[:, c].abs().max()) for c in row_chunks(m, got.shape[1]))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_input_check_h16_pages_alone_stay_within_the_row_bound(case):
    """What the GPU row-parity test (test 4 of test_gpu_state_paged_h16.py) may hide is capped here: with ITS inputs, rows decoded
    in fp64 from finished chunks that went through decode(encode(fp32(.))) stay within ROW_EXTRA of the exact fp64 rows, per
    chunk of every request, with and without the gate x norm epilogue.  Observed (worst chunk over the three requests; plain /
    gate-norm): fp32 2.4e-4 / 2.2e-4, bf16 2.4e-4 / 2.7e-4, fp32-G2 2.2e-4 / 2.8e-4, bf16-G2 2.3e-4 / 2.4e-4, fp32-K40V72
    2.5e-4 / 2.5e-4 -- under three tenths of the bound."""
    worst = [0.0, 0.0]
    for b in range(3):
        q, k, v, gate, w, mix, m = sequence(case, b)
        exact = rows_fp64(q, k, v, mix)[:, m:]
        paged = rows_fp64(q, k, v, mix, through_h16)[:, m:]
        worst[0] = max(worst[0], worst_chunk(paged, exact, m))
        worst[1] = max(worst[1], worst_chunk(gate_norm(paged, gate, w), gate_norm(exact, gate, w), m))
    print(f"input check {IDS[CASES.index(case)]}: h16 pages alone, worst chunk: plain {worst[0]:.2e}, gate-norm {worst[1]:.2e} (bound {ROW_EXTRA:.0e})")
    assert worst[0] < ROW_EXTRA and worst[1] < ROW_EXTRA
