"""A paged state pool (`PagedCausalState`), host side, no GPU: the page table validated by name, the all-or-nothing `PoolExhausted`,
reference counts through `reserve`, `fork`, `reset` and `trim`, the page rule of every call kind against the host mirror, the six
mhla_causal_*_paged names in header, library and binding, the library calls a view of a paged pool makes (recorded by
tools/fake_decode_lib.py on CPU tensors): the paged namesake, (pages, n_pages, table_dev) where S stood, the slot map sliced with
the tokens -- and that everything refused is refused before the library is loaded."""
import os
import re
import sys

import pytest
import torch

import mhla_amd
from mhla_amd import CausalState, PagedCausalState, PagedStateView, PoolExhausted, _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fake_decode_lib import Session, batch_of  # noqa: E402

N_SLOTS, H, K, V, CAP, N_PAGES = 5, 2, 8, 12, 4, 9
NAMES = ("mhla_causal_step_paged", "mhla_causal_step_dev_paged", "mhla_causal_extend_paged", "mhla_causal_verify_paged",
         "mhla_causal_commit_paged", "mhla_causal_varlen_state_init_paged")
LENGTHS = (5, 0, 0, 63, 130)
ROWS = [[4, -1, -1, -1], [-1] * 4, [-1] * 4, [6, -1, -1, -1], [7, 5, 2, -1]]   # scrambled: interleaved across slots, descending within


def new_pool(lengths=LENGTHS, rows=ROWS, n_pages=N_PAGES):
    z = lambda *s: torch.zeros(s)
    return PagedCausalState(z(n_pages, H, K, V), z(N_SLOTS, H, K, V), z(N_SLOTS, H, K, V), [list(r) for r in rows], lengths=lengths)


def toks(B, T=1):
    g = torch.Generator().manual_seed(5)
    return torch.randn(B, T, H, K, generator=g), torch.randn(B, T, H, K, generator=g), torch.randn(B, T, H, V, generator=g), torch.rand(CAP, CAP, generator=g)


def counts_consistent(pool):
    """The reference counts are the table's, the free list is exactly the pages nobody names, and the device table is the mirror."""
    named = [p for r in pool.table for p in r if p >= 0]
    assert pool.refs == [named.count(p) for p in range(len(pool.refs))]
    assert sorted(pool.free) == [p for p in range(len(pool.refs)) if p not in named]
    assert pool.pages_free == len(pool.free) and pool.pages_used == len(set(named)) and pool.table_dev.tolist() == pool.table


@pytest.fixture
def no_library(monkeypatch):
    """Whatever the test raises, it raises before the library is asked for."""
    def load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", load)


def test_an_empty_pool_and_what_it_holds(no_library):
    pool = PagedCausalState.empty(N_SLOTS, H, K, V, CAP, N_PAGES, "cpu")
    assert tuple(pool.pages.shape) == (N_PAGES, H, K, V) and tuple(pool.P.shape) == tuple(pool.Cur.shape) == (N_SLOTS, H, K, V)
    assert pool.S is None and pool.lengths == (0,) * N_SLOTS and pool.pos.tolist() == [0] * N_SLOTS and not pool.stale
    assert pool.capacity_chunks == CAP and pool.dims == (N_SLOTS, H, CAP, K, V)
    assert pool.table == [[-1] * CAP] * N_SLOTS and pool.table_dev.dtype == torch.int32 and tuple(pool.table_dev.shape) == (N_SLOTS, CAP)
    assert pool.pages_free == N_PAGES and pool.pages_used == 0
    assert pool.nbytes == 4 * ((N_PAGES + 2 * N_SLOTS) * H * K * V + N_SLOTS + N_SLOTS * CAP)
    pool.full
    assert pool.nbytes == 4 * ((N_PAGES + 2 * N_SLOTS) * H * K * V + 2 * N_SLOTS + N_SLOTS * CAP)
    assert pool.to_ragged() is pool
    with pytest.raises(ValueError, match="non-positive"):
        PagedCausalState.empty(N_SLOTS, H, K, V, CAP, 0, "cpu")


@pytest.mark.parametrize("rows, what", [
    ([[0, -1, -1, -1]] * 4, "4 rows, the pool 5 slots"),
    ([[0, -1, -1, -1]] * 4 + [[1, -1]], r"rows \[4\] do not have the 4 entries"),
    ([[0, -1, -1, 9]] + [[-1] * 4] * 4, r"entries \[9\] are outside -1 \.\. 8"),
    ([[0, -2, -1, 12]] + [[-1] * 4] * 4, r"entries \[-2, 12\] are outside -1 \.\. 8"),
    ([[0, 1.0, -1, -1]] + [[-1] * 4] * 4, r"must be ints, got \[1\.0\]"),
    ([[True, -1, -1, -1]] + [[-1] * 4] * 4, "must be ints"),
    ([[3, 3, -1, -1]] + [[-1] * 4] * 4, r"pages \[3\] are named more than once within one slot"),
])
def test_a_bad_table_is_refused_by_name(rows, what, no_library):
    z = lambda *s: torch.zeros(s)
    with pytest.raises(ValueError, match=what):
        PagedCausalState(z(N_PAGES, H, K, V), z(N_SLOTS, H, K, V), z(N_SLOTS, H, K, V), rows)


def test_the_constructor_holds_lengths_to_the_table(no_library):
    with pytest.raises(ValueError, match=r"slots \[4\] hold tokens in chunks that have no page: \{4: \[2\]\}"):
        new_pool(rows=ROWS[:4] + [[7, 5, -1, -1]])
    with pytest.raises(IndexError, match=r"slots \[1\].*exceed the capacity of 4 chunks"):
        new_pool(lengths=(5, 257, 0, 63, 130))
    z = lambda *s: torch.zeros(s)
    with pytest.raises(ValueError, match=r"pages \[n_pages, Hkv, K, V\]"):
        PagedCausalState(z(N_PAGES, H, K, V), z(N_SLOTS, H, K, V + 4), z(N_SLOTS, H, K, V + 4), ROWS)
    with pytest.raises(ValueError, match="contiguous float32"):
        PagedCausalState(z(N_PAGES, H, K, V).double(), z(N_SLOTS, H, K, V), z(N_SLOTS, H, K, V), ROWS)
    pool = new_pool()
    assert pool.lengths == LENGTHS and pool.pos.tolist() == list(LENGTHS) and pool.pages_used == 5 and sorted(pool.free) == [0, 1, 3, 8]
    counts_consistent(pool)
    # a page named by two slots is a shared page
    shared = new_pool(lengths=(64, 64, 0, 0, 0), rows=[[3, -1, -1, -1], [3, 8, -1, -1]] + [[-1] * 4] * 3)
    assert shared.refs[3] == 2 and shared.pages_used == 2
    counts_consistent(shared)


def test_the_pool_itself_is_no_state(no_library):
    pool = new_pool()
    q, k, v, mix = toks(N_SLOTS)
    for fn in (mhla_amd.mhla_causal_step, mhla_amd.mhla_causal_step_dev, mhla_amd.mhla_causal_extend, mhla_amd.mhla_causal_verify):
        with pytest.raises(TypeError, match=r"is a pool, not a state: pass pool\.at\(slots\)"):
            fn(q, k, v, mix, pool)
    draft = ops.CausalDraft(k, v, (1,) * N_SLOTS, False, LENGTHS)
    with pytest.raises(TypeError, match=r"pool\.at\(slots\)"):
        mhla_amd.mhla_causal_commit(draft, mix, pool, (1,) * N_SLOTS)
    with pytest.raises(TypeError, match=r"pool\.at\(slots\)"):
        CausalState.cat([pool])
    with pytest.raises(TypeError, match="into must be a CausalStateView"):
        mhla_amd.mhla_causal_state(k[:1], v[:1], mix, cu_seqlens=[0, 1], into=pool)
    with pytest.raises(ValueError, match="not copied as a whole"):
        pool.clone()


def test_views_and_their_refusals(no_library):
    pool = new_pool()
    view = pool.at([3, 0, 4])
    assert isinstance(view, PagedStateView) and isinstance(view, mhla_amd.CausalStateView) and view.pool is pool
    assert view.lengths == (63, 5, 130) and view.rows == 3 and view.capacity_chunks == CAP and view.pages is pool.pages
    assert view.P is pool.P and view.Cur is pool.Cur and view.pos is pool.pos and view.full is pool.full
    with pytest.raises(AttributeError, match="no dense S"):
        view.S
    for slots, what in (([3, 3], "more than once"), ([5], "outside 0"), ([], "no slot given"), ([1.0], "must be ints")):
        for call in (pool.at, pool.reset, pool.trim, lambda s: pool.reserve(s, 1)):
            with pytest.raises(ValueError, match=what):
                call(slots)
    with pytest.raises(ValueError, match="view of a view"):
        view.at([0])
    with pytest.raises(ValueError, match="on the pool"):
        view.reset([0])
    dev_view = pool.at(torch.tensor([3, -1, 4], dtype=torch.int32))
    q, k, v, mix = toks(3)
    for fn in (mhla_amd.mhla_causal_step, mhla_amd.mhla_causal_extend, mhla_amd.mhla_causal_verify):
        with pytest.raises(ValueError, match="only mhla_causal_step_dev takes"):
            fn(q, k, v, mix, dev_view)
    with pytest.raises(ValueError, match="only mhla_causal_step_dev takes"):
        dev_view.compact()
    pool.stale = True
    for call in (lambda: mhla_amd.mhla_causal_step(q, k, v, mix, view), view.compact, lambda: pool.reset([0]), lambda: pool.trim([0]),
                 lambda: pool.fork(0, 1)):
        with pytest.raises(ValueError, match="stale"):
            call()
    assert pool.reserve([1], 1) is pool and pool.table[1][0] == 0, "reserve reads the table alone: a stale pool is fine"
    pool.stale = False
    with pytest.raises(IndexError, match=r"slots \[1\] would hold more than the capacity"):
        pool.reserve([0, 1], [5, 257])
    assert pool.lengths == LENGTHS


def test_compact_gathers_pages_into_a_dense_state(no_library):
    pool = new_pool()
    g = torch.Generator().manual_seed(1)
    for t in (pool.pages, pool.P, pool.Cur):
        t.copy_(torch.randn(t.shape, generator=g))
    c = pool.at([4, 0]).compact()
    assert type(c) is CausalState and c.lengths == (130, 5) and tuple(c.S.shape) == (2, H, CAP, K, V) and c.pos.tolist() == [130, 5]
    for j, p in enumerate((7, 5, 2)):
        assert torch.equal(c.S[0, :, j], pool.pages[p])
    assert torch.equal(c.S[1, :, 0], pool.pages[4]) and float(c.S[0, :, 3].abs().max()) == float(c.S[1, :, 1:].abs().max()) == 0.0
    assert torch.equal(c.P, pool.P[[4, 0]]) and torch.equal(c.Cur, pool.Cur[[4, 0]]) and c.P.data_ptr() != pool.P.data_ptr()
    both = CausalState.cat([pool.at([4]), pool.at([0])])
    assert both.lengths == (130, 5) and torch.equal(both.S, c.S)


def test_pool_exhausted_is_all_or_nothing():
    from mhla_amd import build
    build.build(verbose=False)
    pool = new_pool()
    table, refs, free = [list(r) for r in pool.table], list(pool.refs), sorted(pool.free)
    # slots 1 and 2 to 256 tokens and slot 0 to 65: 4 + 4 + 1 = 9 pages, 4 are free
    with pytest.raises(PoolExhausted, match=r"slots \[0, 1, 2\] need 9 more pages, the pool has 4 free \(of 9") as e:
        pool.reserve([1, 2, 0], [256, 256, 65])
    assert isinstance(e.value, RuntimeError)
    assert pool.table == table and pool.refs == refs and sorted(pool.free) == free and pool.lengths == LENGTHS
    counts_consistent(pool)
    # a host-positioned call: the extend of slot 0 by 250 tokens needs 3 more pages beside slot 3's one; nothing moves, nothing launches
    q, k, v, mix = toks(2, 250)
    pool.reserve([1], 192)   # (one page is left)
    with pytest.raises(PoolExhausted, match=r"mhla_causal_extend: slots \[0\] need 3 more pages, the pool has 1 free"):
        with Session(ops, _lib) as s:
            s.call("extend", mhla_amd.mhla_causal_extend, q, k, v, mix, pool.at([0, 3]), counts=(250, 1), catch=False)
    assert s.calls == [] and pool.lengths == LENGTHS and pool.pos.tolist() == list(LENGTHS) and pool.pages_free == 1
    counts_consistent(pool)


def test_reference_counts_through_reserve_fork_reset_and_trim(no_library):
    pool = new_pool()
    g = torch.Generator().manual_seed(2)
    for t in (pool.P, pool.Cur):
        t.copy_(torch.randn(t.shape, generator=g))
    pool.full[4] = 1
    assert pool.reserve([1, 0], [65, 5]) is pool
    assert pool.table[1] == [0, 1, -1, -1] and pool.table[0] == ROWS[0], "the lowest free pages first; slot 0 had its page"
    counts_consistent(pool)
    pool.reset([1])
    assert pool.table[1] == [-1] * 4 and sorted(pool.free) == [0, 1, 3, 8]
    # slot 4 (130 tokens: chunks 0 and 1 finished, on pages 7 and 5) shared by three slots
    assert pool.fork(4, 1) is pool and pool.fork(4, 2) is pool
    assert pool.table[1] == pool.table[2] == [7, 5, -1, -1] and pool.refs[7] == pool.refs[5] == 3 and pool.refs[2] == 1
    assert pool.pages_used == 5, "no page was taken: the finished chunks by reference, the open one lives in Cur"
    assert pool.lengths == (5, 130, 130, 63, 130) and pool.pos.tolist() == [5, 130, 130, 63, 130] and pool.full.tolist() == [0, 1, 1, 0, 1]
    assert torch.equal(pool.P[1], pool.P[4]) and torch.equal(pool.Cur[2], pool.Cur[4])
    counts_consistent(pool)
    pool.reset([4])
    assert pool.refs[7] == pool.refs[5] == 2 and pool.refs[2] == 0 and 2 in pool.free and 7 not in pool.free
    assert pool.lengths[4] == 0 and float(pool.P[4].abs().max()) == float(pool.Cur[4].abs().max()) == 0.0 and pool.full.tolist() == [0, 1, 1, 0, 0]
    pool.reset([1])
    assert pool.refs[7] == pool.refs[5] == 1 and 7 not in pool.free and 5 not in pool.free
    counts_consistent(pool)
    pool.reset([2])
    assert pool.refs[7] == pool.refs[5] == 0 and {7, 5} <= set(pool.free), "freed by the last release only"
    counts_consistent(pool)
    # a fork over a slot that held pages releases them first; forking back shares again
    pool.reserve([2], 100)
    held = pool.table[2][:2]
    pool.fork(3, 2)
    assert pool.table[2] == [-1] * 4 and all(pool.refs[p] == 0 for p in held) and pool.lengths[2] == 63, "63 tokens: no finished chunk to share"
    # trim: beyond ceil(length / 64) chunks
    pool.reserve([3, 0], [200, 64])
    assert [p >= 0 for p in pool.table[3]] == [True] * 4 and pool.table[0][1] == -1
    pool.trim([3, 0])
    assert pool.table[3] == [6, -1, -1, -1] and pool.table[0] == [4, -1, -1, -1]
    counts_consistent(pool)
    with pytest.raises(ValueError, match=r"\[2\] are given more than once"):
        pool.fork(2, 2)


def test_the_six_entry_points_are_declared_exported_and_bound():
    from mhla_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mhla_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared in include/mhla_hip.h"
        assert name in _lib.SIGNATURES and callable(getattr(lib, name))
        # `float* S` of the slotted namesake replaced by (pages, n_pages, table_dev): two parameters more
        slots = _lib.SIGNATURES[name.replace("_paged", "_slots")][1]
        args = _lib.SIGNATURES[name][1]
        at = slots.index(_lib.c_int) + 1   # (S follows ldmix, the first int)
        assert args == slots[:at] + [_lib.c_void_p, _lib.c_int, _lib.c_void_p] + slots[at + 1:]
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == len(args) and "float* pages, int n_pages" in decl and "const int32_t* table_dev, int cap_chunks" in " ".join(decl.split())
    assert lib.mhla_abi_version() == _lib.ABI_VERSION == 9
    # the host checks of the pages and the table come first, then the map's, and need no device
    null = _lib.NULL_VIEW
    buf = (_lib.ctypes.c_float * 8)()
    addr = (_lib.ctypes.addressof(buf) + 15) // 16 * 16
    commit = lambda pages, n_pages, table: lib.mhla_causal_commit_paged(null, null, None, 0, pages, n_pages, table, 4, None, None, None, None, 5, None,
                                                                        None, 1, 0, 0, 0, 0, None, 0, 1, 1, 4, 4, 64, 0, None)
    for args, what in (((None, 9, addr), b"pages null"), ((addr + 4, 9, addr), b"pages null or not 16-byte aligned"),
                       ((addr, 9, None), b"table_dev null"), ((addr, 9, addr + 2), b"table_dev null or not 4-byte aligned"),
                       ((addr, 0, addr), b"n_pages=0 must be positive"), ((addr, 9, addr), b"slot_dev null")):
        assert commit(*args) != 0
        assert what in lib.mhla_last_error(), (what, lib.mhla_last_error())


ENTRIES = {"step": "mhla_causal_step_paged", "step_dev": "mhla_causal_step_dev_paged", "extend": "mhla_causal_extend_paged",
           "verify": "mhla_causal_verify_paged", "commit": "mhla_causal_commit_paged"}
# the table after the call: chunks 0 .. ceil(n_after / 64) - 1 of the view's slots [3, 0, 4], the lowest free page first (0, 1, 3, 8)
RULE = {"step": {3: [6, -1, -1, -1], 0: [4, -1, -1, -1], 4: [7, 5, 2, -1]},          # 64, 6, 131 tokens: every page was there
        "step_dev": {3: [6, -1, -1, -1], 0: [4, -1, -1, -1], 4: [7, 5, 2, -1]},      # never assigns
        "extend": {3: [6, 0, -1, -1], 0: [4, -1, -1, -1], 4: [7, 5, 2, 1]},          # 63 + 3, 5 + 2, 130 + 70
        "verify": {3: [6, 0, -1, -1], 0: [4, -1, -1, -1], 4: [7, 5, 2, 1]},          # the draft's end
        "commit": {3: [6, 0, -1, -1], 0: [4, -1, -1, -1], 4: [7, 5, 2, 1]}}          # what the verify assigned covers what is accepted
COUNTS, ACCEPT = (3, 2, 70), (1, 2, 1)


def _run(entry, s, device_map=False):
    """One public call of `entry` on the view [3, 0, 4] of a CPU pool; returns (its library calls, the pool, the view)."""
    from mhla_amd import build
    build.build(verbose=False)
    pool = new_pool()
    view = pool.at(torch.tensor([3, 0, 4], dtype=torch.int32) if device_map else [3, 0, 4])
    q, k, v, mix = toks(3, 1 if "step" in entry else 70)
    s.name(q=q, k=k, v=v, mix=mix, pages=pool.pages, table=pool.table_dev, P=pool.P, Cur=pool.Cur, pos=pool.pos, full=pool.full, map=view.map)
    first = len(s.calls)
    call = lambda fn, *a, **kw: s.call(entry, fn, *a, catch=False, **kw)
    if entry == "step":
        call(mhla_amd.mhla_causal_step, q, k, v, mix, view)
    elif entry == "step_dev":
        call(mhla_amd.mhla_causal_step_dev, q, k, v, mix, view)
    elif entry == "extend":
        call(mhla_amd.mhla_causal_extend, q, k, v, mix, view, counts=COUNTS)
    else:
        _, draft = call(mhla_amd.mhla_causal_verify, q, k, v, mix, view, counts=COUNTS)
        assert draft.view is view
        if entry == "commit":
            first = len(s.calls)
            with pytest.raises(TypeError, match=r"pool\.at\(slots\)"):
                mhla_amd.mhla_causal_commit(draft, mix, pool, ACCEPT)
            with pytest.raises(ValueError, match="pass the view"):
                mhla_amd.mhla_causal_commit(draft, mix, pool.at([3, 0, 1]), ACCEPT)
            assert call(mhla_amd.mhla_causal_commit, draft, mix, view, ACCEPT) is view
    return s.calls[first:], pool, view


def _pointers(call):
    out = {}
    for a in call.args:
        if isinstance(a, tuple) and a[0] == "ptr":
            out.setdefault(a[1], []).append(a[2])
    return out


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_a_view_makes_the_paged_call_and_follows_the_page_rule(entry):
    with Session(ops, _lib) as s:
        calls, pool, view = _run(entry, s, device_map=entry == "step_dev")
    assert [c.name for c in calls] == [ENTRIES[entry]] and batch_of(calls[0]) == 3
    ptr = _pointers(calls[0])
    assert all(ptr[n] == [0] for n in ("mix", "pages", "table", "P", "Cur", "pos", "map") + (("full",) if entry == "step_dev" else ()))
    args = calls[0].args
    i = args.index(("ptr", "pages", 0))
    assert args[i + 1] == N_PAGES and args[i + 2] == ("ptr", "table", 0) and args[i + 3] == CAP and args[i + 4] == ("ptr", "P", 0), \
        "pages, n_pages, table_dev, then the capacity, where the slotted call has S and the capacity"
    i = args.index(("ptr", "map", 0))
    assert args[i - 1] == ("ptr", "pos", 0) and args[i + 1] == N_SLOTS, "the map and the pool's size follow the positions"
    assert pool.lengths == {"step": (6, 0, 0, 64, 131), "extend": (7, 0, 0, 66, 200), "commit": (7, 0, 0, 64, 131)}.get(entry, LENGTHS)
    assert pool.stale == (entry == "step_dev")
    for slot, row in RULE[entry].items():
        assert pool.table[slot] == row, f"{entry}: the page rule for slot {slot}"
    assert pool.table[1] == pool.table[2] == [-1] * CAP
    counts_consistent(pool)
    if entry == "commit":   # slot 4 accepted 1 of 70: the page its draft reached goes back
        pool.trim([3, 0, 4])
        assert pool.table[4] == [7, 5, 2, -1] and pool.table[3] == [6, -1, -1, -1] and pool.table[0] == [4, -1, -1, -1]
        counts_consistent(pool)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_a_sliced_paged_view_slices_its_map_and_not_the_pool(entry, monkeypatch):
    monkeypatch.setattr(ops, "_MAX_GRID_BH", 2 * H)
    with Session(ops, _lib) as s:
        calls, pool, view = _run(entry, s)
    assert [c.name for c in calls] == [ENTRIES[entry]] * 2 and [batch_of(c) for c in calls] == [2, 1]
    for c, first in zip(calls, (0, 2)):
        ptr = _pointers(c)
        assert ptr["map"] == [4 * first], "rows [first, ...) of the map"
        assert all(ptr[n] == [0] for n in ("pages", "table", "P", "Cur", "pos") + (("full",) if entry == "step_dev" else ())), "the pool passes whole"
        for a in c.args:
            if isinstance(a, tuple) and a[0] == "view":
                assert a[2] == first * a[3], f"{c.name}: the view of {a[1]} does not start at row {first}"


def test_a_pack_prefill_into_a_paged_view_is_one_paged_call():
    from mhla_amd import build
    build.build(verbose=False)
    pool = new_pool()
    view = pool.at([4, 1])
    _, k, v, mix = toks(1, 70)
    with Session(ops, _lib) as s:
        s.name(k=k, v=v, mix=mix, pages=pool.pages, table=pool.table_dev, P=pool.P, Cur=pool.Cur, pos=pool.pos, map=view.map)
        assert s.call("prefill", mhla_amd.mhla_causal_state, k, v, mix, cu_seqlens=[0, 64, 70], into=view, catch=False) is view
    assert [c.name for c in s.calls] == ["mhla_causal_varlen_state_init_paged"]
    args = s.calls[0].args
    i = args.index(("ptr", "pages", 0))
    assert args[i + 1] == N_PAGES and args[i + 2] == ("ptr", "table", 0) and args[i + 3] == CAP
    i = args.index(("ptr", "map", 0))
    assert args[i - 2] == 2 and args[i - 1][0] == "ptr" and args[i - 1][1].startswith("new") and args[i + 1] == N_SLOTS, \
        "n_seqs, the pack's own lengths (not the pool's positions), the map, the pool's size"
    assert pool.lengths == (5, 6, 0, 63, 64) and pool.pos.tolist() == [5, 6, 0, 63, 64] and view.lengths == (64, 6)
    # the slots start anew: slot 4's three pages went back, then one page each by the rule, the lowest free first
    assert pool.table[4] == [0, -1, -1, -1] and pool.table[1] == [1, -1, -1, -1] and pool.pages_used == 4
    counts_consistent(pool)
    # a pack that does not fit raises before anything changes -- the pages a fresh start gives back count as free
    table = [list(r) for r in pool.table]
    _, k, v, mix = toks(1, 256 + 200)
    pool.reserve([2], 200)
    with pytest.raises(PoolExhausted, match=r"mhla_causal_state: slots \[1, 4\] need 8 more pages, the pool has 3 free"):
        with Session(ops, _lib) as s:
            s.call("prefill", mhla_amd.mhla_causal_state, k, v, mix, cu_seqlens=[0, 256, 456], into=view, catch=False)
    assert s.calls == [] and pool.table[4] == table[4] and pool.table[1] == table[1] and pool.lengths == (5, 6, 0, 63, 64)
    counts_consistent(pool)


def test_sync_names_a_missing_page(no_library):
    pool = new_pool()
    pool.full[3] = 1
    with pytest.raises(IndexError, match=r"PagedCausalState\.sync: sequences \[3\] were stepped beyond the capacity of 4 chunks \(256 tokens\) or onto "
                                         r"a chunk that has no page"):
        pool.sync()
    dense = CausalState.empty(2, H, K, V, CAP, "cpu").to_ragged()
    dense.full[1] = 1
    with pytest.raises(IndexError, match=r"^CausalState\.sync: sequences \[1\] were stepped beyond the capacity of 4 chunks \(256 tokens\): their rows"):
        dense.sync()
