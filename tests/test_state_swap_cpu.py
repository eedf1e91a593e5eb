"""Swapping slots of a paged state pool out and back in (`PagedCausalState.swap_out` / `swap_in`, `SwappedSlots`), host side, no GPU:
the blob's size against the layout's arithmetic, the host bookkeeping of both directions against `reset` and the page rule, shared
pages stored once, the library calls a swap makes (recorded by tools/fake_decode_lib.py on CPU tensors) -- one on a device blob, a
tiling of the item list on a host blob --, every refusal before anything is launched or changed, and the checks of the two entry
points that return before a launch.  The pools are `pool_util.host_pool`, as in test_state_paged_h16_cpu.py: lengths (63, 5, 130) at
slots [3, 0, 4], a scrambled table."""
import os
import re
import sys

import pytest
import torch

from mhla_amd import PagedCausalState, PoolExhausted, SwappedSlots, _lib, ops
from pool_util import CAP, GROUP, HOST_DIMS, HOST_ROWS as ROWS, N_SLOTS, host_pool, host_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fake_decode_lib import Session  # noqa: E402

H, K, V, N_PAGES = HOST_DIMS
FORMATS = ["fp32", "h16"]
OUT, IN = "mhla_causal_swap_out_paged", "mhla_causal_swap_in_paged"
EINVAL = -22


def _build():
    from mhla_amd import build
    build.build(verbose=False)


def up16(n):
    return (n + 15) // 16 * 16


def seq_bytes(Hkv, K, V):
    """P and Cur, fp32, then pos and full as two int32 padded to 16 bytes."""
    return 2 * 4 * Hkv * K * V + 16


def page_bytes(Hkv, K, V, fmt):
    """fp32: the chunk; h16: the fp16 payload, then one fp32 multiplier per 64 elements, padded to 16 bytes."""
    return 4 * Hkv * K * V if fmt == "fp32" else up16(2 * Hkv * K * V + 4 * Hkv * (K * V // GROUP))


def state(pool):
    """Every host field of a pool, and the device positions."""
    return host_state(pool) + (list(pool.have), pool.pages_free, pool.pages_used, pool.seen, pool.stale)


def swap_out(pool, slots, **kw):
    with Session(ops, _lib) as s:
        blob = s.call("swap_out", pool.swap_out, slots, catch=False, **kw)
    return blob, s.calls


def swap_in(pool, blob, slots):
    with Session(ops, _lib) as s:
        s.call("swap_in", pool.swap_in, blob, slots, catch=False)
    return s.calls


# ---- the blob's size
@pytest.mark.parametrize("Hkv, K, V", [(2, 64, 64), (2, 40, 72), (3, 8, 24)], ids=["64x64", "40x72", "8x24"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_the_blob_size_is_the_layouts_arithmetic(fmt, Hkv, K, V):
    _build()
    lib = _lib.load()
    code = FORMATS.index(fmt)
    sb, pb = seq_bytes(Hkv, K, V), page_bytes(Hkv, K, V, fmt)
    assert sb % 16 == 0 and pb % 16 == 0
    if fmt == "h16" and (K, V) != (64, 64):
        assert (4 * Hkv * (K * V // GROUP)) % 16 != 0, "a multiplier section that needs padding"
    assert lib.mhla_causal_swap_ws_bytes(1, 0, Hkv, K, V, code) == sb
    assert lib.mhla_causal_swap_ws_bytes(0, 1, Hkv, K, V, code) == pb
    for n_seqs, n_pages in ((0, 0), (3, 0), (2, 5), (7, 11)):
        assert lib.mhla_causal_swap_ws_bytes(n_seqs, n_pages, Hkv, K, V, code) == n_seqs * sb + n_pages * pb
    # sizes it does not take
    assert lib.mhla_causal_swap_ws_bytes(-1, 0, Hkv, K, V, code) == 0 and lib.mhla_causal_swap_ws_bytes(1, 1, Hkv, K, V, 2) == 0
    assert lib.mhla_causal_swap_ws_bytes(1, 1, Hkv, 3, 6, 0) == 0, "K V % 4"
    assert lib.mhla_causal_swap_ws_bytes(1, 1, Hkv, 8, 12, 1) == 0 and lib.mhla_causal_swap_ws_bytes(1, 1, Hkv, 8, 12, 0) > 0, "K V % 64 on h16 pages alone"


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_blob_reports_the_size_the_library_gives(fmt):
    _build()
    blob, _ = swap_out(host_pool(fmt), [3, 0, 4], release=False)
    assert blob.nbytes == blob.buffer.numel() == 3 * seq_bytes(H, K, V) + 2 * page_bytes(H, K, V, fmt)
    assert blob.buffer.dtype == torch.uint8 and blob.buffer.is_contiguous() and blob.buffer.data_ptr() % 16 == 0
    assert blob.nbytes == _lib.load().mhla_causal_swap_ws_bytes(3, 2, H, K, V, FORMATS.index(fmt))
    assert blob.host and blob.device.type == "cpu" and blob.n_seqs == 3 and "n_pages=2" in repr(blob)
    again = blob.to("cpu")
    assert again.buffer is not blob.buffer and torch.equal(again.buffer, blob.buffer) and again.host
    assert (again.lengths, again.seq_pages, again.n_pages, again.dims, again.page_format) == (blob.lengths, blob.seq_pages, 2, (H, K, V), fmt)


# ---- host bookkeeping of swap_out
@pytest.mark.parametrize("fmt", FORMATS)
def test_swap_out_leaves_the_pool_as_reset_does(fmt):
    _build()
    pool, twin = host_pool(fmt), host_pool(fmt)
    blob, calls = swap_out(pool, [3, 4])
    twin.reset([3, 4])
    assert isinstance(blob, SwappedSlots) and blob.lengths == (63, 130) and blob.page_format == fmt and blob.dims == (H, K, V)
    assert blob.n_pages == 2 and blob.seq_pages == ((), (0, 1)), "0 + 2 finished pages: the open chunks' pages 6 and 2 are not saved"
    assert state(pool) == state(twin), "table, refs, free, have, lengths and pages_free are those after reset([3, 4])"
    assert pool.table[0] == ROWS[0] and pool.lengths[0] == 5 and pool.refs[4] == 1, "slot 0 is untouched"
    assert pool.table[3] == pool.table[4] == [-1] * CAP and pool.lengths == (5, 0, 0, 0, 0) and sorted(pool.free) == [0, 1, 2, 3, 5, 6, 7, 8]
    assert pool.pos.tolist() == [5, 0, 0, 0, 0]
    assert len(calls) >= 1 and {c.name for c in calls} == {OUT}


@pytest.mark.parametrize("fmt", FORMATS)
def test_release_false_leaves_every_host_field(fmt):
    _build()
    pool = host_pool(fmt)
    before = state(pool)
    blob, calls = swap_out(pool, [3, 0, 4], release=False)
    assert state(pool) == before and blob.lengths == (63, 5, 130) and blob.seq_pages == ((), (), (0, 1))
    assert [c.name for c in calls] == [OUT]


# ---- the call log
def _ranges(calls):
    return [(c.args[11], c.args[12]) for c in calls]


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_device_blob_is_one_call_on_the_named_pool(fmt, monkeypatch):
    _build()
    pool = host_pool(fmt)
    pool.full
    seen = []
    launch = ops._swap_launch
    monkeypatch.setattr(ops, "_swap_launch", lambda d, p, b, items: (seen.append((d, list(items))), launch(d, p, b, items))[1])
    with Session(ops, _lib) as s:
        s.name(pages=pool.pages, mult=pool.page_mult, P=pool.P, Cur=pool.Cur, pos=pool.pos, full=pool.full, table=pool.table_dev)
        blob = s.call("swap_out", pool.swap_out, [3, 4], device=None, catch=False)
        s.name(blob=blob.buffer)
        other = PagedCausalState.empty(3, H, K, V, 5, 6, "cpu", page_format=fmt)
        s.call("swap_in", other.swap_in, blob, [2, 0], catch=False)
    assert not blob.host and [c.name for c in s.calls] == [OUT, IN]
    mult = ("ptr", "mult", 0) if fmt == "h16" else ("null",)
    out = s.calls[0].args
    assert out[:8] == (("ptr", "pages", 0), mult, N_PAGES, ("ptr", "P", 0), ("ptr", "Cur", 0), ("ptr", "pos", 0), ("ptr", "full", 0), N_SLOTS)
    assert out[8][0] == "ptr" and out[8][1].startswith("new") and out[9:13] == (2, 2, 0, 4), "the item list, n_seqs, n_pages_moved, [i0, i1)"
    assert out[13][0] == "ptr" and out[13][2] == 0 and out[14:17] == (H, K, V) and out[17][0] == "stream"
    assert len(out) == len(_lib.SIGNATURES[OUT][1]) == len(_lib.SIGNATURES[IN][1])
    back = s.calls[1].args
    assert back[2] == 6 and back[7] == 3 and back[9:13] == (2, 2, 0, 4) and back[13] == ("ptr", "blob", 0) and back[14:17] == (H, K, V)
    assert all(a[0] == "ptr" and a[1] not in ("pages", "mult", "P", "Cur", "pos", "full") for a in back[:2] + back[3:7] if a != ("null",))
    # the item lists: the slots in call order, then the pool page of every blob page
    assert seen == [("out", [3, 4, 7, 5]), ("in", [2, 0, 1, 2])]
    assert other.table[2] == [0, -1, -1, -1, -1] and other.table[0] == [1, 2, 3, -1, -1] and other.lengths == (130, 0, 63)


@pytest.mark.parametrize("cap", ["one-byte", "one-sequence", "sequence-and-page"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_host_blob_is_staged_in_slices_that_tile_the_item_list(fmt, cap, monkeypatch):
    _build()
    sb, pb = seq_bytes(H, K, V), page_bytes(H, K, V, fmt)
    assert 2 * pb <= sb
    cap = {"one-byte": 1, "one-sequence": sb, "sequence-and-page": sb + pb}[cap]
    at = lambda i: i * sb if i < 3 else 3 * sb + (i - 3) * pb
    monkeypatch.setattr(ops, "SWAP_STAGE_CAP_BYTES", cap)
    pool = host_pool(fmt)
    blob, calls = swap_out(pool, [3, 0, 4], device="cpu")   # 3 sequences + 2 pages = 5 items
    target = PagedCausalState.empty(4, H, K, V, CAP, 7, "cpu", page_format=fmt)
    back = swap_in(target, blob, [1, 3, 0])
    for name, log in ((OUT, calls), (IN, back)):
        assert len(log) >= 3 and {c.name for c in log} == {name}
        ranges = _ranges(log)
        assert ranges[0][0] == 0 and ranges[-1][1] == 5 and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), f"{ranges} tile [0, 5)"
        assert all(i < j and (at(j) - at(i) <= cap or j == i + 1) for i, j in ranges), "whole items within the cap; a single item where none fits"
        assert len({c.args[13] for c in log}) == 1 and log[0].args[13][2] == 0, "one staging buffer, reused from its start"
        assert all(c.args[9:11] == (3, 2) for c in log)
    if cap == 1:
        assert _ranges(calls) == [(i, i + 1) for i in range(5)]
    elif cap == sb:
        assert _ranges(calls) == [(0, 1), (1, 2), (2, 3), (3, 5)]
    else:
        assert _ranges(calls) == [(0, 1), (1, 2), (2, 4), (4, 5)]
    assert blob.host and target.lengths == (130, 63, 0, 5) and target.table[0][:3] == [2, 3, 4] and target.table[1][0] == 0 and target.table[3][0] == 1


# ---- shared pages
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_shared_page_is_stored_once_and_placed_once(fmt):
    _build()
    pool = host_pool(fmt).fork(4, 2)
    assert pool.table[2] == [7, 5, -1, -1] and pool.refs[7] == pool.refs[5] == 2
    blob, _ = swap_out(pool, [4, 2])
    assert blob.n_pages == 2 and blob.seq_pages == ((0, 1), (0, 1)) and blob.lengths == (130, 130)
    assert pool.refs[7] == pool.refs[5] == 0 and pool.pages_used == 2, "both holders left: slots 0 and 3 keep their pages"
    target = PagedCausalState.empty(3, H, K, V, CAP, 6, "cpu", page_format=fmt)
    swap_in(target, blob, [2, 0])
    assert target.table[2] == [0, 1, 2, -1] and target.table[0] == [0, 1, 3, -1], "the same two pages, and a page each for the open chunk"
    assert target.refs == [2, 2, 1, 1, 0, 0] and sorted(target.free) == [4, 5] and target.have == [3, 0, 3]
    assert target.lengths == (130, 0, 130) and target.table_dev.tolist() == target.table
    # a second swap_in of the same blob: a fork across pools
    swap_in(pool, blob, [1, 2])
    assert pool.table[1][:2] == pool.table[2][:2] and pool.refs[pool.table[1][0]] == 2 and pool.lengths == (5, 130, 130, 63, 0)


@pytest.mark.parametrize("fmt", FORMATS)
def test_swapping_out_one_holder_leaves_the_other(fmt):
    _build()
    pool = host_pool(fmt).fork(4, 2)
    blob, _ = swap_out(pool, [4])
    assert blob.n_pages == 2 and blob.seq_pages == ((0, 1),)
    assert pool.table[2] == [7, 5, -1, -1] and pool.refs[7] == pool.refs[5] == 1 and pool.lengths[2] == 130 and pool.pos.tolist()[2] == 130
    assert pool.table[4] == [-1] * CAP and pool.refs[2] == 0 and 2 in pool.free and 7 not in pool.free


# ---- refusals
def _refused(pool, exc, match, call):
    before = state(pool)
    with Session(ops, _lib) as s:
        with pytest.raises(exc, match=match):
            s.call("refused", call, catch=False)
    assert s.calls == [] and state(pool) == before, "nothing launched, nothing changed"


@pytest.mark.parametrize("fmt", FORMATS)
def test_swap_out_refusals_change_nothing(fmt):
    _build()
    pool = host_pool(fmt)
    for slots, what in (([3, 3], "more than once"), ([5], "outside 0"), ([-1], "outside 0"), ([], "no slot given"), ([1.0], "must be ints")):
        _refused(pool, ValueError, what, lambda: pool.swap_out(slots))
    _refused(pool, ValueError, "'cpu' or the pool's device", lambda: pool.swap_out([3], device="meta"))
    pool.stale = True
    _refused(pool, ValueError, "stale", lambda: pool.swap_out([3]))


@pytest.mark.parametrize("fmt", FORMATS)
def test_swap_in_refusals_change_nothing(fmt):
    _build()
    src = host_pool(fmt)
    blob, _ = swap_out(src, [3, 4], release=False)
    pool = host_pool(fmt)
    for slots, what in (([1, 1], "more than once"), ([1, 5], "outside 0"), ([1, 2.0], "must be ints")):
        _refused(pool, ValueError, what, lambda: pool.swap_in(blob, slots))
    _refused(pool, ValueError, r"1 slots for the 2 sequences", lambda: pool.swap_in(blob, [1]))
    _refused(pool, ValueError, r"3 slots for the 2 sequences", lambda: pool.swap_in(blob, [1, 2, 0]))
    _refused(pool, ValueError, r"slots \[3\] are not empty", lambda: pool.swap_in(blob, [1, 3]))
    pool.reserve([2], 1)   # (length 0, but a page in its row)
    _refused(pool, ValueError, r"slots \[2, 0\] are not empty", lambda: pool.swap_in(blob, [2, 0]))
    _refused(pool, TypeError, "SwappedSlots", lambda: pool.swap_in(blob.buffer, [1, 2]))
    pool.trim([2])
    pool.stale = True
    _refused(pool, ValueError, "stale", lambda: pool.swap_in(blob, [1, 2]))
    pool.stale = False
    # another geometry or format
    other = "fp32" if fmt == "h16" else "h16"
    for target in (PagedCausalState.empty(4, H + 1, K, V, CAP, 9, "cpu", page_format=fmt), PagedCausalState.empty(4, H, 2 * K, V, CAP, 9, "cpu", page_format=fmt),
                   PagedCausalState.empty(4, H, K, 2 * V, CAP, 9, "cpu", page_format=fmt), PagedCausalState.empty(4, H, K, V, CAP, 9, "cpu", page_format=other)):
        _refused(target, ValueError, "nothing is converted", lambda: target.swap_in(blob, [0, 1]))
    # a sequence beyond the target's capacity
    short = PagedCausalState.empty(4, H, K, V, 2, 9, "cpu", page_format=fmt)
    _refused(short, IndexError, r"slots \[1\] would hold more than the capacity of 2 chunks", lambda: short.swap_in(blob, [0, 1]))
    exact = PagedCausalState.empty(2, H, K, V, 3, 4, "cpu", page_format=fmt)
    swap_in(exact, blob, [0, 1])
    assert exact.lengths == (63, 130) and exact.pages_free == 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_pool_exhausted_is_raised_before_anything_changes(fmt):
    _build()
    blob, _ = swap_out(host_pool(fmt), [3, 4], release=False)   # needs 1 + 3 pages
    pool = host_pool(fmt)                                       # 4 free of 9 ...
    pool.reserve([0], 65)                                      # ... 3 free: one too few
    assert pool.pages_free == 3
    _refused(pool, PoolExhausted, r"need 4 pages, the pool has 3 free", lambda: pool.swap_in(blob, [1, 2]))
    pool.reset([0])
    calls = swap_in(pool, blob, [1, 2])
    assert [c.name for c in calls] == [IN] and pool.lengths == (0, 63, 130, 63, 130) and pool.pages_free == 1
    assert pool.table[1] == [0, -1, -1, -1] and pool.table[2] == [1, 3, 4, -1], "lowest free page first"


def test_entry_points_abi_and_the_checks_ahead_of_a_launch():
    """(the header against `_lib.SIGNATURES`, symbol by symbol: test_host_cpu.py)  Addresses are plain integers here: every call below
    returns before it would launch."""
    _build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mhla_hip.h")).read()
    assert _lib.ABI_VERSION == lib.mhla_abi_version() == 9 and re.search(r"#define MHLA_ABI_VERSION 9\b", header)
    for name in ("mhla_causal_swap_ws_bytes", OUT, IN):
        assert name in _lib.SIGNATURES and callable(getattr(lib, name)) and re.search(r"\b(int|size_t) " + name + r"\(", header)
    assert ops.SWAP_STAGE_CAP_BYTES == ops.EXTEND_WS_CAP_BYTES
    good = dict(pages=4096, mult=None, n_pages=9, P=8192, Cur=12288, pos=64, full=None, n_slots=5, items=128, n_seqs=2, n_moved=2, i0=0, i1=0,
                blob=16384, Hkv=2, K=8, V=16, stream=None)
    for fn in (lib.mhla_causal_swap_out_paged, lib.mhla_causal_swap_in_paged):
        call = lambda **kw: fn(*{**good, **kw}.values())
        assert call() == 0 and call(i0=4, i1=4) == 0 and call(mult=256, full=68, i0=3, i1=3) == 0, "an empty range: 0, no launch"
        bad = [dict(pages=None), dict(P=None), dict(Cur=None), dict(blob=None), dict(pos=None), dict(items=None), dict(pages=4104), dict(P=8196),
               dict(Cur=12296), dict(blob=16392), dict(mult=258), dict(pos=66), dict(full=70), dict(items=130), dict(n_pages=0), dict(n_slots=0),
               dict(Hkv=0), dict(K=0), dict(V=-1), dict(K=3, V=6), dict(mult=256, K=8, V=12), dict(n_seqs=-1), dict(n_moved=-1),
               dict(i0=-1), dict(i0=2, i1=1), dict(i1=5), dict(i0=5, i1=5)]
        for kw in bad:
            assert call(**kw) == EINVAL and lib.mhla_last_error(), kw
