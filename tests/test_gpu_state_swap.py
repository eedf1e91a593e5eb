"""Swapping slots of a paged state pool out and back in on the device (`PagedCausalState.swap_out` / `swap_in`, the library's
mhla_causal_swap_out_paged / mhla_causal_swap_in_paged), fp32 and h16 pages.  A swap is data movement, so EVERY comparison is of bits
(integer views: the NaN poison compares) and there is no tolerance anywhere: the saved pages -- payload and multipliers -- P, Cur,
pos and full come back through other slots, other pages and another pool; a swapped-in slot steps and extends to the bits of one
that never left; shared pages are stored and placed once and their holders write apart; a host blob holds the bytes of the device
blob of the same call, whole or staged in slices; nothing a call does not name changes a bit.  The pools, shapes, tokens,
VIEW = [3, 0, 4], LENGTHS = (63, 5, 130), the poison, the scrambled table, the snapshot and the isolation check are the pool family's
(tests/pool_util.py: `make_pool`, `snapshot`, `check_untouched`).  What a pool holds in pages beyond a sequence's finished chunks (the
open chunk's page, reserved pages) is outside the state's contract and is not saved: `compact()` is compared on the finished chunks."""
import pytest
import torch

import mhla_amd
from mhla_amd import PagedCausalState, PoolExhausted, SwappedSlots, ops
from gpu_util import DEV
from pool_util import CAP, CASES, COUNTS, IDS, LENGTHS, N_PAGES, N_SLOTS, NAN, VIEW, check_untouched, make_pool, same_bits, snapshot, tokens, windows

pytestmark = pytest.mark.gpu

FORMATS = ["fp32", "h16"]
both = lambda f: pytest.mark.parametrize("fmt", FORMATS)(pytest.mark.parametrize("shape", CASES, ids=IDS)(f))


def make(shape, fmt):
    """The family's poisoned pool of 5 slots and 10 pages with LENGTHS at VIEW through the scrambled TABLE, in either page format."""
    return make_pool({"fp32": "paged", "h16": "h16"}[fmt], shape)


def restored(name, pool, slot, was, src):
    """Slot `slot` of `pool` holds what slot `src` held in the snapshot `was`: its finished pages through the table rows -- payload, and
    multipliers on h16 pages --, P, Cur, pos, full and the length."""
    n = was.lengths[src]
    assert pool.lengths[slot] == n and int(pool.pos[slot]) == int(was.pos[src]) == n, f"{name}: length and pos of slot {slot}"
    assert all(p >= 0 for p in pool.table[slot][:-(-n // 64)]) and all(p < 0 for p in pool.table[slot][-(-n // 64):]), f"{name}: ceil(n / 64) pages"
    for j in range(n // 64):
        a, b = pool.table[slot][j], was.table[src][j]
        same_bits(f"{name}: chunk {j} of slot {slot} (page {a}, was page {b})", pool.pages[a], was.chunks[b])
        if pool.page_mult is not None:
            same_bits(f"{name}: multipliers of chunk {j} of slot {slot}", pool.page_mult[a], was.page_mult[b])
    for part in ("P", "Cur", "full"):
        same_bits(f"{name}: {part} of slot {slot}", getattr(pool, part)[slot], getattr(was, part)[src])


def poison(pool, pages, slots=()):
    for t in (pool.pages, pool.page_mult):
        if t is not None and pages:
            t[list(pages)] = NAN
    for t in (pool.P, pool.Cur):
        if slots:
            t[list(slots)] = NAN


def finished(view):
    """`view.compact()` with every chunk beyond a sequence's finished ones zeroed (their pages are outside the contract)."""
    c = view.compact()
    for b, n in enumerate(c.lengths):
        c.S[b, :, n // 64:] = 0
    return c


def same_state(name, a, b, cap=CAP):
    assert a.lengths == b.lengths
    for part in ("P", "Cur", "pos", "full"):
        same_bits(f"{name}: {part}", getattr(a, part), getattr(b, part))
    same_bits(f"{name}: the finished chunks", a.S[:, :, :cap], b.S[:, :, :cap])
    assert float(a.S[:, :, cap:].abs().sum()) == float(b.S[:, :, cap:].abs().sum()) == 0.0


# ---- 1: round trip into other slots and pages
@both
def test_a_round_trip_into_other_slots_and_pages(shape, fmt):
    pool = make(shape, fmt)
    before = snapshot(pool)
    blob = pool.swap_out([3, 4], device=DEV)
    assert isinstance(blob, SwappedSlots) and not blob.host and blob.buffer.device.type == "cuda" and blob.n_pages == 2
    assert blob.lengths == (63, 130) and blob.seq_pages == ((), (0, 1)) and blob.nbytes == blob.buffer.numel()
    check_untouched("swap_out", pool, before, [3, 4])
    assert pool.lengths == (5, 0, 0, 0, 0) and pool.table[3] == pool.table[4] == [-1] * CAP and sorted(pool.free) == [0, 1, 2, 3, 5, 6, 7, 8, 9]
    for part in ("P", "Cur", "pos", "full"):
        assert float(getattr(pool, part)[[3, 4]].float().abs().max()) == 0.0, f"{part} of the released slots, as reset leaves it"
    poison(pool, [6, 7, 5, 2], [3, 4])
    pool.reserve([1], 1)   # (page 0: the free list differs from the one the slots left)
    mid = snapshot(pool)
    assert pool.swap_in(blob, [2, 3]) is pool
    assert pool.table[2] == [1, -1, -1, -1] and pool.table[3] == [2, 3, 5, -1] and pool.lengths == (5, 0, 63, 130, 0), "lowest free page first"
    assert pool.refs[1] == pool.refs[2] == pool.refs[3] == pool.refs[5] == 1 and pool.have[2:4] == [1, 3]
    restored("swap_in", pool, 2, before, 3)
    restored("swap_in", pool, 3, before, 4)
    check_untouched("swap_in", pool, mid, [2, 3], pages=[2, 3])   # (the finished chunks' pages alone: the open chunks' 1 and 5 are not written)
    if fmt == "h16":   # (the same with the writable pages by the rule of the calls: the pages of the two new rows are the only ones it lets change)
        check_untouched("swap_in", pool, mid, [2, 3], reach=(63, 130))
    same_bits("the pages nobody freed or named", pool.pages[[4, 8, 9]], before.chunks[[4, 8, 9]])


# ---- 2: a swapped-in slot goes on like one that never left
@both
def test_a_swapped_in_slot_goes_on_like_one_that_never_left(shape, fmt):
    """Round trip into the same slots through a host blob (other pages); then the same calls on this pool and on a twin that was
    never swapped: two steps on the view -- the 63-token sequence crosses its boundary, a page is written and P re-mixed from the
    pages, the swapped-in ones included -- and, on fp32 pages, one extend with counts (1, 70, 0)."""
    _, _, q, k, v, gate, w, mix = tokens(*shape)
    pool, twin = make(shape, fmt), make(shape, fmt)
    blob = pool.swap_out([3, 4])
    poison(pool, [6, 7, 5, 2], [3, 4])
    pool.reserve([1], 1)
    pool.swap_in(blob, [3, 4])
    assert pool.table != twin.table and pool.lengths == twin.lengths
    for p in (pool, twin):
        p.reset([1])
    rows = {}
    for name, p in (("swapped", pool), ("twin", twin)):
        view = p.at(VIEW)
        out = [mhla_amd.mhla_causal_step(q[:, t:t + 1], k[:, t:t + 1], v[:, t:t + 1], mix, view, gate=gate[:, t:t + 1], norm_weight=w) for t in range(2)]
        if fmt == "fp32":
            wq, wk, wv, wg = (windows(t, COUNTS, False) for t in (q, k, v, gate))
            out.append(mhla_amd.mhla_causal_extend(wq, wk, wv, mix, view, counts=COUNTS, gate=wg, norm_weight=w))
        rows[name] = out
    for a, b in zip(rows["swapped"], rows["twin"]):
        same_bits("rows", a, b)
    after = tuple(n + 2 + (c if fmt == "fp32" else 0) for n, c in zip(LENGTHS, COUNTS))
    assert pool.at(VIEW).lengths == twin.at(VIEW).lengths == after
    same_state("after the calls", finished(pool.at(VIEW)), finished(twin.at(VIEW)))
    torch.cuda.synchronize()
    assert pool.table_dev.tolist() == pool.table and pool.full.tolist() == [0] * N_SLOTS


# ---- 3: shared pages
@both
def test_shared_pages_are_stored_once_and_their_holders_write_apart(shape, fmt):
    _, _, q, k, v, _, _, mix = tokens(*shape)
    pool = make(shape, fmt)
    pool.fork(4, 2)
    before = snapshot(pool)
    blob = pool.swap_out([4, 2], device=DEV)
    assert blob.n_pages == 2 and blob.seq_pages == ((0, 1), (0, 1))
    assert blob.nbytes == ops._swap_bytes(2, 2, shape[2], shape[3], shape[4], fmt)
    poison(pool, [7, 5, 2], [4, 2])
    pool.swap_in(blob, [2, 1])
    assert pool.table[2][:2] == pool.table[1][:2] == [0, 1] and pool.refs[0] == pool.refs[1] == 2, "one pool page per blob page, two holders"
    assert pool.table[2][2] == 2 and pool.table[1][2] == 3 and pool.refs[2] == pool.refs[3] == 1, "and a page each for the open chunk"
    restored("shared swap_in", pool, 2, before, 4)
    restored("shared swap_in", pool, 1, before, 2)
    same_bits("P", pool.P[2], pool.P[1])
    same_bits("Cur", pool.Cur[2], pool.Cur[1])
    mid = snapshot(pool)
    mhla_amd.mhla_causal_step(q[:1, :1], k[:1, :1], v[:1, :1], mix, pool.at([2]))
    check_untouched("a step of one holder", pool, mid, [2])
    assert not torch.equal(pool.Cur[2], mid.Cur[2]) and pool.lengths[2] == 131 and pool.lengths[1] == 130
    mhla_amd.mhla_causal_step(q[1:2, :1], k[1:2, :1], v[1:2, :1], mix, pool.at([1]))
    assert not torch.equal(pool.Cur[2], pool.Cur[1])
    same_bits("P", pool.P[2], pool.P[1])
    check_untouched("a step of the other", pool, mid, [2, 1])


@both
def test_a_slot_whose_sharer_was_swapped_out_steps_as_if_nothing_had_happened(shape, fmt):
    """62 steps take slot 2 from 130 across the boundary at 192: P is re-mixed from the two pages it shared with slot 4."""
    _, _, q, k, v, _, _, mix = tokens(*shape)
    pool, twin = make(shape, fmt), make(shape, fmt)
    for p in (pool, twin):
        p.fork(4, 2)
    before = snapshot(pool)
    blob = pool.swap_out([4])
    assert blob.n_pages == 2 and pool.table[2] == [7, 5, -1, -1] and pool.refs[7] == pool.refs[5] == 1 and pool.lengths[2] == 130
    check_untouched("swap_out of one holder", pool, before, [4])
    poison(pool, [2], [4])
    rows = []
    for p in (pool, twin):
        view = p.at([2])
        rows.append(torch.cat([mhla_amd.mhla_causal_step(q[:1, t:t + 1], k[:1, t:t + 1], v[:1, t:t + 1], mix, view) for t in range(62)], dim=1))
    same_bits("rows", rows[0], rows[1])
    assert pool.lengths[2] == twin.lengths[2] == 192
    same_state("slot 2", finished(pool.at([2])), finished(twin.at([2])))
    assert float(pool.Cur[2].abs().max()) == 0.0 and float(pool.P[2].abs().max()) > 0.0


# ---- 4: release=False and migration
@both
def test_a_snapshot_migrates_into_a_pool_of_another_geometry(shape, fmt):
    _, _, Hkv, K, V = shape
    pool = make(shape, fmt)
    before = snapshot(pool)
    blob = pool.swap_out(VIEW, device=DEV, release=False)
    assert blob.lengths == LENGTHS and blob.n_pages == 2 and blob.seq_pages == ((), (), (0, 1))
    other = PagedCausalState.empty(7, Hkv, K, V, CAP + 2, 12, DEV, page_format=fmt)
    poison(other, range(12), range(7))
    other.pos.fill_(-7)
    start = snapshot(other)
    other.swap_in(blob, [5, 0, 2])
    assert other.table[5][:2] == [0, -1] and other.table[0][:2] == [1, -1] and other.table[2][:4] == [2, 3, 4, -1]
    same_state("migration", finished(other.at([5, 0, 2])), finished(pool.at(VIEW)))
    check_untouched("migration: the target", other, start, [5, 0, 2], pages=[2, 3])
    check_untouched("migration: the source keeps every bit", pool, before, ())
    assert pool.lengths == before.lengths and pool.table == before.table


# ---- 5: host blob
@both
def test_a_host_blob_holds_the_bytes_of_the_device_blob_whole_or_in_slices(shape, fmt, monkeypatch):
    pool = make(shape, fmt)
    before = snapshot(pool)
    on_device = pool.swap_out(VIEW, device=DEV, release=False)
    whole = pool.swap_out(VIEW, device="cpu", release=False)
    assert whole.host and whole.buffer.is_pinned() and whole.nbytes == on_device.nbytes
    seq_b, page_b = (ops._swap_bytes(*n, shape[2], shape[3], shape[4], fmt) for n in ((1, 0), (0, 1)))
    monkeypatch.setattr(ops, "SWAP_STAGE_CAP_BYTES", seq_b + page_b)   # 5 items: [0, 1), [1, 2), [2, 4), [4, 5)
    sliced = pool.swap_out(VIEW, release=False)
    up, down = sliced.to(DEV), on_device.to("cpu")
    torch.cuda.synchronize()   # (nothing before this line synchronised: the host reads the bytes only now)
    want = on_device.buffer.cpu()
    assert torch.equal(whole.buffer, want), "the host blob of an unsliced swap"
    assert torch.equal(sliced.buffer, want) and sliced.buffer.is_pinned(), "the host blob staged in four slices"
    assert torch.equal(up.buffer, on_device.buffer) and not up.host and torch.equal(down.buffer, want) and down.host and down.buffer.is_pinned()
    check_untouched("three snapshots", pool, before, ())
    # back in from the host blob, sliced the same way, into the slots and pages a release leaves
    pool.reset(VIEW)
    poison(pool, range(N_PAGES), VIEW)
    mid = snapshot(pool)
    pool.swap_in(sliced, [1, 2, 3])
    assert pool.table[1][:2] == [0, -1] and pool.table[2][:2] == [1, -1] and pool.table[3] == [2, 3, 4, -1]
    for slot, src in zip([1, 2, 3], VIEW):
        restored("swap_in from the host", pool, slot, before, src)
    check_untouched("swap_in from the host", pool, mid, [1, 2, 3], pages=[2, 3])


# ---- 6: edges
EDGE_SLOTS, EDGE_LENGTHS = [1, 4, 0, 2], (0, 64, 128, 64 * CAP)
EDGE_TABLE = {1: [], 4: [9], 0: [3, 8], 2: [7, 1, 6, 0]}


def edge_pool(shape, fmt):
    """Random bits in every tensor (a swap moves bits, whatever they mean): an empty slot, one of exactly a chunk, one of two chunks
    with no open token (Cur zero), one at the capacity -- every chunk a page, its `full` flag set."""
    _, _, Hkv, K, V = shape
    g = torch.Generator().manual_seed(77)
    r = lambda *s: torch.randn(s, generator=g).to(DEV)
    rows, lengths = [[-1] * CAP for _ in range(N_SLOTS)], [0] * N_SLOTS
    for s, n in zip(EDGE_SLOTS, EDGE_LENGTHS):
        rows[s][:len(EDGE_TABLE[s])], lengths[s] = EDGE_TABLE[s], n
    kw = dict(page_mult=torch.exp2(torch.randint(-20, 20, (N_PAGES, Hkv, K * V // 64), generator=g).float()).to(DEV)) if fmt == "h16" else {}
    pages = r(N_PAGES, Hkv, K, V)
    pool = PagedCausalState(pages.half() if fmt == "h16" else pages, r(N_SLOTS, Hkv, K, V), r(N_SLOTS, Hkv, K, V), rows, lengths=lengths, **kw)
    pool.Cur[0] = 0
    pool.full[2] = 1
    return pool


@pytest.mark.parametrize("where", ["device", "host"])
@both
def test_edges_round_trip_in_one_call(shape, fmt, where):
    _, _, Hkv, K, V = shape
    pool = edge_pool(shape, fmt)
    before = snapshot(pool)
    blob = pool.swap_out(EDGE_SLOTS, device=DEV if where == "device" else "cpu")
    assert blob.lengths == EDGE_LENGTHS and blob.n_pages == 7 and blob.seq_pages == ((), (0,), (1, 2), (3, 4, 5, 6))
    check_untouched("swap_out", pool, before, EDGE_SLOTS)
    assert pool.pages_used == 0 and pool.lengths == (0,) * N_SLOTS and pool.full.tolist() == [0] * N_SLOTS
    other = PagedCausalState.empty(4, Hkv, K, V, CAP, 8, DEV, page_format=fmt)
    poison(other, range(8), range(4))
    start = snapshot(other)
    other.swap_in(blob, [3, 2, 1, 0])
    assert other.table == [[3, 4, 5, 6], [1, 2, -1, -1], [0, -1, -1, -1], [-1] * CAP] and other.pages_free == 1 and other.lengths == (256, 128, 64, 0)
    for slot, src in zip([3, 2, 1, 0], EDGE_SLOTS):
        restored("edges", other, slot, before, src)
    assert other.full.tolist() == [1, 0, 0, 0] and float(other.Cur[1].abs().max()) == 0.0
    check_untouched("edges", other, start, [0, 1, 2, 3], pages=range(7))
    # and back into the pool they left: the same slots, other pages
    back = other.swap_out([0, 1, 2, 3], device=DEV)
    poison(pool, range(N_PAGES), range(N_SLOTS))
    pool.swap_in(back, [2, 0, 4, 1])
    for s in EDGE_SLOTS:
        restored("edges, back", pool, s, before, s)
    assert pool.full.tolist() == [0, 0, 1, 0, 0] and pool.pages_used == 7


# ---- 7: PoolExhausted
@both
def test_pool_exhausted_changes_nothing_on_the_device(shape, fmt):
    pool = make(shape, fmt)
    blob = pool.swap_out([3, 4], device=DEV, release=False)   # needs 1 + 3 pages
    pool.reserve([0], 193)                                    # pages 0, 1, 3: two of the five free ones are left
    before = snapshot(pool)
    with pytest.raises(PoolExhausted, match=r"need 4 pages, the pool has 2 free"):
        pool.swap_in(blob, [2, 1])
    with pytest.raises(PoolExhausted, match=r"need 4 pages, the pool has 2 free"):
        pool.swap_in(blob.to("cpu"), [2, 1])
    check_untouched("PoolExhausted", pool, before, ())
    assert pool.lengths == before.lengths and pool.table == before.table and pool.pages_free == 2
