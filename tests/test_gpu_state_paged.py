"""What a PAGED state pool (`PagedCausalState`, the library's mhla_causal_*_paged entry points) has beyond the view contract it shares
with a dense pool (test_gpu_state_slots.py: step, extend with counts, verify / commit and pack prefill on both kinds): the setup
itself, an extend without counts, a fork that shares pages, the device-positioned step on a chunk without a page, and walks ten
chunks deep -- every call on a view of a NaN-poisoned pool of 5 slots and 10 pages against the existing un-paged, un-slotted call on
`view.compact()`, BIT FOR BIT (integer views, so the poison compares), with tests/pool_util.py's pool (`make_pool("paged", ...)`: built
through the explicit-table constructor from an un-paged pack prefill by plain tensor copies, with a SCRAMBLED table) and checks
(`check_pool`).  One captured graph of a device-positioned step, with the slot map and the page table rewritten in place between
replays, is held to the fp64 oracle of every request alone (the K split depends on B H: no bit equality there)."""
import pytest
import torch

import mhla_amd
from mhla_amd import CausalState, PagedCausalState
from gpu_util import DEV
from decode_util import check_state, check_step_rows, ragged_inputs
from pool_util import CAP, CASES, IDS, L, LENGTHS, N_PAGES, N_SLOTS, T, VIEW, check_pool, make_pool, same_bits, snapshot, tokens

pytestmark = pytest.mark.gpu


def test_the_compact_state_of_a_view_is_the_prefill():
    """(the setup itself) `compact()` of the scrambled pool gives back the un-paged prefill's finished chunks."""
    shape = CASES[0]
    hk, hv, *_, mix = tokens(*shape)
    n = sum(LENGTHS)
    src = mhla_amd.mhla_causal_state(hk[:, :n], hv[:, :n], mix, cu_seqlens=[0, 63, 68, n], capacity_chunks=CAP)
    pool = make_pool("paged", shape)
    c = pool.at(VIEW).compact()
    assert type(c) is CausalState and c.lengths == LENGTHS and pool.nbytes < 4 * (N_PAGES + 2 * N_SLOTS + 1) * shape[2] * shape[3] * shape[4]
    same_bits("S[2][:2]", c.S[2, :, :2], src.S[2, :, :2])
    same_bits("P", c.P, src.P)
    same_bits("Cur", c.Cur, src.Cur)
    with pytest.raises(TypeError, match=r"\.at\(slots\)"):
        mhla_amd.mhla_causal_step(hk[:, :1].expand(N_SLOTS, -1, -1, -1), hk[:, :1].expand(N_SLOTS, -1, -1, -1),
                                  hv[:, :1].expand(N_SLOTS, -1, -1, -1), mix, pool)


@pytest.mark.parametrize("shape", CASES, ids=IDS)
def test_extend_without_counts_on_a_paged_view(shape):
    """Every slot takes all T = 70 tokens: slot 4 mixes chunks 0 .. 2 through the table for its later segment, nine pages in use."""
    _, _, q, k, v, gate, w, mix = tokens(*shape)
    pool = make_pool("paged", shape)
    view = pool.at(VIEW)
    ref, before = view.compact(), snapshot(pool)
    call = lambda st: mhla_amd.mhla_causal_extend(q, k, v, mix, st, gate=gate, norm_weight=w)
    want = call(ref)
    got = call(view)
    same_bits("rows", got, want)
    after = tuple(p + T for p in LENGTHS)
    assert view.lengths == ref.lengths == after and pool.pages_used == 9 and pool.pages_free == 1
    check_pool("extend", pool, before, ref, VIEW, after)


@pytest.mark.parametrize("shape", CASES[:2], ids=IDS[:2])
def test_a_fork_shares_pages_and_both_go_on_alone(shape):
    _, _, q, k, v, gate, w, mix = tokens(*shape)
    pool = make_pool("paged", shape)
    used = pool.pages_used
    src_before = pool.at([4]).compact()
    pool.fork(4, 2)
    assert pool.table[2] == [7, 5, -1, -1] and pool.refs[7] == pool.refs[5] == 2 and pool.refs[2] == 1, "the two finished chunks, by reference"
    assert pool.pages_used == used and pool.lengths[2] == 130 and int(pool.pos[2]) == 130
    same_bits("P", pool.P[2], pool.P[4])
    same_bits("Cur", pool.Cur[2], pool.Cur[4])
    # dst alone takes 70 tokens across the boundary at 192; src's pages and a later step of src are what they were without the fork
    view = pool.at([2])
    ref, before = view.compact(), snapshot(pool)
    call = lambda st: mhla_amd.mhla_causal_extend(q[:1], k[:1], v[:1], mix, st, gate=gate[:1], norm_weight=w)
    same_bits("rows of dst", call(view), call(ref))
    check_pool("fork, dst extended", pool, before, ref, [2], (200,))
    assert pool.table[2][:2] == [7, 5] and pool.table[2][2] not in (-1, 2) and pool.refs[7] == 2
    now = pool.at([4]).compact()
    for part in ("S", "P", "Cur", "pos"):
        same_bits(f"{part} of src", getattr(now, part), getattr(src_before, part))
    step = lambda st: mhla_amd.mhla_causal_step(q[1:2, :1], k[1:2, :1], v[1:2, :1], mix, st)
    same_bits("rows of src", step(pool.at([4])), step(src_before))
    # the shared pages are freed by the last release only
    pool.reset([4])
    assert pool.refs[7] == pool.refs[5] == 1 and 7 not in pool.free
    pool.reset([2])
    assert pool.refs[7] == pool.refs[5] == 0 and {7, 5} <= set(pool.free) and pool.pages_used == 2


@pytest.mark.parametrize("shape", CASES, ids=IDS)
def test_step_dev_freezes_a_slot_without_a_page_until_it_is_reserved(shape):
    _, _, q, k, v, gate, w, mix = tokens(*shape)
    step = lambda st: mhla_amd.mhla_causal_step_dev(q[:, :1], k[:, :1], v[:, :1], mix, st, gate=gate[:, :1], norm_weight=w)
    # slot 3 is at position 64: chunk 0 finished on page 6, no page for chunk 1
    pool = make_pool("paged", shape, lengths=(64, 5, 129))   # (the pack of `tokens` holds 198 tokens)
    dev_view = pool.at(torch.tensor(VIEW, dtype=torch.int32, device=DEV))
    ref, before = pool.at(VIEW).compact(), snapshot(pool)
    ref.pos[0] = -1   # (the reference freezes that row with the position the step knows)
    want = step(ref)
    got = step(dev_view)
    same_bits("rows", got, want)
    assert float(got[0].float().abs().max()) == 0.0 and pool.stale
    check_pool("step_dev without a page", pool, before, ref, VIEW, (64, 6, 130), touched=[0, 4], flagged=[3])
    assert pool.full.tolist() == [0, 0, 0, 1, 0] and pool.table == before.table, "step_dev assigns no page"
    with pytest.raises(IndexError, match="no page"):
        pool.sync()
    # reserved, the flag cleared: the same call is the live step
    pool.full.zero_()
    pool.sync().reserve([3], 65)
    assert pool.table[3][:2] == [6, 0] and tuple(pool.lengths[s] for s in VIEW) == (64, 6, 130)
    ref, before = pool.at(VIEW).compact(), snapshot(pool)
    want = step(ref)
    got = step(dev_view)
    same_bits("rows", got, want)
    assert float(got[0].float().abs().max()) > 0.0
    check_pool("step_dev after reserve", pool, before, ref, VIEW, (65, 7, 131))
    assert pool.full.tolist() == [0] * N_SLOTS


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_one_graph_serves_a_paged_pool_whose_map_and_table_change(dtype):
    """A captured step_dev on a device map [B = 3] of a paged pool, replayed for 70 tokens: pages are reserved one token ahead
    between replays (the table rewritten in place), request 1 leaves (its row goes to -1) after 25 tokens, request 3 is
    pack-prefilled eagerly into slot 1 and takes that row from token 40.  Every request against its own fp64 oracle."""
    H, K, V, n = 2, 64, 64, 70
    start = (60, 5, 130, 20)                        # requests 0 .. 3; 0 and 2 cross boundaries while replayed
    slot_of, leave, join = (3, 0, 4, 1), 25, 40
    q, k, v, mix, want = ragged_inputs(start, n, H, K, V, L, dtype)
    qd, kd, vd, md = (t.to(DEV) for t in (q, k, v, mix))
    pool = PagedCausalState.empty(N_SLOTS, H, K, V, CAP, N_PAGES, DEV)
    for t in (pool.pages, pool.P, pool.Cur):
        t.fill_(float("nan"))
    pool.full

    def prefill(requests):
        """(eagerly, one pack) the first start[r] tokens of `requests` into their slots"""
        kk, vv = (torch.cat([t[r:r + 1, :start[r]] for r in requests], dim=1) for t in (kd, vd))
        cu = [0]
        for r in requests:
            cu.append(cu[-1] + start[r])
        mhla_amd.mhla_causal_state(kk, vv, md, cu_seqlens=cu, into=pool.at([slot_of[r] for r in requests]))

    prefill([0, 1, 2])
    assert pool.pages_used == 1 + 1 + 3
    slot_map = torch.full((3,), -1, dtype=torch.int32, device=DEV)
    view = pool.at(slot_map)
    sq, sk, sv = (torch.zeros(3, 1, H, d, dtype=dtype, device=DEV) for d in (K, K, V))
    step = lambda: mhla_amd.mhla_causal_step_dev(sq, sk, sv, md, view)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()   # warm-up with every row inactive: code objects loaded, no slot touched
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    torch.cuda.synchronize()
    assert pool.pos.tolist() == [5, 0, 0, 60, 130] and pool.full.tolist() == [0] * N_SLOTS, "neither the warm-up nor the capture moved a slot"
    slot_map.copy_(torch.tensor([3, 0, 4], dtype=torch.int32))
    row_of = {0: 0, 1: 1, 2: 2}     # request -> call row
    taken = {r: 0 for r in range(4)}
    rows = {r: [] for r in range(4)}
    for t in range(n):
        if t == leave:
            slot_map[1] = -1
            del row_of[1]
        if t == join:
            pool.sync()
            prefill([3])
            slot_map[1] = slot_of[3]
            row_of[3] = 1
        for r, b in row_of.items():
            p = start[r] + taken[r]
            pool.reserve([slot_of[r]], p + 1)   # (a new page where the token opens a chunk: the table changes under the graph)
            sq[b], sk[b], sv[b] = qd[r, p:p + 1], kd[r, p:p + 1], vd[r, p:p + 1]
        graph.replay()
        for r, b in row_of.items():
            rows[r].append(out[b:b + 1].clone())
            taken[r] += 1
        if leave <= t < join:
            assert float(out[1].float().abs().max()) == 0.0, f"replay {t}: the inactive row is not zeros"
    pool.sync()
    assert taken == {0: n, 1: leave, 2: n, 3: n - join}
    assert pool.lengths == (start[1] + leave, start[3] + n - join, 0, start[0] + n, start[2] + n)
    assert pool.pages_used == 1 + 1 + 3 + 4 and pool.table_dev.tolist() == pool.table
    for r in range(4):
        got = torch.cat(rows[r], dim=1)
        check_step_rows(f"request {r}", got, want[r][:, :start[r] + taken[r]], start[r], dtype)
        check_state(pool.at([slot_of[r]]).compact(), q[r:r + 1], k[r:r + 1], v[r:r + 1], mix, f"request {r} (slot {slot_of[r]})", b=0,
                    s=start[r] + taken[r])


def test_ten_chunks_deep_the_unrolled_walks_read_through_the_table():
    """Capacity 4 never fills a group of eight: the step's boundary roll, the extend's prefix mixes and the pack prefill's roll fetch
    eight table entries ahead of eight tile loads only from the ninth finished chunk on.  One slot of a capacity-12 pool at
    position 639 (nine finished chunks, the tenth closing), pages descending and interleaved with free ones: the boundary step, an
    extend across the next boundary and a pack prefill of the same length, each against the un-paged call, bit for bit."""
    H, K, V, cap, n_pages, n0 = 2, 16, 24, 12, 16, 639
    g = torch.Generator().manual_seed(99)
    from decode_util import signed_features
    hk, hv = signed_features(g, 1, n0 + 1, H, K).to(DEV), torch.randn(1, n0 + 1, H, V, generator=g).to(DEV)
    q, k, v = signed_features(g, 1, T, H, K).to(DEV), signed_features(g, 1, T, H, K).to(DEV), torch.randn(1, T, H, V, generator=g).to(DEV)
    mix = torch.tril(torch.rand(cap, cap, generator=g).clamp(1e-5, 1)).to(DEV)
    src = mhla_amd.mhla_causal_state(hk[:, :n0], hv[:, :n0], mix, cu_seqlens=[0, n0], capacity_chunks=cap)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)
    row = [13, 11, 9, 7, 5, 3, 1, 0, 2, 4, -1, -1]
    pool = PagedCausalState(nan(n_pages, H, K, V), nan(2, H, K, V), nan(2, H, K, V), [[-1] * cap, row], lengths=[0, n0])
    for j in range(n0 // 64):
        pool.pages[row[j]] = src.S[0, :, j]
    pool.P[1], pool.Cur[1] = src.P[0], src.Cur[0]
    view = pool.at([1])

    def check(name, ref, n, kept=None):
        """(kept: the pages as they were, where released ones are no longer poison: every page the slot does not hold now keeps them)"""
        torch.cuda.synchronize()
        for j in range(n // 64):
            same_bits(f"{name}: chunk {j}", pool.pages[pool.table[1][j]], ref.S[0, :, j])
        same_bits(f"{name}: P", pool.P[1], ref.P[0])
        same_bits(f"{name}: Cur", pool.Cur[1], ref.Cur[0])
        assert int(pool.pos[1]) == int(ref.pos[0]) == n and pool.table_dev.tolist() == pool.table
        for p in pool.free:
            if kept is None:
                assert bool(torch.isnan(pool.pages[p]).all()), f"{name}: free page {p} was written"
            else:
                same_bits(f"{name}: free page {p}", pool.pages[p], kept[p])

    ref = view.compact()
    step = lambda st: mhla_amd.mhla_causal_step(q[:, :1], k[:, :1], v[:, :1], mix, st)
    same_bits("step rows", step(view), step(ref))
    check("step", ref, 640)
    ext = lambda st: mhla_amd.mhla_causal_extend(q, k, v, mix, st)
    same_bits("extend rows", ext(view), ext(ref))
    check("extend", ref, 640 + T)
    assert pool.table[1][10:] == [6, 8] and pool.pages_used == 12
    want = mhla_amd.mhla_causal_state(hk, hv, mix, cu_seqlens=[0, n0 + 1], capacity_chunks=cap)
    kept = pool.pages.clone()
    mhla_amd.mhla_causal_state(hk, hv, mix, cu_seqlens=[0, n0 + 1], into=view)
    check("pack prefill", want, 640, kept)
    assert pool.pages_used == 10 and pool.table[1][10:] == [-1, -1]
