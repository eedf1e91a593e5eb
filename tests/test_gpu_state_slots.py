"""Decode calls on chosen slots of a state pool, DENSE (`CausalState.at`, the library's mhla_causal_*_slots entry points) and PAGED
(`PagedCausalState`, mhla_causal_*_paged: 10 pages through a scrambled table): every call on the non-monotonic view [3, 0, 4] of a
NaN-poisoned pool of 5 slots against the existing un-slotted, un-paged call on `view.compact()`, BIT FOR BIT (integer views, so the
poison compares): the rows, the finished chunks (of S, or read back through the page table), P, Cur and pos of the three slots, every
bit of the slots the call does not name, and every bit of every page the call must not write -- the free ones, other slots', and the
view's own finished chunks.  The pools, their inputs and the checks are tests/pool_util.py's (`make_pool`, `tokens`, `check_pool`):
filled from an un-slotted pack prefill by plain tensor copies, so that no setup depends on what is tested.  The view contract is
written once for both kinds, what a paged pool adds to it (its page accounting) under `kind == "paged"`; the dense pool's own tests
follow, the paged pool's own are in test_gpu_state_paged.py.  One captured graph of a device-positioned step on a device map,
rewritten in place while the graph is replayed, is held to the fp64 oracle of every request alone (the K split depends on B H: no
bit equality with a batch of one there)."""
import itertools

import pytest
import torch

import mhla_amd
from mhla_amd import CausalState
from gpu_util import DEV
from decode_util import check_state, check_step_rows, ragged_inputs
from pool_util import (ACCEPT, CAP, CASES, COUNTS, IDS, L, LENGTHS, N_SLOTS, VIEW, check_pool, make_pool, same_bits, snapshot, tokens,
                       windows)

pytestmark = pytest.mark.gpu

SHAPES = (CASES, IDS)


def both_kinds(names, *axes):
    """Parametrise a test over `names` and `kind`: the product of the axes [(values, ids), ...] on a dense pool, under the ids these cases
    have always had, and on a paged pool, under the same ids with `-paged`."""
    combos = list(itertools.product(*(list(zip(*axis)) for axis in axes)))
    return pytest.mark.parametrize(names + ", kind", [pytest.param(*(v for v, _ in c), kind, id="-".join(i for _, i in c) + tail)
                                                      for kind, tail in (("dense", ""), ("paged", "-paged")) for c in combos])


# ---- the view contract, on a dense and on a paged pool
@both_kinds("shape, epilogue", SHAPES, ([False, True], ["plain", "gate-norm"]))
def test_step_on_a_view_is_the_step_on_the_compact_state(shape, epilogue, kind):
    _, _, q, k, v, gate, w, mix = tokens(*shape)
    kw = dict(gate=gate[:, :1], norm_weight=w) if epilogue else {}
    pool = make_pool(kind, shape)
    view = pool.at(VIEW)
    assert view.lengths == LENGTHS
    ref, before = view.compact(), snapshot(pool)
    want = mhla_amd.mhla_causal_step(q[:, :1], k[:, :1], v[:, :1], mix, ref, **kw)
    got = mhla_amd.mhla_causal_step(q[:, :1], k[:, :1], v[:, :1], mix, view, **kw)
    same_bits("rows", got, want)
    after = tuple(n + 1 for n in LENGTHS)
    assert view.lengths == ref.lengths == after and tuple(pool.lengths[s] for s in VIEW) == after and pool.lengths[1] == pool.lengths[2] == 0
    if kind == "paged":
        assert pool.table == before.table, "every chunk the step touches had its page"
    check_pool("step", pool, before, ref, VIEW, after)


@both_kinds("shape, left", SHAPES, ([False, True], ["right-padded", "left-padded"]))
def test_extend_with_counts_on_a_view(shape, left, kind):
    _, _, q, k, v, gate, w, mix = tokens(*shape)
    q, k, v, gate = (windows(t, COUNTS, left) for t in (q, k, v, gate))
    pool = make_pool(kind, shape)
    view = pool.at(VIEW)
    ref, before = view.compact(), snapshot(pool)
    call = lambda st: mhla_amd.mhla_causal_extend(q, k, v, mix, st, counts=COUNTS, left_padded=left, gate=gate, norm_weight=w)
    want = call(ref)
    got = call(view)
    same_bits("rows", got, want)
    after = tuple(p + n for p, n in zip(LENGTHS, COUNTS))
    assert view.lengths == ref.lengths == after
    if kind == "paged":
        assert pool.table[0][:2] == [4, 0] and pool.pages_used == 6, "slot 0 grew into chunk 1: the lowest free page"
    check_pool("extend", pool, before, ref, VIEW, after)


@both_kinds("shape", SHAPES)
def test_verify_then_commit_on_a_view(shape, kind):
    _, _, q, k, v, gate, w, mix = tokens(*shape)
    q, k, v, gate = (windows(t, COUNTS, False) for t in (q, k, v, gate))
    pool = make_pool(kind, shape)
    view = pool.at(VIEW)
    ref, before = view.compact(), snapshot(pool)
    want, draft_ref = mhla_amd.mhla_causal_verify(q, k, v, mix, ref, counts=COUNTS, gate=gate, norm_weight=w)
    got, draft = mhla_amd.mhla_causal_verify(q, k, v, mix, view, counts=COUNTS, gate=gate, norm_weight=w)
    same_bits("rows", got, want)
    assert draft.view is view and view.lengths == LENGTHS
    ends = tuple(p + n for p, n in zip(LENGTHS, COUNTS))
    # (only the finished chunks -- rows of S -- are specified after a verify: the header; on a paged pool the draft's pages are assigned,
    # and `reach` names them; a dense pool has no pages and `reach` is not looked at)
    if kind == "paged":
        assert pool.pages_used == 6
    check_pool("verify", pool, before, ref, VIEW, LENGTHS, reach=ends)
    mhla_amd.mhla_causal_commit(draft_ref, mix, ref, ACCEPT)
    assert mhla_amd.mhla_causal_commit(draft, mix, view, ACCEPT) is view
    after = tuple(p + a for p, a in zip(LENGTHS, ACCEPT))
    assert view.lengths == ref.lengths == after
    check_pool("commit", pool, before, ref, VIEW, after, reach=ends)
    if kind == "paged":
        # slot 0 was verified to 75 tokens and accepted 38: the page of chunk 1 goes back
        page = pool.table[0][1]
        pool.trim(VIEW)
        assert pool.table[0] == [4, -1, -1, -1] and pool.pages_used == 5 and page in pool.free and pool.table_dev.tolist() == pool.table


@both_kinds("shape, lengths", SHAPES, ([(130, 0), (64, 70)], ["130+0", "64+70"]))
def test_pack_prefill_into_slots(shape, lengths, kind):
    hk, hv, *_, mix = tokens(*shape)
    n, slots = sum(lengths), [4, 1]
    cu = [0, lengths[0], n]
    # (the pack: other tokens than those slot 4 was filled from)
    k, v = hk[:, 10:10 + n], hv[:, 10:10 + n]
    pool = make_pool(kind, shape)
    before = snapshot(pool)
    ref = mhla_amd.mhla_causal_state(k, v, mix, cu_seqlens=cu, capacity_chunks=CAP)
    view = pool.at(slots)
    assert mhla_amd.mhla_causal_state(k, v, mix, cu_seqlens=cu, into=view) is view
    assert view.lengths == ref.lengths == lengths and pool.lengths == (5, lengths[1], 0, 63, lengths[0])
    if kind == "paged":
        assert pool.pages_used == 2 + sum(-(-m // 64) for m in lengths), "slot 4 starts anew: its three pages went back first"
    # (a prefill starts the slot anew: every chunk up to its length may be written)
    start = before._replace(lengths=tuple(0 if s in slots else m for s, m in enumerate(before.lengths)))
    check_pool("pack prefill", pool, start, ref, slots, lengths)
    assert pool.full.tolist() == [0] * N_SLOTS


# ---- the dense pool's own
@pytest.mark.parametrize("shape", CASES, ids=IDS)
def test_step_dev_with_an_inactive_row_and_a_slot_at_capacity(shape):
    _, _, q, k, v, gate, w, mix = tokens(*shape)
    step = lambda st: mhla_amd.mhla_causal_step_dev(q[:, :1], k[:, :1], v[:, :1], mix, st, gate=gate[:, :1], norm_weight=w)
    # ---- map [3, -1, 4]: row 1 is zeros and touches no slot; the reference freezes that row with the position the step knows
    pool = make_pool("dense", shape)
    ref, before = pool.at(VIEW).compact(), snapshot(pool)
    ref.pos[1] = -1
    want = step(ref)
    got = step(pool.at(torch.tensor([3, -1, 4], dtype=torch.int32, device=DEV)))
    same_bits("rows", got, want)
    assert float(got[1].float().abs().max()) == 0.0
    assert pool.stale
    check_pool("step_dev", pool, before, ref, VIEW, (64, 5, 131), touched=[3, 4])
    assert pool.full.tolist() == [0] * N_SLOTS, "no flag: slot 0 was not named, the named slots are live"
    # ---- slot 3 at the capacity: full[3] = 1, the row zeros, the slot untouched
    pool = make_pool("dense", shape)
    pool.pos[3] = 64 * CAP
    ref, before = pool.at(VIEW).compact(), snapshot(pool)
    want = step(ref)
    got = step(pool.at(torch.tensor(VIEW, dtype=torch.int32, device=DEV)))
    same_bits("rows", got, want)
    assert float(got[0].float().abs().max()) == 0.0
    check_pool("step_dev at capacity", pool, before, ref, VIEW, (64 * CAP, 6, 131), touched=[0, 4], flagged=[3])
    assert pool.full.tolist() == [0, 0, 0, 1, 0] and ref.full.tolist() == [1, 0, 0]


@pytest.mark.parametrize("shape", CASES[:2], ids=IDS[:2])
def test_a_forked_slot_steps_like_its_source(shape):
    _, _, q, k, v, _, _, mix = tokens(*shape)
    pool = make_pool("dense", shape)
    pool.fork(3, 2)
    assert pool.lengths[2] == 63 and int(pool.pos[2]) == 63
    a = mhla_amd.mhla_causal_step(q[:1, :1], k[:1, :1], v[:1, :1], mix, pool.at([3]))
    b = mhla_amd.mhla_causal_step(q[:1, :1], k[:1, :1], v[:1, :1], mix, pool.at([2]))
    same_bits("rows", a, b)
    assert pool.lengths[2] == pool.lengths[3] == 64 and pool.pos[[2, 3]].tolist() == [64, 64]
    same_bits("S", pool.S[2, :, :1], pool.S[3, :, :1])
    same_bits("P", pool.P[2], pool.P[3])
    same_bits("Cur", pool.Cur[2], pool.Cur[3])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_one_graph_serves_requests_that_leave_and_join(dtype):
    """A captured step_dev on a device map [B = 3], replayed for 70 tokens: request 1 leaves (its row goes to -1) after 25 tokens,
    request 3 is pack-prefilled eagerly into slot 1 and takes that row from token 40.  Every request against its own fp64 oracle."""
    H, K, V, n = 2, 64, 64, 70
    start = (60, 5, 130, 20)                        # requests 0 .. 3; 0 and 2 cross boundaries while replayed
    slot_of, leave, join = (3, 0, 4, 1), 25, 40
    q, k, v, mix, want = ragged_inputs(start, n, H, K, V, L, dtype)
    qd, kd, vd, md = (t.to(DEV) for t in (q, k, v, mix))
    e = CausalState.empty(N_SLOTS, H, K, V, CAP, DEV)
    for t in (e.S, e.P, e.Cur):
        t.fill_(float("nan"))
    pool = e.to_ragged()
    pool.full

    def prefill(requests):
        """(eagerly, one pack) the first start[r] tokens of `requests` into their slots"""
        kk, vv = (torch.cat([t[r:r + 1, :start[r]] for r in requests], dim=1) for t in (kd, vd))
        cu = [0]
        for r in requests:
            cu.append(cu[-1] + start[r])
        mhla_amd.mhla_causal_state(kk, vv, md, cu_seqlens=cu, into=pool.at([slot_of[r] for r in requests]))

    prefill([0, 1, 2])
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
    # q, k, v by slot, as `check_state` pairs them with the state's rows (slot 2 holds no request)
    by_slot = [1, 3, 0, 0, 2]
    qs, ks, vs = (t[by_slot] for t in (q, k, v))
    for r in range(4):
        got = torch.cat(rows[r], dim=1)
        check_step_rows(f"request {r}", got, want[r][:, :start[r] + taken[r]], start[r], dtype)
        check_state(pool, qs, ks, vs, mix, f"request {r} (slot {slot_of[r]})", b=slot_of[r], s=start[r] + taken[r])
