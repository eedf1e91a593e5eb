"""Decode calls on a paged state pool of h16 pages (`PagedCausalState.empty(..., page_format="h16")`, the library's
mhla_causal_*_paged_h16 entry points), held to the format's contract: a page is the ENCODING of the fp32 pool's page, bit for bit
(integer views against the torch codec of tests/pool_util.py, which tests/test_state_paged_h16_cpu.py checks); P is the ascending fmaf
sum over DECODED pages, the chunk a boundary just committed included (the derived bound of an n-term fp32 fmaf chain, which a sum that
adds the un-rounded chunk misses by orders of magnitude); a prefilled slot holds the bits of a stepped one; rows stay within the bound
the 11-bit forward is held to, per chunk, against the fp64 operator on every request alone; and nothing a call does not name changes
a bit -- payload, multipliers, slots, flags (`pool_util.check_untouched`).  Shapes, tokens, VIEW = [3, 0, 4], LENGTHS = (63, 5, 130),
the NaN poison and the scrambled table are the pool family's (`pool_util.make_pool("paged" / "h16", ...)`); what the rows' inputs may
cost on their own is capped on the CPU (test_state_paged_h16_cpu.py: test_input_check_h16_pages_alone_stay_within_the_row_bound)."""
import functools

import pytest
import torch

import mhla_amd
from mhla_amd import PagedCausalState
from gpu_util import CAUSAL_TOL, DEV, check, check_chunks
from decode_util import ragged_inputs, signed_features
from pool_util import (CAP, CASES, GROUP, IDS, L, LENGTHS, N_PAGES, N_SLOTS, NAN, ROW_EXTRA, TABLE, VIEW, check_untouched, decode, encode,
                       gate_norm, make_pool, rows_fp64, same_bits, sequence, snapshot, tokens)

pytestmark = pytest.mark.gpu

# rows: the bound the 11-bit forward is held to (u + 1e-3: gpu_util.CAUSAL_TOL); fp32 tensors: the same rule, no final rounding
ROW_TOL = {torch.float32: ROW_EXTRA, torch.bfloat16: CAUSAL_TOL[torch.bfloat16], torch.float16: CAUSAL_TOL[torch.float16]}


def empty_h16(H, K, V, n_slots=N_SLOTS, cap=CAP, n_pages=N_PAGES):
    """An h16 pool without a token whose every byte of state is poison."""
    pool = PagedCausalState.empty(n_slots, H, K, V, cap, n_pages, DEV, page_format="h16")
    for t in (pool.pages, pool.page_mult, pool.P, pool.Cur):
        t.fill_(NAN)
    pool.full
    return pool


def page_is_encoded(name, pool, page, chunk):
    """Payload and multipliers of `page` are the encoding of the fp32 chunk [Hkv, K, V], compared as integers."""
    pay, mult = encode(chunk.contiguous())
    same_bits(f"{name}: payload of page {page}", pool.pages[page], pay)
    same_bits(f"{name}: multipliers of page {page}", pool.page_mult[page], mult)


def decoded(pool, page):
    return decode(pool.pages[page], pool.page_mult[page]).double()


def p_is_the_sum_over_decoded_pages(name, pool, slot, mix, n):
    """P of `slot`, whose n finished chunks the table names, against the fp64 sum of mix[n][j] decode(page_j): every element within the
    bound of an n-term fp32 fmaf chain, n 2^-23 sum_j |mix[n][j]| |decode(page_j)|."""
    terms = [mix[n, j].double() * decoded(pool, pool.table[slot][j]) for j in range(n)]
    want, mag = sum(terms), sum(t.abs() for t in terms)
    err = (pool.P[slot].double() - want).abs()
    over = err > n * 2.0 ** -23 * mag
    worst = float((err / mag.clamp_min(1e-300)).max())
    print(f"{name}: P of slot {slot} over {n} decoded pages: worst |err| / sum|terms| = {worst:.2e} (bound {n * 2.0 ** -23:.2e})")
    assert not bool(over.any()), f"{name}: P of slot {slot} is not the sum over its {n} decoded pages: {int(over.sum())} elements beyond the bound, worst {worst:.2e}"


def check_rows(name, got, want, m, dtype):
    """decode_util.check_step_rows at ROW_TOL: rows m .. of one request within the bound of its maximum, and chunk by chunk of its own chunks."""
    tol, ref = ROW_TOL[dtype], want[:, m:]
    e = check(name, got, ref, tol)
    first = min(got.shape[1], 64 - m % 64)
    e = max(e, check_chunks(f"{name} (open chunk)", got[:, :first], ref[:, :first], tol))
    if first < got.shape[1]:
        e = max(e, check_chunks(name, got[:, first:], ref[:, first:], tol))
    return e


# ---- 1, 2: pages are the encoded fp32 pages; P is the sum over decoded pages
@pytest.mark.parametrize("shape", CASES, ids=IDS)
def test_a_boundary_step_writes_the_encoded_page_and_mixes_decoded_pages(shape):
    _, _, q, k, v, _, _, mix = tokens(*shape)
    src, pool = make_pool("paged", shape), make_pool("h16", shape)
    step = lambda view: mhla_amd.mhla_causal_step(q[:, :1], k[:, :1], v[:, :1], mix, view)
    step(src.at(VIEW))
    step(pool.at(VIEW))   # slot 3 crosses the boundary at 63 -> 64: chunk 0 goes to page 6
    torch.cuda.synchronize()
    assert pool.table == src.table and pool.lengths == src.lengths == (6, 0, 0, 64, 131) and TABLE[3] == [6]
    page_is_encoded("boundary step", pool, 6, src.pages[6])
    for s in VIEW:
        same_bits(f"Cur of slot {s}", pool.Cur[s], src.Cur[s])
        assert int(pool.pos[s]) == int(src.pos[s])
    assert float(pool.Cur[3].abs().max()) == 0.0
    p_is_the_sum_over_decoded_pages("boundary step", pool, 3, mix, 1)
    # the fp32 chunk itself is NOT what was added: it differs from the decoded page at the 12th bit
    assert float((src.pages[6] - decode(pool.pages[6], pool.page_mult[6])).abs().max()) > 0.0


@pytest.mark.parametrize("lengths", [(130, 0), (64, 70)], ids=["130+0", "64+70"])
@pytest.mark.parametrize("shape", CASES, ids=IDS)
def test_a_pack_prefill_writes_the_encoded_pages(shape, lengths):
    hk, hv, *_, mix = tokens(*shape)
    n, slots = sum(lengths), [4, 1]
    cu = [0, lengths[0], n]
    kk, vv = hk[:, 10:10 + n], hv[:, 10:10 + n]
    src, pool = make_pool("paged", shape), make_pool("h16", shape)
    before = snapshot(pool)
    mhla_amd.mhla_causal_state(kk, vv, mix, cu_seqlens=cu, into=src.at(slots))
    view = pool.at(slots)
    assert mhla_amd.mhla_causal_state(kk, vv, mix, cu_seqlens=cu, into=view) is view
    torch.cuda.synchronize()
    assert pool.table == src.table and pool.lengths == src.lengths and view.lengths == lengths
    for s, m in zip(slots, lengths):
        for j in range(m // 64):
            page_is_encoded(f"prefill, chunk {j} of slot {s}", pool, pool.table[s][j], src.pages[src.table[s][j]])
        same_bits(f"Cur of slot {s}", pool.Cur[s], src.Cur[s])
        assert int(pool.pos[s]) == m
        if m // 64:
            p_is_the_sum_over_decoded_pages("prefill", pool, s, mix, m // 64)
        else:
            assert float(pool.P[s].abs().max()) == 0.0
    # (a prefill starts the slot anew: every chunk up to its length may be written)
    start = before._replace(lengths=tuple(0 if s in slots else m for s, m in enumerate(before.lengths)))
    check_untouched("pack prefill", pool, start, slots, lengths)
    assert pool.full.tolist() == [0] * N_SLOTS


@pytest.mark.parametrize("shape", [CASES[1], CASES[4]], ids=[IDS[1], IDS[4]])
def test_a_pack_prefill_in_slices_of_the_chunk_list_holds_the_bits_of_one_pass(shape, monkeypatch):
    """A workspace that holds ONE chunk: the library stages and encodes the pack's five chunks one at a time (the roll once at the
    end) and leaves the bits of the prefill whose workspace took them all."""
    from mhla_amd import ops
    dtype, H, Hkv, K, V = shape
    hk, hv, *_, mix = tokens(*shape)
    n = sum(LENGTHS)
    pools = []
    for cap_bytes in (ops.EXTEND_WS_CAP_BYTES, 16):
        monkeypatch.setattr(ops, "EXTEND_WS_CAP_BYTES", cap_bytes)
        pool = empty_h16(Hkv, K, V)
        mhla_amd.mhla_causal_state(hk[:, :n], hv[:, :n], mix, cu_seqlens=[0, 63, 68, n], into=pool.at(VIEW))
        pools.append(pool)
    torch.cuda.synchronize()
    one, sliced = pools
    assert one.table == sliced.table and one.lengths == sliced.lengths and one.pages_used == 5
    for part in ("pages", "page_mult", "P", "Cur", "pos"):
        same_bits(part, getattr(sliced, part), getattr(one, part))
    assert bool(torch.isfinite(one.P[VIEW]).all()) and bool(torch.isfinite(one.Cur[VIEW]).all()) and float(one.Cur[4].abs().max()) > 0.0


# ---- 3: prefilled equals stepped
@pytest.mark.parametrize("shape", CASES, ids=IDS)
def test_a_prefilled_slot_holds_the_bits_of_a_stepped_one(shape):
    dtype, H, Hkv, K, V = shape
    hk, hv, q, *_, mix = tokens(*shape)
    pool = empty_h16(Hkv, K, V)
    mhla_amd.mhla_causal_state(hk[:, :130], hv[:, :130], mix, cu_seqlens=[0, 130], into=pool.at([4]))
    mhla_amd.mhla_causal_state(hk[:, :5], hv[:, :5], mix, cu_seqlens=[0, 5], into=pool.at([1]))
    view = pool.at([1])
    for t in range(5, 130):
        mhla_amd.mhla_causal_step(q[:1, :1], hk[:, t:t + 1], hv[:, t:t + 1], mix, view)
    torch.cuda.synchronize()
    assert pool.lengths[1] == pool.lengths[4] == 130 and int(pool.pos[1]) == int(pool.pos[4]) == 130
    for j in range(2):
        a, b = pool.table[4][j], pool.table[1][j]
        assert a != b and min(a, b) >= 0
        same_bits(f"payload of chunk {j}", pool.pages[a], pool.pages[b])
        same_bits(f"multipliers of chunk {j}", pool.page_mult[a], pool.page_mult[b])
    same_bits("P", pool.P[4], pool.P[1])
    same_bits("Cur", pool.Cur[4], pool.Cur[1])


# ---- 4: rows against the fp64 operator on every request alone
@functools.lru_cache(maxsize=None)
def row_reference(shape):
    """Per request (the exact fp64 rows [1, m + 70, H, V], the same through the gate x norm epilogue), once per shape."""
    out = []
    for b in range(3):
        q, k, v, gate, w, mix, m = sequence(shape, b)
        o = rows_fp64(q, k, v, mix)
        y = torch.cat([o[:, :m], gate_norm(o[:, m:], gate, w)], dim=1)
        out.append((o, y))
    return out


@pytest.mark.parametrize("epilogue", [False, True], ids=["plain", "gate-norm"])
@pytest.mark.parametrize("shape", CASES, ids=IDS)
def test_seventy_steps_on_h16_pages_against_the_fp64_operator(shape, epilogue):
    """Observed (worst of rel_err over the tensor and per chunk, over the three requests; plain / gate-norm): see
    profiles/causal_state_h16.md."""
    dtype, H, Hkv, K, V = shape
    hk, hv, q, k, v, gate, w, mix = tokens(*shape)
    pool = empty_h16(Hkv, K, V)
    view = pool.at(VIEW)
    n = sum(LENGTHS)
    mhla_amd.mhla_causal_state(hk[:, :n], hv[:, :n], mix, cu_seqlens=[0, 63, 68, n], into=view)
    rows = []
    for t in range(70):
        kw = dict(gate=gate[:, t:t + 1], norm_weight=w) if epilogue else {}
        rows.append(mhla_amd.mhla_causal_step(q[:, t:t + 1], k[:, t:t + 1], v[:, t:t + 1], mix, view, **kw))
    got = torch.cat(rows, dim=1)
    assert view.lengths == tuple(m + 70 for m in LENGTHS) and pool.pos.tolist()[3] == 133 and pool.full.tolist() == [0] * N_SLOTS
    worst = 0.0
    for b, m in enumerate(LENGTHS):
        worst = max(worst, check_rows(f"request {b}", got[b:b + 1], row_reference(shape)[b][int(epilogue)], m, dtype))
    print(f"rows {IDS[CASES.index(shape)]} {'gate-norm' if epilogue else 'plain'}: worst rel_err {worst:.2e} (bound {ROW_TOL[dtype]:.2e})")


# ---- 5: isolation
@pytest.mark.parametrize("call", ["step", "step_dev"])
@pytest.mark.parametrize("shape", CASES, ids=IDS)
def test_a_step_changes_nothing_it_does_not_name(shape, call):
    _, _, q, k, v, gate, w, mix = tokens(*shape)
    pool = make_pool("h16", shape)
    before = snapshot(pool)
    if call == "step":
        mhla_amd.mhla_causal_step(q[:, :1], k[:, :1], v[:, :1], mix, pool.at(VIEW), gate=gate[:, :1], norm_weight=w)
    else:
        mhla_amd.mhla_causal_step_dev(q[:, :1], k[:, :1], v[:, :1], mix, pool.at(torch.tensor(VIEW, dtype=torch.int32, device=DEV)),
                                      gate=gate[:, :1], norm_weight=w)
        assert pool.stale
    after = tuple(m + 1 for m in LENGTHS)
    # (ahead of the sync, which reads pos back into the host lengths of EVERY slot, the unnamed ones' poison too)
    check_untouched(call, pool, before, VIEW, after)
    pool.sync()
    assert tuple(pool.lengths[s] for s in VIEW) == after and pool.table == before.table
    assert pool.full.tolist() == [0] * N_SLOTS


# ---- 6: the device-positioned step
@pytest.mark.parametrize("shape", CASES, ids=IDS)
def test_step_dev_freezes_a_slot_without_a_page_until_it_is_reserved(shape):
    _, _, q, k, v, gate, w, mix = tokens(*shape)
    step = lambda st: mhla_amd.mhla_causal_step_dev(q[:, :1], k[:, :1], v[:, :1], mix, st, gate=gate[:, :1], norm_weight=w)
    # slot 3 is at position 64: chunk 0 finished on page 6, no page for chunk 1
    pool = make_pool("h16", shape, lengths=(64, 5, 129))
    dev_view = pool.at(torch.tensor(VIEW, dtype=torch.int32, device=DEV))
    # (off a boundary a step reads P and Cur alone: its rows are, bit for bit, those of the step on the decoded compact state)
    ref, before = pool.at(VIEW).compact(), snapshot(pool)
    ref.pos[0] = -1
    want = step(ref)
    got = step(dev_view)
    same_bits("rows", got, want)
    assert float(got[0].float().abs().max()) == 0.0 and pool.stale
    check_untouched("step_dev without a page", pool, before, [0, 4], (6, 130), flagged=[3])
    assert pool.full.tolist() == [0, 0, 0, 1, 0] and pool.table == before.table, "step_dev assigns no page"
    assert pool.pos.tolist()[0] == 6 and pool.pos.tolist()[3:] == [64, 130]
    with pytest.raises(IndexError, match="no page"):
        pool.sync()
    pool.full.zero_()
    pool.sync().reserve([3], 65)
    assert pool.table[3][:2] == [6, 0]
    ref, before = pool.at(VIEW).compact(), snapshot(pool)
    want = step(ref)
    got = step(dev_view)
    same_bits("rows", got, want)
    assert float(got[0].float().abs().max()) > 0.0
    pool.sync()
    check_untouched("step_dev after reserve", pool, before, VIEW, (65, 7, 131))
    assert tuple(pool.lengths[s] for s in VIEW) == (65, 7, 131) and pool.full.tolist() == [0] * N_SLOTS


def test_one_graph_serves_an_h16_pool_whose_map_and_table_change():
    """The scenario of test_gpu_state_paged.test_one_graph_serves_a_paged_pool_whose_map_and_table_change on h16 pages, bf16: a
    captured step_dev on a device map [B = 3], replayed for 70 tokens; pages reserved one token ahead between replays (the table
    rewritten in place), request 1 leaves after 25 tokens, request 3 is pack-prefilled eagerly into slot 1 and takes that row from
    token 40.  Every request against its own fp64 oracle at ROW_TOL."""
    dtype, H, K, V, n = torch.bfloat16, 2, 64, 64, 70
    start = (60, 5, 130, 20)
    slot_of, leave, join = (3, 0, 4, 1), 25, 40
    q, k, v, mix, want = ragged_inputs(start, n, H, K, V, L, dtype)
    qd, kd, vd, md = (t.to(DEV) for t in (q, k, v, mix))
    pool = empty_h16(H, K, V)

    def prefill(requests):
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
        step()   # warm-up with every row inactive
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    torch.cuda.synchronize()
    assert pool.pos.tolist() == [5, 0, 0, 60, 130] and pool.full.tolist() == [0] * N_SLOTS
    slot_map.copy_(torch.tensor([3, 0, 4], dtype=torch.int32))
    row_of = {0: 0, 1: 1, 2: 2}
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
            pool.reserve([slot_of[r]], p + 1)
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
        check_rows(f"request {r}", torch.cat(rows[r], dim=1), want[r][:, :start[r] + taken[r]], start[r], dtype)
        s = slot_of[r]
        for j in range(pool.lengths[s] // 64):   # (every finished chunk's multipliers are powers of two: a page was really encoded)
            m = pool.page_mult[pool.table[s][j]].view(torch.int32)
            assert bool(((m & 0x807FFFFF) == 0).all())


# ---- 7: ten chunks deep
def test_ten_chunks_deep_the_unrolled_walk_reads_decoded_pages_through_the_table():
    """One slot of a capacity-12 pool at position 639 (nine finished chunks, the tenth closing), pages descending and interleaved with
    free ones: the boundary roll and the pack prefill's roll fetch eight table entries ahead of eight payload pieces and multipliers,
    then the tail -- P against the fp64 sum over the ten decoded pages, the pages against the encoded fp32 chunks."""
    H, K, V, cap, n_pages, n0 = 2, 16, 24, 12, 16, 639
    g = torch.Generator().manual_seed(99)
    hk, hv = signed_features(g, 1, n0 + 1, H, K).to(DEV), torch.randn(1, n0 + 1, H, V, generator=g).to(DEV)
    q = signed_features(g, 1, 1, H, K).to(DEV)
    mix = torch.tril(torch.rand(cap, cap, generator=g).clamp(1e-5, 1)).to(DEV)
    src = mhla_amd.mhla_causal_state(hk, hv, mix, cu_seqlens=[0, n0 + 1], capacity_chunks=cap)   # (fp32, un-paged: all ten chunks)
    row = [13, 11, 9, 7, 5, 3, 1, 0, 2, 4, -1, -1]
    nan = lambda *s: torch.full(s, NAN, dtype=torch.float32, device=DEV)
    pool = PagedCausalState(nan(n_pages, H, K, V).half(), nan(2, H, K, V), nan(2, H, K, V), [[-1] * cap, row], lengths=[0, n0],
                            page_mult=nan(n_pages, H, K * V // GROUP))
    at639 = mhla_amd.mhla_causal_state(hk[:, :n0], hv[:, :n0], mix, cu_seqlens=[0, n0], capacity_chunks=cap)
    for j in range(9):
        pool.pages[row[j]], pool.page_mult[row[j]] = encode(src.S[0, :, j].contiguous())
    pool.P[1], pool.Cur[1] = at639.P[0], at639.Cur[0]
    view = pool.at([1])

    def check(name, chunks):
        torch.cuda.synchronize()
        assert pool.lengths[1] == int(pool.pos[1]) == 640 and pool.table_dev.tolist() == pool.table
        for j in range(10):
            page_is_encoded(f"{name}, chunk {j}", pool, pool.table[1][j], chunks[0, :, j])
        p_is_the_sum_over_decoded_pages(name, pool, 1, mix, 10)
        assert float(pool.Cur[1].abs().max()) == 0.0
        for p in pool.free:
            assert bool(torch.isnan(pool.pages[p].float()).all()) and bool(torch.isnan(pool.page_mult[p]).all()), f"{name}: free page {p} was written"

    mhla_amd.mhla_causal_step(q, hk[:, n0:], hv[:, n0:], mix, view)
    mhla_amd.mhla_causal_step(q, hk[:, n0:], hv[:, n0:], mix, at639)   # (the fp32 chunk the same step finishes: 639 prefilled tokens and one)
    check("step", torch.cat([src.S[:, :, :9], at639.S[:, :, 9:10]], dim=2))
    assert pool.table[1][:10] == row[:10]
    # the same 640 tokens as one pack prefill into the slot: the pages go back first, then the ten lowest
    for t in (pool.pages, pool.page_mult):
        t.fill_(NAN)
    mhla_amd.mhla_causal_state(hk, hv, mix, cu_seqlens=[0, n0 + 1], into=view)
    assert pool.table[1][:10] == list(range(10)) and pool.pages_used == 10
    check("pack prefill", src.S)


# ---- 8: fork
@pytest.mark.parametrize("shape", CASES[:2], ids=IDS[:2])
def test_a_fork_shares_pages_and_both_hold_equal_bits_until_their_tokens_differ(shape):
    _, _, q, k, v, gate, w, mix = tokens(*shape)
    pool = make_pool("h16", shape)
    used, pages, mult = pool.pages_used, pool.pages.clone(), pool.page_mult.clone()
    pool.fork(4, 2)
    assert pool.table[2] == [7, 5, -1, -1] and pool.refs[7] == pool.refs[5] == 2 and pool.refs[2] == 1, "the two finished chunks, by reference"
    assert pool.pages_used == used and pool.lengths[2] == 130 and int(pool.pos[2]) == 130
    same_bits("payload: no page was copied or written", pool.pages, pages)
    same_bits("multipliers", pool.page_mult, mult)
    same_bits("P", pool.P[2], pool.P[4])
    same_bits("Cur", pool.Cur[2], pool.Cur[4])
    # each alone, the same 63 tokens: across the boundary at 192, into pages of their own
    for s in (4, 2):
        view = pool.at([s])
        rows = [mhla_amd.mhla_causal_step(q[:1, t:t + 1], k[:1, t:t + 1], v[:1, t:t + 1], mix, view) for t in range(63)]
        if s == 4:
            first = torch.cat(rows, dim=1)
    same_bits("rows", torch.cat(rows, dim=1), first)
    torch.cuda.synchronize()
    assert pool.lengths[4] == pool.lengths[2] == 193 and pool.table[4][:2] == pool.table[2][:2] == [7, 5] and pool.refs[7] == 2
    a, b = pool.table[4][2], pool.table[2][2]
    assert a == 2 and b not in (-1, 2) and pool.refs[a] == pool.refs[b] == 1
    same_bits("payload of chunk 2", pool.pages[a], pool.pages[b])
    same_bits("multipliers of chunk 2", pool.page_mult[a], pool.page_mult[b])
    same_bits("P", pool.P[2], pool.P[4])
    same_bits("Cur", pool.Cur[2], pool.Cur[4])
    same_bits("the shared pages", pool.pages[[7, 5]], pages[[7, 5]])
    # another token each: they part
    mhla_amd.mhla_causal_step(q[:1, 63:64], k[:1, 63:64], v[:1, 63:64], mix, pool.at([4]))
    mhla_amd.mhla_causal_step(q[1:2, 63:64], k[1:2, 63:64], v[1:2, 63:64], mix, pool.at([2]))
    assert not torch.equal(pool.Cur[2], pool.Cur[4])
    same_bits("P", pool.P[2], pool.P[4])
    pool.reset([4])
    assert pool.refs[7] == pool.refs[5] == 1 and 7 not in pool.free
    pool.reset([2])
    assert pool.refs[7] == pool.refs[5] == 0 and {7, 5} <= set(pool.free)
