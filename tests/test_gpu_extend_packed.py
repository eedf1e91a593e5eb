"""GPU: packed new tokens (`cu_seqlens=`) in mhla_causal_extend, mhla_causal_verify and mhla_causal_commit -- the library's
mhla_causal_{extend,verify,commit}_packed -- against today's PADDED calls on the same start state, BIT FOR BIT per sequence (rows,
finished chunks, P, Cur, pos, lengths), and against the fp64 segment formula at the tolerances `check_step_rows` / `check_state`
carry.  The sequences are `decode_util.TABLE` (8 sequences, 305 tokens, capacity 4, a 5 x 5 matrix), the drafts `SPEC_TABLE`; the
shapes are the smallest at which the tiling branches differ.  On views of a dense and of an fp32 paged pool (slots permuted, one
unused, every other byte poison: `pool_util.fill_pool`) the reference is the same packed call on `view.compact()`, and nothing the
call does not name changes a bit (`pool_util.check_untouched`)."""
import functools

import pytest
import torch

import mhla_amd
from decode_util import (ACCEPT, COUNTS, DRAFTS, SPEC_CAP, SPEC_L, SPEC_T, TABLE, TABLE_CAP, check_state, check_step_rows, cpu_state,
                         extend_ragged_ref, one_sequence, packed_views, ragged_start, same_seq_state, table_inputs, unchanged)
from gpu_util import DEV, launches, poison
from pool_util import check_untouched, fill_pool, snapshot

pytestmark = pytest.mark.gpu

# (dtype, H, Hkv, K, V)
SHAPES = [(torch.float32, 2, 2, 64, 64), (torch.bfloat16, 2, 2, 64, 64), (torch.float32, 2, 2, 40, 72), (torch.bfloat16, 4, 2, 64, 64)]
IDS = ["fp32-K64V64", "bf16-K64V64", "fp32-K40V72", "bf16-G2"]


def _cu(counts):
    cu = [0]
    for n in counts:
        cu.append(cu[-1] + n)
    return cu


def _pack(x, counts):
    """[B, T, ...] right-padded -> [1, N, ...]: every sequence's window, one after the other."""
    return torch.cat([x[b, :n] for b, n in enumerate(counts)]).unsqueeze(0).contiguous()


@functools.lru_cache(maxsize=None)
def _batch(dtype, H, Hkv, K, V, spec=False):
    """The histories (k, v on Hkv heads), the padded tokens with NaN in every padding row, the pack, the offsets, a gate, a norm
    weight and the matrix, on the device -- built once per shape."""
    table = DRAFTS if spec else TABLE
    hist, q, k, v, mix = table_inputs(H, K, V, dtype, table=tuple(table), T=SPEC_T, L=SPEC_L)
    hist = [(qs, ks[:, :, :Hkv].contiguous(), vs[:, :, :Hkv].contiguous()) for qs, ks, vs in hist]
    k, v = k[:, :, :Hkv].contiguous(), v[:, :, :Hkv].contiguous()
    counts = tuple(n for _, n in table)
    gen = torch.Generator().manual_seed(5)
    gate = torch.randn(len(table), SPEC_T, H, V, generator=gen).to(dtype)
    w = (torch.rand(V, generator=gen) + 0.5).to(DEV)
    pad = tuple(t.to(DEV) for t in (q, k, v, gate))
    pack = tuple(_pack(t, counts).to(DEV) for t in (q, k, v, gate))
    return table, hist, counts, _cu(counts), pad, pack, w, mix


def _start(shape, spec=False):
    table, hist, *_, mix = _batch(*shape, spec)
    return ragged_start(table, hist, mix, SPEC_CAP if spec else TABLE_CAP)


@functools.lru_cache(maxsize=None)
def _padded_extend(shape):
    """Today's padded call on the start state: (rows, the state afterwards, the state before), once per shape."""
    table, hist, counts, cu, (q, k, v, _), _, _, mix = _batch(*shape)
    state = _start(shape)
    before = state.clone()
    o = mhla_amd.mhla_causal_extend(q, k, v, mix.to(DEV), state, counts=counts)
    return o, state, before


def _same_rows(name, got, want, counts, cu):
    """The pack's rows of every sequence equal the padded call's window, bit for bit; nothing is NaN."""
    assert got.shape == (1, cu[-1]) + tuple(want.shape[2:]) and got.dtype == want.dtype
    assert not bool(torch.isnan(got).any()), f"{name}: NaN in the rows of the pack"
    for b, n in enumerate(counts):
        assert torch.equal(got[0, cu[b]:cu[b + 1]], want[b, :n]), f"{name}: rows of sequence {b} ({n} tokens) differ from the padded call's"


def _same_states(name, a, b, lengths):
    torch.cuda.synchronize()
    assert a.lengths == b.lengths == tuple(lengths) and a.seen == b.seen == max(lengths)
    assert torch.equal(a.pos, b.pos) and a.pos.tolist() == list(lengths), f"{name}: pos"
    for i, n in enumerate(lengths):
        same_seq_state(f"{name}: sequence {i}", a, i, b, i, n)
    for part in ("P", "Cur"):
        assert not bool(torch.isnan(getattr(a, part)).any()), f"{name}: NaN in {part}"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_extend_packed_equals_padded(shape):
    table, hist, counts, cu, _, (q, k, v, _), _, mix = _batch(*shape)
    want, ref, before = _padded_extend(shape)
    poison()
    state = before.clone()
    got = mhla_amd.mhla_causal_extend(q, k, v, mix.to(DEV), state, cu_seqlens=cu)
    _same_rows("extend", got, want, counts, cu)
    _same_states("extend", state, ref, [p + n for p, n in table])
    same_seq_state("an idle sequence keeps its state", state, 1, before, 1, 64 * TABLE_CAP)
    # (offsets as a tensor and as a plan: the same call)
    for form in (torch.tensor(cu, dtype=torch.int32, device=DEV), mhla_amd.causal_varlen_plan(cu, DEV)):
        again = before.clone()
        assert torch.equal(mhla_amd.mhla_causal_extend(q, k, v, mix.to(DEV), again, cu_seqlens=form), got)
        _same_states("extend (another form of cu_seqlens)", again, ref, [p + n for p, n in table])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_extend_packed_against_fp64(shape):
    dtype, H, Hkv, K, V = shape
    G = H // Hkv
    table, hist, counts, cu, (qp, kp, vp, _), (q, k, v, _), _, mix = _batch(*shape)
    state = _start(shape)
    S, P, Cur, lengths = cpu_state(state)
    rep = lambda t, dim: t.repeat_interleave(G, dim=dim)
    # (padding rows hold NaN: the reference never reads them either)
    o_ref, _ = extend_ragged_ref((rep(S, 1), rep(P, 1), rep(Cur, 1), lengths), qp.cpu(), rep(kp.cpu(), 2), rep(vp.cpu(), 2), mix, counts)
    got = mhla_amd.mhla_causal_extend(q, k, v, mix.to(DEV), state, cu_seqlens=cu)
    T0 = max(p + n for p, n in table) + 1
    kh, vh = torch.zeros(len(table), T0, Hkv, K), torch.zeros(len(table), T0, Hkv, V)
    for b, (p, n) in enumerate(table):
        kh[b, :p + n], vh[b, :p + n] = hist[b][1][0].float(), hist[b][2][0].float()
        if not n:
            continue
        whole = torch.zeros(1, p + n, H, V, dtype=torch.float64)   # (check_step_rows takes the sequence's rows from its first token)
        whole[:, p:] = o_ref[b:b + 1, :n]
        check_step_rows(f"sequence {b} (pos {p}, n {n}): rows", got[:, cu[b]:cu[b + 1]], whole.float(), p, dtype)
        check_state(state, torch.zeros_like(kh), kh, vh, mix, f"sequence {b} (pos {p}, n {n})", b=b, s=p + n)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_verify_then_commit_packed_equal_padded(shape):
    table, hist, counts, cu, (qp, kp, vp, _), (q, k, v, _), _, mix = _batch(*shape, True)
    assert counts == COUNTS
    md = mix.to(DEV)
    ref = _start(shape, True)
    state, keep = ref.clone(), ref.clone()
    want, draft_pad = mhla_amd.mhla_causal_verify(qp, kp, vp, md, ref, counts=counts)
    poison()
    got, draft = mhla_amd.mhla_causal_verify(q, k, v, md, state, cu_seqlens=cu)
    assert draft.cu == tuple(cu) and draft.counts == counts and draft_pad.cu is None
    _same_rows("verify", got, want, counts, cu)
    n_before = [p // 64 for p, _ in table]
    torch.cuda.synchronize()
    assert state.lengths == keep.lengths and state.seen == keep.seen and torch.equal(state.pos, keep.pos)
    assert torch.equal(state.P, keep.P) and torch.equal(state.Cur, keep.Cur)
    for b, nf in enumerate(n_before):
        assert torch.equal(state.S[b, :, :nf], keep.S[b, :, :nf]), f"the verify changed a finished chunk of sequence {b}"
    assert mhla_amd.mhla_causal_commit(draft_pad, md, ref, ACCEPT) is ref
    assert mhla_amd.mhla_causal_commit(draft, md, state, ACCEPT) is state
    _same_states("commit", state, ref, [p + a for (p, _), a in zip(table, ACCEPT)])
    # every draft rejected: nothing is launched, every bit stays
    st0 = _start(shape, True)
    keep0 = st0.clone()
    _, d0 = mhla_amd.mhla_causal_verify(q, k, v, md, st0, cu_seqlens=cu)
    keep0.S.copy_(st0.S)   # (rows of S beyond the finished chunks are the verify's scratch)
    assert launches(lambda: mhla_amd.mhla_causal_commit(d0, md, st0, (0,) * len(table))) == {}
    unchanged(st0, keep0)


@pytest.mark.parametrize("kind", ["dense", "paged"])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=[IDS[1], IDS[3]])
def test_the_same_three_on_views_of_a_pool(shape, kind):
    md = _batch(*shape)[-1].to(DEV)
    for spec in (False, True):
        table, hist, counts, cu, _, (q, k, v, _), _, _ = _batch(*shape, spec)
        B = len(table)
        unused = B // 2
        slots = [s for s in reversed(range(B + 1)) if s != unused]
        slots = slots[1::2] + slots[0::2]   # (neither ascending nor descending)
        start = _start(shape, spec)
        # (pages handed out from the top of 4 B: every sequence's block below the one before it)
        pages, top = {}, 4 * B
        for s, n in zip(slots, start.lengths):
            pages[s], top = list(range(top - -(-n // 64), top)), top - -(-n // 64)
        pool = fill_pool(kind, start, slots, n_slots=B + 1, table=pages, n_pages=4 * B)
        view = pool.at(slots)
        assert view.lengths == start.lengths
        ref, before = view.compact(), snapshot(pool)
        if not spec:
            want = mhla_amd.mhla_causal_extend(q, k, v, md, ref, cu_seqlens=cu)
            got = mhla_amd.mhla_causal_extend(q, k, v, md, view, cu_seqlens=cu)
            after = [p + n for p, n in table]
        else:
            want, dr = mhla_amd.mhla_causal_verify(q, k, v, md, ref, cu_seqlens=cu)
            got, dv = mhla_amd.mhla_causal_verify(q, k, v, md, view, cu_seqlens=cu)
            assert dv.view is view and view.lengths == start.lengths
            mhla_amd.mhla_causal_commit(dr, md, ref, ACCEPT)
            assert mhla_amd.mhla_causal_commit(dv, md, view, ACCEPT) is view
            after = [p + a for (p, _), a in zip(table, ACCEPT)]
        assert torch.equal(got, want), f"{kind} view, {'verify' if spec else 'extend'}: rows differ from the call on view.compact()"
        _same_states(f"{kind} view", view.compact(), ref, after)
        assert [pool.lengths[s] for s in slots] == after and pool.lengths[unused] == 0
        # the unused slot and every page but those the new tokens reach (to the draft's end, for a verify) keep every bit
        check_untouched(f"{kind} view", pool, before, slots, reach=[p + n for p, n in table])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_token_per_sequence_is_the_step(shape):
    dtype, H, Hkv, K, V = shape
    table = ((63, 1), (64, 1), (5, 1))
    hist, q, k, v, mix = table_inputs(H, K, V, dtype, table=table, T=1)
    hist = [(qs, ks[:, :, :Hkv].contiguous(), vs[:, :, :Hkv].contiguous()) for qs, ks, vs in hist]
    q, k, v, md = q.to(DEV), k[:, :, :Hkv].contiguous().to(DEV), v[:, :, :Hkv].contiguous().to(DEV), mix.to(DEV)
    state = ragged_start(table, hist, mix)
    before = state.clone()
    got = mhla_amd.mhla_causal_extend(*(t.transpose(0, 1).contiguous() for t in (q, k, v)), md, state, cu_seqlens=[0, 1, 2, 3])
    assert state.lengths == (64, 65, 6) and state.pos.tolist() == [64, 65, 6]
    for b, (p, _) in enumerate(table):
        alone = one_sequence(before, b)
        want = mhla_amd.mhla_causal_step(q[b:b + 1], k[b:b + 1], v[b:b + 1], md, alone)
        assert torch.equal(got[:, b:b + 1], want), f"the one token of sequence {b} (pos {p}) is not the step's"
        same_seq_state(f"sequence {b} (pos {p})", state, b, alone, 0, p + 1)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]], ids=[IDS[1], IDS[2]])
def test_strided_views_and_the_epilogue(shape):
    table, hist, counts, cu, (qp, kp, vp, gp), (q, k, v, g), w, mix = _batch(*shape)
    md = mix.to(DEV)
    _, _, before = _padded_extend(shape)
    ref, state = before.clone(), before.clone()
    kw = dict(norm_weight=w, norm_eps=1e-5)
    want = mhla_amd.mhla_causal_extend(*packed_views(qp, kp, vp), md, ref, counts=counts, gate=gp, **kw)
    poison()
    got = mhla_amd.mhla_causal_extend(*packed_views(q, k, v), md, state, cu_seqlens=cu, gate=g, **kw)
    _same_rows("strided views, norm x gate", got, want, counts, cu)
    _same_states("strided views, norm x gate", state, ref, [p + n for p, n in table])


def test_a_pack_cut_into_two_chains(monkeypatch):
    shape = SHAPES[0]
    dtype, H, Hkv, K, V = shape
    table, hist, counts, cu, _, (q, k, v, _), _, mix = _batch(*shape)
    md = mix.to(DEV)
    _, _, before = _padded_extend(shape)
    whole, cut = before.clone(), before.clone()
    call = lambda st: mhla_amd.mhla_causal_extend(q, k, v, md, st, cu_seqlens=cu)
    want = None

    def run_whole():
        nonlocal want
        want = call(whole)
    uncut = launches(run_whole)
    from mhla_amd import _lib, ops
    need = _lib.load().mhla_causal_extend_packed_ws_bytes(len(table), cu[-1], H, Hkv, K, V, 2, 0)
    monkeypatch.setattr(ops, "EXTEND_WS_CAP_BYTES", need - 1)   # (the whole pack no longer fits; every sequence alone does)
    got = None

    def run_cut():
        nonlocal got
        got = call(cut)
    names = launches(run_cut)
    assert uncut["k_cs_step_finish_packed"] == 1 and names["k_cs_step_finish_packed"] == 2, (uncut, names)
    assert sum(uncut.values()) <= 6
    assert torch.equal(got, want)
    _same_states("two chains", cut, whole, [p + n for p, n in table])
