"""GPU parity: extending a ragged decode state by a token count per sequence in ONE launch chain
(mhla_causal_extend(..., counts=, left_padded=), mhla_causal_extend_ragged), through the fla layer's `token_counts` and the GPT
host.  References are existing code only, applied per sequence on that sequence's own tokens: rows of `orc.causal_fwd` over its
pos + n tokens, states against `oracle_state` and the fp64 segment formula (`extend_ragged_ref` = `extend_ref` per sequence), and,
bit for bit, `mhla_causal_extend` / `mhla_causal_step` on that sequence alone in a batch of one."""
import functools

import pytest
import torch

from decode_util import (NAN, SHAPE_IDS, SHAPES, TABLE, TABLE_CAP, TABLE_T, close_or_zero, cpu_state, extend_ragged_ref, layer_inputs,
                         one_sequence, oracle_state, padding_is_zero, ragged_start, same_seq_state, table_inputs, unchanged, window)
from gpu_util import DEV, CAUSAL_TOL, TOL, check, launches, poison, _fla_layer
from oracle import mhla_oracle as orc

pytestmark = pytest.mark.gpu

# a batch twice as large, with other counts (capacity 4 as well)
TABLE2 = TABLE + [(10, 5), (100, 130), (63, 2), (0, 1), (128, 64), (200, 7), (1, 0), (64, 64)]


@functools.lru_cache(maxsize=None)
def _batch(dtype, H, K, V, left_padded, big=False):
    """Histories, the padded extension (NaN in every padding row), the matrix, the oracle's rows per sequence -- computed once."""
    table = TABLE2 if big else TABLE
    hist, q, k, v, mix = table_inputs(H, K, V, dtype, table=tuple(table), left_padded=left_padded)
    want = [orc.causal_fwd(qs.float(), ks.float(), vs.float(), mix)[:, p:p + n] if n else None for (qs, ks, vs), (p, n) in zip(hist, table)]
    return table, hist, q, k, v, mix, want


def _extend(q, k, v, mix, state, counts, left_padded, **kw):
    import mhla_amd
    before = state.lengths
    o = mhla_amd.mhla_causal_extend(q, k, v, mix, state, counts=counts, left_padded=left_padded, **kw)
    want = tuple(p + n for p, n in zip(before, counts))
    assert state.lengths == want and state.seen == max(want) and state.pos.tolist() == list(want) and not state.stale
    assert o.shape == (q.shape[0], q.shape[1], q.shape[2], v.shape[-1]) and o.dtype == q.dtype
    return o


@pytest.mark.parametrize("left_padded", [False, True], ids=["right-padded", "left-padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_rows_and_states_of_every_sequence(shape, left_padded):
    dtype, H, K, V = shape
    table, hist, q, k, v, mix, want = _batch(dtype, H, K, V, left_padded)
    counts = tuple(n for _, n in table)
    poison()
    state = ragged_start(table, hist, mix)
    before = state.clone()
    o = _extend(q.to(DEV), k.to(DEV), v.to(DEV), mix.to(DEV), state, counts, left_padded)
    padding_is_zero(o, counts, left_padded)
    o_ref, ref = extend_ragged_ref(cpu_state(before), q, k, v, mix, counts, left_padded)
    tol = TOL[torch.float32]
    checked = 0
    for b, (p, n) in enumerate(table):
        name = f"sequence {b} (pos {p}, n {n})"
        if not n:
            same_seq_state(name + ": an idle slot keeps its state", state, b, before, b, 64 * TABLE_CAP)
            continue
        w = window(TABLE_T, n, left_padded)
        check(f"{name}: rows", o[b:b + 1, w], want[b], CAUSAL_TOL[dtype])
        check(f"{name}: rows vs extend_ref", o[b:b + 1, w], o_ref[b:b + 1, w].float(), CAUSAL_TOL[dtype])
        orc_state = oracle_state(hist[b][1].float(), hist[b][2].float(), mix, p + n, TABLE_CAP)
        nfull = (p + n) // 64
        for part, got, a, r in (("S", state.S[b:b + 1, :, :nfull], orc_state[0][:, :, :nfull], ref[0][b:b + 1, :, :nfull]),
                                ("P", state.P[b:b + 1], orc_state[1], ref[1][b:b + 1]), ("Cur", state.Cur[b:b + 1], orc_state[2], ref[2][b:b + 1])):
            close_or_zero(f"{name}: {part} vs the oracle", got, a, tol)
            close_or_zero(f"{name}: {part} vs extend_ref", got, r.float(), tol)
        if (p + n) % 64 == 0:
            assert float(state.Cur[b].abs().max()) == 0.0, f"{name}: Cur on a boundary must be exactly 0"
        if p + n == 64 * TABLE_CAP:
            assert float(state.P[b].abs().max()) == 0.0, f"{name}: P of a full state must be exactly 0"
        checked += 1
    assert checked == sum(1 for _, n in table if n) == 7


@pytest.mark.parametrize("left_padded", [False, True], ids=["right-padded", "left-padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_same_bits_as_each_sequence_alone(shape, left_padded):
    """Rows and state of every sequence equal, bit for bit, `mhla_causal_extend` on that sequence alone in a batch of one -- which
    for a count of 1 is `mhla_causal_step`."""
    import mhla_amd
    dtype, H, K, V = shape
    table, hist, q, k, v, mix, _ = _batch(dtype, H, K, V, left_padded)
    counts = tuple(n for _, n in table)
    q, k, v, mix = (t.to(DEV) for t in (q, k, v, mix))
    state = ragged_start(table, hist, mix.cpu())
    before = state.clone()
    o = _extend(q, k, v, mix, state, counts, left_padded)
    for b, (p, n) in enumerate(table):
        if not n:
            continue
        w = window(TABLE_T, n, left_padded)
        alone = one_sequence(before, b)
        fn = mhla_amd.mhla_causal_step if n == 1 else mhla_amd.mhla_causal_extend
        oa = fn(q[b:b + 1, w], k[b:b + 1, w], v[b:b + 1, w], mix, alone)
        assert alone.seen == p + n
        name = f"sequence {b} (pos {p}, n {n})"
        diff = (o[b:b + 1, w].float() - oa.float()).abs().max().item()
        print(f"{name}: max |batch - alone| = {diff:.3e}")
        assert torch.equal(o[b:b + 1, w], oa), f"{name}: rows differ from the sequence alone (max {diff:.3e})"
        same_seq_state(name, state, b, alone, 0, p + n)


def test_padding_is_never_read_and_always_written():
    dtype, H, K, V = SHAPES[2]
    for left_padded in (False, True):
        table, hist, q, k, v, mix, want = _batch(dtype, H, K, V, left_padded)
        counts = tuple(n for _, n in table)
        assert bool(torch.isnan(q[1]).all()) and bool(torch.isnan(v[5, window(TABLE_T, 3, not left_padded)]).any())   # padding rows hold NaN
        gen = torch.Generator().manual_seed(9)
        g = torch.full((len(table), TABLE_T, H, V), NAN)
        for b, n in enumerate(counts):
            g[b, window(TABLE_T, n, left_padded)] = torch.randn(n, H, V, generator=gen)
        wgt = torch.rand(V, generator=gen) + 0.5
        qd, kd, vd, md, gd = (t.to(DEV) for t in (q, k, v, mix, g.to(dtype)))
        state = ragged_start(table, hist, mix)
        nanned = state.clone()
        for b, (p, n) in enumerate(table):
            nanned.S[b, :, (p + n) // 64:] = NAN        # rows of S beyond the chunks this sequence will have finished
        before = state.clone()
        poison()
        o = _extend(qd, kd, vd, md, state, counts, left_padded)
        y = _extend(qd, kd, vd, md, before.clone(), counts, left_padded, gate=gd, norm_weight=wgt.to(DEV))
        for name, res in (("o", o), ("y", y)):
            padding_is_zero(res, counts, left_padded)
            for b, n in enumerate(counts):
                assert bool(torch.isfinite(res[b, window(TABLE_T, n, left_padded)]).all()), f"{name}: sequence {b} holds non-finite rows"
        for name, t in (("S", state.S), ("P", state.P), ("Cur", state.Cur)):
            assert bool(torch.isfinite(t).all()), f"{name} holds non-finite values"
        same_seq_state("an idle slot keeps its state", state, 1, before, 1, 64 * TABLE_CAP)
        assert torch.equal(state.S[1], before.S[1])
        o2 = _extend(qd, kd, vd, md, nanned, counts, left_padded)
        assert torch.equal(o2, o)
        for b, (p, n) in enumerate(table):
            nfull = (p + n) // 64
            same_seq_state(f"sequence {b}: NaN beyond the finished chunks", nanned, b, state, b, p + n)
            assert bool(torch.isnan(nanned.S[b, :, nfull:]).all()), f"sequence {b}: S beyond chunk {nfull} was written"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_epilogue_and_strided_views(dtype):
    """gate and norm_weight in the chain, q, k, v as strided slices of one packed projection: y against the norm x gate of the plain
    rows, at the bound the epilogue tests of the step and the uniform extend hold."""
    H, K, V = 2, 64, 128
    left_padded = True
    table, hist, q, k, v, mix, want = _batch(dtype, H, K, V, left_padded)
    counts = tuple(n for _, n in table)
    B = len(table)
    gen = torch.Generator().manual_seed(21)
    g = torch.randn(B, TABLE_T, H, V, generator=gen).to(dtype)
    wgt = torch.rand(V, generator=gen) + 0.5
    packed = torch.cat([q, k, v], dim=-1).reshape(B, TABLE_T, H * (2 * K + V)).contiguous().view(B, TABLE_T, H, 2 * K + V).to(DEV)
    qv, kv, vv = packed[..., :K], packed[..., K:2 * K], packed[..., 2 * K:]
    assert not kv.is_contiguous() and kv.data_ptr() != packed.data_ptr()
    poison()
    state = ragged_start(table, hist, mix)
    plain = state.clone()
    y = _extend(qv, kv, vv, mix.to(DEV), state, counts, left_padded, gate=g.to(DEV), norm_weight=wgt.to(DEV), norm_eps=1e-5)
    padding_is_zero(y, counts, left_padded)
    for b, (p, n) in enumerate(table):
        if n:
            w = window(TABLE_T, n, left_padded)
            y_ref = orc.rms_norm_swish_gate(want[b], g[b:b + 1, w].float(), wgt, 1e-5)
            check(f"sequence {b} (pos {p}, n {n}): y", y[b:b + 1, w], y_ref, CAUSAL_TOL[dtype])
    # the state does not depend on the epilogue or on the views
    _extend(q.to(DEV), k.to(DEV), v.to(DEV), mix.to(DEV), plain, counts, left_padded)
    for b, (p, n) in enumerate(table):
        same_seq_state(f"sequence {b}: epilogue or not", state, b, plain, b, p + n)


def test_launch_count_depends_on_nothing():
    import mhla_amd
    dtype, H, K, V = SHAPES[2]
    ran = {}
    for big in (False, True):
        table, hist, q, k, v, mix, _ = _batch(dtype, H, K, V, False, big)
        counts = tuple(n for _, n in table)
        q, k, v, mix = (t.to(DEV) for t in (q, k, v, mix))
        state = ragged_start(table, hist, mix.cpu())
        loop = state.clone()
        ran[big] = launches(lambda: _extend(q, k, v, mix, state, counts, False))
        assert ran[big] and "k_cs_step" not in ran[big] and "k_cx_out_ragged" in ran[big], ran[big]
        assert sum(ran[big].values()) <= 8, ran[big]

        def per_sequence():
            for b, (p, n) in enumerate(table):
                if n:
                    mhla_amd.mhla_causal_extend(q[b:b + 1, :n], k[b:b + 1, :n], v[b:b + 1, :n], mix, one_sequence(loop, b))
        looped = launches(per_sequence)
        assert sum(looped.values()) > sum(ran[big].values()), (looped, ran[big])
    assert sum(ran[True].values()) == sum(ran[False].values()), ran


def test_two_runs_give_equal_bits():
    dtype, H, K, V = SHAPES[2]
    table, hist, q, k, v, mix, _ = _batch(dtype, H, K, V, True)
    counts = tuple(n for _, n in table)
    q, k, v, mix = (t.to(DEV) for t in (q, k, v, mix))
    s0 = ragged_start(table, hist, mix.cpu())
    runs = []
    for _ in range(2):
        st = s0.clone()
        assert st.S.data_ptr() != s0.S.data_ptr()
        runs.append((_extend(q, k, v, mix, st, counts, True), st))
    (oa, sa), (ob, sb) = runs
    assert torch.equal(oa, ob) and torch.equal(sa.P, sb.P) and torch.equal(sa.Cur, sb.Cur) and torch.equal(sa.S, sb.S)
    assert torch.equal(sa.pos, sb.pos)


def test_refusals_leave_the_state_untouched():
    import mhla_amd
    from mhla_amd import _lib, ops
    dtype, H, K, V = SHAPES[0]
    table, hist, q, k, v, mix, _ = _batch(dtype, H, K, V, False)
    B = len(table)
    q, k, v, mix = (t.to(DEV) for t in (q, k, v, mix))
    state = ragged_start(table, hist, mix.cpu())
    keep = state.clone()
    ext = lambda counts, m=mix: mhla_amd.mhla_causal_extend(q, k, v, m, state, counts=counts)
    with pytest.raises(IndexError, match=r"sequences \[7\].*the state holds only 4"):
        ext([0, 0, 0, 0, 0, 0, 0, 65])              # sequence 7 is at 192 of 256
    unchanged(state, keep)
    with pytest.raises(IndexError, match=r"sequences \[3, 7\].*mixing_matrix has only 1 rows"):
        ext([1, 1, 1, 1, 1, 1, 1, 1], m=mix[:1, :1].contiguous())   # sequences 3 (at 64) and 7 (at 192) are beyond chunk 0
    unchanged(state, keep)

    # the raw entry point
    lib = _lib.load()
    counts = [n for _, n in table]
    ntok = torch.tensor(counts, dtype=torch.int32, device=DEV)
    plan = ops._ragged_plan(state.lengths, counts, TABLE_CAP)
    assert plan[:3] == (256, 2, True)
    need = lib.mhla_causal_extend_ragged_ws_bytes(B, TABLE_T, H, K, V, plan[1], _lib.F32)
    ws = torch.empty(need // 4 + 4, dtype=torch.float32, device=DEV)
    out = torch.empty(B, TABLE_T, H, V, device=DEV)
    mixf = mix.contiguous()

    def raw(T=TABLE_T, ws_bytes=need, ldmix=mixf.shape[1], max_end=plan[0], pos=state.pos):
        return lib.mhla_causal_extend_ragged(ops._view(q), ops._view(k), ops._view(v), mixf.data_ptr(), ldmix, state.S.data_ptr(), TABLE_CAP,
                                             state.P.data_ptr(), state.Cur.data_ptr(), pos.data_ptr() if pos is not None else None,
                                             ntok.data_ptr(), T, max_end, plan[1], 1, 0, ops._view(out), _lib.NULL_VIEW, None, 1e-5,
                                             _lib.NULL_VIEW, ws.data_ptr(), ws_bytes, B, H, K, V, 64, K ** -0.5, _lib.F32, ops._stream())
    EINVAL = -22
    assert raw(ws_bytes=need - 4) == EINVAL and b"workspace too small" in lib.mhla_last_error()
    assert raw(ldmix=3) == EINVAL and b"ldmix=3 < 4" in lib.mhla_last_error()
    assert raw(T=0) == EINVAL and b"T=0" in lib.mhla_last_error()
    assert raw(T=65536) == EINVAL and b"T=65536" in lib.mhla_last_error()
    assert raw(max_end=257) == EINVAL and b"max_end=257" in lib.mhla_last_error()
    assert raw(pos=None) == EINVAL and b"pos_dev" in lib.mhla_last_error()
    unchanged(state, keep)


def test_interleaved_with_ragged_steps():
    """Ragged extend, a ragged step, a ragged extend with other counts: the state of `mhla_causal_state(lengths=)` over every
    sequence's whole history, and every row that of the operator over that history."""
    import mhla_amd
    dtype, H, K, V, cap, L = torch.bfloat16, 2, 64, 64, 3, 4
    pos0, first, second = (60, 0, 37, 64), (10, 0, 27, 70), (3, 64, 0, 1)
    total = [p + a + 1 + c for p, a, c in zip(pos0, first, second)]
    table = tuple((0, n) for n in total)
    hist, _, _, _, mix = table_inputs(H, K, V, dtype, table=table, T=max(total), L=L, seed=5)
    want = [orc.causal_fwd(qs.float(), ks.float(), vs.float(), mix) for qs, ks, vs in hist]
    B = len(total)
    state = ragged_start(tuple((p, 0) for p in pos0), hist, mix, cap)
    md = mix.to(DEV)

    def padded(counts, T, left_padded):
        q, k = (torch.full((B, T, H, K), NAN, dtype=dtype) for _ in range(2))
        v = torch.full((B, T, H, V), NAN, dtype=dtype)
        for b, n in enumerate(counts):
            p, w = state.lengths[b], window(T, n, left_padded)
            q[b, w], k[b, w], v[b, w] = hist[b][0][0, p:p + n], hist[b][1][0, p:p + n], hist[b][2][0, p:p + n]
        return q.to(DEV), k.to(DEV), v.to(DEV)

    def rows(o, counts, left_padded, at):
        for b, n in enumerate(counts):
            if n:
                check(f"sequence {b}: rows {at[b]} .. {at[b] + n - 1}", o[b:b + 1, window(o.shape[1], n, left_padded)], want[b][:, at[b]:at[b] + n],
                      CAUSAL_TOL[dtype])

    poison()
    at = state.lengths
    rows(_extend(*padded(first, 70, True), md, state, first, True), first, True, at)
    at = state.lengths
    o = mhla_amd.mhla_causal_step(*padded((1,) * B, 1, False), md, state)
    rows(o, (1,) * B, False, at)
    at = state.lengths
    rows(_extend(*padded(second, 64, False), md, state, second, False), second, False, at)
    assert state.lengths == tuple(total)
    k_all, v_all = (torch.zeros(B, max(total), H, d, dtype=dtype) for d in (K, V))
    for b, n in enumerate(total):
        k_all[b, :n], v_all[b, :n] = hist[b][1][0], hist[b][2][0]
    ref = mhla_amd.mhla_causal_state(k_all.to(DEV), v_all.to(DEV), md, lengths=total, capacity_chunks=cap)
    for b, n in enumerate(total):
        for part, x, y in (("S", state.S[b, :, :n // 64], ref.S[b, :, :n // 64]), ("P", state.P[b], ref.P[b]), ("Cur", state.Cur[b], ref.Cur[b])):
            close_or_zero(f"sequence {b}: {part} vs one prefill of its whole history", x, y.cpu(), TOL[torch.float32])


def test_no_counts_on_differing_lengths_takes_the_ragged_chain():
    """Without `counts` a ragged state of differing lengths gets T tokens per sequence in the one ragged chain (the same bits as
    every sequence alone); equal lengths keep the uniform chain."""
    import mhla_amd
    dtype, H, K, V, T = torch.bfloat16, 2, 64, 64, 70
    table = ((60, T), (0, T), (64, T))
    hist, q, k, v, mix = table_inputs(H, K, V, dtype, table=table, T=T, L=4, seed=11)
    q, k, v, md = (t.to(DEV) for t in (q, k, v, mix))
    state = ragged_start(table, hist, mix, 4)
    before = state.clone()
    ran = launches(lambda: mhla_amd.mhla_causal_extend(q, k, v, md, state))
    assert "k_cx_out_ragged" in ran and sum(ran.values()) <= 8, ran
    assert state.lengths == (130, 70, 134) and state.pos.tolist() == [130, 70, 134] and state.seen == 134
    o = mhla_amd.mhla_causal_extend(q, k, v, md, before.clone())
    for b, (p, n) in enumerate(table):
        alone = one_sequence(before, b)
        assert torch.equal(o[b:b + 1], mhla_amd.mhla_causal_extend(q[b:b + 1], k[b:b + 1], v[b:b + 1], md, alone))
        same_seq_state(f"sequence {b}", state, b, alone, 0, p + n)
    same = ragged_start(((60, T), (60, T)), hist[:1] * 2, mix, 4)
    ran = launches(lambda: mhla_amd.mhla_causal_extend(q[:2], k[:2], v[:2], md, same))
    assert "k_cx_out" in ran and "k_cx_out_ragged" not in ran, ran


def test_large_batches_are_sliced_and_a_workspace_over_the_cap_falls_back(monkeypatch):
    """A (b, h) range of three batch entries slices the batch: the same kernels on every slice, so the same bits as one chain.  A
    workspace cap of one byte sends the call through the uniform chain sequence by sequence: the same rows and state within
    the rounding of fp32 sums taken in another order, padding rows zero, positions advanced."""
    from mhla_amd import ops
    dtype, H, K, V = SHAPES[2]
    table, hist, q, k, v, mix, want = _batch(dtype, H, K, V, True)
    counts = tuple(n for _, n in table)
    q, k, v, mix = (t.to(DEV) for t in (q, k, v, mix))
    s0 = ragged_start(table, hist, mix.cpu())
    whole = s0.clone()
    o_whole = _extend(q, k, v, mix, whole, counts, True)
    monkeypatch.setattr(ops, "_MAX_GRID_BH", 3 * H)
    sliced = s0.clone()
    ran = launches(lambda: _extend(q, k, v, mix, sliced, counts, True))
    assert ran["k_cs_step_finish_ragged"] == 3 and "k_cx_out" not in ran, ran      # slices of 3, 3 and 2 sequences
    sliced = s0.clone()
    assert torch.equal(_extend(q, k, v, mix, sliced, counts, True), o_whole)
    for b, (p, n) in enumerate(table):
        same_seq_state(f"sequence {b}: sliced vs one chain", sliced, b, whole, b, p + n)
    monkeypatch.setattr(ops, "EXTEND_WS_CAP_BYTES", 1)
    cut = s0.clone()
    ran = launches(lambda: _extend(q, k, v, mix, cut, counts, True))
    assert "k_cx_out" in ran and "k_cx_out_ragged" not in ran, ran
    cut = s0.clone()
    o_cut = _extend(q, k, v, mix, cut, counts, True)
    padding_is_zero(o_cut, counts, True)
    for b, (p, n) in enumerate(table):
        if n:
            check(f"sequence {b}: rows of the fallback", o_cut[b:b + 1, window(TABLE_T, n, True)], want[b], CAUSAL_TOL[dtype])
        nfull = (p + n) // 64
        for part, x, y in (("S", cut.S[b, :, :nfull], whole.S[b, :, :nfull]), ("P", cut.P[b], whole.P[b]), ("Cur", cut.Cur[b], whole.Cur[b])):
            close_or_zero(f"sequence {b}: {part} of the fallback vs the chain", x, y.cpu(), TOL[torch.float32])


def test_all_counts_zero_is_a_no_op():
    dtype, H, K, V = SHAPES[0]
    table, hist, q, k, v, mix, _ = _batch(dtype, H, K, V, False)
    state = ragged_start(table, hist, mix)
    keep = state.clone()
    ran = launches(lambda: _extend(q.to(DEV), k.to(DEV), v.to(DEV), mix.to(DEV), state, (0,) * len(table), False))
    assert not ran, ran
    unchanged(state, keep)


@pytest.mark.parametrize("opts", [{}, {"use_output_gate": False}], ids=["default", "no-output-gate"])
def test_fla_layer_token_counts(opts):
    """A call with `token_counts` equals, per sequence, that sequence run alone through the same layer with a cache of its own."""
    from mhla_amd import modules
    m = _fla_layer(**opts).to(DEV).eval()
    prompts, counts, T = (70, 20, 64), (3, 130, 0), 130
    x0 = layer_inputs(3, 70, 31).to(DEV)
    x1 = layer_inputs(3, T, 32).to(DEV)
    mask = torch.zeros(3, 70, dtype=torch.long, device=DEV)
    for b, n in enumerate(prompts):
        mask[b, 70 - n:] = 1
    cache = modules.DecodeCache()
    with torch.no_grad():
        m(x0, attention_mask=mask, past_key_values=cache, use_cache=True)
        y = m(x1, past_key_values=cache, use_cache=True, token_counts=counts)[0]
        st = cache[0]["recurrent_state"]
        assert st.lengths == (73, 150, 64) and cache.get_seq_length() == 150
        for b, (p, n) in enumerate(zip(prompts, counts)):
            assert n == T or float(y[b, :T - n].abs().max()) == 0.0, f"sequence {b}: padding rows must be zero"
            if n:
                own = modules.DecodeCache()
                m(x0[b:b + 1, 70 - p:], past_key_values=own, use_cache=True)
                alone = m(x1[b:b + 1, T - n:], past_key_values=own, use_cache=True)[0]
                check(f"sequence {b}: {n} tokens at {p}", y[b:b + 1, T - n:], alone.cpu(), 1e-4)


def test_fla_layer_token_counts_refusals():
    from mhla_amd import modules
    m = _fla_layer().to(DEV).eval()
    x0, x1 = layer_inputs(2, 10, 41).to(DEV), layer_inputs(2, 4, 42).to(DEV)
    mask = torch.tensor([[0] * 5 + [1] * 5, [1] * 10], device=DEV)
    cache = modules.DecodeCache()
    with torch.no_grad():
        m(x0, attention_mask=mask, past_key_values=cache, use_cache=True)
        with pytest.raises(ValueError, match="token_counts"):
            m(x1, past_key_values=cache, use_cache=True, token_counts=[1, 5])
        with pytest.raises(ValueError, match="token_counts"):
            m(x1, past_key_values=cache, use_cache=True, token_counts=[1])
        assert cache[0]["recurrent_state"].lengths == (5, 10)


def test_gpt_host_token_counts():
    from mhla_amd.hosts.gpt import GPT_MHLA
    from mhla_amd.modules import DecodeCache
    torch.manual_seed(5)
    model = GPT_MHLA(vocab_size=512, hidden_size=128, num_layers=2, num_heads=4, max_seq_len=2048, exact_decoding=True).to(DEV).eval()
    gen = torch.Generator().manual_seed(6)
    prompts, counts, T0, T = (30, 66), (70, 1), 66, 70
    ids0 = torch.randint(0, 512, (2, T0), generator=gen).to(DEV)
    ids1 = torch.randint(0, 512, (2, T), generator=gen).to(DEV)
    mask = torch.zeros(2, T0, dtype=torch.long, device=DEV)
    for b, n in enumerate(prompts):
        mask[b, T0 - n:] = 1
    with torch.no_grad():
        cache = DecodeCache()
        model(ids0, cache=cache, attention_mask=mask)
        logits = model(ids1, cache=cache, token_counts=torch.tensor(counts))
        assert cache[1]["recurrent_state"].lengths == (100, 67) and cache.get_seq_length(0) == cache.get_seq_length(1) == 100
        for b, (p, n) in enumerate(zip(prompts, counts)):
            own = DecodeCache()
            model(ids0[b:b + 1, T0 - p:], cache=own)
            alone = model(ids1[b:b + 1, T - n:], cache=own)
            check(f"sequence {b}: logits of its {n} tokens at {p} vs the sequence alone", logits[b:b + 1, T - n:], alone.cpu(), 1e-4)
