"""GPU parity: verifying a draft without committing it and committing the accepted prefix (mhla_causal_verify / mhla_causal_commit,
mhla_causal_verify_ragged / mhla_causal_commit_ragged), through the fla layer's `speculative=True` with `DecodeCache.commit`, and
the GPT host's `generate(draft=)`.  References are existing code only: bit for bit `mhla_causal_extend(counts=)` on a clone of the
state, rows of `orc.causal_fwd` and states of `oracle_state` per sequence, the layer and the host on one sequence alone, and
plain greedy `generate`."""
import functools

import pytest
import torch

from decode_util import (ACCEPT, COUNTS, DRAFTS, NAN, SHAPE_IDS, SHAPES, SPEC_CAP, SPEC_L, SPEC_T, SPEC_TABLE, close_or_zero, layer_inputs,
                         oracle_state, padding_is_zero, ragged_start, same_seq_state, table_inputs, unchanged, window)
from gpu_util import DEV, CAUSAL_TOL, TOL, check, launches, poison, _fla_layer
from oracle import mhla_oracle as orc

pytestmark = pytest.mark.gpu

B = len(SPEC_TABLE)
# other accepted counts with a chunk closing somewhere, as in ACCEPT: the commit's launches must not depend on the counts
ACCEPT2 = (10, 0, 9, 1, 0, 0, 1, 130, 3, 1, 0, 64)
# no sequence closes a chunk
ACCEPT_OPEN = (3, 2, 1, 0, 0, 0, 0, 63, 3, 63, 10, 0)


@functools.lru_cache(maxsize=None)
def _batch(dtype, H, K, V, left_padded):
    """Histories, the padded drafts (NaN in every padding row), the matrix, the oracle's rows per sequence -- computed once."""
    hist, q, k, v, mix = table_inputs(H, K, V, dtype, table=DRAFTS, T=SPEC_T, L=SPEC_L, left_padded=left_padded)
    want = [orc.causal_fwd(qs.float(), ks.float(), vs.float(), mix)[:, p:p + n] if n else None for (qs, ks, vs), (p, n) in zip(hist, DRAFTS)]
    return hist, q.to(DEV), k.to(DEV), v.to(DEV), mix, want


def _state(hist, mix, cap=SPEC_CAP, table=DRAFTS):
    """The ragged state before the verify, with NaN in every row of S at or beyond each sequence's finished chunks: a read of an
    unfinished row shows."""
    state = ragged_start(table, hist, mix, cap)
    for b, (p, _) in enumerate(table):
        state.S[b, :, p // 64:] = NAN
    return state


def _verify(q, k, v, mix, state, counts, left_padded, **kw):
    import mhla_amd
    o, draft = mhla_amd.mhla_causal_verify(q, k, v, mix, state, counts=counts, left_padded=left_padded, **kw)
    assert isinstance(draft, mhla_amd.CausalDraft) and draft.counts == tuple(counts) and draft.lengths == state.lengths
    assert draft.left_padded == bool(left_padded)
    assert o.shape == (q.shape[0], q.shape[1], q.shape[2], v.shape[-1]) and o.dtype == q.dtype
    return o, draft


def _verify_left_the_state(state, before):
    torch.cuda.synchronize()
    assert state.lengths == before.lengths and state.seen == before.seen and not state.stale
    assert torch.equal(state.pos, before.pos) and torch.equal(state.P, before.P) and torch.equal(state.Cur, before.Cur)
    for b, p in enumerate(before.lengths):
        assert torch.equal(state.S[b, :, :p // 64], before.S[b, :, :p // 64]), f"sequence {b}: a finished chunk of S changed"


def _accepted(k, v, counts, accept, left_padded):
    """k, v with the first accept[b] rows of every draft window moved to where a window of accept[b] rows lies (NaN elsewhere): what
    `mhla_causal_extend(counts=accept)` takes."""
    T = k.shape[1]
    ka, va = torch.full_like(k, NAN), torch.full_like(v, NAN)
    for b, (n, a) in enumerate(zip(counts, accept)):
        s0 = window(T, n, left_padded).start
        ka[b, window(T, a, left_padded)], va[b, window(T, a, left_padded)] = k[b, s0:s0 + a], v[b, s0:s0 + a]
    return ka, va


def _extended(q, k, v, mix, before, counts, accept, left_padded):
    """The state `mhla_causal_extend(counts=accept)` leaves on a clone of `before` with the accepted rows as the tokens."""
    import mhla_amd
    ref = before.clone()
    ka, va = _accepted(k, v, counts, accept, left_padded)
    if any(accept):
        mhla_amd.mhla_causal_extend(torch.zeros_like(q), ka, va, mix, ref, counts=accept, left_padded=left_padded)
    return ref


def _same_as_extended(state, ref, before, accept):
    assert state.lengths == ref.lengths == tuple(p + a for p, a in zip(before.lengths, accept))
    assert state.seen == max(state.lengths) and not state.stale
    assert torch.equal(state.pos, ref.pos) and state.pos.tolist() == list(state.lengths)
    for b, n in enumerate(state.lengths):
        same_seq_state(f"sequence {b} (accepted {accept[b]})", state, b, ref, b, n)


@pytest.mark.parametrize("left_padded", [False, True], ids=["right-padded", "left-padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_verify_rows_and_the_state_it_leaves(shape, left_padded):
    """The rows are those of `mhla_causal_extend(counts=n)` on a clone, bit for bit, and the oracle's; padding rows are exactly zero;
    `P`, `Cur`, `pos`, `lengths`, `seen` and every finished chunk of `S` are as before."""
    import mhla_amd
    dtype, H, K, V = shape
    hist, q, k, v, mix, want = _batch(dtype, H, K, V, left_padded)
    md = mix.to(DEV)
    poison()
    state = _state(hist, mix)
    before = state.clone()
    o, _ = _verify(q, k, v, md, state, COUNTS, left_padded)
    _verify_left_the_state(state, before)
    o_ext = mhla_amd.mhla_causal_extend(q, k, v, md, before.clone(), counts=COUNTS, left_padded=left_padded)
    assert torch.equal(o, o_ext), f"rows differ from mhla_causal_extend (max {(o.float() - o_ext.float()).abs().max().item():.3e})"
    padding_is_zero(o, COUNTS, left_padded)
    for b, (p, n) in enumerate(DRAFTS):
        if n:
            check(f"sequence {b} (pos {p}, n {n}): rows", o[b:b + 1, window(SPEC_T, n, left_padded)], want[b], CAUSAL_TOL[dtype])


@pytest.mark.parametrize("left_padded", [False, True], ids=["right-padded", "left-padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_commit_is_the_extend_by_the_accepted_prefix(shape, left_padded):
    import mhla_amd
    dtype, H, K, V = shape
    hist, q, k, v, mix, _ = _batch(dtype, H, K, V, left_padded)
    md = mix.to(DEV)
    poison()
    state = _state(hist, mix)
    before = state.clone()
    _, draft = _verify(q, k, v, md, state, COUNTS, left_padded)
    assert mhla_amd.mhla_causal_commit(draft, md, state, torch.tensor(ACCEPT)) is state
    _same_as_extended(state, _extended(q, k, v, md, before, COUNTS, ACCEPT, left_padded), before, ACCEPT)
    tol = TOL[torch.float32]
    for b, (p, n, a) in enumerate(SPEC_TABLE):
        name = f"sequence {b} (pos {p}, n {n}, accepted {a})"
        nfull = (p + a) // 64
        ref = oracle_state(hist[b][1].float(), hist[b][2].float(), mix, p + a, SPEC_CAP)
        for part, got, r in (("S", state.S[b:b + 1, :, :nfull], ref[0][:, :, :nfull]), ("P", state.P[b:b + 1], ref[1]), ("Cur", state.Cur[b:b + 1], ref[2])):
            close_or_zero(f"{name}: {part} vs the oracle", got, r, tol)
        if (p + a) % 64 == 0:
            assert float(state.Cur[b].abs().max()) == 0.0, f"{name}: Cur on a boundary must be exactly 0"
        if p + a == 64 * SPEC_CAP:
            assert float(state.P[b].abs().max()) == 0.0, f"{name}: P of a full state must be exactly 0"
        if not a:
            assert torch.equal(state.P[b], before.P[b]) and torch.equal(state.Cur[b], before.Cur[b]), f"{name}: P or Cur changed"
            assert torch.equal(state.S[b, :, :nfull], before.S[b, :, :nfull]), f"{name}: a finished chunk changed"
    # nothing accepted anywhere: nothing is launched, bit for bit as before
    again = before.clone()
    _, draft = _verify(q, k, v, md, again, COUNTS, left_padded)
    ran = launches(lambda: mhla_amd.mhla_causal_commit(draft, md, again, (0,) * B))
    assert not ran, ran
    _verify_left_the_state(again, before)


def test_scribbles_on_unfinished_rows_are_harmless():
    """Verify, commit less than the draft, two ragged steps, one more extend past every chunk the verify scribbled on: every row is
    the operator's over the sequence that was really taken, and the state that of one prefill of it."""
    import mhla_amd
    dtype, H, K, V, cap, L = torch.bfloat16, 2, 64, 64, 3, 4
    pos0, drafted, accept, last = (60, 0, 37, 64), (10, 70, 27, 70), (2, 3, 0, 64), (3, 64, 30, 10)
    nb, T = len(pos0), 70
    proposed = table_inputs(H, K, V, dtype, table=tuple((0, p + n) for p, n in zip(pos0, drafted)), T=134, L=L, seed=5)
    fresh = table_inputs(H, K, V, dtype, table=tuple((0, 2 + c) for c in last), T=66, L=L, seed=6)[0]
    mix = proposed[4]
    # the sequence really taken: the history, the accepted prefix of the draft, then tokens the draft did not propose
    real = [tuple(torch.cat([pr[:, :p + a], fr], dim=1) for pr, fr in zip(proposed[0][b], fresh[b])) for b, (p, a) in enumerate(zip(pos0, accept))]
    total = [p + a + 2 + c for p, a, c in zip(pos0, accept, last)]
    assert all(r[0].shape[1] == n for r, n in zip(real, total)) and max(total) <= 64 * cap
    want = [orc.causal_fwd(qs.float(), ks.float(), vs.float(), mix) for qs, ks, vs in real]
    want_draft = [orc.causal_fwd(qs.float(), ks.float(), vs.float(), mix) for qs, ks, vs in proposed[0]]
    md = mix.to(DEV)

    def padded(src, at, counts, width, left_padded):
        q, k = (torch.full((nb, width, H, K), NAN, dtype=dtype) for _ in range(2))
        v = torch.full((nb, width, H, V), NAN, dtype=dtype)
        for b, n in enumerate(counts):
            w = window(width, n, left_padded)
            q[b, w], k[b, w], v[b, w] = (src[b][i][0, at[b]:at[b] + n] for i in range(3))
        return q.to(DEV), k.to(DEV), v.to(DEV)

    def rows(o, ref, counts, left_padded, at, what):
        for b, n in enumerate(counts):
            if n:
                check(f"sequence {b}: {what} rows {at[b]} .. {at[b] + n - 1}", o[b:b + 1, window(o.shape[1], n, left_padded)],
                      ref[b][:, at[b]:at[b] + n], CAUSAL_TOL[dtype])

    poison()
    state = _state(proposed[0], mix, cap, tuple((p, 0) for p in pos0))
    qd, kd, vd = padded(proposed[0], pos0, drafted, T, True)
    o, draft = _verify(qd, kd, vd, md, state, drafted, True)
    rows(o, want_draft, drafted, True, pos0, "verified")
    mhla_amd.mhla_causal_commit(draft, md, state, accept)
    assert state.lengths == tuple(p + a for p, a in zip(pos0, accept))
    for _ in range(2):
        at = state.lengths
        rows(mhla_amd.mhla_causal_step(*padded(real, at, (1,) * nb, 1, False), md, state), want, (1,) * nb, False, at, "step")
    at = state.lengths
    o = mhla_amd.mhla_causal_extend(*padded(real, at, last, 64, False), md, state, counts=last)
    rows(o, want, last, False, at, "extend")
    assert state.lengths == tuple(total)
    k_all, v_all = (torch.zeros(nb, max(total), H, d, dtype=dtype) for d in (K, V))
    for b, n in enumerate(total):
        k_all[b, :n], v_all[b, :n] = real[b][1][0], real[b][2][0]
    ref = mhla_amd.mhla_causal_state(k_all.to(DEV), v_all.to(DEV), md, lengths=total, capacity_chunks=cap)
    for b, n in enumerate(total):
        for part, x, y in (("S", state.S[b, :, :n // 64], ref.S[b, :, :n // 64]), ("P", state.P[b], ref.P[b]), ("Cur", state.Cur[b], ref.Cur[b])):
            close_or_zero(f"sequence {b}: {part} vs one prefill of the sequence really taken", x, y.cpu(), TOL[torch.float32])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_epilogue_and_strided_views(dtype):
    """gate, norm_weight and `epilogue` in the chain, q, k, v as strided slices of one packed projection: the bits of the extend
    call; the draft keeps the views, and the commit reads them in place."""
    import mhla_amd
    H, K, V = 2, 64, 128
    left_padded = True
    hist, q, k, v, mix, _ = _batch(dtype, H, K, V, left_padded)
    md = mix.to(DEV)
    gen = torch.Generator().manual_seed(21)
    g = torch.randn(B, SPEC_T, H, V, generator=gen).to(dtype).to(DEV)
    wgt = (torch.rand(V, generator=gen) + 0.5).to(DEV)
    packed = torch.cat([q, k, v], dim=-1).reshape(B, SPEC_T, H * (2 * K + V)).contiguous().view(B, SPEC_T, H, 2 * K + V)
    qv, kv, vv = packed[..., :K], packed[..., K:2 * K], packed[..., 2 * K:]
    assert not kv.is_contiguous() and kv.data_ptr() != packed.data_ptr()
    poison()
    state = _state(hist, mix)
    before = state.clone()
    for kw in (dict(gate=g, norm_weight=wgt, norm_eps=1e-5), dict(norm_weight=wgt), dict(epilogue=True), dict(gate=g, scale=0.37)):
        y, draft = _verify(qv, kv, vv, md, state, COUNTS, left_padded, **kw)
        _verify_left_the_state(state, before)
        y_ext = mhla_amd.mhla_causal_extend(qv, kv, vv, md, before.clone(), counts=COUNTS, left_padded=left_padded, **kw)
        assert torch.equal(y, y_ext), f"{sorted(kw)}: rows differ from mhla_causal_extend"
        padding_is_zero(y, COUNTS, left_padded)
    assert draft.k.data_ptr() == kv.data_ptr() and draft.v.data_ptr() == vv.data_ptr()      # references, not copies
    mhla_amd.mhla_causal_commit(draft, md, state, ACCEPT)
    _same_as_extended(state, _extended(q, k, v, md, before, COUNTS, ACCEPT, left_padded), before, ACCEPT)


def test_launch_counts():
    """A verify makes the launches of the ragged extend for the same inputs; a commit at most four, none of them an output kernel,
    and as many whatever is accepted as long as some sequence closes a chunk."""
    import mhla_amd
    dtype, H, K, V = SHAPES[2]
    hist, q, k, v, mix, _ = _batch(dtype, H, K, V, False)
    md = mix.to(DEV)
    state = _state(hist, mix)
    before = state.clone()
    ext = before.clone()
    ran_ext = launches(lambda: mhla_amd.mhla_causal_extend(q, k, v, md, ext, counts=COUNTS))
    drafts = []
    ran = launches(lambda: drafts.append(_verify(q, k, v, md, state, COUNTS, False)[1]))
    assert ran == ran_ext and sum(ran.values()) == 6 and ran["k_cs_step_finish_ragged"] == 1, (ran, ran_ext)
    counts = {}
    for name, accept in (("table", ACCEPT), ("other", ACCEPT2), ("open", ACCEPT_OPEN)):
        st = before.clone()
        counts[name] = launches(lambda: mhla_amd.mhla_causal_commit(drafts[0], md, st, accept))
        assert not any(n.startswith(("k_cx_out", "k_cs_step")) for n in counts[name]), counts[name]
        assert counts[name]["k_cx_advance"] == 1 and sum(counts[name].values()) <= 4, counts[name]
        _same_as_extended(st, _extended(q, k, v, md, before, COUNTS, accept, False), before, accept)
    assert counts["table"] == counts["other"] and sum(counts["table"].values()) == 4, counts
    assert counts["open"] == {"k_cx_xty_acc_ragged": 1, "k_cx_advance": 1}, counts
    idle = launches(lambda: _verify(q, k, v, md, state, (0,) * B, False))
    assert not idle, idle


def test_two_runs_give_equal_bits():
    import mhla_amd
    dtype, H, K, V = SHAPES[2]
    hist, q, k, v, mix, _ = _batch(dtype, H, K, V, True)
    md = mix.to(DEV)
    s0 = _state(hist, mix)
    runs = []
    for _ in range(2):
        st = s0.clone()
        o, draft = _verify(q, k, v, md, st, COUNTS, True)
        mhla_amd.mhla_causal_commit(draft, md, st, ACCEPT)
        runs.append((o, st))
    (oa, sa), (ob, sb) = runs
    assert sa.S.data_ptr() != sb.S.data_ptr()
    assert torch.equal(oa, ob) and torch.equal(sa.P, sb.P) and torch.equal(sa.Cur, sb.Cur) and torch.equal(sa.pos, sb.pos)
    for b, n in enumerate(sa.lengths):
        assert torch.equal(sa.S[b, :, :n // 64], sb.S[b, :, :n // 64])


def test_large_batches_are_sliced(monkeypatch):
    """A (b, h) range of five batch entries slices verify and commit: the same kernels on every slice, so the same bits."""
    import mhla_amd
    from mhla_amd import ops
    dtype, H, K, V = SHAPES[2]
    hist, q, k, v, mix, _ = _batch(dtype, H, K, V, True)
    md = mix.to(DEV)
    s0 = _state(hist, mix)
    whole = s0.clone()
    o_whole, draft = _verify(q, k, v, md, whole, COUNTS, True)
    mhla_amd.mhla_causal_commit(draft, md, whole, ACCEPT)
    monkeypatch.setattr(ops, "_MAX_GRID_BH", 5 * H)
    sliced = s0.clone()
    got = []
    ran = launches(lambda: got.extend(_verify(q, k, v, md, sliced, COUNTS, True)))
    assert ran["k_cs_step_finish_ragged"] == 3, ran      # slices of 5, 5 and 2 sequences
    assert torch.equal(got[0], o_whole)
    _verify_left_the_state(sliced, s0)
    ran = launches(lambda: mhla_amd.mhla_causal_commit(got[1], md, sliced, ACCEPT))
    assert ran["k_cx_advance"] == 3, ran
    _same_as_extended(sliced, whole, s0, ACCEPT)


def test_refusals_behind_the_device_check_leave_the_state_untouched(monkeypatch):
    import mhla_amd
    from mhla_amd import _lib, ops
    dtype, H, K, V = SHAPES[0]
    hist, q, k, v, mix, _ = _batch(dtype, H, K, V, False)
    md = mix.to(DEV)
    state = ragged_start(DRAFTS, hist, mix, SPEC_CAP)
    keep = state.clone()
    ver = lambda counts, m=md: mhla_amd.mhla_causal_verify(q, k, v, m, state, counts=counts)
    with pytest.raises(IndexError, match=r"sequences \[11\].*the state holds only 4"):
        ver([0] * 11 + [65])                           # sequence 11 is at 192 of 256: the whole draft must fit
    with pytest.raises(IndexError, match=r"mixing_matrix has only 1 rows"):
        ver([1] * B, m=md[:1, :1].contiguous())
    unchanged(state, keep)
    monkeypatch.setattr(ops, "EXTEND_WS_CAP_BYTES", 1)
    with pytest.raises(ValueError, match="EXTEND_WS_CAP_BYTES"):
        ver(COUNTS)
    monkeypatch.undo()
    unchanged(state, keep)
    _, draft = _verify(q, k, v, md, state, COUNTS, False)
    with pytest.raises(ValueError, match="must be in 0"):
        mhla_amd.mhla_causal_commit(draft, md, state, [11] + [0] * (B - 1))
    with pytest.raises(ValueError, match="must be in 0"):
        mhla_amd.mhla_causal_commit(draft, md, state, [-1] + [0] * (B - 1))
    with pytest.raises(ValueError, match="accept has 3 entries"):
        mhla_amd.mhla_causal_commit(draft, md, state, [0, 0, 0])
    with pytest.raises(IndexError, match="mixing_matrix"):
        mhla_amd.mhla_causal_commit(draft, md[:, :1].contiguous(), state, ACCEPT)
    _verify_left_the_state(state, keep)
    moved = keep.clone()
    mhla_amd.mhla_causal_step(q[:, :1].nan_to_num(), k[:, :1].nan_to_num(), v[:, :1].nan_to_num(), md, moved)
    after = moved.clone()
    with pytest.raises(ValueError, match="moved since the verify"):
        mhla_amd.mhla_causal_commit(draft, md, moved, ACCEPT)
    unchanged(moved, after)

    # the raw entry points
    lib = _lib.load()
    state = keep.clone()
    ntok = torch.tensor(COUNTS, dtype=torch.int32, device=DEV)
    acc = torch.tensor(ACCEPT, dtype=torch.int32, device=DEV)
    plan = ops._ragged_plan(state.lengths, COUNTS, SPEC_CAP)
    need = lib.mhla_causal_extend_ragged_ws_bytes(B, SPEC_T, H, K, V, plan[1], _lib.F32)
    ws = torch.empty(need // 4 + 4, dtype=torch.float32, device=DEV)
    out = torch.empty(B, SPEC_T, H, V, device=DEV)
    mixf = md.contiguous()

    def raw_verify(T=SPEC_T, ws_bytes=need, ldmix=mixf.shape[1], max_end=plan[0], pos=state.pos):
        return lib.mhla_causal_verify_ragged(ops._view(q), ops._view(k), ops._view(v), mixf.data_ptr(), ldmix, state.S.data_ptr(), SPEC_CAP,
                                             state.P.data_ptr(), state.Cur.data_ptr(), pos.data_ptr() if pos is not None else None,
                                             ntok.data_ptr(), T, max_end, plan[1], 1, 0, ops._view(out), _lib.NULL_VIEW, None, 1e-5,
                                             _lib.NULL_VIEW, ws.data_ptr(), ws_bytes, B, H, K, V, 64, K ** -0.5, _lib.F32, ops._stream())
    aplan = ops._ragged_plan(state.lengths, ACCEPT, SPEC_CAP)
    cneed = lib.mhla_causal_commit_ragged_ws_bytes(B, _lib.F32)

    def raw_commit(T=SPEC_T, ws_bytes=cneed, ldmix=mixf.shape[1], max_end=aplan[0], max_later=aplan[1], any_close=1, accept=acc):
        return lib.mhla_causal_commit_ragged(ops._view(k), ops._view(v), mixf.data_ptr(), ldmix, state.S.data_ptr(), SPEC_CAP,
                                             state.P.data_ptr(), state.Cur.data_ptr(), state.pos.data_ptr(), ntok.data_ptr(),
                                             accept.data_ptr() if accept is not None else None, T, max_end, max_later, any_close, 0,
                                             ws.data_ptr(), ws_bytes, B, H, K, V, 64, _lib.F32, ops._stream())
    EINVAL = -22
    assert raw_verify(ws_bytes=need - 4) == EINVAL and b"workspace too small" in lib.mhla_last_error()
    assert raw_verify(ldmix=3) == EINVAL and b"ldmix=3 < 4" in lib.mhla_last_error()
    assert raw_verify(T=0) == EINVAL and b"T=0" in lib.mhla_last_error()
    assert raw_verify(max_end=257) == EINVAL and b"max_end=257" in lib.mhla_last_error()
    assert raw_verify(pos=None) == EINVAL and b"pos_dev" in lib.mhla_last_error()
    assert raw_commit(ws_bytes=cneed - 4) == EINVAL and b"workspace too small" in lib.mhla_last_error()
    assert raw_commit(ldmix=3) == EINVAL and b"ldmix=3 < 4" in lib.mhla_last_error()
    assert raw_commit(T=65536) == EINVAL and b"T=65536" in lib.mhla_last_error()
    assert raw_commit(max_end=257) == EINVAL and b"max_end=257" in lib.mhla_last_error()
    assert raw_commit(max_later=1, any_close=0) == EINVAL and b"without any_close" in lib.mhla_last_error()
    assert raw_commit(accept=None) == EINVAL and b"accept_dev" in lib.mhla_last_error()
    unchanged(state, keep)
    # defence: host values that vouch for less than the arrays hold skip those sequences -- state and position untouched
    assert raw_commit(max_end=100, max_later=0, any_close=0) == 0
    torch.cuda.synchronize()
    moved = [b for b in range(B) if state.pos[b].item() != keep.pos[b].item()]
    ok = [b for b, (p, n, a) in enumerate(SPEC_TABLE) if a and p + a <= 100 and p % 64 + a < 64]
    assert moved == ok == [1, 8], (moved, ok)
    for b in range(B):
        if b not in ok:
            assert torch.equal(state.P[b], keep.P[b]) and torch.equal(state.Cur[b], keep.Cur[b]) and torch.equal(state.S[b], keep.S[b])


@pytest.mark.parametrize("opts", [{}, {"use_output_gate": False}], ids=["default", "no-output-gate"])
def test_fla_layer_speculative_then_commit(opts):
    """A speculative call, `cache.commit(accept)`, a normal call: per sequence, that sequence alone fed its accepted tokens and then
    the next call through a cache of its own."""
    from mhla_amd import modules
    m = _fla_layer(**opts).to(DEV).eval()
    prompts, counts, accept, nxt, T, T2 = (70, 20, 64), (3, 70, 5), (2, 66, 0), (4, 1, 4), 70, 4
    x0, x1, x2 = layer_inputs(3, 70, 31).to(DEV), layer_inputs(3, T, 32).to(DEV), layer_inputs(3, T2, 33).to(DEV)
    mask = torch.zeros(3, 70, dtype=torch.long, device=DEV)
    for b, n in enumerate(prompts):
        mask[b, 70 - n:] = 1
    cache = modules.DecodeCache()
    with torch.no_grad():
        m(x0, attention_mask=mask, past_key_values=cache, use_cache=True)
        st = cache[0]["recurrent_state"]
        keep = st.clone()
        y = m(x1, past_key_values=cache, use_cache=True, token_counts=counts, speculative=True)[0]
        assert cache[0]["recurrent_state"] is st and cache[0]["draft"].counts == counts and cache.get_seq_length() == 70
        _verify_left_the_state(st, keep)
        plain = modules.DecodeCache()
        m(x0, attention_mask=mask, past_key_values=plain, use_cache=True)
        check("a verify gives the extend's output", y, m(x1, past_key_values=plain, use_cache=True, token_counts=counts)[0].cpu(), 1e-6)
        cache.commit(accept)
        assert "draft" not in cache[0] and st.lengths == (72, 86, 64) and st.pos.tolist() == [72, 86, 64] and cache.get_seq_length() == 86
        z = m(x2, past_key_values=cache, use_cache=True, token_counts=nxt)[0]
        assert st.lengths == (76, 87, 68) and cache.get_seq_length() == 87
        for b, (p, n, a, c) in enumerate(zip(prompts, counts, accept, nxt)):
            own = modules.DecodeCache()
            m(x0[b:b + 1, 70 - p:], past_key_values=own, use_cache=True)
            if a:
                alone = m(x1[b:b + 1, T - n:T - n + a], past_key_values=own, use_cache=True)[0]
                check(f"sequence {b}: the {a} accepted of {n} drafted tokens at {p}", y[b:b + 1, T - n:T - n + a], alone.cpu(), 1e-4)
            alone = m(x2[b:b + 1, T2 - c:], past_key_values=own, use_cache=True)[0]
            check(f"sequence {b}: {c} tokens after the commit", z[b:b + 1, T2 - c:], alone.cpu(), 1e-4)


def test_fla_layer_speculative_drafts_and_refusals():
    from mhla_amd import modules
    m = _fla_layer().to(DEV).eval()
    x0, x1 = layer_inputs(2, 10, 41).to(DEV), layer_inputs(2, 4, 42).to(DEV)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="empty cache"):
            m(x1, past_key_values=modules.DecodeCache(), use_cache=True, speculative=True)
        dev = modules.DecodeCache(device_positions=True)
        m(x0, past_key_values=dev, use_cache=True)
        with pytest.raises(NotImplementedError, match="device_positions"):
            m(x1[:, :1], past_key_values=dev, use_cache=True, speculative=True)
        conv = _fla_layer(use_short_conv=True).to(DEV).eval()
        cc = modules.DecodeCache()
        conv(x0, past_key_values=cc, use_cache=True)
        with pytest.raises(NotImplementedError, match="use_short_conv"):
            conv(x1, past_key_values=cc, use_cache=True, speculative=True)
        # a uniform cached state becomes ragged on the same storage; without token_counts every sequence drafts the whole call
        cache = modules.DecodeCache()
        m(x0, past_key_values=cache, use_cache=True)
        uniform = cache[0]["recurrent_state"]
        assert uniform.lengths is None
        y = m(x1, past_key_values=cache, use_cache=True, speculative=True)[0]
        st = cache[0]["recurrent_state"]
        assert st.lengths == (10, 10) and st.S.data_ptr() == uniform.S.data_ptr() and cache.get_seq_length() == 10
        first = cache[0]["draft"]
        assert first.counts == (4, 4)
        with pytest.raises(ValueError, match="commit or discard first"):
            m(x1, past_key_values=cache, use_cache=True)
        assert cache[0]["draft"] is first and st.lengths == (10, 10)
        # a new speculative call replaces the pending draft; discard drops it and the plain call gives the verified rows
        m(x1[:, :2], past_key_values=cache, use_cache=True, speculative=True)
        assert cache[0]["draft"] is not first and cache[0]["draft"].counts == (2, 2)
        cache.discard()
        assert "draft" not in cache[0] and st.lengths == (10, 10) and cache.get_seq_length() == 10
        check("the plain call after a discard gives the verified rows", m(x1, past_key_values=cache, use_cache=True)[0], y.cpu(), 1e-4)
        assert st.lengths == (14, 14) and cache.get_seq_length() == 14
        # without exact_decoding the flag is ignored
        loose = modules.MHLA(mode="chunk", hidden_size=256, num_heads=2, feature_map="relu", layer_idx=0).to(DEV).eval()
        check("speculative=True without exact_decoding", loose(x1, speculative=True)[0], loose(x1)[0].cpu(), 1e-6)


# The seed of the GPT host test's model.  The test's condition on the reference -- every emitted token's top-2 logit margin above
# 10 x 1e-4 of max |logit| -- is invariant under a scaling of lm_head, so the SEED is picked for it (the smallest margin over the
# 48 emitted tokens is printed by the test: 1.3e-2 with this seed, among 1e-4 .. 1.3e-2 over seeds 0 .. 23).
GPT_SEED = 14


def test_gpt_host_speculative_generate():
    """Greedy speculative decoding returns the ids of plain greedy decoding whatever the draft proposes, and an all-accepted draft
    takes ceil(24 / 5) verify rounds after the prefill."""
    from mhla_amd.hosts.gpt import GPT_MHLA
    vocab, new, k = 128, 24, 4
    torch.manual_seed(GPT_SEED)
    model = GPT_MHLA(vocab_size=vocab, hidden_size=128, num_layers=2, num_heads=4, max_seq_len=2048, exact_decoding=True).to(DEV).eval()
    gen = torch.Generator().manual_seed(6)
    prompts, T0 = (30, 66), 66
    ids0 = torch.randint(0, vocab, (2, T0), generator=gen).to(DEV)
    mask = torch.zeros(2, T0, dtype=torch.long, device=DEV)
    for b, n in enumerate(prompts):
        mask[b, T0 - n:] = 1
    ref, logits = model.generate(ids0, new, attention_mask=mask, return_logits=True)
    # a condition on the reference alone: no emitted token is a near tie, at ten times what the host tests allow between two paths
    top2 = logits.float().topk(2, dim=-1).values
    margin = ((top2[..., 0] - top2[..., 1]) / logits.float().abs().amax(-1)).min().item()
    print(f"smallest top-2 margin of the reference, relative to max |logit|: {margin:.3e}")
    assert margin > 10 * 1e-4, f"the reference has a near tie ({margin:.3e}): pick another GPT_SEED"
    ref_host = ref.tolist()

    def greedy(hist, corrupt=lambda e, j, t: t):
        rows = []
        for b, h in enumerate(hist):
            assert h.dim() == 1 and torch.equal(h[:prompts[b]], ids0[b, T0 - prompts[b]:]), "histories are the prompts without padding"
            e = h.numel() - prompts[b]                 # tokens emitted so far, the last of them not yet fed
            assert 1 <= e <= new and h[prompts[b]:].tolist() == ref_host[b][:e]
            rows.append([corrupt(e, j, ref_host[b][e + j]) if e + j < new else 0 for j in range(k)])
        return torch.tensor(rows)

    rng = torch.Generator().manual_seed(7)
    drafts = {"greedy": greedy,
              "random": lambda hist: torch.randint(0, vocab, (2, k), generator=rng),
              "every-third-corrupted": lambda hist: greedy(hist, lambda e, j, t: (t + 1) % vocab if (e + j) % 3 == 2 else t)}
    calls = {}
    forward = model.forward
    for name, fn in drafts.items():
        n_calls = [0]

        def counting(*a, **kw):
            n_calls[0] += 1
            return forward(*a, **kw)
        model.forward = counting
        try:
            ids = model.generate(ids0, new, attention_mask=mask, draft=fn, draft_len=k)
        finally:
            del model.forward
        calls[name] = n_calls[0]
        assert ids.shape == (2, new) and ids.tolist() == ref_host, f"{name} draft: ids differ from plain greedy decoding"
    print(f"model calls per draft: {calls}")
    assert calls["greedy"] == -(-new // (k + 1)) + 1 == 6, calls
    assert calls["greedy"] < calls["every-third-corrupted"] <= new and calls["greedy"] < calls["random"] <= new, calls
    ids, kept = model.generate(ids0, new, attention_mask=mask, draft=greedy, draft_len=k, return_logits=True)
    assert ids.tolist() == ref_host
    check("logits every speculative id was picked from", kept, logits.cpu(), 1e-4)
    with pytest.raises(NotImplementedError, match="graph=True"):
        model.generate(ids0, new, attention_mask=mask, draft=greedy, draft_len=k, graph=True)
