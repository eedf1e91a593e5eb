"""GPU parity: the prefill of a PACK of prompts (cu_seqlens) into one ragged decode state -- mhla_causal_varlen_state_init through
mhla_causal_state / mhla_causal_prefill(cu_seqlens=), the fla layer on DecodeCache(packed_prefill=True) and the GPT host.  Every
sequence must come out exactly as if it had been prefilled alone: the state bit for bit that of mhla_causal_state over the
sequence's own tokens, rows and later steps within the operator's tolerances of orc.causal_fwd per sequence."""
import functools

import pytest
import torch

from decode_util import check_state, check_step_rows, ragged_steps, signed_features
from gpu_util import DEV, CAUSAL_TOL, check, launches, poison, _fla_layer
from oracle import mhla_oracle as orc

pytestmark = pytest.mark.gpu

# one token, 64 + 1, empty, exactly one chunk, three chunks with a tail, and one that fills the capacity of 3 chunks
PACK, CAP, L = (1, 65, 0, 64, 191, 192), 3, 4
CASES = [(torch.float32, 2, 20, 24),      # K no multiple of 16, V no multiple of 64: both strip tails
         (torch.bfloat16, 2, 128, 256),   # the C5 head: 2 x 4 strips
         (torch.float16, 1, 64, 64)]
IDS = ["fp32-20x24", "bf16-128x256", "fp16-64x64"]


def _cu(lengths):
    cu = [0]
    for m in lengths:
        cu.append(cu[-1] + m)
    return cu


def _pack(x, lengths):
    """[1, sum(lengths), ...]: the first lengths[b] rows of every x[b], one after the other."""
    return torch.cat([x[b, :m] for b, m in enumerate(lengths)], dim=0).unsqueeze(0)


@functools.lru_cache(maxsize=None)
def _seqs(lengths, n, H, K, V, rows, dtype, seed=1234):
    """As decode_util.ragged_inputs makes them -- B sequences on timelines of their own, rows [0, lengths[b] + n] of q[b],
    k[b], v[b], q and k with signs as roped feature maps have them, a random lower-triangular mix -- and the fp32 oracle of every
    sequence alone over its lengths[b] + n tokens (None for no token at all), computed once per case."""
    B, T = len(lengths), max(lengths) + n + 1
    g = torch.Generator().manual_seed(seed)
    q = signed_features(g, B, T, H, K).to(dtype)
    k = signed_features(g, B, T, H, K).to(dtype)
    v = torch.randn(B, T, H, V, generator=g).to(dtype)
    mix = torch.tril(torch.rand(rows, rows, generator=g).clamp(1e-5, 1))
    want = tuple(orc.causal_fwd(q[b:b + 1, :m + n].float(), k[b:b + 1, :m + n].float(), v[b:b + 1, :m + n].float(), mix) if m + n else None
                 for b, m in enumerate(lengths))
    return q, k, v, mix, want


def _case(dtype, H, K, V, lengths=PACK, n=0, rows=L):
    q, k, v, mix, want = _seqs(lengths, n, H, K, V, rows, dtype)
    return tuple(t.to(DEV) for t in (q, k, v, mix)) + (want,)


def _alone(k, v, mix, lengths, cap):
    import mhla_amd
    return [mhla_amd.mhla_causal_state(k[b:b + 1, :m], v[b:b + 1, :m], mix, capacity_chunks=cap) for b, m in enumerate(lengths)]


def _same_bits(name, state, alone, lengths):
    for b, m in enumerate(lengths):
        nfull = m // 64
        a = alone[b]
        assert torch.equal(state.S[b:b + 1, :, :nfull], a.S[:, :, :nfull]), f"{name}: S of sequence {b} ({m} tokens)"
        assert torch.equal(state.P[b:b + 1], a.P), f"{name}: P of sequence {b} ({m} tokens)"
        assert torch.equal(state.Cur[b:b + 1], a.Cur), f"{name}: Cur of sequence {b} ({m} tokens)"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_state_bits_are_those_of_every_sequence_alone(case):
    import mhla_amd
    dtype, H, K, V = case
    q, k, v, mix, _ = _case(*case)
    kp, vp = _pack(k, PACK), _pack(v, PACK)
    alone = _alone(k, v, mix, PACK, CAP)
    poison()
    state = mhla_amd.mhla_causal_state(kp, vp, mix, cu_seqlens=_cu(PACK), capacity_chunks=CAP)
    assert state.lengths == PACK and state.seen == 192 and state.pos.tolist() == list(PACK) and state.pos.dtype == torch.int32
    assert state.capacity_chunks == CAP and state.S.shape == (6, H, CAP, K, V) and state.P.shape == state.Cur.shape == (6, H, K, V)
    assert state.S.dtype == state.P.dtype == state.Cur.dtype == torch.float32
    _same_bits("pack", state, alone, PACK)
    zero = lambda t: float(t.abs().max()) == 0.0
    assert zero(state.S[2]) and zero(state.P[2]) and zero(state.Cur[2])                  # the empty sequence
    assert zero(state.P[5]) and zero(state.Cur[5]) and not zero(state.S[5, :, 2])        # 192 tokens: the state is full
    assert zero(state.Cur[3]) and not zero(state.P[3]) and not zero(state.S[3, :, 0])    # 64 tokens: Cur = 0, the boundary P
    assert zero(state.P[0]) and not zero(state.Cur[0])                                   # one token: no finished chunk
    assert bool(torch.isfinite(state.P).all()) and bool(torch.isfinite(state.Cur).all())
    # a tensor and a plan give the same state as the list
    for cu in (torch.tensor(_cu(PACK), dtype=torch.int32, device=DEV), mhla_amd.causal_varlen_plan(_cu(PACK), DEV)):
        again = mhla_amd.mhla_causal_state(kp, vp, mix, cu_seqlens=cu, capacity_chunks=CAP)
        assert again.lengths == PACK and torch.equal(again.P, state.P) and torch.equal(again.Cur, state.Cur) and torch.equal(again.S, state.S)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_state_against_the_oracle(case):
    import mhla_amd
    q, k, v, mix, _ = _case(*case)
    poison()
    state = mhla_amd.mhla_causal_state(_pack(k, PACK), _pack(v, PACK), mix, cu_seqlens=_cu(PACK), capacity_chunks=CAP)
    for b, m in enumerate(PACK):
        check_state(state, q, k, v, mix, f"seq {b} after the packed prefill({m})", b, m)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_strided_views_of_one_buffer(case):
    import mhla_amd
    dtype, H, K, V = case
    q, k, v, mix, _ = _case(*case)
    kp, vp = _pack(k, PACK), _pack(v, PACK)
    fused = torch.cat([kp, vp], dim=-1).contiguous()
    kv, vv = fused[..., :K], fused[..., K:]
    assert not kv.is_contiguous() and not vv.is_contiguous() and vv.data_ptr() != fused.data_ptr()
    want = mhla_amd.mhla_causal_state(kp, vp, mix, cu_seqlens=_cu(PACK), capacity_chunks=CAP)
    poison()
    got = mhla_amd.mhla_causal_state(kv, vv, mix, cu_seqlens=_cu(PACK), capacity_chunks=CAP)
    assert torch.equal(got.S, want.S) and torch.equal(got.P, want.P) and torch.equal(got.Cur, want.Cur)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_two_runs_give_equal_bits(case):
    import mhla_amd
    q, k, v, mix, _ = _case(*case)
    kp, vp = _pack(k, PACK), _pack(v, PACK)
    plan = mhla_amd.causal_varlen_plan(_cu(PACK), DEV)
    a = mhla_amd.mhla_causal_state(kp, vp, mix, cu_seqlens=plan, capacity_chunks=CAP)
    poison()
    b = mhla_amd.mhla_causal_state(kp, vp, mix, cu_seqlens=plan, capacity_chunks=CAP)
    assert torch.equal(a.S, b.S) and torch.equal(a.P, b.P) and torch.equal(a.Cur, b.Cur) and a.pos.tolist() == b.pos.tolist()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_prefill_rows_and_70_steps(case):
    """The pack without the sequence that fills the state, then 70 steps: every sequence at a position of its own, rolling at a step
    of its own (1: step 63; 65: step 63; 0: step 64; 64: step 64; 191: steps 1 and 65).  191 + 70 tokens are five chunks, so the
    matrix has five rows here and the capacity is its default, the rows of the matrix."""
    import mhla_amd
    dtype, H, K, V = case
    lengths, n, rows = PACK[:5], 70, 5
    q, k, v, mix, want = _case(dtype, H, K, V, lengths, n, rows)
    qp, kp, vp = (_pack(t, lengths) for t in (q, k, v))
    cu = _cu(lengths)
    parts = [mhla_amd.mhla_causal_prefill(q[b:b + 1, :m], k[b:b + 1, :m], v[b:b + 1, :m], mix) for b, m in enumerate(lengths)]
    cat = mhla_amd.CausalState.cat([s for _, s in parts])
    poison()
    o, state = mhla_amd.mhla_causal_prefill(qp, kp, vp, mix, cu_seqlens=cu)
    assert o.shape == (1, cu[-1], H, V) and o.dtype == dtype
    assert state.lengths == lengths and state.seen == 191 and state.capacity_chunks == rows and state.pos.tolist() == list(lengths)
    _same_bits("prefill", state, [s for _, s in parts], lengths)
    for b, m in enumerate(lengths):
        if m:
            check(f"seq {b}: prefill rows", o[:, cu[b]:cu[b + 1]], want[b][:, :m], CAUSAL_TOL[dtype])
    o1 = ragged_steps(q, k, v, mix, state, lengths, 0, n)
    o2 = ragged_steps(q, k, v, mix, cat, lengths, 0, n)
    assert state.lengths == tuple(m + n for m in lengths) and state.pos.tolist() == list(state.lengths)
    for b, m in enumerate(lengths):
        check_step_rows(f"seq {b}: step rows", o1[b:b + 1], want[b], m, dtype)
    assert torch.equal(o1, o2), "steps on the packed state differ from the steps on CausalState.cat of the prefills alone"
    assert torch.equal(state.P, cat.P) and torch.equal(state.Cur, cat.Cur)
    for b, m in enumerate(lengths):
        nfull = (m + n) // 64
        assert torch.equal(state.S[b, :, :nfull], cat.S[b, :, :nfull])


def test_launches_do_not_grow_with_the_sequences():
    import mhla_amd
    dtype, H, K, V = CASES[1]
    q, k, v, mix, _ = _case(*CASES[1])
    count = lambda fn: sum(launches(fn).values())
    two = (65, 191)
    k2, v2 = _pack(k[[1, 4]], two), _pack(v[[1, 4]], two)
    p2, p6 = mhla_amd.causal_varlen_plan(_cu(two), DEV), mhla_amd.causal_varlen_plan(_cu(PACK), DEV)
    kp, vp = _pack(k, PACK), _pack(v, PACK)
    n2 = count(lambda: mhla_amd.mhla_causal_state(k2, v2, mix, cu_seqlens=p2, capacity_chunks=CAP))
    n6 = count(lambda: mhla_amd.mhla_causal_state(kp, vp, mix, cu_seqlens=p6, capacity_chunks=CAP))
    each2 = count(lambda: _alone(k[[1, 4]], v[[1, 4]], mix, two, CAP))
    each6 = count(lambda: _alone(k, v, mix, PACK, CAP))
    print(f"launches: pack of 2: {n2}, pack of 6: {n6}; one call per sequence: {each2}, {each6}")
    assert 0 < n2 == n6 <= 3
    assert n2 < each2 and n6 < each6


def _alone_layer_rows(m, x, n_prompt, n_steps):
    """The layer on one sequence alone (B = 1, no mask, a cache of its own): the prompt's rows and the rows of the steps after it."""
    from mhla_amd import modules
    cache = modules.DecodeCache()
    outs = [m(x[:, :n_prompt], past_key_values=cache, use_cache=True)[0]] if n_prompt else []
    outs += [m(x[:, n_prompt + t:n_prompt + t + 1], past_key_values=cache, use_cache=True)[0] for t in range(n_steps)]
    return torch.cat(outs, dim=1), cache[0]["recurrent_state"]


# fp32: the bound test_fla_layer_left_padded_prefill_and_ragged_steps holds the layer to.  bf16, two bf16 computations of the same
# rows against each other: each side's fused norm x gate y is within 3u + 1e-3 of the exact one (the bound of test_fused_normgate and
# test_layer_bf16_takes_the_fused_varlen_node for that quantity, u = 2^-8), and the output projection rounds once on each side
U16 = 2.0 ** -8
LAYER_TOL = {torch.float32: 1e-4, torch.bfloat16: 2 * (3 * U16 + 1e-3) + 2 * U16}


@pytest.mark.parametrize("dtype,dev", [(torch.float32, False), (torch.float32, True), (torch.bfloat16, False)],
                         ids=["fp32", "fp32-device-positions", "bf16-fused"])
def test_fla_layer_packed_prefill_and_steps(dtype, dev):
    """Prompts of 140, 103, 0 and 64 tokens, once as cu_seqlens and once left-padded with attention_mask, then 5 one-token calls:
    every sequence's rows are those of the layer on that sequence alone."""
    import mhla_amd
    from mhla_amd import modules
    lens, n = (140, 103, 0, 64), 5
    m = _fla_layer(isolate_sequences=True).to(DEV).to(dtype).eval()
    assert m.fuse_norm_and_gate
    xs = [torch.randn(1, p + n, 256, generator=torch.Generator().manual_seed(21 + b)).to(dtype).to(DEV) for b, p in enumerate(lens)]
    T0, cu = max(lens), _cu(lens)
    packed = torch.cat([x[:, :p] for x, p in zip(xs, lens)], dim=1)
    padded = torch.full((4, T0, 256), float("nan"), dtype=dtype, device=DEV)   # (padding rows are never to reach a real row)
    mask = torch.zeros(4, T0, dtype=torch.long, device=DEV)
    for b, p in enumerate(lens):
        if p:
            padded[b, T0 - p:], mask[b, T0 - p:] = xs[b][0, :p], 1
    steps = torch.cat([x[:, p:] for x, p in zip(xs, lens)])
    tol = LAYER_TOL[dtype]
    with torch.no_grad():
        alone = [_alone_layer_rows(m, x, p, n) for x, p in zip(xs, lens)]
        for how in ("cu_seqlens", "attention_mask"):
            cache = modules.DecodeCache(packed_prefill=True, device_positions=dev)
            poison()
            if how == "cu_seqlens":
                o0, attn, c = m(packed, cu_seqlens=torch.tensor(cu, dtype=torch.int32, device=DEV), past_key_values=cache, use_cache=True)
                assert o0.shape == (1, cu[-1], 256)
                rows0 = [o0[:, cu[b]:cu[b + 1]] for b in range(4)]
            else:
                o0, attn, c = m(padded, attention_mask=mask, past_key_values=cache, use_cache=True)
                assert o0.shape == (4, T0, 256)
                assert all(float(o0[b, :T0 - p].abs().max()) == 0.0 for b, p in enumerate(lens) if p < T0), "padding rows are not zero"
                rows0 = [o0[b:b + 1, T0 - p:] for b, p in enumerate(lens)]
            assert attn is None and c is cache and cache.get_seq_length(0) == T0
            st = cache[0]["recurrent_state"]
            assert isinstance(st, mhla_amd.CausalState) and st.lengths == lens and st.pos.tolist() == list(lens)
            assert st.S.shape == (4, 2, 32, 64, 128)
            o1 = torch.cat([m(steps[:, t:t + 1], past_key_values=cache, use_cache=True)[0] for t in range(n)], dim=1)
            if dev:
                cache.sync()
            for b, p in enumerate(lens):
                check(f"{how} seq {b}: o (prefill + steps)", torch.cat([rows0[b], o1[b:b + 1]], dim=1), alone[b][0].float().cpu(), tol)
            assert st.lengths == tuple(p + n for p in lens) == tuple(a[1].seen for a in alone) and st.pos.tolist() == list(st.lengths)
            assert cache.get_seq_length(0) == T0 + n


def test_gpt_host_generates_from_a_packed_prefill():
    """generate on a model with exact_decoding and isolate_sequences prefills the left-padded prompts as a pack.  The comparison is
    built as test_gpt_host_left_padded_prompts builds it -- teacher-forced on generate's own tokens, so that a near-tie cannot send
    two runs down different continuations: the cached logits of the batch against one plain forward of every sequence alone, and
    generate's ids are the argmax of the cached logits.  Per-prompt generate must then return the same ids wherever the logits it
    picks from separate the best two tokens by more than twice that tolerance."""
    from mhla_amd.hosts.gpt import GPT_MHLA
    from mhla_amd.modules import DecodeCache
    torch.manual_seed(5)
    model = GPT_MHLA(vocab_size=512, hidden_size=128, num_layers=2, num_heads=4, exact_decoding=True, isolate_sequences=True).to(DEV).eval()
    lens, T0, n = (70, 7, 64), 70, 8
    gen = torch.Generator().manual_seed(6)
    prompts = [torch.randint(0, 512, (m,), generator=gen) for m in lens]
    padded, mask = torch.zeros(3, T0, dtype=torch.long), torch.zeros(3, T0, dtype=torch.long)
    for b, p in enumerate(prompts):
        padded[b, T0 - len(p):], mask[b, T0 - len(p):] = p, 1
    padded, mask = padded.to(DEV), mask.to(DEV)
    poison()
    new = model.generate(padded, n, attention_mask=mask)
    assert new.shape == (3, n) and new.dtype == torch.long
    with torch.no_grad():
        cache = DecodeCache(packed_prefill=True)
        steps = [model(padded, cache=cache, attention_mask=mask)] + [model(new[:, t:t + 1], cache=cache) for t in range(n)]
        cached = torch.cat(steps, dim=1)   # [3, T0 + n]: row T0 - 1 + t holds the logits after t new tokens
        st = cache[0]["recurrent_state"]
        assert st.lengths == tuple(m + n for m in lens) and st.pos.tolist() == list(st.lengths)
        for b, m in enumerate(lens):
            ids = torch.cat([prompts[b].to(DEV), new[b]])[None]
            full = model(ids)   # the sequence alone, one plain forward
            check(f"seq {b}: logits, packed prefill({m}) + {n} cached steps vs one forward alone", cached[b:b + 1, T0 - m:], full.cpu(), 1e-4)
            own, logits = model.generate(prompts[b][None].to(DEV), n, return_logits=True)
            top = logits[0].float().topk(2, dim=-1).values
            clear = (top[:, 0] - top[:, 1]) > 2e-4 * logits.float().abs().max()
            upto = n if bool(clear.all()) else int((~clear).nonzero()[0])   # (the ids are compared up to the first near-tie)
            assert torch.equal(own[0, :upto], new[b, :upto]), f"seq {b}: generate alone {own[0].tolist()} != in the batch {new[b].tolist()}"
        # the pack as cu_seqlens on an empty cache: the same prefill; on the cache that now holds a state it is refused
        pack_ids = torch.cat([p.to(DEV) for p in prompts])[None]
        cu = torch.tensor(_cu(lens), dtype=torch.int32, device=DEV)
        c2 = DecodeCache(packed_prefill=True)
        logits = model(pack_ids, cache=c2, cu_seqlens=cu)
        assert logits.shape == (1, sum(lens), 512) and c2[0]["recurrent_state"].lengths == lens
        off = 0
        for b, m in enumerate(lens):
            check(f"seq {b}: packed logits", logits[:, off:off + m], cached[b:b + 1, T0 - m:T0].float().cpu(), 1e-4)
            off += m
        with pytest.raises(NotImplementedError, match="cu_seqlens with a cache"):
            model(pack_ids, cache=c2, cu_seqlens=cu)
        with pytest.raises(NotImplementedError, match="cu_seqlens with a cache"):
            model(pack_ids, cache=cache, cu_seqlens=cu)
    assert torch.equal(new, cached[:, T0 - 1:T0 - 1 + n].argmax(-1))
