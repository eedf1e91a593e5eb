"""GPU parity: decoding a RAGGED batch -- a `CausalState` with one length per sequence (`lengths=`, `CausalState.cat`), the ragged
step kernels, extend on a ragged state, the fla layer's left-padded prefill and the GPT host's `attention_mask`.  Sequence b must
behave exactly as if it lived alone in a batch of one, so the reference is `orc.causal_fwd` (resp. the layer / the host's full
forward) per sequence, on that sequence's own tokens."""
import pytest
import torch

from decode_util import check_state, check_step_rows, packed_views, ragged_inputs, ragged_prefill, ragged_steps, window_rows
from gpu_util import DEV, CAUSAL_TOL, check, poison, _fla_layer
from oracle import mhla_oracle as orc

pytestmark = pytest.mark.gpu


def _run_rows(dtype, H, K, V, lengths, n, L, cap, how, state_checks=True):
    q, k, v, mix, want = ragged_inputs(lengths, n, H, K, V, L, dtype)
    q, k, v, mix = (t.to(DEV) for t in (q, k, v, mix))
    poison()
    o0, state = ragged_prefill(q, k, v, mix, lengths, how, cap)
    assert state.lengths == tuple(lengths) and state.seen == max(lengths) and state.pos.tolist() == list(lengths)
    assert state.capacity_chunks == (cap or L)
    for b, m in enumerate(lengths):
        if m:
            check(f"seq {b}: prefill rows", o0[b], want[b][:, :m], CAUSAL_TOL[dtype])
        if state_checks:
            check_state(state, q, k, v, mix, f"seq {b} after prefill({m})", b, m)
    o1 = ragged_steps(q, k, v, mix, state, lengths, 0, n)
    assert o1.dtype == dtype and o1.shape == (len(lengths), n, H, V)
    assert state.lengths == tuple(m + n for m in lengths) and state.seen == max(lengths) + n
    assert state.pos.tolist() == list(state.lengths)
    for b, m in enumerate(lengths):
        check_step_rows(f"seq {b}: step rows", o1[b:b + 1], want[b], m, dtype)
        if state_checks:
            check_state(state, q, k, v, mix, f"seq {b} after {n} steps", b, m + n)
    return state


@pytest.mark.parametrize("how", ["left_padded", "cat"])
def test_rows_three_positions_at_once(how):
    """fp32, K no multiple of 16, V no multiple of 64: sequence 1 rolls on its first step, sequence 2 at step 62, sequence 0 at step
    64 -- in the same launches, with three different diagonal entries of mix live at once."""
    _run_rows(torch.float32, 2, 20, 24, (0, 63, 130), 70, 5, 4, how)


@pytest.mark.parametrize("case", [
    (torch.bfloat16, 2, 128, 256, (120, 60), 80),   # C5 head: the K split is active, two rolls
    (torch.float16, 1, 64, 64, (100, 64), 30),      # one sequence starts on a boundary with Cur = 0
], ids=["bf16-ksplit", "fp16-boundary-start"])
def test_dtypes_and_k_split(case):
    dtype, H, K, V, lengths, n = case
    _run_rows(dtype, H, K, V, lengths, n, (max(lengths) + n + 63) // 64 + 1, None, "left_padded")


def test_equal_lengths_give_the_uniform_bits():
    import mhla_amd
    dtype, H, K, V, T0, n = torch.bfloat16, 2, 64, 128, 60, 10
    q, k, v, mix, _ = ragged_inputs((T0, T0), n, H, K, V, 3, dtype)
    q, k, v, mix = (t.to(DEV) for t in (q, k, v, mix))
    rag = mhla_amd.mhla_causal_state(k[:, :T0], v[:, :T0], mix, lengths=[T0, T0])
    uni = mhla_amd.mhla_causal_state(k[:, :T0], v[:, :T0], mix)
    assert rag.lengths == (T0, T0) and uni.lengths is None and uni.pos is None
    for t in range(T0, T0 + n):   # (step 4 closes the chunk)
        a = mhla_amd.mhla_causal_step(q[:, t:t + 1], k[:, t:t + 1], v[:, t:t + 1], mix, rag)
        b = mhla_amd.mhla_causal_step(q[:, t:t + 1], k[:, t:t + 1], v[:, t:t + 1], mix, uni)
        assert torch.equal(a, b), f"step {t}: outputs differ"
        assert torch.equal(rag.S, uni.S) and torch.equal(rag.P, uni.P) and torch.equal(rag.Cur, uni.Cur), f"step {t}: states differ"
    assert rag.lengths == (T0 + n, T0 + n) and uni.seen == rag.seen == T0 + n and rag.pos.tolist() == [T0 + n] * 2
    assert float(rag.S[:, :, 0].abs().max()) > 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_epilogue_and_strided_views(dtype):
    """The fused norm x gate epilogue on a ragged state, q, k, v read in place as slices of one packed projection: sequence 0 closes
    its chunk at the fourth step, sequence 1 is in its first chunk."""
    H, K, V, lengths, n = 2, 64, 128, (60, 5), 6
    q, k, v, mix, want = ragged_inputs(lengths, n, H, K, V, 3, dtype)
    gen = torch.Generator().manual_seed(7)
    g = torch.randn(2, n, H, V, generator=gen).to(dtype)
    w = torch.rand(V, generator=gen) + 0.5
    eps = 1e-5
    qd, kd, vd, md = (t.to(DEV) for t in (q, k, v, mix))
    poison()
    _, state = ragged_prefill(qd, kd, vd, md, lengths, "left_padded")
    y = ragged_steps(qd, kd, vd, md, state, lengths, 0, n, views=packed_views, gate=g.to(DEV), norm_weight=w.to(DEV), norm_eps=eps)
    assert y.dtype == dtype and state.lengths == (66, 11)
    for b, m in enumerate(lengths):
        y_ref = orc.rms_norm_swish_gate(want[b][:, m:], g[b:b + 1].float(), w, eps)
        check(f"seq {b}: y", y[b:b + 1], y_ref, CAUSAL_TOL[dtype])


def test_full_state_and_refusal():
    """cap = 2: the step that closes sequence 0's LAST chunk leaves its P zero (decided per sequence) while sequence 1 steps on; the
    step after that would open chunk 2 of sequence 0 and is refused before anything is launched."""
    import mhla_amd
    dtype, H, K, V, lengths = torch.float32, 2, 16, 24, (127, 30)
    q, k, v, mix, want = ragged_inputs(lengths, 1, H, K, V, 2, dtype)
    q, k, v, mix = (t.to(DEV) for t in (q, k, v, mix))
    state = _run_rows(dtype, H, K, V, lengths, 1, 2, None, "left_padded")   # (checks rows and, per sequence, S, P, Cur)
    assert state.capacity_chunks == 2 and state.lengths == (128, 31)
    assert float(state.P[0].abs().max()) == 0.0 and float(state.Cur[0].abs().max()) == 0.0 and float(state.P[1].abs().max()) == 0.0
    assert float(state.Cur[1].abs().max()) > 0
    keep = state.clone()
    qs, ks, vs = (window_rows(t, lengths, 1, 1) for t in (q, k, v))
    with pytest.raises(IndexError, match="needs 3 chunks"):
        mhla_amd.mhla_causal_step(qs, ks, vs, mix, state)
    with pytest.raises(IndexError, match="needs 3 chunks"):
        mhla_amd.mhla_causal_extend(torch.cat([qs, qs], 1), torch.cat([ks, ks], 1), torch.cat([vs, vs], 1), mix, state)
    torch.cuda.synchronize()
    assert state.lengths == keep.lengths == (128, 31) and state.seen == 128 and state.pos.tolist() == [128, 31]
    assert all(torch.equal(a, b) for a, b in ((state.S, keep.S), (state.P, keep.P), (state.Cur, keep.Cur)))


def test_extend_on_a_ragged_state():
    import mhla_amd
    dtype, H, K, V, lengths, T, n = torch.float32, 2, 32, 64, (10, 70), 130, 5
    q, k, v, mix, want = ragged_inputs(lengths, T + n, H, K, V, 5, dtype)
    q, k, v, mix = (t.to(DEV) for t in (q, k, v, mix))
    poison()
    _, state = ragged_prefill(q, k, v, mix, lengths, "left_padded")
    o = mhla_amd.mhla_causal_extend(*(window_rows(t, lengths, 0, T) for t in (q, k, v)), mix, state)
    assert o.shape == (2, T, H, V) and state.lengths == (140, 200) and state.seen == 200 and state.pos.tolist() == [140, 200]
    for b, m in enumerate(lengths):
        check_step_rows(f"seq {b}: extend rows", o[b:b + 1], want[b][:, :m + T], m, dtype)
        check_state(state, q, k, v, mix, f"seq {b} after extend({T})", b, m + T)
    o1 = ragged_steps(q, k, v, mix, state, lengths, T, n)
    for b, m in enumerate(lengths):
        check_step_rows(f"seq {b}: step rows after extend", o1[b:b + 1], want[b], m + T, dtype)
    assert state.pos.tolist() == list(state.lengths) == [145, 205]


@pytest.mark.parametrize("opts", [{}, {"num_kv_heads": 1}], ids=["default", "gqa"])
def test_fla_layer_left_padded_prefill_and_ragged_steps(opts):
    import mhla_amd
    from mhla_amd import modules
    m = _fla_layer(**opts)
    pads, T0, n = (0, 37), 100, 40
    # sequence b alone: T0 - pads[b] prompt tokens, then n decoded ones
    xs = [torch.randn(1, T0 - p + n, 256, generator=torch.Generator().manual_seed(11 + b)) for b, p in enumerate(pads)]
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    want = [orc.fla_layer_forward(sd, x, 2, 64, 128, norm_eps=1e-6, **opts) for x in xs]
    m = m.to(DEV).eval()
    prompt = torch.full((2, T0, 256), float("nan"))   # (padding rows are never to reach a real row)
    mask = torch.zeros(2, T0, dtype=torch.long)
    for b, p in enumerate(pads):
        prompt[b, p:], mask[b, p:] = xs[b][0, :T0 - p], 1
    steps = torch.cat([x[:, -n:] for x in xs]).to(DEV)
    cache = modules.DecodeCache()
    with torch.no_grad():
        right = torch.flip(mask, dims=[1])
        with pytest.raises(NotImplementedError):
            m(prompt.to(DEV), attention_mask=right.to(DEV), past_key_values=modules.DecodeCache(), use_cache=True)
        o0, attn, c = m(prompt.to(DEV), attention_mask=mask.to(DEV), past_key_values=cache, use_cache=True)
        assert attn is None and c is cache and o0.shape == (2, T0, 256)
        st = cache[0]["recurrent_state"]
        assert isinstance(st, mhla_amd.CausalState) and st.lengths == (100, 63) and st.S.shape == (2, 2, 32, 64, 128)
        outs = [m(steps[:, t:t + 1], past_key_values=cache, use_cache=True)[0] for t in range(n)]
    o1 = torch.cat(outs, dim=1)
    assert float(o0[1, :37].abs().max()) == 0.0, "padding rows of the prefill output are not zero"
    for b, p in enumerate(pads):
        check(f"seq {b}: o (prefill + steps)", torch.cat([o0[b:b + 1, p:], o1[b:b + 1]], dim=1), want[b], 1e-4)
    assert st.lengths == (140, 103) and st.pos.tolist() == [140, 103]


def test_gpt_host_left_padded_prompts():
    from mhla_amd.hosts.gpt import GPT_MHLA
    from mhla_amd.modules import DecodeCache
    torch.manual_seed(5)
    model = GPT_MHLA(vocab_size=512, hidden_size=128, num_layers=2, num_heads=4, exact_decoding=True).to(DEV).eval()
    lens, T0, n = (20, 7, 63), 63, 60
    gen = torch.Generator().manual_seed(6)
    prompts = [torch.randint(0, 512, (m,), generator=gen) for m in lens]
    padded, mask = torch.zeros(3, T0, dtype=torch.long), torch.zeros(3, T0, dtype=torch.long)
    for b, p in enumerate(prompts):
        padded[b, T0 - len(p):], mask[b, T0 - len(p):] = p, 1
    padded, mask = padded.to(DEV), mask.to(DEV)
    new = model.generate(padded, n, attention_mask=mask)
    assert new.shape == (3, n) and new.dtype == torch.long
    # teacher-forced on generate's own tokens: prefill of the padded prompts, then n cached steps of the whole batch
    with torch.no_grad():
        cache = DecodeCache()
        steps = [model(padded, cache=cache, attention_mask=mask)] + [model(new[:, t:t + 1], cache=cache) for t in range(n)]
        cached = torch.cat(steps, dim=1)   # [3, T0 + n]: row T0 - 1 + t holds the logits after t new tokens
        st = cache[0]["recurrent_state"]
        assert st.lengths == tuple(m + n for m in lens) and st.pos.tolist() == list(st.lengths)
        for b, m in enumerate(lens):
            ids = torch.cat([prompts[b].to(DEV), new[b]])[None]
            full = model(ids)   # the sequence alone, one plain forward
            check(f"seq {b}: logits, padded prefill({m}) + {n} cached steps vs one forward alone", cached[b:b + 1, T0 - m:], full.cpu(), 1e-4)
    assert torch.equal(new, cached[:, T0 - 1:T0 - 1 + n].argmax(-1))
