"""GPU parity: the device-positioned decode step (`mhla_causal_step_dev`) -- a launch chain that depends on no host position, so
that a captured graph can replay it token after token.  Live sequences must give the bits of the ragged step and the rows of the
oracle over each sequence alone; a sequence at the capacity is frozen (zero rows, state untouched, `full` set); the fused q / k
prologue must leave the state `featmap_rotary` + `mhla_causal_step` leave; a replayed graph must give the eager bits; and the fla
layer (`DecodeCache(device_positions=True)`) and the GPT host (`generate(graph=True)`) must decode as their eager paths do.

Bit-equality figures of the prologue check (fused step against `featmap_rotary` + `mhla_causal_step`, MI355X): see
profiles/causal_decode_graph.md."""
import functools

import pytest
import torch

from decode_util import check_state, check_step_rows, ragged_inputs, ragged_prefill, window_rows
from gpu_util import DEV, CAUSAL_TOL, TOL, check, poison, _fla_layer
from neighbour_refs import featmap_rotary_ref
from oracle import mhla_oracle as orc

pytestmark = pytest.mark.gpu

LENGTHS, CAP, NSTEP = (0, 5, 62, 63, 64, 130), 4, 4


def _equal_states(a, b, what):
    for n in ("S", "P", "Cur", "pos"):
        assert torch.equal(getattr(a, n), getattr(b, n)), f"{what}: {n} differs"


@functools.lru_cache(maxsize=None)
def _dev_and_ragged(dtype, K, V, epilogue):
    """NSTEP device-positioned steps on one clone of a prefilled ragged state and NSTEP ragged steps on another: (rows of both,
    both states, the inputs, the per-sequence oracle, the epilogue's gate and weight).  Run once per case, shared by the tests."""
    import mhla_amd
    H = 2
    q, k, v, mix, want = ragged_inputs(LENGTHS, NSTEP, H, K, V, CAP, dtype)
    qd, kd, vd, md = (t.to(DEV) for t in (q, k, v, mix))
    kw, g, w = {}, None, None
    if epilogue:
        gen = torch.Generator().manual_seed(7)
        g = torch.randn(len(LENGTHS), NSTEP, H, V, generator=gen).to(dtype)
        w = torch.rand(V, generator=gen) + 0.5
        kw = dict(norm_weight=w.to(DEV), norm_eps=1e-5)
    poison()
    _, state = ragged_prefill(qd, kd, vd, md, LENGTHS, "left_padded", CAP)
    a, b = state.clone(), state.clone()
    qs, ks, vs = (window_rows(t, LENGTHS, 0, NSTEP) for t in (qd, kd, vd))
    rows_dev, rows_rag = [], []
    for t in range(NSTEP):
        tok = (qs[:, t:t + 1], ks[:, t:t + 1], vs[:, t:t + 1])
        gk = dict(kw, gate=g[:, t:t + 1].to(DEV)) if epilogue else {}
        rows_dev.append(mhla_amd.mhla_causal_step_dev(*tok, md, a, **gk))
        rows_rag.append(mhla_amd.mhla_causal_step(*tok, md, b, **gk))
    return torch.cat(rows_dev, 1), torch.cat(rows_rag, 1), a, b, (qd, kd, vd, md), want, g, w


CASES = [(dt, K, V, False) for dt in (torch.bfloat16, torch.float32) for K, V in ((64, 64), (128, 256), (40, 68))] + \
        [(torch.bfloat16, 128, 256, True)]
IDS = [f"{'bf16' if c[0] is torch.bfloat16 else 'fp32'}-{c[1]}x{c[2]}{'-epilogue' if c[3] else ''}" for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_same_bits_as_the_ragged_step(case):
    """An empty state, mid-chunk, a boundary on the second step and on the first, a chunk start, the third chunk -- in one batch."""
    rows_dev, rows_rag, a, b, _, _, _, _ = _dev_and_ragged(*case)
    assert rows_dev.dtype == case[0] and rows_dev.shape == (len(LENGTHS), NSTEP, 2, case[2])
    assert torch.equal(rows_dev, rows_rag), "rows differ from the ragged step's"
    _equal_states(a, b, "after the steps")
    assert a.pos.tolist() == [m + NSTEP for m in LENGTHS]
    assert a.full.tolist() == [0] * len(LENGTHS)
    # the device-positioned call left the host mirror where it was, and says so; sync() brings it up
    assert a.stale and a.lengths == LENGTHS and b.lengths == tuple(m + NSTEP for m in LENGTHS) and not b.stale
    c = a.clone().sync()
    assert not c.stale and c.lengths == b.lengths and c.seen == b.seen


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_and_state_match_the_oracle(case):
    dtype = case[0]
    rows_dev, _, a, _, (qd, kd, vd, md), want, g, w = _dev_and_ragged(*case)
    for s, m in enumerate(LENGTHS):
        if g is None:
            check_step_rows(f"seq {s}: rows", rows_dev[s:s + 1], want[s], m, dtype)
        else:
            y_ref = orc.rms_norm_swish_gate(want[s][:, m:], g[s:s + 1].float(), w, 1e-5)
            check(f"seq {s}: y", rows_dev[s:s + 1], y_ref, CAUSAL_TOL[dtype])
        check_state(a, qd, kd, vd, md, f"seq {s} after {NSTEP} steps", s, m + NSTEP)


def _tables(rows, K, dtype, seed=5):
    """cos / sin of `rows` positions, K/2 frequencies, as the layer keeps them: computed in fp32, stored in the activation dtype."""
    inv = 1.0 / (10000.0 ** (torch.arange(0, K, 2, dtype=torch.float32) / K))
    fr = torch.outer(torch.arange(rows, dtype=torch.float32), inv)
    return torch.cos(fr).to(dtype), torch.sin(fr).to(dtype)


@functools.lru_cache(maxsize=None)
def _raw_seqs(lengths, n, H, K, V, L, dtype, fmap, seed=4321):
    """Projections' q, k (before the prologue), v and a mix, every sequence on its own timeline starting at position 0; the tables of
    exactly 64 L rows; the prologue's fp64 reference rounded to the dtype; the oracle per sequence on those."""
    B, T = len(lengths), max(lengths) + n + 1
    g = torch.Generator().manual_seed(seed)
    xq, xk = (torch.randn(B, T, H, K, generator=g).to(dtype) for _ in range(2))
    v = torch.randn(B, T, H, V, generator=g).to(dtype)
    mix = torch.tril(torch.rand(L, L, generator=g).clamp(1e-5, 1))
    cos, sin = _tables(64 * L, K, dtype)
    q, k = (featmap_rotary_ref(x, cos, sin, fmap, 0).to(dtype) for x in (xq, xk))
    want = tuple(orc.causal_fwd(q[b:b + 1, :m + n].float(), k[b:b + 1, :m + n].float(), v[b:b + 1, :m + n].float(), mix)
                 for b, m in enumerate(lengths))
    return xq, xk, v, mix, cos, sin, q, k, want


def _unfused_step(xq, xk, vt, mix, state, cos, sin, fmap):
    """The chain the fused step replaces: `featmap_rotary` on the table rows gathered at the device positions, then the ragged step."""
    import mhla_amd
    B, _, H, K = xq.shape
    c, s = cos.index_select(0, state.pos.long()), sin.index_select(0, state.pos.long())
    q = mhla_amd.featmap_rotary(xq.reshape(1, B, H, K), c, s, fmap, 0).reshape(B, 1, H, K)
    k = mhla_amd.featmap_rotary(xk.reshape(1, B, H, K), c, s, fmap, 0).reshape(B, 1, H, K)
    return mhla_amd.mhla_causal_step(q, k, vt, mix, state), q, k


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("K,V", [(64, 64), (40, 68)])
@pytest.mark.parametrize("fmap", ["identity", "relu", "elu"])
def test_fused_prologue(fmap, K, V, dtype):
    """Rows against the oracle on the fp64 prologue's rounded outputs; state against what `featmap_rotary` + `mhla_causal_step` leave."""
    import mhla_amd
    H = 2
    xq, xk, v, mix, cos, sin, q, k, want = _raw_seqs(LENGTHS, NSTEP, H, K, V, CAP, dtype, fmap)
    xqd, xkd, vd, md, cd, sd, qd, kd = (t.to(DEV) for t in (xq, xk, v, mix, cos, sin, q, k))
    assert cd.shape == (64 * CAP, K // 2)
    poison()
    _, state = ragged_prefill(qd, kd, vd, md, LENGTHS, "left_padded", CAP)
    a, b = state.clone(), state.clone()
    xqs, xks, vs = (window_rows(t, LENGTHS, 0, NSTEP) for t in (xqd, xkd, vd))
    rows, rows_unfused = [], []
    for t in range(NSTEP):
        rows.append(mhla_amd.mhla_causal_step_dev(xqs[:, t:t + 1], xks[:, t:t + 1], vs[:, t:t + 1], md, a, feature_map=fmap, rotary=(cd, sd)))
        rows_unfused.append(_unfused_step(xqs[:, t:t + 1], xks[:, t:t + 1], vs[:, t:t + 1], md, b, cd, sd, fmap)[0])
    rows, rows_unfused = torch.cat(rows, 1), torch.cat(rows_unfused, 1)
    same = {n: torch.equal(getattr(a, n), getattr(b, n)) for n in ("S", "P", "Cur")}
    print(f"prologue {fmap} K={K} {dtype}: rows bit-equal to the unfused chain: {torch.equal(rows, rows_unfused)}; state bit-equal: {same}")
    assert a.pos.tolist() == b.pos.tolist() == [m + NSTEP for m in LENGTHS]
    for s, m in enumerate(LENGTHS):
        check_step_rows(f"seq {s}: rows", rows[s:s + 1], want[s], m, dtype)
    for n in ("S", "P", "Cur"):
        x, y = getattr(a, n), getattr(b, n)
        if float(y.abs().max()) == 0.0:
            assert float(x.abs().max()) == 0.0
        else:
            check(f"state {n} against the unfused chain", x, y.cpu(), TOL[torch.float32])


def test_capacity_freezes_a_sequence():
    """cap = 2: sequence 0 closes its last chunk on the second step (P = 0) and is frozen from then on -- zero rows, the state of
    step 2, `full` set -- while the others step on; `sync()` reports it after refreshing the mirror."""
    import mhla_amd
    dtype, H, K, V, lengths, cap, L, n = torch.float32, 2, 16, 24, (126, 120, 0), 2, 3, 4
    q, k, v, mix, want = ragged_inputs(lengths, n, H, K, V, L, dtype)
    qd, kd, vd, md = (t.to(DEV) for t in (q, k, v, mix))
    poison()
    _, state = ragged_prefill(qd, kd, vd, md, lengths, "left_padded", cap)
    assert state.capacity_chunks == cap
    qs, ks, vs = (window_rows(t, lengths, 0, n) for t in (qd, kd, vd))
    rows, snap = [], None
    for t in range(n):
        poison()
        rows.append(mhla_amd.mhla_causal_step_dev(qs[:, t:t + 1], ks[:, t:t + 1], vs[:, t:t + 1], md, state))
        if t == 1:
            snap = state.clone()
            assert snap.pos.tolist() == [128, 122, 2] and snap.full.tolist() == [0, 0, 0]
            assert float(snap.P[0].abs().max()) == 0.0 and float(snap.Cur[0].abs().max()) == 0.0 and float(snap.S[0, :, 1].abs().max()) > 0
    rows = torch.cat(rows, 1)
    assert torch.equal(rows[0, 2:], torch.zeros_like(rows[0, 2:])), "rows of the frozen sequence are not exactly zero"
    for name in ("S", "P", "Cur"):
        assert torch.equal(getattr(state, name)[0], getattr(snap, name)[0]), f"{name} of the frozen sequence moved"
    assert state.pos.tolist() == [128, 124, 4] and state.full.tolist() == [1, 0, 0]
    check_step_rows("seq 0: rows before the capacity", rows[0:1, :2], want[0][:, :128], 126, dtype)
    check_state(state, qd, kd, vd, md, "seq 0 at the capacity", 0, 128)
    for s in (1, 2):
        check_step_rows(f"seq {s}: rows", rows[s:s + 1], want[s], lengths[s], dtype)
        check_state(state, qd, kd, vd, md, f"seq {s} after {n} steps", s, lengths[s] + n)
    assert state.stale and state.lengths == lengths
    with pytest.raises(ValueError, match=r"sync\(\)"):
        mhla_amd.mhla_causal_step(qs[:, :1], ks[:, :1], vs[:, :1], md, state)
    with pytest.raises(IndexError, match=r"sequences \[0\]"):
        state.sync()
    assert state.lengths == (128, 124, 4) and state.seen == 128 and not state.stale


def test_graph_replay_gives_the_eager_bits():
    """What no host-positioned call can give: ONE captured step, replayed for 5 tokens, while sequences cross a boundary on the
    first replay (63), on the third (61) and on the first with the next chunk's row (127), prologue and epilogue on."""
    import mhla_amd
    dtype, H, K, V, lengths, cap, n, fmap = torch.bfloat16, 2, 64, 128, (0, 61, 63, 127), 4, 5, "relu"
    xq, xk, v, mix, cos, sin, q, k, want = _raw_seqs(lengths, n, H, K, V, cap, dtype, fmap)
    xqd, xkd, vd, md, cd, sd, qd, kd = (t.to(DEV) for t in (xq, xk, v, mix, cos, sin, q, k))
    gen = torch.Generator().manual_seed(9)
    g = torch.randn(len(lengths), n, H, V, generator=gen).to(dtype)
    w = torch.rand(V, generator=gen) + 0.5
    gd, wd = g.to(DEV), w.to(DEV)
    _, state = ragged_prefill(qd, kd, vd, md, lengths, "left_padded", cap)
    xqs, xks, vs = (window_rows(t, lengths, 0, n) for t in (xqd, xkd, vd))
    step = lambda tq, tk, tv, tg, st: mhla_amd.mhla_causal_step_dev(tq, tk, tv, md, st, feature_map=fmap, rotary=(cd, sd), gate=tg,
                                                                    norm_weight=wd, norm_eps=1e-5)
    eager, replayed = state.clone(), state.clone()
    replayed.full   # (created before the capture: a tensor made while capturing belongs to the graph)
    sq, sk, sv, sg = (t[:, :1].clone() for t in (xqs, xks, vs, gd))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sq, sk, sv, sg, state.clone())   # warm-up on a throw-away clone: code objects loaded, allocator warm
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(sq, sk, sv, sg, replayed)
    torch.cuda.synchronize()
    _equal_states(replayed, state, "the capture itself ran nothing")
    rows = []
    for t in range(n):
        for buf, src in ((sq, xqs), (sk, xks), (sv, vs), (sg, gd)):
            buf.copy_(src[:, t:t + 1])
        graph.replay()
        ref = step(xqs[:, t:t + 1], xks[:, t:t + 1], vs[:, t:t + 1], gd[:, t:t + 1], eager)
        assert torch.equal(out, ref), f"replay {t}: rows differ from the eager step's"
        _equal_states(replayed, eager, f"replay {t}")
        rows.append(out.clone())
    rows = torch.cat(rows, 1)
    assert replayed.pos.tolist() == [m + n for m in lengths] and replayed.full.tolist() == [0] * 4
    for s, m in enumerate(lengths):
        y_ref = orc.rms_norm_swish_gate(want[s][:, m:], g[s:s + 1].float(), w, 1e-5)
        check(f"seq {s}: y over the replays", rows[s:s + 1], y_ref, CAUSAL_TOL[dtype])
    assert replayed.sync().lengths == tuple(m + n for m in lengths)


def test_fla_layer_device_positions_and_graph_replay():
    """The layer on a `DecodeCache(device_positions=True)` against an ordinary `DecodeCache` (left-padded prefill, then one-token
    calls), and a captured layer step replayed against the eager device-positioned bits."""
    import mhla_amd
    from mhla_amd import modules
    m = _fla_layer().to(DEV).to(torch.bfloat16).eval()
    lens, T0, n = (70, 33), 70, 3
    gen = torch.Generator().manual_seed(21)
    prompt = torch.randn(2, T0, 256, generator=gen)
    mask = torch.zeros(2, T0, dtype=torch.long)
    for b, ln in enumerate(lens):
        prompt[b, :T0 - ln], mask[b, T0 - ln:] = float("nan"), 1
    prompt, mask = prompt.to(DEV).to(torch.bfloat16), mask.to(DEV)
    steps = torch.randn(2, n, 256, generator=gen).to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        plain, dev, rep = modules.DecodeCache(), modules.DecodeCache(device_positions=True), modules.DecodeCache(device_positions=True)
        o_plain = [m(prompt, attention_mask=mask, past_key_values=plain, use_cache=True)[0]]
        o_dev = [m(prompt, attention_mask=mask, past_key_values=dev, use_cache=True)[0]]
        m(prompt, attention_mask=mask, past_key_values=rep, use_cache=True)
        assert torch.equal(o_plain[0], o_dev[0])
        st = dev[0]["recurrent_state"]
        assert isinstance(st, mhla_amd.CausalState) and st.lengths == lens and dev[0]["dev_cos"].shape == (64 * 32, 32)
        assert dev[0]["dev_mix"].dtype == torch.float32 and dev[0]["dev_mix"].shape == (32, 32)
        with pytest.raises(NotImplementedError, match="one token per call"):
            m(steps[:, :2], past_key_values=dev, use_cache=True)
        for t in range(n):
            o_plain.append(m(steps[:, t:t + 1], past_key_values=plain, use_cache=True)[0])
            matrix = m.mixing_matrix.data_ptr()   # (the ordinary call above stored a new clamped copy)
            o_dev.append(m(steps[:, t:t + 1], past_key_values=dev, use_cache=True)[0])
            assert m.mixing_matrix.data_ptr() == matrix, "a device-positioned step reassigned mixing_matrix.data"
        check("layer: device-positioned cache against the ordinary cache", torch.cat(o_dev, 1)[:, T0:], torch.cat(o_plain, 1)[:, T0:].float().cpu(), 1e-4)
        assert st.stale and st.lengths == lens and dev.get_seq_length(0) == T0
        dev.sync()
        assert st.lengths == tuple(x + n for x in lens) and dev.get_seq_length(0) == plain.get_seq_length(0) == T0 + n
        assert st.pos.tolist() == plain[0]["recurrent_state"].pos.tolist()
        # graph: token 0 eagerly on a side stream (the warm-up), then one captured step replayed for the others
        x = steps[:, :1].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(x, past_key_values=rep, use_cache=True)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(x, past_key_values=rep, use_cache=True)[0]
        for t in range(1, n):
            x.copy_(steps[:, t:t + 1])
            graph.replay()
            assert torch.equal(out, o_dev[1 + t]), f"replay of token {t}: the layer's output differs from the eager device-positioned step's"
        _equal_states(rep[0]["recurrent_state"], st, "after the replays")
        rep.sync()
        assert rep.get_seq_length(0) == T0 + n


def test_gpt_host_generate_with_a_graph():
    from mhla_amd.hosts.gpt import GPT_MHLA
    torch.manual_seed(5)
    model = GPT_MHLA(vocab_size=64, hidden_size=128, num_layers=2, num_heads=2, max_seq_len=256, exact_decoding=True).to(DEV).eval()
    prompt = torch.randint(0, 64, (2, 60), generator=torch.Generator().manual_seed(6)).to(DEV)
    n, tol = 70, 1e-4                                   # (crosses the boundaries at 64 and 128; the host decode tests' tolerance)
    ids_e, log_e = model.generate(prompt, n, return_logits=True)
    ids_g, log_g = model.generate(prompt, n, graph=True, return_logits=True)
    assert ids_g.shape == ids_e.shape == (2, n) and log_g.shape == log_e.shape == (2, n, 64)
    assert torch.equal(model.generate(prompt, n), ids_e)
    for t in range(n):
        check(f"logits of new token {t}: graph replay against the eager steps", log_g[:, t], log_e[:, t].cpu(), tol)
        top2 = log_e[:, t].float().topk(2, dim=-1).values
        clear = (top2[:, 0] - top2[:, 1]) > tol * log_e[:, t].abs().max()
        assert torch.equal(ids_g[:, t][clear], ids_e[:, t][clear]), f"new token {t}: ids differ where the eager margin is clear"
        if not torch.equal(ids_g[:, t], ids_e[:, t]):   # a near-tie went the other way: from here on the two decode different texts
            break
    for short in (0, 1, 2):                             # (no step to capture; the warm-up step alone; one replay)
        assert torch.equal(model.generate(prompt, short, graph=True), ids_g[:, :short])
