"""GPU parity: decoding with grouped-query heads -- k, v and the `CausalState` with Hkv heads, q with H = G Hkv (the *_gqa entry
points).  The state is a function of k and v alone, so the reference is the code that exists: the same call on k, v repeated G
times per head with a state of H heads, which the grouped call must equal BIT FOR BIT (rows, and the state against heads [::G] of
the repeated one); one case per dtype is also held to the CPU oracle over the whole sequence on repeated heads.

Shapes: K = 40 (a partial 16-row group; K % 8 == 0 for the fused prologue), V = 72 (a second, partial 64-column tile), B = 3,
G = 2, 3, 8, a state of 4 chunks.  Every sequence is a prefix of one stream of tokens per batch entry, so one oracle run per case
serves every position."""
import functools

import pytest
import torch

from decode_util import NAN, signed_features
from gpu_util import DEV, CAUSAL_TOL, check, poison
from oracle import mhla_oracle as orc

pytestmark = pytest.mark.gpu

B, K, V, CAP, L = 3, 40, 72, 4, 5
HEADS = [(4, 2), (6, 2), (8, 1)]
DTYPES = [torch.bfloat16, torch.float32]
LENGTHS = (5, 63, 127)        # mid-chunk; on a boundary; the token that closes chunk 1
COUNTS = (1, 70, 0)           # one token (the step's arithmetic); a chunk closed, a whole one, a tail; a slot that sits out
T_EXT = 70
STREAM = 64 * CAP + 8
cases = pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
heads = pytest.mark.parametrize("H,Hk", HEADS, ids=[f"H{h}kv{k}" for h, k in HEADS])


def rep(t, G):
    return t.repeat_interleave(G, 2)


@functools.lru_cache(maxsize=None)
def _stream(dtype, H, Hk):
    """One stream of tokens per batch entry (q with H heads, k, v with Hk), gate, norm weight, the matrix -- on the device."""
    g = torch.Generator().manual_seed(97 + H + Hk)
    q, k = signed_features(g, B, STREAM, H, K).to(dtype), signed_features(g, B, STREAM, Hk, K).to(dtype)
    v, gate = torch.randn(B, STREAM, Hk, V, generator=g).to(dtype), torch.randn(B, STREAM, H, V, generator=g).to(dtype)
    mix = torch.tril(torch.rand(L, L, generator=g).clamp(1e-5, 1))
    w = torch.rand(V, generator=g) + 0.5
    return tuple(t.to(DEV) for t in (q, k, v, gate, mix, w))


@functools.lru_cache(maxsize=None)
def _oracle(dtype, H, Hk):
    """Rows of the causal operator over every whole stream, on repeated heads (CPU, once per case)."""
    q, k, v, _, mix, _ = (t.cpu() for t in _stream(dtype, H, Hk))
    return orc.causal_fwd(q.float(), rep(k, H // Hk).float(), rep(v, H // Hk).float(), mix)


def _states(k, v, mix, lengths, G):
    """The grouped ragged state after `lengths` tokens of the streams and the repeated-head one built the same way; NaN in every row
    of S at or beyond a sequence's finished chunks (a read of an unfinished row shows)."""
    import mhla_amd
    T = max(max(lengths), 1)
    kh, vh = k[:, :T].clone(), v[:, :T].clone()
    for b, n in enumerate(lengths):
        kh[b, n:], vh[b, n:] = NAN, NAN
    grouped = mhla_amd.mhla_causal_state(kh, vh, mix, lengths=lengths, capacity_chunks=CAP)
    repeated = mhla_amd.mhla_causal_state(rep(kh, G), rep(vh, G), mix, lengths=lengths, capacity_chunks=CAP)
    for st in (grouped, repeated):
        for b, n in enumerate(lengths):
            st.S[b, :, n // 64:] = NAN
    assert grouped.S.shape == (B, k.shape[2], CAP, K, V) and repeated.S.shape == (B, k.shape[2] * G, CAP, K, V)
    return grouped, repeated


def _same_state(name, grouped, repeated, G):
    """The grouped state against heads [::G] of the repeated one, bit for bit: P, Cur, pos, the finished chunks of S."""
    torch.cuda.synchronize()
    assert grouped.lengths == repeated.lengths and grouped.seen == repeated.seen, name
    assert torch.equal(grouped.pos, repeated.pos), f"{name}: pos {grouped.pos.tolist()} vs {repeated.pos.tolist()}"
    for part in ("P", "Cur"):
        a, b = getattr(grouped, part), getattr(repeated, part)[:, ::G]
        assert not torch.isnan(a).any(), f"{name}: NaN in {part}"
        assert torch.equal(a, b), f"{name}: {part} differs (max {(a - b).abs().max().item():.3e})"
    for g in range(1, G):   # (the premise: the repeated heads of a group hold equal copies)
        assert torch.equal(repeated.P[:, g::G], repeated.P[:, ::G]) and torch.equal(repeated.Cur[:, g::G], repeated.Cur[:, ::G])
    for s, n in enumerate(grouped.pos.tolist()):
        a, b = grouped.S[s, :, :n // 64], repeated.S[s, ::G, :n // 64]
        assert not torch.isnan(a).any() and torch.equal(a, b), f"{name}: sequence {s}: a finished chunk of S differs"


def _same_rows(name, got, ref):
    assert got.shape == ref.shape and got.dtype == ref.dtype
    assert not torch.isnan(got).any(), f"{name}: NaN in the rows"
    assert torch.equal(got, ref), f"{name}: rows differ from the repeated-head call (max {(got.float() - ref.float()).abs().max().item():.3e})"


def _tok(x, lengths):
    """[B, 1, ...]: token lengths[b] of stream b."""
    return torch.stack([x[b, n:n + 1] for b, n in enumerate(lengths)])


def _window(x, lengths, counts, T):
    """[B, T, ...]: tokens lengths[b] .. lengths[b] + counts[b] of stream b, left-padded with NaN."""
    out = torch.full((x.shape[0], T, *x.shape[2:]), NAN, dtype=x.dtype, device=x.device)
    for b, (p, n) in enumerate(zip(lengths, counts)):
        if n:
            out[b, T - n:] = x[b, p:p + n]
    return out


@heads
@cases
@pytest.mark.parametrize("epilogue", [False, True], ids=["rows", "normgate"])
def test_ragged_step_equals_the_repeated_head_step(dtype, H, Hk, epilogue):
    import mhla_amd
    G = H // Hk
    q, k, v, gate, mix, w = _stream(dtype, H, Hk)
    grouped, repeated = _states(k, v, mix, LENGTHS, G)
    qt, kt, vt, gt = (_tok(x, LENGTHS) for x in (q, k, v, gate))
    kw = dict(gate=gt, norm_weight=w, norm_eps=1e-6) if epilogue else {}
    poison()
    o = mhla_amd.mhla_causal_step(qt, kt, vt, mix, grouped, **kw)
    ref = mhla_amd.mhla_causal_step(qt, rep(kt, G), rep(vt, G), mix, repeated, **kw)
    assert o.shape == (B, 1, H, V) and grouped.lengths == tuple(n + 1 for n in LENGTHS)
    _same_rows("step", o, ref)
    _same_state("step", grouped, repeated, G)


@heads
@cases
def test_four_steps_across_a_roll(dtype, H, Hk):
    """From length 62 (and 125: the roll into chunk 2) four consecutive steps; the oracle's rows for one case per dtype."""
    import mhla_amd
    G = H // Hk
    q, k, v, _, mix, _ = _stream(dtype, H, Hk)
    start = (62, 5, 125)
    grouped, repeated = _states(k, v, mix, start, G)
    rows = []
    for t in range(4):
        at = tuple(n + t for n in start)
        qt, kt, vt = (_tok(x, at) for x in (q, k, v))
        poison()
        o = mhla_amd.mhla_causal_step(qt, kt, vt, mix, grouped)
        ref = mhla_amd.mhla_causal_step(qt, rep(kt, G), rep(vt, G), mix, repeated)
        _same_rows(f"step {t}", o, ref)
        _same_state(f"step {t}", grouped, repeated, G)
        rows.append(o)
    assert grouped.lengths == (66, 9, 129) and grouped.pos.tolist() == [66, 9, 129]
    if (H, Hk) == HEADS[0]:
        want = _oracle(dtype, H, Hk)
        rows = torch.cat(rows, 1)
        for b, n in enumerate(start):
            check(f"sequence {b}: step rows vs the oracle", rows[b:b + 1], want[b:b + 1, n:n + 4], CAUSAL_TOL[dtype])


@heads
@cases
@pytest.mark.parametrize("prologue", [False, True], ids=["plain", "fused-prologue"])
@pytest.mark.parametrize("lengths", [LENGTHS, (5, 63, 64 * CAP)], ids=["live", "one-frozen"])
def test_device_positioned_step_equals_the_repeated_head_step(dtype, H, Hk, prologue, lengths):
    """`one-frozen`: the last sequence is at the capacity -- zero rows for all G heads of every group, its state untouched, `full` set."""
    import mhla_amd
    G = H // Hk
    frozen = lengths[2] == 64 * CAP
    q, k, v, gate, mix, w = _stream(dtype, H, Hk)
    grouped, repeated = _states(k, v, mix, lengths, G)
    at = lengths[:2] + (0 if frozen else lengths[2],)     # (a frozen sequence's token is not read into anything)
    kw = dict(gate=_tok(gate, at), norm_weight=w, norm_eps=1e-6)
    if prologue:
        ang = torch.outer(torch.arange(64 * CAP, dtype=torch.float32), 1.0 / (10000 ** (torch.arange(0, K, 2, dtype=torch.float32) / K)))
        kw.update(feature_map="relu", rotary=(torch.cos(ang).to(dtype).to(DEV), torch.sin(ang).to(dtype).to(DEV)))
    qt, kt, vt = (_tok(x, at) for x in (q, k, v))
    before = grouped.clone()
    poison()
    o = mhla_amd.mhla_causal_step_dev(qt, kt, vt, mix, grouped, **kw)
    ref = mhla_amd.mhla_causal_step_dev(qt, rep(kt, G), rep(vt, G), mix, repeated, **kw)
    _same_rows("device-positioned step", o, ref)
    assert grouped.stale and grouped.full.tolist() == [0, 0, int(frozen)] == repeated.full.tolist()
    if frozen:
        assert float(o[2].float().abs().max()) == 0.0, "a frozen sequence's rows must be zeros for every head of the group"
        assert torch.equal(grouped.P[2], before.P[2]) and torch.equal(grouped.Cur[2], before.Cur[2]), "a frozen sequence's state changed"
        for st in (grouped, repeated):
            with pytest.raises(IndexError):
                st.sync()
    else:
        assert float(o[2].float().abs().max()) > 0.0
        grouped.sync(), repeated.sync()
    assert grouped.lengths == (6, 64, lengths[2] + (0 if frozen else 1)) and not grouped.stale
    _same_state("device-positioned step", grouped, repeated, G)


@heads
@cases
def test_ragged_extend_and_verify_equal_the_repeated_head_calls(dtype, H, Hk):
    import mhla_amd
    G = H // Hk
    q, k, v, gate, mix, w = _stream(dtype, H, Hk)
    qw, kw_, vw, gw = (_window(x, LENGTHS, COUNTS, T_EXT) for x in (q, k, v, gate))
    epi = dict(gate=gw, norm_weight=w, norm_eps=1e-6)
    grouped, repeated = _states(k, v, mix, LENGTHS, G)
    before = grouped.clone()
    # the verify first: rows, and nothing of the committed state moved
    poison()
    o_v, draft = mhla_amd.mhla_causal_verify(qw, kw_, vw, mix, grouped, counts=COUNTS, left_padded=True, **epi)
    ref_v, _ = mhla_amd.mhla_causal_verify(qw, rep(kw_, G), rep(vw, G), mix, repeated, counts=COUNTS, left_padded=True, **epi)
    _same_rows("verify", o_v, ref_v)
    assert draft.k.shape[2] == Hk and grouped.lengths == LENGTHS
    _same_state("verify", grouped, repeated, G)
    assert torch.equal(grouped.P, before.P) and torch.equal(grouped.Cur, before.Cur) and torch.equal(grouped.pos, before.pos)
    for b, n in enumerate(LENGTHS):
        assert torch.equal(grouped.S[b, :, :n // 64], before.S[b, :, :n // 64]), f"sequence {b}: the verify changed a finished chunk"
    # then the extend, on the same states (the verify scribbled on unfinished rows of S only)
    poison()
    o = mhla_amd.mhla_causal_extend(qw, kw_, vw, mix, grouped, counts=COUNTS, left_padded=True, **epi)
    ref = mhla_amd.mhla_causal_extend(qw, rep(kw_, G), rep(vw, G), mix, repeated, counts=COUNTS, left_padded=True, **epi)
    _same_rows("extend", o, ref)
    _same_rows("extend vs verify", o, o_v)
    assert grouped.lengths == tuple(p + n for p, n in zip(LENGTHS, COUNTS))
    _same_state("extend", grouped, repeated, G)
    assert float(o[2].float().abs().max()) == 0.0 and float(o[0, :T_EXT - 1].float().abs().max()) == 0.0, "padding rows must be zeros"
    assert torch.equal(grouped.P[2], before.P[2]) and torch.equal(grouped.Cur[2], before.Cur[2]), "a count of 0 must leave the state"


@cases
def test_extend_rows_against_the_oracle(dtype):
    """One oracle case per dtype: the grouped extend's rows (no epilogue) against the operator over the whole stream, repeated heads."""
    import mhla_amd
    H, Hk = HEADS[0]
    q, k, v, _, mix, _ = _stream(dtype, H, Hk)
    want = _oracle(dtype, H, Hk)
    grouped, _ = _states(k, v, mix, LENGTHS, H // Hk)
    poison()
    o = mhla_amd.mhla_causal_extend(*(_window(x, LENGTHS, COUNTS, T_EXT) for x in (q, k, v)), mix, grouped, counts=COUNTS, left_padded=True)
    for b, (p, n) in enumerate(zip(LENGTHS, COUNTS)):
        if n:
            check(f"sequence {b} (pos {p}, n {n}): extend rows vs the oracle", o[b:b + 1, T_EXT - n:], want[b:b + 1, p:p + n], CAUSAL_TOL[dtype])


@cases
def test_extend_beyond_the_workspace_cap_runs_window_by_window(dtype, monkeypatch):
    """A grouped call whose workspace would exceed `EXTEND_WS_CAP_BYTES` has no uniform chain to fall back to: it runs the ragged
    chain over windows of whole chunks of tokens.  The cap is lowered to what a 64-token window needs, so that the 70-token call is
    cut in two; rows against the oracle, the state against the one-chain call's within fp32 rounding (the sums are cut elsewhere)."""
    import mhla_amd
    from mhla_amd import ops, _lib
    from gpu_util import TOL
    H, Hk = HEADS[0]
    q, k, v, _, mix, _ = _stream(dtype, H, Hk)
    want = _oracle(dtype, H, Hk)
    windows = [_window(x, LENGTHS, COUNTS, T_EXT) for x in (q, k, v)]
    one, _ = _states(k, v, mix, LENGTHS, H // Hk)
    cut = one.clone()
    mhla_amd.mhla_causal_extend(*windows, mix, one, counts=COUNTS, left_padded=True)
    lib = _lib.load()
    cap = lib.mhla_causal_extend_ragged_gqa_ws_bytes(B, 64, H, Hk, K, V, 1, 0)
    assert lib.mhla_causal_extend_ragged_gqa_ws_bytes(B, T_EXT, H, Hk, K, V, 2, 0) > cap
    monkeypatch.setattr(ops, "EXTEND_WS_CAP_BYTES", cap)
    calls = []
    chain = ops._causal_extend_ragged
    monkeypatch.setattr(ops, "_causal_extend_ragged", lambda *a, **kw: (calls.append(a[0].shape[1]), chain(*a, **kw))[1])
    poison()
    o = mhla_amd.mhla_causal_extend(*windows, mix, cut, counts=COUNTS, left_padded=True)
    assert calls == [64, T_EXT - 64], calls
    assert cut.lengths == one.lengths and torch.equal(cut.pos, one.pos) and not torch.isnan(o).any()
    for b, (p, n) in enumerate(zip(LENGTHS, COUNTS)):
        if n:
            check(f"sequence {b} (pos {p}, n {n}): rows vs the oracle", o[b:b + 1, T_EXT - n:], want[b:b + 1, p:p + n], CAUSAL_TOL[dtype])
    assert float(o[2].float().abs().max()) == 0.0 and float(o[0, :T_EXT - 1].float().abs().max()) == 0.0, "padding rows must be zeros"
    for part in ("P", "Cur"):
        check(part, getattr(cut, part), getattr(one, part).cpu(), TOL[torch.float32])
    check("S[1]", cut.S[1:2, :, :2], one.S[1:2, :, :2].cpu(), TOL[torch.float32])
    assert torch.equal(cut.P[2], one.P[2]) and torch.equal(cut.Cur[2], one.Cur[2])


@heads
@cases
def test_uniform_state_prefill_then_steps(dtype, H, Hk):
    """A uniform grouped state is served by the ragged grouped chain: prefill 62 tokens, three steps (one roll), against the
    repeated-head calls on `state.to_ragged()`."""
    import mhla_amd
    G = H // Hk
    q, k, v, _, mix, _ = _stream(dtype, H, Hk)
    poison()
    o0, state = mhla_amd.mhla_causal_prefill(q[:, :62], k[:, :62], v[:, :62], mix, capacity_chunks=CAP)
    r0, uniform = mhla_amd.mhla_causal_prefill(q[:, :62], rep(k[:, :62], G), rep(v[:, :62], G), mix, capacity_chunks=CAP)
    _same_rows("prefill", o0, r0)
    assert state.lengths is None and state.seen == 62 and state.S.shape == (B, Hk, CAP, K, V) and uniform.S.shape[1] == H
    assert state.nbytes * G == uniform.nbytes
    repeated = uniform.to_ragged()
    for t in range(62, 65):
        poison()
        o = mhla_amd.mhla_causal_step(q[:, t:t + 1], k[:, t:t + 1], v[:, t:t + 1], mix, state)
        ref = mhla_amd.mhla_causal_step(q[:, t:t + 1], rep(k[:, t:t + 1], G), rep(v[:, t:t + 1], G), mix, repeated)
        _same_rows(f"step at {t}", o, ref)
        assert state.lengths is None and state.pos is None and state.seen == t + 1
        for part in ("P", "Cur"):
            assert torch.equal(getattr(state, part), getattr(repeated, part)[:, ::G]), f"step at {t}: {part} differs"
        assert torch.equal(state.S[:, :, :(t + 1) // 64], repeated.S[:, ::G, :(t + 1) // 64]), f"step at {t}: S differs"
    # several tokens on the uniform state: the ragged grouped chain again
    poison()
    o = mhla_amd.mhla_causal_extend(q[:, 65:135], k[:, 65:135], v[:, 65:135], mix, state)
    ref = mhla_amd.mhla_causal_extend(q[:, 65:135], rep(k[:, 65:135], G), rep(v[:, 65:135], G), mix, repeated, counts=(70,) * B)
    _same_rows("extend on the uniform state", o, ref)
    assert state.seen == 135 and state.lengths is None
    assert torch.equal(state.P, repeated.P[:, ::G]) and torch.equal(state.Cur, repeated.Cur[:, ::G])
    assert torch.equal(state.S[:, :, :2], repeated.S[:, ::G, :2])


@heads
@cases
def test_commit_is_the_grouped_extend_by_the_accepted_prefix(dtype, H, Hk):
    import mhla_amd
    G = H // Hk
    accept = (1, 3, 0)
    q, k, v, _, mix, _ = _stream(dtype, H, Hk)
    qw, kw_, vw = (_window(x, LENGTHS, COUNTS, T_EXT) for x in (q, k, v))
    state, _ = _states(k, v, mix, LENGTHS, G)
    ref = state.clone()
    poison()
    _, draft = mhla_amd.mhla_causal_verify(qw, kw_, vw, mix, state, counts=COUNTS, left_padded=True)
    assert mhla_amd.mhla_causal_commit(draft, mix, state, accept) is state
    mhla_amd.mhla_causal_extend(*(_window(x, LENGTHS, accept, T_EXT) for x in (q, k, v)), mix, ref, counts=accept, left_padded=True)
    torch.cuda.synchronize()
    assert state.lengths == ref.lengths == (6, 66, 127) and torch.equal(state.pos, ref.pos)
    assert torch.equal(state.P, ref.P) and torch.equal(state.Cur, ref.Cur) and not torch.isnan(state.P).any() and not torch.isnan(state.Cur).any()
    for b, n in enumerate(state.lengths):
        assert torch.equal(state.S[b, :, :n // 64], ref.S[b, :, :n // 64]), f"sequence {b}: a finished chunk differs"


def _layers(dtype):
    from mhla_amd import modules
    torch.manual_seed(5)
    mk = lambda grouped: modules.MHLA(mode="chunk", hidden_size=256, expand_k=0.5, expand_v=1.0, num_heads=4, num_kv_heads=2,
                                      feature_map="relu", norm_eps=1e-6, layer_idx=0, exact_decoding=True, grouped_state=grouped)
    plain, grouped = mk(False), mk(True)
    with torch.no_grad():
        plain.g_norm_swish_gate.weight.uniform_(0.5, 1.5)
        plain.mixing_matrix.copy_(torch.rand(32, 32).view(32, 32, 1, 1, 1, 1))
    grouped.load_state_dict(plain.state_dict())
    return plain.to(DEV).to(dtype).eval(), grouped.to(DEV).to(dtype).eval()


@pytest.mark.parametrize("device_positions", [False, True], ids=["host-positions", "device-positions"])
def test_fla_layer_grouped_state(device_positions):
    """`MHLA(grouped_state=True)` against the same layer without it: prefill 70 tokens, three one-token calls, one 5-token call (which
    a `DecodeCache(device_positions=True)` refuses from either layer: there the three steps are the whole walk)."""
    from mhla_amd import modules
    dtype = torch.bfloat16
    plain, grouped = _layers(dtype)
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(2, 78, 256, generator=gen).to(DEV).to(dtype)
    calls = [(0, 70), (70, 71), (71, 72), (72, 73)] + ([] if device_positions else [(73, 78)])
    with torch.no_grad():
        cp, cg = modules.DecodeCache(device_positions=device_positions), modules.DecodeCache(device_positions=device_positions)
        for a, b in calls:
            poison()
            op = plain(x[:, a:b], past_key_values=cp, use_cache=True)[0]
            og = grouped(x[:, a:b], past_key_values=cg, use_cache=True)[0]
            assert not torch.isnan(og).any() and torch.equal(og, op), f"tokens {a}:{b}: the grouped layer's output differs"
        if device_positions:
            for m, c in ((plain, cp), (grouped, cg)):
                with pytest.raises(NotImplementedError, match="one token per call"):
                    m(x[:, 73:78], past_key_values=c, use_cache=True)
            cp.sync(), cg.sync()
    sp, sg = cp[0]["recurrent_state"], cg[0]["recurrent_state"]
    assert sg.S.shape[1] == 2 and sp.S.shape[1] == 4 and sg.seen == sp.seen == calls[-1][1]
    assert all(2 * getattr(sg, n).numel() == getattr(sp, n).numel() for n in ("S", "P", "Cur"))
    if not device_positions:
        assert 2 * sg.nbytes == sp.nbytes
    assert torch.equal(sg.P, sp.P[:, ::2]) and torch.equal(sg.Cur, sp.Cur[:, ::2]) and torch.equal(sg.S[:, :, :1], sp.S[:, ::2, :1])


@cases
def test_group_of_one_through_the_new_entry_points(dtype, monkeypatch):
    """Hkv = H through the *_gqa symbols (ctypes, as `ops` marshals them) against the ungrouped symbols on the same inputs: bit for bit."""
    import mhla_amd
    from mhla_amd import ops, _lib
    H = 4
    q, k, v, gate, mix, w = _stream(dtype, H, H)
    called = []

    def gqa_call(lib, name, h, hkv):
        called.append(name + "_gqa")
        return getattr(lib, name + "_gqa"), (h, hkv)

    def gqa_ws(lib, b, t, h, hkv, kk, vv, later, dt):
        assert lib.mhla_causal_extend_ragged_gqa_ws_bytes(b, t, h, hkv, kk, vv, later, dt) == lib.mhla_causal_extend_ragged_ws_bytes(b, t, h, kk, vv, later, dt)
        return lib.mhla_causal_extend_ragged_gqa_ws_bytes(b, t, h, hkv, kk, vv, later, dt)

    ang = torch.outer(torch.arange(64 * CAP, dtype=torch.float32), 1.0 / (10000 ** (torch.arange(0, K, 2, dtype=torch.float32) / K)))
    rot = (torch.cos(ang).to(dtype).to(DEV), torch.sin(ang).to(dtype).to(DEV))
    qw, kw_, vw, gw = (_window(x, LENGTHS, COUNTS, T_EXT) for x in (q, k, v, gate))
    qt, kt, vt, gt = (_tok(x, (6, 133, 127)) for x in (q, k, v, gate))

    def run(state):
        epi = dict(norm_weight=w, norm_eps=1e-6)
        rows = [mhla_amd.mhla_causal_verify(qw, kw_, vw, mix, state, counts=COUNTS, left_padded=True, gate=gw, **epi)[0]]
        rows.append(mhla_amd.mhla_causal_extend(qw, kw_, vw, mix, state, counts=COUNTS, left_padded=True, gate=gw, **epi))
        rows.append(mhla_amd.mhla_causal_step(qt, kt, vt, mix, state, gate=gt, **epi))
        rows.append(mhla_amd.mhla_causal_step_dev(qt, kt, vt, mix, state, gate=gt, **epi))
        rows.append(mhla_amd.mhla_causal_step_dev(qt, kt, vt, mix, state, gate=gt, feature_map="relu", rotary=rot, **epi))
        return rows, state.sync()

    old_state, _ = _states(k, v, mix, LENGTHS, 1)
    new_state = old_state.clone()
    poison()
    old_rows, old_state = run(old_state)
    assert not called
    monkeypatch.setattr(ops, "_gqa_call", gqa_call)
    monkeypatch.setattr(ops, "_extend_ragged_ws_bytes", gqa_ws)
    poison()
    new_rows, new_state = run(new_state)
    assert sorted(set(called)) == ["mhla_causal_extend_ragged_gqa", "mhla_causal_step_dev_gqa", "mhla_causal_step_ragged_gqa",
                                   "mhla_causal_verify_ragged_gqa"] and _lib.ABI_VERSION == 9
    for i, (a, b) in enumerate(zip(new_rows, old_rows)):
        _same_rows(f"call {i}", a, b)
    _same_state("G = 1", new_state, old_state, 1)
