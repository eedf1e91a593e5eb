"""Shared by the decode-family tests (prefill / step, extend, ragged, ragged extend, speculative verify / commit, grouped-query
heads, the device-positioned step, packed prefill): the fp64 references and their tables, the seeded inputs, views and windows, and
the state checks.  The references need no GPU (tests/test_extend_cpu.py, test_extend_ragged_cpu.py and test_speculative_cpu.py hold
them to the oracle); `mhla_amd` is imported only inside the helpers that call it.  Nothing here is used by one file alone."""
import functools

import torch

from gpu_util import DEV, CAUSAL_TOL, TOL, check, check_chunks
from oracle import mhla_oracle as orc

NAN = float("nan")


# -------------------------------------------------------------------------------------------------
# references (CPU)
# -------------------------------------------------------------------------------------------------
def extend_ref(state, q, k, v, mix, scale=None):
    """`state` = (S [B, H, cap, K, V], P [B, H, K, V], Cur [B, H, K, V], seen); q, k [B, T, H, K], v [B, T, H, V]; chunk 64.
    Returns (o [B, T, H, V], (S, P, Cur, seen) after the T tokens), all fp64, by the segment formula: with i = seen / 64,
    r = seen % 64 a segment is a run of new tokens inside one chunk c,
        O = scale (Q (P_c + m_cc Cur_before) + m_cc tril(Q K^T) V),  Cur = Cur_before + K^T V,
        chunk full: S[c] = Cur, Cur = 0, P_{c+1} = sum_{j<=c} mix[c+1][j] S[j]  (0 when c + 1 == capacity)."""
    S, P, Cur, seen = state
    S, P, Cur = S.double().clone(), P.double().clone(), Cur.double().clone()
    m = mix.reshape(mix.shape[0], mix.shape[1]).double()
    cap = S.shape[2]
    qh, kh, vh = (t.double().permute(0, 2, 1, 3) for t in (q, k, v))
    T, K = qh.shape[2], qh.shape[3]
    scale = K ** -0.5 if scale is None else scale
    outs, t = [], 0
    while t < T:
        c, r = divmod(seen, 64)
        assert c < cap, "the state is full"
        a = min(T - t, 64 - r)
        Q, Kc, Vc = qh[:, :, t:t + a], kh[:, :, t:t + a], vh[:, :, t:t + a]
        A = torch.tril(Q @ Kc.transpose(-1, -2))
        outs.append(scale * (Q @ (P + m[c, c] * Cur) + m[c, c] * (A @ Vc)))
        Cur = Cur + Kc.transpose(-1, -2) @ Vc
        t, seen = t + a, seen + a
        if seen % 64 == 0:
            S[:, :, c] = Cur
            Cur = torch.zeros_like(Cur)
            P = torch.einsum("j,bhjkv->bhkv", m[c + 1, :c + 1], S[:, :, :c + 1]) if c + 1 < cap else torch.zeros_like(P)
    return torch.cat(outs, dim=2).permute(0, 2, 1, 3), (S, P, Cur, seen)


def oracle_state(k, v, mix, seen, cap):
    """The state after `seen` tokens from the oracle's chunk summaries (fp32)."""
    B, _, H, K = k.shape
    V = v.shape[-1]
    S = torch.zeros(B, H, cap, K, V)
    P, Cur = torch.zeros(B, H, K, V), torch.zeros(B, H, K, V)
    if seen:
        # (one more token than `seen` on a boundary, so that the oracle forms the open chunk's prefix mix)
        n = seen + (1 if seen % 64 == 0 else 0)
        z, kk, vv = torch.zeros(B, n, H, K), torch.zeros(B, n, H, K), torch.zeros(B, n, H, V)
        kk[:, :seen], vv[:, :seen] = k[:, :seen].float(), v[:, :seen].float()
        _, aux = orc.causal_fwd(z, kk, vv, mix, return_aux=True)
        nfull = seen // 64
        S[:, :, :nfull] = aux["S"][:, :, :nfull]
        if nfull < cap:
            Cur, P = aux["S"][:, :, nfull].clone(), aux["P"][:, :, nfull].clone()
    return S, P, Cur, seen


# (pos, n) of one batch, capacity 4 chunks, padded width 130: every branch of the per-sequence plan beside every other
TABLE = [(60, 10),    # crosses a boundary
         (0, 0),      # an idle slot
         (63, 1),     # closes on its only row
         (64, 130),   # starts on a boundary, then two whole chunks and a tail
         (37, 27),    # lands exactly on a boundary: Cur = 0, P the next chunk's
         (5, 3),      # stays inside its chunk
         (0, 70),     # an empty state used as a prefill
         (192, 64)]   # fills the state: P = Cur = 0
TABLE_T, TABLE_CAP, TABLE_L = 130, 4, 5   # (one row of the matrix more than the capacity: the oracle opens chunk 4 for its summaries)


def window(T, n, left_padded):
    """Rows of the padded [B, T, ...] tensors that hold a sequence's n tokens."""
    t0 = T - n if left_padded else 0
    return slice(t0, t0 + n)


def extend_ragged_ref(state, q, k, v, mix, counts, left_padded=False, scale=None):
    """`state` = (S [B, H, cap, K, V], P, Cur [B, H, K, V], lengths); q, k [B, T, H, K], v [B, T, H, V] padded; sequence b takes
    `counts[b]` tokens -- rows [0, n) or, left-padded, [T - n, T) -- at position lengths[b]: `extend_ref` on every sequence alone.
    Returns (o [B, T, H, V] fp64, zeros outside every window, (S, P, Cur, lengths) afterwards, fp64).  Padding rows are never read."""
    S, P, Cur, lengths = state
    S, P, Cur = S.double().clone(), P.double().clone(), Cur.double().clone()
    B, T, H, _ = q.shape
    o = torch.zeros(B, T, H, v.shape[-1], dtype=torch.float64)
    out_len = []
    for b, (p, n) in enumerate(zip(lengths, counts)):
        out_len.append(p + n)
        if not n:
            continue
        w = window(T, n, left_padded)
        ob, (Sb, Pb, Cb, seen) = extend_ref((S[b:b + 1], P[b:b + 1], Cur[b:b + 1], p), q[b:b + 1, w], k[b:b + 1, w], v[b:b + 1, w], mix, scale)
        assert seen == p + n
        o[b:b + 1, w], S[b:b + 1], P[b:b + 1], Cur[b:b + 1] = ob, Sb, Pb, Cb
    return o, (S, P, Cur, tuple(out_len))


def table_inputs(H, K, V, dtype=torch.float32, table=TABLE, T=TABLE_T, L=TABLE_L, seed=77, left_padded=False):
    """Per sequence of `table` its whole history of pos + n tokens (q, k with signs as roped feature maps have them, rounded to
    `dtype`), the padded tensors of the extension with NaN in every padding row, and a random lower-triangular mix [L, L]."""
    g = torch.Generator().manual_seed(seed)
    mix = torch.tril(torch.rand(L, L, generator=g).clamp(1e-5, 1))
    hist = []
    B = len(table)
    q, k = (torch.full((B, T, H, K), float("nan")).to(dtype) for _ in range(2))
    v = torch.full((B, T, H, V), float("nan")).to(dtype)
    for b, (p, n) in enumerate(table):
        m = max(p + n, 1)
        qs = (torch.relu(torch.randn(1, m, H, K, generator=g)) * torch.sign(torch.randn(1, m, H, K, generator=g))).to(dtype)
        ks = (torch.relu(torch.randn(1, m, H, K, generator=g)) * torch.sign(torch.randn(1, m, H, K, generator=g))).to(dtype)
        vs = torch.randn(1, m, H, V, generator=g).to(dtype)
        hist.append((qs, ks, vs))
        w = window(T, n, left_padded)
        q[b, w], k[b, w], v[b, w] = qs[0, p:p + n], ks[0, p:p + n], vs[0, p:p + n]
    return hist, q, k, v, mix


def start_state(hist, table, mix, cap):
    """The batch's state before the extension, sequence by sequence from the oracle's summaries (fp32)."""
    parts = [oracle_state(ks.float(), vs.float(), mix, p, cap) for (_, ks, vs), (p, _) in zip(hist, table)]
    return tuple(torch.cat([x[i] for x in parts]) for i in range(3)) + (tuple(p for p, _ in table),)


# (pos, n, accept) of one batch, capacity 4 chunks, padded width 130, a 5 x 5 matrix
SPEC_TABLE = [(60, 10, 0),     # all rejected after the verify crossed a boundary
              (60, 10, 3),     # accepted inside the open chunk
              (60, 10, 4),     # accepted exactly closes the chunk
              (60, 10, 10),
              (0, 0, 0),       # idle
              (63, 1, 1),
              (63, 1, 0),
              (64, 130, 70),   # whole chunks, ends inside a later one
              (5, 3, 2),
              (0, 70, 64),     # an empty state
              (192, 64, 64),   # fills the state: P = Cur = 0
              (192, 64, 63)]
SPEC_T, SPEC_CAP, SPEC_L = 130, 4, 5
DRAFTS = tuple((p, n) for p, n, _ in SPEC_TABLE)
COUNTS = tuple(n for _, n, _ in SPEC_TABLE)
ACCEPT = tuple(a for _, _, a in SPEC_TABLE)


def verify_ref(state, q, k, v, mix, counts, left_padded=False, scale=None):
    """(the rows `extend_ragged_ref` gives, the INPUT state): a verify commits nothing."""
    return extend_ragged_ref(state, q, k, v, mix, counts, left_padded, scale)[0], state


def commit_ref(state, k, v, mix, counts, accept, left_padded=False):
    """The state after the first accept[b] rows of every sequence's counts[b]-row window: `extend_ragged_ref(counts=accept)` on the
    accepted rows, moved to where a window of accept[b] rows lies."""
    B, T = k.shape[:2]
    ka, va = torch.zeros_like(k), torch.zeros_like(v)
    for b, (n, a) in enumerate(zip(counts, accept)):
        assert 0 <= a <= n
        src = window(T, n, left_padded)
        dst = window(T, a, left_padded)
        ka[b, dst], va[b, dst] = k[b, src.start:src.start + a], v[b, src.start:src.start + a]
    return extend_ragged_ref(state, torch.zeros_like(ka), ka, va, mix, accept, left_padded)[1]


# -------------------------------------------------------------------------------------------------
# inputs
# -------------------------------------------------------------------------------------------------
def signed_features(g, *shape):
    """relu(randn) with random signs: q, k as roped feature maps have them (two draws from `g`, the magnitudes first)."""
    return torch.relu(torch.randn(*shape, generator=g)) * torch.sign(torch.randn(*shape, generator=g))


@functools.lru_cache(maxsize=None)
def decode_inputs(B, T, H, K, V, L, dtype, seed=1234, scale=None):
    """q, k with signs as roped feature maps have them, random lower-triangular mix; the fp32 oracle (output and summaries) of
    the dtype-rounded tensors, computed once per case."""
    g = torch.Generator().manual_seed(seed)
    q = signed_features(g, B, T, H, K).to(dtype)
    k = signed_features(g, B, T, H, K).to(dtype)
    v = torch.randn(B, T, H, V, generator=g).to(dtype)
    mix = torch.tril(torch.rand(L, L, generator=g).clamp(1e-5, 1))
    want = orc.causal_fwd(q.float(), k.float(), v.float(), mix, scale=scale)
    return q, k, v, mix, want


@functools.lru_cache(maxsize=None)
def ragged_inputs(lengths, n, H, K, V, L, dtype, seed=1234):
    """B sequences on timelines of their own: sequence b's tokens are rows [0, lengths[b] + n] of q[b], k[b], v[b] (one more than
    the n decoded ones, for the state check on a boundary).  q, k with signs as roped feature maps have them, a random lower-
    triangular mix; the fp32 oracle of every sequence alone over its lengths[b] + n tokens, computed once per case."""
    B, T = len(lengths), max(lengths) + n + 1
    g = torch.Generator().manual_seed(seed)
    q = signed_features(g, B, T, H, K).to(dtype)
    k = signed_features(g, B, T, H, K).to(dtype)
    v = torch.randn(B, T, H, V, generator=g).to(dtype)
    mix = torch.tril(torch.rand(L, L, generator=g).clamp(1e-5, 1))
    want = tuple(orc.causal_fwd(q[b:b + 1, :m + n].float(), k[b:b + 1, :m + n].float(), v[b:b + 1, :m + n].float(), mix)
                 for b, m in enumerate(lengths))
    return q, k, v, mix, want


def layer_inputs(B, T, seed):
    return torch.randn(B, T, 256, generator=torch.Generator().manual_seed(seed))


# the (dtype, H, K, V) of the ragged-extend and speculative tests
SHAPES = [(torch.float32, 2, 16, 24),      # below one tile
          (torch.float32, 2, 80, 72),      # not multiples of 64
          (torch.bfloat16, 2, 64, 128),
          (torch.float16, 2, 64, 64)]
SHAPE_IDS = ["fp32-K16V24", "fp32-K80V72", "bf16-K64V128", "fp16-K64V64"]


# -------------------------------------------------------------------------------------------------
# views and windows
# -------------------------------------------------------------------------------------------------
def packed_views(qt, kt, vt):
    """q, k, v of the T tokens as strided slices of ONE packed projection output [B, T, H * (2 K + V)]."""
    B, T, H, K = qt.shape
    V = vt.shape[-1]
    packed = torch.cat([qt, kt, vt], dim=-1).reshape(B, T, H * (2 * K + V)).contiguous().view(B, T, H, 2 * K + V)
    views = packed[..., :K], packed[..., K:2 * K], packed[..., 2 * K:]
    assert not views[1].is_contiguous() and views[1].data_ptr() != packed.data_ptr()
    return views


def left_padded(x, lengths):
    """[B, max(lengths), ...]: sequence b's first lengths[b] rows at the END of row b, NaN (never to be read) before them."""
    T = max(lengths)
    out = torch.full((len(lengths), T) + tuple(x.shape[2:]), float("nan"), dtype=x.dtype, device=x.device)
    for b, m in enumerate(lengths):
        if m:
            out[b, T - m:] = x[b, :m]
    return out


def window_rows(x, lengths, t0, n):
    """[B, n, ...]: rows lengths[b] + t0 .. of every sequence (the tokens the next n steps take)."""
    return torch.stack([x[b, m + t0:m + t0 + n] for b, m in enumerate(lengths)])


# -------------------------------------------------------------------------------------------------
# ragged states: how the tests make and advance them
# -------------------------------------------------------------------------------------------------
def ragged_prefill(q, k, v, mix, lengths, how, cap=None):
    """(prefill rows per sequence, ragged state) through `lengths=` on a left-padded batch, or `CausalState.cat` of B = 1 prefills."""
    import mhla_amd
    if how == "left_padded":
        T = max(lengths)
        o, state = mhla_amd.mhla_causal_prefill(*(left_padded(t, lengths) for t in (q, k, v)), mix, lengths=list(lengths), left_padded=True,
                                                capacity_chunks=cap)
        for b, m in enumerate(lengths):
            assert float(o[b, :T - m].abs().max() if m < T else 0.0) == 0.0, f"padding rows of sequence {b} are not zero"
        return [o[b:b + 1, T - m:] for b, m in enumerate(lengths)], state
    parts = [mhla_amd.mhla_causal_prefill(q[b:b + 1, :m], k[b:b + 1, :m], v[b:b + 1, :m], mix, capacity_chunks=cap) for b, m in enumerate(lengths)]
    return [o for o, _ in parts], mhla_amd.CausalState.cat([s for _, s in parts])


def ragged_steps(q, k, v, mix, state, lengths, t0, n, views=None, **kw):
    import mhla_amd
    qs, ks, vs = (window_rows(t, lengths, t0, n) for t in (q, k, v))
    outs = []
    for t in range(n):
        qt, kt, vt = (views or (lambda *a: a))(qs[:, t:t + 1], ks[:, t:t + 1], vs[:, t:t + 1])
        outs.append(mhla_amd.mhla_causal_step(qt, kt, vt, mix, state, **{a: (b[:, t:t + 1] if a == "gate" else b) for a, b in kw.items()}))
    return torch.cat(outs, dim=1)


def ragged_start(table, hist, mix, cap=TABLE_CAP):
    """The ragged state of the batch before the extension: `mhla_causal_state(lengths=)` over the right-padded histories."""
    import mhla_amd
    B, T0 = len(table), max(max(p for p, _ in table), 1)
    _, k0, v0 = hist[0]
    k = torch.zeros(B, T0, *k0.shape[2:], dtype=k0.dtype)
    v = torch.zeros(B, T0, *v0.shape[2:], dtype=v0.dtype)
    for b, (p, _) in enumerate(table):
        k[b, :p], v[b, :p] = hist[b][1][0, :p], hist[b][2][0, :p]
    state = mhla_amd.mhla_causal_state(k.to(DEV), v.to(DEV), mix.to(DEV), lengths=[p for p, _ in table], capacity_chunks=cap)
    assert state.lengths == tuple(p for p, _ in table)
    return state


def one_sequence(state, b):
    """Sequence b of a ragged state as a uniform state of a batch of one (a copy)."""
    import mhla_amd
    return mhla_amd.CausalState(state.S[b:b + 1].clone(), state.P[b:b + 1].clone(), state.Cur[b:b + 1].clone(), state.lengths[b], 64)


def cpu_state(state):
    """(S, P, Cur, seen) of a uniform state, (S, P, Cur, lengths) of a ragged one, on the CPU: what extend_ref / extend_ragged_ref take."""
    return state.S.cpu(), state.P.cpu(), state.Cur.cpu(), state.seen if state.lengths is None else state.lengths


# -------------------------------------------------------------------------------------------------
# checks
# -------------------------------------------------------------------------------------------------
def check_step_rows(name, got, want, m, dtype):
    """Rows m .. of one sequence: within CAUSAL_TOL of the sequence's maximum, and chunk by chunk of the sequence's OWN chunks (the
    rows up to its next boundary, then whole chunks) within CAUSAL_TOL of each chunk's maximum: step rows come from the fp32 state."""
    ref = want[:, m:]
    check(name, got, ref, CAUSAL_TOL[dtype])
    first = min(got.shape[1], 64 - m % 64)
    check_chunks(f"{name} (open chunk)", got[:, :first], ref[:, :first], CAUSAL_TOL[dtype])
    if first < got.shape[1]:
        check_chunks(name, got[:, first:], ref[:, first:], CAUSAL_TOL[dtype])


def check_state(state, q, k, v, mix, name, b=None, s=None):
    """S, P, Cur against the oracle's summaries of the tokens seen so far (fp32 state whatever the tensor dtype).  With `b`:
    sequence b of a ragged state, against that sequence's own first `s` tokens."""
    rows = slice(None) if b is None else slice(b, b + 1)
    s = state.seen if s is None else s
    nfull, tail = s // 64, s % 64
    f = lambda t, n: t[rows, :n].float().cpu()
    tol = TOL[torch.float32]
    S, P, Cur = state.S[rows], state.P[rows], state.Cur[rows]
    assert S.dtype == P.dtype == Cur.dtype == torch.float32
    _, aux = orc.causal_fwd(f(q, s), f(k, s), f(v, s), mix.cpu(), return_aux=True) if s else (None, None)
    if nfull:
        check(f"{name}: S", S[:, :, :nfull], aux["S"][:, :, :nfull], tol)
    if tail:
        check(f"{name}: Cur", Cur, aux["S"][:, :, nfull], tol)
        if nfull:
            check(f"{name}: P", P, aux["P"][:, :, nfull], tol)
        else:
            assert float(P.abs().max()) == 0.0
    else:
        assert float(Cur.abs().max()) == 0.0, f"{name}: Cur on a boundary must be exactly 0"
        if nfull == state.capacity_chunks:
            assert float(P.abs().max()) == 0.0   # a full state has no open chunk
        elif s + 1 <= q.shape[1]:   # on a boundary: the prefix mix the NEXT token will read
            _, aux1 = orc.causal_fwd(f(q, s + 1), f(k, s + 1), f(v, s + 1), mix.cpu(), return_aux=True)
            check(f"{name}: P (boundary)", P, aux1["P"][:, :, nfull], tol, atol=1e-30 if nfull == 0 else 0.0)


def close_or_zero(name, got, want, tol):
    w = want.float().cpu()
    if w.numel() == 0:
        return
    if float(w.abs().max()) == 0.0:
        assert float(got.abs().max()) == 0.0, f"{name} must be exactly zero"
    else:
        check(name, got, w, tol)


def same_state(name, a, b, tol=None):
    """States a, b (a CausalState, or extend_ref's tuple): finished chunks, P and Cur equal (tol None: bit for bit)."""
    ta = (a.S, a.P, a.Cur, a.seen) if hasattr(a, "seen") else a
    tb = (b.S, b.P, b.Cur, b.seen) if hasattr(b, "seen") else b
    assert ta[3] == tb[3]
    nfull = ta[3] // 64
    for part, x, y in (("S", ta[0][:, :, :nfull], tb[0][:, :, :nfull]), ("P", ta[1], tb[1]), ("Cur", ta[2], tb[2])):
        if tol is None:
            assert torch.equal(x, y), f"{name}: {part} differs"
        else:
            close_or_zero(f"{name}: {part}", x, y, tol)


def same_seq_state(name, a, ia, b, ib, seen):
    """Sequence ia of state a and ib of b: finished chunks, P and Cur bit for bit."""
    nfull = seen // 64
    for part in ("S", "P", "Cur"):
        x, y = getattr(a, part)[ia], getattr(b, part)[ib]
        if part == "S":
            x, y = x[:, :nfull], y[:, :nfull]
        assert torch.equal(x, y), f"{name}: {part} differs"


def padding_is_zero(o, counts, left_padded):
    T = o.shape[1]
    for b, n in enumerate(counts):
        pad = torch.ones(T, dtype=torch.bool)
        pad[window(T, n, left_padded)] = False
        if bool(pad.any()):
            assert float(o[b].cpu()[pad].float().abs().max()) == 0.0, f"sequence {b}: padding rows must be exactly zero"


def unchanged(state, keep):
    torch.cuda.synchronize()
    assert state.lengths == keep.lengths and state.seen == keep.seen and torch.equal(state.pos, keep.pos)
    assert torch.equal(state.S, keep.S) and torch.equal(state.P, keep.P) and torch.equal(state.Cur, keep.Cur)
