"""Extending a ragged decode state by a token count per sequence (mhla_causal_extend(..., counts=)), the parts that need no
GPU: a per-sequence restatement (`extend_ragged_ref`, test_extend_cpu.extend_ref applied to every sequence's own window, which
the GPU tests import) held to the oracle, the workspace arithmetic of the ragged entry point and the validation that runs before
the device check."""
import pytest
import torch

from conftest import rel_err
from oracle import mhla_oracle as orc
from test_extend_cpu import extend_ref, oracle_state

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


@pytest.mark.parametrize("left_padded", [False, True], ids=["right-padded", "left-padded"])
@pytest.mark.parametrize("scale", [None, 0.37])
def test_extend_ragged_ref_reproduces_the_oracle(left_padded, scale):
    H, K, V = 2, 16, 24
    hist, q, k, v, mix = table_inputs(H, K, V, left_padded=left_padded)
    counts = tuple(n for _, n in TABLE)
    o, (S, P, Cur, lengths) = extend_ragged_ref(start_state(hist, TABLE, mix, TABLE_CAP), q, k, v, mix, counts, left_padded, scale)
    assert lengths == tuple(p + n for p, n in TABLE) and bool(torch.isfinite(o).all())
    for b, (p, n) in enumerate(TABLE):
        w = window(TABLE_T, n, left_padded)
        pad = torch.ones(TABLE_T, dtype=torch.bool)
        pad[w] = False
        assert not bool(pad.any()) or float(o[b, pad].abs().max()) == 0.0, f"sequence {b}: padding rows must be zero"
        qs, ks, vs = hist[b]
        if n:
            want = orc.causal_fwd(qs, ks, vs, mix, scale=scale)[0, p:p + n]
            e = (o[b, w] - want.double()).abs().max().item() / want.abs().max().item()
            assert e < 1e-6, f"sequence {b} (pos {p}, n {n}): {e:.2e} of the oracle's maximum"
        ref = oracle_state(ks, vs, mix, p + n, TABLE_CAP)
        nfull = (p + n) // 64
        for name, a, r in (("S", S[b:b + 1, :, :nfull], ref[0][:, :, :nfull]), ("P", P[b:b + 1], ref[1]), ("Cur", Cur[b:b + 1], ref[2])):
            if r.numel() and float(r.abs().max()) > 0:
                assert rel_err(a.float(), r) < 1e-6, f"sequence {b}: {name} after {p + n} tokens"
            elif a.numel():
                assert float(a.abs().max()) == 0.0, f"sequence {b}: {name} after {p + n} tokens must be zero"


def test_extend_ragged_workspace_size_is_host_arithmetic():
    from mhla_amd import _lib
    lib = _lib.load()
    ws = lambda B, T, H, K, V, later, dt=_lib.BF16: lib.mhla_causal_extend_ragged_ws_bytes(B, T, H, K, V, later, dt)
    al4 = lambda n: (n + 3) & ~3
    # in 4-byte words: a [K][V] tile per (b, h) and later chunk of the longest sequence, a row [V] per (b, h) and padded token, B ints
    for (B, T, H, K, V, later) in ((8, 130, 2, 16, 24, 3), (8, 256, 4, 128, 256, 4), (3, 1, 1, 4, 4, 0), (5, 77, 3, 80, 72, 2)):
        want = 4 * (al4(B * H * later * K * V) + al4(B * H * T * V) + al4(B))
        assert ws(B, T, H, K, V, later) == want and want % 16 == 0
        for dt in (_lib.F32, _lib.F16):
            assert ws(B, T, H, K, V, later, dt) == want   # fp32 tiles and rows whatever the dtype
    assert ws(0, 8, 2, 16, 24, 1) == 0 and ws(2, 0, 2, 16, 24, 1) == 0 and ws(2, 8, 2, 16, 24, -1) == 0 and ws(2, 8, 2, 0, 24, 1) == 0
    assert ws(2, 8, -1, 16, 24, 1) == 0 and ws(2, 8, 2, 16, 0, 1) == 0


def test_counts_are_validated_before_the_device_check():
    import mhla_amd
    B, H, K, V, cap, T = 3, 2, 16, 24, 4, 5
    z = lambda *s: torch.zeros(s)
    mix = torch.ones(cap + 1, cap + 1)
    q, k, v = z(B, T, H, K), z(B, T, H, K), z(B, T, H, V)

    def ragged(lengths):
        s = mhla_amd.CausalState(z(B, H, cap, K, V), z(B, H, K, V), z(B, H, K, V), 0, 64, lengths=lengths)
        s.Cur.fill_(0.5)
        return s

    def untouched(s, lengths):
        assert s.lengths == tuple(lengths) and s.seen == max(lengths) and s.pos.tolist() == list(lengths) and not s.stale
        assert float(s.S.abs().max()) == 0.0 and float(s.P.abs().max()) == 0.0 and bool((s.Cur == 0.5).all())

    L0 = (7, 100, 64 * cap - 2)
    s = ragged(L0)
    ext = lambda counts, state=s, m=mix, **kw: mhla_amd.mhla_causal_extend(q, k, v, m, state, counts=counts, **kw)
    with pytest.raises(ValueError, match="counts has 2 entries, expected B=3"):
        ext([1, 2])
    with pytest.raises(ValueError, match=r"must be in 0 \.\. T=5"):
        ext([1, 6, 0])
    with pytest.raises(ValueError, match=r"must be in 0 \.\. T=5"):
        ext(torch.tensor([1, -1, 0]))
    # the capacity: sequence 2 has room for two tokens
    with pytest.raises(IndexError, match=r"sequences \[2\].*the state holds only 4"):
        ext([5, 5, 3])
    with pytest.raises(IndexError, match=r"sequences \[1, 2\].*mixing_matrix has only 1 rows"):
        ext([5, 5, 2], m=torch.ones(1, 1))
    # what fits passes every check and reaches the device check: CPU tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ext([5, 0, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ext([0, 0, 0], left_padded=True)
    untouched(s, L0)
    # a uniform state has no positions on the device
    u = mhla_amd.CausalState.empty(B, H, K, V, cap, device="cpu")
    u.seen = 7
    with pytest.raises(ValueError, match=r"to_ragged\(\)"):
        ext([1, 1, 1], state=u)
    assert u.seen == 7 and u.lengths is None
    # a state whose host mirror is behind the device
    st = ragged(L0)
    st.stale = True
    with pytest.raises(ValueError, match="stale"):
        ext([1, 1, 1], state=st)
    st.stale = False
    untouched(st, L0)
    # B of the state and of the tokens
    with pytest.raises(ValueError):
        mhla_amd.mhla_causal_extend(q[:2], k[:2], v[:2], mix, s, counts=[1, 1])
    untouched(s, L0)
