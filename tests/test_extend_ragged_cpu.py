"""Extending a ragged decode state by a token count per sequence (mhla_causal_extend(..., counts=)), the parts that need no
GPU: a per-sequence restatement (`decode_util.extend_ragged_ref`, `extend_ref` applied to every sequence's own window, which
the GPU tests use) held to the oracle, the workspace arithmetic of the ragged entry point and the validation that runs before
the device check."""
import pytest
import torch

from conftest import rel_err
from decode_util import TABLE, TABLE_CAP, TABLE_T, extend_ragged_ref, oracle_state, start_state, table_inputs, window
from oracle import mhla_oracle as orc

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
