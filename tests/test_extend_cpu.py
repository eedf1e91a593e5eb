"""Extending a decode state by several tokens (mhla_causal_extend), the parts that need no GPU: an fp64 restatement of the
formula (`decode_util.extend_ref`, which the GPU tests use for their state comparisons) held to the oracle, the workspace
arithmetic and the validation that runs before anything is launched."""
import pytest
import torch

from conftest import rel_err
from decode_util import extend_ref, oracle_state
from oracle import mhla_oracle as orc


RUNS = [(0, (70,)), (60, (10, 1, 57, 64, 3)), (64, (65, 130)), (37, (27, 200, 64, 1, 63))]


@pytest.mark.parametrize("start,runs", RUNS, ids=lambda x: str(x).replace(" ", ""))
@pytest.mark.parametrize("scale", [None, 0.37])
def test_extend_ref_reproduces_the_oracle(start, runs, scale):
    B, H, K, V = 2, 2, 16, 24
    T = start + sum(runs)
    L = (T + 63) // 64 + 1
    g = torch.Generator().manual_seed(start + 1)
    q, k, v = torch.randn(B, T, H, K, generator=g), torch.randn(B, T, H, K, generator=g), torch.randn(B, T, H, V, generator=g)
    mix = torch.tril(torch.rand(L, L, generator=g).clamp(1e-5, 1))
    want = orc.causal_fwd(q, k, v, mix, scale=scale)
    state = oracle_state(k, v, mix, start, L)
    t = start
    for n in runs:
        o, state = extend_ref(state, q[:, t:t + n], k[:, t:t + n], v[:, t:t + n], mix, scale)
        assert o.shape == (B, n, H, V) and state[3] == t + n
        e = (o - want[:, t:t + n].double()).abs().max().item() / want.abs().max().item()
        assert e < 1e-6, f"rows {t} .. {t + n - 1}: {e:.2e} of the oracle's maximum"
        t += n
        ref = oracle_state(k, v, mix, t, L)
        nfull = t // 64
        for name, a, b in (("S", state[0][:, :, :nfull], ref[0][:, :, :nfull]), ("P", state[1], ref[1]), ("Cur", state[2], ref[2])):
            if b.numel() and float(b.abs().max()) > 0:
                assert rel_err(a.float(), b) < 1e-6, f"{name} after {t} tokens"
            else:
                assert float(a.abs().max()) == 0.0, f"{name} after {t} tokens must be zero"


def test_extend_ref_fills_the_state_to_capacity():
    B, H, K, V = 1, 1, 8, 8
    g = torch.Generator().manual_seed(3)
    q, k, v = torch.randn(B, 128, H, K, generator=g), torch.randn(B, 128, H, K, generator=g), torch.randn(B, 128, H, V, generator=g)
    mix = torch.tril(torch.rand(2, 2, generator=g).clamp(1e-5, 1))
    o, (S, P, Cur, seen) = extend_ref(oracle_state(k, v, mix, 120, 2), q[:, 120:], k[:, 120:], v[:, 120:], mix)
    assert seen == 128 and float(P.abs().max()) == 0.0 and float(Cur.abs().max()) == 0.0
    assert rel_err(o.float(), orc.causal_fwd(q, k, v, mix)[:, 120:]) < 1e-6


def test_extend_workspace_size_is_host_arithmetic():
    from mhla_amd import _lib
    lib = _lib.load()
    ws = lambda B, T, H, K, V, pos, dt=_lib.BF16: lib.mhla_causal_extend_ws_bytes(B, T, H, K, V, pos, dt)
    B, H, K, V = 1, 4, 128, 256
    tile = 4 * K * V
    base = ws(B, 200, H, K, V, 100)
    assert base > 0 and base % 16 == 0
    # grows with the number of chunks touched: 100 + 200 touches chunks 1 .. 4, 100 + 264 chunks 1 .. 5, 100 + 8 chunk 1 alone
    assert ws(B, 264, H, K, V, 100) >= base + B * H * tile
    assert ws(B, 8, H, K, V, 100) < ws(B, 30, H, K, V, 100) < base
    assert ws(2 * B, 200, H, K, V, 100) > base and ws(B, 200, 2 * H, K, V, 100) > base
    # the same tokens from a boundary touch one chunk fewer
    assert ws(B, 192, H, K, V, 128) < ws(B, 192, H, K, V, 100)   # chunks 2 .. 4 against 1 .. 4
    for dt in (_lib.F32, _lib.F16):
        assert ws(B, 200, H, K, V, 100, dt) == base   # fp32 tiles and rows whatever the dtype
    # inside the open chunk no prefix mix is formed: the workspace is the T <= 64 fp32 rows [V] the epilogue reads alone, which is
    # at most one [K][V] tile per (b, h) for every head with K >= 64 (the shapes of the layer: 64 .. 256)
    for pos in (0, 1, 37, 100, 127):
        for T in (1, 64 - pos % 64):
            for (k_, v_) in ((128, 256), (64, 64), (256, 512)):
                assert 0 < ws(B, T, H, k_, v_, pos) <= B * H * 4 * k_ * v_, (pos, T, k_, v_)
    assert ws(B, 65, H, K, V, 0) > B * H * tile
    assert ws(0, 8, H, K, V, 0) == 0 and ws(B, 0, H, K, V, 0) == 0 and ws(B, 8, H, K, V, -1) == 0


def test_extend_validates_before_it_launches():
    import mhla_amd
    B, H, K, V, cap = 2, 3, 16, 24, 5
    s = mhla_amd.CausalState.empty(B, H, K, V, cap, device="cpu")
    s.seen = 7
    mix = torch.ones(cap, cap)
    q, k, v = torch.zeros(B, 5, H, K), torch.zeros(B, 5, H, K), torch.zeros(B, 5, H, V)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mhla_amd.mhla_causal_extend(q, k, v, mix, s)                        # CPU tensors
    with pytest.raises(ValueError, match="v has shape"):
        mhla_amd.mhla_causal_extend(q, k, v[:, :4], mix, s)                 # T of q and v differ
    with pytest.raises(TypeError, match="must be a CausalState"):
        mhla_amd.mhla_causal_extend(q, k, v, mix, state=(s.S, s.P, s.Cur))  # a wrong state type
    with pytest.raises(ValueError):
        mhla_amd.mhla_causal_extend(q, k.bfloat16(), v, mix, s)             # dtype
    with pytest.raises(RuntimeError, match="inference only"):
        mhla_amd.mhla_causal_extend(q.clone().requires_grad_(True), k, v, mix, s)
    assert s.seen == 7 and float(s.S.abs().max()) == float(s.P.abs().max()) == float(s.Cur.abs().max()) == 0.0
