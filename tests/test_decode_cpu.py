"""Decoding support of the causal operator, the parts that need no GPU: workspace arithmetic, the state container, the cache
protocol and the layer's flag."""
import pytest
import torch


def test_step_workspace_size_is_host_arithmetic():
    from mhla_amd import _lib
    lib = _lib.load()
    ws = lambda B, H, K, V: lib.mhla_causal_step_ws_bytes(B, H, K, V, _lib.BF16)
    base = ws(1, 4, 128, 256)
    assert base > 0 and base % 16 == 0
    assert ws(2, 4, 128, 256) > base and ws(1, 8, 128, 256) > base and ws(1, 4, 128, 512) > base
    assert ws(32, 4, 256, 512) >= 32 * 4 * 512 * 4          # at least one fp32 partial row of V per (b, h)
    assert ws(1, 4, 128, 256) == lib.mhla_causal_step_ws_bytes(1, 4, 128, 256, _lib.F32)   # fp32 partials whatever the dtype


def test_causal_state_container():
    import mhla_amd
    B, H, K, V, cap = 2, 3, 16, 24, 5
    s = mhla_amd.CausalState.empty(B, H, K, V, cap, device="cpu")
    assert s.S.shape == (B, H, cap, K, V) and s.P.shape == s.Cur.shape == (B, H, K, V)
    assert s.S.dtype == s.P.dtype == s.Cur.dtype == torch.float32
    assert s.seen == 0 and s.chunk_size == 64 and s.capacity_chunks == cap
    assert float(s.S.abs().max()) == float(s.P.abs().max()) == float(s.Cur.abs().max()) == 0.0
    assert s.nbytes == 4 * B * H * K * V * (cap + 2)
    s.seen = 7
    s.Cur += 1
    c = s.clone()
    assert c.seen == 7 and c.chunk_size == 64 and torch.equal(c.Cur, s.Cur) and c.Cur.data_ptr() != s.Cur.data_ptr()
    c.Cur += 1
    c.seen = 8
    assert s.seen == 7 and float(s.Cur.max()) == 1.0
    with pytest.raises(ValueError):
        mhla_amd.CausalState.empty(B, H, K, V, 0, device="cpu")
    # the step validates before it launches: a CPU token is refused, the state stays as it was
    q, k, v = torch.zeros(B, 1, H, K), torch.zeros(B, 1, H, K), torch.zeros(B, 2, H, V)
    with pytest.raises(ValueError):
        mhla_amd.mhla_causal_step(q, k, v, torch.ones(cap, cap), s)
    with pytest.raises(TypeError):
        mhla_amd.mhla_causal_step(q, k, v[:, :1], torch.ones(cap, cap), state=None)
    assert s.seen == 7


def test_decode_cache_protocol():
    from mhla_amd.modules import DecodeCache
    c = DecodeCache()
    assert len(c) == 0 and c.get_seq_length() == 0 and c.get_seq_length(3) == 0
    c.update(recurrent_state="s0", conv_state=None, layer_idx=0, offset=5)
    assert len(c) == 1 and c[0] == {"recurrent_state": "s0", "conv_state": None} and c.get_seq_length(0) == 5
    c.update(recurrent_state="s1", conv_state=("a", "b", "c"), layer_idx=1, offset=5)
    c.update(recurrent_state="s0'", layer_idx=0, offset=1)
    assert len(c) == 2 and c.get_seq_length(0) == 6 and c.get_seq_length(1) == 5 and c.get_seq_length() == 6
    assert c[0]["recurrent_state"] == "s0'" and c[1]["conv_state"] == ("a", "b", "c")
    with pytest.raises(IndexError):
        c[2]


def test_exact_decoding_flag_adds_no_parameters():
    from mhla_amd.modules import MHLA
    kw = dict(mode="chunk", hidden_size=128, expand_k=0.5, expand_v=1.0, num_heads=2, feature_map="relu")
    a, b = MHLA(exact_decoding=False, **kw), MHLA(exact_decoding=True, **kw)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    assert MHLA(**kw).exact_decoding is False and b.exact_decoding is True
    b.load_state_dict(a.state_dict(), strict=True)


def test_gpt_host_accepts_the_flag():
    from mhla_amd.hosts.gpt import GPT_MHLA
    kw = dict(vocab_size=64, hidden_size=128, num_layers=1, num_heads=4)
    a, b = GPT_MHLA(**kw), GPT_MHLA(exact_decoding=True, **kw)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    assert not a.layers[0].attn.exact_decoding and b.layers[0].attn.exact_decoding and hasattr(b, "generate")
