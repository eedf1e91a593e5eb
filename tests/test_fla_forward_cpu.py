"""The fla layer's refusals, the parts of `MHLA.forward` that need no GPU: every refusal's exception type and message, whether
`mixing_matrix.data` was clamped when it fired (the device-positioned refusals fire before the clamp, all others after), that the
cache and its states are untouched, which refusal wins when two conditions hold, and the two warnings (text, category, once per
layer, the frame they are attributed to)."""
import warnings

import pytest
import torch

MASK = torch.tensor([[0, 1, 1], [1, 1, 1]])           # left-padded over a call of 3 tokens
RIGHT = torch.tensor([[1, 1, 0], [1, 1, 1]])


def _layer(hidden=64, **kw):
    from mhla_amd.modules.fla import MHLA
    m = MHLA(**{**dict(hidden_size=hidden, num_heads=2, feature_map="relu", layer_idx=0, exact_decoding=True), **kw})
    with torch.no_grad():
        m.mixing_matrix.fill_(2.0)                    # (outside the clamp's range: a clamp is visible)
    return m


def _cache(state=None, device_positions=False):
    """A DecodeCache; `state`: "uniform" / "ragged" stores a CausalState of B = 2, H = 2, K = 16, V = 32 as layer 0's, 7 tokens counted."""
    from mhla_amd import CausalState
    from mhla_amd.modules.fla import DecodeCache
    cache = DecodeCache(device_positions=device_positions)
    if state is not None:
        st = CausalState.empty(2, 2, 16, 32, 4, "cpu")
        cache.update(recurrent_state=st.to_ragged() if state == "ragged" else st, layer_idx=0, offset=7)
    return cache


def _refused(m, cache, exc, match, clamped, T=3, **kw):
    st = cache[0]["recurrent_state"] if len(cache) else None
    before = (len(cache), cache.get_seq_length(0), None if st is None else (st.seen, st.lengths, st.stale))
    snap = None if st is None else st.clone()
    x = torch.randn(2, T, m.hidden_size, generator=torch.Generator().manual_seed(1))
    with pytest.raises(exc, match=match):
        m(x, past_key_values=cache, use_cache=True, **kw)
    assert bool((m.mixing_matrix.data == 2.0).all()) == (not clamped), "clamped" if not clamped else "not clamped"
    if clamped:
        assert bool((m.mixing_matrix.data == 1.0).all())   # (clamp(2, 1e-5, 1); tril() acts on the two trailing axes of size 1)
    assert before == (len(cache), cache.get_seq_length(0), None if st is None else (st.seen, st.lengths, st.stale))
    if st is not None:
        assert cache[0]["recurrent_state"] is st and cache[0]["conv_state"] is None
        assert all(torch.equal(getattr(st, n), getattr(snap, n)) for n in ("S", "P", "Cur"))
        assert st.pos is None or torch.equal(st.pos, snap.pos)


# (layer options, cache, call keywords, exception, a distinctive part of the message, clamped when it fires)
REFUSALS = {
    "dev-layer_idx-none": (dict(layer_idx=None), dict(device_positions=True), {}, ValueError, "indexed by layer_idx, which is None", False),
    "dev-short-conv": (dict(use_short_conv=True), dict(device_positions=True), {}, NotImplementedError,
                       r"device_positions=True\) with use_short_conv", False),
    "dev-head_k_dim": (dict(hidden=48), dict(device_positions=True), {}, NotImplementedError, r"needs head_k_dim % 8 == 0 .*got 12", False),
    "dev-several-tokens": ({}, dict(device_positions=True, state="ragged"), dict(T=5), NotImplementedError,
                           r"a call of 5 tokens on a DecodeCache\(device_positions=True\) that holds a state", False),
    "isolate-with-cache": (dict(isolate_sequences=True), {}, dict(attention_mask=MASK), NotImplementedError,
                           r"isolate_sequences=True\): an attention_mask or cu_seqlens with use_cache", True),
    "exact-layer_idx-none": (dict(layer_idx=None), {}, {}, ValueError, "indexed by layer_idx, which is None", True),
    "uniform-state-with-mask": ({}, dict(state="uniform"), dict(attention_mask=MASK), NotImplementedError,
                                "the cached decode state is uniform", True),
    "short-conv-with-mask": (dict(use_short_conv=True), {}, dict(attention_mask=MASK), NotImplementedError,
                             "use_short_conv with a padding attention_mask", True),
    "right-padded-mask": ({}, {}, dict(attention_mask=RIGHT), NotImplementedError,
                          "must be left-padded, each row zeros then ones over the 3 tokens of the call", True),
    "counts-with-short-conv": (dict(use_short_conv=True), dict(state="ragged"), dict(token_counts=(1, 2)), NotImplementedError,
                               "use_short_conv with token_counts", True),
    "counts-wrong-length": ({}, dict(state="ragged"), dict(token_counts=(1, 2, 3)), ValueError,
                            r"token_counts=\(1, 2, 3\) must be 2 ints in 0 \.\. 3", True),
    "counts-out-of-range": ({}, dict(state="ragged"), dict(token_counts=torch.tensor([1, 4])), ValueError,
                            r"token_counts=\(1, 4\) must be 2 ints in 0 \.\. 3", True),
    "mask-3d": ({}, {}, dict(attention_mask=torch.ones(2, 3, 3, dtype=torch.long)), AssertionError,
                "Expected attention_mask as a 0-1 matrix with shape", True),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusal(case):
    opts, cache, kw, exc, match, clamped = REFUSALS[case]
    _refused(_layer(**opts), _cache(**cache), exc, match, clamped, **kw)


# two conditions at once: the refusal that wins (and, with it, whether the clamp has run)
PRECEDENCE = {
    "isolate-over-layer_idx": (dict(isolate_sequences=True, layer_idx=None), {}, dict(attention_mask=MASK), NotImplementedError,
                               "isolate_sequences=True", True),
    "uniform-state-over-short-conv": (dict(use_short_conv=True), dict(state="uniform"), dict(attention_mask=MASK), NotImplementedError,
                                      "the cached decode state is uniform", True),
    "short-conv-over-not-left-padded": (dict(use_short_conv=True), {}, dict(attention_mask=RIGHT), NotImplementedError,
                                        "use_short_conv with a padding attention_mask", True),
    "short-conv-counts-over-range": (dict(use_short_conv=True), dict(state="ragged"), dict(token_counts=(1, 9)), NotImplementedError,
                                     "use_short_conv with token_counts", True),
    "dev-layer_idx-over-short-conv-over-8": (dict(hidden=48, layer_idx=None, use_short_conv=True), dict(device_positions=True), {}, ValueError,
                                             "indexed by layer_idx", False),
    "dev-short-conv-over-8": (dict(hidden=48, use_short_conv=True), dict(device_positions=True), {}, NotImplementedError,
                              "with use_short_conv", False),
    "dev-refusals-over-isolate": (dict(hidden=48, isolate_sequences=True), dict(device_positions=True), dict(attention_mask=MASK),
                                  NotImplementedError, "needs head_k_dim % 8 == 0", False),
}


@pytest.mark.parametrize("case", list(PRECEDENCE))
def test_refusal_precedence(case):
    opts, cache, kw, exc, match, clamped = PRECEDENCE[case]
    _refused(_layer(**opts), _cache(**cache), exc, match, clamped, **kw)


def test_ragged_state_does_not_read_the_mask_and_ignores_counts_elsewhere():
    """What is NOT refused: a right-padded mask on a cached ragged state (the state carries the lengths; the call goes on to the
    operator, which takes no CPU tensor), and token_counts of any kind anywhere but on a cached ragged state."""
    with pytest.raises(RuntimeError, match="run only on a ROCm GPU"):
        _layer()(torch.zeros(2, 3, 64), attention_mask=RIGHT, past_key_values=_cache(state="ragged"), use_cache=True)
    with pytest.raises(RuntimeError, match="run only on a ROCm GPU"):
        _layer()(torch.zeros(2, 3, 64), past_key_values=_cache(), use_cache=True, token_counts=(9, 9, 9))
    with pytest.raises(RuntimeError, match="run only on a ROCm GPU"):
        _layer(use_short_conv=True)(torch.zeros(2, 3, 64), past_key_values=_cache(state="uniform"), use_cache=True, token_counts=(9,))


def test_warnings_once_per_layer_and_attributed_to_the_caller():
    """head_k_dim = 12: the eager feature map + rotary warning; a padded batch of 2 x 40 tokens that unpads to 70 > 64: the
    recurrent-branch warning.  Each once per layer, a UserWarning attributed to the frame that called `forward` (for a module call
    that is torch's `Module._call_impl`), and the `_warned_*` attributes say so."""
    m = _layer(hidden=48, exact_decoding=False)
    x = torch.zeros(2, 40, 48)
    mask = torch.ones(2, 40, dtype=torch.long)
    mask[0, :10] = 0
    for expected in (2, 0):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            with pytest.raises(RuntimeError, match="run only on a ROCm GPU"):
                m(x, attention_mask=mask)
        ours = [w for w in caught if str(w.message).startswith("MHLA: ")]
        assert len(ours) == expected, [str(w.message) for w in caught]
        if expected:
            assert all(w.category is UserWarning and w.filename.endswith("module.py") for w in ours), [(w.category, w.filename) for w in ours]
            assert str(ours[0].message).startswith("MHLA: head_k_dim=12 is not a multiple of 8: feature map and rotary run as eager PyTorch ops")
            assert str(ours[1].message).startswith("MHLA: a padded batch of 2 x 40 tokens unpads to one packed sequence of 70 > 64 tokens; the "
                                                   "recurrent branch then runs the multi-chunk chunk operator")
        assert m._warned_eager_rotary is True and m._warned_recurrent_packed is True
    direct = _layer(hidden=48, exact_decoding=False)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with pytest.raises(RuntimeError, match="run only on a ROCm GPU"):
            direct.forward(x, attention_mask=mask)            # called directly: attributed to this file
    assert [w.filename for w in caught if str(w.message).startswith("MHLA: ")] == [__file__] * 2
