"""Verifying a draft without committing it and committing an accepted prefix (mhla_causal_verify / mhla_causal_commit), the parts
that need no GPU: the restatement in decode_util (`verify_ref`, `commit_ref`, built from `extend_ragged_ref`) held to the oracle
on the table of (pos, draft, accepted), the validation that runs before the device check, and the bookkeeping of
`DecodeCache.commit` / `discard`."""
import pytest
import torch

from conftest import rel_err
from decode_util import (ACCEPT, COUNTS, DRAFTS, SPEC_CAP, SPEC_T, SPEC_L, SPEC_TABLE, commit_ref, oracle_state, start_state, table_inputs,
                         verify_ref, window)
from oracle import mhla_oracle as orc

@pytest.mark.parametrize("left_padded", [False, True], ids=["right-padded", "left-padded"])
def test_verify_and_commit_refs_reproduce_the_oracle(left_padded):
    H, K, V = 2, 16, 24
    hist, q, k, v, mix = table_inputs(H, K, V, table=DRAFTS, T=SPEC_T, L=SPEC_L, left_padded=left_padded)
    start = start_state(hist, DRAFTS, mix, SPEC_CAP)
    o, same = verify_ref(start, q, k, v, mix, COUNTS, left_padded)
    assert same is start and same[3] == tuple(p for p, _ in DRAFTS)
    S, P, Cur, lengths = commit_ref(start, k, v, mix, COUNTS, ACCEPT, left_padded)
    assert lengths == tuple(p + a for p, _, a in SPEC_TABLE)
    for b, (p, n, a) in enumerate(SPEC_TABLE):
        qs, ks, vs = hist[b]
        w = window(SPEC_T, n, left_padded)
        pad = torch.ones(SPEC_T, dtype=torch.bool)
        pad[w] = False
        assert not bool(pad.any()) or float(o[b, pad].abs().max()) == 0.0, f"sequence {b}: padding rows must be zero"
        if n:
            want = orc.causal_fwd(qs, ks, vs, mix)[0, p:p + n]
            e = (o[b, w] - want.double()).abs().max().item() / want.abs().max().item()
            assert e < 1e-6, f"sequence {b} (pos {p}, n {n}): {e:.2e} of the oracle's maximum"
        ref = oracle_state(ks, vs, mix, p + a, SPEC_CAP)
        nfull = (p + a) // 64
        for name, x, r in (("S", S[b:b + 1, :, :nfull], ref[0][:, :, :nfull]), ("P", P[b:b + 1], ref[1]), ("Cur", Cur[b:b + 1], ref[2])):
            if r.numel() and float(r.abs().max()) > 0:
                assert rel_err(x.float(), r) < 1e-6, f"sequence {b}: {name} after {p} + {a} tokens"
            elif x.numel():
                assert float(x.abs().max()) == 0.0, f"sequence {b}: {name} after {p} + {a} tokens must be zero"
        if not a:
            for x, y in ((S[b], start[0][b]), (P[b], start[1][b]), (Cur[b], start[2][b])):
                assert torch.equal(x.float(), y), f"sequence {b}: nothing accepted, the state must be untouched"


def _ragged(lengths, H=2, K=16, V=24, cap=4):
    import mhla_amd
    B = len(lengths)
    z = lambda *s: torch.zeros(s)
    s = mhla_amd.CausalState(z(B, H, cap, K, V), z(B, H, K, V), z(B, H, K, V), 0, 64, lengths=lengths)
    s.Cur.fill_(0.5)
    return s


def _untouched(s, lengths):
    assert s.lengths == tuple(lengths) and s.seen == max(lengths) and s.pos.tolist() == list(lengths) and not s.stale
    assert float(s.S.abs().max()) == 0.0 and float(s.P.abs().max()) == 0.0 and bool((s.Cur == 0.5).all())


def test_verify_is_validated_before_the_device_check():
    import mhla_amd
    B, H, K, V, cap, T = 3, 2, 16, 24, 4, 5
    z = lambda *s: torch.zeros(s)
    mix = torch.ones(cap + 1, cap + 1)
    q, k, v = z(B, T, H, K), z(B, T, H, K), z(B, T, H, V)
    L0 = (7, 100, 64 * cap - 2)
    s = _ragged(L0)
    ver = lambda counts, state=s, m=mix, **kw: mhla_amd.mhla_causal_verify(q, k, v, m, state, counts=counts, **kw)
    with pytest.raises(ValueError, match="counts has 2 entries, expected B=3"):
        ver([1, 2])
    with pytest.raises(ValueError, match=r"must be in 0 \.\. T=5"):
        ver([1, 6, 0])
    # the WHOLE draft must fit: sequence 2 has room for two tokens, and without counts every sequence takes all five
    with pytest.raises(IndexError, match=r"sequences \[2\].*the state holds only 4"):
        ver([5, 5, 3])
    with pytest.raises(IndexError, match=r"sequences \[2\].*the state holds only 4"):
        ver(None)
    with pytest.raises(IndexError, match=r"sequences \[1, 2\].*mixing_matrix has only 1 rows"):
        ver([5, 5, 2], m=torch.ones(1, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ver([5, 0, 2])
    _untouched(s, L0)
    u = mhla_amd.CausalState.empty(B, H, K, V, cap, device="cpu")
    u.seen = 7
    with pytest.raises(ValueError, match=r"to_ragged\(\)"):
        ver([1, 1, 1], state=u)
    assert u.seen == 7 and u.lengths is None
    st = _ragged(L0)
    st.stale = True
    with pytest.raises(ValueError, match="stale"):
        ver([1, 1, 1], state=st)
    st.stale = False
    _untouched(st, L0)
    with pytest.raises(TypeError, match="CausalState"):
        mhla_amd.mhla_causal_verify(q, k, v, mix, None)


def test_commit_is_validated_before_the_device_check():
    import mhla_amd
    B, H, K, V, cap, T = 3, 2, 16, 24, 4, 5
    mix = torch.ones(cap + 1, cap + 1)
    L0 = (7, 100, 200)
    s = _ragged(L0)
    draft = mhla_amd.CausalDraft(torch.zeros(B, T, H, K), torch.zeros(B, T, H, V), (5, 0, 2), True, L0)
    assert draft.counts == (5, 0, 2) and draft.lengths == L0 and draft.left_padded and "counts=(5, 0, 2)" in repr(draft)
    com = lambda accept, state=s, d=draft: mhla_amd.mhla_causal_commit(d, mix, state, accept)
    with pytest.raises(ValueError, match=r"accept=\(6, 0, 0\) must be in 0 \.\. counts=\(5, 0, 2\)"):
        com([6, 0, 0])                    # more than the draft holds
    with pytest.raises(ValueError, match="must be in 0"):
        com([1, 1, 0])                    # sequence 1 drafted nothing
    with pytest.raises(ValueError, match="must be in 0"):
        com(torch.tensor([1, 0, -1]))
    with pytest.raises(ValueError, match="accept has 2 entries, the draft B=3"):
        com([1, 0])
    _untouched(s, L0)
    u = mhla_amd.CausalState.empty(B, H, K, V, cap, device="cpu")
    u.seen = 7
    with pytest.raises(ValueError, match="uniform"):
        com([1, 0, 1], state=u)
    st = _ragged(L0)
    st.stale = True
    with pytest.raises(ValueError, match="stale"):
        com([1, 0, 1], state=st)
    moved = _ragged((8, 100, 200))
    with pytest.raises(ValueError, match="moved since the verify"):
        com([1, 0, 1], state=moved)
    _untouched(moved, (8, 100, 200))
    with pytest.raises(TypeError, match="CausalDraft"):
        mhla_amd.mhla_causal_commit(None, mix, s, [0, 0, 0])
    # what passes every check reaches the device check: CPU tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        com([5, 0, 1])
    _untouched(s, L0)
    # nothing accepted: nothing is launched (no device check either), the state as before
    assert com([0, 0, 0]) is s
    _untouched(s, L0)


def test_commit_workspace_size_is_host_arithmetic():
    from mhla_amd import _lib
    lib = _lib.load()
    for B in (1, 3, 4, 5, 4097):
        want = 4 * ((B + 3) & ~3)
        assert all(lib.mhla_causal_commit_ragged_ws_bytes(B, dt) == want for dt in (_lib.F32, _lib.BF16, _lib.F16))
    assert lib.mhla_causal_commit_ragged_ws_bytes(0, _lib.F32) == 0 and lib.mhla_causal_commit_ragged_ws_bytes(-2, _lib.F32) == 0


class _StubState:
    def __init__(self, seen):
        self.seen = seen


def test_decode_cache_commit_and_discard_bookkeeping(monkeypatch):
    """`commit` runs the operator's commit for every layer that holds a draft, adds what the furthest sequence grew to that layer's
    count and drops the drafts; `discard` only drops them."""
    from mhla_amd.modules import fla
    calls = []

    def fake_commit(draft, mix, state, accept):
        calls.append((draft, mix, state, accept))
        state.seen += max(accept)
        return state

    monkeypatch.setattr(fla, "mhla_causal_commit", fake_commit)
    cache = fla.DecodeCache()
    states = [_StubState(10), _StubState(10), _StubState(10)]
    for i, st in enumerate(states):
        cache.update(recurrent_state=st, layer_idx=i, offset=10)
    cache[0].update(draft="d0", draft_mix="m0")
    cache[2].update(draft="d2", draft_mix="m2")          # layer 1 holds no draft
    assert cache.commit(torch.tensor([2, 0, 3])) is cache
    assert calls == [("d0", "m0", states[0], (2, 0, 3)), ("d2", "m2", states[2], (2, 0, 3))]
    assert [cache.get_seq_length(i) for i in range(3)] == [13, 10, 13] and [s.seen for s in states] == [13, 10, 13]
    assert all("draft" not in e and "draft_mix" not in e for e in cache.states)
    cache.commit([1, 1, 1])                                # no draft anywhere: nothing runs, nothing moves
    assert len(calls) == 2 and [cache.get_seq_length(i) for i in range(3)] == [13, 10, 13]
    cache[1].update(draft="d1", draft_mix="m1")
    assert cache.discard() is cache
    assert all("draft" not in e and "draft_mix" not in e for e in cache.states) and len(calls) == 2
    assert [cache.get_seq_length(i) for i in range(3)] == [13, 10, 13] and cache[1]["recurrent_state"] is states[1]


def test_speculative_refusals_of_the_layer_need_no_gpu():
    """The refusals that depend on the call kind alone are raised before any projection runs."""
    from mhla_amd import modules
    torch.manual_seed(0)
    x = torch.zeros(2, 3, 64)
    m = modules.MHLA(mode="chunk", hidden_size=64, num_heads=2, feature_map="relu", layer_idx=0, exact_decoding=True)
    with pytest.raises(NotImplementedError, match="empty cache"):
        m(x, past_key_values=modules.DecodeCache(), use_cache=True, speculative=True)
    with pytest.raises(NotImplementedError, match="device_positions"):
        m(x, past_key_values=modules.DecodeCache(device_positions=True), use_cache=True, speculative=True)
    conv = modules.MHLA(mode="chunk", hidden_size=64, num_heads=2, feature_map="relu", layer_idx=0, exact_decoding=True, use_short_conv=True)
    with pytest.raises(NotImplementedError, match="use_short_conv"):
        conv(x, past_key_values=modules.DecodeCache(), use_cache=True, speculative=True)
    # a pending draft: any other call is refused until commit or discard
    cache = modules.DecodeCache()
    cache.update(recurrent_state=_ragged((5, 9), K=16, V=32), layer_idx=0, offset=9)
    cache[0].update(draft="pending", draft_mix=None)
    with pytest.raises(ValueError, match="commit or discard first"):
        m(x, past_key_values=cache, use_cache=True)
    assert cache[0]["draft"] == "pending" and cache.get_seq_length() == 9
