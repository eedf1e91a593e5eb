"""Prefill of a pack of prompts (cu_seqlens) into one ragged decode state, the parts that need no GPU: the plan's destination
table, the argument refusals of mhla_causal_state / mhla_causal_prefill, the validation of mhla_causal_varlen_state_init (host
arithmetic, before any launch), and the layer's opt-in on DecodeCache(packed_prefill=True)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CU = [0, 1, 66, 66, 130, 321]   # lengths 1, 65, 0, 64, 191: 7 chunks, one empty sequence
EINVAL, ENOTSUP = -22, -95


def expected_dst(cu, chunk=64):
    """(sequence, index of the chunk within its sequence) of every chunk, written out the slow way: one chunk at a time."""
    dst = []
    for s in range(len(cu) - 1):
        p, j = cu[s], 0
        while p < cu[s + 1]:
            dst.append([s, j])
            p += chunk
            j += 1
    return dst


def test_destination_table_of_the_issue_pack():
    from mhla_amd import causal_varlen_plan
    plan = causal_varlen_plan(CU, "cpu")
    assert plan.dst.tolist() == [[0, 0], [1, 0], [1, 1], [3, 0], [4, 0], [4, 1], [4, 2]]
    assert plan.dst.dtype == torch.int32 and plan.dst.shape == (7, 2) and plan.dst.is_contiguous()
    # the attributes the operator reads keep their types and values
    assert plan.table.tolist() == [[0, 1], [1, 64], [65, 1], [66, 64], [130, 64], [194, 64], [258, 63]] and plan.table.dtype == torch.int32
    assert plan.loc.tolist() == [0, 0, 1, 0, 0, 1, 2] and plan.seq.tolist() == [0, 1, 1, 3, 4, 4, 4]
    assert plan.loc.dtype == plan.seq.dtype == torch.int64


@pytest.mark.parametrize("cu", [[0, 0, 0, 70, 70], [0, 64], [0, 65], [0, 64, 128], [0, 65, 130], [0], [0, 0], [0, 5, 5, 5, 200, 201],
                                [0, 63, 128, 257, 258, 458]])
def test_destination_table_of_edge_packs(cu):
    from mhla_amd import causal_varlen_plan
    want = expected_dst(cu)
    for given in (cu, torch.tensor(cu, dtype=torch.int32)):
        plan = causal_varlen_plan(given, "cpu")
        assert plan.dst.dtype == torch.int32 and plan.dst.shape == (len(want), 2) and plan.dst.is_contiguous()
        assert plan.dst.tolist() == want
        assert plan.dst[:, 0].tolist() == plan.seq.tolist() and plan.dst[:, 1].tolist() == plan.loc.tolist()
        # a chunk of 64 rows is a finished one (a tile of S), a shorter one the last of its sequence (Cur): the destinations are distinct
        assert len({tuple(d) for d in want}) == len(want)
        for (s, j), (_, rows) in zip(want, plan.table.tolist()):
            n = cu[s + 1] - cu[s]
            assert (rows == 64 and j < n // 64) or (rows == n % 64 and j == n // 64)


def _no_load(monkeypatch):
    from mhla_amd import _lib

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)


def test_refusals_come_before_the_library_and_the_device_check(monkeypatch):
    import mhla_amd
    from mhla_amd import ops
    _no_load(monkeypatch)
    T, H, K, V, L = 321, 2, 16, 24, 4
    q, k, v = torch.zeros(1, T, H, K), torch.zeros(1, T, H, K), torch.zeros(1, T, H, V)
    mix = torch.tril(torch.ones(L, L))
    state = lambda cu, k=k, v=v, mix=mix, **kw: mhla_amd.mhla_causal_state(k, v, mix, cu_seqlens=cu, **kw)
    prefill = lambda cu, k=k, v=v, mix=mix, **kw: mhla_amd.mhla_causal_prefill(kw.pop("q", q), k, v, mix, cu_seqlens=cu, **kw)
    two = lambda t: t.expand(2, -1, -1, -1)
    for name, call in (("mhla_causal_state", state), ("mhla_causal_prefill", prefill)):
        with pytest.raises(ValueError, match="B = 1") as ei:
            call(CU, k=two(k), v=two(v), **({"q": two(q)} if call is prefill else {}))
        assert name in str(ei.value)
        with pytest.raises(ValueError, match="excludes lengths") as ei:
            call(CU, lengths=[321])
        assert name in str(ei.value)
        with pytest.raises(ValueError, match="excludes lengths"):
            call(CU, left_padded=True)
        with pytest.raises(ValueError, match="ends at 100"):           # the plan of another pack
            call(ops.causal_varlen_plan([0, 100], "cpu"))
        with pytest.raises(ValueError, match="chunk_size=32"):          # a plan cut into other chunks
            call(ops.causal_varlen_plan(CU, "cpu", chunk_size=32))
        # 2 chunks of capacity hold 128 tokens: sequence 4 (191 tokens) is named, the others are not
        with pytest.raises(IndexError, match=r"sequences \[4\] of lengths \[191\]") as ei:
            call(CU, capacity_chunks=2)
        assert "2 chunks" in str(ei.value) and "128 tokens" in str(ei.value)
        # ... and more than the rows of the matrix: the operator's message
        with pytest.raises(IndexError, match=r"sequences \[1, 3\]"):
            call([0, 0, 129, 129, 321], mix=mix[:2, :2])
        with pytest.raises(ValueError, match="capacity_chunks=5"):
            call(CU, capacity_chunks=5)
        # 40 000 empty sequences and a real one: the plan stays tiny, 40 001 x 2 heads do not fit one launch's range
        with pytest.raises(ValueError, match="65535") as ei:
            call([0] * 40001 + [5], k=k[:, :5], v=v[:, :5], **({"q": q[:, :5]} if call is prefill else {}))
        assert "40001 sequences" in str(ei.value)
        # every check passed: the device check is what is left (through the real loader)
    with pytest.raises(ValueError, match="supports 64 only"):
        mhla_amd.mhla_causal_prefill(q, k, v, mix, 32, cu_seqlens=CU)
    monkeypatch.undo()
    for call in (state, prefill):
        with pytest.raises(RuntimeError, match="run only on a ROCm GPU"):
            call(CU)
        with pytest.raises(RuntimeError, match="run only on a ROCm GPU"):
            call(mhla_amd.causal_varlen_plan(CU, "cpu"))


def test_all_empty_pack_is_an_empty_ragged_state_without_a_launch(monkeypatch):
    import mhla_amd
    _no_load(monkeypatch)
    H, K, V, L = 2, 16, 24, 4
    q, k, v = torch.zeros(1, 0, H, K), torch.zeros(1, 0, H, K), torch.zeros(1, 0, H, V)
    mix = torch.tril(torch.ones(L, L))
    st = mhla_amd.mhla_causal_state(k, v, mix, cu_seqlens=[0, 0, 0, 0], capacity_chunks=3)
    assert st.lengths == (0, 0, 0) and st.seen == 0 and st.pos.tolist() == [0, 0, 0] and st.pos.dtype == torch.int32
    assert st.S.shape == (3, H, 3, K, V) and st.P.shape == st.Cur.shape == (3, H, K, V) and st.capacity_chunks == 3
    assert float(st.S.abs().max()) == float(st.P.abs().max()) == float(st.Cur.abs().max()) == 0.0
    o, st = mhla_amd.mhla_causal_prefill(q, k, v, mix, cu_seqlens=[0, 0])
    assert o.shape == (1, 0, H, V) and st.lengths == (0,) and st.capacity_chunks == L


def test_entry_point_declared_bound_and_exported_at_abi_9():
    from mhla_amd import build as b, _lib
    b.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mhla_hip.h")).read()
    name = "mhla_causal_varlen_state_init"
    assert name in set(re.findall(r"\b(mhla_[a-z0-9_]+)\s*\(", header)), f"{name} not declared in include/mhla_hip.h"
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert lib.mhla_abi_version() == _lib.ABI_VERSION == 9
    assert re.search(r"#define\s+MHLA_ABI_VERSION\s+9\b", header)


def test_entry_point_validates_before_it_launches():
    """Host arithmetic only.  The addresses are made up and never dereferenced on the host; every case has a second, independent
    reason to be refused -- a null chunk table, the last check before the launches -- so that no loosening of one check can launch
    on them."""
    from mhla_amd import build as b, _lib
    b.build()
    lib = _lib.load()
    nv = _lib.NULL_VIEW
    fake = lambda: _lib.View(0x10000, 1 << 20, 64, 16)
    base = dict(k=None, v=None, mix=0x10000, ldmix=4, S=0x10000, cap=3, P=0x10000, Cur=0x10000, n_seqs=6, seq_len=0x10000, max_len=192,
                T=513, H=2, K=16, V=16, chunk=64, n_chunks=11, tab=None, dst=0x10000, dtype=_lib.F32)

    def raw(**kw):
        a = dict(base, **kw)
        k = fake() if a["k"] is None else a["k"]
        v = fake() if a["v"] is None else a["v"]
        return lib.mhla_causal_varlen_state_init(k, v, a["mix"], a["ldmix"], a["S"], a["cap"], a["P"], a["Cur"], a["n_seqs"], a["seq_len"],
                                                 a["max_len"], a["T"], a["H"], a["K"], a["V"], a["chunk"], a["n_chunks"], a["tab"], a["dst"],
                                                 a["dtype"], None)

    def refused(code, text, **kw):
        rc, msg = raw(**kw), lib.mhla_last_error()
        assert rc == code and text in msg, (kw, rc, msg)

    refused(EINVAL, b"chunk_tab_dev null")                               # (the second reason, on its own)
    refused(EINVAL, b"not 8-byte aligned", tab=0x10004)
    # dimensions, chunk, dtype: what mhla_causal_state_init checks
    refused(EINVAL, b"non-positive dimension", H=0)
    refused(ENOTSUP, b"only 64 is supported", chunk=32)
    refused(EINVAL, b"multiples of 4", K=18)
    refused(EINVAL, b"unknown dtype", dtype=3)
    refused(EINVAL, b"n_seqs=0", n_seqs=0)
    refused(ENOTSUP, b"n_seqs*H=65536 exceeds grid limit 65535", n_seqs=32768)
    refused(EINVAL, b"T=0", T=0)
    refused(EINVAL, b"n_chunks=0", n_chunks=0)
    # views and state
    assert raw(k=nv) == EINVAL and lib.mhla_last_error()
    refused(EINVAL, b"cap_chunks=0", cap=0)
    refused(EINVAL, b"S, P or Cur null", P=None)
    refused(EINVAL, b"16-byte aligned", Cur=0x10004)
    # the table's row count: ceil(T / 64) .. T
    refused(EINVAL, b"n_chunks=8 outside ceil(T / 64)=9 .. T=513", n_chunks=8)
    refused(EINVAL, b"n_chunks=514 outside", n_chunks=514)
    # the longest sequence
    refused(EINVAL, b"max_len=-1 outside 0 .. T=513", max_len=-1)
    refused(EINVAL, b"max_len=514 outside 0 .. T=513", max_len=514)
    refused(EINVAL, b"max_len=193 tokens need 4 chunks, the state holds 3", max_len=193)
    # rows of mix: row max_len / 64 up to its diagonal, or the state's last row when the longest sequence fills the state
    refused(EINVAL, b"mix null", mix=None)
    refused(EINVAL, b"row 2 of mix is read", ldmix=2, max_len=191)
    refused(EINVAL, b"row 2 of mix is read", ldmix=2, max_len=192)
    refused(EINVAL, b"chunk_tab_dev null", ldmix=3, max_len=192)        # (covered: the next reason is the table)
    refused(EINVAL, b"row 1 of mix is read", ldmix=1, max_len=64)
    # the device arrays
    refused(EINVAL, b"seq_len_dev null", seq_len=None)
    refused(EINVAL, b"seq_len_dev null or not 4-byte aligned", seq_len=0x10002)
    refused(EINVAL, b"chunk_dst_dev null", dst=None)
    refused(EINVAL, b"chunk_dst_dev null or not 4-byte aligned", dst=0x10001)


MASK = torch.tensor([[0, 1, 1, 1, 1], [1, 1, 1, 1, 1]])


def _layer(**kw):
    from mhla_amd.modules.fla import MHLA
    return MHLA(**{**dict(hidden_size=64, num_heads=2, feature_map="relu", isolate_sequences=True, exact_decoding=True, layer_idx=0), **kw})


def test_layer_takes_a_pack_on_a_packed_prefill_cache():
    """The calls test_layer_refuses_isolation_with_a_cache makes, on DecodeCache(packed_prefill=True) and a layer with both flags:
    every check passes and the operator's device check is what stops a CPU call; the cache stays empty."""
    from mhla_amd.modules.fla import DecodeCache
    layer = _layer()
    for kw in (dict(x=torch.zeros(1, 10, 64), cu_seqlens=torch.tensor([0, 4, 10])), dict(x=torch.zeros(2, 5, 64), attention_mask=MASK)):
        for dev in (False, True):
            cache = DecodeCache(packed_prefill=True, device_positions=dev)
            assert cache.packed_prefill is True and cache.device_positions is dev
            with pytest.raises(RuntimeError, match="run only on a ROCm GPU"):
                layer(kw["x"], use_cache=True, past_key_values=cache, **{n: t for n, t in kw.items() if n != "x"})
            assert len(cache) == 0 and cache.get_seq_length(0) == 0


def test_layer_refusals_on_the_packed_path_leave_the_cache_untouched():
    from mhla_amd import CausalState
    from mhla_amd.modules.fla import DecodeCache
    x, cu = torch.zeros(1, 10, 64), torch.tensor([0, 4, 10])
    # use_short_conv
    conv = _layer(use_short_conv=True)
    for kw in (dict(cu_seqlens=cu), dict(attention_mask=torch.ones(1, 10, dtype=torch.long))):
        cache = DecodeCache(packed_prefill=True)
        with pytest.raises(NotImplementedError, match="use_short_conv with a packed exact prefill"):
            conv(x, use_cache=True, past_key_values=cache, **kw)
        assert len(cache) == 0
    # a pack on a cache that already holds a state
    layer = _layer()
    cache = DecodeCache(packed_prefill=True)
    state = CausalState.empty(2, 2, 16, 32, 4, device="cpu")
    state = CausalState(state.S, state.P, state.Cur, 0, 64, lengths=(4, 6))
    cache.update(recurrent_state=state, layer_idx=0, offset=6)
    with pytest.raises(NotImplementedError, match="cu_seqlens on a cache that already holds a decode state"):
        layer(x, use_cache=True, past_key_values=cache, cu_seqlens=cu)
    assert cache[0]["recurrent_state"] is state and cache.get_seq_length(0) == 6 and state.lengths == (4, 6)
    assert float(state.S.abs().max()) == float(state.P.abs().max()) == float(state.Cur.abs().max()) == 0.0
    # B = 2 rows with cu_seqlens
    with pytest.raises(ValueError, match="B = 1"):
        layer(torch.zeros(2, 5, 64), use_cache=True, past_key_values=DecodeCache(packed_prefill=True), cu_seqlens=torch.tensor([0, 5]))


def test_default_cache_and_layers_without_exact_decoding_refuse_as_before():
    from mhla_amd.modules.fla import DecodeCache
    x, cu = torch.zeros(1, 10, 64), torch.tensor([0, 4, 10])
    old = ("MHLA(isolate_sequences=True): an attention_mask or cu_seqlens with use_cache -- a decode state per packed sequence, and the "
           "exact_decoding prefill of a padded batch, are not implemented for it")
    assert DecodeCache().packed_prefill is False
    for layer, cache in ((_layer(), DecodeCache()), (_layer(), DecodeCache(device_positions=True)),
                         (_layer(exact_decoding=False), DecodeCache(packed_prefill=True))):
        with pytest.raises(NotImplementedError) as ei:
            layer(x, use_cache=True, past_key_values=cache, cu_seqlens=cu)
        assert str(ei.value) == old
        with pytest.raises(NotImplementedError) as ei:
            layer(torch.zeros(2, 5, 64), attention_mask=MASK, use_cache=True, past_key_values=cache)
        assert str(ei.value) == old
        assert len(cache) == 0


def test_gpt_host_refuses_a_pack_on_a_cache_it_cannot_prefill():
    from mhla_amd.hosts.gpt import GPT_MHLA
    from mhla_amd.modules.fla import DecodeCache
    from mhla_amd import CausalState
    kw = dict(vocab_size=50, hidden_size=64, num_layers=1, num_heads=2, max_seq_len=128)
    ids, cu = torch.zeros(1, 10, dtype=torch.long), torch.tensor([0, 4, 10])
    both = GPT_MHLA(exact_decoding=True, isolate_sequences=True, **kw)
    with pytest.raises(NotImplementedError, match="cu_seqlens with a cache"):
        both(ids, cache=DecodeCache(), cu_seqlens=cu)                      # not a packed_prefill cache
    with pytest.raises(NotImplementedError, match="cu_seqlens with a cache"):
        GPT_MHLA(exact_decoding=True, **kw)(ids, cache=DecodeCache(packed_prefill=True), cu_seqlens=cu)   # not an isolating model
    held = DecodeCache(packed_prefill=True)
    held.update(recurrent_state=CausalState.empty(2, 2, 16, 32, 2, device="cpu"), layer_idx=0, offset=6)
    with pytest.raises(NotImplementedError, match="cu_seqlens with a cache that already holds a state"):
        both(ids, cache=held, cu_seqlens=cu)
    # an empty packed_prefill cache: the layers' packed prefill, stopped on a CPU by the operator's device check
    cache = DecodeCache(packed_prefill=True)
    with pytest.raises(RuntimeError, match="run only on a ROCm GPU"):
        both(ids, cache=cache, cu_seqlens=cu)
    assert len(cache) == 0
