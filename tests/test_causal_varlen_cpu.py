"""Packed sequences of the causal operator (cu_seqlens), the parts that need no GPU: the chunk table, the effective mixing
matrix against the oracle, the argument validation, and the C ABI's declarations and workspace sizes."""
import os
import re

import pytest
import torch

from oracle import mhla_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CU = [0, 1, 66, 66, 130, 321]   # lengths 1, 65, 0, 64, 191: 7 chunks, one empty sequence

NEW_SYMBOLS = ("mhla_causal_varlen_fwd", "mhla_causal_varlen_normgate_fwd", "mhla_causal_varlen_bwd",
               "mhla_causal_varlen_fwd_ws_bytes", "mhla_causal_varlen_bwd_ws_bytes", "mhla_causal_varlen_normgate_fusable")


def expected_plan(cu, chunk=64):
    """(table rows, loc, seq) written out the slow way: one chunk at a time."""
    table, loc, seq = [], [], []
    for s in range(len(cu) - 1):
        p, j = cu[s], 0
        while p < cu[s + 1]:
            table.append([p, min(chunk, cu[s + 1] - p)])
            loc.append(j)
            seq.append(s)
            p += chunk
            j += 1
    return table, loc, seq


def test_plan_of_the_issue_pack():
    from mhla_amd import causal_varlen_plan
    plan = causal_varlen_plan(CU, "cpu")
    assert plan.cu == tuple(CU) and plan.n_chunks == 7 and plan.max_chunks == 3
    assert plan.table.dtype == torch.int32 and plan.table.shape == (7, 2) and plan.table.is_contiguous()
    assert plan.table.tolist() == [[0, 1], [1, 64], [65, 1], [66, 64], [130, 64], [194, 64], [258, 63]]
    assert plan.loc.tolist() == [0, 0, 1, 0, 0, 1, 2]
    assert plan.seq.tolist() == [0, 1, 1, 3, 4, 4, 4]
    assert plan.lengths == (1, 65, 0, 64, 191)


@pytest.mark.parametrize("cu", [[0, 0, 0, 70, 70], [0, 64], [0, 65], [0, 64, 128], [0, 65, 130], [0], [0, 0], [0, 5, 5, 5, 200, 201],
                                [0, 63, 128, 257, 258, 458]])
def test_plan_edge_packs(cu):
    """All sequences empty but one, exactly 64 and exactly 65 tokens, no sequence at all; a tensor gives the same plan as a list."""
    from mhla_amd import causal_varlen_plan
    table, loc, seq = expected_plan(cu)
    for given in (cu, torch.tensor(cu, dtype=torch.int32), torch.tensor(cu, dtype=torch.int64), tuple(cu)):
        plan = causal_varlen_plan(given, "cpu")
        assert plan.n_chunks == len(table) and plan.cu == tuple(cu)
        assert plan.table.shape == (len(table), 2) and plan.table.dtype == torch.int32
        assert plan.table.tolist() == table and plan.loc.tolist() == loc and plan.seq.tolist() == seq
        # every token row belongs to exactly one chunk, in order
        rows = [r for p, c in table for r in range(p, p + c)]
        assert rows == list(range(cu[-1])) and all(1 <= c <= 64 for _, c in table)
        n_lo, n_hi = (cu[-1] + 63) // 64, cu[-1]
        assert n_lo <= plan.n_chunks <= n_hi   # what the library checks of a table it cannot read


def test_mix_eff_is_lower_triangular_and_block_structured():
    from mhla_amd import causal_varlen_plan
    plan = causal_varlen_plan(CU, "cpu")
    mix = torch.tril(torch.rand(5, 5, generator=torch.Generator().manual_seed(1)).clamp(1e-5, 1))
    eff = plan.mix_eff(mix.view(5, 5, 1, 1, 1, 1))
    assert eff.dtype == torch.float32 and eff.shape == (7, 7)
    assert torch.equal(eff, eff.tril())
    table, loc, seq = expected_plan(CU)
    for c in range(7):
        for d in range(7):
            want = mix[loc[c], loc[d]].item() if seq[c] == seq[d] and d <= c else 0.0
            assert eff[c, d].item() == want, (c, d)


def repack_chunk_padded(plan, *tensors):
    """[1, T, H, D] pack -> [1, 64 n, H, D]: chunk c in rows 64 c .., zero rows behind a ragged chunk."""
    out = []
    for t in tensors:
        p = t.new_zeros(1, 64 * plan.n_chunks, *t.shape[2:])
        for c, (s, cnt) in enumerate(plan.table.tolist()):
            p[:, 64 * c:64 * c + cnt] = t[:, s:s + cnt]
        out.append(p)
    return out


def test_mix_eff_through_the_oracle_is_the_per_sequence_operator():
    """The observation the feature rests on: the uniform operator over the pack's chunks (repacked chunk-padded) with mix_eff equals
    the operator over every sequence alone -- forward, and dmix through autograd of mix_eff.  Bounds: both sides are the same fp32
    products; zero weights and zero rows add exact zeros, so only the order of fp32 sums may differ -- 1e-5 of the maximum is
    a hundred fp32 roundings."""
    from mhla_amd import causal_varlen_plan
    from conftest import rel_err
    plan = causal_varlen_plan(CU, "cpu")
    T, H, K, V, L = CU[-1], 2, 16, 24, 4
    g = torch.Generator().manual_seed(5)
    q, k = torch.randn(1, T, H, K, generator=g), torch.randn(1, T, H, K, generator=g)
    v, do = torch.randn(1, T, H, V, generator=g), torch.randn(1, T, H, V, generator=g)
    mix = torch.tril(torch.rand(L, L, generator=g).clamp(1e-5, 1))
    # per sequence
    m1 = mix.clone().requires_grad_(True)
    want = torch.cat([orc.causal_fwd(q[:, a:b], k[:, a:b], v[:, a:b], m1) for a, b in zip(CU, CU[1:]) if b > a], dim=1)
    (want * do).sum().backward()
    # the pack's chunks with mix_eff
    m2 = mix.clone().requires_grad_(True)
    qp, kp, vp, dop = repack_chunk_padded(plan, q, k, v, do)
    got_p = orc.causal_fwd(qp, kp, vp, plan.mix_eff(m2))
    (got_p * dop).sum().backward()
    got = torch.cat([got_p[:, 64 * c:64 * c + cnt] for c, (s, cnt) in enumerate(plan.table.tolist())], dim=1)
    assert rel_err(got.detach(), want.detach()) < 1e-5
    assert rel_err(m2.grad, m1.grad) < 1e-5
    assert torch.equal(m2.grad, m2.grad.tril())


def test_validation_raises_before_the_library_is_loaded(monkeypatch):
    import mhla_amd
    from mhla_amd import _lib, ops

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    T, H, K, V, L = 321, 2, 64, 64, 2
    q, k, v = torch.zeros(1, T, H, K), torch.zeros(1, T, H, K), torch.zeros(1, T, H, V)
    gate, w = torch.zeros(1, T, H, V), torch.ones(V)
    mix = torch.tril(torch.ones(L, L))
    calls = (lambda cu, q=q, k=k, v=v, mix=mix: mhla_amd.mhla_causal(q, k, v, mix, cu_seqlens=cu),
             lambda cu, q=q, k=k, v=v, mix=mix: mhla_amd.mhla_causal_normgate(q, k, v, mix, gate, w, cu_seqlens=cu))
    bad = [([1, 321], "start at 0"), ([0, 100, 50, 321], "non-decreasing"), ([0, 100, 320], "ends at"), ([0, 100, 322], "ends at"),
           ([], "start at 0"), (torch.tensor([[0, 321]]), "1-D"), (torch.tensor([0.0, 321.0]), "integer"), ([0, 1.5, 321], "ints")]
    for call in calls:
        for cu, what in bad:
            with pytest.raises(ValueError, match=what):
                call(cu)
        with pytest.raises(ValueError, match="B = 1"):
            call([0, 321], q=q.expand(2, -1, -1, -1), k=k.expand(2, -1, -1, -1), v=v.expand(2, -1, -1, -1))
        # L = 2 rows: 128 tokens per sequence at the most; sequences 1 (129 tokens) and 3 (192) are named, the empty 0 and 2 are not
        with pytest.raises(IndexError, match=r"sequences \[1, 3\]") as ei:
            call([0, 0, 129, 129, 321])
        assert "129" in str(ei.value) and "192" in str(ei.value)
        with pytest.raises(ValueError, match="chunk_size"):
            call(ops.causal_varlen_plan([0, 321], "cpu", chunk_size=32))
    # a plan of another pack
    with pytest.raises(ValueError, match="ends at"):
        mhla_amd.mhla_causal(q, k, v, mix, cu_seqlens=ops.causal_varlen_plan([0, 100], "cpu"))
    # T == 0: the empty result, as without cu_seqlens
    e = mhla_amd.mhla_causal(q[:, :0], k[:, :0], v[:, :0], mix, cu_seqlens=[0, 0])
    assert e.shape == (1, 0, H, V)


def test_layer_refuses_isolation_with_a_cache():
    from mhla_amd.modules.fla import MHLA, DecodeCache
    layer = MHLA(hidden_size=64, num_heads=2, feature_map="relu", isolate_sequences=True, layer_idx=0)
    x = torch.zeros(1, 10, 64)
    with pytest.raises(NotImplementedError, match="isolate_sequences"):
        layer(x, use_cache=True, past_key_values=DecodeCache(), cu_seqlens=torch.tensor([0, 4, 10]))
    with pytest.raises(NotImplementedError, match="isolate_sequences"):
        layer(torch.zeros(2, 5, 64), attention_mask=torch.tensor([[0, 1, 1, 1, 1], [1, 1, 1, 1, 1]]), use_cache=True,
              past_key_values=DecodeCache())
    # the exact_decoding prefill of a padded batch is refused as well, not served silently by the exact path
    exact = MHLA(hidden_size=64, num_heads=2, feature_map="relu", isolate_sequences=True, exact_decoding=True, layer_idx=0)
    with pytest.raises(NotImplementedError, match="isolate_sequences"):
        exact(torch.zeros(2, 5, 64), attention_mask=torch.tensor([[0, 1, 1, 1, 1], [1, 1, 1, 1, 1]]), use_cache=True,
              past_key_values=DecodeCache())
    assert MHLA(hidden_size=64, num_heads=2, feature_map="relu").isolate_sequences is False


def test_new_symbols_declared_bound_and_exported_at_abi_9():
    from mhla_amd import build as b, _lib
    b.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mhla_hip.h")).read()
    declared = set(re.findall(r"\b(mhla_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in include/mhla_hip.h"
        assert name in _lib.SIGNATURES, f"{name} not bound in _lib.SIGNATURES"
        assert hasattr(lib, name), f"{name} not exported"
    assert lib.mhla_abi_version() == _lib.ABI_VERSION == 9
    assert re.search(r"#define\s+MHLA_ABI_VERSION\s+9\b", header)


@pytest.mark.parametrize("dt,flags", [(1, 0), (1, "split"), (1, "bf16"), (1, "generic"), (0, 0), (2, 0)])
@pytest.mark.parametrize("K,V", [(64, 64), (128, 256), (256, 512), (48, 40)])
def test_varlen_workspaces_equal_the_uniform_ones_at_the_same_chunk_count(dt, flags, K, V):
    from mhla_amd import build as b, _lib
    b.build()
    lib = _lib.load()
    fl = {0: 0, "split": _lib.CAUSAL_FP32_GRADE_SUMMARIES, "bf16": _lib.CAUSAL_BF16_SUMMARIES, "generic": _lib.CAUSAL_FORCE_GENERIC}[flags]
    for n in (1, 7, 66, 130, 256, 260):   # 260: beyond the 16-bit pipeline's 256 chunks
        for T in (64 * n, 64 * n - 13, max(n, 64 * (n - 1) + 1) if n > 1 else 5):   # T does not size the workspace, n_chunks does
            assert lib.mhla_causal_varlen_fwd_ws_bytes(1, T, 4, K, V, 64, n, dt, fl) == lib.mhla_causal_fwd_ws_bytes(1, 64 * n, 4, K, V, 64, dt, fl) > 0
            assert lib.mhla_causal_varlen_bwd_ws_bytes(1, T, 4, K, V, 64, n, dt, fl) == lib.mhla_causal_bwd_ws_bytes(1, 64 * n, 4, K, V, 64, dt, fl) > 0
            assert lib.mhla_causal_varlen_normgate_fusable(T, K, V, 64, n, dt, fl) == lib.mhla_causal_normgate_fusable(64 * n, K, V, 64, dt, fl)
