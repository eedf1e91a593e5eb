"""Grouped-query decode (k, v and the state with Hkv heads, q with H = G Hkv) as far as a machine without a GPU reaches it: the
new C-ABI symbols with their static argument checks and workspace arithmetic, and the refusals `ops` and the fla layer make before
the library is loaded or a state is touched.  The kernels are in tests/test_gpu_causal_gqa.py."""
import os
import re

import pytest
import torch

import mhla_amd
from mhla_amd import CausalState

NEW = ("mhla_causal_step_ragged_gqa", "mhla_causal_step_dev_gqa", "mhla_causal_extend_ragged_gqa", "mhla_causal_verify_ragged_gqa",
       "mhla_causal_extend_ragged_gqa_ws_bytes")
EINVAL, ENOTSUP = -22, -95


def _lib():
    from mhla_amd import build as b, _lib
    b.build()
    return _lib, _lib.load()


def test_new_symbols_are_declared_bound_and_exported_at_abi_9():
    _l, lib = _lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mhla_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b(int|size_t) " + name + r"\(", header), f"{name} is not declared in mhla_hip.h"
        assert name in _l.SIGNATURES and callable(getattr(lib, name))
    # each call is its namesake with ONE more integer (Hkv, after H)
    for name in NEW:
        old = name.replace("_gqa", "")
        assert len(_l.SIGNATURES[name][1]) == len(_l.SIGNATURES[old][1]) + 1 and _l.SIGNATURES[name][0] is _l.SIGNATURES[old][0]
    assert lib.mhla_abi_version() == _l.ABI_VERSION == 9


def _raw_calls(_l, lib):
    """The four calls on made-up addresses, never dereferenced on the host.  Every case below has a second, independent reason
    to be refused -- a null workspace, the last check before the launches -- so that no loosening of one check can launch on them."""
    nv = _l.NULL_VIEW
    fake = lambda: _l.View(0x10000, 64, 64, 16)
    A = 0x10000

    def step(H=4, Hkv=2, pos=A, ws=None, ws_bytes=0):
        return lib.mhla_causal_step_ragged_gqa(fake(), fake(), fake(), A, 2, A, 2, A, A, pos, 0, 0, fake(), nv, None, 1e-5, nv, ws, ws_bytes,
                                               1, H, Hkv, 8, 4, 64, 1.0, _l.F32, None)

    def dev(H=4, Hkv=2, pos=A, ws=None, ws_bytes=0):
        return lib.mhla_causal_step_dev_gqa(fake(), fake(), fake(), A, 2, A, 2, A, A, pos, A, None, None, 0, 0, 0, fake(), nv, None, 1e-5, nv,
                                            ws, ws_bytes, 1, H, Hkv, 8, 4, 64, 1.0, _l.F32, None)

    def chain(fn):
        def call(H=4, Hkv=2, pos=A, ws=None, ws_bytes=0):
            return fn(fake(), fake(), fake(), A, 2, A, 2, A, A, pos, A, 3, 3, 0, 0, 0, fake(), nv, None, 1e-5, nv, ws, ws_bytes,
                      1, H, Hkv, 8, 4, 64, 1.0, _l.F32, None)
        return call

    return {"mhla_causal_step_ragged_gqa": step, "mhla_causal_step_dev_gqa": dev,
            "mhla_causal_extend_ragged_gqa": chain(lib.mhla_causal_extend_ragged_gqa),
            "mhla_causal_verify_ragged_gqa": chain(lib.mhla_causal_verify_ragged_gqa)}


@pytest.mark.parametrize("name", NEW[:4])
def test_static_checks_before_anything_touches_a_device(name):
    _l, lib = _lib()
    raw = _raw_calls(_l, lib)[name]
    err = lambda: lib.mhla_last_error()
    assert raw() == EINVAL and b"workspace too small" in err()                      # (the second reason, on its own)
    assert raw(H=4, Hkv=4) == EINVAL and b"workspace too small" in err()            # (G = 1 is a grouped call like any other)
    assert raw(H=8, Hkv=1) == EINVAL and b"workspace too small" in err()            # (G = 8: the largest group)
    assert raw(H=4, Hkv=3) == EINVAL and b"Hkv=3" in err() and b"H=4" in err()
    assert raw(H=4, Hkv=0) == EINVAL and b"Hkv=0" in err()
    assert raw(H=4, Hkv=-2) == EINVAL and b"Hkv=-2" in err()
    assert raw(H=9, Hkv=1) == ENOTSUP and b"at most 8" in err()
    assert raw(H=18, Hkv=2) == ENOTSUP and b"at most 8" in err()
    assert raw(pos=None) == EINVAL and b"pos_dev" in err()
    # a workspace one byte short of what the call needs (a made-up, aligned address: the size is checked first)
    if "step" in name:
        need = lib.mhla_causal_step_ws_bytes(1, 4, 8, 4, _l.F32)
    else:
        need = lib.mhla_causal_extend_ragged_gqa_ws_bytes(1, 3, 4, 2, 8, 4, 0, _l.F32)
    assert need > 0
    assert raw(ws=0x20000, ws_bytes=need - 1) == EINVAL and b"workspace too small" in err()


def test_workspace_query_is_the_documented_formula():
    _l, lib = _lib()
    al4 = lambda n: (n + 3) // 4 * 4
    q = lib.mhla_causal_extend_ragged_gqa_ws_bytes
    for B, T, H, Hkv, K, V, later in ((3, 70, 6, 2, 40, 72, 2), (1, 1, 8, 1, 4, 4, 0), (5, 129, 4, 2, 128, 256, 3), (7, 3, 3, 3, 12, 20, 1)):
        want = 4 * (al4(B * Hkv * later * K * V) + al4(B * H * T * V) + al4(B))
        assert q(B, T, H, Hkv, K, V, later, _l.F32) == want == q(B, T, H, Hkv, K, V, later, _l.BF16)
        # Hkv = H: the ungrouped query
        assert q(B, T, H, H, K, V, later, _l.F32) == lib.mhla_causal_extend_ragged_ws_bytes(B, T, H, K, V, later, _l.F32)
    assert q(3, 70, 6, 2, 40, 72, 2, 0) < lib.mhla_causal_extend_ragged_ws_bytes(3, 70, 6, 40, 72, 2, 0)
    assert q(3, 70, 6, 4, 40, 72, 2, 0) == 0 and q(3, 70, 6, 0, 40, 72, 2, 0) == 0      # (no such grouping: no size)


B, H, HK, K, V, CAP = 2, 4, 2, 16, 24, 3


def _state(heads, lengths=None):
    e = CausalState.empty(B, heads, K, V, CAP, device="cpu")
    return e if lengths is None else CausalState(e.S, e.P, e.Cur, 0, 64, lengths=lengths)


def _tok(T, hk=HK, h=H):
    return torch.zeros(B, T, h, K), torch.zeros(B, T, hk, K), torch.zeros(B, T, hk, V)


def test_ops_refuse_a_head_count_that_does_not_divide():
    mix = torch.ones(CAP, CAP)
    rag = _state(3, (5, 9))
    for fn, T, kw in ((mhla_amd.mhla_causal_step, 1, {}), (mhla_amd.mhla_causal_step_dev, 1, {}), (mhla_amd.mhla_causal_extend, 5, {}),
                      (mhla_amd.mhla_causal_extend, 5, {"counts": (1, 2)}), (mhla_amd.mhla_causal_verify, 5, {})):
        with pytest.raises(ValueError, match="multiple of Hkv") as info:
            fn(*_tok(T, hk=3), mix, rag, **kw)
        assert "H=4" in str(info.value) and "Hkv=3" in str(info.value)
    with pytest.raises(ValueError, match="multiple of Hkv"):
        mhla_amd.mhla_causal_prefill(*_tok(70, hk=3), mix)
    # more than eight query heads per k/v head: refused as not implemented, by host arithmetic
    q, k, v = torch.zeros(B, 1, 9, K), torch.zeros(B, 1, 1, K), torch.zeros(B, 1, 1, V)
    with pytest.raises(NotImplementedError, match="at most 8"):
        mhla_amd.mhla_causal_step(q, k, v, mix, _state(1, (5, 9)))
    with pytest.raises(NotImplementedError, match="at most 8"):
        mhla_amd.mhla_causal_prefill(torch.zeros(B, 70, 9, K), torch.zeros(B, 70, 1, K), torch.zeros(B, 70, 1, V), mix)
    assert rag.lengths == (5, 9) and rag.pos.tolist() == [5, 9] and not rag.stale


def test_ops_refuse_a_state_of_neither_head_count():
    mix = torch.ones(CAP, CAP)
    for heads in (H, 1, 3):       # k, v have HK = 2 heads: a state of the QUERY head count is refused too
        for st in (_state(heads), _state(heads, (5, 9))):
            with pytest.raises(ValueError, match="state is CausalState") as info:
                mhla_amd.mhla_causal_step(*_tok(1), mix, st)
            assert "mhla_causal_step" in str(info.value)
            with pytest.raises(ValueError, match="state is CausalState"):
                mhla_amd.mhla_causal_extend(*_tok(5), mix, st)
    with pytest.raises(ValueError, match="state is CausalState"):
        mhla_amd.mhla_causal_verify(*_tok(5), mix, _state(H, (5, 9)))
    with pytest.raises(ValueError, match="state is CausalState"):
        mhla_amd.mhla_causal_step_dev(*_tok(1), mix, _state(H, (5, 9)))
    # the right one goes on to the device check: grouped heads are accepted by every shape test
    for st in (_state(HK), _state(HK, (5, 9))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mhla_amd.mhla_causal_step(*_tok(1), mix, st)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mhla_amd.mhla_causal_extend(*_tok(5), mix, st)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mhla_amd.mhla_causal_verify(*_tok(5), mix, _state(HK, (5, 9)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mhla_amd.mhla_causal_step_dev(*_tok(1), mix, _state(HK, (5, 9)))
    # v must have k's head count
    q, k, v = _tok(1)
    with pytest.raises(ValueError, match="v has shape"):
        mhla_amd.mhla_causal_step(q, k, torch.zeros(B, 1, H, V), mix, _state(HK))


def test_layer_refuses_grouped_state_without_exact_decoding():
    from mhla_amd.modules.fla import MHLA
    with pytest.raises(ValueError, match="exact_decoding"):
        MHLA(hidden_size=64, num_heads=4, num_kv_heads=2, feature_map="relu", grouped_state=True, layer_idx=0)
    layer = MHLA(hidden_size=64, num_heads=4, num_kv_heads=2, feature_map="relu", exact_decoding=True, grouped_state=True, layer_idx=0)
    assert layer.grouped_state and not MHLA(hidden_size=64, num_heads=4, feature_map="relu").grouped_state
    from mhla_amd.hosts.gpt import GPT_MHLA
    model = GPT_MHLA(vocab_size=32, hidden_size=64, num_layers=2, num_heads=4, exact_decoding=True, num_kv_heads=2, grouped_state=True)
    assert all(blk.attn.grouped_state and blk.attn.num_kv_heads == 2 for blk in model.layers)
