"""Grouped-query heads in the causal operator's forward (k, v with Hkv heads, q with H = G Hkv) as far as a machine without a GPU
reaches it: the refusals `ops` makes before the library is loaded, the empty-sequence early return, the order in which the
gradient path expands k and v, and the new C-ABI symbols with their static checks.  The kernels are in
tests/test_gpu_causal_gqa_forward.py."""
import os
import re

import pytest
import torch

import mhla_amd
from mhla_amd import ops

NEW = ("mhla_causal_fwd_gqa", "mhla_causal_normgate_fwd_gqa", "mhla_causal_varlen_fwd_gqa", "mhla_causal_varlen_normgate_fwd_gqa")
EINVAL, ENOTSUP = -22, -95
B, T, K, V = 2, 70, 16, 8


@pytest.fixture
def no_load(monkeypatch):
    """Every refusal below must come before the library is loaded."""
    from mhla_amd import _lib

    def load():
        raise AssertionError("the library was loaded before the arguments were refused")
    monkeypatch.setattr(_lib, "load", load)


def _tok(H, Hk, Hv=None, T=T):
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(B, T, H, K), r(B, T, Hk, K), r(B, T, Hk if Hv is None else Hv, V), torch.rand(4, 4, generator=g)


@pytest.mark.parametrize("fn", ["mhla_causal", "mhla_causal_normgate", "mhla_causal_prefill"])
def test_head_counts_are_refused_before_the_library(fn, no_load):
    call = {"mhla_causal": lambda q, k, v, m: mhla_amd.mhla_causal(q, k, v, m),
            "mhla_causal_normgate": lambda q, k, v, m: mhla_amd.mhla_causal_normgate(q, k, v, m, None, None),
            "mhla_causal_prefill": lambda q, k, v, m: mhla_amd.mhla_causal_prefill(q, k, v, m)}[fn]
    with pytest.raises(ValueError, match="H must be a multiple of Hkv"):
        call(*_tok(6, 4))
    with pytest.raises(NotImplementedError, match="at most 8 per k/v head"):
        call(*_tok(16, 1))


@pytest.mark.parametrize("fn", ["mhla_causal", "mhla_causal_normgate"])
def test_k_and_v_on_different_head_counts(fn, no_load):
    q, k, v, m = _tok(4, 2, Hv=1)
    with pytest.raises(ValueError, match=r"v has shape \(2, 70, 1, 8\), expected \(2, 70, 2, 8\)"):
        getattr(mhla_amd, fn)(q, k, v, m, *((None, None) if fn == "mhla_causal_normgate" else ()))


def test_gate_on_the_kv_heads(no_load):
    q, k, v, m = _tok(4, 2)
    with pytest.raises(ValueError, match=r"gate has shape \(2, 70, 2, 8\), expected \(2, 70, 4, 8\)"):
        mhla_amd.mhla_causal_normgate(q, k, v, m, torch.zeros(B, T, 2, V), None)


@pytest.mark.parametrize("grad", [False, True], ids=["no-grad", "grad"])
def test_empty_sequence_returns_query_heads_without_the_library(grad, no_load):
    q, k, v, m = _tok(4, 2, T=0)
    q.requires_grad_(grad)
    o = mhla_amd.mhla_causal(q, k, v, m)
    assert o.shape == (B, 0, 4, V) and o.dtype == v.dtype
    q0, k0, v0, _ = _tok(4, 2)
    assert mhla_amd.mhla_causal(q0[:0], k0[:0], v0[:0], m).shape == (0, T, 4, V)


def test_gradient_path_expands_in_the_layers_order():
    """Head h of the expanded tensor is k/v head h // G: the labelled tensor's expand + reshape equals repeat_interleave(G, 2), and
    the gradient of a head is the sum over its group."""
    Hk, G = 3, 4
    lab = (torch.arange(Hk, dtype=torch.float32).view(1, 1, Hk, 1) * 100 + torch.arange(5, dtype=torch.float32).view(1, 5, 1, 1) * 10
           + torch.arange(2, dtype=torch.float32)).repeat(2, 1, 1, 1).requires_grad_(True)
    e = ops._expand_kv(lab, G)
    assert e.shape == (2, 5, Hk * G, 2) and torch.equal(e, lab.repeat_interleave(G, 2))
    assert [int(e[0, 0, h, 0]) // 100 for h in range(Hk * G)] == [h // G for h in range(Hk * G)]
    w = torch.arange(Hk * G, dtype=torch.float32).view(1, 1, Hk * G, 1).expand_as(e)
    (e * w).sum().backward()
    want = torch.tensor([sum(range(j * G, (j + 1) * G)) for j in range(Hk)], dtype=torch.float32).view(1, 1, Hk, 1).expand_as(lab)
    assert torch.equal(lab.grad, want)
    from mhla_amd.modules import MHLA
    layer = MHLA(hidden_size=64, num_heads=4, num_kv_heads=2, feature_map="relu")
    k = torch.randn(1, 3, 2, layer.head_k_dim)
    v = torch.randn(1, 3, 2, layer.head_v_dim)
    rk, rv = layer._repeat_kv(k, v)
    assert torch.equal(rk, ops._expand_kv(k, 2)) and torch.equal(rv, ops._expand_kv(v, 2))


def _lib():
    from mhla_amd import build as b, _lib
    b.build()
    return _lib, _lib.load()


def test_new_symbols_are_declared_bound_and_exported_at_abi_9():
    _l, lib = _lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mhla_hip.h")).read()
    for name in NEW:
        old = name[:-len("_gqa")]
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared in mhla_hip.h"
        assert callable(getattr(lib, name))
        # the namesake with ONE more integer (Hkv, after H)
        assert len(_l.SIGNATURES[name][1]) == len(_l.SIGNATURES[old][1]) + 1 and _l.SIGNATURES[name][0] is _l.SIGNATURES[old][0]
    assert lib.mhla_abi_version() == _l.ABI_VERSION == 9


@pytest.mark.parametrize("name", NEW)
def test_head_counts_are_checked_before_anything_touches_a_device(name):
    """Null tensors and a null workspace: a call that got past the head-count checks fails on them (EINVAL) without a launch."""
    _l, lib = _lib()
    nul = _l.NULL_VIEW
    y = _l.View(4096, 64, 64, 64)   # (never read: the fused calls look at y's pointer first, and q's null pointer stops every call)
    varlen, norm = "varlen" in name, "normgate" in name

    def call(H, Hkv, Bc=1):
        args = [nul, nul, nul, None, 4, nul] + ([nul, None, 1e-5, y] if norm else []) + [None, 0, Bc, 64, H, Hkv, 64, 64, 64]
        args += ([1, 4096] if varlen else [])   # (a table pointer that is never read)
        args += [0.125, _l.BF16, 0, None]
        rc = getattr(lib, name)(*args)
        return rc, lib.mhla_last_error().decode()

    rc, msg = call(4, 0)
    assert rc == EINVAL and "Hkv" in msg
    rc, msg = call(6, 4)
    assert rc == EINVAL and "multiple of Hkv" in msg
    rc, msg = call(16, 1)
    assert rc == ENOTSUP and "at most 8" in msg
    rc, msg = call(8, 1, Bc=8192)   # B * H counts query heads: 65536 pairs on 8192 k/v pairs
    assert rc == ENOTSUP and "grid limit" in msg
    rc, msg = call(4, 2)            # accepted head counts: the namesake's own checks follow
    assert rc == EINVAL and "Hkv" not in msg
