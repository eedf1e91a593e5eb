"""The argument checks that mhla_causal_step and mhla_causal_extend share, as far as a machine without a GPU (and without the
built library) reaches them: every check up to the device test.  Both functions refuse the same arguments with the same
exception type, name the function that was called, in the same order, and leave the state untouched.  The checks behind the
device test are in tests/test_gpu_causal_extend.py."""
import pytest
import torch

import mhla_amd

B, H, K, V, CAP = 2, 3, 16, 24, 5
FUNCS = [("mhla_causal_step", 1), ("mhla_causal_extend", 5)]
OTHER = {"mhla_causal_step": "mhla_causal_extend", "mhla_causal_extend": "mhla_causal_step"}


def _setup(T):
    state = mhla_amd.CausalState.empty(B, H, K, V, CAP, device="cpu")
    state.seen = 7
    return state, torch.ones(CAP, CAP), torch.zeros(B, T, H, K), torch.zeros(B, T, H, K), torch.zeros(B, T, H, V)


def _raises(name, exc, match, *args, **kw):
    with pytest.raises(exc, match=match) as info:
        getattr(mhla_amd, name)(*args, **kw)
    assert type(info.value) is exc, f"{type(info.value).__name__}, expected {exc.__name__}"
    assert OTHER[name] not in str(info.value), f"{name} raised a message naming {OTHER[name]}: {info.value}"
    return str(info.value)


@pytest.mark.parametrize("name,T", FUNCS)
def test_checks_before_the_device_check(name, T):
    state, mix, q, k, v = _setup(T)
    _raises(name, RuntimeError, "no CPU fallback", q, k, v, mix, state)
    assert name in _raises(name, TypeError, "must be a CausalState", q, k, v, mix, (state.S, state.P, state.Cur))
    _raises(name, ValueError, None, q[0], k, v, mix, state)
    assert name in _raises(name, ValueError, "v has shape", q, k, v[:, :, :2], mix, state)
    assert name in _raises(name, ValueError, "k has dtype", q, k.bfloat16(), v, mix, state)
    assert name in _raises(name, ValueError, "unsupported dtype", q.double(), k.double(), v.double(), mix, state)
    assert name in _raises(name, ValueError, "gate has shape", q, k, v, mix, state, gate=torch.zeros(B, T, H, V + 1))
    other_v = mhla_amd.CausalState(state.S, torch.zeros(B, H, K, V + 1), state.Cur, 7)
    assert name in _raises(name, ValueError, r"state is CausalState\(", q, k, v, mix, other_v)
    assert name in _raises(name, ValueError, "norm_weight has 25 entries", q, k, v, mix, state, norm_weight=torch.ones(V + 1))
    assert name in _raises(name, RuntimeError, "inference only", q.clone().requires_grad_(), k, v, mix, state)
    assert state.seen == 7 and other_v.seen == 7
    assert float(state.S.abs().max()) == float(state.P.abs().max()) == float(state.Cur.abs().max()) == 0.0


def test_token_counts():
    state, mix, q, k, v = _setup(2)
    assert "mhla_causal_step" in _raises("mhla_causal_step", ValueError, "one token per call", q, k, v, mix, state)
    assert "mhla_causal_extend" in _raises("mhla_causal_extend", ValueError, "at least one token", q[:, :0], k[:, :0], v[:, :0], mix, state)
    assert state.seen == 7 and float(state.S.abs().max()) == float(state.P.abs().max()) == float(state.Cur.abs().max()) == 0.0


@pytest.mark.parametrize("name,T", FUNCS)
def test_order_of_the_checks(name, T):
    state, mix, q, k, v = _setup(T)
    # the state's type comes before the tensors' shapes
    _raises(name, TypeError, "must be a CausalState", q, k, v[:, :, :2], mix, (state.S, state.P, state.Cur))
    # the size of norm_weight comes before requires-grad
    _raises(name, ValueError, "norm_weight has 25 entries", q.clone().requires_grad_(), k, v, mix, state, norm_weight=torch.ones(V + 1))
    assert state.seen == 7
