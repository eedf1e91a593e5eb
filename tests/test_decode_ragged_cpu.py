"""Ragged decode states (one length per sequence) as far as a machine without a GPU reaches them: the `CausalState` container with
`lengths` / `pos`, `CausalState.cat`, the `lengths=` checks of mhla_causal_state / mhla_causal_prefill, the checks mhla_causal_step
and mhla_causal_extend share (the cases of tests/test_decode_validation_cpu.py, on a ragged state), and the C-ABI symbol.  The
kernels are in tests/test_gpu_causal_ragged.py."""
import pytest
import torch

import mhla_amd
from mhla_amd import CausalState

B, H, K, V, CAP = 2, 3, 16, 24, 5
LENGTHS = (7, 70)


def _from_empty(lengths, k=K, cap=CAP, chunk=64):
    e = CausalState.empty(len(lengths), H, k, V, cap, device="cpu", chunk_size=chunk)
    return CausalState(e.S, e.P, e.Cur, 0, chunk, lengths=lengths)


def test_state_with_lengths():
    st = _from_empty([7, 70])
    assert st.lengths == (7, 70) and st.seen == 70
    assert st.pos.dtype == torch.int32 and st.pos.tolist() == [7, 70] and st.pos.device == st.S.device
    assert "lengths=(7, 70)" in repr(st) and "seen=" not in repr(st)
    assert st.nbytes == 4 * (st.S.numel() + st.P.numel() + st.Cur.numel() + 2)
    c = st.clone()
    assert c.lengths == st.lengths and c.seen == 70 and torch.equal(c.pos, st.pos)
    assert c.pos.data_ptr() != st.pos.data_ptr() and c.S.data_ptr() != st.S.data_ptr()
    c.pos += 1
    c.lengths = tuple(n + 1 for n in c.lengths)
    assert st.pos.tolist() == [7, 70] and st.lengths == (7, 70)
    # equal lengths given as lengths= stay ragged; a state without them is uniform as before
    eq = _from_empty([60, 60])
    assert eq.lengths == (60, 60) and eq.pos is not None and eq.seen == 60
    u = CausalState.empty(2, H, K, V, CAP, device="cpu")
    assert u.lengths is None and u.pos is None and "seen=0" in repr(u) and u.clone().lengths is None
    assert u.nbytes == 4 * (u.S.numel() + u.P.numel() + u.Cur.numel())
    # the positional signature is the old one
    p = CausalState(u.S, u.P, u.Cur, 9, 64)
    assert p.seen == 9 and p.chunk_size == 64 and p.lengths is None
    for bad in ([1], [1, 2, 3], [-1, 2]):
        with pytest.raises(ValueError, match="lengths"):
            CausalState(u.S, u.P, u.Cur, lengths=bad)


def test_cat():
    def uniform(b, seen, **kw):
        s = CausalState.empty(b, H, kw.get("k", K), V, kw.get("cap", CAP), device="cpu", chunk_size=kw.get("chunk", 64))
        s.seen = seen
        s.Cur.fill_(float(seen))
        return s
    a, b, c = uniform(1, 5), uniform(2, 5), uniform(1, 9)
    same = CausalState.cat([a, b])
    assert same.lengths is None and same.pos is None and same.seen == 5 and same.S.shape[0] == same.P.shape[0] == same.Cur.shape[0] == 3
    mixed = CausalState.cat([a, b, c])
    assert mixed.lengths == (5, 5, 5, 9) and mixed.seen == 9 and mixed.pos.tolist() == [5, 5, 5, 9] and mixed.S.shape[0] == 4
    assert mixed.Cur[:, 0, 0, 0].tolist() == [5.0, 5.0, 5.0, 9.0]
    assert mixed.Cur.data_ptr() != a.Cur.data_ptr()
    # a ragged input keeps the result ragged, even at equal lengths
    r = CausalState.cat([_from_empty([5]), a])
    assert r.lengths == (5, 5)
    again = CausalState.cat([mixed, _from_empty([0, 64])])
    assert again.lengths == (5, 5, 5, 9, 0, 64) and again.seen == 64
    for other in (uniform(1, 5, k=K + 4), uniform(1, 5, cap=CAP + 1), uniform(1, 5, chunk=32)):
        with pytest.raises(ValueError, match="CausalState.cat"):
            CausalState.cat([a, other])
    with pytest.raises(ValueError):
        CausalState.cat([])


@pytest.mark.parametrize("fn", ["mhla_causal_state", "mhla_causal_prefill"])
def test_lengths_are_checked_before_the_device(fn):
    T = 10
    q, k, v, mix = torch.zeros(B, T, H, K), torch.zeros(B, T, H, K), torch.zeros(B, T, H, V), torch.ones(CAP, CAP)
    call = (lambda **kw: mhla_amd.mhla_causal_state(k, v, mix, **kw)) if fn == "mhla_causal_state" else \
        (lambda **kw: mhla_amd.mhla_causal_prefill(q, k, v, mix, **kw))
    for bad in ([3], [3, 4, 5], [-1, 4], [3, T + 1], torch.tensor([3, T + 1])):
        with pytest.raises(ValueError, match="lengths"):
            call(lengths=bad)
        with pytest.raises(ValueError, match="lengths"):
            call(lengths=bad, left_padded=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # good lengths reach the device check
        call(lengths=[3, T], left_padded=True)


FUNCS = [("mhla_causal_step", 1), ("mhla_causal_extend", 5)]
OTHER = {"mhla_causal_step": "mhla_causal_extend", "mhla_causal_extend": "mhla_causal_step"}


def _raises(name, exc, match, *args, **kw):
    with pytest.raises(exc, match=match) as info:
        getattr(mhla_amd, name)(*args, **kw)
    assert type(info.value) is exc, f"{type(info.value).__name__}, expected {exc.__name__}"
    assert OTHER[name] not in str(info.value), f"{name} raised a message naming {OTHER[name]}: {info.value}"
    return str(info.value)


@pytest.mark.parametrize("name,T", FUNCS)
def test_shared_checks_on_a_ragged_state(name, T):
    state = _from_empty(LENGTHS)
    mix, q, k, v = torch.ones(CAP, CAP), torch.zeros(B, T, H, K), torch.zeros(B, T, H, K), torch.zeros(B, T, H, V)
    _raises(name, RuntimeError, "no CPU fallback", q, k, v, mix, state)
    assert name in _raises(name, TypeError, "must be a CausalState", q, k, v, mix, (state.S, state.P, state.Cur))
    _raises(name, ValueError, None, q[0], k, v, mix, state)
    assert name in _raises(name, ValueError, "v has shape", q, k, v[:, :, :2], mix, state)
    assert name in _raises(name, ValueError, "k has dtype", q, k.bfloat16(), v, mix, state)
    assert name in _raises(name, ValueError, "unsupported dtype", q.double(), k.double(), v.double(), mix, state)
    assert name in _raises(name, ValueError, "gate has shape", q, k, v, mix, state, gate=torch.zeros(B, T, H, V + 1))
    other_v = CausalState(state.S, torch.zeros(B, H, K, V + 1), state.Cur, lengths=LENGTHS)
    msg = _raises(name, ValueError, r"state is CausalState\(", q, k, v, mix, other_v)
    assert name in msg and "lengths=(7, 70)" in msg
    assert name in _raises(name, ValueError, "norm_weight has 25 entries", q, k, v, mix, state, norm_weight=torch.ones(V + 1))
    assert name in _raises(name, RuntimeError, "inference only", q.clone().requires_grad_(), k, v, mix, state)
    # order: the state's type before the shapes, the size of norm_weight before requires-grad
    _raises(name, TypeError, "must be a CausalState", q, k, v[:, :, :2], mix, (state.S, state.P, state.Cur))
    _raises(name, ValueError, "norm_weight has 25 entries", q.clone().requires_grad_(), k, v, mix, state, norm_weight=torch.ones(V + 1))
    for st in (state, other_v):
        assert st.lengths == LENGTHS and st.seen == 70 and st.pos.tolist() == list(LENGTHS)
    assert float(state.S.abs().max()) == float(state.P.abs().max()) == float(state.Cur.abs().max()) == 0.0


def test_token_counts_on_a_ragged_state():
    state = _from_empty(LENGTHS)
    mix, q, k, v = torch.ones(CAP, CAP), torch.zeros(B, 2, H, K), torch.zeros(B, 2, H, K), torch.zeros(B, 2, H, V)
    assert "mhla_causal_step" in _raises("mhla_causal_step", ValueError, "one token per call", q, k, v, mix, state)
    assert "mhla_causal_extend" in _raises("mhla_causal_extend", ValueError, "at least one token", q[:, :0], k[:, :0], v[:, :0], mix, state)
    assert state.lengths == LENGTHS and state.pos.tolist() == list(LENGTHS)


def test_ragged_entry_point_is_exported_at_abi_9():
    from mhla_amd import build as b, _lib
    b.build()
    lib = _lib.load()
    assert "mhla_causal_step_ragged" in _lib.SIGNATURES and callable(lib.mhla_causal_step_ragged)
    assert lib.mhla_abi_version() == _lib.ABI_VERSION == 9
    # its argument checks are host arithmetic, run before anything touches a device: a null position array is refused
    nv = _lib.NULL_VIEW
    rc = lib.mhla_causal_step_ragged(nv, nv, nv, None, 0, None, 0, None, None, None, 0, 0, nv, nv, None, 1e-5, nv, None, 0,
                                     1, 1, 4, 4, 64, 1.0, _lib.F32, None)
    assert rc == -22 and lib.mhla_last_error()
    # max_pos and any_boundary take the place of pos in the checks of the uniform step, all made before any launch.  The addresses
    # below are made up and never dereferenced on the host; every case has a second, independent reason to be refused -- a null
    # workspace, the last check before the launches -- so that no loosening of one check can launch on them.
    fake = lambda: _lib.View(0x10000, 64, 64, 16)

    def raw(max_pos, any_boundary, ldmix=2, cap=2, pos=0x10000):
        return lib.mhla_causal_step_ragged(fake(), fake(), fake(), 0x10000, ldmix, 0x10000, cap, 0x10000, 0x10000, pos, max_pos, any_boundary,
                                           fake(), nv, None, 1e-5, nv, None, 0, 1, 1, 4, 4, 64, 1.0, _lib.F32, None)
    assert raw(10, 0) == -22 and b"workspace too small" in lib.mhla_last_error()   # (the second reason, on its own)
    assert raw(128, 0) == -22 and b"the state holds 2" in lib.mhla_last_error()
    assert raw(-1, 0) == -22 and b"max_pos" in lib.mhla_last_error()
    assert raw(0, 0, pos=None) == -22 and b"pos_dev" in lib.mhla_last_error()
    assert raw(63, 1, ldmix=1) == -22 and b"row 1 of mix is read" in lib.mhla_last_error()   # a boundary at chunk 0 reads row 1
    assert raw(64, 0, ldmix=1) == -22 and b"row 1 of mix is read" in lib.mhla_last_error()
