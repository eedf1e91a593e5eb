"""The block-mix host layer of `mhla_amd/ops.py` (`mhla_blockmix`, `mhla_blockmix_rope`, `mhla_dit_core`, `mhla_blockmix_wan_pro`)
on CPU tensors against the recording stand-in for the library (tools/fake_decode_lib.py), with the Python autograd nodes forced:
what each public call hands the C ABI -- views, offsets, strides, workspaces, flags and the order of launches -- forward and
backward.  tools/record_blockmix_calls.py records the whole section the same way."""
import os
import sys

import pytest
import torch

from mhla_amd import _lib, ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from fake_decode_lib import Session  # noqa: E402

B, M, S, H, D = 3, 4, 16, 2, 32
N, C = M * S, H * D
TOKENS = (N * H * D, H * D, D)   # strides of a contiguous [B, N, H, D]
PACKED = (N * 3 * C, 3 * C, D)   # strides of a slice of the packed projection [B, N, 3, H, D]


@pytest.fixture(autouse=True)
def python_nodes(monkeypatch):
    from mhla_amd import build
    build.build(verbose=False)
    monkeypatch.setattr(ops, "_native_nodes", lambda: False)   # (the C++ nodes refuse CPU tensors)


def _rand(*shape, dtype=torch.float32, seed=0, grad=True):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).requires_grad_(grad)


def _record(s, fn, wrt=(), **names):
    """The library calls of `fn()` and, with `wrt`, of its backward; both inside one recorded call, so that storage the forward
    allocates ("new<n>", or the name `_named_workspaces` gives) keeps its name in the backward's arguments."""
    s.name(**names)

    def both():
        out = fn()
        return torch.autograd.grad(out, wrt, torch.ones_like(out)) if wrt else out
    first = len(s.calls)
    s.call("case", both, catch=False)
    return s.calls[first:]


def _named_workspaces(s, monkeypatch):
    """Every workspace the section allocates (`ops._ws`) is named "ws<n>" in order; returns the list they are collected in."""
    made, real = [], ops._ws

    def named(nbytes, device):
        made.append(real(nbytes, device))
        s.name(**{f"ws{len(made) - 1}": made[-1]})
        return made[-1]
    monkeypatch.setattr(ops, "_ws", named)
    return made


def _tail(call):
    """(kept forward workspace or None, B, H, M, S, D, dtype code, eps, flags) of a block-mix launch: what follows its workspace"""
    i = next(i for i, a in enumerate(call.args) if isinstance(a, tuple) and a[0] == "ws")
    rest = call.args[i + 1:-1]
    return (rest[0], *rest[1:]) if isinstance(rest[0], tuple) else (None, *rest)


def _views(call):
    return [a for a in call.args if isinstance(a, tuple) and a[0] == "view"]


def test_dit_core_and_blockmix_hand_the_operator_the_same_arguments():
    qkv, W = _rand(B, N, 3, H, D, dtype=torch.bfloat16, seed=1), _rand(M, M, seed=2)
    lw, lb = _rand(C, 1, 3, 3, seed=3), _rand(C, seed=4)
    with Session(ops, _lib) as s:
        dit = _record(s, lambda: ops.mhla_dit_core(qkv, W, lw, lb, 2, 4), (qkv, W, lw, lb), qkv=qkv, W=W, lw=lw, lb=lb)
        bm = _record(s, lambda: ops.mhla_blockmix(*qkv.unbind(2), W, relu_eps=True), (qkv, W), qkv=qkv, W=W)
    assert [c.name for c in dit] == ["mhla_blockmix_fwd", "mhla_lepe2d", "mhla_blockmix_bwd", "mhla_lepe2d", "mhla_lepe2d_wgrad"]
    assert [c.name for c in bm] == ["mhla_blockmix_fwd", "mhla_blockmix_bwd"]
    # forward: everything but the output view (argument 7), which is fresh contiguous storage in both
    f_dit, f_bm = dit[0].args, bm[0].args
    assert f_dit[:7] == f_bm[:7] and f_dit[8:] == f_bm[8:]
    assert [a[1:] for a in f_dit[:3]] == [("qkv", 0, *PACKED), ("qkv", C, *PACKED), ("qkv", 2 * C, *PACKED)]   # read in place
    assert f_dit[3:5] == f_dit[:2]                                                      # the normaliser reads q, k themselves
    assert f_dit[7][0] == f_bm[7][0] == "view" and f_dit[7][2:] == f_bm[7][2:] == (0, *TOKENS)
    assert f_dit[7][1].startswith("new") and f_bm[7][1].startswith("new")
    assert _tail(dit[0])[-1] == _tail(bm[0])[-1] == _lib.FLAG_RELU_EPS
    # backward: everything but out, dout, the five gradient views, dW and the kept workspace (arguments 7 ... 14 and 17)
    b_dit, b_bm = dit[2].args, bm[1].args
    assert len(b_dit) == len(b_bm) == len(_lib.SIGNATURES["mhla_blockmix_bwd"][1]) - 1    # (workspace and size are one entry)
    assert b_dit[:7] == b_bm[:7] == f_dit[:7] and b_dit[15:17] == b_bm[15:17] and b_dit[18:] == b_bm[18:]
    for i in (7, 8):     # out and dout: contiguous [B, N, H, D] in both
        assert b_dit[i][0] == b_bm[i][0] == "view" and b_dit[i][2:] == b_bm[i][2:] == (0, *TOKENS)
    assert b_dit[7] == f_dit[7] and b_bm[7] == f_bm[7]                                   # the forward's own output
    # dq, dk: the q and k slices of one packed gradient from the DiT node, fresh tensors from the plain node; dv fresh in both
    packed = b_dit[9][1]
    assert [a[1:] for a in b_dit[9:11]] == [(packed, 0, *PACKED), (packed, C, *PACKED)] and b_dit[11][2:] == (0, *TOKENS)
    assert b_dit[11][1] != packed
    assert all(a[2:] == (0, *TOKENS) for a in b_bm[9:12]) and len({a[1] for a in b_bm[9:12]}) == 3
    assert b_dit[12:14] == b_bm[12:14] == (("null",), ("null",))
    assert b_dit[14][0] == b_bm[14][0] == "ptr" and b_dit[14][2] == b_bm[14][2] == 0
    assert b_dit[17][0] == b_bm[17][0]                                                   # kept by both or recomputed by both


@pytest.mark.parametrize("den", [False, True], ids=["q k", "q_den k_den"])
def test_a_sliced_batch_covers_every_sequence_once_and_backward_in_reverse(den, monkeypatch):
    monkeypatch.setattr(ops, "_MAX_GRID_BH", 2 * H)
    t = dict(q=_rand(B, N, H, D, seed=1), k=_rand(B, N, H, D, seed=2), v=_rand(B, N, H, D, seed=3), W=_rand(M, M, seed=4))
    extra = dict(q_den=_rand(B, N, H, D, seed=5), k_den=_rand(B, N, H, D, seed=6)) if den else {}
    with Session(ops, _lib) as s:
        calls = _record(s, lambda: ops.mhla_blockmix(t["q"], t["k"], t["v"], t["W"], **extra), (*t.values(), *extra.values()), **t, **extra)
    assert [c.name for c in calls] == ["mhla_blockmix_fwd"] * 2 + ["mhla_blockmix_bwd"] * 2
    assert [_tail(c)[1] for c in calls] == [2, 1, 1, 2]
    inputs = ("q", "k", "v") + tuple(extra)
    for c, first in zip(calls, (0, 2, 2, 0)):
        mine = {a[1]: a for a in _views(c) if a[1] in inputs}
        assert set(mine) == set(inputs)
        for _, base, offset, sb, sn, sh in mine.values():
            assert (offset, sb, sn, sh) == (first * sb, *TOKENS), f"{c.name}: the view of {base} does not start at sequence {first}"
        assert c.args[3][1] == ("q_den" if den else "q") and c.args[4][1] == ("k_den" if den else "k")
        assert c.args[5] == ("ptr", "W", 0)
        # the output and the gradients are storage made inside the call, never the caller's
        assert all(a[1].startswith("new") for a in _views(c) if a[1] not in inputs)


def test_a_batch_within_the_limit_is_one_call_on_the_callers_tensors():
    assert ops._MAX_GRID_BH == 65535
    proj, W = _rand(B, N, 3 * C, seed=1), _rand(M, M, seed=2)
    with Session(ops, _lib) as s:
        calls = _record(s, lambda: ops.mhla_blockmix(*proj.view(B, N, 3, H, D).unbind(2), W), (proj, W), proj=proj, W=W)
    assert [c.name for c in calls] == ["mhla_blockmix_fwd", "mhla_blockmix_bwd"] and [_tail(c)[1] for c in calls] == [B, B]
    for c in calls:
        assert list(c.args[:5]) == [("view", "proj", i * C, *PACKED) for i in (0, 1, 2, 0, 1)]


def _keep_cases():
    """(node, entry point, forward, inputs) at blocks of 64 tokens: the library keeps no state for the single-launch path of 16"""
    N = M * 64
    W = _rand(M, M, seed=4)
    q, k, v = (_rand(B, N, H, D, dtype=torch.bfloat16, seed=i) for i in (1, 2, 3))
    yield "_BlockMix", "mhla_blockmix", (lambda: ops.mhla_blockmix(q, k, v, W)), (q, k, v, W)
    qf, kf, vf = (_rand(B, N, H, D, seed=i) for i in (1, 2, 3))
    cos, sin = _rand(N, D // 2, seed=5, grad=False), _rand(N, D // 2, seed=6, grad=False)
    yield "_BlockMixRope", "mhla_blockmix_rope", (lambda: ops.mhla_blockmix_rope(qf, kf, vf, W, cos, sin)), (qf, kf, vf, W)
    qkv, lw = _rand(B, N, 3, H, D, dtype=torch.bfloat16, seed=1), _rand(C, 1, 3, 3, seed=3)
    yield "_DitCore", "mhla_blockmix", (lambda: ops.mhla_dit_core(qkv, W, lw, None, 2, 8)), (qkv, W, lw)


@pytest.mark.parametrize("limit", [1 << 30, 0])
@pytest.mark.parametrize("node", ["_BlockMix", "_BlockMixRope", "_DitCore"])
def test_the_backward_is_handed_the_forwards_workspace_within_the_keep_limit(node, limit, monkeypatch):
    monkeypatch.setattr(ops, "KEEP_STATE_LIMIT_BYTES", limit)
    _, entry, fn, wrt = next(c for c in _keep_cases() if c[0] == node)
    with Session(ops, _lib) as s:
        made = _named_workspaces(s, monkeypatch)
        calls = {c.name: c for c in _record(s, fn, wrt)}
    fwd, bwd = calls[entry + "_fwd"], calls[entry + "_bwd"]
    assert _tail(fwd)[0] is None                                                 # a forward takes no kept workspace
    assert 0 < made[0].numel() * 4 <= 1 << 30
    assert _tail(bwd)[0] == (("ptr", "ws0", 0) if limit else ("null",))          # ws0: the first workspace made, the forward's
    assert _tail(bwd)[1:] == _tail(fwd)[1:]                                      # the same problem, eps and flags both ways


def test_an_aligned_view_is_passed_in_place_and_a_misaligned_one_as_a_copy():
    proj, W = _rand(B, N, 3 * C, seed=1), _rand(M, M, seed=2)
    flat, wide = _rand(B * N * 3 * C + 2, seed=3), _rand(B, N, H, 2 * D, seed=4)
    q, k, v = proj.view(B, N, 3, H, D)[:, :, 1], flat[2:].view(B, N, 3, H, D)[:, :, 1], wide[..., ::2]
    assert q.data_ptr() % 16 == 0 and k.data_ptr() % 16 == 8 and k.stride() == q.stride() and v.stride(3) == 2
    with Session(ops, _lib) as s:
        fwd, bwd = _record(s, lambda: ops.mhla_blockmix(q, k, v, W), (proj, flat, wide, W), proj=proj, flat=flat, wide=wide, W=W)
    for c in (fwd, bwd):
        qv, kv, vv = c.args[:3]
        assert qv == ("view", "proj", C, *PACKED)                                # the caller's storage, the caller's strides
        for copied in (kv, vv):                                                  # new contiguous storage
            assert copied[1].startswith("new") and copied[2:] == (0, *TOKENS)
        assert kv[1] != vv[1]
    assert bwd.args[:3] == fwd.args[:3]                                          # the backward reads the forward's copies


@pytest.mark.parametrize("call", ["mhla_blockmix", "mhla_dit_core"])
def test_the_flags_tell_the_forward_whether_a_backward_will_come(call):
    W, lw = _rand(M, M, seed=2, grad=False), _rand(C, 1, 3, 3, seed=3, grad=False)

    def flags(grad, no_grad=False):
        qkv = _rand(B, N, 3, H, D, seed=1, grad=grad)
        fn = (lambda: ops.mhla_blockmix(*qkv.unbind(2), W)) if call == "mhla_blockmix" else (lambda: ops.mhla_dit_core(qkv, W, lw, None, 2, 4))
        with Session(ops, _lib) as s, torch.set_grad_enabled(not no_grad):
            return _tail(_record(s, fn, qkv=qkv, W=W)[0])[-1]
    assert flags(grad=True) & _lib.FLAG_NO_BWD_STATE == 0                        # one leaf requires grad
    assert flags(grad=False) & _lib.FLAG_NO_BWD_STATE
    assert flags(grad=True, no_grad=True) & _lib.FLAG_NO_BWD_STATE


def test_wan_pro_launches_its_two_rstd_kernels_before_the_operator():
    proj = _rand(B, N, 3 * C, dtype=torch.bfloat16, seed=1, grad=False)
    q, k, v = proj.view(B, N, 3 * H, D).split(H, dim=2)
    W, wq = _rand(M, M, seed=2, grad=False), _rand(C, seed=3, grad=False)

    def launches(**kw):
        with Session(ops, _lib) as s:
            return _record(s, lambda: ops.mhla_blockmix_wan_pro(q, k, v, wq, wq, 1e-6, W, None, None, None, 1e-6, None, **kw), proj=proj, W=W, wq=wq)
    calls = launches()
    assert [c.name for c in calls] == ["mhla_rms_rstd", "mhla_rms_rstd", "mhla_blockmix_wan_pro_fwd"]
    # the rows of q, then of k, each into an rstd vector of its own, which the operator then reads in that order
    assert [c.args[0] for c in calls[:2]] == [("ptr", "proj", 0), ("ptr", "proj", C * proj.element_size())] and all(c.args[1] == 3 * C for c in calls[:2])
    assert calls[2].args[3:5] == (calls[0].args[2], calls[1].args[2]) and calls[0].args[2] != calls[1].args[2]
    assert [c.name for c in launches(qk_norm=False)] == ["mhla_blockmix_wan_pro_fwd"]
    assert launches(qk_norm=False)[0].args[3:5] == (("null",), ("null",))
