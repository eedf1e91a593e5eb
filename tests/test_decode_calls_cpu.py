"""The batch slicing of the decode host layer (`ops._batch_slices`), which is otherwise reached only with more than 65535 (b, h)
pairs or a lowered limit on a GPU: each of the five sliced entry points runs on CPU tensors against the recording stand-in for the
library (tools/fake_decode_lib.py), once with `_MAX_GRID_BH = 2 H`, so that B = 3 runs as 2 + 1, and once with the limit untouched."""
import os
import sys

import pytest
import torch

import mhla_amd
from mhla_amd import CausalState, _lib, ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from fake_decode_lib import Session, batch_of  # noqa: E402

B, H, K, V, CAP, T = 3, 4, 16, 24, 5, 5
LENGTHS, COUNTS, ACCEPT = (6, 133, 127), (3, 2, 5), (1, 2, 3)


def _inputs(Hk, T):
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(q=r(B, T, H, K), k=r(B, T, Hk, K), v=r(B, T, Hk, V), gate=r(B, T, H, V), mix=torch.rand(CAP, CAP, generator=g), w=torch.rand(V, generator=g))


def _run(entry, Hk, s):
    """One public call of `entry` on a fresh ragged state; returns (the library calls it made, its named tensors, the state)."""
    from mhla_amd import build
    build.build(verbose=False)
    t = _inputs(Hk, 1 if "step" in entry else T)
    e = CausalState.empty(B, Hk, K, V, CAP, device="cpu")
    state = CausalState(e.S, e.P, e.Cur, 0, 64, lengths=LENGTHS)
    s.name(**t, S=state.S, P=state.P, Cur=state.Cur, pos=state.pos, full=state.full)
    tok, epi = (t["q"], t["k"], t["v"], t["mix"], state), dict(gate=t["gate"], norm_weight=t["w"])
    first = len(s.calls)
    call = lambda fn, *a, **kw: s.call(entry, fn, *a, catch=False, **kw)   # (storage allocated inside is named "new<n>")
    if entry == "step":
        call(mhla_amd.mhla_causal_step, *tok, **epi)
    elif entry == "step_dev":
        call(mhla_amd.mhla_causal_step_dev, *tok, **epi)
    elif entry == "extend":
        call(mhla_amd.mhla_causal_extend, *tok, counts=COUNTS, **epi)
    else:
        _, draft = call(mhla_amd.mhla_causal_verify, *tok, counts=COUNTS, **epi)
        if entry == "commit":
            first = len(s.calls)
            assert call(mhla_amd.mhla_causal_commit, draft, t["mix"], state, ACCEPT) is state
    return s.calls[first:], t, state


NAMES = {"step": "mhla_causal_step_ragged", "step_dev": "mhla_causal_step_dev", "extend": "mhla_causal_extend_ragged",
         "verify": "mhla_causal_verify_ragged", "commit": "mhla_causal_commit_ragged"}


def _name(entry, Hk):
    return NAMES[entry] + ("_gqa" if Hk != H and entry != "commit" else "")


def _views(call):
    return [a for a in call.args if isinstance(a, tuple) and a[0] == "view"]


def _pointers(call):
    """base -> the byte offsets of the call's pointers into it, in argument order"""
    out = {}
    for a in call.args:
        if isinstance(a, tuple) and a[0] == "ptr":
            out.setdefault(a[1], []).append(a[2])
    return out


@pytest.mark.parametrize("Hk", [4, 2], ids=["Hkv=4", "Hkv=2"])
@pytest.mark.parametrize("entry", list(NAMES))
def test_a_sliced_batch_covers_every_sequence_once_and_in_order(entry, Hk, monkeypatch):
    monkeypatch.setattr(ops, "_MAX_GRID_BH", 2 * (Hk if entry == "commit" else H))   # (a commit launches over the k/v heads)
    with Session(ops, _lib) as s:
        calls, t, state = _run(entry, Hk, s)
    assert [c.name for c in calls] == [_name(entry, Hk)] * 2 and [batch_of(c) for c in calls] == [2, 1]
    first = 0
    for c in calls:
        views = _views(c)
        assert len(views) == (2 if entry == "commit" else 5)       # k, v; with q, the rows and the gate for the others
        for _, base, offset, sb, sn, sh in views:
            assert offset == first * sb, f"{c.name}: the view of {base} starts at element {offset}, sequence {first} is at {first * sb}"
        ptr = _pointers(c)
        assert ptr["mix"] == [0] and ptr["pos"] == [4 * first]
        for part in ("S", "P", "Cur"):
            assert ptr[part] == [4 * first * getattr(state, part).stride(0)]
        if entry == "step_dev":
            assert ptr["full"] == [4 * first]
        # the counts (and, for the commit, the accepted counts in the second row of the same [2, B] tensor) of these sequences
        fresh = [v for n, vs in ptr.items() if n.startswith("new") for v in vs]
        assert fresh == {"extend": [4 * first], "verify": [4 * first], "commit": [4 * first, 4 * (B + first)]}.get(entry, [])
        first += batch_of(c)
    assert first == B
    assert state.lengths == {"step": (7, 134, 128), "extend": (9, 135, 132), "commit": (7, 135, 130)}.get(entry, LENGTHS)
    assert state.stale == (entry == "step_dev")


@pytest.mark.parametrize("Hk", [4, 2], ids=["Hkv=4", "Hkv=2"])
@pytest.mark.parametrize("entry", list(NAMES))
def test_a_batch_within_the_limit_is_one_call_on_the_callers_tensors(entry, Hk):
    assert ops._MAX_GRID_BH == 65535
    with Session(ops, _lib) as s:
        calls, t, state = _run(entry, Hk, s)
    assert [c.name for c in calls] == [_name(entry, Hk)] and batch_of(calls[0]) == B
    views = {base: (offset, sb, sn, sh) for _, base, offset, sb, sn, sh in _views(calls[0])}
    for name in ("k", "v") if entry == "commit" else ("q", "k", "v", "gate"):
        assert views[name] == (0, *t[name].stride()[:3]), f"{name} is not passed as the caller's tensor"
    assert len(views) == (2 if entry == "commit" else 5)
    assert all(offset == 0 for offset, *_ in views.values())
    ptr = _pointers(calls[0])
    assert all(ptr[n] == [0] for n in ("mix", "S", "P", "Cur", "pos") + (("full",) if entry == "step_dev" else ()))
