"""Views of a state pool (`CausalState.at`), host side, no GPU: what is refused -- all of it before the library is loaded --, the
host mirror of a view, `reset` / `fork` on CPU tensors, the six mhla_causal_*_slots names in header, library and binding, and the
library calls a view makes (recorded by tools/fake_decode_lib.py on CPU tensors): the slotted namesake, the pool's tensors whole,
the slot map sliced with the tokens."""
import os
import re
import sys

import pytest
import torch

import mhla_amd
from mhla_amd import CausalState, CausalStateView, _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fake_decode_lib import Session, batch_of  # noqa: E402

N_SLOTS, H, K, V, CAP = 5, 2, 8, 12, 4
NAMES = ("mhla_causal_step_slots", "mhla_causal_step_dev_slots", "mhla_causal_extend_slots", "mhla_causal_verify_slots",
         "mhla_causal_commit_slots", "mhla_causal_varlen_state_init_slots")


def new_pool(lengths=(5, 0, 0, 63, 130)):
    e = CausalState.empty(N_SLOTS, H, K, V, CAP, device="cpu")
    return CausalState(e.S, e.P, e.Cur, 0, 64, lengths=lengths)


def toks(B, T=1):
    g = torch.Generator().manual_seed(5)
    return torch.randn(B, T, H, K, generator=g), torch.randn(B, T, H, K, generator=g), torch.randn(B, T, H, V, generator=g), torch.rand(CAP, CAP, generator=g)


@pytest.fixture
def no_library(monkeypatch):
    """Whatever the test raises, it raises before the library is asked for."""
    def load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", load)


@pytest.mark.parametrize("slots, what", [([3, 3, 0], r"\[3\] are given more than once"), ([0, -1], r"\[-1\] are outside 0 \.\. 4"),
                                         ([5, 1, 7], r"\[5, 7\] are outside 0 \.\. 4"), ([0, 1.0], r"must be ints, got \[1\.0\]"),
                                         ([True], r"must be ints"), (["2"], r"must be ints"), ([], "no slot given")])
def test_bad_slots_are_refused_by_name(slots, what, no_library):
    pool = new_pool()
    with pytest.raises(ValueError, match=what):
        pool.at(slots)
    with pytest.raises(ValueError, match=what):
        pool.reset(slots)


def test_a_view_of_a_uniform_pool_is_refused(no_library):
    uniform = CausalState.empty(N_SLOTS, H, K, V, CAP, device="cpu")
    with pytest.raises(ValueError, match=r"uniform.*to_ragged\(\)"):
        uniform.at([0, 1])
    with pytest.raises(ValueError, match=r"uniform.*to_ragged\(\)"):
        uniform.reset([0])
    view = uniform.to_ragged().at([1, 0])
    assert isinstance(view, CausalStateView) and view.S is uniform.S and view.lengths == (0, 0)
    with pytest.raises(ValueError, match="view of a view"):
        view.at([0])
    for bad in (torch.tensor([0, 1]), torch.tensor([[0]], dtype=torch.int32), torch.zeros(0, dtype=torch.int32)):
        with pytest.raises(ValueError, match="contiguous int32"):
            uniform.to_ragged().at(bad)


def test_a_device_map_is_for_step_dev_alone(no_library):
    pool = new_pool()
    view = pool.at(torch.tensor([3, -1, 4], dtype=torch.int32))
    assert view.lengths is None and view.rows == 3 and view.slots is None
    q, k, v, mix = toks(3)
    for fn, kw in ((mhla_amd.mhla_causal_step, {}), (mhla_amd.mhla_causal_extend, {}), (mhla_amd.mhla_causal_extend, dict(counts=[1, 1, 1])),
                   (mhla_amd.mhla_causal_verify, {})):
        with pytest.raises(ValueError, match="only mhla_causal_step_dev takes"):
            fn(q, k, v, mix, view, **kw)
    draft = ops.CausalDraft(k, v, (1, 1, 1), False, (63, 5, 130))
    with pytest.raises(ValueError, match="only mhla_causal_step_dev takes"):
        mhla_amd.mhla_causal_commit(draft, mix, view, (1, 1, 1))
    with pytest.raises(ValueError, match="only mhla_causal_step_dev takes"):
        view.compact()
    with pytest.raises(ValueError, match="only mhla_causal_step_dev takes"):
        mhla_amd.mhla_causal_state(k[:1], v[:1], mix, cu_seqlens=[0, 1], into=pool.at(torch.tensor([1], dtype=torch.int32)))


def test_a_stale_pool_is_refused_through_its_views(no_library):
    pool = new_pool()
    view = pool.at([3, 0, 4])
    pool.stale = True
    assert view.stale
    q, k, v, mix = toks(3)
    for fn in (mhla_amd.mhla_causal_step, mhla_amd.mhla_causal_extend, mhla_amd.mhla_causal_verify):
        with pytest.raises(ValueError, match=r"stale: call state\.sync\(\)"):
            fn(q, k, v, mix, view)
    for call in (lambda: pool.reset([0]), lambda: pool.fork(0, 1), view.compact,
                 lambda: mhla_amd.mhla_causal_state(k[:1], v[:1], mix, cu_seqlens=[0, 1, 1, 1], into=view)):
        with pytest.raises(ValueError, match="stale"):
            call()


def test_into_checks_the_pack_against_the_view(no_library):
    pool = new_pool()
    _, k, v, mix = toks(1, 70)
    with pytest.raises(ValueError, match="holds 2 sequences, the view selects 3 slots"):
        mhla_amd.mhla_causal_state(k, v, mix, cu_seqlens=[0, 64, 70], into=pool.at([3, 0, 4]))
    with pytest.raises(ValueError, match="capacity_chunks=4 given together with into"):
        mhla_amd.mhla_causal_state(k, v, mix, cu_seqlens=[0, 64, 70], into=pool.at([4, 1]), capacity_chunks=4)
    with pytest.raises(ValueError, match="capacity_chunks=2 given together with into"):
        mhla_amd.mhla_causal_prefill(k, k, v, mix, cu_seqlens=[0, 64, 70], into=pool.at([4, 1]), capacity_chunks=2)
    with pytest.raises(ValueError, match="into= takes a pack"):
        mhla_amd.mhla_causal_state(k, v, mix, into=pool.at([4]))
    with pytest.raises(TypeError, match="into must be a CausalStateView"):
        mhla_amd.mhla_causal_state(k, v, mix, cu_seqlens=[0, 64, 70], into=pool)
    other = CausalState.empty(N_SLOTS, H, K, V + 4, CAP, device="cpu").to_ragged()
    with pytest.raises(ValueError, match="into is CausalStateView"):
        mhla_amd.mhla_causal_state(k, v, mix, cu_seqlens=[0, 64, 70], into=other.at([4, 1]))
    assert pool.lengths == (5, 0, 0, 63, 130)


def test_a_views_lengths_mirror_the_pools(no_library):
    pool = new_pool()
    view = pool.at([3, 0, 4])
    assert view.lengths == (63, 5, 130) and view.seen == 130 and view.rows == 3 and view.capacity_chunks == CAP
    assert view.S is pool.S and view.P is pool.P and view.Cur is pool.Cur and view.pos is pool.pos and view.full is pool.full
    view.lengths = (64, 6, 130)            # (what a call leaves)
    assert pool.lengths == (6, 0, 0, 64, 130) and pool.seen == 130
    assert pool.at([0]).seen == 6
    c = view.compact()
    assert type(c) is CausalState and c.lengths == (64, 6, 130) and c.S.shape[0] == 3 and c.S.data_ptr() != pool.S.data_ptr()


def test_reset_and_fork_keep_the_mirror_consistent(no_library):
    pool = new_pool()
    g = torch.Generator().manual_seed(1)
    for t in (pool.S, pool.P, pool.Cur):
        t.copy_(torch.randn(t.shape, generator=g))
    pool.full[4] = 1
    keep = pool.clone()
    assert pool.fork(4, 1) is pool
    assert pool.lengths == (5, 130, 0, 63, 130) and pool.pos.tolist() == [5, 130, 0, 63, 130] and pool.full.tolist() == [0, 1, 0, 0, 1]
    assert torch.equal(pool.S[1, :, :2], keep.S[4, :, :2]) and torch.equal(pool.S[1, :, 2:], keep.S[1, :, 2:]), "the finished chunks, no more"
    assert torch.equal(pool.P[1], keep.P[4]) and torch.equal(pool.Cur[1], keep.Cur[4])
    for s in (0, 2, 3, 4):
        assert all(torch.equal(getattr(pool, n)[s], getattr(keep, n)[s]) for n in ("S", "P", "Cur", "pos", "full"))
    assert pool.reset([4, 0]) is pool
    assert pool.lengths == (0, 130, 0, 63, 0) and pool.seen == 130 and pool.pos.tolist() == [0, 130, 0, 63, 0] and pool.full.tolist() == [0, 1, 0, 0, 0]
    for s in (0, 4):
        assert float(pool.P[s].abs().max()) == float(pool.Cur[s].abs().max()) == 0.0
        assert torch.equal(pool.S[s], keep.S[s]), "S needs no clearing"
    assert torch.equal(pool.P[3], keep.P[3]) and torch.equal(pool.Cur[1], keep.Cur[4])
    with pytest.raises(ValueError, match=r"\[2\] are given more than once"):
        pool.fork(2, 2)
    with pytest.raises(ValueError, match="on the pool"):
        pool.at([1]).reset([0])


def test_the_six_entry_points_are_declared_exported_and_bound():
    from mhla_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mhla_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared in include/mhla_hip.h"
        assert name in _lib.SIGNATURES and callable(getattr(lib, name))
    # a map (pointer, count) after the positions, and Hkv after H where the namesake takes q
    extra = {"mhla_causal_step_slots": ("mhla_causal_step_ragged", 3), "mhla_causal_step_dev_slots": ("mhla_causal_step_dev", 3),
             "mhla_causal_extend_slots": ("mhla_causal_extend_ragged", 3), "mhla_causal_verify_slots": ("mhla_causal_verify_ragged", 3),
             "mhla_causal_commit_slots": ("mhla_causal_commit_ragged", 2), "mhla_causal_varlen_state_init_slots": ("mhla_causal_varlen_state_init", 2)}
    for name, (old, more) in extra.items():
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[old][1]) + more
    assert lib.mhla_abi_version() == _lib.ABI_VERSION == 9
    # the host checks of the map come first and need no device
    null = _lib.NULL_VIEW
    assert lib.mhla_causal_commit_slots(null, null, None, 0, None, 0, None, None, None, None, 5, None, None, 1, 0, 0, 0, 0, None, 0, 1, 1, 4, 4, 64,
                                        0, None) != 0
    assert b"slot_dev null" in lib.mhla_last_error()


ENTRIES = {"step": "mhla_causal_step_slots", "step_dev": "mhla_causal_step_dev_slots", "extend": "mhla_causal_extend_slots",
           "verify": "mhla_causal_verify_slots", "commit": "mhla_causal_commit_slots"}


def _run(entry, s, device_map=False):
    """One public call of `entry` on the view [3, 0, 4] of a CPU pool; returns (its library calls, the pool, the view)."""
    from mhla_amd import build
    build.build(verbose=False)
    pool = new_pool()
    view = pool.at(torch.tensor([3, 0, 4], dtype=torch.int32) if device_map else [3, 0, 4])
    q, k, v, mix = toks(3, 1 if "step" in entry else 5)
    s.name(q=q, k=k, v=v, mix=mix, S=pool.S, P=pool.P, Cur=pool.Cur, pos=pool.pos, full=pool.full, map=view.map)
    first = len(s.calls)
    call = lambda fn, *a, **kw: s.call(entry, fn, *a, catch=False, **kw)
    if entry == "step":
        call(mhla_amd.mhla_causal_step, q, k, v, mix, view)
    elif entry == "step_dev":
        call(mhla_amd.mhla_causal_step_dev, q, k, v, mix, view)
    elif entry == "extend":
        call(mhla_amd.mhla_causal_extend, q, k, v, mix, view, counts=(3, 2, 1))
    else:
        _, draft = call(mhla_amd.mhla_causal_verify, q, k, v, mix, view, counts=(3, 2, 1))
        assert draft.view is view
        if entry == "commit":
            first = len(s.calls)
            with pytest.raises(ValueError, match="pass the view"):
                mhla_amd.mhla_causal_commit(draft, mix, pool, (1, 2, 1))
            with pytest.raises(ValueError, match="pass the view"):
                mhla_amd.mhla_causal_commit(draft, mix, pool.at([3, 0, 1]), (1, 2, 1))
            assert call(mhla_amd.mhla_causal_commit, draft, mix, view, (1, 2, 1)) is view
    return s.calls[first:], pool, view


def _pointers(call):
    out = {}
    for a in call.args:
        if isinstance(a, tuple) and a[0] == "ptr":
            out.setdefault(a[1], []).append(a[2])
    return out


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_a_view_makes_the_slotted_call_on_the_pools_tensors(entry):
    with Session(ops, _lib) as s:
        calls, pool, view = _run(entry, s, device_map=entry == "step_dev")
    assert [c.name for c in calls] == [ENTRIES[entry]] and batch_of(calls[0]) == 3
    ptr = _pointers(calls[0])
    assert all(ptr[n] == [0] for n in ("mix", "S", "P", "Cur", "pos", "map") + (("full",) if entry == "step_dev" else ()))
    args = calls[0].args
    i = args.index(("ptr", "map", 0))
    assert args[i - 1] == ("ptr", "pos", 0) and args[i + 1] == N_SLOTS, "the map and the pool's size follow the positions"
    assert pool.lengths == {"step": (6, 0, 0, 64, 131), "extend": (7, 0, 0, 66, 131), "commit": (7, 0, 0, 64, 131)}.get(entry, (5, 0, 0, 63, 130))
    assert pool.stale == (entry == "step_dev")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_a_sliced_view_slices_its_map_and_not_the_pool(entry, monkeypatch):
    monkeypatch.setattr(ops, "_MAX_GRID_BH", 2 * H)
    with Session(ops, _lib) as s:
        calls, pool, view = _run(entry, s)
    assert [c.name for c in calls] == [ENTRIES[entry]] * 2 and [batch_of(c) for c in calls] == [2, 1]
    for c, first in zip(calls, (0, 2)):
        ptr = _pointers(c)
        assert ptr["map"] == [4 * first], "rows [first, ...) of the map"
        assert all(ptr[n] == [0] for n in ("S", "P", "Cur", "pos") + (("full",) if entry == "step_dev" else ())), "the pool passes whole"
        for a in c.args:
            if isinstance(a, tuple) and a[0] == "view":
                assert a[2] == first * a[3], f"{c.name}: the view of {a[1]} does not start at row {first}"


def test_a_pack_prefill_into_a_view_is_one_slotted_call():
    from mhla_amd import build
    build.build(verbose=False)
    pool = new_pool()
    view = pool.at([4, 1])
    _, k, v, mix = toks(1, 70)
    with Session(ops, _lib) as s:
        s.name(k=k, v=v, mix=mix, S=pool.S, P=pool.P, Cur=pool.Cur, pos=pool.pos, map=view.map)
        assert s.call("prefill", mhla_amd.mhla_causal_state, k, v, mix, cu_seqlens=[0, 64, 70], into=view, catch=False) is view
    assert [c.name for c in s.calls] == ["mhla_causal_varlen_state_init_slots"]
    args = s.calls[0].args
    i = args.index(("ptr", "map", 0))
    assert args[i - 2] == 2 and args[i - 1][0] == "ptr" and args[i - 1][1].startswith("new") and args[i + 1] == N_SLOTS, \
        "n_seqs, the pack's own lengths (not the pool's positions), the map, the pool's size"
    assert pool.lengths == (5, 6, 0, 63, 64) and pool.pos.tolist() == [5, 6, 0, 63, 64] and view.lengths == (64, 6)
