"""The decode section of `mhla_amd/ops.py` (CausalState ... mhla_causal_commit) run on CPU tensors against a recording stand-in for
the library (tools/fake_decode_lib.py): every library call with every argument, every public call's effect on the state's host
mirror, every exception's type and message, and the signature and docstring hash of every public name of the section.  Two trees
whose logs are byte-identical make the same calls in the same order and refuse the same things with the same words: the check
of a refactor of that section (profiles/decode_host_refactor.md).

    python tools/record_decode_calls.py [--tree DIR] [-o LOG]     the log (sha256 on stderr); DIR: another checkout to import
    python tools/record_decode_calls.py --raises                  also list the `raise` lines of the section no scenario reached
    python tools/record_decode_calls.py --counts                  Python function calls per public call (cProfile), no log
"""
import argparse
import cProfile
import hashlib
import inspect
import itertools
import os
import pstats
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.join(HERE, ".."))
ap.add_argument("-o", "--output")
ap.add_argument("--raises", action="store_true")
ap.add_argument("--counts", action="store_true")
opt = ap.parse_args()
sys.path.insert(0, os.path.abspath(opt.tree))

import torch  # noqa: E402

import mhla_amd  # noqa: E402
from mhla_amd import CausalState, _lib, ops  # noqa: E402
from mhla_amd import build as _build  # noqa: E402
from fake_decode_lib import Session  # noqa: E402

_build.build(verbose=False)
B, K, V, CAP = 3, 16, 24, 5
PUBLIC = ("CausalState", "CausalState.empty", "CausalState.to_ragged", "CausalState.sync", "CausalState.clone", "CausalState.cat",
          "mhla_causal_prefill", "mhla_causal_state", "mhla_causal_step", "mhla_causal_step_dev", "mhla_causal_extend", "CausalDraft",
          "mhla_causal_verify", "mhla_causal_commit")


def rand(*shape, dtype=torch.float32, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def tokens(dtype, H, Hk, T, k_dim=K):
    return (rand(B, T, H, k_dim, dtype=dtype, seed=1), rand(B, T, Hk, k_dim, dtype=dtype, seed=2), rand(B, T, Hk, V, dtype=dtype, seed=3),
            rand(B, T, H, V, dtype=dtype, seed=4))


def new_state(Hk, lengths=None, seen=0, k_dim=K, batch=B):
    e = CausalState.empty(batch, Hk, k_dim, V, CAP, device="cpu")
    if lengths is None:
        e.seen = seen
        return e
    return CausalState(e.S, e.P, e.Cur, 0, 64, lengths=lengths)


def name_all(s, state=None, **tensors):
    s.name(**tensors)
    if state is not None:
        s.name(S=state.S, P=state.P, Cur=state.Cur, pos=state.pos, full=state._full)


def scenarios(s, tag, dtype, H, Hk):
    """Every scenario of one (heads, dtype, grid limit) configuration; every call on a fresh state."""
    mix, w = torch.rand(CAP, CAP, generator=torch.Generator().manual_seed(9)), torch.rand(V, generator=torch.Generator().manual_seed(8)) + 0.5
    ws64 = _lib.load().mhla_causal_extend_ragged_gqa_ws_bytes(B, 64, H, Hk, K, V, 1, 0)

    def run(label, fn, q, k, v, state, *, names=None, **kw):
        name_all(s, state, mix=mix, w=w, **(names or dict(q=q, k=k, v=v)), gate=kw.get("gate"))
        return s.call(f"{tag} {label}", fn, q, k, v, mix, state, state=state, **kw)

    # ---- mhla_causal_state
    _, k70, v70, _ = tokens(dtype, H, Hk, 70)
    for label, kw in (("uniform", {}), ("lengths", dict(lengths=(6, 70, 33))), ("lengths left-padded", dict(lengths=[6, 70, 33], left_padded=True)),
                      ("lengths tensor with zero", dict(lengths=torch.tensor([0, 70, 70]))), ("capacity 3", dict(capacity_chunks=3))):
        s.name(k=k70, v=v70, mix=mix)
        s.call(f"{tag} state {label}", lambda **kw: _named_state(s, mhla_amd.mhla_causal_state(k70, v70, mix, **kw)), **kw)
    s.call(f"{tag} state T=0", mhla_amd.mhla_causal_state, k70[:, :0], v70[:, :0], mix)
    kp, vp = rand(1, 109, Hk, K, dtype=dtype, seed=5), rand(1, 109, Hk, V, dtype=dtype, seed=6)
    s.name(k=kp, v=vp, mix=mix)
    s.call(f"{tag} state cu_seqlens", lambda: _named_state(s, mhla_amd.mhla_causal_state(kp, vp, mix, cu_seqlens=[0, 6, 76, 76, 109])))

    # ---- mhla_causal_step
    q, k, v, g = tokens(dtype, H, Hk, 1)
    for pos in (5, 63):
        run(f"step uniform at {pos}", mhla_amd.mhla_causal_step, q, k, v, new_state(Hk, seen=pos))
    run("step ragged", mhla_amd.mhla_causal_step, q, k, v, new_state(Hk, (6, 133, 127)))
    packed = rand(B, 1, H * K + Hk * K + Hk * V, dtype=dtype, seed=7)
    qs, ks, vs = (t.unflatten(2, (h, -1)) for t, h in zip(packed.split((H * K, Hk * K, Hk * V), dim=2), (H, Hk, Hk)))
    for lengths in (None, (6, 133, 127)):
        run(f"step strided views lengths={lengths}", mhla_amd.mhla_causal_step, qs, ks, vs, new_state(Hk, lengths, seen=5), names=dict(qkv=packed))
    wide = rand(B, 1, H, K + 1, dtype=dtype, seed=10)
    for lengths in (None, (6, 133, 127)):
        run(f"step copied view lengths={lengths}", mhla_amd.mhla_causal_step, wide[..., :K], k, v, new_state(Hk, lengths, seen=5), names=dict(qwide=wide, k=k, v=v))
    for gate, nw, epi in itertools.product((None, g), (None, w), (None, True, False)):
        for lengths in (None, (6, 133, 127)):
            run(f"step gate={gate is not None} norm_weight={nw is not None} epilogue={epi} lengths={lengths}", mhla_amd.mhla_causal_step, q, k, v,
                new_state(Hk, lengths, seen=5), gate=gate, norm_weight=nw, epilogue=epi, norm_eps=1e-6, scale=0.5)
    run("step bf16 norm weight", mhla_amd.mhla_causal_step, q, k, v, new_state(Hk, (6, 133, 127)), norm_weight=w.to(torch.bfloat16))

    # ---- mhla_causal_step_dev
    ang = torch.outer(torch.arange(64 * CAP, dtype=torch.float32), 1.0 / (10000 ** (torch.arange(0, K, 2, dtype=torch.float32) / K)))
    rot = (torch.cos(ang).to(dtype), torch.sin(ang).to(dtype))
    both = torch.stack((torch.cos(ang), torch.sin(ang)), dim=2).to(dtype)   # (interleaved tables: made contiguous by the call)
    for label, kw in (("bare", {}), ("feature_map", dict(feature_map="relu")), ("rotary", dict(rotary=rot)),
                      ("feature_map and rotary", dict(feature_map="elu", rotary=rot, gate=g, norm_weight=w)),
                      ("rotary interleaved", dict(rotary=(both[..., 0], both[..., 1])))):
        st = new_state(Hk, (6, 133, 127))
        st.full
        s.name(cos=rot[0], sin=rot[1], both=both)
        run(f"step_dev {label}", mhla_amd.mhla_causal_step_dev, q, k, v, st, **kw)
    run("step after step_dev (stale)", mhla_amd.mhla_causal_step, q, k, v, st)
    s.call(f"{tag} sync", st.sync, state=st)

    # ---- mhla_causal_extend
    for T in (1, 2, 70):
        qT, kT, vT, gT = tokens(dtype, H, Hk, T)
        run(f"extend T={T} uniform", mhla_amd.mhla_causal_extend, qT, kT, vT, new_state(Hk, seen=5))
        run(f"extend T={T} ragged equal", mhla_amd.mhla_causal_extend, qT, kT, vT, new_state(Hk, (6, 6, 6)), gate=gT)
        run(f"extend T={T} ragged equal pairs", mhla_amd.mhla_causal_extend, qT, kT, vT, new_state(Hk, (6, 6, 70)))
        run(f"extend T={T} ragged unequal", mhla_amd.mhla_causal_extend, qT, kT, vT, new_state(Hk, (6, 133, 127)), norm_weight=w)
    for counts, left in (((3, 0, 70), False), ((3, 0, 70), True), (torch.tensor([0, 0, 0]), False), ((0, 0, 64), True)):
        run(f"extend counts={counts} left_padded={left}", mhla_amd.mhla_causal_extend, qT, kT, vT, new_state(Hk, (6, 133, 127)), counts=counts,
            left_padded=left, gate=gT)
    q2, k2, v2, g2 = tokens(dtype, H, Hk, 200)
    for cap, what in ((1, "cap 1"), (ws64, "cap of a 64-token window")):
        saved, ops.EXTEND_WS_CAP_BYTES = ops.EXTEND_WS_CAP_BYTES, cap
        try:
            run(f"extend T=200 uniform, {what}", mhla_amd.mhla_causal_extend, q2, k2, v2, new_state(Hk, seen=5), gate=g2)
            run(f"extend T=200 ragged equal pairs, {what}", mhla_amd.mhla_causal_extend, q2, k2, v2, new_state(Hk, (6, 6, 70)))
            run(f"extend T=70 ragged unequal, {what}", mhla_amd.mhla_causal_extend, qT, kT, vT, new_state(Hk, (6, 133, 127)), gate=gT)
            for left in (False, True):
                run(f"extend counts left_padded={left}, {what}", mhla_amd.mhla_causal_extend, qT, kT, vT, new_state(Hk, (6, 133, 127)),
                    counts=(3, 0, 70), left_padded=left, gate=gT, norm_weight=w)
                run(f"extend T=200 counts left_padded={left}, {what}", mhla_amd.mhla_causal_extend, q2, k2, v2, new_state(Hk, (6, 100, 0)),
                    counts=(3, 0, 200), left_padded=left)
            run(f"verify, {what}", mhla_amd.mhla_causal_verify, qT, kT, vT, new_state(Hk, (6, 133, 127)))
        finally:
            ops.EXTEND_WS_CAP_BYTES = saved

    # ---- mhla_causal_verify, mhla_causal_commit
    q5, k5, v5, g5 = tokens(dtype, H, Hk, 5)
    for counts, left, accepts in (((3, 0, 5), False, ((2, 0, 0), (0, 0, 0), (3, 0, 5))), ((3, 0, 5), True, ((0, 0, 5), torch.tensor([3, 0, 1]))),
                                  (None, False, ((5, 5, 5),)), ((0, 0, 0), False, ((0, 0, 0),))):
        for accept in accepts:
            st = new_state(Hk, (60, 133, 127))
            got = run(f"verify counts={counts} left_padded={left}", mhla_amd.mhla_causal_verify, q5, k5, v5, st, counts=counts, left_padded=left,
                      gate=g5, norm_weight=w)
            s.call(f"{tag} commit accept={accept}", mhla_amd.mhla_causal_commit, got[1], mix, st, accept, state=st)
    st = new_state(Hk, (60, 133, 127))
    got = run("verify copied view", mhla_amd.mhla_causal_verify, rand(B, 5, H, K + 1, dtype=dtype, seed=11)[..., :K], rand(B, 5, Hk, K + 1, dtype=dtype, seed=12)[..., :K],
              v5, st, names=dict(v=v5))
    s.name(draft_k=got[1].k)
    s.call(f"{tag} commit of the copies",mhla_amd.mhla_causal_commit, got[1], mix, st, (1, 2, 3), state=st)


def _named_state(s, state):
    s.name(S=state.S, P=state.P, Cur=state.Cur, pos=state.pos)
    return state


def refusals(s):
    """Every `raise` of the section, once at least (H = 4, Hkv = 2, fp32 unless the refusal is about something else)."""
    H, Hk = 4, 2
    mix, w = torch.rand(CAP, CAP), torch.rand(V)
    meta = torch.device("meta")
    q, k, v, g = tokens(torch.float32, H, Hk, 1)
    q5, k5, v5, g5 = tokens(torch.float32, H, Hk, 5)
    rag = lambda *a, **kw: new_state(Hk, (6, 133, 127), *a, **kw)
    call = lambda label, fn, *a, **kw: s.call(f"refusal: {label}", fn, *a, **kw)
    e = CausalState.empty(B, Hk, K, V, CAP, device="cpu")
    # CausalState
    call("pos dtype", CausalState, e.S, e.P, e.Cur, lengths=(1, 2, 3), pos=torch.zeros(3))
    call("pos shape", CausalState, e.S, e.P, e.Cur, lengths=(1, 2, 3), pos=torch.zeros(2, dtype=torch.int32))
    call("pos without lengths", CausalState, e.S, e.P, e.Cur, pos=torch.zeros(3, dtype=torch.int32))
    call("lengths count", CausalState, e.S, e.P, e.Cur, lengths=(1, 2))
    call("lengths negative", CausalState, e.S, e.P, e.Cur, lengths=torch.tensor([1, -2, 3]))
    call("empty size", CausalState.empty, B, 0, K, V, CAP, "cpu")
    st = rag()
    st._full = torch.tensor([0, 1, 1], dtype=torch.int32)
    call("sync over capacity", st.sync, state=st)
    call("cat of nothing", CausalState.cat, [])
    call("cat of another thing", CausalState.cat, [e, 3])
    call("cat of differing states", CausalState.cat, [e, CausalState.empty(B, Hk, K, V, CAP + 1, device="cpu")])
    st = rag()
    st.stale = True
    call("cat of a stale state", CausalState.cat, [e, st])
    for fn, T in ((mhla_amd.mhla_causal_step, 1), (mhla_amd.mhla_causal_extend, 5), (mhla_amd.mhla_causal_verify, 5)):
        call(f"stale state, {fn.__name__}", fn, *tokens(torch.float32, H, Hk, T)[:3], mix, st, state=st)
    call("stale state, commit", mhla_amd.mhla_causal_commit, ops.CausalDraft(k5, v5, (5, 5, 5), False, st.lengths), mix, st, (1, 1, 1), state=st)
    # prefill, state
    call("prefill rank", mhla_amd.mhla_causal_prefill, q[0], k, v, mix)
    call("prefill chunk size", mhla_amd.mhla_causal_prefill, q, k, v, mix, 32)
    call("prefill lengths", mhla_amd.mhla_causal_prefill, q5, k5, v5, mix, lengths=(1, 2, 9))
    k70, v70 = tokens(torch.float32, H, Hk, 70)[1:3]
    kp, vp = k70[:1], v70[:1]
    call("pack rank", mhla_amd.mhla_causal_state, kp[0], vp, mix, cu_seqlens=[0, 70])
    call("pack with lengths", mhla_amd.mhla_causal_state, kp, vp, mix, cu_seqlens=[0, 70], lengths=(70,))
    call("pack left-padded", mhla_amd.mhla_causal_state, kp, vp, mix, cu_seqlens=[0, 70], left_padded=True)
    call("pack v shape", mhla_amd.mhla_causal_state, kp, vp[:, :5], mix, cu_seqlens=[0, 70])
    call("pack capacity 0", mhla_amd.mhla_causal_state, kp, vp, mix, cu_seqlens=[0, 70], capacity_chunks=0)
    call("pack of no sequence", mhla_amd.mhla_causal_state, kp[:, :0], vp[:, :0], mix, cu_seqlens=[0])
    saved, ops._MAX_GRID_BH = ops._MAX_GRID_BH, Hk
    call("pack beyond the grid", mhla_amd.mhla_causal_state, kp, vp, mix, cu_seqlens=[0, 6, 70])
    ops._MAX_GRID_BH = saved
    call("pack beyond the capacity", mhla_amd.mhla_causal_state, kp, vp, mix, cu_seqlens=[0, 1, 70], capacity_chunks=1)
    call("pack narrow matrix", mhla_amd.mhla_causal_state, kp, vp, torch.rand(CAP, 1), cu_seqlens=[0, 6, 70])
    call("pack matrix elsewhere", mhla_amd.mhla_causal_state, kp, vp, torch.rand(CAP, CAP, device=meta), cu_seqlens=[0, 6, 70])
    call("state rank", mhla_amd.mhla_causal_state, k70[0], v70, mix)
    call("state v shape", mhla_amd.mhla_causal_state, k70, v70[:, :5], mix)
    call("state v dtype", mhla_amd.mhla_causal_state, k70, v70.double(), mix)
    call("state lengths count", mhla_amd.mhla_causal_state, k70, v70, mix, lengths=(1, 2))
    call("state lengths beyond T", mhla_amd.mhla_causal_state, k70, v70, mix, lengths=(1, 2, 71))
    call("state capacity 6", mhla_amd.mhla_causal_state, k70, v70, mix, capacity_chunks=6)
    call("state beyond the capacity", mhla_amd.mhla_causal_state, k70, v70, mix, capacity_chunks=1)
    call("state narrow matrix", mhla_amd.mhla_causal_state, k70, v70, torch.rand(CAP, 1))
    call("state matrix elsewhere", mhla_amd.mhla_causal_state, k70, v70, torch.rand(CAP, CAP, device=meta))
    call("state dtype", mhla_amd.mhla_causal_state, k70.double(), v70.double(), mix)
    # the entry check, for each of the four
    for fn, T in ((mhla_amd.mhla_causal_step, 1), (mhla_amd.mhla_causal_step_dev, 1), (mhla_amd.mhla_causal_extend, 5), (mhla_amd.mhla_causal_verify, 5)):
        qT, kT, vT, _ = tokens(torch.float32, H, Hk, T)
        call(f"{fn.__name__} state type", fn, qT, kT, vT, mix, (1, 2))
        call(f"{fn.__name__} rank", fn, qT, kT[0], vT, mix, rag())
        call(f"{fn.__name__} T=2 or 0", fn, *tokens(torch.float32, H, Hk, 2 if T == 1 else 0)[:3], mix, rag())
    # _decode_prepare, through each of the four (the order of refusals is the order of these calls)
    for fn, T in ((mhla_amd.mhla_causal_step, 1), (mhla_amd.mhla_causal_step_dev, 1), (mhla_amd.mhla_causal_extend, 5), (mhla_amd.mhla_causal_verify, 5)):
        qT, kT, vT, gT = tokens(torch.float32, H, Hk, T)
        n = fn.__name__
        call(f"{n} heads", fn, qT, tokens(torch.float32, H, 3, T)[1], vT, mix, new_state(3, (6, 133, 127)))
        call(f"{n} too many heads per k/v head", fn, rand(B, T, 9, K), rand(B, T, 1, K), rand(B, T, 1, V), mix, new_state(1, (6, 133, 127)))
        call(f"{n} v shape", fn, qT, kT, rand(B, T, H, V), mix, rag())
        call(f"{n} gate shape", fn, qT, kT, vT, mix, rag(), gate=gT[:, :, :Hk])
        call(f"{n} k dtype", fn, qT, kT.to(torch.bfloat16), vT, mix, rag())
        call(f"{n} k elsewhere", fn, qT, kT.to(meta), vT, mix, rag())
        call(f"{n} dtype", fn, qT.double(), kT.double(), vT.double(), mix, rag())
        call(f"{n} state shape", fn, qT, kT, vT, mix, new_state(H, (6, 133, 127)))
        call(f"{n} uniform state shape", fn, qT, kT, vT, mix, new_state(H, seen=5))
        call(f"{n} matrix elsewhere", fn, qT, kT, vT, torch.rand(CAP, CAP, device=meta), rag())
        call(f"{n} norm weight elsewhere", fn, qT, kT, vT, mix, rag(), norm_weight=w.to(meta))
        st = rag()
        st.P = st.P.to(meta)
        call(f"{n} state.P elsewhere", fn, qT, kT, vT, mix, st)
        call(f"{n} norm weight size", fn, qT, kT, vT, mix, rag(), norm_weight=torch.rand(V + 1))
        call(f"{n} requires grad", fn, qT, kT.clone().requires_grad_(), vT, mix, rag())
        call(f"{n} matrix rank", fn, qT, kT, vT, torch.rand(CAP), rag())
        call(f"{n} matrix narrower than its rows", fn, qT, kT, vT, torch.rand(CAP, 2), rag())
        st = rag()
        st.chunk_size = 32
        call(f"{n} chunk size", fn, qT, kT, vT, mix, st)
        call(f"{n} matrix rows", fn, qT, kT, vT, torch.rand(2, 2), rag())
        call(f"{n} uniform matrix rows", fn, qT, kT, vT, torch.rand(2, 2), new_state(Hk, seen=130))
        call(f"{n} capacity", fn, qT, kT, vT, torch.rand(8, 8), new_state(Hk, (6, 133, 320)))
        call(f"{n} uniform capacity", fn, qT, kT, vT, torch.rand(8, 8), new_state(Hk, seen=320))
        call(f"{n} epilogue=False with a gate", fn, qT, kT, vT, mix, rag(), gate=gT, epilogue=False)
        z = torch.zeros(B, Hk, CAP, V, K).transpose(3, 4)
        call(f"{n} state contiguity", fn, qT, kT, vT, mix, CausalState(z, e.P, e.Cur, 0, 64, lengths=(6, 133, 127)))
        st = rag()
        st.pos = st.pos.to(torch.int64)
        call(f"{n} pos dtype", fn, qT, kT, vT, mix, st)
    # the step's own row test against _ragged_slices': lengths (63, 100) ask the step for row 2 and the plan for row 1
    two = torch.rand(2, 2)
    call("step closes a chunk beyond the matrix", mhla_amd.mhla_causal_step, q, k, v, two, new_state(Hk, (63, 100, 5)))
    call("extend counts of one on the same state", mhla_amd.mhla_causal_extend, q, k, v, two, new_state(Hk, (63, 100, 5)), counts=(1, 1, 1))
    call("extend counts beyond the matrix columns", mhla_amd.mhla_causal_extend, *tokens(torch.float32, H, Hk, 28)[:3], torch.rand(3, 2), new_state(Hk, (63, 100, 5)),
         counts=(1, 28, 0))
    # mhla_causal_step_dev
    dev = mhla_amd.mhla_causal_step_dev
    call("step_dev uniform state", dev, q, k, v, mix, new_state(Hk, seen=5))
    call("step_dev matrix below the capacity", dev, q, k, v, torch.rand(CAP - 1, CAP), rag())
    good = torch.zeros(64 * CAP, K // 2)
    for label, t in (("rows", good[:-1]), ("rank", good[0]), ("dtype", good.double()), ("elsewhere", good.to(meta)), ("columns", good[:, :-1])):
        call(f"step_dev rotary cos {label}", dev, q, k, v, mix, rag(), rotary=(t, good))
        call(f"step_dev rotary sin {label}", dev, q, k, v, mix, rag(), rotary=(good, t))
    q12, k12, v12, _ = tokens(torch.float32, H, Hk, 1, k_dim=12)
    call("step_dev K % 8 with a feature map", dev, q12, k12, v12, mix, new_state(Hk, (6, 133, 127), k_dim=12), feature_map="relu")
    call("step_dev K % 8 with rotary", dev, q12, k12, v12, mix, new_state(Hk, (6, 133, 127), k_dim=12), rotary=(torch.zeros(64 * CAP, 6), torch.zeros(64 * CAP, 6)))
    call("step_dev feature map", dev, q, k, v, mix, rag(), feature_map="gelu")
    capturing, torch.cuda.is_current_stream_capturing = torch.cuda.is_current_stream_capturing, lambda: True
    call("step_dev state.full under capture", dev, q, k, v, mix, rag())
    torch.cuda.is_current_stream_capturing = capturing
    # counts
    for fn in (mhla_amd.mhla_causal_extend, mhla_amd.mhla_causal_verify):
        n = fn.__name__
        call(f"{n} counts count", fn, q5, k5, v5, mix, rag(), counts=(1, 2))
        call(f"{n} counts beyond T", fn, q5, k5, v5, mix, rag(), counts=torch.tensor([1, 6, 0]))
        call(f"{n} counts negative", fn, q5, k5, v5, mix, rag(), counts=(1, -1, 0))
        call(f"{n} counts on a uniform state", fn, q5, k5, v5, mix, new_state(Hk, seen=5), counts=(1, 2, 3))
        call(f"{n} counts, state of another batch", fn, q5, k5, v5, mix, new_state(Hk, (6, 133), batch=2), counts=(1, 2, 3))
        call(f"{n} counts matrix rank", fn, q5, k5, v5, torch.rand(CAP), rag(), counts=(1, 2, 3))
        call(f"{n} counts matrix rows", fn, q5, k5, v5, torch.rand(2, 2), rag(), counts=(1, 2, 3))
        call(f"{n} counts capacity", fn, q5, k5, v5, torch.rand(8, 8), new_state(Hk, (6, 133, 318)), counts=(1, 0, 3))
    # commit
    commit = mhla_amd.mhla_causal_commit
    st = rag()
    draft = ops.CausalDraft(k5, v5, (3, 0, 5), False, st.lengths)
    call("commit draft type", commit, (k5, v5), mix, st, (1, 0, 1))
    call("commit state type", commit, draft, mix, None, (1, 0, 1))
    call("commit uniform state", commit, draft, mix, new_state(Hk, seen=5), (1, 0, 1))
    call("commit accept count", commit, draft, mix, st, (1, 0))
    call("commit accept beyond the counts", commit, draft, mix, st, (1, 1, 1))
    call("commit accept negative", commit, draft, mix, st, torch.tensor([1, 0, -1]))
    call("commit state moved", commit, draft, mix, new_state(Hk, (6, 133, 128)), (1, 0, 1))
    call("commit state shape", commit, draft, mix, new_state(H, (6, 133, 127)), (1, 0, 1))
    call("commit matrix rank", commit, draft, torch.rand(CAP), st, (1, 0, 1))
    call("commit matrix elsewhere", commit, draft, torch.rand(CAP, CAP, device=meta), st, (1, 0, 1))
    call("commit matrix columns", commit, ops.CausalDraft(k5, v5, (3, 0, 5), False, (6, 133, 127)), torch.rand(CAP, 2), st, (1, 0, 3))
    call("commit matrix rows", commit, ops.CausalDraft(k5, v5, (3, 0, 5), False, (6, 133, 127)), torch.rand(2, CAP), st, (1, 0, 3))
    call("commit dtype", commit, ops.CausalDraft(k5.double(), v5.double(), (3, 0, 5), False, (6, 133, 127)), mix, st, (1, 0, 3))


def record():
    lines = []
    for name in PUBLIC:
        obj = ops
        for part in name.split("."):
            obj = getattr(obj, part)
        doc = hashlib.sha256((obj.__doc__ or "").encode()).hexdigest()
        lines.append(f"{name}{inspect.signature(obj)} doc {doc}")
    with Session(ops, _lib) as s:
        for (H, Hk), dtype, limit in itertools.product(((4, 4), (4, 2)), (torch.float32, torch.bfloat16), (None, 2)):
            saved = ops._MAX_GRID_BH
            if limit:
                ops._MAX_GRID_BH = limit * H
            try:
                scenarios(s, f"[H={H} Hkv={Hk} {dtype} grid={'default' if limit is None else f'{limit}H'}]", dtype, H, Hk)
            finally:
                ops._MAX_GRID_BH = saved
        refusals(s)
    return lines + s.lines


def raise_lines():
    src = open(ops.__file__).read().split("\n")
    lo = next(i for i, ln in enumerate(src) if ln.startswith("class CausalState"))
    hi = next(i for i, ln in enumerate(src) if ln.startswith("# per-head RMSNorm x swish gate"))
    return {i + 1 for i in range(lo, hi) if src[i].lstrip().startswith("raise ")}, src


def count_calls():
    """Python function calls (cProfile, builtins included) of one public call, caches warm; the count does not depend on the machine."""
    H = 4
    mix = torch.rand(CAP, CAP)
    out = []
    with Session(ops, _lib) as s:
        def measure(label, fn, make_args):
            fn(*make_args()[0], **make_args()[1])   # (warm: the cached workspace sizes)
            args, kw = make_args()
            prof = cProfile.Profile()
            prof.enable()
            fn(*args, **kw)
            prof.disable()
            out.append(f"{label}: {pstats.Stats(prof).total_calls}")

        for Hk in (4, 2):
            q, k, v, g = tokens(torch.float32, H, Hk, 1)
            q5, k5, v5, g5 = tokens(torch.float32, H, Hk, 5)
            tag = f"Hkv={Hk}"
            measure(f"mhla_causal_step uniform {tag}", mhla_amd.mhla_causal_step, lambda: ((q, k, v, mix, new_state(Hk, seen=5)), {}))
            measure(f"mhla_causal_step ragged, one chain {tag}", mhla_amd.mhla_causal_step, lambda: ((q, k, v, mix, new_state(Hk, (6, 133, 127))), {}))

            def dev_args():
                st = new_state(Hk, (6, 133, 127))
                st.full
                return (q, k, v, mix, st), {}
            measure(f"mhla_causal_step_dev {tag}", mhla_amd.mhla_causal_step_dev, dev_args)
            measure(f"mhla_causal_step_dev gate, norm weight {tag}", mhla_amd.mhla_causal_step_dev,
                    lambda: (dev_args()[0], dict(gate=g, norm_weight=torch.ones(V))))
            measure(f"mhla_causal_extend T=5 uniform {tag}", mhla_amd.mhla_causal_extend, lambda: ((q5, k5, v5, mix, new_state(Hk, seen=5)), {}))
            measure(f"mhla_causal_extend T=5 ragged {tag}", mhla_amd.mhla_causal_extend, lambda: ((q5, k5, v5, mix, new_state(Hk, (6, 133, 127))), {}))
            measure(f"mhla_causal_extend counts {tag}", mhla_amd.mhla_causal_extend,
                    lambda: ((q5, k5, v5, mix, new_state(Hk, (6, 133, 127))), dict(counts=(3, 0, 5))))
            measure(f"mhla_causal_verify {tag}", mhla_amd.mhla_causal_verify, lambda: ((q5, k5, v5, mix, new_state(Hk, (6, 133, 127))), dict(counts=(3, 0, 5))))

            def commit_args():
                st = new_state(Hk, (6, 133, 127))
                return (ops.CausalDraft(k5, v5, (3, 0, 5), False, st.lengths), mix, st, (1, 0, 3)), {}
            measure(f"mhla_causal_commit {tag}", mhla_amd.mhla_causal_commit, commit_args)
    return out


if __name__ == "__main__":
    if opt.counts:
        print("\n".join(count_calls()))
        sys.exit(0)
    seen = set()
    if opt.raises:
        path = ops.__file__

        def tracer(frame, event, arg):
            if frame.f_code.co_filename != path:
                return None
            if event == "line":
                seen.add(frame.f_lineno)
            return tracer
        sys.settrace(tracer)
    log = "\n".join(record()) + "\n"
    sys.settrace(None)
    if opt.output:
        open(opt.output, "w").write(log)
    else:
        sys.stdout.write(log)
    print(f"sha256 {hashlib.sha256(log.encode()).hexdigest()}  {log.count(chr(10))} lines", file=sys.stderr)
    if opt.raises:
        want, src = raise_lines()
        for n in sorted(want - seen):
            print(f"never raised: {n}: {src[n - 1].strip()[:120]}", file=sys.stderr)
        print(f"{len(want & seen)} of {len(want)} raise statements of the section were reached", file=sys.stderr)
