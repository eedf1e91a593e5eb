"""`PagedDecodeCache`, the fla layer's scheduler step on it and `serve_schedule`, host side, no GPU: every ValueError of `schedule` with
the cache unchanged, every refusal of the layer before any library call, the two library calls one layer step records under
tools/fake_decode_lib.py (CPU tensors), and the continuous-batching policy as a pure function."""
import os
import sys

import pytest
import torch

from mhla_amd import PagedCausalState, PoolExhausted, _lib, modules, ops
from mhla_amd.hosts.gpt import GPT_MHLA, serve_schedule
from mhla_amd.modules import MHLA, DecodeCache, PagedDecodeCache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fake_decode_lib import Session  # noqa: E402

D, HEADS, K, V = 64, 2, 16, 32     # hidden 64, expand_k 0.5: K = 16, V = 32
PRO, EXT = "mhla_featmap_rotary_decode", "mhla_causal_extend_packed"
# positions of the recorded arguments (test_decode_prologue_cpu.py, test_extend_packed_cpu.py)
XP = dict(q=0, k=1, cos=2, tab_rows=5, pos=6, slot=7, n_slots=8, ntok=9, off=10, T=11, yq=13, yk=14, B=15, H=16, Hkv=17, fmap=19)
XE = dict(q=0, k=1, S=5, n_pages=6, table=7, cap=8, pos=11, slot=12, n_slots=13, off=14, n_tokens=15, out=19, y=23, B=25, H=26, Hkv=27)


def layer(**kw):
    torch.manual_seed(2)
    return MHLA(mode="chunk", hidden_size=D, num_heads=HEADS, feature_map="relu", layer_idx=0, max_chunks=4, **{"exact_decoding": True, **kw}).eval()


def cache(n_slots=4, cap=4, n_pages=6):
    return PagedDecodeCache(n_slots, cap, n_pages, "cpu")


def snapshot(c):
    return (c._step, c.lengths, c.pages_free, len(c), [[list(r) for r in p.table] for p in c._pools if p is not None])


def test_the_cache_is_exported_and_refuses_h16():
    assert modules.PagedDecodeCache is PagedDecodeCache and "PagedDecodeCache" in modules.__all__
    with pytest.raises(ValueError, match="h16.*fp32 pages only"):
        PagedDecodeCache(2, 4, 6, "cpu", page_format="h16")
    with pytest.raises(ValueError, match="non-positive size"):
        PagedDecodeCache(0, 4, 6, "cpu")
    c = cache()
    assert c.lengths == (0, 0, 0, 0) and c.pages_free == 6 and len(c) == 0 and c.get_seq_length() == 0


def test_every_value_error_of_schedule_leaves_the_cache_as_it_was():
    c = cache()
    m = layer()
    x = torch.randn(1, 5, D)
    with Session(ops, _lib), torch.no_grad():
        c.schedule([2, 0], [0, 3, 5])
        m(x, past_key_values=c, use_cache=True)
    assert c.lengths == (2, 0, 3, 0)
    before = snapshot(c)
    for slots, cu, match in [
            ([0, 4], [0, 1, 2], r"slots \[4\] are outside 0 \.\. 3"),
            ([0, -1], [0, 1, 2], r"slots \[-1\] are outside"),
            ([1, 1], [0, 1, 2], r"slots \[1\] are given more than once"),
            ([], [0], "no slot given"),
            ([0, 1.0], [0, 1, 2], "slots must be ints"),
            ([0, True], [0, 1, 2], "slots must be ints"),
            ([0, 1], [1, 2, 3], "must start at 0"),
            ([0, 1], [0, 2, 1], "non-decreasing"),
            ([0, 1], [0, 1], "cu_seqlens has 2 entries for 2 slots"),
            ([0, 1], [0, 1, 2, 3], "cu_seqlens has 4 entries for 2 slots"),
            ([0, 1], torch.tensor([[0, 1, 2]]), "1-D integer tensor"),
            ([0, 1], [0, 1.5, 2], "1-D sequence of ints")]:
        with pytest.raises(ValueError, match=match):
            c.schedule(slots, cu)
        assert snapshot(c) == before, (slots, cu)


def test_every_layer_runs_exactly_once_between_two_schedules():
    c = cache()
    m0, m1 = layer(), layer()
    m1.layer_idx = 1
    x = torch.randn(1, 5, D)
    with Session(ops, _lib) as s, torch.no_grad():
        with pytest.raises(ValueError, match="no step is scheduled"):
            m0(x, past_key_values=c, use_cache=True)
        c.schedule([2, 0], [0, 3, 4])
        with pytest.raises(ValueError, match="ends at 4, the pack has N = 5"):
            m0(x, past_key_values=c, use_cache=True)
        assert s.calls == [] and c.lengths == (0, 0, 0, 0) and len(c) == 0
        c.schedule([2, 0], [0, 3, 5])
        m0(x, past_key_values=c, use_cache=True)
        m1(x, past_key_values=c, use_cache=True)
        n = len(s.calls)
        with pytest.raises(ValueError, match="layer 0 has already run the scheduled step"):
            m0(x, past_key_values=c, use_cache=True)
        assert len(s.calls) == n and c.lengths == (2, 0, 3, 0)
        c.schedule([0], [0, 5])
        m0(x, past_key_values=c, use_cache=True)
        before = snapshot(c)
        with pytest.raises(ValueError, match=r"layers \[1\] have not run the last scheduled step"):
            c.schedule([0], [0, 5])
        assert snapshot(c) == before
        m1(x, past_key_values=c, use_cache=True)
        c.schedule([1], [0, 5])
    assert c.lengths == c.pool(1).lengths == (7, 0, 3, 0) and len(c) == 2


def test_every_refusal_of_the_layer_comes_before_any_library_call():
    x = torch.randn(1, 5, D)

    def refused(exc, match, m, hidden=x, use_cache=True, **kw):
        c = cache()
        c.schedule([1], [0, hidden.shape[1]])
        with Session(ops, _lib) as s, torch.no_grad():
            with pytest.raises(exc, match=match):
                m(hidden, past_key_values=c, use_cache=use_cache, **kw)
        assert s.calls == [] and len(c) == 0 and c.lengths == (0,) * 4 and c._step.ran == set()

    refused(ValueError, "exact_decoding=True", layer(exact_decoding=False))
    refused(ValueError, "use_cache=True", layer(), use_cache=False)
    refused(ValueError, r"the step's pack \[1, N, D\]", layer(), hidden=torch.randn(2, 5, D))
    refused(ValueError, "no attention_mask", layer(), attention_mask=torch.ones(1, 5, dtype=torch.long))
    refused(NotImplementedError, "cu_seqlens as an argument", layer(), cu_seqlens=torch.tensor([0, 5]))
    refused(NotImplementedError, "token_counts as an argument", layer(), token_counts=[5])
    refused(NotImplementedError, "speculative as an argument", layer(), speculative=True)
    refused(NotImplementedError, "use_short_conv", layer(use_short_conv=True))
    refused(NotImplementedError, r"head_k_dim % 8 == 0", MHLA(hidden_size=48, num_heads=2, feature_map="relu", layer_idx=0, exact_decoding=True).eval(),
            hidden=torch.randn(1, 5, 48))
    m = layer()
    m.layer_idx = None
    refused(ValueError, "layer_idx, which is None", m)
    # an existing cache keeps its refusals: the new call kind is recognised by the cache's type alone
    with Session(ops, _lib) as s, torch.no_grad():
        with pytest.raises(NotImplementedError, match="speculative=True on an empty cache"):
            layer()(x, past_key_values=DecodeCache(), use_cache=True, speculative=True)
    assert s.calls == []


def test_what_the_operators_refuse_is_raised_before_the_first_launch():
    m = layer()
    with Session(ops, _lib) as s, torch.no_grad():
        c = cache(n_pages=2)
        c.schedule([0, 1], [0, 130, 140])   # 3 + 1 pages of 2
        with pytest.raises(PoolExhausted, match="need 4 more pages, the pool has 2 free"):
            m(torch.randn(1, 140, D), past_key_values=c, use_cache=True)
        assert s.calls == [] and c.lengths == (0,) * 4 and c.pages_free == 2 and c._step.ran == set()
        c = cache(cap=2, n_pages=8)
        c.schedule([0, 3], [0, 129, 130])   # slot 0 would need 3 chunks of 2
        with pytest.raises(IndexError, match=r"sequences \[0\].*need up to 3 chunks but the state holds only 2"):
            m(torch.randn(1, 130, D), past_key_values=c, use_cache=True)
        assert s.calls == [] and c.lengths == (0,) * 4 and c.pages_free == 8
        big = MHLA(hidden_size=D, num_heads=HEADS, feature_map="relu", layer_idx=0, max_chunks=2, exact_decoding=True).eval()
        c = cache(cap=4, n_pages=8)
        c.schedule([0], [0, 129])
        with pytest.raises(IndexError, match="mixing_matrix has only 2 rows"):
            big(torch.randn(1, 129, D), past_key_values=c, use_cache=True)
        assert s.calls == [] and c.pages_free == 8


@pytest.mark.parametrize("opts", [{}, {"num_kv_heads": 1, "grouped_state": True}, {"num_kv_heads": 1}, {"use_output_gate": False}],
                         ids=["default", "grouped-state", "repeated-kv", "no-output-gate"])
def test_a_recorded_layer_step(opts):
    m = layer(**opts)
    hkv = 1 if opts.get("grouped_state") else HEADS
    c = cache(n_pages=7)
    with Session(ops, _lib) as s, torch.no_grad():
        c.schedule([3, 0], [0, 70, 75])
        o, attn, back = m(torch.randn(1, 75, D), past_key_values=c, use_cache=True)
        assert tuple(o.shape) == (1, 75, D) and attn is None and back is c
        pool = c.pool(0)
        assert isinstance(pool, PagedCausalState) and pool.page_format == "fp32" and pool.dims == (4, hkv, 4, K, V)
        assert c.lengths == (5, 0, 0, 70) and c.pages_free == 7 - 3 and c.get_seq_length() == 70 and len(c) == 1
        first = len(s.calls)
        c.schedule([0, 3, 1], [0, 1, 60, 190])
        s.name(pages=pool.pages, table=pool.table_dev, pos=pool.pos, P=pool.P, cos=c._rotary[0][0], step=c._step.off_dev)   # (offsets and slot map: one upload)
        m(torch.randn(1, 190, D), past_key_values=c, use_cache=True)
    # (a layer that does not fuse norm x gate into the chain runs its norm kernel afterwards, as on every other path)
    tail = [] if m.fuse_norm_and_gate else ["mhla_rmsnorm_gate_fwd"]
    assert [x.name for x in s.calls[:first]] == [x.name for x in s.calls[first:]] == [PRO, EXT] + tail, "one prologue, one packed extend, in this order"
    assert not any(x.name == "mhla_featmap_rotary" for x in s.calls)
    p, e = (x.args for x in s.calls[first:first + 2])
    # the prologue: q and k in place at the positions of the pool's slots, the step's offsets, the layer's tables of 64 x capacity rows
    assert p[XP["q"]] == p[XP["yq"]] and p[XP["k"]] == p[XP["yk"]] and p[XP["q"]][0] == "view" and p[XP["q"]][3] == 0
    assert p[XP["cos"]] == ("ptr", "cos", 0) and p[XP["tab_rows"]] == 256
    assert p[XP["pos"]] == ("ptr", "pos", 0) and p[XP["slot"]] == ("ptr", "step", 4 * 4) and p[XP["n_slots"]] == 4
    assert p[XP["off"]] == ("ptr", "step", 0) and p[XP["ntok"]] == ("null",)
    assert (p[XP["T"]], p[XP["B"]], p[XP["H"]], p[XP["Hkv"]], p[XP["fmap"]]) == (190, 3, HEADS, hkv, 1)
    # the extend: the same q and k, the pool's pages and table, the same slot map
    assert e[XE["q"]] == p[XP["q"]] and e[XE["k"]] == p[XP["k"]]
    assert e[XE["S"]] == ("ptr", "pages", 0) and e[XE["n_pages"]] == 7 and e[XE["table"]] == ("ptr", "table", 0) and e[XE["cap"]] == 4
    assert e[XE["pos"]] == ("ptr", "pos", 0) and e[XE["slot"]] == ("ptr", "step", 4 * 4) and e[XE["n_slots"]] == 4
    assert (e[XE["n_tokens"]], e[XE["B"]], e[XE["H"]], e[XE["Hkv"]]) == (190, 3, HEADS, hkv)
    fused = m.fuse_norm_and_gate
    assert (e[XE["out"]] == ("null",)) == fused and (e[XE["y"]] == ("null",)) == (not fused), "norm x gate in the chain exactly when the layer fuses them"
    assert c.lengths == (6, 130, 0, 129) and c.pages_free == 0
    # release and fork act on every layer's pool
    c.fork(0, 2)
    assert c.lengths == (6, 130, 6, 129)
    c.release([3, 1])
    assert c.lengths == (6, 0, 6, 0) and c.pages_free == 6 and "PagedDecodeCache(" in repr(c)


def test_the_host_runs_a_step_and_keeps_its_refusals():
    torch.manual_seed(4)
    model = GPT_MHLA(vocab_size=32, hidden_size=D, num_layers=2, num_heads=HEADS, max_seq_len=256, exact_decoding=True).eval()
    ids = torch.randint(0, 32, (1, 75))
    c = PagedDecodeCache(4, 32, 6, "cpu")
    with Session(ops, _lib) as s, torch.no_grad():
        with pytest.raises(NotImplementedError, match="cu_seqlens with a cache"):
            model(ids, cache=c, cu_seqlens=torch.tensor([0, 70, 75]))
        assert s.calls == []
        c.schedule([3, 0], [0, 70, 75])
        logits = model(ids, cache=c)
    assert tuple(logits.shape) == (1, 75, 32)
    assert [x.name for x in s.calls] == [PRO, EXT] * 2
    assert c.pool(0).table == c.pool(1).table and c.pool(0).lengths == c.pool(1).lengths == (5, 0, 0, 70), "identical page-rule calls, identical tables"
    with pytest.raises(ValueError, match="exact_decoding=True"):
        GPT_MHLA(vocab_size=32, hidden_size=D, num_layers=1, num_heads=HEADS).serve([[1, 2]], 2, n_slots=1, n_pages=2)


PROMPTS = (70, 5, 130, 64, 1)


def replay(steps, prompts, n, n_slots, step_tokens, n_pages):
    """Walk a schedule as `serve` would: returns (tokens fed per request, ids emitted per request, facts the tests ask about)."""
    fed, out, where = [0] * len(prompts), [0] * len(prompts), {}
    holder, used, held_pages = {}, [set() for _ in range(n_slots)], 0
    facts = dict(mixed=False, reused=False, first_decode_at=[], max_pages=0)
    for slots, cu, kinds in steps:
        assert cu[0] == 0 and all(b >= a for a, b in zip(cu, cu[1:])) and len(cu) == len(slots) + 1 == len(kinds) + 1
        assert cu[-1] <= step_tokens and cu[-1] > 0, "no step exceeds step_tokens, none is empty"
        assert len(set(slots)) == len(slots) and all(0 <= s < n_slots for s in slots)
        seen = set()
        for slot, a, b, (r, kind) in zip(slots, cu, cu[1:], kinds):
            take = b - a
            assert take > 0
            if r not in where:      # admission: FIFO, into a slot nobody holds
                assert r == len(where), "admission is FIFO"
                assert slot not in holder, "no slot holds two requests at once"
                where[r], holder[slot] = slot, r
                facts["reused"] |= bool(used[slot])
                used[slot].add(r)
                held_pages += -(-(prompts[r] + n) // 64)
            assert where[r] == slot and holder[slot] == r
            if kind == "decode":
                assert take == 1 and fed[r] >= prompts[r]
                if fed[r] == prompts[r]:
                    facts["first_decode_at"].append(fed[r])
                out[r] += 1
            else:
                assert fed[r] + take <= prompts[r] and (kind == "first") == (fed[r] + take == prompts[r])
                out[r] += kind == "first"
            fed[r] += take
            seen.add(kind == "decode")
        facts["mixed"] |= seen == {True, False}
        facts["max_pages"] = max(facts["max_pages"], held_pages)
        assert held_pages <= n_pages
        kinds_of = [k for _, k in kinds]
        assert kinds_of == sorted(kinds_of, key=lambda k: k != "decode"), "every decoding request takes its token first"
        for slot, (r, _) in zip(slots, kinds):   # a finished request's slot is released at once
            if out[r] == n:
                del holder[slot]
                held_pages -= -(-(prompts[r] + n) // 64)
    return fed, out, facts


def test_serve_schedule():
    steps = serve_schedule(PROMPTS, 6, n_slots=2, n_pages=100, capacity_chunks=32, step_tokens=48)
    fed, out, facts = replay(steps, PROMPTS, 6, 2, 48, 100)
    assert fed == [p + 5 for p in PROMPTS], "every request gets exactly its prompt plus 5 further tokens"
    assert out == [6] * 5
    # (conditions of the inputs, traced: they say that the cases below are exercised)
    assert facts["mixed"], "a step mixes a prompt slice with a decode token"
    assert facts["reused"], "a slot is reused"
    assert 64 in facts["first_decode_at"], "a request decodes its first token at position 64"
    assert steps == serve_schedule(list(PROMPTS), 6, 2, 100, 32, 48), "a pure function"


def test_serve_schedule_waits_for_pages():
    steps = serve_schedule(PROMPTS, 6, n_slots=2, n_pages=3, capacity_chunks=32, step_tokens=48)
    fed, out, facts = replay(steps, PROMPTS, 6, 2, 48, 3)
    assert fed == [p + 5 for p in PROMPTS] and out == [6] * 5 and facts["max_pages"] == 3
    # the 130-token request (3 pages) moves in only when nothing else runs, although a slot was free before
    alone = [i for i, (_, _, kinds) in enumerate(steps) if any(r == 2 for r, _ in kinds)]
    assert all(len(steps[i][0]) == 1 for i in alone)
    first = alone[0]
    assert all(out_r == 6 for out_r in replay(steps[:first], PROMPTS[:2], 6, 2, 48, 3)[1]), "requests 0 and 1 have finished before it starts"
    assert any(len(steps[i][0]) == 1 and steps[i][2][0][0] == 0 for i in range(first)), "request 0 ran beside a free slot while it waited"


def test_serve_schedule_refusals_and_edges():
    assert serve_schedule(PROMPTS, 0, 2, 100, 32, 48) == [] and serve_schedule((), 6, 2, 100, 32, 48) == []
    one = serve_schedule((3,), 1, 1, 1, 1, 1)
    assert one == [((0,), (0, 1), ((0, "prompt"),)), ((0,), (0, 1), ((0, "prompt"),)), ((0,), (0, 1), ((0, "first"),))]
    for kw, match in [(dict(prompt_lens=(0, 4)), r"requests \[0\]"), (dict(prompt_lens=(4, 2044)), r"requests \[1\].*capacity of 2048 tokens"),
                      (dict(n_pages=2), r"requests \[2\].*pool's 2 pages"), (dict(step_tokens=1), "at least n_slots"), (dict(n_slots=0), "must be positive")]:
        args = dict(prompt_lens=PROMPTS, max_new_tokens=6, n_slots=2, n_pages=100, capacity_chunks=32, step_tokens=48)
        with pytest.raises(ValueError, match=match):
            serve_schedule(**{**args, **kw})
