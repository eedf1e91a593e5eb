"""The case tables of test_gpu_causal_walk.py and test_gpu_causal_normgate.py, the parts that need no GPU: the chunks per workgroup
each walk case is meant to reach (by the dispatch rule as the tests restate it, and by the rule's text in the library's source),
and that the tables between them run every instantiation they name."""
import os
import re

import pytest

import test_gpu_causal_normgate as ng
import test_gpu_causal_walk as walk
from test_gpu_causal_varlen import tok4_walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walk_cases_reach_two_four_and_eight_chunks_per_workgroup():
    assert (walk.T + 63) // 64 == walk.N_CHUNKS == 19 and walk.T - 18 * 64 == 5
    assert [(B * walk.H, tok4_walk(8, walk.N_CHUNKS, B * walk.H)) for B, _, _ in walk.WALKS] == [(33, 2), (55, 4), (88, 8)]
    for B, cpw, groups in walk.WALKS:
        assert walk.walk_groups(walk.N_CHUNKS, cpw) == groups
        assert groups[0][0] == 0 and groups[-1][1] == 19 and all(a[1] == b[0] for a, b in zip(groups, groups[1:]))
    # the last group: one chunk at cpw = 2, partial and longer than one chunk at 4 and 8
    assert [g[-1][1] - g[-1][0] for _, _, g in walk.WALKS] == [1, 3, 3]
    # the benchmark's C5 shape (B = 4, H = 4, 128 chunks) walks eight; the full-size C5 test (B = 2) four
    assert tok4_walk(8, 128, 16) == 8 and tok4_walk(8, 128, 8) == 4


def test_walk_cases_cover_the_seven_walking_instantiations():
    hl = {"tf32": 2, "split": 1, "bf16": 0}
    inst = sorted((K // 64, hl[s]) for K, _, s in walk.ARITH)
    assert inst == [(1, 1), (1, 2), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2)]
    assert all(walk.tok4_most(K, s) == 8 for K, _, s in walk.ARITH)
    # ... and no other instantiation walks: K = 64 / 128 at single-bf16 summaries and K = 256 keep one chunk per workgroup
    walking = [(nk, h) for nk in (1, 2, 3, 4) for h in (0, 1, 2) if walk.tok4_most(64 * nk, {v: k for k, v in hl.items()}[h]) > 1]
    assert sorted(walking) == inst
    B, K, V, s = walk.CONTROL
    assert walk.tok4_most(K, s) == 1 and tok4_walk(1, walk.N_CHUNKS, B * walk.H) == 1
    assert any(V // 64 >= 2 for K, V, _ in walk.ARITH if K == 64)   # two V slices at K = 64


def test_walk_rule_is_the_one_in_the_source():
    """tok4_walk / tok4_most restate csf_tok4_walk (capi_causal.hip) and csf_tok4_cpw (causal_bf16.hpp): the texts they were written from."""
    squash = lambda s: re.sub(r"\s+", "", s)
    capi = squash(open(os.path.join(ROOT, "mhla_amd", "csrc", "capi_causal.hip")).read())
    hpp = open(os.path.join(ROOT, "mhla_amd", "csrc", "causal_bf16.hpp")).read()
    assert squash("while (cpw * 2 <= most && (long)((n + cpw * 2 - 1) / (cpw * 2)) * bh >= 256) cpw *= 2;") in capi
    assert squash("return (NK <= CSF_TOK4_WALK_NK && (HL || NK > 2)) ? CSF_TOK4_CPW : 1;") in squash(hpp)
    assert re.search(r"#define\s+CSF_TOK4_CPW\s+8\b", hpp) and re.search(r"#define\s+CSF_TOK4_WALK_NK\s+3\b", hpp)


def test_walk_pack_has_66_chunks_and_walks_eight():
    from mhla_amd import causal_varlen_plan
    cu, chunks = walk.pack_cu()
    plan = causal_varlen_plan(cu, "cpu")
    assert chunks == plan.n_chunks == 66 and len(cu) == 31 and cu[-1] == 6 * sum(walk.PACK_LENGTHS) and plan.max_chunks == 4
    assert tok4_walk(8, 66, walk.PACK_H) == 8 and tok4_walk(8, 66, 8) == 2
    # sequence boundaries inside the first walk of eight chunks, ragged chunks in the middle of it
    assert plan.seq[:8].tolist() == [0, 1, 1, 2, 2, 2, 3, 4] and plan.table[:8, 1].tolist() == [63, 64, 1, 64, 64, 1, 1, 64]


def test_fused_kernel_names():
    assert [ng.fused_kernel(V) for V in (64, 256, 384, 512)] == ["k_csf_out4<norm>", "k_csf_out4<norm>", "k_csf_out4<norm,2>", "k_csf_out4<norm,2>"]
    assert [ng.fused_kernel(V, True) for V in (64, 512)] == ["k_csf_out4<norm,tab>", "k_csf_out4<norm,2,tab>"]
    capi = open(os.path.join(ROOT, "mhla_amd", "csrc", "capi_causal.hip")).read()
    for name in ("k_csf_out4<norm>", "k_csf_out4<norm,tab>", "k_csf_out4<norm,2>", "k_csf_out4<norm,2,tab>", "k_csf_bwd_tok4", "k_csf_bwd_tok4<tab>"):
        assert f'"{name}"' in capi, name


@pytest.mark.parametrize("V", [256, 512])
def test_zero_rows_and_visible_eps_inputs(V):
    """What the GPU cases assume of their inputs, on the oracle: exact zeros on the padded rows; a norm_eps of mean(o^2) moves y."""
    import torch
    from conftest import rel_err
    from test_gpu_causal import causal_inputs
    q, k, v, mix, _ = causal_inputs(1, 200, 3, 64, V, 8, torch.bfloat16, seed=200 + V)
    g, w = ng.gate_and_weight(1, 200, 3, V, True, True)
    o = ng.oracle_o(q, k, v, mix)
    assert rel_err(ng.cpu_norm(o, g, w, 1e-5), ng.cpu_norm(o, g, w, float(o.square().mean()))) > 0.2
    for t in (q, k, v):
        t[:, :70] = 0
    o = ng.oracle_o(q, k, v, mix)
    assert float(o[:, :70].abs().max()) == 0.0 and float(o[:, 70:].abs().min(dim=-1).values.max()) > 0.0
    assert float(ng.cpu_norm(o, g, w, 1e-5)[:, :70].abs().max()) == 0.0
