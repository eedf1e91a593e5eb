"""GPU parity of the backward token kernel's chunk walk (k_csf_bwd_tok4, causal_bf16.hpp): a workgroup walks cpw = 1, 2, 4 or 8
consecutive chunks -- csf_tok4_walk of capi_causal.hip takes the largest power of two for which ceil(n / cpw) B H >= 256 -- and
requests the next chunk's Q / K / dO / V tiles into the ring slots of the chunk in flight.  The benchmark's C5 shape (B H = 16,
128 chunks) walks eight chunks; the other GPU tests have B H <= 8 and reach four at the most.

Shape: T = 1157 = 18 full chunks + 5 tokens (n = 19, the last chunk ragged), H = 11, bf16; B = 3, 5, 8 give B H = 33, 55, 88 and
with them cpw = 2, 4, 8 (WALKS below: the last group is partial at 4 and 8, and longer than one chunk).  Crossed with the seven
instantiations <K / 64, summaries> that walk (ARITH below; K = 64 with two V slices: the next chunk's tiles are requested behind
the LAST V slice), one control that does not (K = 256: csf_tok4_cpw<4, .> = 1), and one pack whose sequence boundaries and ragged
chunks fall inside eight-chunk walks.

Runner, reference and bounds: test_gpu_causal.run_causal / test_gpu_causal_varlen.run_varlen unchanged -- forward and backward
against the fp32 oracle, out / dq / dk / dv globally and chunk by chunk, dmix globally.  The fp64 model of the default summaries'
storage format at these inputs (tools/causal_per_chunk_model.py --walk, profiles/causal_walk_parity.md) stays within the figure
CAUSAL_CHUNK_TOL_H16 was derived with, so the constant holds here as it stands."""
import pytest
import torch

from gpu_util import launches
from test_gpu_causal import run_causal
from test_gpu_causal_varlen import run_varlen, tok4_walk

pytestmark = pytest.mark.gpu

T, H, N_CHUNKS = 1157, 11, 19
# (B, chunks per workgroup, the workgroups' chunks along the sequence)
WALKS = [(3, 2, [(c, min(c + 2, 19)) for c in range(0, 19, 2)]),   # nine pairs, then chunk 18 alone
         (5, 4, [(0, 4), (4, 8), (8, 12), (12, 16), (16, 19)]),
         (8, 8, [(0, 8), (8, 16), (16, 19)])]
# (K, V, summaries): the walking instantiations <1,2> <1,1> <2,2> <2,1> <3,2> <3,1> <3,0> of k_csf_bwd_tok4<K / 64, summaries>
# (h16 = 2: "tf32", hi + lo = 1: "split", single bf16 = 0: "bf16")
ARITH = [(64, 128, "tf32"), (64, 128, "split"), (128, 128, "tf32"), (128, 128, "split"),
         (192, 192, "tf32"), (192, 192, "split"), (192, 192, "bf16")]
CONTROL = (8, 256, 256, "tf32")   # B, K, V, summaries: one chunk per workgroup, a grid of 19 x 88
PACK_LENGTHS, PACK_H, PACK_CHUNKS = (63, 65, 129, 1, 200), 32, 66


def tok4_most(K, summaries):
    """csf_tok4_cpw<K / 64, summaries> of causal_bf16.hpp: the most chunks a workgroup of that instantiation walks."""
    nk, hl = K // 64, {"tf32": 2, "split": 1, "bf16": 0}[summaries]
    return 8 if nk <= 3 and (hl or nk > 2) else 1


def walk_groups(n, cpw):
    """[first, behind-last) chunks of every workgroup along the sequence (k_csf_bwd_tok4: c_first = blockIdx.x cpw)."""
    return [(c, min(c + cpw, n)) for c in range(0, n, cpw)]


def pack_cu():
    """The pack of test_gpu_causal_varlen.test_backward_token_kernel_walks_across_sequence_boundaries: lengths 63, 65, 129, 1, 200
    cycled until it has 66 chunks (30 sequences, 2748 tokens); every sequence is cut into its own chunks."""
    cu, chunks = [0], 0
    while chunks < PACK_CHUNKS:
        n = PACK_LENGTHS[(len(cu) - 1) % len(PACK_LENGTHS)]
        cu.append(cu[-1] + n)
        chunks += (n + 63) // 64
    return tuple(cu), chunks


@pytest.mark.parametrize("K,V,summaries", ARITH, ids=[f"K{K}-V{V}-{s}" for K, V, s in ARITH])
@pytest.mark.parametrize("B,cpw,groups", WALKS, ids=[f"B{B}-cpw{c}" for B, c, _ in WALKS])
def test_token_kernel_chunk_walk(B, cpw, groups, K, V, summaries):
    assert (T + 63) // 64 == N_CHUNKS and T % 64 == 5
    assert tok4_most(K, summaries) == 8 and tok4_walk(8, N_CHUNKS, B * H) == cpw, (tok4_most(K, summaries), tok4_walk(8, N_CHUNKS, B * H))
    assert walk_groups(N_CHUNKS, cpw) == groups
    ran = launches(lambda: run_causal(B, T, H, K, V, N_CHUNKS, torch.bfloat16, seed=T + K, summaries=summaries))
    assert ran.get("k_csf_bwd_tok4") == 1, ran


def test_token_kernel_without_a_walk_at_the_same_shape():
    """K = 256 keeps one chunk per workgroup whatever B H is: the control of the cases above."""
    B, K, V, summaries = CONTROL
    assert tok4_most(K, summaries) == 1 and tok4_walk(tok4_most(K, summaries), N_CHUNKS, B * H) == 1
    ran = launches(lambda: run_causal(B, T, H, K, V, N_CHUNKS, torch.bfloat16, seed=T + K, summaries=summaries))
    assert ran.get("k_csf_bwd_tok4") == 1, ran


def test_token_kernel_walks_eight_chunks_across_sequence_boundaries():
    """The pack at H = 32: ceil(66 / 8) 32 = 288 >= 256, so its 66 chunks are walked eight at a time -- 0..7, ..., 56..63, then 64
    and 65 -- with sequence boundaries, one-token and 63-token chunks inside the walks."""
    import mhla_amd
    cu, chunks = pack_cu()
    assert chunks == PACK_CHUNKS and mhla_amd.causal_varlen_plan(cu, "cpu").n_chunks == PACK_CHUNKS
    assert tok4_most(64, "tf32") == 8 and tok4_walk(8, PACK_CHUNKS, 1 * PACK_H) == 8
    ran = launches(lambda: run_varlen(cu, PACK_H, 64, 64, torch.bfloat16, seed=PACK_CHUNKS))
    assert ran.get("k_csf_bwd_tok4<tab>") == 1, ran
