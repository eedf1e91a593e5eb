"""Shared helpers for the -m gpu parity tests: seeded inputs and oracle calls."""
import ctypes

import torch

from conftest import rel_err, rms_ratio
from oracle import mhla_oracle as orc

DEV = "cuda"
# Tolerances, derived from the arithmetic rather than fitted to observations.  u = unit roundoff of the
# tensor dtype (round to nearest: |fl(x) - x| <= u |x|; bf16 has 8 significand bits: u = 2^-8; fp16 11: u = 2^-11).
#  * fp32 tensors: every product is exact (fp32 MFMA) or split into bf16 hi + lo parts (>= 16 significand bits, 2^-17 per
#    operand) with fp32 accumulation: 2e-4 of the tensor's maximum, five times under north_star's 1e-3.
#  * 16-bit tensors, DEFAULT arithmetic (round 5 for the block-mixing operator, round 4 for the causal one): the reference
#    computes in fp32 on the given tensors (mhla_dit/train.py:12-13: no autocast; naive.py:39) and so do the kernels -- every
#    intermediate that feeds a second contraction (block / chunk summaries, dP = dO / n, score tiles) keeps >= 16 significand
#    bits (fp32 summaries, bf16 hi + lo operands).  What is left is the ONE final rounding of a 16-bit result (<= u |x| PER
#    ELEMENT, which no implementation can avoid) plus north_star's 1e-3 for everything the kernels add:
#        max|got - want| <= (u + 1e-3) max|want|   and   max(|got - want| - u |want|) <= 1e-3 max|want|   (check() asserts both);
#    fp32-stored results of 16-bit problems (dW, dmix) get the 1e-3 alone (DW_TOL, CAUSAL_DMIX_TOL).
#  * 16-bit tensors, OPT-IN reduced precision (summaries="bf16": MHLA_FLAG_BF16_SUMMARIES / MHLA_CAUSAL_BF16_SUMMARIES): the
#    kernels keep K intermediate tiles as single bf16 values on their way through the matrix pipe -- K = 1 for outputs (the
#    block / chunk summary, or the score tile of the small-sequence path), K = 2 for gradients (additionally dP = dO / n, resp.
#    the dS / dP summaries).  An intermediate rounding perturbs the result by at most u times the magnitude of what it feeds,
#    i.e. <= u max|x| when nothing averages (contraction length 1: the S = 1, M <= 4 corner cases of the fuzz tests reach
#    0.8 u .. 1.7 u) and ~ u / sqrt(L) over a contraction of length L (BASELINE shapes, L >= 64: 0.2 u .. 0.8 u observed):
#        max|got - want| <= (1 + K) u max|want|     (TOL_BF16SUM = 2 u for outputs, GTOL_BF16SUM = 3 u for gradients).
#    With a mixing matrix that has NEGATIVE entries (the "signed" cases below) a single-bf16 intermediate that feeds the normaliser's
#    signed sum is amplified by kappa_n = max (sum_j |W_ij| z_j + eps) / n_i, the cancellation in that sum:
#        max|got - want| <= (1 + K kappa) u max|want|,   kappa = max(1, kappa_n) of the case from its fp64 reference (bm_tols_signed).
#    Every other bound carries over to signed W unchanged: what the rounding of a stored summary costs is governed by kappa_G and
#    kappa_dKV (mix_conditioning), and the signed cases keep both below 2.5 -- below the 1.9 .. 21.6 of the w="rand" cases the bounds
#    already hold for; the normaliser's rows stay fp32 values (bf16 hi + lo in the matrix pipe): kappa_n x 2^-16 is negligible.
UNIT_ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TOL = {torch.float32: 2e-4, torch.bfloat16: 2.0 ** -8 + 1e-3, torch.float16: 2.0 ** -11 + 1e-3}
GTOL = dict(TOL)
DW_TOL = {torch.float32: 2e-4, torch.bfloat16: 1e-3, torch.float16: 1e-3}
TOL_BF16SUM = {torch.float32: 2e-4, torch.bfloat16: 2 * 2.0 ** -8, torch.float16: 2 * 2.0 ** -11}
GTOL_BF16SUM = {torch.float32: 2e-4, torch.bfloat16: 3 * 2.0 ** -8, torch.float16: 3 * 2.0 ** -11}
CAUSAL_TOL = TOL
CAUSAL_DMIX_TOL = DW_TOL
# PER-CHUNK criterion of the causal operator (check_chunks()).  check() normalises by the largest element of the WHOLE tensor, which
# suits the block-mixing operator (blocks of similar magnitude) but not the causal one, whose magnitudes depend on position by
# construction: out / dq of chunk i sum over i + 1 chunks and grow along the sequence, dk / dv of chunk j collect from the chunks
# behind j and shrink, and the last chunk's dk / dv hold the diagonal term alone -- at T = 8200, K = 192 the last chunk's dk is
# 0.6 % of the tensor's maximum, so under the global bound of 4.9e-3 it may be 80 % wrong.  check_chunks() makes check()'s three
# assertions for every 64-token chunk, normalised by that chunk's own reference.  The bounds carry over chunk by chunk because
# every summary tile (S_j, P_i, dP_i, dS_j) belongs to ONE chunk and is rounded relative to itself, and a chunk of a result is a
# product of that chunk's tokens with that chunk's summaries: fp32 tensors, summaries="split", force_generic and bf16 beyond the
# pipeline keep CAUSAL_TOL[dtype]; summaries="bf16" keeps TOL_BF16SUM / GTOL_BF16SUM.
#  * DEFAULT 11-bit stored summaries ("tf32": h16 -- fp16 payload x one power-of-two multiplier per 16-row strip of a chunk tile,
#    DESIGN.md section 3e): the bound comes from an fp64 model of the storage format (causal_fp64(..., h16=True) below, written
#    from the description: S / dP with measured multipliers, P / dS with bound multipliers, everything else fp64), never from
#    what the kernels give.  Its per-chunk error against the fp64 operator on the bf16-rounded inputs of causal_inputs (seed
#    T + K, B = 1, H = 2) over (321, 64, 64), (449, 128, 256), (1000, 128, 256), (2100, 256, 256), (8192, 64, 64), (8200, 192, 192)
#    -- tools/causal_per_chunk_model.py, profiles/causal_per_chunk_parity.md -- is at most H16_CHUNK_MODEL_ERR.
#    Bound: u + max(1e-3, 2 x that); the factor 2 covers another summation order, the bf16 hi + lo operand split (2^-17 per
#    operand) and one seed.
H16_CHUNK_MODEL_ERR = 4.7e-4   # out and dk at T = 8192, K = V = 64 (the same runs: 3.4e-4 of the tensor's maximum)
H16_CHUNK_EXTRA = max(1e-3, 2 * H16_CHUNK_MODEL_ERR)
CAUSAL_CHUNK_TOL_H16 = {torch.float32: 2e-4, torch.bfloat16: 2.0 ** -8 + H16_CHUNK_EXTRA, torch.float16: 2.0 ** -11 + H16_CHUNK_EXTRA}


def bm_tols(dtype, summaries="split"):
    """(output, token-gradient, dW) tolerances of the block-mixing operator for this dtype and arithmetic."""
    if summaries == "bf16" and dtype == torch.bfloat16:
        return TOL_BF16SUM[dtype], GTOL_BF16SUM[dtype], GTOL_BF16SUM[dtype]
    return TOL[dtype], GTOL[dtype], DW_TOL[dtype]


def make_blockmix_inputs(B, H, M, S, D, dtype, seed=1234, w="linear", split=False):
    g = torch.Generator().manual_seed(seed)
    N = M * S
    q = (torch.relu(torch.randn(B, N, H, D, generator=g)) + 1e-6).to(dtype)
    k = (torch.relu(torch.randn(B, N, H, D, generator=g)) + 1e-6).to(dtype)
    v = torch.randn(B, N, H, D, generator=g).to(dtype)
    do = torch.randn(B, N, H, D, generator=g).to(dtype)
    if w == "rand":
        W = torch.rand(M, M, generator=g)
    else:
        side = int(round(M ** 0.5))
        layout = (side, side) if side * side == M else (M,)
        W = orc.block_distance_weights(layout, "linear") if M > 1 else torch.ones(1, 1)
    qd = kd = None
    if split:   # numerator pair with signs (like roped q, k), positive denominator pair
        qd, kd = q, k
        q = (q.float() * torch.sign(torch.randn(B, N, H, D, generator=g))).to(dtype)
        k = (k.float() * torch.sign(torch.randn(B, N, H, D, generator=g))).to(dtype)
    return q, k, v, W, do, qd, kd


def oracle_blockmix(q, k, v, W, do, qd, kd, eps, normalize, dtype=torch.float32):
    """The oracle's operator and closed-form gradients on the given tensors, evaluated in `dtype` (fp32: the reference of the GPU
    tests; fp64: what tests/test_blockmix_weights_cpu.py measures that reference against)."""
    f = lambda t: None if t is None else t.to(dtype)
    out = orc.blockmix_fwd(f(q), f(k), f(v), f(W), eps, f(qd), f(kd), normalize)
    grads = orc.blockmix_bwd(f(q), f(k), f(v), f(W), f(do), eps, f(qd), f(kd), normalize)
    return out, grads


# ---- mixing matrices with signs and with empty rows / columns, and an eps the results depend on -----------------------------------
# make_blockmix_inputs draws W >= 0 without an empty row or column and every test passes eps = 1e-6 against normalisers in the
# hundreds: a kernel family that drops eps, a mixing kernel that sizes a row multiplier from w instead of |w|, or a store skipped for
# an all-zero row would pass.  The cases below (tests/test_gpu_blockmix_weights.py on the GPU; tests/test_blockmix_weights_cpu.py
# shows without one that they are well conditioned and that the checks reject the errors they are meant for) use
#  * "signed": W = I + R, R with a zero diagonal, entries uniform in [-1, 1], every row rescaled to an absolute sum of 0.5 -- the
#    normaliser n_i[s] = z_i[s] + sum_j R_ij z_j[s] + eps stays positive (z > 0) and loses at most a factor kappa_n <= 4 to cancellation;
#  * "sparse": unit diagonal + two further entries per row (uniform in [0.25, 1], seeded columns), then row M // 2 and column M // 3
#    set to zero: that row's numerator is exactly 0 and its n exactly eps (out exactly 0), that column feeds nobody (dk, dv exactly 0);
#  * "signed_full": 2 rand - 1, for normalize=False only (a normaliser with these weights crosses zero);
#  * eps = visible_eps(): the power of two nearest to median(z) / 4, z the normaliser's product -- replacing it by 1e-6 moves every
#    result by 0.1 .. 1.8 of its maximum.
# Tolerances with these inputs: bm_tols() unchanged, but (1 + K kappa) u for summaries="bf16" with a signed W (bm_tols_signed; both
# derived at the top of this file).
MIX_KINDS = ("signed", "sparse")


def make_mix_weights(kind, M, generator):
    """A seeded [M, M] fp32 mixing matrix of one of the kinds above."""
    if kind == "signed_full":
        return 2 * torch.rand(M, M, generator=generator) - 1
    if kind == "signed":
        R = (2 * torch.rand(M, M, generator=generator) - 1).fill_diagonal_(0.0)
        return torch.eye(M) + R * (0.5 / R.abs().sum(1, keepdim=True).clamp_min(1e-30))
    if kind == "sparse":
        assert M >= 3
        W = torch.eye(M)
        for i in range(M):   # two distinct columns other than i
            others = torch.randperm(M - 1, generator=generator)[:2]
            W[i, others + (others >= i).long()] = 0.25 + 0.75 * torch.rand(2, generator=generator)
        W[M // 2, :] = 0.0
        W[:, M // 3] = 0.0
        return W
    raise ValueError(kind)


def _normaliser_product(q, k, M, q_den=None, k_den=None):
    """z_j[s] = Q_j[s] . ksum_j of the normaliser's pair in fp64: [(B H), M, S]."""
    qd, kd = (q, k) if q_den is None else (q_den, k_den)
    qb, kb = orc._to_blocks(qd.double(), M), orc._to_blocks(kd.double(), M)
    return torch.matmul(qb, kb.sum(-2).unsqueeze(-1)).squeeze(-1)


def visible_eps(q, k, M, q_den=None, k_den=None):
    """eps = 2^round(log2(median(z) / 4)): a power of two (exact in every format, whichever side of a product it is applied on) a
    quarter of the typical normaliser product, so that a result computed without it, or with another one, is far outside any tolerance."""
    import math
    return 2.0 ** round(math.log2(_normaliser_product(q, k, M, q_den, k_den).median().item() / 4))


def mix_conditioning(q, k, v, W, do, eps, q_den=None, k_den=None, normalize=True):
    """How much cancellation a (signed) W puts into the three mixes of a case, from the fp64 reference on its tensors:
      n_min     min n (the normaliser must stay positive);
      kappa_n   max_{i,s} (sum_j |W_ij| z_j[s] + eps) / n_i[s]          (1 for W >= 0);
      kappa_G   max_{bh,i} sum_j |W_ij| max|KV_j| / max|G_i|            (rows of W that are zero excluded: G_i is exactly 0);
      kappa_dKV max_{bh,j} sum_i |W_ij| max|dG_i| / max|dKV_j|          (columns that are zero excluded)."""
    M = W.shape[0]
    Wd = W.double()
    f = lambda t: None if t is None else t.double()
    _, aux = orc.blockmix_fwd(f(q), f(k), f(v), Wd, eps, f(q_den), f(k_den), normalize, return_aux=True)
    res = {}
    if normalize:
        res["n_min"] = aux["n"].min().item()
        res["kappa_n"] = ((torch.einsum("ij,bjs->bis", Wd.abs(), aux["z"].abs()) + eps) / aux["n"]).max().item()
        dP = orc._to_blocks(f(do), M) / aux["n"].unsqueeze(-1)
    else:
        res["n_min"], res["kappa_n"] = float("inf"), 1.0
        dP = orc._to_blocks(f(do), M)
    dG = torch.matmul(orc._to_blocks(f(q), M).transpose(-2, -1), dP)
    amax = lambda t: t.abs().amax((-2, -1))                                        # [(B H), M]
    rows, cols = Wd.abs().sum(1) > 0, Wd.abs().sum(0) > 0
    res["kappa_G"] = ((amax(aux["kv"]) @ Wd.abs().t()) / amax(aux["g"]).clamp_min(1e-300))[:, rows].max().item()
    dKV = torch.einsum("ij,bixy->bjxy", Wd, dG)
    res["kappa_dKV"] = ((amax(dG) @ Wd.abs()) / amax(dKV).clamp_min(1e-300))[:, cols].max().item()
    return res


def bm_tols_signed(dtype, summaries, kappa_n):
    """bm_tols() for a case whose W has negative entries: unchanged but for summaries="bf16", (1 + K max(1, kappa_n)) u there."""
    if summaries == "bf16" and dtype == torch.bfloat16:
        u, kappa = UNIT_ROUNDOFF[dtype], max(1.0, kappa_n)
        return (1 + kappa) * u, (1 + 2 * kappa) * u, (1 + 2 * kappa) * u
    return bm_tols(dtype, summaries)


_BF, _HF, _F32 = torch.bfloat16, torch.float16, torch.float32
_SN, _SNF, _FAST, _SP, _GEN = "small-sequence bf16", "small-sequence fp32", "bf16 fast path", "split-operand", "generic"
# The rows tests/test_gpu_blockmix_weights.py runs with both W kinds and the visible eps:
# (id, dtype, B, H, M, S, D, options, reaches); options: summaries / split (a separate normaliser pair) / gather (a random token
# permutation as the gather map) / no_smalln / force_generic; reaches = (family, summary format, launches the forward's description
# names, launches the backward's names) -- asserted through mhla_amd.describe_dispatch in tests/test_blockmix_weights_cpu.py.
MIX_CASES = [
    ("A1", _BF, 3, 2, 16, 16, 72, dict(summaries="split"), (_SN, "none (score tiles in LDS as bf16 hi + lo", ["k_sn_fwd<5,hl>"], ["k_sn_bwd<5,hl>"])),
    ("A2", _BF, 3, 2, 16, 16, 72, dict(summaries="bf16"), (_SN, "none (score tiles as single bf16", ["k_sn_fwd<5>"], ["k_sn_bwd<5>"])),
    ("A3", _BF, 2, 2, 9, 16, 64, dict(gather=True), (_SN, "none (score tiles in LDS as bf16 hi + lo", ["k_sn_fwd<4,hl>"], ["k_sn_bwd<4,hl>"])),
    ("B1", _F32, 3, 2, 13, 16, 24, {}, (_SNF, "none", ["k_snf_fwd<4>"], ["k_snf_bwd<4>"])),
    ("B2", _F32, 2, 2, 16, 16, 72, {}, (_SNF, "none", ["k_snf_fwd<5>"], ["k_snf_bwd<5>"])),
    ("C1", _BF, 2, 3, 16, 32, 64, dict(summaries="bf16"), (_FAST, "bf16", ["k_fs_wz<0>"], ["k_fs_dw"])),
    ("C2", _BF, 2, 3, 33, 20, 64, dict(summaries="bf16", gather=True), (_FAST, "bf16", ["k_fs_wz<0>"], ["k_fs_dw"])),
    ("D1", _BF, 2, 3, 16, 32, 64, {}, (_SP, "h16", ["k_sp_mixh<0>"], ["k_sp_mixh<1,dw>"])),
    ("D2", _HF, 2, 2, 40, 24, 64, {}, (_SP, "h16", ["k_sp_mixh<0>"], ["k_sp_mixh<1,dw>"])),
    ("D3", _BF, 1, 2, 70, 16, 56, {}, (_SP, "h16", ["k_sp_mixh<0>"], ["k_sp_mixh<1,dw>"])),
    ("D4", _BF, 2, 2, 16, 16, 64, dict(no_smalln=True), (_SP, "h16", ["k_sp_mixh<0>"], ["k_sp_mixh<1,dw>"])),
    ("D5", _BF, 2, 2, 5, 37, 80, dict(split=True), (_SP, "h16", ["k_sp_mixh<0>", "k_wz<0>"], ["k_sp_mixh<1,dw>", "k_wz<1>", "k_dw"])),
    ("E1", _BF, 4, 8, 130, 16, 64, {}, (_SP, "h16", ["k_sp_mixh2<0>"], ["k_sp_mixh2<1>", "k_sp_dwr<3,h16>"])),
    ("E2", _BF, 1, 2, 130, 16, 64, {}, (_SP, "h16", ["k_sp_mixh<0>"], ["k_sp_mixh<1>", "k_sp_dwr<3,h16>"])),
    ("E3", _BF, 1, 2, 200, 16, 64, {}, (_SP, "h16", ["k_sp_mixh<0>"], ["k_sp_mixh<1>", "k_sp_dwr<4,h16>"])),
    ("F1", _BF, 2, 2, 40, 24, 64, dict(summaries="split"), (_SP, "p24", ["k_sp_mixr<0>"], ["k_sp_mixr<1,dw>"])),
    ("F2", _HF, 1, 2, 5, 37, 80, dict(summaries="split", split=True), (_SP, "p24", ["k_sp_mixr<0>", "k_wz<0>"], ["k_sp_mixr<1,dw>", "k_wz<1>", "k_dw"])),
    ("F3", _BF, 1, 2, 70, 8, 64, {}, (_SP, "p24", ["k_sp_mixr<0>"], ["k_sp_mixr<1,dw>"])),
    ("G1", _F32, 1, 2, 70, 8, 64, {}, (_SP, "fp32 words", ["k_sp_mixr<0>"], ["k_sp_mixr<1,dw>"])),
    ("G2", _F32, 1, 2, 150, 21, 128, dict(split=True, gather=True), (_SP, "p24", ["k_sp_mixr<0>", "k_wz<0>"], ["k_sp_mixr<1>", "k_wz<1>", "k_sp_dwt", "k_dw"])),
    ("G3", _F32, 1, 2, 3, 33, 128, dict(split=True), (_SP, "p24", ["k_sp_mixr<0>", "k_wz<0>"], ["k_sp_mixr<1,dw>", "k_wz<1>", "k_dw"])),
    ("H1", _BF, 1, 2, 200, 16, 64, dict(summaries="bf16"), (_SP, "bf16", ["k_s16_state<0>", "k_sp_mixr_dma<0>", "k_s16_out"], ["k_sp_mixr_dma<1>", "k_sp_dwr<4>"])),
    ("H2", _BF, 2, 3, 77, 16, 64, dict(summaries="bf16"), (_SP, "bf16", ["k_s16_state<0>", "k_sp_mixr<0>", "k_wz<0>"], ["k_sp_mixr<1>", "k_wz<1>"])),
    ("I1", _F32, 1, 2, 260, 8, 64, {}, (_SP, "fp32 words", ["k_sp_mix<0>", "k_wz<0>"], ["k_sp_mix<1>", "k_wz<1>", "k_sp_dw"])),
    ("J1", _F32, 1, 2, 9, 20, 40, dict(force_generic=True), (_GEN, "fp32 words", ["k_mix<0,0>"], ["k_mix<1,0>"])),
    ("J2", _F32, 2, 2, 5, 7, 12, {}, (_GEN, "fp32 words", ["k_mix<0,0>"], ["k_mix<1,0>"])),
    # head dim above 128: ops._blockmix_wide_head's own normaliser and eps over un-normalised calls on 72-wide slices (what `reaches` describes)
    ("K1", _F32, 1, 2, 6, 20, 136, {}, (_SP, "fp32 words", ["k_sp_mixr<0>"], ["k_sp_mixr<1,dw>"])),
]
MIX_CASE = {c[0]: c for c in MIX_CASES}
# the relu(x) + eps prologue with eps = MIX_RELU_EPS on raw randn q, k: (id, dtype, B, H, M, S, D, options, reaches)
MIX_RELU_EPS = 0.25
MIX_RELU_CASES = [
    ("R1", _F32, 2, 3, 16, 16, 72, {}, (_SNF, "none", ["k_snf_fwd<5>"], ["k_snf_bwd<5>"])),
    ("R2", _BF, 2, 2, 16, 40, 72, {}, (_SP, "h16", ["k_sp_mixh<0>"], ["k_sp_mixh<1,dw>"])),
    ("R3", _BF, 2, 2, 80, 16, 64, {}, (_SP, "h16", ["k_sp_mixh<0>"], ["k_sp_mixh<1,dw>"])),
    # bf16 tensors on the other two summary formats: relu(x) + eps is no bf16 value, the token operands must keep its lo part there too
    ("R4", _BF, 2, 2, 16, 24, 64, dict(summaries="split"), (_SP, "p24", ["k_sp_mixr<0>"], ["k_sp_mixr<1,dw>"])),
    ("R5", _BF, 1, 2, 12, 24, 128, {}, (_SP, "fp32 words", ["k_sp_mixr<0>"], ["k_sp_mixr<1,dw>"])),
]


# Seeds are M * 1000 + S * 10 + D but for three rows whose "signed" inputs miss the conditions there (kappa_n = 4.5 at D4, 4.8 at G3;
# J2's contraction over D = 12 and 7 tokens lets z vary tenfold between tokens, and n crosses zero): these take the smallest seed
# 1, 2, 3, ... at which the conditions hold.  A choice of INPUTS by conditions on the fp64 reference -- no kernel result enters.
MIX_SEEDS = {"D4": 1, "G3": 3, "J2": 4}


def mix_case_seed(case):
    return MIX_SEEDS.get(case[0], case[4] * 1000 + case[5] * 10 + case[6])


def mix_case_per_block(case):
    """Rows whose arithmetic keeps >= 16 significand bits in every summary element (fp32 tensors, summaries="split", the generic
    kernels): their out, dq, dk, dv are held to the tolerance block by block as well (check_chunks with chunk = S)."""
    return case[1] == torch.float32 or case[7].get("summaries") == "split" or bool(case[7].get("force_generic"))


def make_mix_case(case, kind, eps=None):
    """The tensors of a MIX_CASES row with a W of `kind`: q, k, v, do, qd, kd (block-major, rounded to the row's dtype), W, idx (the
    gather map or None) and eps (given, or the visible one)."""
    _, dtype, B, H, M, S, D, opt, _ = case
    seed = mix_case_seed(case)
    q, k, v, _, do, qd, kd = make_blockmix_inputs(B, H, M, S, D, dtype, seed, "rand", opt.get("split", False))
    W = make_mix_weights(kind, M, torch.Generator().manual_seed(seed + 1))
    idx = torch.randperm(M * S, generator=torch.Generator().manual_seed(seed + 2)).int() if opt.get("gather") else None
    return dict(q=q, k=k, v=v, do=do, qd=qd, kd=kd, W=W, idx=idx, eps=visible_eps(q, k, M, qd, kd) if eps is None else eps)


def mix_case_reference(t, normalize=True, dtype=torch.float32):
    """The oracle on the tensors of make_mix_case(): out and the dict of gradients."""
    return oracle_blockmix(t["q"], t["k"], t["v"], t["W"], t["do"], t["qd"], t["kd"], t["eps"], normalize, dtype)


def make_mix_relu_case(case, kind):
    """The tensors of a MIX_RELU_CASES row: RAW randn q, k (the kernels apply relu(x) + eps), v, do in the row's dtype, W of `kind`."""
    _, dtype, B, H, M, S, D, _, _ = case
    g = torch.Generator().manual_seed(mix_case_seed(case))
    q, k, v, do = (torch.randn(B, M * S, H, D, generator=g).to(dtype) for _ in range(4))
    W = make_mix_weights(kind, M, torch.Generator().manual_seed(mix_case_seed(case) + 1))
    return dict(q=q, k=k, v=v, do=do, qd=None, kd=None, W=W, idx=None, eps=MIX_RELU_EPS)


def mix_relu_reference(t, dtype=torch.float32, prologue=None, eps=None):
    """The oracle on relu(q) + c, relu(k) + c with the normaliser's eps; dq, dk masked by x > 0 (the prologue's gradient).  c = eps =
    the case's unless given: `prologue` / `eps` evaluate the operator with another constant on one side (what a kernel that takes
    the two from different places would compute)."""
    eps = t["eps"] if eps is None else eps
    c = eps if prologue is None else prologue
    qf, kf = torch.relu(t["q"].to(dtype)) + c, torch.relu(t["k"].to(dtype)) + c
    out, g = oracle_blockmix(qf, kf, t["v"], t["W"], t["do"], None, None, eps, True, dtype)
    g["dq"], g["dk"] = g["dq"] * (t["q"] > 0), g["dk"] * (t["k"] > 0)
    return out, g


def zero_rows_and_columns(W):
    """(indices of the rows of W that are entirely zero, of the columns)."""
    return (W == 0).all(1).nonzero().flatten().tolist(), (W == 0).all(0).nonzero().flatten().tolist()


def check_dw_rows(got, want, W, tol):
    """dW in two pieces, each normalised by its own maximum: the rows of W that are entirely zero (their n is eps alone: dW there is
    several times the other rows' and would hide them under check()'s global maximum) and all other rows."""
    zr, _ = zero_rows_and_columns(W)
    if not zr:
        return check("dW", got, want, tol)
    rest = [i for i in range(W.shape[0]) if i not in zr]
    check("dW (rows of W that are zero)", got[zr], want[zr], tol)
    return check("dW (other rows)", got[rest], want[rest], tol)


# The launch shapes of the rotary operator (tests/test_gpu_blockmix_rope.py holds the kernels to fp64 at them, tests/test_rope_ref_cpu.py
# the reference's own conditioning): (B, H, M, S, D, normalize, gather map).  What each one reaches is listed in the GPU test.
ROPE_CASES = [
    (2, 3, 5, 70, 72, True, True), (2, 2, 3, 40, 24, True, True), (2, 2, 9, 16, 8, True, False), (1, 2, 70, 20, 88, True, False),
    (1, 3, 33, 24, 96, True, True), (2, 2, 40, 33, 128, True, False), (1, 2, 150, 17, 104, False, True), (2, 2, 200, 8, 128, True, True),
    (1, 2, 260, 8, 64, True, False), (2, 2, 6, 210, 128, True, True), (1, 2, 1, 48, 64, True, False), (2, 2, 16, 16, 64, False, True),
]


def rope_case_seed(case):
    return case[2] * 1000 + case[3]


def rope_rotate(x, cos, sin):
    """Wan's rotation of x [B, N, H, D] by the token's angles: consecutive channel pairs (x0, x1) -> (x0 c - x1 s, x0 s + x1 c);
    cos / sin: [N, D/2] tables in any float dtype, taken to the dtype of x (fp32 tables are exact in fp64)."""
    B, N, H, D = x.shape
    xs = x.reshape(B, N, H, D // 2, 2)
    c, s = cos[None, :, None, :].to(x.dtype), sin[None, :, None, :].to(x.dtype)
    return torch.stack((xs[..., 0] * c - xs[..., 1] * s, xs[..., 0] * s + xs[..., 1] * c), dim=-1).reshape(B, N, H, D)


def make_rope_inputs(B, H, M, S, D, dtype, seed=1234, gather=False):
    """Seeded inputs of the rotary block-mix operator: q, k = relu(randn) + 1e-6, v, dO = randn (all in `dtype`), W = rand(M, M),
    fp32 cos / sin tables [N, D/2] of angles uniform in [0, 2 pi), and with `gather` a random permutation as the gather map
    (int32[N]: block-major position -> token row; None otherwise).  Returns q, k, v, W, do, cos, sin, perm."""
    g = torch.Generator().manual_seed(seed)
    N = M * S
    q = (torch.relu(torch.randn(B, N, H, D, generator=g)) + 1e-6).to(dtype)
    k = (torch.relu(torch.randn(B, N, H, D, generator=g)) + 1e-6).to(dtype)
    v = torch.randn(B, N, H, D, generator=g).to(dtype)
    do = torch.randn(B, N, H, D, generator=g).to(dtype)
    W = torch.rand(M, M, generator=g)
    ang = torch.rand(N, D // 2, generator=g) * (2 * torch.pi)
    cos, sin = torch.cos(ang), torch.sin(ang)
    perm = torch.randperm(N, generator=g).int() if gather else None
    return q, k, v, W, do, cos, sin, perm


def rope_blockmix_fp64(q, k, v, W, do, cos, sin, perm=None, normalize=True, eps=1e-6, dtype=torch.float64):
    """The rotary block-mix operator on the given tensors in fp64 (`dtype`: the same function in another precision, to measure
    the reference's own conditioning): the un-rotated q, k are rotated by the tables, everything is gathered to block-major order
    (position p reads token row perm[p]), the oracle's operator runs on the rotated pair with the un-rotated pair as the
    normaliser's, and the result is scattered back to token rows.  Gradients of <out, do> w.r.t. the UN-rotated q, k and v, W by
    autograd (tests/test_rope_ref_cpu.py ties them to the oracle's closed form).  Returns out, dq, dk, dv, dW."""
    t = [x.detach().to(dtype).clone().requires_grad_(True) for x in (q, k, v, W)]
    rows = torch.arange(q.shape[1]) if perm is None else perm.long()
    bm = lambda x: x[:, rows]
    o = orc.blockmix_fwd(bm(rope_rotate(t[0], cos, sin)), bm(rope_rotate(t[1], cos, sin)), bm(t[2]), t[3], eps,
                         bm(t[0]) if normalize else None, bm(t[1]) if normalize else None, normalize)
    (o * bm(do.to(dtype))).sum().backward()
    out = torch.empty_like(o)
    out[:, rows] = o.detach()
    return out, t[0].grad, t[1].grad, t[2].grad, t[3].grad


def mix_extra_checks(got, want, W, S, tols, per_block):
    """What a case with a given W is held to beyond check(): `got`, `want`: name -> tensor, token tensors [B, M * S, H, D] in block-major
    order.  Everything finite; the blocks whose row of W is zero have an exactly zero output, those whose column is zero exactly zero
    dk, dv (and dk_den); with `per_block`, out / dq / dk / dv within their tolerance of every block's own maximum (check_chunks)."""
    for name, g in got.items():
        assert bool(torch.isfinite(g.float()).all()), f"{name}: not finite"
    zr, zc = zero_rows_and_columns(W)
    blocks = lambda t: t.reshape(t.shape[0], W.shape[0], S, *t.shape[2:])
    assert not bool(blocks(got["out"])[:, zr].any()), f"out of blocks {zr} (rows of W that are zero) must be exactly zero"
    for name in ("dk", "dv", "dk_den"):
        if name in got:
            assert not bool(blocks(got[name])[:, zc].any()), f"{name} of blocks {zc} (columns of W that are zero) must be exactly zero"
    if per_block:
        for name in ("out", "dq", "dk", "dv"):
            check_chunks(name, got[name], want[name], tols[0] if name == "out" else tols[1], chunk=S)


def make_mix_rope_case(case):
    """make_rope_inputs of a ROPE_CASES row in fp32 with a "signed" W and the visible eps of its (un-rotated) normaliser pair:
    (q, k, v, W, do, cos, sin, perm), eps."""
    B, H, M, S, D, _, gather = case
    q, k, v, _, do, cos, sin, perm = make_rope_inputs(B, H, M, S, D, torch.float32, seed=rope_case_seed(case), gather=gather)
    W = make_mix_weights("signed", M, torch.Generator().manual_seed(rope_case_seed(case) + 1))
    rows = slice(None) if perm is None else perm.long()
    return (q, k, v, W, do, cos, sin, perm), visible_eps(q[:, rows], k[:, rows], M)


def to_dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


# every comparison of a parity run: (test id, name, dtype of the HIP result, max-normalised error, rms-relative error, tolerance);
# conftest writes the summary to gpurun_out/parity_report.json at the end of a -m gpu session (profiles/ keeps a copy per round)
OBSERVED = []


def check(name, got, want, tol, atol=0.0):
    """rel-err = max|got - want| / max|want| < tol (or max|got - want| < atol for ~zero references); the rms-relative error
    (which, unlike the max-normalised one, sees errors on small-magnitude elements) must stay below the same bound."""
    import os
    g, w = got.float().cpu(), want.float()
    if atol and (g - w).abs().max().item() < atol:
        return 0.0
    e, r = rel_err(g, w), rms_ratio(g, w)
    # error beyond the final rounding of the result to its own dtype (|err| <= u |want| elementwise is what storing the exact
    # result in that dtype costs): what the kernels' internal arithmetic adds, normalised like rel_err
    u = UNIT_ROUNDOFF.get(got.dtype, 0.0)
    x = ((g.double() - w.double()).abs() - u * w.double().abs()).clamp_min(0).max().item() / max(w.double().abs().max().item(), 1e-30)
    OBSERVED.append((os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], name, str(got.dtype).replace("torch.", ""), e, r, tol, x))
    assert e < tol, f"{name}: rel_err {e:.3e} (rms ratio {r:.3e}) exceeds {tol:.1e}"
    if u and tol > u:
        assert x < tol - u, f"{name}: error beyond the final {got.dtype} rounding {x:.3e} exceeds {tol - u:.1e} (rel_err {e:.3e})"
    assert r < 2 * tol, f"{name}: rms ratio {r:.3e} exceeds {2 * tol:.1e} (rel_err {e:.3e})"
    return e


def check_chunks(name, got, want, tol, chunk=64, dim=1):
    """The per-chunk form of check(): for every chunk of `chunk` tokens along `dim` (the ragged last one included) the same three
    assertions, each normalised by THAT chunk's reference -- max|got_c - want_c| / max|want_c| < tol, the error beyond the final
    rounding of the result dtype < tol - u (when tol > u), the chunk's rms ratio < 2 tol.  A chunk whose reference is identically
    zero must be identically zero.  One OBSERVED record: the worst figures over the chunks, named after the chunk of the largest
    error (first word = `name`, so conftest classifies it like check()'s record)."""
    import os
    import torch.nn.functional as F
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    g = got.detach().cpu().double().movedim(dim, 0)
    w = want.detach().cpu().double().movedim(dim, 0)
    T = g.shape[0]
    n = (T + chunk - 1) // chunk
    # [n, chunk * rest]; the padding of the last chunk is zero in both and adds nothing to a maximum or a sum of squares
    g, w = (F.pad(t.reshape(T, -1), (0, 0, 0, n * chunk - T)).reshape(n, -1) for t in (g, w))
    u = UNIT_ROUNDOFF.get(got.dtype, 0.0)
    err = (g - w).abs()
    wmax = w.abs().amax(1)
    zero = wmax == 0
    if bool(zero.any()):
        bad = [int(c) for c in zero.nonzero().flatten() if not torch.equal(g[c], torch.zeros_like(g[c]))]
        assert not bad, f"{name}: chunks {bad[:8]} must be exactly zero (their reference is)"
    den = wmax.masked_fill(zero, 1.0)
    e = err.amax(1) / den
    x = (err - u * w.abs()).clamp_min(0).amax(1) / den
    r = err.square().sum(1).sqrt() / w.square().sum(1).sqrt().masked_fill(zero, 1.0)
    ce, cx, cr = (int(torch.argmax(t)) for t in (e, x, r))
    em, xm, rm = e[ce].item(), x[cx].item(), r[cr].item()
    OBSERVED.append((os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], f"{name} per-chunk (worst: {ce})",
                     str(got.dtype).replace("torch.", ""), em, rm, tol, xm))
    assert em < tol, f"{name}: chunk {ce} of {n}: rel_err {em:.3e} of the chunk's maximum exceeds {tol:.1e}"
    if u and tol > u:
        assert xm < tol - u, f"{name}: chunk {cx} of {n}: error beyond the final {got.dtype} rounding {xm:.3e} of the chunk's maximum exceeds {tol - u:.1e}"
    assert rm < 2 * tol, f"{name}: chunk {cr} of {n}: rms ratio {rm:.3e} exceeds {2 * tol:.1e}"
    return em


def _h16_strips(x):
    """[..., K, V] -> [..., K/16, 16, V/64, 64]: the 16-row strips of the 64 x 64 tiles of a chunk summary."""
    K, V = x.shape[-2:]
    return x.reshape(*x.shape[:-2], K // 16, 16, V // 64, 64)


def _h16_store(x, mult):
    """payload = fp16(x / mult) (round to nearest, fp16 subnormals included), value = payload x mult."""
    m = mult[..., :, None, :, None]
    pay = (_h16_strips(x) / m).to(torch.float16).double()
    return (pay * m).reshape(x.shape)


def _h16_measured(x):
    """Producer of a whole strip (S, dP): m = 2^(floor(log2 max|strip|) - 14), payload maximum in [2^14, 2^15); (stored value, m)."""
    amax = _h16_strips(x).abs().amax((-3, -1))                        # [..., K/16, V/64]
    mult = torch.where(amax > 0, torch.exp2(torch.floor(torch.log2(amax.clamp_min(1e-300))) - 14), torch.ones_like(amax))
    return _h16_store(x, mult), mult


def _h16_mixed(w, x, mult):
    """Mixing kernel (out_i = sum_j w_ij x_j): x, mult are the stored inputs [B, H, n, ...] and their strip multipliers; the output
    strip's multiplier is the power of two >= beta_i = sum_j |w_ij| mult_j (a bound every workgroup computes alike), payload
    bound 2^15 beta_i; a row without terms stores zero."""
    y = torch.einsum("ij,bhjkv->bhikv", w, x)
    beta = torch.einsum("ij,bhjsc->bhisc", w.abs(), mult)
    mo = torch.where(beta > 0, torch.exp2(torch.ceil(torch.log2(beta.clamp_min(1e-300)))), torch.ones_like(beta))
    return _h16_store(y, mo)


def causal_fp64(q, k, v, mix, do, scale=None, chunk=64, h16=False):
    """The causal operator and its closed-form gradients (oracle causal_fwd / causal_bwd) in fp64 on the given tensors; with
    `h16` the chunk summaries S, P, dP, dS pass through the 2-byte storage format of DESIGN.md section 3e (fp16 payload x one
    power-of-two multiplier per 16-row strip of a 64 x 64 chunk tile; K and V multiples of 64) and everything else stays fp64:
    the model CAUSAL_CHUNK_TOL_H16 is derived from.  Returns out, dq, dk, dv [B, T, H, .] and dmix [n, n], unrounded."""
    import torch.nn.functional as F
    qf, kf, vf, dof = (t.permute(0, 2, 1, 3).double() for t in (q, k, v, do))
    B, H, T, K = qf.shape
    scale = K ** -0.5 if scale is None else scale
    C = chunk
    n = (T + C - 1) // C
    m = mix.reshape(mix.shape[0], mix.shape[1]).double()[:n, :n]
    qc, kc, vc, doc = (F.pad(t, (0, 0, 0, n * C - T)).reshape(B, H, n, C, t.shape[-1]) for t in (qf, kf, vf, dof))
    qs = qc * scale
    tril = torch.tril(torch.ones(C, C, dtype=torch.float64))
    ms, md = torch.tril(m, diagonal=-1), torch.diagonal(m).view(1, 1, n, 1, 1)
    S = torch.matmul(kc.transpose(-1, -2), vc)
    dP = torch.matmul(qs.transpose(-1, -2), doc)
    if h16:
        (S, mS), (dP, mdP) = _h16_measured(S), _h16_measured(dP)
        P, dS = _h16_mixed(ms, S, mS), _h16_mixed(ms.t().contiguous(), dP, mdP)
    else:
        P, dS = torch.einsum("ij,bhjkv->bhikv", ms, S), torch.einsum("ij,bhikv->bhjkv", ms, dP)
    A = torch.matmul(qs, kc.transpose(-1, -2)) * tril
    dA = torch.matmul(doc, vc.transpose(-1, -2)) * tril
    o = torch.matmul(qs, P) + md * torch.matmul(A, vc)
    dQ = (torch.matmul(doc, P.transpose(-1, -2)) + md * torch.matmul(dA, kc)) * scale
    dK = torch.matmul(vc, dS.transpose(-1, -2)) + md * torch.matmul(dA.transpose(-1, -2), qs)
    dV = torch.matmul(kc, dS) + md * torch.matmul(A.transpose(-1, -2), doc)
    dm = torch.tril(torch.einsum("bhikv,bhjkv->ij", dP, S), diagonal=-1) + torch.diag(torch.einsum("bhicv,bhicv->i", doc, torch.matmul(A, vc)))
    back = lambda t: t.reshape(B, H, n * C, -1).permute(0, 2, 1, 3)[:, :T]
    return {"out": back(o), "dq": back(dQ), "dk": back(dK), "dv": back(dV), "dmix": dm}


def chunk_errors(got, want, chunk=64, dim=1):
    """(max over the chunks of max|got_c - want_c| / max|want_c|, the same ratio over the whole tensor): what the model is measured in."""
    g, w = got.double().movedim(dim, 0), want.double().movedim(dim, 0)
    per = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(g.split(chunk), w.split(chunk)) if float(b.abs().max()) > 0)
    return per, ((g - w).abs().max() / w.abs().max()).item()


def _fla_layer(**kw):
    """The fla layer the decoding tests share: hidden 256, 2 heads (K = 64, V = 128), exact_decoding, seeded norm weight and mixing matrix."""
    from mhla_amd import modules
    torch.manual_seed(3)
    m = modules.MHLA(mode="chunk", hidden_size=256, expand_k=0.5, expand_v=1.0, num_heads=2, feature_map="relu", norm_eps=1e-6,
                     layer_idx=0, exact_decoding=True, **kw)
    with torch.no_grad():
        (m.g_norm_swish_gate if m.fuse_norm_and_gate else m.g_norm).weight.uniform_(0.5, 1.5)
        m.mixing_matrix.copy_(torch.rand(32, 32).view(32, 32, 1, 1, 1, 1))
    return m


def launches(fn):
    """Kernel launches of the library while `fn` runs: {name: count} (mhla_prof_*)."""
    from mhla_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 14)
    torch.cuda.synchronize()
    lib.mhla_prof_report(buf, len(buf))   # (clears records an earlier user may have left)
    lib.mhla_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.mhla_prof_enable(0)
        lib.mhla_prof_report(buf, len(buf))
    return {ln.rsplit(" ", 2)[0]: int(ln.rsplit(" ", 2)[1]) for ln in buf.value.decode().splitlines() if ln.strip()}


def poison():
    """Fill ~350 MB of device memory with NaN and free it again: the next torch.empty() calls of the ops (workspaces,
    outputs, gradients) start as NaN, and the registers of idle CUs hold NaN -- reads of memory or registers that were never
    written show up as NaN in the parity checks."""
    slabs = [torch.full((n,), float("nan"), dtype=torch.float32, device=DEV) for n in (1 << 26, 1 << 24, 1 << 22, 1 << 20)]
    del slabs
