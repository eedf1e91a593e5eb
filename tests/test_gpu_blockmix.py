"""GPU parity: block-mixing MHLA operator (HIP, through the C ABI) vs the CPU oracle and the golden fixtures."""
import pytest
import torch

from conftest import load_golden
from gpu_util import (poison, DEV, GTOL, TOL, DW_TOL, GTOL_BF16SUM, TOL_BF16SUM, bm_tols, bm_tols_signed, check, check_dw_rows, make_blockmix_inputs,
                      mix_conditioning, mix_extra_checks, oracle_blockmix, to_dev)
from oracle import mhla_oracle as orc

pytestmark = pytest.mark.gpu


def run_case(B, H, M, S, D, dtype, normalize=True, split=False, w="linear", idx=None, seed=1234, summaries="tf32", W=None, eps=1e-6,
             per_block=False, **opkw):
    """One forward + backward through mhla_amd.mhla_blockmix against the oracle.  summaries="tf32" (the library's default: block
    summaries stored with 11 significand bits where the kernels have the 2-byte format, >= 16 elsewhere) and "split" (>= 16 bits
    everywhere): the reference's arithmetic on the given tensors, held to one final rounding + 1e-3 (1e-3 for the fp32-stored dW);
    "bf16": the opt-in reduced-precision form (single-bf16 summaries / intermediates) at its (1 + K) u bounds.
    W (a mixing matrix in place of the seeded one: gpu_util.make_mix_weights), eps and per_block (out, dq, dk, dv additionally held to
    the tolerance block by block) serve tests/test_gpu_blockmix_weights.py: with a W given, dW is checked in two pieces (the rows of W
    that are zero, the others), everything must be finite, a block whose row of W is zero must have an exactly zero output and one
    whose column is zero exactly zero dk, dv, and a normalised "bf16" case with negative weights takes bm_tols_signed's bound.
    Returns the results by name, in block-major token order."""
    import mhla_amd
    otol, gtol, wtol = bm_tols(dtype, summaries)
    q, k, v, W0, do, qd, kd = make_blockmix_inputs(B, H, M, S, D, dtype, seed, w, split)
    given = W is not None
    if not given:
        W = W0
    elif normalize and bool((W < 0).any()):
        otol, gtol, wtol = bm_tols_signed(dtype, summaries, mix_conditioning(q, k, v, W, do, eps, qd, kd)["kappa_n"])
    want, wg = oracle_blockmix(q, k, v, W, do, qd, kd, eps, normalize)
    if idx is not None:   # scatter tokens so that block-major position p lives at row idx[p]
        def scat(t):
            if t is None:
                return None
            r = torch.empty_like(t)
            r[:, idx.long()] = t
            return r
        q, k, v, do, qd, kd = (scat(t) for t in (q, k, v, do, qd, kd))
    dq_, dk_, dv_, dW_, ddo, dqd, dkd = to_dev(q, k, v, W, do, qd, kd)
    leaves = [t.requires_grad_(True) for t in (dq_, dk_, dv_, dW_)]
    if split:
        dqd.requires_grad_(True)
        dkd.requires_grad_(True)
    poison()
    out = mhla_amd.mhla_blockmix(dq_, dk_, dv_, dW_, eps=eps, q_den=dqd, k_den=dkd, normalize=normalize,
                                 block_index=None if idx is None else idx.to(DEV), summaries=summaries, **opkw)
    poison()
    out.backward(ddo)
    torch.cuda.synchronize()

    def gather(t):
        return t if idx is None else t[:, idx.long().to(t.device)]
    check("out", gather(out), want, otol)
    check("dq", gather(leaves[0].grad), wg["dq"], gtol)
    check("dk", gather(leaves[1].grad), wg["dk"], gtol)
    check("dv", gather(leaves[2].grad), wg["dv"], gtol)
    if given:
        check_dw_rows(leaves[3].grad, wg["dW"], W, wtol)
    else:
        # M == 1: the output does not depend on W (numerator and normaliser scale together), dW ~ 0
        check("dW", leaves[3].grad, wg["dW"], wtol, atol=(1e9 if dtype != torch.float32 else 1e-3) if M == 1 else 0.0)
    got = {"out": gather(out.detach()), "dq": gather(leaves[0].grad), "dk": gather(leaves[1].grad), "dv": gather(leaves[2].grad), "dW": leaves[3].grad}
    if split and normalize:
        check("dq_den", gather(dqd.grad), wg["dq_den"], gtol)
        check("dk_den", gather(dkd.grad), wg["dk_den"], gtol)
        got.update(dq_den=gather(dqd.grad), dk_den=gather(dkd.grad))
    if given or per_block:
        mix_extra_checks(got, dict(wg, out=want), W, S, (otol, gtol, wtol), per_block)
    return got


@pytest.mark.parametrize("tag", ["dit_a", "dit_b", "vit_a"])
def test_golden_op(tag):
    import mhla_amd
    g = load_golden("blockmix2d_" + tag)
    q, k, v, W, do = (g[n].to(DEV) for n in ("q", "k", "v", "W", "dout"))
    for t in (q, k, v, W):
        t.requires_grad_(True)
    out = mhla_amd.mhla_blockmix(q, k, v, W, eps=1e-6)
    out.backward(do)
    check("out", out, g["out"], 1e-4)
    for n, t in (("dq", q), ("dk", k), ("dv", v), ("dW", W)):
        check(n, t.grad, g[n], 2e-4)


def test_golden_bf16_fixture_default_arithmetic():
    """`dit_c` (verdict r4 item 1): the reference module's operator evaluated in fp32 on bf16-rounded q, k, v, dO.  The library's default
    arithmetic on those bf16 tensors meets it within one final rounding + 1e-3 (dW, fp32-stored: 1e-3) -- and is closer to it than the
    reference module itself when that is run in bf16; the opt-in bf16 summaries are held to their own bound."""
    import mhla_amd
    g = load_golden("blockmix2d_dit_c")
    u = 2.0 ** -8
    for summ, otol, gtol, wtol in (("split", u + 1e-3, u + 1e-3, 1e-3), ("bf16", 2 * u, 3 * u, 3 * u)):
        q, k, v, do = (g[n].to(DEV).bfloat16() for n in ("q", "k", "v", "dout"))
        W = g["W"].to(DEV)
        for t in (q, k, v, W):
            t.requires_grad_(True)
        out = mhla_amd.mhla_blockmix(q, k, v, W, eps=1e-6, summaries=summ)
        out.backward(do)
        check("out", out, g["out"], otol)
        for n, t in (("dq", q), ("dk", k), ("dv", v)):
            check(n, t.grad, g[n], gtol)
        check("dW", W.grad, g["dW"], wtol)
        if summ == "split":
            ours = (out.float().cpu() - g["out"]).abs().max() / g["out"].abs().max()
            theirs = (g["out_reference_module_in_bf16"] - g["out"]).abs().max() / g["out"].abs().max()
            assert ours < theirs, (float(ours), float(theirs))


@pytest.mark.parametrize("M,S,D", [(16, 16, 64), (16, 16, 72), (4, 49, 64), (9, 49, 72), (64, 64, 64), (1, 64, 32),
                                   (16, 256, 64), (150, 14, 128), (6, 210, 128), (25, 20, 96), (4, 16, 16)])
def test_shapes_fp32(M, S, D):
    run_case(2, 2, M, S, D, torch.float32, w="rand")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,S,D", [(16, 16, 72), (64, 64, 64), (6, 210, 128)])
def test_shapes_lowp(M, S, D, dtype):
    run_case(2, 2, M, S, D, dtype)


@pytest.mark.parametrize("M,S", [(64, 64), (16, 16), (16, 256), (4, 49), (5, 64), (33, 32), (40, 80), (1, 128), (64, 8),
                                 (3, 320), (5, 200), (17, 136)])   # blocks of 5 / 4 (ragged) / 3 chunks: chunk parts over several workgroups
@pytest.mark.parametrize("summaries", ["tf32", "split", "bf16"])
def test_fast_path_bf16_d64(M, S, summaries):
    """bf16, D = 64, M <= 64.  summaries="bf16": the bf16-MFMA fast path (interleaved bf16 block summaries, fused mix + output);
    default: the same shapes at the reference's arithmetic (fp32 summaries, hi + lo operands)."""
    run_case(2, 3, M, S, 64, torch.bfloat16, w="rand", summaries=summaries)


@pytest.mark.parametrize("M,D", [(16, 64), (16, 72), (9, 72), (4, 80), (1, 64), (13, 24), (16, 8)])
@pytest.mark.parametrize("summaries", ["split", "bf16"])
def test_small_sequence_path(M, D, summaries):
    """bf16, S = 16, M <= 16, D <= 80 (DiT / ViT regime): single-launch attention-form kernels (smalln.hpp), with hi + lo score
    tiles (default) and with single-bf16 ones (opt-in)."""
    run_case(3, 2, M, 16, D, torch.bfloat16, w="rand", summaries=summaries)
    run_case(2, 2, M, 16, D, torch.bfloat16, normalize=False, summaries=summaries)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_full_size_c3_dit_xl2_every_head(dtype):
    """BASELINE.json configs[2] at its full per-GPU size -- B = 32, N = 256 (16 blocks of 16), H = 16, D = 72 -- the north-star
    shape: the output and every gradient of all 512 (b, h) pairs and the full dW against the oracle.  bf16: the single-launch
    small-sequence kernels on the benchmarked grid of 512 workgroups (their (b, h) comes from xcd_swizzle(blockIdx, gridDim));
    fp32 (how the reference trains DiT-XL, mhla_dit/train.py:12-13): the split-operand path."""
    run_case(32, 16, 16, 16, 72, dtype, w="rand")


def test_small_sequence_grid_not_a_multiple_of_8():
    """B H = 231 workgroups (33 x 7): the XCD-aware (b, h) mapping with a remainder, values checked against the oracle."""
    run_case(33, 7, 16, 16, 72, torch.bfloat16, w="rand")
    run_case(33, 7, 16, 16, 64, torch.bfloat16, w="rand", normalize=False)
    run_case(33, 7, 16, 16, 72, torch.bfloat16, w="rand", summaries="bf16")


def test_c1_shape_dit_s2_on_the_gpu():
    """BASELINE.json configs[0]'s operator shape (DiT-S/2 256x256: B = 1, 6 heads of 64, 16 blocks of 16 tokens; a CPU plumbing
    configuration in the reference) launched on the GPU as well: six workgroups, fp32 (how the configuration runs) and bf16."""
    run_case(1, 6, 16, 16, 64, torch.float32)
    run_case(1, 6, 16, 16, 64, torch.bfloat16)
    run_case(1, 6, 16, 16, 64, torch.bfloat16, summaries="bf16")


@pytest.mark.parametrize("M,D", [(16, 64), (16, 72), (9, 72), (4, 80), (1, 64), (13, 24), (16, 8)])
def test_small_sequence_path_fp32(M, D):
    """fp32 tensors, S = 16, M <= 16, D <= 80: the attention-form kernels with hi + lo bf16 operands (smalln_f32.hpp), held to
    the fp32 tolerance; with and without the normaliser, and with the relu + eps prologue."""
    run_case(3, 2, M, 16, D, torch.float32, w="rand")
    run_case(2, 2, M, 16, D, torch.float32, normalize=False)


def test_small_sequence_fp32_vs_split_path_agree():
    import mhla_amd
    q, k, v, W, do, _, _ = make_blockmix_inputs(4, 6, 16, 16, 72, torch.float32, seed=3, w="rand")
    res = []
    for ns in (False, True):
        t = [x.clone().requires_grad_(True) for x in to_dev(q, k, v, W)]
        out = mhla_amd.mhla_blockmix(*t, no_smalln=ns)
        out.backward(do.to(DEV))
        res.append([out] + [x.grad for x in t])
    for name, a_, b_ in zip(("out", "dq", "dk", "dv", "dW"), res[0], res[1]):
        check(name, a_, b_.float().cpu(), 2e-4)


@pytest.mark.parametrize("summaries,tol", [("split", 2 * 2.0 ** -8 + 1e-3), ("bf16", 1.2e-2)])
def test_small_sequence_vs_summary_path_agree(summaries, tol):
    """(two bf16-rounded results of the same exact value differ by up to one ulp = 2 u)"""
    import mhla_amd
    q, k, v, W, do, _, _ = make_blockmix_inputs(4, 6, 16, 16, 64, torch.bfloat16, seed=3, w="rand")
    res = []
    for ns in (False, True):
        t = [x.clone().requires_grad_(True) for x in to_dev(q, k, v, W)]
        out = mhla_amd.mhla_blockmix(*t, no_smalln=ns, summaries=summaries)
        out.backward(do.to(DEV))
        res.append([out] + [x.grad for x in t])
    for name, a_, b_ in zip(("out", "dq", "dk", "dv", "dW"), res[0], res[1]):
        check(name, a_, b_.float().cpu(), tol if name != "dW" or summaries == "bf16" else 1e-3)


@pytest.mark.parametrize("summaries", ["tf32", "split", "bf16"])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("M,S", [(16, 32), (9, 64), (20, 40)])
def test_fast_path_gather_map(M, S, normalize, summaries):
    """The bf16 D = 64 summaries / tile kernels with a gather map (the k_fs_state1c<.., IDX> instantiations read the map's rows up
    front): shapes that are not the small-sequence path's (S != 16), a random token permutation, a short last block group (M = 9, 20)."""
    idx = torch.randperm(M * S, generator=torch.Generator().manual_seed(M * 100 + S)).int()
    run_case(2, 3, M, S, 64, torch.bfloat16, normalize=normalize, idx=idx, w="rand", summaries=summaries)


@pytest.mark.parametrize("normalize", [True, False])
def test_fast_path_options(normalize):
    idx = orc.block_index_2d(4, 4).int()
    run_case(2, 2, 16, 16, 64, torch.bfloat16, normalize=normalize, idx=idx)
    run_case(2, 2, 16, 16, 64, torch.bfloat16, normalize=normalize, idx=idx, summaries="bf16")
    run_case(1, 2, 64, 64, 64, torch.bfloat16, normalize=normalize, force_generic=True)   # same shape, generic kernels


@pytest.mark.parametrize("summaries,tol", [("split", 2 * 2.0 ** -8 + 1e-3), ("bf16", 1.2e-2)])
def test_fast_vs_generic_agree(summaries, tol):
    """The D = 64 bf16 shape on the kernels the dispatcher picks (split-operand path at the default arithmetic, the bf16-summary
    fast path with summaries="bf16") against the exact fp32-MFMA kernels."""
    import mhla_amd
    q, k, v, W, do, _, _ = make_blockmix_inputs(2, 4, 64, 64, 64, torch.bfloat16, seed=5, w="rand")
    res = []
    for fg in (False, True):
        t = [x.clone().requires_grad_(True) for x in to_dev(q, k, v, W)]
        out = mhla_amd.mhla_blockmix(*t, force_generic=fg, summaries=summaries)
        out.backward(do.to(DEV))
        res.append([out] + [x.grad for x in t])
    for name, a, b in zip(("out", "dq", "dk", "dv", "dW"), res[0], res[1]):
        check(name, a, b.float().cpu(), tol if name != "dW" or summaries == "bf16" else 1e-3)


@pytest.mark.parametrize("normalize,split", [(False, False), (True, True)])
@pytest.mark.parametrize("M,S,D", [(16, 16, 64), (24, 8, 128)])
def test_wan_modes(M, S, D, normalize, split):
    run_case(1, 3, M, S, D, torch.float32, normalize=normalize, split=split, w="rand")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,S,D,split", [(150, 21, 128, True), (70, 50, 64, False), (9, 210, 128, True), (3, 33, 64, True),
                                          (65, 16, 128, False), (16, 64, 72, False), (5, 37, 80, True), (7, 20, 96, False),
                                          (4, 50, 40, True), (3, 19, 8, False), (6, 45, 104, True), (5, 23, 24, True), (4, 31, 56, False),
                                          (3, 40, 88, True), (2, 33, 120, False), (40, 24, 64, False), (200, 8, 64, True)])
def test_split_operand_path(M, S, D, split, dtype):
    """Head dims that are multiples of 8, outside the bf16 fast paths: forward and backward on the split-bf16 MFMA
    kernels (split.hpp), including the zero-padded tile shapes (D = 72, 80, 104 ...).  33 .. 256 blocks run the resident-sequence
    mixing kernel: M = 40, 65 / 70, 150, 200 instantiate its 4-, 8-, 12- and 16-wave variants (fp32 summaries; bf16 tensors also
    with the opt-in bf16 summaries)."""
    run_case(1, 2, M, S, D, dtype, split=split, w="rand", seed=M + S)
    if dtype == torch.bfloat16:
        run_case(1, 2, M, S, D, dtype, split=split, w="rand", seed=M + S, summaries="bf16")


@pytest.mark.parametrize("summaries", ["split", "bf16"])
def test_c2_variant_256_blocks_of_16(summaries):
    """SURVEY 8(d) C2 variant (M, S) = (256, 16): bf16, D = 64, more than 64 blocks -> split-operand path (fp32 summaries by
    default; summaries="bf16": the wave-per-block kernels with bf16 summaries)."""
    run_case(1, 2, 256, 16, 64, torch.bfloat16, w="rand", summaries=summaries)


@pytest.mark.parametrize("M,normalize,gather", [(65, True, False), (130, False, False), (203, True, True), (256, True, True), (77, False, True)])
def test_blocks_of_16_tokens_wave_per_block_kernels(M, normalize, gather):
    """bf16, D = 64, S = 16, more than 64 blocks, summaries="bf16": the wave-per-block token kernels (split16.hpp) and the
    whole-matrix dW kernel (M not a multiple of the 4 blocks of a workgroup, with and without the normaliser, with a gather map);
    the same shapes at the default arithmetic."""
    idx = torch.randperm(M * 16, generator=torch.Generator().manual_seed(M)).int() if gather else None
    run_case(2, 3, M, 16, 64, torch.bfloat16, normalize=normalize, w="rand", idx=idx, seed=M, summaries="bf16")
    run_case(2, 3, M, 16, 64, torch.bfloat16, normalize=normalize, w="rand", idx=idx, seed=M)


def test_blocks_of_16_tokens_views_into_a_packed_projection():
    """The same kernels on strided views (q, k, v slices of one [B, N, 3, H, D] projection output) and a non-contiguous dout."""
    import mhla_amd
    B, H, M, S, D = 2, 4, 96, 16, 64
    q, k, v, W, do, _, _ = make_blockmix_inputs(B, H, M, S, D, torch.bfloat16, 5, "rand", False)
    want, wg = oracle_blockmix(q, k, v, W, do, None, None, 1e-6, True)
    qkv = torch.stack([q, k, v], dim=2).to(DEV).requires_grad_(True)
    Wd = W.to(DEV).requires_grad_(True)
    out = mhla_amd.mhla_blockmix(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], Wd, eps=1e-6)
    out.backward(do.to(DEV))
    check("out", out, want, TOL[torch.bfloat16])
    for i, name in enumerate(("dq", "dk", "dv")):
        check(name, qkv.grad[:, :, i], wg[name], GTOL[torch.bfloat16])
    check("dW", Wd.grad, wg["dW"], DW_TOL[torch.bfloat16])


@pytest.mark.parametrize("D,grid", [(72, (4, 4)), (128, (4, 4)), (64, (8, 10))])
def test_split_operand_path_relu_prologue(D, grid):
    """relu(x) + eps folded into the loads (mhla_dit/mhla/mhla.py:229-230) and its gradient mask, split path."""
    import mhla_amd
    g = torch.Generator().manual_seed(D)
    B, H, M, S = 2, 2, grid[0] * grid[1], (40 if grid == (4, 4) else 16)   # 80 blocks of 16 at D = 64: the wave-per-block kernels
    q0, k0, v, do = (torch.randn(B, M * S, H, D, generator=g).bfloat16() for _ in range(4))
    W = orc.block_distance_weights(grid, "linear")
    qf, kf = (orc.relu_eps(t.float(), 1e-6) for t in (q0, k0))
    want = orc.blockmix_fwd(qf, kf, v.float(), W, 1e-6)
    leaves = [t.to(DEV).requires_grad_(True) for t in (q0, k0, v)]
    Wd = W.to(DEV).requires_grad_(True)
    out = mhla_amd.mhla_blockmix(*leaves, Wd, eps=1e-6, relu_eps=True)
    out.backward(do.to(DEV))
    check("out", out, want, TOL[torch.bfloat16])
    qa, ka, va = (t.float().requires_grad_(True) for t in (q0, k0, v))
    Wa = W.clone().requires_grad_(True)
    ref = orc.blockmix_fwd(torch.relu(qa) + 1e-6, torch.relu(ka) + 1e-6, va, Wa, 1e-6)
    ref.backward(do.float())
    for name, got, ex in zip(("dq", "dk", "dv", "dW"), [t.grad for t in leaves] + [Wd.grad], (qa.grad, ka.grad, va.grad, Wa.grad)):
        check(name, got, ex, DW_TOL[torch.bfloat16] if name == "dW" else GTOL[torch.bfloat16])


def test_split_operand_path_matches_exact_fp32():
    """fp32 tensors: hi/lo bf16 operands keep 16 mantissa bits -> agreement with the exact fp32-MFMA kernels ~1e-5."""
    import mhla_amd
    q, k, v, W, do, qd, kd = make_blockmix_inputs(1, 3, 40, 100, 128, torch.float32, seed=11, w="rand", split=True)
    idx = torch.randperm(40 * 100, generator=torch.Generator().manual_seed(3)).int()
    t = to_dev(q, k, v, W, qd, kd)
    outs = [mhla_amd.mhla_blockmix(t[0], t[1], t[2], t[3], q_den=t[4], k_den=t[5], block_index=idx.to(DEV), force_generic=fg)
            for fg in (False, True)]
    check("out", outs[0], outs[1].cpu(), 1e-4)
    assert (outs[0] != outs[1]).any(), "force_generic selected the same kernels"
    grads = []
    do = torch.randn(outs[0].shape, generator=torch.Generator().manual_seed(4)).to(DEV)
    for fg in (False, True):
        leaves = [x.clone().requires_grad_(True) for x in t]
        o = mhla_amd.mhla_blockmix(leaves[0], leaves[1], leaves[2], leaves[3], q_den=leaves[4], k_den=leaves[5],
                                   block_index=idx.to(DEV), force_generic=fg)
        o.backward(do)
        grads.append([x.grad for x in leaves])
    for name, a, b in zip(("dq", "dk", "dv", "dW", "dq_den", "dk_den"), grads[0], grads[1]):
        check(name, a, b.cpu(), 2e-4)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,S,D,normalize", [(64, 64, 64, True), (33, 20, 64, True), (128, 8, 64, True), (50, 37, 56, True), (100, 12, 32, False),
                                              (64, 16, 64, True), (70, 50, 64, False)])
def test_24_bit_summaries_vs_fp32_summaries(M, S, D, normalize, dtype, monkeypatch):
    """16-bit tensors, 33 .. 128 blocks, D <= 64: the three storage formats of the block summaries on the resident-mixing pipeline --
    h16 (summaries="tf32", the default: fp16 payload x row multiplier, 11 significand bits; blocks of >= 16 tokens), 24-bit floats
    (summaries="split") and fp32 words (the process option "fp32_summaries").  All meet the oracle at the default tolerance; the two
    16-bit-grade forms agree with each other far inside it, h16 stays within 1e-3 (+ a rounding step of the output) of them."""
    import mhla_amd
    from mhla_amd import ops
    monkeypatch.setattr(ops, "_native_nodes", lambda: False)   # the Python autograd nodes: their workspace plans are cached per shape and
    res = {}                                                    # flags -- set_option drops the plans when the process-wide format changes
    try:
        for form, summ, fp32 in (("h16", "tf32", 0), ("p24", "split", 0), ("fp32", "split", 1)):
            mhla_amd.set_option("fp32_summaries", fp32)
            run_case(2, 3, M, S, D, dtype, normalize=normalize, w="rand", summaries=summ)
            q, k, v, W, do, _, _ = make_blockmix_inputs(2, 3, M, S, D, dtype, 77, "rand", False)
            t = [x.requires_grad_(True) for x in to_dev(q, k, v, W)]
            out = mhla_amd.mhla_blockmix(t[0], t[1], t[2], t[3], normalize=normalize, summaries=summ)
            out.backward(do.to(DEV))
            res[form] = [out.detach()] + [x.grad for x in t]
    finally:
        mhla_amd.set_option("fp32_summaries", 0)
    for name, a, b, c in zip(("out", "dq", "dk", "dv", "dW"), res["h16"], res["p24"], res["fp32"]):
        check(name + " (p24 vs fp32)", b, c.cpu(), 2.0 ** -7 if name != "dW" else 2e-4)   # (16-bit results: at most a rounding step of the output apart)
        check(name + " (h16 vs fp32)", a, c.cpu(), 2.0 ** -7 + 1e-3 if name != "dW" else 1e-3)


@pytest.mark.parametrize("summaries", ["tf32", "split"])
def test_24_bit_summaries_kept_state_and_gather_map(monkeypatch, summaries):
    """The forward's kept workspace (h16 / 24-bit KV, G) feeds the backward bit-identically to a recompute, through a gather map too."""
    import mhla_amd
    from mhla_amd import ops
    B, H, M, S, D = 1, 4, 40, 24, 64
    q, k, v, W, do, _, _ = make_blockmix_inputs(B, H, M, S, D, torch.bfloat16, seed=5, w="rand", split=False)
    idx = torch.randperm(M * S, generator=torch.Generator().manual_seed(1)).int()
    run_case(B, H, M, S, D, torch.bfloat16, w="rand", idx=idx, summaries=summaries)
    res = []
    for limit in (1 << 30, 0):
        monkeypatch.setattr(ops, "KEEP_STATE_LIMIT_BYTES", limit)
        t = [x.clone().requires_grad_(True) for x in to_dev(q, k, v, W)]
        mhla_amd.mhla_blockmix(t[0], t[1], t[2], t[3], summaries=summaries).backward(do.to(DEV))
        res.append([x.grad for x in t])
    for name, a, b in zip(("dq", "dk", "dv", "dW"), *res):
        assert torch.equal(a, b), name


def test_split_path_kept_summaries_match_recompute(monkeypatch):
    """Backward with the forward's workspace kept (KV, G, z, ksum, 1/n reused) == backward that recomputes them."""
    import mhla_amd
    from mhla_amd import ops
    q, k, v, W, do, qd, kd = make_blockmix_inputs(1, 2, 20, 40, 128, torch.float32, seed=3, w="rand", split=True)
    res = []
    for limit in (1 << 30, 0):
        monkeypatch.setattr(ops, "KEEP_STATE_LIMIT_BYTES", limit)
        t = [x.clone().requires_grad_(True) for x in to_dev(q, k, v, W, qd, kd)]
        mhla_amd.mhla_blockmix(t[0], t[1], t[2], t[3], q_den=t[4], k_den=t[5]).backward(do.to(DEV))
        res.append([x.grad for x in t])
    for name, a, b in zip(("dq", "dk", "dv", "dW", "dq_den", "dk_den"), *res):
        assert torch.equal(a, b), name


def test_block_index_gather():
    idx = orc.block_index_3d((4, 6, 8), (2, 3, 4)).int()
    run_case(1, 2, 24, 8, 64, torch.float32, split=True, idx=idx)
    idx2 = orc.block_index_2d(4, 4).int()
    run_case(2, 1, 16, 16, 72, torch.bfloat16, idx=idx2)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_golden_wan_op(tag):
    import mhla_amd
    g = load_golden("wan_" + tag)
    B, H, D, M, S, fb, hb, wb, F_, H_, W_, normalize, gated = [int(x) for x in g["meta"]]
    idx = orc.block_index_3d((F_, H_, W_), (fb, hb, wb)).int().to(DEV)
    qr, kr, v, q, k, W, do = (g[n].to(DEV).requires_grad_(True) for n in ("q_rope", "k_rope", "v", "q", "k", "W", "dout"))
    if normalize:
        out = mhla_amd.mhla_blockmix(qr, kr, v, W, eps=1e-6, q_den=q, k_den=k, block_index=idx)
    else:
        out = mhla_amd.mhla_blockmix(qr, kr, v, W, eps=1e-6, normalize=False, block_index=idx)
    out.backward(do.detach())
    check("out", out, g["out"], 1e-4)
    check("dq_rope", qr.grad, g["dq_rope"], 2e-4)
    check("dk_rope", kr.grad, g["dk_rope"], 2e-4)
    check("dv", v.grad, g["dv"], 2e-4)
    check("dW", W.grad, g["dW"], 2e-4)


def test_fused_qkv_views_and_relu_prologue():
    """q, k, v read in place from a fused [B, N, 3, H, D] projection output; relu(x)+eps applied in-kernel."""
    import mhla_amd
    B, N, H, D, M = 2, 256, 4, 72, 16
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(B, N, 3, H, D, generator=g)
    W = orc.block_distance_weights((4, 4), "linear")
    do = torch.randn(B, N, H, D, generator=g)
    ref = qkv.clone().requires_grad_(True)
    Wr = W.clone().requires_grad_(True)
    o_ref = orc.blockmix_fwd(orc.relu_eps(ref[:, :, 0]), orc.relu_eps(ref[:, :, 1]), ref[:, :, 2], Wr, 1e-6)
    (o_ref * do).sum().backward()
    dev = qkv.to(DEV).requires_grad_(True)
    Wd = W.to(DEV).requires_grad_(True)
    out = mhla_amd.mhla_blockmix(dev[:, :, 0], dev[:, :, 1], dev[:, :, 2], Wd, eps=1e-6, relu_eps=True)
    out.backward(do.to(DEV))
    check("out", out, o_ref.detach(), 1e-4)
    check("dqkv", dev.grad, ref.grad, 2e-4)
    check("dW", Wd.grad, Wr.grad, 2e-4)
    # same through the bf16 fast path (D = 64)
    B, N, H, D, M = 2, 256, 4, 64, 16
    qkv = torch.randn(B, N, 3, H, D, generator=g).bfloat16()
    do = torch.randn(B, N, H, D, generator=g).bfloat16()
    ref = qkv.float().requires_grad_(True)
    Wr = W.clone().requires_grad_(True)
    o_ref = orc.blockmix_fwd(orc.relu_eps(ref[:, :, 0]), orc.relu_eps(ref[:, :, 1]), ref[:, :, 2], Wr, 1e-6)
    (o_ref * do.float()).sum().backward()
    dev = qkv.to(DEV).requires_grad_(True)
    Wd = W.to(DEV).requires_grad_(True)
    out = mhla_amd.mhla_blockmix(dev[:, :, 0], dev[:, :, 1], dev[:, :, 2], Wd, eps=1e-6, relu_eps=True)
    out.backward(do.to(DEV))
    check("out_bf16", out, o_ref.detach(), TOL[torch.bfloat16])
    check("dqkv_bf16", dev.grad, ref.grad, GTOL[torch.bfloat16])
    check("dW_bf16", Wd.grad, Wr.grad, DW_TOL[torch.bfloat16])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,S,D,normalize,split,gather", [(16, 16, 256, True, False, False), (9, 20, 192, True, True, True), (33, 12, 160, False, False, False),
                                                           (4, 49, 144, True, False, True),
                                                           # no divisor among the kernels' head dims: zero-padded slices (136 = 2 x 72 - 8, 184 = 2 x 96 - 8)
                                                           (6, 20, 136, True, False, False), (5, 16, 184, True, True, True)])
def test_head_dims_above_128_compose_from_slices(M, S, D, normalize, split, gather, dtype):
    """dim_head > 128 (the reference module takes any, mhla_dit/mhla/mhla.py:155-158): (D / c)^2 un-normalised calls on c-wide slices of
    q / k and v plus the normaliser in tensor ops (ops._blockmix_wide_head) -- outputs and every gradient against the oracle."""
    idx = torch.randperm(M * S, generator=torch.Generator().manual_seed(M)).int() if gather else None
    run_case(1, 2, M, S, D, dtype, normalize=normalize, split=split, w="rand", idx=idx, seed=D)


def test_head_dims_above_128_relu_prologue_and_padding():
    """dim_head > 128 with the relu + eps prologue (applied before the zero padding of a slice: padded columns stay 0) against the oracle."""
    import mhla_amd
    B, H, M, S, D = 1, 2, 6, 20, 136
    g = torch.Generator().manual_seed(3)
    q, k, v, do = (torch.randn(B, M * S, H, D, generator=g) for _ in range(4))
    W = torch.rand(M, M, generator=g)
    want, wg = oracle_blockmix(torch.relu(q) + 1e-6, torch.relu(k) + 1e-6, v, W, do, None, None, 1e-6, True)
    t = [x.requires_grad_(True) for x in to_dev(q, k, v, W)]
    out = mhla_amd.mhla_blockmix(*t, relu_eps=True)
    out.backward(do.to(DEV))
    check("out", out, want, TOL[torch.float32])
    check("dv", t[2].grad, wg["dv"], GTOL[torch.float32])
    check("dW", t[3].grad, wg["dW"], DW_TOL[torch.float32])
    mask = lambda gq, x: gq * (x > 0)
    check("dq", t[0].grad, mask(wg["dq"], q), GTOL[torch.float32])
    check("dk", t[1].grad, mask(wg["dk"], k), GTOL[torch.float32])


@pytest.mark.parametrize("vscale,doscale", [(1e-18, 1e12), (3e14, 1e-25), (1.0, 1.0)])
def test_h16_summaries_keep_their_precision_at_extreme_scales(vscale, doscale):
    """The 2-byte summaries carry one power-of-two multiplier per block row (measured maximum in k_sp_state, bound of the inputs in the
    mixing kernels): v or dO scaled by 1e-18 .. 3e14 -- far outside what a bare fp16 holds -- leave the relative error where it was;
    an all-zero block (its row multiplier clamps at 2^-126) and a block 2^40 above the others ride along."""
    import mhla_amd
    B, H, M, S, D = 1, 2, 16, 32, 64
    q, k, v, W, do, _, _ = make_blockmix_inputs(B, H, M, S, D, torch.float32, 11, "rand", False)
    v = v * vscale
    v[:, 3 * S:4 * S] = 0.0                       # a block whose KV summary is exactly zero
    v[:, 5 * S:6 * S] *= 2.0 ** 40                # ... and one that dwarfs the others
    do = do * doscale
    q, k, v, do = (t.to(torch.bfloat16) for t in (q, k, v, do))
    assert mhla_amd.describe_dispatch(B, H, M, S, D, torch.bfloat16)["summaries"].startswith("h16")
    want, wg = oracle_blockmix(q, k, v, W, do, None, None, 1e-6, True)
    t = [x.requires_grad_(True) for x in to_dev(q, k, v, W)]
    out = mhla_amd.mhla_blockmix(*t)
    out.backward(do.to(DEV))
    otol, gtol, wtol = bm_tols(torch.bfloat16)
    check("out", out, want, otol)
    check("dq", t[0].grad, wg["dq"], gtol)
    check("dk", t[1].grad, wg["dk"], gtol)
    check("dv", t[2].grad, wg["dv"], gtol)
    check("dW", t[3].grad, wg["dW"], wtol)


def test_empty_batch():
    """B = 0 (and T = 0 for the causal op): empty result, zero gradients, no launch."""
    import mhla_amd
    q = torch.empty(0, 64, 2, 32, device=DEV, requires_grad=True)
    W = torch.eye(4, device=DEV, requires_grad=True)
    out = mhla_amd.mhla_blockmix(q, q, q, W)
    assert out.shape == (0, 64, 2, 32)
    out.sum().backward()
    assert W.grad is not None and float(W.grad.abs().max()) == 0.0
    qc = torch.empty(2, 0, 2, 16, device=DEV)
    assert mhla_amd.mhla_causal(qc, qc, qc, torch.ones(4, 4, device=DEV)).shape == (2, 0, 2, 16)


def test_errors_fail_loudly():
    import mhla_amd
    q = torch.randn(1, 64, 2, 64, device=DEV)
    W = torch.eye(4, device=DEV)
    with pytest.raises(RuntimeError):
        mhla_amd.mhla_blockmix(q.cpu(), q.cpu(), q.cpu(), W.cpu())            # no CPU fallback
    with pytest.raises(ValueError):
        mhla_amd.mhla_blockmix(q, q, q, torch.eye(5, device=DEV))             # N not divisible by M
    big = torch.randn(1, 64, 2, 160, device=DEV)
    with pytest.raises(ValueError):
        mhla_amd.mhla_blockmix(big, big, big, W, q_den=big, k_den=big, relu_eps=True)   # relu prologue with a separate normaliser pair (as for D <= 128)
    with pytest.raises(TypeError):
        mhla_amd.mhla_blockmix(q.double(), q.double(), q.double(), W)


@pytest.mark.parametrize("summaries", ["tf32", "split", "bf16"])
def test_full_size_c2_properties_and_sampled_heads(summaries):
    """BASELINE config C2 (B=8, N=4096, H=16, D=64, bf16, M=S=64): sampled (b, h) slices vs the oracle,
    plus size-independent properties: linearity in v, and W = I decouples blocks.  Default arithmetic (the number of record:
    one final rounding + 1e-3, dW within 1e-3) and the opt-in bf16-summary fast path at its own bounds."""
    import mhla_amd
    otol, gtol, wtol = bm_tols(torch.bfloat16, summaries)
    B, N, H, D, M = 8, 4096, 16, 64, 64
    q, k, v, W, do, _, _ = make_blockmix_inputs(B, H, M, N // M, D, torch.bfloat16, seed=1234)
    dq, dk, dv, dW, ddo = to_dev(q, k, v, W, do)
    for t in (dq, dk, dv, dW):
        t.requires_grad_(True)
    out = mhla_amd.mhla_blockmix(dq, dk, dv, dW, summaries=summaries)
    out.backward(ddo)
    for (b, h) in [(0, 0), (3, 7), (7, 15)]:
        sl = lambda t: t[b:b + 1, :, h:h + 1]
        want, wg = oracle_blockmix(sl(q), sl(k), sl(v), W, sl(do), None, None, 1e-6, True)
        check("out", sl(out), want, otol)
        check("dq", sl(dq.grad), wg["dq"], gtol)
        check("dk", sl(dk.grad), wg["dk"], gtol)
        check("dv", sl(dv.grad), wg["dv"], gtol)
    # dW is a sum over all 128 (b, h) pairs: the whole batch through the oracle (a few seconds on the host)
    _, wg_all = oracle_blockmix(q, k, v, W, do, None, None, 1e-6, True)
    check("dW (all heads)", dW.grad, wg_all["dW"], wtol)
    # linearity in v (fp32 so the property is tight)
    qf, kf, vf = dq.detach().float(), dk.detach().float(), dv.detach().float()
    v2 = torch.randn_like(vf)
    o1 = mhla_amd.mhla_blockmix(qf, kf, vf, dW.detach())
    o2 = mhla_amd.mhla_blockmix(qf, kf, v2, dW.detach())
    o12 = mhla_amd.mhla_blockmix(qf, kf, vf + 2 * v2, dW.detach())
    check("linearity", o12, (o1 + 2 * o2).cpu(), 1e-4)
    # W = I: changing block 5's k, v must not change any other block's output
    eye = torch.eye(M, device=DEV)
    oa = mhla_amd.mhla_blockmix(qf, kf, vf, eye)
    k2, v3 = kf.clone(), vf.clone()
    S = N // M
    k2[:, 5 * S:6 * S] += 1.0
    v3[:, 5 * S:6 * S] *= -2.0
    ob = mhla_amd.mhla_blockmix(qf, k2, v3, eye)
    mask = torch.ones(N, dtype=torch.bool, device=DEV)
    mask[5 * S:6 * S] = False
    assert torch.equal(oa[:, mask], ob[:, mask])
    assert not torch.equal(oa[:, ~mask], ob[:, ~mask])


def _check_dw_additive(mhla_amd, q, k, v, do, Wd, W, chunk, summaries="split"):
    """dW of the whole (huge) batch = sum of the dW of batch chunks (size-independent property: catches indexing errors of the
    partial / reduction buffers at large grids), and the first chunk's dW is anchored on the oracle."""
    full = Wd.grad.detach().double().cpu()
    acc = torch.zeros_like(full)
    B = q.shape[0]
    for b0 in range(0, B, chunk):
        qs, ks, vs = (t.detach()[b0:b0 + chunk].requires_grad_(True) for t in (q, k, v))
        Wc = W.to(DEV).requires_grad_(True)
        mhla_amd.mhla_blockmix(qs, ks, vs, Wc, summaries=summaries).backward(do[b0:b0 + chunk])
        acc += Wc.grad.double().cpu()
        if b0 == 0:
            f = lambda t: t.detach()[:8].float().cpu()
            _, wg = oracle_blockmix(f(q), f(k), f(v), W, f(do), None, None, 1e-6, True)
            Wa = W.to(DEV).requires_grad_(True)
            mhla_amd.mhla_blockmix(q.detach()[:8].requires_grad_(True), k.detach()[:8], v.detach()[:8], Wa, summaries=summaries).backward(do[:8])
            check("dW (first 8 samples vs oracle)", Wa.grad, wg["dW"], bm_tols(torch.bfloat16, summaries)[2])
    # fp32 partial sums in different groupings: agreement to fp32 summation noise
    check("dW additivity over batch chunks", full.float(), acc.float(), 2e-4)


def test_more_than_2_31_elements_per_tensor():
    """Maximum sizes: 2.2e9 elements (4.4 GB) per token tensor -- element offsets no longer fit 32 bits.  Inputs are generated
    on the device; the first, a middle and the last (b, h) slices are checked against the oracle, forward and backward.
    (summaries="bf16": the fast path's indexing; the split-operand path has its own test below, at the default arithmetic.)"""
    import mhla_amd
    otol, gtol, _ = bm_tols(torch.bfloat16, "bf16")
    B, N, H, D, M = 528, 4096, 16, 64, 64
    assert B * N * H * D > 2 ** 31
    gen = torch.Generator(device=DEV).manual_seed(7)
    mk = lambda relu: (torch.randn(B, N, H, D, device=DEV, dtype=torch.bfloat16, generator=gen).relu_().add_(1e-3) if relu
                       else torch.randn(B, N, H, D, device=DEV, dtype=torch.bfloat16, generator=gen))
    q, k, v, do = mk(True), mk(True), mk(False), mk(False)
    W = orc.block_distance_weights((8, 8), "linear")
    Wd = W.to(DEV).requires_grad_(True)
    for t in (q, k, v):
        t.requires_grad_(True)
    out = mhla_amd.mhla_blockmix(q, k, v, Wd, summaries="bf16")
    out.backward(do)
    for (b, h) in [(0, 0), (263, 9), (B - 1, H - 1)]:
        sl = lambda t: t.detach()[b:b + 1, :, h:h + 1].cpu()
        want, wg = oracle_blockmix(sl(q), sl(k), sl(v), W, sl(do), None, None, 1e-6, True)
        check("out", sl(out), want, otol)
        check("dq", sl(q.grad), wg["dq"], gtol)
        check("dk", sl(k.grad), wg["dk"], gtol)
        check("dv", sl(v.grad), wg["dv"], gtol)
    _check_dw_additive(mhla_amd, q, k, v, do, Wd, W, chunk=48, summaries="bf16")
    del q, k, v, do, out
    torch.cuda.empty_cache()


def test_more_than_2_31_elements_split_path():
    """The same on the split-operand path (DiT-XL/2 512x512 shape, D = 72, bf16): 2.15e9 elements per tensor, 29 184 (b, h) pairs."""
    import mhla_amd
    B, N, H, D, M = 1824, 1024, 16, 72, 16
    assert B * N * H * D > 2 ** 31 and B * H <= 65535
    gen = torch.Generator(device=DEV).manual_seed(11)
    mk = lambda relu: (torch.randn(B, N, H, D, device=DEV, dtype=torch.bfloat16, generator=gen).relu_().add_(1e-3) if relu
                       else torch.randn(B, N, H, D, device=DEV, dtype=torch.bfloat16, generator=gen))
    q, k, v, do = mk(True), mk(True), mk(False), mk(False)
    W = orc.block_distance_weights((4, 4), "linear")
    Wd = W.to(DEV).requires_grad_(True)
    for t in (q, k, v):
        t.requires_grad_(True)
    out = mhla_amd.mhla_blockmix(q, k, v, Wd)
    out.backward(do)
    for (b, h) in [(0, 0), (B - 1, H - 1)]:
        sl = lambda t: t.detach()[b:b + 1, :, h:h + 1].cpu()
        want, wg = oracle_blockmix(sl(q), sl(k), sl(v), W, sl(do), None, None, 1e-6, True)
        check("out", sl(out), want, TOL[torch.bfloat16])
        check("dq", sl(q.grad), wg["dq"], GTOL[torch.bfloat16])
        check("dk", sl(k.grad), wg["dk"], GTOL[torch.bfloat16])
        check("dv", sl(v.grad), wg["dv"], GTOL[torch.bfloat16])
    _check_dw_additive(mhla_amd, q, k, v, do, Wd, W, chunk=152)
    del q, k, v, do, out
    torch.cuda.empty_cache()


def test_full_size_c4_wan_sampled_head():
    """BASELINE config C4 (Wan2.1-1.3B: N = 31500 = 150 blocks x 210 tokens, H = 12, D = 128, fp32, roped numerator pair
    / un-roped normaliser pair, raster tokens gathered through the block index): forward on all heads, one head vs oracle."""
    import mhla_amd
    B, H, D, layout, grid = 1, 12, 128, (3, 5, 10), (21, 30, 50)
    N, M = 21 * 30 * 50, 150
    g = torch.Generator().manual_seed(99)
    q = torch.relu(torch.randn(B, N, H, D, generator=g)) + 1e-6
    k = torch.relu(torch.randn(B, N, H, D, generator=g)) + 1e-6
    v = torch.randn(B, N, H, D, generator=g)
    qr = q * torch.sign(torch.randn(B, N, H, D, generator=g))
    kr = k * torch.sign(torch.randn(B, N, H, D, generator=g))
    W = orc.block_distance_weights(layout, "linear")
    idx = orc.block_index_3d(grid, layout)
    out = mhla_amd.mhla_blockmix(qr.to(DEV), kr.to(DEV), v.to(DEV), W.to(DEV), q_den=q.to(DEV), k_den=k.to(DEV),
                                 block_index=idx.int().to(DEV))
    h = 7
    sl = lambda t: t[:, idx][:, :, h:h + 1]
    want = orc.blockmix_fwd(sl(qr), sl(kr), sl(v), W, 1e-6, q_den=sl(q), k_den=sl(k))
    check("out", out[:, idx.to(DEV)][:, :, h:h + 1], want, 1e-3)
    out2 = mhla_amd.mhla_blockmix(qr.to(DEV), kr.to(DEV), v.to(DEV), W.to(DEV), normalize=False, block_index=idx.int().to(DEV))
    want2 = orc.blockmix_fwd(sl(qr), sl(kr), sl(v), W, 1e-6, normalize=False)
    check("out_nonorm", out2[:, idx.to(DEV)][:, :, h:h + 1], want2, 1e-3)


def test_full_size_c4_wan_backward_sampled_head_and_full_dw():
    """C4 shape, training direction: forward + backward on all 12 heads (fp32, split q/k pairs, gather map); every token
    gradient of one head and the mixing-weight gradient summed over ALL heads against the oracle's closed form."""
    import mhla_amd
    B, H, D, layout, grid = 1, 12, 128, (3, 5, 10), (21, 30, 50)
    N = 21 * 30 * 50
    g = torch.Generator().manual_seed(199)
    q = torch.relu(torch.randn(B, N, H, D, generator=g)) + 1e-6
    k = torch.relu(torch.randn(B, N, H, D, generator=g)) + 1e-6
    v = torch.randn(B, N, H, D, generator=g)
    do = torch.randn(B, N, H, D, generator=g)
    qr = q * torch.sign(torch.randn(B, N, H, D, generator=g))
    kr = k * torch.sign(torch.randn(B, N, H, D, generator=g))
    W = orc.block_distance_weights(layout, "linear")
    idx = orc.block_index_3d(grid, layout)
    leaves = [t.to(DEV).requires_grad_(True) for t in (qr, kr, v, W, q, k)]
    poison()
    out = mhla_amd.mhla_blockmix(leaves[0], leaves[1], leaves[2], leaves[3], q_den=leaves[4], k_den=leaves[5],
                                 block_index=idx.int().to(DEV))
    poison()
    out.backward(do.to(DEV))
    torch.cuda.synchronize()
    bm = lambda t: t[:, idx]                      # raster -> block-major token order (what the oracle works on)
    wg = orc.blockmix_bwd(bm(qr), bm(kr), bm(v), W, bm(do), 1e-6, q_den=bm(q), k_den=bm(k))
    h = 5
    hd = lambda t: t[:, :, h:h + 1]
    for name, leaf in zip(("dq", "dk", "dv", None, "dq_den", "dk_den"), leaves):
        if name:
            check(name, hd(bm(leaf.grad.cpu())), hd(wg[name]), 1e-3)
    check("dW (12 heads)", leaves[3].grad, wg["dW"], 1e-3)


def test_more_batch_head_pairs_than_one_launch_addresses():
    """B * H > 65535 (the kernels' grid.y range): the operator slices the batch and accumulates dW over the slices; same
    results as the oracle on sampled samples and dW against a two-half evaluation."""
    import mhla_amd
    B, N, H, D, M = 16400, 16, 4, 16, 4
    g = torch.Generator(device=DEV).manual_seed(3)
    q = torch.rand(B, N, H, D, device=DEV, generator=g) + 1e-3
    k = torch.rand(B, N, H, D, device=DEV, generator=g) + 1e-3
    v = torch.randn(B, N, H, D, device=DEV, generator=g)
    do = torch.randn(B, N, H, D, device=DEV, generator=g)
    W = orc.block_distance_weights((2, 2), "linear")
    assert B * H > 65535
    leaves = [t.requires_grad_(True) for t in (q, k, v, W.to(DEV))]
    out = mhla_amd.mhla_blockmix(*leaves)
    out.backward(do)
    for b in (0, 16383, 16384, B - 1):     # both sides of the slice boundary
        sl = lambda t: t.detach()[b:b + 1].cpu()
        want, wg = oracle_blockmix(sl(q), sl(k), sl(v), W, sl(do), None, None, 1e-6, True)
        check("out", sl(out), want, 1e-3)
        check("dq", sl(q.grad), wg["dq"], 1e-3)
        check("dv", sl(v.grad), wg["dv"], 1e-3)
    half = B // 2
    acc = 0
    for b0 in (0, half):
        Wc = W.to(DEV).requires_grad_(True)
        mhla_amd.mhla_blockmix(q.detach()[b0:b0 + half], k.detach()[b0:b0 + half], v.detach()[b0:b0 + half], Wc).backward(do[b0:b0 + half])
        acc = acc + Wc.grad
    check("dW over slices", leaves[3].grad, acc.cpu(), 1e-4)


@pytest.mark.parametrize("summaries", ["split", "bf16"])
def test_repetitions_bit_identical_alone_and_beside_a_second_stream(summaries):
    """Determinism: the backward runs dz = W^T dn and the dW products as workgroups of ONE launch, and a host
    may run several operators on several streams (DDP buckets, side streams).  Round 1 saw run-to-run differences in the
    normaliser gradients when two of the library's kernels overlapped; this test repeats the C2-shaped operator alone and
    with a second instance running concurrently on another stream and demands bit-identical gradients every time."""
    import mhla_amd
    g = torch.Generator(device=DEV).manual_seed(5)
    mk = lambda b: torch.randn(b, 4096, 4, 64, device=DEV, dtype=torch.bfloat16, generator=g).abs_().add_(1e-3)
    q, k, v, do = mk(8), mk(8), mk(8), mk(8)
    q2, k2, v2, do2 = mk(6), mk(6), mk(6), mk(6)
    W = torch.rand(64, 64, device=DEV, generator=g)
    side = torch.cuda.Stream()

    def run(concurrent):
        ts = [x.clone().requires_grad_(True) for x in (q, k, v, W)]
        if concurrent:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                t2 = [x.clone().requires_grad_(True) for x in (q2, k2, v2, W)]
                for _ in range(2):
                    mhla_amd.mhla_blockmix(*t2, summaries=summaries).backward(do2)
        out = mhla_amd.mhla_blockmix(*ts, summaries=summaries)
        out.backward(do)
        torch.cuda.synchronize()
        return [out.detach().clone()] + [x.grad.clone() for x in ts]

    ref = run(False)
    for rep in range(6):
        got = run(rep % 2 == 1)
        for name, a_, b_ in zip(["out", "dq", "dk", "dv", "dW"], ref, got):
            assert torch.equal(a_, b_), f"repetition {rep} ({'two streams' if rep % 2 else 'alone'}): {name} differs"


@pytest.mark.parametrize("B,H,M,S", [(1, 1, 3, 5), (1, 3, 17, 33), (2, 16, 33, 64), (8, 16, 64, 64), (33, 7, 16, 16), (2, 16, 16, 256)])
def test_token_gradient_launch_handover_on_two_streams(B, H, M, S, monkeypatch):
    """The backward's token gradients are one launch in which a tile's dK/dV workgroup waits for the flag of its dQ workgroup
    (DESIGN.md 3b).  Shapes with partly empty tiles, one tile per (b,h), few and many (b,h) pairs, multi-chunk blocks.  Every
    repetition has its OWN inputs (a waiter that passed early would otherwise read the previous repetition's identical dksum
    rows out of the recycled workspace and go unnoticed) and its own reference: the same backward with the two roles as two
    launches (mhla_set_option("bwd_two_launches", 1): the kernel boundary orders the hand-over), alone on the device.  The fused launch then
    runs beside a second instance of the operator on another stream, must be bit-identical to the reference, and the
    library's status call must report no expired wait (tools/stress_fast_path.py is the long version)."""
    import mhla_amd
    from gpu_util import poison
    g = torch.Generator(device=DEV).manual_seed(B * 1000 + M)
    mk = lambda: torch.randn(B, M * S, H, 64, device=DEV, dtype=torch.bfloat16, generator=g).abs_().add_(1e-3)
    side = torch.cuda.Stream()
    for rep in range(3):
        q, k, v, do = mk(), mk(), mk(), mk()
        W = torch.rand(M, M, device=DEV, generator=g).add_(0.1)

        def run(beside):
            if beside:
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    t2 = [x.flip(0).clone().requires_grad_(True) for x in (q, k, v)]
                    mhla_amd.mhla_blockmix(*t2, W, summaries="bf16").backward(do)
            ts = [x.clone().requires_grad_(True) for x in (q, k, v, W)]
            out = mhla_amd.mhla_blockmix(*ts, summaries="bf16")
            out.backward(do)
            torch.cuda.synchronize()
            return [out.detach()] + [x.grad for x in ts]

        lib = mhla_amd._lib.load()
        lib.mhla_set_option(b"bwd_two_launches", 1)
        ref = run(False)
        lib.mhla_set_option(b"bwd_two_launches", 0)
        poison()   # the workspace blocks the reference used come back NaN-filled
        monkeypatch.setenv("MHLA_CHECK_HANDOVER", "1")
        res = run(True)
        monkeypatch.delenv("MHLA_CHECK_HANDOVER")
        assert all(bool(torch.isfinite(r.float()).all()) for r in res)
        for name, a_, b_ in zip(["out", "dq", "dk", "dv", "dW"], ref, res):
            assert torch.equal(a_, b_), f"repetition {rep}: {name} of the fused launch differs from the two-launch reference"


def test_handover_wait_is_bounded_and_reported(monkeypatch):
    """A flag that never arrives must end as an error code, not as a hung GPU: with the dQ role's signal suppressed
    (mhla_set_option("debug_drop_signal", 1), a testing aid of the library) the backward still returns, and
    mhla_blockmix_bwd_status -- here through MHLA_CHECK_HANDOVER=1 in the autograd function -- reports the expired wait.
    The failure heals itself: the library copies every fused launch's error word to the host asynchronously and looks at it at
    its next backward -- after ONE expired hand-over the process runs the two roles as two launches, without any environment
    variable or host synchronisation (round 5, verdict item 8)."""
    import mhla_amd
    lib = mhla_amd._lib.load()
    g = torch.Generator(device=DEV).manual_seed(7)
    B, H, M, S = 1, 2, 16, 64
    mk = lambda: torch.randn(B, M * S, H, 64, device=DEV, dtype=torch.bfloat16, generator=g).abs_().add_(1e-3)
    q, k, v, do = mk(), mk(), mk(), mk()
    W = torch.rand(M, M, device=DEV, generator=g).add_(0.1)

    def bwd():
        ts = [x.clone().requires_grad_(True) for x in (q, k, v, W)]
        mhla_amd.mhla_blockmix(*ts, summaries="bf16").backward(do)
        torch.cuda.synchronize()
        return [x.grad for x in ts]

    try:
        lib.mhla_set_option(b"bwd_two_launches", 1)
        ref = bwd()                                   # the two-launch reference
        lib.mhla_set_option(b"bwd_two_launches", 0)
        assert all(torch.equal(a_, b_) for a_, b_ in zip(ref, bwd())), "fused launch differs from the two-launch form"
        # (1) no synchronous check (the default: no host sync on the training path): the failure is still loud -- the waiter that
        # gave up poisons its dksum rows, so the tile's dk is NaN, never a finite, silently wrong gradient
        lib.mhla_set_option(b"debug_drop_signal", 1)
        bad = bwd()
        lib.mhla_set_option(b"debug_drop_signal", 0)
        assert bool(torch.isnan(bad[1].float()).all()), "dk of a tile whose hand-over expired must be NaN"
        assert bool(torch.isfinite(bad[0].float()).all()) and bool(torch.isfinite(bad[2].float()).all())
        # (2) ... and the NEXT backward is finite and bit-identical to the two-launch reference: the library has seen the error word
        # of the launch above (asynchronous copy + event, examined at this call) and switched the process to two launches itself
        healed = bwd()
        assert all(bool(torch.isfinite(x.float()).all()) for x in healed)
        for name, a_, b_ in zip(("dq", "dk", "dv", "dW"), ref, healed):
            assert torch.equal(a_, b_), f"{name} after the self-healing switch differs from the two-launch reference"
        assert lib.mhla_set_option(b"bwd_two_launches", 0) == 1, "the process should have latched the two-launch form"
        # (3) the synchronous form of the same report: mhla_blockmix_bwd_status through MHLA_CHECK_HANDOVER=1 (Python autograd node)
        lib.mhla_set_option(b"debug_drop_signal", 1)
        monkeypatch.setenv("MHLA_CHECK_HANDOVER", "1")
        ts = [x.clone().requires_grad_(True) for x in (q, k, v, W)]
        out = mhla_amd.mhla_blockmix(*ts, summaries="bf16")
        with pytest.raises(RuntimeError, match="gave up waiting"):
            out.backward(do)
        torch.cuda.synchronize()
        monkeypatch.delenv("MHLA_CHECK_HANDOVER")
        lib.mhla_set_option(b"debug_drop_signal", 0)
        bwd()                                          # (consumes the pending report of the launch above)
    finally:
        lib.mhla_set_option(b"debug_drop_signal", 0)
        lib.mhla_set_option(b"bwd_two_launches", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("M,S", [(160, 64), (256, 48), (130, 130)])
def test_more_than_128_blocks_of_many_tokens_dw_stages(M, S):
    """More than 128 blocks with blocks longer than 16 tokens: the whole-matrix dW kernel (k_sp_dwr<.., h16>) deals the fp32 stages of the
    <dn, z> term over its E-slice workgroups (S / 16 of them; all on slice 0 they were one serial chain) -- against the oracle, with a
    block length that is not a multiple of 4 among them (scalar loads)."""
    run_case(1, 2, M, S, 64, torch.bfloat16, w="rand", seed=M + S)


@pytest.mark.gpu
@pytest.mark.parametrize("M,B,H,D", [(256, 8, 16, 64), (192, 8, 16, 64), (160, 8, 16, 64), (256, 5, 20, 64), (144, 4, 24, 72)])
def test_recut_mixing_kernel_is_bit_identical_to_the_one_it_replaced(M, B, H, D):
    """129 .. 256 blocks with enough slices per workgroup run k_sp_mixh2 (mixh2.hpp: the rescaled weight pairs kept per (b, h), output rows of
    256 blocks in two workgroups); mhla_set_option("recut_kernels", 0) runs k_sp_mixh instead.  Same expressions in the same order: every
    output and gradient must agree bit for bit, and the dispatcher must say which one ran.  (5 x 20 and 4 x 24 (b, h): 25 resp. 31 slices per
    workgroup of 64 / 81 per (b, h) -- ranges that cross (b, h) boundaries, i.e. the mid-range rebuild with its flush.)"""
    import mhla_amd
    S = 16
    N = M * S
    g = torch.Generator().manual_seed(M)
    q, k, v = (torch.randn(B, N, H, D, generator=g).bfloat16().cuda() for _ in range(3))
    W = torch.rand(M, M, generator=g).cuda()
    do = torch.randn(B, N, H, D, generator=g).bfloat16().cuda()

    def run():
        ts = [t.clone().requires_grad_(True) for t in (q, k, v, W)]
        out = mhla_amd.mhla_blockmix(ts[0].abs(), ts[1].abs(), ts[2], ts[3])
        out.backward(do)
        torch.cuda.synchronize()
        return [out.detach()] + [t.grad for t in ts]

    assert mhla_amd.describe_dispatch(B, H, M, S, D, torch.bfloat16)["fwd"][1] == "k_sp_mixh2<0>"
    new = run()
    prev = mhla_amd.set_option("recut_kernels", 0)
    try:
        assert mhla_amd.describe_dispatch(B, H, M, S, D, torch.bfloat16)["fwd"][1] == "k_sp_mixh<0>"
        old = run()
    finally:
        mhla_amd.set_option("recut_kernels", prev)
    for name, a, b in zip(("out", "dq", "dk", "dv", "dW"), new, old):
        assert torch.equal(a, b), f"{name} differs between k_sp_mixh2 and k_sp_mixh at M={M}"
