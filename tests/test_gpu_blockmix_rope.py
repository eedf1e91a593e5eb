"""GPU parity: the rotary block-mix operator (mhla_blockmix_rope: Wan's rotation of q and k inside the kernels, forward and backward)
against the fp64 operator on the same tensors (gpu_util.rope_blockmix_fp64), at every launch shape of its kernel variants --
k_sp_state<rope> in both modes on fp32-word and p24 summaries, the table branches of k_sp_out, k_sp_bwd_dq<rope>, k_sp_bwd_dkv<rope>.

The plan of each fp32 case, read from bm_plan (capi_common.hpp) and the kernels' tiling (split.hpp): the summary kernel walks a block in
32-row chunks (first fetch, steady-state loop, peeled last chunk), the token kernels in passes of 64 tokens (four 16-token tiles);
tile classes DT = 2 / 4 / 5 / 6 / 8 serve head dims up to 32 / 64 / 80 / 96 / 128, smaller ones zero-padded.

 #  B H   M   S   D norm map   reaches
 1  2 3   5  70  72  T   map   DT=5, padded D; 3 chunks (steady state + peeled last of 6 rows); 2 passes, a 6-row last tile; B > 1 with a map
 2  2 2   3  40  24  T   map   DT=2, padded D; partial second chunk
 3  2 2   9  16   8  T    -    D = 8 (DT=2); without tables the small-sequence family's shape: the tables send it to the typed path
 4  1 2  70  20  88  T    -    DT=6, padded D; 8-wave resident mixing on fp32 words
 5  1 3  33  24  96  T   map   DT=6 exact; 4-wave mixing
 6  2 2  40  33 128  T    -    p24 summaries; 4-wave mixing; odd S: the normaliser's product is a k_wz launch, <dn, z> of dW a k_dw launch
 7  1 2 150  17 104  F   map   p24, padded D; 12-wave mixing; dW by k_sp_dwt; no normaliser
 8  2 2 200   8 128  T   map   M > 192 at D = 128: fp32 words, 16-wave mixing, dW by k_sp_dw
 9  1 2 260   8  64  T    -    M > 256: the tiled k_sp_mix
10  2 2   6 210 128  T   map   the Wan training shape's block length: 7 chunks, 4 passes with a 2-row last tile; p24
11  1 2   1  48  64  T    -    M = 1
12  2 2  16  16  64  F   map   DT=4 exact; no normaliser

mhla_describe_dispatch has no argument for "with tables", and the tables change neither the summary format nor the mixing / dW
kernels of a plan (bm_plan: `rope` only names the state and token kernels and excludes the small-sequence / fast families), so each
case asserts those three from the description of the table-less call with the small-sequence family excluded; the wave counts above
follow bm_plan's rule (2 up to 32 blocks, 4 up to 64, 8 up to 128, 12 up to 192, 16 beyond) and are not part of the description.

Tolerances are gpu_util's (TOL / DW_TOL; derived there) and, for the fused epilogue, the ones test_qk_prologue_and_rope_op uses."""
import functools

import pytest
import torch

from gpu_util import DEV, DW_TOL, ROPE_CASES, TOL, check, make_rope_inputs, poison, rope_blockmix_fp64, rope_case_seed

pytestmark = pytest.mark.gpu

F32W, P24 = "fp32 words", "p24"
# (summary format, forward mixing kernel, what the backward's description must name) per case, in ROPE_CASES' order
PLAN = [
    (F32W, "k_sp_mixr<0>", ["k_sp_mixr<1,dw>"]), (F32W, "k_sp_mixr<0>", ["k_sp_mixr<1,dw>"]), (F32W, "k_sp_mixr<0>", ["k_sp_mixr<1,dw>"]),
    (F32W, "k_sp_mixr<0>", ["k_sp_mixr<1,dw>"]), (F32W, "k_sp_mixr<0>", ["k_sp_mixr<1,dw>"]),
    (P24, "k_sp_mixr<0>", ["k_sp_mixr<1,dw>", "k_wz<1>", "k_dw"]), (P24, "k_sp_mixr<0>", ["k_sp_mixr<1>", "k_sp_dwt"]),
    (F32W, "k_sp_mixr<0>", ["k_sp_mixr<1>", "k_sp_dw"]), (F32W, "k_sp_mix<0>", ["k_sp_mix<1>", "k_sp_dw"]),
    (P24, "k_sp_mixr<0>", ["k_sp_mixr<1,dw>"]), (F32W, "k_sp_mixr<0>", ["k_sp_mixr<1,dw>"]), (F32W, "k_sp_mixr<0>", ["k_sp_mixr<1,dw>"]),
]
_ids = lambda c: "-".join(str(int(x)) for x in c)


@functools.lru_cache(maxsize=None)
def _inputs(case, dtype):
    B, H, M, S, D, normalize, gather = case
    return make_rope_inputs(B, H, M, S, D, dtype, seed=rope_case_seed(case), gather=gather)


@functools.lru_cache(maxsize=None)
def _reference(case, dtype):
    """out, dq, dk, dv, dW in fp64 on the case's tensors (as rounded to `dtype`), computed once per session and never modified."""
    q, k, v, W, do, cos, sin, perm = _inputs(case, dtype)
    return rope_blockmix_fp64(q, k, v, W, do, cos, sin, perm, case[5])


def _fwd_bwd(case):
    """One forward + backward of mhla_blockmix_rope on the case's fp32 tensors: out and the gradients of q, k, v, W."""
    import mhla_amd
    q, k, v, W, do, cos, sin, perm = _inputs(case, torch.float32)
    t = [x.to(DEV).requires_grad_(True) for x in (q, k, v, W)]
    poison()
    out = mhla_amd.mhla_blockmix_rope(*t, cos.to(DEV), sin.to(DEV), eps=1e-6, normalize=case[5], block_index=None if perm is None else perm.to(DEV))
    poison()
    out.backward(do.to(DEV))
    torch.cuda.synchronize()
    return [out.detach()] + [x.grad for x in t]


@pytest.mark.parametrize("n", range(len(ROPE_CASES)), ids=[_ids(c) for c in ROPE_CASES])
def test_rope_fp32_forward_backward_vs_fp64(n):
    import mhla_amd
    case = ROPE_CASES[n]
    B, H, M, S, D, normalize, gather = case
    fmt, mix0, bwd_names = PLAN[n]
    d = mhla_amd.describe_dispatch(B, H, M, S, D, torch.float32, no_smalln=True)
    assert d["family"].startswith("split-operand") and d["summaries"].startswith(fmt), d["text"]
    assert mix0 in d["fwd"] and all(name in d["bwd"] for name in bwd_names), d["text"]
    assert ("k_wz<0>" in d["fwd"]) == (S % 2 == 1 or M > 256), d["text"]   # the normaliser's product rides in the resident mixing at even S
    got = _fwd_bwd(case)
    want = _reference(case, torch.float32)
    tol = TOL[torch.float32]
    for name, g, w in zip(("out", "dq", "dk", "dv"), got, want):
        assert g.dtype == torch.float32 and g.shape == w.shape
        check(name, g, w, tol)
    # M == 1: the output does not depend on W (numerator and normaliser scale together), dW ~ 0
    check("dW", got[4], want[4], DW_TOL[torch.float32], atol=1e-3 if M == 1 else 0.0)


@pytest.mark.parametrize("n", [0, 5], ids=[_ids(ROPE_CASES[0]), _ids(ROPE_CASES[5])])
def test_rope_kept_summaries_match_recompute(n, monkeypatch):
    """Backward with the forward's workspace kept (KV of the rotated keys, G, z, ksum, 1 / n reused) == backward that was handed none and
    runs k_sp_state<rope> and the mixing again with the tables: bit for bit."""
    from mhla_amd import ops
    res = []
    for limit in (1 << 30, 0):
        monkeypatch.setattr(ops, "KEEP_STATE_LIMIT_BYTES", limit)
        res.append(_fwd_bwd(ROPE_CASES[n]))
    for name, a, b in zip(("out", "dq", "dk", "dv", "dW"), *res):
        assert torch.equal(a, b), name


# 16-bit forwards the library serves: head dims above 96 (fp32-word summaries), and D <= 96 where M > 128 and S < 16 decline h16 and p24
CASES_16 = [(2, 2, 6, 40, 128, True, True), (2, 2, 3, 70, 104, True, False), (1, 2, 40, 33, 128, False, True), (2, 2, 5, 17, 120, True, False),
            (2, 2, 130, 8, 64, True, True)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES_16, ids=_ids)
def test_rope_16bit_forward_vs_fp64(case, dtype):
    """The 16-bit rotary forward at the default arithmetic: the fp64 operator on the 16-bit-rounded tensors (fp32 tables) within one final
    rounding + 1e-3 -- the rotated q and k are fp32 values and enter the products as bf16 hi + lo pairs whatever the tensor type.
    (Kernels that drop the lo part of the rotated bf16 operands -- two single-bf16 intermediates, the opt-in summaries="bf16" class of
    arithmetic -- sit 1.7e-3 .. 2.5e-3 beyond the final rounding at these shapes: profiles/rope_parity.md.)"""
    import mhla_amd
    B, H, M, S, D, normalize, gather = case
    assert mhla_amd.describe_dispatch(B, H, M, S, D, dtype, no_smalln=True)["summaries"].startswith(F32W)
    q, k, v, W, do, cos, sin, perm = _inputs(case, dtype)
    want = _reference(case, dtype)[0]
    with torch.no_grad():
        poison()
        got = mhla_amd.mhla_blockmix_rope(q.to(DEV), k.to(DEV), v.to(DEV), W.to(DEV), cos.to(DEV), sin.to(DEV), eps=1e-6, normalize=normalize,
                                          block_index=None if perm is None else perm.to(DEV))   # served: must not raise
        torch.cuda.synchronize()
    assert got.dtype == dtype and got.shape == q.shape
    check("out", got, want, TOL[dtype])


@pytest.mark.parametrize("dtype,M,S,D,match", [
    (torch.float16, 8, 8, 64, "h16 / p24 summaries is not built"),      # p24: D <= 96, M <= 128, blocks shorter than 16 tokens
    (torch.bfloat16, 130, 16, 64, "h16 / p24 summaries is not built"),  # h16 at 129 .. 256 blocks
    (torch.float32, 4, 8, 12, "rope tables|rotary prologue needs D"),   # a head dim that is no multiple of 8
], ids=["fp16-p24", "bf16-h16-M130", "D12"])
def test_rope_forward_refusals(dtype, M, S, D, match):
    """What the rotary forward does not serve is refused by the library before anything is launched (the output stays as allocated)."""
    import mhla_amd
    q, k, v, W, do, cos, sin, _ = make_rope_inputs(1, 2, M, S, D, dtype, seed=7)
    with torch.no_grad(), pytest.raises(RuntimeError, match=match):
        mhla_amd.mhla_blockmix_rope(q.to(DEV), k.to(DEV), v.to(DEV), W.to(DEV), cos.to(DEV), sin.to(DEV))
    torch.cuda.synchronize()


@pytest.mark.parametrize("D", [24, 72, 104])
def test_wan_fused_epilogue_at_padded_head_dims(D):
    """mhla_blockmix_wan (rotary prologue + per-head RMSNorm x SiLU gate before the store) == rmsnorm_gate(mhla_blockmix_rope(...)) where
    the head dim does not fill its tile: the RMS over D must not see the padded features.  Both sides are HIP: the rotary operator is
    tied to fp64 above, rmsnorm_gate in test_gpu_neighbours.py."""
    import mhla_amd
    B, H, M, S = 2, 2, 5, 40
    q, k, v, W, do, cos, sin, perm = (t.to(DEV) for t in make_rope_inputs(B, H, M, S, D, torch.float32, seed=D, gather=True))
    g = torch.Generator().manual_seed(D + 1)
    nw = (torch.rand(D, generator=g) + 0.5).to(DEV)
    poison()
    o = mhla_amd.mhla_blockmix_rope(q, k, v, W, cos, sin, eps=1e-6, block_index=perm)
    for odt in (torch.bfloat16, torch.float32):
        for gated in (True, False):
            gate = torch.randn(B, M * S, H, D, generator=g).to(odt).to(DEV) if gated else None
            want = mhla_amd.rmsnorm_gate(o.to(odt), gate, nw, 1e-5)
            poison()
            got = mhla_amd.mhla_blockmix_wan(q, k, v, W, cos, sin, nw, 1e-5, gate, odt, eps=1e-6, block_index=perm)
            assert got.dtype == odt
            check(f"wan fused D={D} {odt} gate={gated}", got, want.float().cpu(), 1e-5 if odt == torch.float32 else 8e-3)
