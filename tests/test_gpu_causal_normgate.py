"""GPU parity of the fused norm x gate output kernel of the causal operator (mhla_causal_normgate: k_csf_out4<NV, true, summaries>
for V = 64 .. 256, k_csf_out4<3 | 4, true, summaries, 2> for V = 384 / 512, and their chunk-table variants for packs) at every
summary format -- single-bf16 summaries included, which cs_epi_ok admits and no other test runs -- and at the shapes the other
fused tests leave out: a single chunk, an odd head count behind a ragged tail, strided views, rows whose o is exactly zero, kept
against recomputed summaries, and the shapes the epilogue does not cover.

What the checks rest on.  The fused node stores the operator's own o from the same accumulators and with the same scaling as the
plain output kernel, and its backward is _rmsnorm_gate_bwd followed by _causal_bwd -- the very calls of the unfused composition
rmsnorm_gate(mhla_causal(...)).  So at the same `summaries` and keep-state setting every gradient of the fused node (dq, dk, dv,
dmix, dgate, dweight) is BIT-IDENTICAL to the composition's: no tolerance, a wrong stored o in any row of either half shows, and
it holds at single-bf16 summaries, where no derived bound for gradients behind a norm exists.  The composition's two operators are
each held to the oracle elsewhere (test_gpu_causal, test_gpu_neighbours).

Forward, u = 2^-8:
  * y against the oracle's exact composition (causal_fwd -> rms_norm_swish_gate, or the plain norm): 2u + 1e-3, derived in
    test_gpu_causal.run_normgate; for summaries "tf32" and "split".
  * y against the CPU fp32 norm x gate of the DEVICE's unfused o (mhla_causal at the same summaries, upcast): 3u + 1e-3 -- the
    roundings of o, of the staging tile and of y; the accumulators are the same, so the bound does not depend on the format.
  * y against the unfused HIP composition: 3u + 1e-3.
  For summaries="bf16" the last two are the anchor (the operator alone is held to TOL_BF16SUM against the oracle); there is no
  direct bound against the oracle, because the norm divides by each row's own rms.
  * the inference call (no_grad: o is not stored) gives the training y bit for bit, and the launch profile names the fused kernel."""
import pytest
import torch

from gpu_util import DEV, check, launches, poison
from oracle import mhla_oracle as orc
from test_gpu_causal import causal_inputs
from test_gpu_causal_varlen import CU, seqs

pytestmark = pytest.mark.gpu

U = 2.0 ** -8
SUMMARIES = ["tf32", "split", "bf16"]
GRADS = ("dq", "dk", "dv", "dmix", "dgate", "dweight")


def fused_kernel(V, packed=False):
    """The launch-profile name of the fused output kernel (capi_causal.hip: OUT4 / OUT4H2)."""
    return "k_csf_out4<norm" + (",2" if V > 256 else "") + (",tab" if packed else "") + ">"


def gate_and_weight(B, T, H, V, gate, affine, dtype=torch.bfloat16):
    """As test_gpu_causal.run_normgate makes them."""
    gen = torch.Generator().manual_seed(7)
    g = torch.randn(B, T, H, V, generator=gen).to(dtype) if gate else None
    w = (torch.rand(V, generator=gen) + 0.5) if affine else None
    return g, w


def cpu_norm(o, g, w, eps):
    """fp32 norm x gate on the CPU (the oracle's; without a gate the plain norm of run_normgate)."""
    if g is not None:
        return orc.rms_norm_swish_gate(o.float(), g.float(), w, eps)
    o = o.float()
    return o * torch.rsqrt(o.pow(2).mean(-1, keepdim=True) + eps) * (1.0 if w is None else w)


def oracle_o(q, k, v, mix, cu=None):
    if cu is None:
        return orc.causal_fwd(q.float(), k.float(), v.float(), mix)
    return torch.cat([orc.causal_fwd(q[:, a:b].float(), k[:, a:b].float(), v[:, a:b].float(), mix) for a, b in seqs(cu)], 1)


def leaves(*ts):
    return [None if t is None else t.detach().to(DEV).requires_grad_(True) for t in ts]


def grads_of(ts):
    return dict(zip(GRADS, (None if t is None else t.grad for t in ts)))


def assert_same_gradients(a, b, what):
    for n in GRADS:
        assert (a[n] is None) == (b[n] is None), n
        if a[n] is not None:
            assert bool(torch.isfinite(a[n].float()).all()), f"{n}: non-finite"
            assert a[n].shape == b[n].shape and torch.equal(a[n], b[n]), \
                f"{n}: {what} differ (max |difference| {float((a[n].float() - b[n].float()).abs().max()):.3e})"


def run_fused(q, k, v, mix, do, g, w, summaries, norm_eps=1e-5, cu=None, keep_state_limit=None, fusable=True):
    """Training call of mhla_causal_normgate on device copies, the explicit composition on others, the inference call; every
    forward check of the module docstring and the bit-identity of the gradients.  `fusable` False: the shapes the epilogue does not
    cover -- y as well is the composition's bit for bit.  Returns (y, gradients of the fused call)."""
    import mhla_amd
    from mhla_amd import ops
    V, dtype = v.shape[-1], q.dtype
    plan = None if cu is None else mhla_amd.causal_varlen_plan(cu, DEV)
    kw = dict(summaries=summaries, keep_state_limit=keep_state_limit, cu_seqlens=plan)
    fd, cd = leaves(q, k, v, mix, g, w), leaves(q, k, v, mix, g, w)
    assert ops.causal_normgate_fusable(fd[0], fd[2], cu_seqlens=plan, flags=ops._causal_flags(summaries, False)) == fusable
    dod, res = do.to(DEV), {}
    poison()
    ran = launches(lambda: res.__setitem__("y", mhla_amd.mhla_causal_normgate(fd[0], fd[1], fd[2], fd[3], fd[4], fd[5], norm_eps, **kw)))
    y = res["y"]
    assert y.dtype == dtype and y.shape == v.shape
    fused = [n for n in ran if n.startswith("k_csf_out4<norm")]
    assert fused == ([fused_kernel(V, plan is not None)] if fusable else []) and (ran[fused[0]] == 1 if fusable else True), ran
    poison()
    y.backward(dod)
    poison()
    o2 = mhla_amd.mhla_causal(cd[0], cd[1], cd[2], cd[3], **kw)
    y2 = mhla_amd.rmsnorm_gate(o2, cd[4], cd[5], norm_eps)
    poison()
    y2.backward(dod)
    gf, gc = grads_of(fd), grads_of(cd)
    assert_same_gradients(gf, gc, "fused node and unfused composition")
    with torch.no_grad():
        y3 = mhla_amd.mhla_causal_normgate(fd[0], fd[1], fd[2], fd[3], fd[4], fd[5], norm_eps, **kw)
    assert torch.equal(y3, y), "inference call (o not stored) vs training call"
    if not fusable:
        assert torch.equal(y, y2), "y: not the composition's"
        return y.detach(), gf
    if summaries != "bf16":
        check("y vs exact composition", y, cpu_norm(oracle_o(q, k, v, mix, cu), g, w, norm_eps), 2 * U + 1e-3)
    check("y vs norm of the device's o", y, cpu_norm(o2.detach().cpu(), g, w, norm_eps), 3 * U + 1e-3)
    check("y fused vs unfused", y, y2.detach().float().cpu(), 3 * U + 1e-3)
    return y.detach(), gf


def uniform_case(B, T, H, K, V, summaries, gate=True, affine=True, norm_eps=1e-5, inputs=None, **kw):
    q, k, v, mix, do = causal_inputs(B, T, H, K, V, 8, torch.bfloat16, seed=T + V) if inputs is None else inputs
    g, w = gate_and_weight(B, T, H, V, gate, affine)
    return run_fused(q, k, v, mix, do, g, w, summaries, norm_eps=norm_eps, **kw)


# ---- 1. every fused instantiation x tails ----------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 64, 65, 200], ids=lambda T: f"T{T}")
@pytest.mark.parametrize("V", [64, 128, 192, 256, 384, 512], ids=lambda V: f"V{V}")
@pytest.mark.parametrize("summaries", SUMMARIES)
def test_variants_and_tails(summaries, V, T):
    """K = 64, B = 1, H = 3: a single token, exactly one chunk, a one-token and an eight-token last chunk -- behind a ragged tail lie
    another head's finite rows, which poison() cannot flag.  T <= 64: behind a norm the loss does not depend on m_00 (dmix is
    rounding noise around zero), so dmix is held by the identity alone -- as every gradient is."""
    uniform_case(1, T, 3, 64, V, summaries)


@pytest.mark.parametrize("K,V", [(256, 512), (192, 192)], ids=["K256-V512", "K192-V192"])
@pytest.mark.parametrize("summaries", SUMMARIES)
def test_variants_wide_keys(summaries, K, V):
    uniform_case(1, 200, 3, K, V, summaries)


# ---- 2. without gate / without weight --------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate,affine", [(False, True), (True, False), (False, False)], ids=["nogate", "noweight", "neither"])
@pytest.mark.parametrize("V", [256, 512], ids=lambda V: f"V{V}")
@pytest.mark.parametrize("summaries", SUMMARIES)
def test_without_gate_or_weight(summaries, V, gate, affine):
    uniform_case(1, 200, 3, 64, V, summaries, gate=gate, affine=affine)


# ---- 3. a norm_eps the result depends on, in the two-halves kernel -----------------------------------------------------------
@pytest.mark.parametrize("summaries", SUMMARIES)
def test_visible_norm_eps_two_halves(summaries):
    """norm_eps = mean(o^2): a kernel that dropped the argument, or applied it to one half only, fails every forward check."""
    from conftest import rel_err
    B, T, H, K, V = 1, 200, 3, 64, 512
    inputs = causal_inputs(B, T, H, K, V, 8, torch.bfloat16, seed=T + V)
    g, w = gate_and_weight(B, T, H, V, True, True)
    o = oracle_o(*inputs[:4])
    eps = float(o.square().mean())
    assert rel_err(cpu_norm(o, g, w, 1e-5), cpu_norm(o, g, w, eps)) > 0.2, "norm_eps is not visible: the case proves nothing"
    uniform_case(B, T, H, K, V, summaries, norm_eps=eps, inputs=inputs)


# ---- 4. rows whose o is exactly zero ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [256, 512], ids=lambda V: f"V{V}")
@pytest.mark.parametrize("summaries", SUMMARIES)
def test_rows_of_exact_zeros(summaries, V):
    """q = k = v = 0 on tokens 0..69 (left padding across a chunk boundary): o there is exactly zero, rstd = eps^-1/2 = 316, and the
    rows' do is that much larger than the others' -- y and dq, dk, dv, dgate on those rows are exactly zero, everything is finite."""
    B, T, H, K, pad = 1, 200, 3, 64, 70
    q, k, v, mix, do = causal_inputs(B, T, H, K, V, 8, torch.bfloat16, seed=T + V)
    for t in (q, k, v):
        t[:, :pad] = 0
    assert float(oracle_o(q, k, v, mix)[:, :pad].abs().max()) == 0.0
    y, grads = uniform_case(B, T, H, K, V, summaries, inputs=(q, k, v, mix, do))
    assert bool(torch.isfinite(y.float()).all()) and bool((y[:, :pad] == 0).all()), "y on the padded rows"
    assert bool((y[:, pad:] != 0).any())
    for n in ("dq", "dk", "dv", "dgate"):
        assert bool((grads[n][:, :pad] == 0).all()), f"{n}: a padded row's gradient is not zero"
        assert bool((grads[n][:, pad:] != 0).any()), n


# ---- 5. views ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("summaries", SUMMARIES)
def test_strided_views(summaries):
    """q, k, v as slices of one [B, T, 3, H, 64] projection, the gate as a slice of a [B, T, 2, H, V] buffer, dy a non-contiguous
    view: y and every gradient are those of the call on contiguous copies, bit for bit."""
    import mhla_amd
    B, T, H, D = 2, 200, 3, 64
    gen = torch.Generator().manual_seed(11)
    qkv = torch.randn(B, T, 3, H, D, generator=gen).bfloat16()
    gg = torch.randn(B, T, 2, H, D, generator=gen).bfloat16()
    dyy = torch.randn(B, T, H, 2 * D, generator=gen).bfloat16()
    mix = torch.tril(torch.rand(8, 8, generator=gen).clamp(1e-5, 1))
    w = torch.rand(D, generator=gen) + 0.5
    # contiguous copies, through the runner: the forward checks and the identity with the composition
    y_ref, g_ref = run_fused(qkv[:, :, 0].contiguous(), qkv[:, :, 1].contiguous(), qkv[:, :, 2].contiguous(), mix, dyy[..., D:].contiguous(),
                             gg[:, :, 1].contiguous(), w, summaries)
    dqkv, dgg, dm, dw = leaves(qkv, gg, mix, w)
    dy = dyy.to(DEV)[..., D:]
    gate = dgg[:, :, 1]
    assert not gate.is_contiguous() and not dy.is_contiguous() and not dqkv[:, :, 0].is_contiguous()
    res = {}
    poison()
    ran = launches(lambda: res.__setitem__("y", mhla_amd.mhla_causal_normgate(dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2], dm, gate, dw, 1e-5,
                                                                              summaries=summaries)))
    assert ran.get(fused_kernel(D)) == 1, ran
    poison()
    res["y"].backward(dy)
    assert torch.equal(res["y"], y_ref), "y"
    got = {"dq": dqkv.grad[:, :, 0], "dk": dqkv.grad[:, :, 1], "dv": dqkv.grad[:, :, 2], "dmix": dm.grad, "dgate": dgg.grad[:, :, 1], "dweight": dw.grad}
    assert_same_gradients(got, g_ref, "views and contiguous copies")
    assert bool((dgg.grad[:, :, 0] == 0).all())   # (the buffer's other half takes no gradient)


# ---- 6. kept vs recomputed summaries -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [128, 512], ids=lambda V: f"V{V}")
@pytest.mark.parametrize("summaries", SUMMARIES)
def test_kept_summaries_match_recompute(summaries, V):
    """keep_state_limit=0 (the backward recomputes S and P) against the default (it reuses the fused forward's workspace)."""
    y_keep, g_keep = uniform_case(1, 200, 3, 64, V, summaries)
    y_re, g_re = uniform_case(1, 200, 3, 64, V, summaries, keep_state_limit=0)
    assert torch.equal(y_keep, y_re)
    assert_same_gradients(g_keep, g_re, "kept and recomputed summaries")


# ---- 7. shapes the epilogue does not cover -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,K,V,pack", [(torch.float16, 64, 64, False), (torch.float32, 64, 64, False), (torch.bfloat16, 64, 320, False),
                                            (torch.bfloat16, 48, 64, False), (torch.bfloat16, 64, 64, True)],
                         ids=["fp16", "fp32", "bf16-V320", "bf16-K48", "bf16-260-chunks"])
def test_shapes_outside_the_epilogue_compose(dtype, K, V, pack):
    """causal_normgate_fusable is False and the call is the explicit composition of the two HIP operators: y and every gradient bit
    for bit, no fused kernel in the launch profile (a pack of 260 chunks is outside by its chunk count, not by T)."""
    cu = tuple(range(0, 5 * 260 + 1, 5)) if pack else None
    B, T, H = (1, cu[-1], 2) if pack else (1, 200, 3)
    q, k, v, mix, do = causal_inputs(B, T, H, K, V, 8, dtype, seed=T + V)
    g, w = gate_and_weight(B, T, H, V, True, True, dtype)
    run_fused(q, k, v, mix, do, g, w, "tf32", cu=cu, fusable=False)


# ---- 8. packed sequences, single-bf16 summaries ------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [64, 256, 512], ids=lambda V: f"V{V}")
def test_packed_single_bf16_summaries(V):
    """The pack of test_gpu_causal_varlen.test_fused_normgate (lengths 1, 65, 0, 64, 191) through the chunk-table variants of the
    fused kernel at summaries="bf16"."""
    H, K, T = 2, 64, CU[-1]
    q, k, v, mix, do = causal_inputs(1, T, H, K, V, 4, torch.bfloat16, seed=T + V)
    g, w = gate_and_weight(1, T, H, V, True, True)
    run_fused(q, k, v, mix, do, g, w, "bf16", cu=CU)
