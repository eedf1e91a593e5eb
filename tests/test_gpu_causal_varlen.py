"""GPU parity of the causal operator over packed sequences (cu_seqlens): every sequence of the pack must come out exactly as if it
were alone in a call of its own.  Reference throughout: the fp32 oracle on each sequence's slice alone, concatenated; dmix summed
over the sequences.  Bounds: the derived ones of gpu_util / test_gpu_causal -- every chunk is the same arithmetic as in a uniform
call, so they carry over unchanged; outputs and token gradients are held to them chunk by chunk of every sequence (check_chunks on
the sequence's slice aligns with the sequence's own chunks)."""
import functools

import pytest
import torch

from gpu_util import (poison, DEV, OBSERVED, TOL_BF16SUM, GTOL_BF16SUM, CAUSAL_TOL, CAUSAL_CHUNK_TOL_H16, CAUSAL_DMIX_TOL, check,
                      check_chunks)
from oracle import mhla_oracle as orc
from test_gpu_causal import causal_inputs

pytestmark = pytest.mark.gpu

CU = (0, 1, 66, 66, 130, 321)   # lengths 1, 65, 0, 64, 191: 7 chunks; boundaries inside one workgroup's walk of four chunks


def seqs(cu):
    return [(a, b) for a, b in zip(cu, cu[1:]) if b > a]


def oracle_per_sequence(q, k, v, mix, do, cu, scale=None):
    """(out, dq, dk, dv, dmix): the fp32 oracle on every sequence alone, token tensors concatenated along the pack, dmix summed."""
    f = [t.float() for t in (q, k, v, do)]
    outs, gq, gk, gv, dmix = [], [], [], [], torch.zeros_like(mix)
    for a, b in seqs(cu):
        qs, ks, vs, ds = (t[:, a:b] for t in f)
        outs.append(orc.causal_fwd(qs, ks, vs, mix, scale=scale))
        g = orc.causal_bwd(qs, ks, vs, mix, ds, scale=scale)
        gq.append(g["dq"]); gk.append(g["dk"]); gv.append(g["dv"])
        dmix += g["dmix"]
    return torch.cat(outs, 1), torch.cat(gq, 1), torch.cat(gk, 1), torch.cat(gv, 1), dmix


@functools.lru_cache(maxsize=None)
def pack_case(cu, H, K, V, L, dtype, seed):
    """Seeded inputs of a pack (the project's causal_inputs recipe) and their per-sequence reference, computed once and shared."""
    q, k, v, mix, do = causal_inputs(1, cu[-1], H, K, V, L, dtype, seed)
    return (q, k, v, mix, do), oracle_per_sequence(q, k, v, mix, do, cu)


def tols(dtype, summaries, force_generic=False, generic_fallback=False):
    """(out, token gradients, dmix): CAUSAL_CHUNK_TOL_H16 at the default summaries of the 16-bit pipeline; CAUSAL_TOL for split,
    force_generic, fp32, fp16 and the generic fallback; the bf16-summaries bounds for summaries="bf16" (test_gpu_causal.causal_chunk_tols);
    dmix: CAUSAL_DMIX_TOL in every case."""
    if summaries == "bf16" and dtype == torch.bfloat16 and not (force_generic or generic_fallback):
        return TOL_BF16SUM[dtype], GTOL_BF16SUM[dtype], CAUSAL_DMIX_TOL[dtype]
    if summaries == "tf32" and dtype == torch.bfloat16 and not (force_generic or generic_fallback):
        return CAUSAL_CHUNK_TOL_H16[dtype], CAUSAL_CHUNK_TOL_H16[dtype], CAUSAL_DMIX_TOL[dtype]
    return CAUSAL_TOL[dtype], CAUSAL_TOL[dtype], CAUSAL_DMIX_TOL[dtype]


def check_per_sequence(name, got, want, cu, tol):
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert bool(torch.isfinite(got.float()).all()), f"{name}: non-finite rows (a row no chunk wrote?)"
    for i, (a, b) in enumerate(zip(cu, cu[1:])):
        if b > a:
            check_chunks(f"{name} seq {i} [{a}:{b}]", got[:, a:b], want[:, a:b], tol)


def run_varlen(cu, H, K, V, dtype, seed=1234, summaries="tf32", force_generic=False, generic_fallback=False, keep_state_limit=None,
               cu_as="list"):
    import mhla_amd
    cu = tuple(cu)
    L = max(2, max((b - a + 63) // 64 for a, b in zip(cu, cu[1:])))
    (q, k, v, mix, do), (want, wq, wk, wv, wm) = pack_case(cu, H, K, V, L, dtype, seed)
    dq, dk, dv, dm = (t.to(DEV).requires_grad_(True) for t in (q, k, v, mix.view(L, L, 1, 1, 1, 1)))
    given = {"list": list(cu), "tensor": torch.tensor(cu, dtype=torch.int32, device=DEV), "plan": mhla_amd.causal_varlen_plan(cu, DEV)}[cu_as]
    poison()
    out = mhla_amd.mhla_causal(dq, dk, dv, dm, summaries=summaries, force_generic=force_generic, keep_state_limit=keep_state_limit,
                               cu_seqlens=given)
    assert out.dtype == dtype and out.shape == (1, cu[-1], H, V)
    dod = do.to(DEV)
    poison()
    out.backward(dod)
    otol, gtol, mtol = tols(dtype, summaries, force_generic, generic_fallback)
    check_per_sequence("out", out, want, cu, otol)
    check_per_sequence("dq", dq.grad, wq, cu, gtol)
    check_per_sequence("dk", dk.grad, wk, cu, gtol)
    check_per_sequence("dv", dv.grad, wv, cu, gtol)
    assert dm.grad.shape == dm.shape
    check("dmix", dm.grad.reshape(L, L), wm, mtol)
    return out, (dq.grad, dk.grad, dv.grad, dm.grad)


# ---- 1. boundaries anywhere ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,summaries,force_generic", [(torch.bfloat16, "tf32", False), (torch.bfloat16, "split", False),
                                                            (torch.bfloat16, "bf16", False), (torch.bfloat16, "tf32", True),
                                                            (torch.float32, "tf32", False), (torch.float16, "tf32", False)])
def test_boundaries_anywhere(dtype, summaries, force_generic):
    """One-token, 65-token, empty, exactly-64 and 191-token sequences in one pack: sequence boundaries fall inside the walks of the
    summaries kernel (four chunks per workgroup) and of the output kernel, ragged chunks sit in the middle of the tensor."""
    run_varlen(CU, 2, 64, 64, dtype, summaries=summaries, force_generic=force_generic,
               cu_as="tensor" if dtype == torch.bfloat16 and summaries == "tf32" and not force_generic else "list")


@pytest.mark.parametrize("summaries", ["tf32", "split"])
def test_boundaries_anywhere_backward_recomputes_the_summaries(summaries):
    run_varlen(CU, 2, 64, 64, torch.bfloat16, summaries=summaries, keep_state_limit=0, cu_as="plan")


# ---- 2. head shapes of every token-kernel variant ---------------------------------------------------------------------------
@pytest.mark.parametrize("K,V", [(128, 256), (192, 192), (256, 128), (64, 512)])
@pytest.mark.parametrize("summaries", ["tf32", "split"])
def test_head_shapes(K, V, summaries):
    run_varlen((0, 100, 449), 2, K, V, torch.bfloat16, seed=K + V, summaries=summaries)


# ---- 3. chunk walk of the backward token kernel -----------------------------------------------------------------------------
def tok4_walk(most, n, bh):
    """csf_tok4_walk of capi_causal.hip: chunks per workgroup of k_csf_bwd_tok4."""
    cpw = 1
    while cpw * 2 <= most and ((n + cpw * 2 - 1) // (cpw * 2)) * bh >= 256:
        cpw *= 2
    return cpw


def test_backward_token_kernel_walks_across_sequence_boundaries():
    import mhla_amd
    H, lengths, cu = 8, (63, 65, 129, 1, 200), [0]
    while mhla_amd.causal_varlen_plan(cu, "cpu").n_chunks < 66:
        cu.append(cu[-1] + lengths[(len(cu) - 1) % len(lengths)])
    n = mhla_amd.causal_varlen_plan(cu, "cpu").n_chunks
    # K = 64 with the default summaries: up to CSF_TOK4_CPW = 8 chunks per workgroup (causal_bf16.hpp: csf_tok4_cpw<1, 2>)
    assert n >= 66 and tok4_walk(8, n, 1 * H) >= 2, (n, tok4_walk(8, n, H))
    run_varlen(cu, H, 64, 64, torch.bfloat16, seed=66)


# ---- 4. dispatch edges by chunk count ---------------------------------------------------------------------------------------
def test_130_chunks_two_launch_mixing_backward():
    run_varlen(tuple(range(0, 3 * 130 + 1, 3)), 2, 64, 64, torch.bfloat16, seed=130)


def test_260_chunks_fall_to_the_generic_kernels():
    import mhla_amd
    from mhla_amd import ops
    cu = tuple(range(0, 5 * 260 + 1, 5))
    plan = mhla_amd.causal_varlen_plan(cu, DEV)
    assert plan.n_chunks == 260
    z = torch.zeros(1, cu[-1], 2, 64, dtype=torch.bfloat16, device=DEV)
    assert not ops.causal_normgate_fusable(z, z, cu_seqlens=plan) and ops.causal_normgate_fusable(z, z)   # by chunk count, not by T
    run_varlen(cu, 2, 64, 64, torch.bfloat16, seed=260, generic_fallback=True, cu_as="plan")


# ---- 5. fused norm x gate ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [64, 256, 512])
@pytest.mark.parametrize("summaries", ["tf32", "split"])
def test_fused_normgate(V, summaries):
    """mhla_causal_normgate(cu_seqlens=) -- NV = 1, NV = 4 and the two-halves variant of the fused output kernel -- against
    oracle.rms_norm_swish_gate of the per-sequence operator, with the reference layer's dtype flow and the bounds of
    test_gpu_causal.run_normgate (derived there, restated here unchanged)."""
    import mhla_amd
    from mhla_amd import ops
    H, K, L, T, norm_eps = 2, 64, 4, CU[-1], 1e-5
    q, k, v, mix, do = causal_inputs(1, T, H, K, V, L, torch.bfloat16, seed=T + V)
    gen = torch.Generator().manual_seed(7)
    g = torch.randn(1, T, H, V, generator=gen).bfloat16()
    w = torch.rand(V, generator=gen) + 0.5

    class _R16(torch.autograd.Function):   # the operator returns o in the activation dtype and receives a bf16 do (run_normgate)
        @staticmethod
        def forward(ctx, x):
            return x.bfloat16().float()

        @staticmethod
        def backward(ctx, g):
            return g.bfloat16().float()

    ref = [t.float().clone().requires_grad_(True) for t in (q, k, v, mix)]
    gr, wr = g.float().clone().requires_grad_(True), w.clone().requires_grad_(True)
    o_exact = torch.cat([orc.causal_fwd(ref[0][:, a:b], ref[1][:, a:b], ref[2][:, a:b], ref[3]) for a, b in seqs(CU)], 1)
    y_ref = orc.rms_norm_swish_gate(_R16.apply(o_exact), gr, wr, norm_eps)
    (y_ref * do.float()).sum().backward()

    dev = [t.to(DEV).requires_grad_(True) for t in (q, k, v, mix)]
    gd, wd = g.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    plan = mhla_amd.causal_varlen_plan(CU, DEV)
    assert ops.causal_normgate_fusable(dev[0], dev[2], cu_seqlens=plan)
    poison()
    y = mhla_amd.mhla_causal_normgate(dev[0], dev[1], dev[2], dev[3], gd, wd, norm_eps, summaries=summaries, cu_seqlens=plan)
    assert y.dtype == torch.bfloat16 and y.shape == (1, T, H, V)
    poison()
    y.backward(do.to(DEV))
    u = 2.0 ** -8
    extra = 2e-3 if summaries == "tf32" else 0.0
    with torch.no_grad():
        check("y vs exact composition", y, orc.rms_norm_swish_gate(o_exact, gr, wr, norm_eps), 2 * u + 1e-3)
    check("y", y, y_ref.detach(), 3 * u + 1e-3)
    for name, a, b in zip(("dq", "dk", "dv"), dev, ref):
        check(name, a.grad, b.grad, u + 2e-3 + extra)
    check("dmix", dev[3].grad, ref[3].grad, 2e-3 + 2 * extra)
    check("dgate", gd.grad, gr.grad, u + 2e-3 + extra)
    check("dweight", wd.grad, wr.grad, 2e-3 + extra)
    with torch.no_grad():   # inference (o is not stored) and the unfused composition of the two HIP operators
        y3 = mhla_amd.mhla_causal_normgate(dev[0], dev[1], dev[2], dev[3], gd, wd, norm_eps, summaries=summaries, cu_seqlens=plan)
        y2 = mhla_amd.rmsnorm_gate(mhla_amd.mhla_causal(dev[0], dev[1], dev[2], dev[3], summaries=summaries, cu_seqlens=plan), gd, wd, norm_eps)
    check("inference vs training path", y3, y.detach().float().cpu(), 1e-6)
    check("fused vs unfused", y3, y2.float().cpu(), 3 * u + 1e-3)


# ---- 6. isolation, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("summaries,force_generic", [("tf32", False), ("split", False), ("tf32", True)])
def test_isolation_bit_for_bit(summaries, force_generic):
    """What a sequence gets depends on its own tokens only: other values in sequence 1 leave every other sequence's rows of `out`
    bit-identical, a loss over sequence 3 alone leaves every other sequence's token gradients identically zero, and two runs on the
    same inputs are bit-identical.  Outputs and gradients are allocated over NaN: a skipped row shows."""
    import mhla_amd
    H, K, V, L = 2, 64, 64, 4
    q, k, v, mix, do = causal_inputs(1, CU[-1], H, K, V, L, torch.bfloat16, seed=6)
    q2, k2, v2, _, _ = causal_inputs(1, CU[-1], H, K, V, L, torch.bfloat16, seed=7)
    a1, b1 = CU[1], CU[2]
    a3, b3 = CU[3], CU[4]
    plan = mhla_amd.causal_varlen_plan(CU, DEV)

    def run(q, k, v, do):
        dq, dk, dv, dm = (t.to(DEV).requires_grad_(True) for t in (q, k, v, mix))
        poison()
        out = mhla_amd.mhla_causal(dq, dk, dv, dm, summaries=summaries, force_generic=force_generic, cu_seqlens=plan)
        poison()
        out.backward(do.to(DEV))
        return out.detach(), dq.grad, dk.grad, dv.grad, dm.grad

    base = run(q, k, v, do)
    again = run(q, k, v, do)
    for name, x, y in zip(("out", "dq", "dk", "dv", "dmix"), base, again):
        assert bool(torch.isfinite(x.float()).all()), f"{name}: non-finite"
        assert torch.equal(x, y), f"{name}: two runs on the same inputs differ"
    qm, km, vm = q.clone(), k.clone(), v.clone()
    for t, s in ((qm, q2), (km, k2), (vm, v2)):
        t[:, a1:b1] = s[:, a1:b1]
    other = run(qm, km, vm, do)
    keep = torch.ones(CU[-1], dtype=torch.bool)
    keep[a1:b1] = False
    for name, x, y in zip(("out", "dq", "dk", "dv"), base, other):
        assert torch.equal(x[:, keep], y[:, keep]), f"{name}: rows of other sequences changed with sequence 1's values"
        assert not torch.equal(x[:, a1:b1], y[:, a1:b1]), f"{name}: sequence 1 did not change with its values"
    do3 = torch.zeros_like(do)
    do3[:, a3:b3] = do[:, a3:b3]
    _, gq, gk, gv, _ = run(q, k, v, do3)
    outside = torch.ones(CU[-1], dtype=torch.bool)
    outside[a3:b3] = False
    for name, x in (("dq", gq), ("dk", gk), ("dv", gv)):
        assert bool((x[:, outside] == 0).all()), f"{name}: a loss over sequence 3 reached another sequence's rows"
        assert bool((x[:, a3:b3] != 0).any()), f"{name}: no gradient on sequence 3"


# ---- 7. one sequence is the uniform operator --------------------------------------------------------------------------------
@pytest.mark.parametrize("summaries", ["tf32", "split"])
def test_one_sequence_is_the_uniform_operator(summaries):
    import os
    import mhla_amd
    cu = (0, 321)
    out, grads = run_varlen(cu, 2, 64, 64, torch.bfloat16, summaries=summaries)
    (q, k, v, mix, do), _ = pack_case(cu, 2, 64, 64, 6, torch.bfloat16, 1234)
    dq, dk, dv, dm = (t.to(DEV).requires_grad_(True) for t in (q, k, v, mix.view(6, 6, 1, 1, 1, 1)))
    uni = mhla_amd.mhla_causal(dq, dk, dv, dm, summaries=summaries)
    uni.backward(do.to(DEV))
    pairs = list(zip(("out", "dq", "dk", "dv", "dmix"), (out,) + grads, (uni, dq.grad, dk.grad, dv.grad, dm.grad)))
    same = all(torch.equal(a, b) for _, a, b in pairs)
    worst = max(float((a.detach().float() - b.detach().float()).abs().max()) for _, a, b in pairs)
    OBSERVED.append((os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], f"varlen one sequence vs uniform call: bit-equal={same}",
                     "bfloat16", worst, 0.0, 0.0, 0.0))
    otol, gtol, mtol = tols(torch.bfloat16, summaries)   # the tolerances of case 1, chunk by chunk; dmix: CAUSAL_DMIX_TOL
    for name, a, b in pairs[:4]:
        check_chunks(f"{name} varlen vs uniform", a, b.detach().float().cpu(), otol if name == "out" else gtol)
    check("dmix varlen vs uniform", pairs[4][1].reshape(6, 6), pairs[4][2].detach().float().cpu().reshape(6, 6), mtol)


# ---- 8. strided views -------------------------------------------------------------------------------------------------------
def test_strided_views_of_one_projection():
    """q, k, v as slices of one packed [1, T, H, 3 * 64] projection (strides multiples of 8: used in place)."""
    import mhla_amd
    T, H, D, L = CU[-1], 2, 64, 4
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(1, T, H, 3 * D, generator=g).bfloat16()
    mix = torch.tril(torch.rand(L, L, generator=g).clamp(1e-5, 1))
    do = torch.randn(1, T, H, D, generator=g).bfloat16()
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    want, wq, wk, wv, wm = oracle_per_sequence(q, k, v, mix, do, CU)
    dqkv = qkv.to(DEV).requires_grad_(True)
    dm = mix.to(DEV).requires_grad_(True)
    poison()
    out = mhla_amd.mhla_causal(dqkv[..., :D], dqkv[..., D:2 * D], dqkv[..., 2 * D:], dm, cu_seqlens=list(CU))
    poison()
    out.backward(do.to(DEV))
    otol, gtol, mtol = tols(torch.bfloat16, "tf32")
    check_per_sequence("out", out, want, CU, otol)
    for i, (n, wgt) in enumerate((("dq", wq), ("dk", wk), ("dv", wv))):
        check_per_sequence(n, dqkv.grad[..., i * D:(i + 1) * D], wgt, CU, gtol)
    check("dmix", dm.grad, wm, mtol)


# ---- 9. layer ---------------------------------------------------------------------------------------------------------------
def test_layer_isolates_sequences():
    """MHLA(isolate_sequences=True) on a left-padded batch (attention_mask) and on the same tokens packed (cu_seqlens): row for row the
    module on each sequence alone at B = 1, within the bound test_gpu_modules holds the layer to against oracle.fla_layer_forward
    (fp32 module, 1e-4); isolate_sequences=False is the layer without the flag, bit for bit."""
    import mhla_amd
    from mhla_amd import modules
    kw = dict(mode="chunk", hidden_size=256, expand_k=0.5, expand_v=1.0, num_heads=2, feature_map="relu", norm_eps=1e-6)
    torch.manual_seed(3)
    m = modules.MHLA(isolate_sequences=True, **kw)
    with torch.no_grad():
        m.g_norm_swish_gate.weight.uniform_(0.5, 1.5)
        m.mixing_matrix.copy_(torch.rand(32, 32).view(32, 32, 1, 1, 1, 1))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    lens, T = (37, 100), 100
    x = torch.randn(2, T, 256)
    mask = torch.zeros(2, T, dtype=torch.long)
    for b, n in enumerate(lens):
        mask[b, T - n:] = 1
    m = m.to(DEV)
    xd = x.to(DEV)
    with torch.no_grad():
        alone = [m(xd[b:b + 1, T - n:])[0] for b, n in enumerate(lens)]
        for b, n in enumerate(lens):   # (and the oracle's restatement of the layer on the sequence alone, the same bound)
            check(f"alone seq {b} vs oracle", alone[b], orc.fla_layer_forward(sd, x[b:b + 1, T - n:], 2, 64, 128, norm_eps=1e-6), 1e-4)
        padded = m(xd, attention_mask=mask.to(DEV))[0]
        packed_x = torch.cat([xd[b, T - n:] for b, n in enumerate(lens)], 0).unsqueeze(0)
        cu = torch.tensor([0, lens[0], lens[0] + lens[1]], dtype=torch.int32, device=DEV)
        packed = m(packed_x, cu_seqlens=cu)[0]
        planned = m(packed_x, cu_seqlens=cu, varlen_plan=mhla_amd.causal_varlen_plan(cu))[0]
    assert padded.shape == (2, T, 256) and packed.shape == (1, sum(lens), 256)
    assert torch.equal(planned, packed)
    assert bool((padded[0, :T - lens[0]] == 0).all())
    off = 0
    for b, n in enumerate(lens):
        check(f"padded seq {b}", padded[b:b + 1, T - n:], alone[b].float().cpu(), 1e-4)
        check(f"packed seq {b}", packed[:, off:off + n], alone[b].float().cpu(), 1e-4)
        off += n
    # calls of <= 64 tokens (the layer's token-recurrent branch otherwise): the chunk operator over the pack, no recurrent state
    with torch.no_grad():
        short = m(xd[:, -50:], attention_mask=mask[:, -50:].to(DEV))[0]   # lengths 37 and 50, left-padded to 50
        for b, n in enumerate((37, 50)):
            check(f"short padded seq {b}", short[b:b + 1, 50 - n:], m(xd[b:b + 1, T - n:])[0].float().cpu(), 1e-4)
    # gradients flow through the plan's effective matrix into the layer's parameter
    xg = packed_x.clone().requires_grad_(True)
    m(xg, cu_seqlens=cu)[0].square().sum().backward()
    gm = m.mixing_matrix.grad.reshape(32, 32)
    assert bool(torch.isfinite(gm).all()) and bool((gm[:2, :2].tril() != 0).any()) and bool((gm[2:] == 0).all())   # 100 tokens: rows 0, 1
    # the flag off: the parent behaviour (the pack as one sequence), bit for bit
    plain, off_flag = modules.MHLA(**kw).to(DEV), modules.MHLA(isolate_sequences=False, **kw).to(DEV)
    plain.load_state_dict(m.state_dict())
    off_flag.load_state_dict(m.state_dict())
    with torch.no_grad():
        assert torch.equal(off_flag(xd, attention_mask=mask.to(DEV))[0], plain(xd, attention_mask=mask.to(DEV))[0])
        assert torch.equal(off_flag(packed_x, cu_seqlens=cu)[0], plain(packed_x, cu_seqlens=cu)[0])
        mixed = plain(packed_x, cu_seqlens=cu)[0]
    assert not torch.equal(mixed[:, lens[0]:], packed[:, lens[0]:])   # (without the flag sequence 1 sees sequence 0)



def test_layer_bf16_takes_the_fused_varlen_node(monkeypatch):
    """A bf16 layer with isolate_sequences hands the pack to the fused norm x gate node (_CausalNormGate with the pack's plan), padded batch and
    explicit cu_seqlens alike.  What the layer passed to the operator is recorded, and the operator's y is held to
    oracle.rms_norm_swish_gate of the per-sequence oracle on exactly those tensors, with the reference layer's rounding of o:
    3u + 1e-3, the bound of test_fused_normgate / test_gpu_causal.run_normgate for this quantity."""
    from mhla_amd import modules, ops
    from mhla_amd.modules import fla
    torch.manual_seed(3)
    m = modules.MHLA(mode="chunk", hidden_size=256, expand_k=0.5, expand_v=1.0, num_heads=2, feature_map="relu", norm_eps=1e-6,
                     isolate_sequences=True)
    with torch.no_grad():
        m.g_norm_swish_gate.weight.uniform_(0.5, 1.5)
        m.mixing_matrix.copy_(torch.rand(32, 32).view(32, 32, 1, 1, 1, 1))
    m = m.to(DEV).bfloat16()
    lens, T = (37, 100), 100
    x = torch.randn(2, T, 256).bfloat16().to(DEV)
    mask = torch.zeros(2, T, dtype=torch.long)
    for b, n in enumerate(lens):
        mask[b, T - n:] = 1
    seen, nodes = [], []
    real_op, real_apply = fla.mhla_causal_normgate, ops._CausalNormGate.apply

    def recording_op(q, k, v, mix, g, w, eps, **kw):
        y = real_op(q, k, v, mix, g, w, eps, **kw)
        seen.append((q, k, v, mix, g, w, eps, kw["cu_seqlens"], y))
        return y

    def counting_apply(*a):
        nodes.extend(1 for x in a if isinstance(x, ops.CausalVarlenPlan))   # (the node's plan argument: None for a uniform call)
        return real_apply(*a)
    monkeypatch.setattr(fla, "mhla_causal_normgate", recording_op)
    monkeypatch.setattr(ops._CausalNormGate, "apply", counting_apply)
    packed_x = torch.cat([x[b, T - n:] for b, n in enumerate(lens)], 0).unsqueeze(0)
    cu = torch.tensor([0, lens[0], lens[0] + lens[1]], dtype=torch.int32, device=DEV)
    with torch.no_grad():
        poison()
        padded = m(x, attention_mask=mask.to(DEV))[0]
        poison()
        packed = m(packed_x, cu_seqlens=cu)[0]
    assert len(seen) == 2 and len(nodes) == 2, (len(seen), len(nodes))   # the fused node both times, not the unfused composition
    assert padded.dtype == torch.bfloat16 and bool(torch.isfinite(packed.float()).all())
    assert torch.equal(torch.cat([padded[b, T - n:] for b, n in enumerate(lens)], 0), packed[0])   # the same pack either way
    assert bool((padded[0, :T - lens[0]] == 0).all())
    q, k, v, mix, g, w, eps, plan, y = seen[1]
    assert plan.cu == (0, 37, 137) and q.dtype == torch.bfloat16 and q.shape == (1, 137, 2, 64) and v.shape == (1, 137, 2, 128)
    qf, kf, vf, gf = (t.float().cpu() for t in (q, k, v, g))
    mixf = mix.detach().float().cpu().reshape(32, 32)
    o = torch.cat([orc.causal_fwd(qf[:, a:b], kf[:, a:b], vf[:, a:b], mixf) for a, b in seqs(plan.cu)], 1)
    want = orc.rms_norm_swish_gate(o.bfloat16().float(), gf, w.detach().float().cpu(), eps)
    check("layer's fused y", y, want, 3 * 2.0 ** -8 + 1e-3)


def test_host_builds_the_plan_once_for_all_layers(monkeypatch):
    """GPT_MHLA(isolate_sequences=True): one plan per forward, made by the host and used as is by every layer; padded and packed
    batches give every sequence the logits it gets alone.  Bound: two layers, each held to 1e-4 of its output (test_gpu_modules),
    and as much again for the eager norms, MLPs and head that carry those perturbations on: 4e-4."""
    from mhla_amd.hosts import gpt as host
    from mhla_amd.modules import fla
    made = {"host": 0, "layer": 0}

    def counting(where, fn):
        def wrapped(*a, **kw):
            made[where] += 1
            return fn(*a, **kw)
        return wrapped
    monkeypatch.setattr(host, "causal_varlen_plan", counting("host", host.causal_varlen_plan))
    monkeypatch.setattr(fla, "causal_varlen_plan", counting("layer", fla.causal_varlen_plan))
    lens, T = (37, 100), 100
    mask = torch.zeros(2, T, dtype=torch.long)
    for b, n in enumerate(lens):
        mask[b, T - n:] = 1
    cu = torch.tensor([0, lens[0], lens[0] + lens[1]], dtype=torch.int32, device=DEV)
    torch.manual_seed(4)
    gpt = host.GPT_MHLA(vocab_size=64, hidden_size=256, num_layers=2, num_heads=2, max_seq_len=256, isolate_sequences=True).to(DEV)
    ids = torch.randint(0, 64, (2, T), device=DEV)
    with torch.no_grad():
        lp = gpt(ids, attention_mask=mask.to(DEV))
        assert made == {"host": 1, "layer": 0}, made
        packed_ids = torch.cat([ids[b, T - n:] for b, n in enumerate(lens)], 0).unsqueeze(0)
        lk = gpt(packed_ids, cu_seqlens=cu)
        assert made == {"host": 2, "layer": 0}, made
        la = [gpt(ids[b:b + 1, T - n:]) for b, n in enumerate(lens)]
        assert made == {"host": 2, "layer": 0}, made
    off = 0
    for b, n in enumerate(lens):
        check(f"gpt padded seq {b}", lp[b:b + 1, T - n:], la[b].float().cpu(), 4e-4)
        check(f"gpt packed seq {b}", lk[:, off:off + n], la[b].float().cpu(), 4e-4)
        off += n
