"""Grouped-query heads in the causal operator's forward: k, v with Hkv heads, q (gate, out, y) with H = G Hkv, query head h on
k/v head h // G.  The claim is derivable and gets no tolerance: the grouped call returns, bit for bit, what the same call returns on
k, v repeated G times per head -- the chunk summaries and their prefix mixes are the same sums in the same order whatever the number
of (b, head) pairs, and the output kernel's arithmetic per query head is the plain kernel's.  One case against the fp64 oracle keeps
the two paths from being wrong together in the indexing."""
import pytest
import torch

from gpu_util import DEV, TOL, causal_fp64, check_chunks, launches, poison

pytestmark = pytest.mark.gpu

T330 = 330   # six chunks: more than one walk of the plain output kernel's workgroups, last chunk 10 rows
CU = [0, 70, 70, 199, 330]   # an empty sequence, ragged last chunks


def rep(t, G):
    return t.repeat_interleave(G, 2)


def inputs(B, T, H, Hk, K, V, dtype, seed=None, L=8):
    """q [B, T, H, K], k [B, T, Hk, K], v [B, T, Hk, V], gate [B, T, H, V], a random lower-triangular mixing matrix, on the device:
    every head drawn on its own, so query heads differ within a group and k/v heads from each other."""
    g = torch.Generator().manual_seed(1000 * H + 100 * Hk + K + V + T if seed is None else seed)
    signed = lambda *s: torch.relu(torch.randn(*s, generator=g)) * torch.sign(torch.randn(*s, generator=g))
    q, k = signed(B, T, H, K), signed(B, T, Hk, K)
    v, gate = torch.randn(B, T, Hk, V, generator=g), torch.randn(B, T, H, V, generator=g)
    mix = torch.tril(torch.rand(L, L, generator=g).clamp(1e-5, 1))
    return tuple(t.to(dtype).to(DEV) for t in (q, k, v, gate)) + (mix.to(DEV),)


def same_bits(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, f"{name}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}"
    assert not torch.isnan(got).any(), f"{name}: NaN in the grouped result"
    if not torch.equal(got, want):
        d = (got.float() - want.float()).abs()
        raise AssertionError(f"{name}: {int((got != want).sum())} of {got.numel()} elements differ from the repeated-head call "
                             f"(largest difference {d.max().item():.3e}, first at {tuple(int(i) for i in (got != want).nonzero()[0])})")


def grouped_and_repeated(fn, q, k, v, *rest, **kw):
    """fn on the un-repeated k, v and on k, v repeated per head; no graph in either."""
    G = q.shape[2] // k.shape[2]
    with torch.no_grad():
        poison()
        got = fn(q, k, v, *rest, **kw)
        poison()
        want = fn(q, rep(k, G), rep(v, G), *rest, **kw)
    return got, want


@pytest.mark.parametrize("summaries", ["tf32", "split", "bf16"])
@pytest.mark.parametrize("K,V", [(64, 64), (128, 128), (64, 192), (128, 256)], ids=lambda x: str(x))
@pytest.mark.parametrize("H,Hk", [(4, 2), (8, 1), (6, 2)])
def test_pipeline_equals_the_repeated_head_call(H, Hk, K, V, summaries):
    import mhla_amd
    q, k, v, _, mix = inputs(2, T330, H, Hk, K, V, torch.bfloat16)
    got, want = grouped_and_repeated(mhla_amd.mhla_causal, q, k, v, mix, summaries=summaries)
    same_bits(f"H={H} Hkv={Hk} K={K} V={V} {summaries}", got, want)


@pytest.mark.parametrize("summaries", ["tf32", "split", "bf16"])
@pytest.mark.parametrize("V", [64, 128, 192, 256, 384, 512])
def test_fused_normgate_equals_the_repeated_head_call(V, summaries):
    import mhla_amd
    from mhla_amd import ops
    q, k, v, gate, mix = inputs(2, T330, 4, 2, 64, V, torch.bfloat16)
    w = (torch.rand(V, generator=torch.Generator().manual_seed(V)) + 0.5).to(DEV)
    assert ops.causal_normgate_fusable(q, v, flags=ops._causal_flags(summaries, False))
    got, want = grouped_and_repeated(mhla_amd.mhla_causal_normgate, q, k, v, mix, gate, w, 1e-5, summaries=summaries)
    same_bits(f"V={V} {summaries}", got, want)
    if V == 128 or V == 512:
        got, want = grouped_and_repeated(mhla_amd.mhla_causal_normgate, q, k, v, mix, None, None, 1e-5, summaries=summaries)
        same_bits(f"V={V} {summaries} without gate and weight", got, want)


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("H,Hk,K,V", [(4, 2, 64, 128), (6, 2, 128, 256), (8, 1, 64, 384)])
def test_packed_sequences_equal_the_repeated_head_call(H, Hk, K, V, fused):
    import mhla_amd
    if V == 384 and not fused:
        V = 192
    q, k, v, gate, mix = inputs(1, CU[-1], H, Hk, K, V, torch.bfloat16)
    plan = mhla_amd.causal_varlen_plan(CU, DEV)
    if fused:
        w = torch.linspace(0.5, 1.5, V, device=DEV)
        got, want = grouped_and_repeated(mhla_amd.mhla_causal_normgate, q, k, v, mix, gate, w, 1e-5, cu_seqlens=plan)
    else:
        got, want = grouped_and_repeated(mhla_amd.mhla_causal, q, k, v, mix, cu_seqlens=plan)
    same_bits(f"pack H={H} Hkv={Hk} V={V}", got, want)


GENERIC = [("fp32", torch.float32, 40, 24, {}), ("fp16", torch.float16, 64, 64, {}), ("bf16-forced", torch.bfloat16, 64, 64, {"force_generic": True})]


@pytest.mark.parametrize("name,dtype,K,V,kw", GENERIC, ids=[c[0] for c in GENERIC])
def test_generic_path_equals_the_repeated_head_call(name, dtype, K, V, kw):
    import mhla_amd
    q, k, v, _, mix = inputs(2, 130, 4, 1, K, V, dtype)
    got, want = grouped_and_repeated(mhla_amd.mhla_causal, q, k, v, mix, **kw)
    same_bits(name, got, want)
    names = launches(lambda: mhla_amd.mhla_causal(q, k, v, mix, **kw))
    assert names.get("k_cs_out<gqa>") == 1 and "k_cs_out" not in names and names.get("k_bm_state<2>") == 1, names


def test_generic_path_packed():
    import mhla_amd
    q, k, v, _, mix = inputs(1, 130, 4, 1, 40, 24, torch.float32)
    got, want = grouped_and_repeated(mhla_amd.mhla_causal, q, k, v, mix, cu_seqlens=[0, 50, 50, 130])
    same_bits("generic pack", got, want)
    names = launches(lambda: mhla_amd.mhla_causal(q, k, v, mix, cu_seqlens=[0, 50, 50, 130]))
    assert names.get("k_cs_out<tab,gqa>") == 1 and "k_cs_out<tab>" not in names, names


def test_launch_names_tell_the_grouped_output_kernel():
    import mhla_amd
    q, k, v, gate, mix = inputs(1, 130, 4, 2, 64, 64, torch.bfloat16)
    with torch.no_grad():
        grouped = launches(lambda: mhla_amd.mhla_causal(q, k, v, mix))
        plain = launches(lambda: mhla_amd.mhla_causal(q, rep(k, 2), rep(v, 2), mix))
        same = launches(lambda: mhla_amd.mhla_causal(q[:, :, :2], k, v, mix))   # Hkv == H
        fused = launches(lambda: mhla_amd.mhla_causal_normgate(q, k, v, mix, gate, None))
        packed = launches(lambda: mhla_amd.mhla_causal(q, k, v, mix, cu_seqlens=[0, 70, 130]))
    assert grouped == {"k_csf_state": 1, "k_csf_mixf": 1, "k_csf_out4<gqa>": 1}, grouped
    assert plain == same == {"k_csf_state": 1, "k_csf_mixf": 1, "k_csf_out4": 1}, (plain, same)
    assert fused == {"k_csf_state": 1, "k_csf_mixf": 1, "k_csf_out4<norm,gqa>": 1}, fused
    assert packed == {"k_csf_state<tab>": 1, "k_csf_mixf": 1, "k_csf_out4<tab,gqa>": 1}, packed


@pytest.mark.parametrize("dtype,K,V,cu", [(torch.bfloat16, 128, 256, None), (torch.bfloat16, 64, 64, CU), (torch.float32, 40, 24, None)],
                         ids=["pipeline", "pipeline-pack", "generic"])
def test_workspace_is_sized_by_the_kv_heads(dtype, K, V, cu, monkeypatch):
    import mhla_amd
    from mhla_amd import ops
    B, T, H, Hk = (2, T330, 8, 2) if cu is None else (1, CU[-1], 8, 2)
    q, k, v, _, mix = inputs(B, T, H, Hk, K, V, dtype)
    asked = []
    real = ops._ws
    monkeypatch.setattr(ops, "_ws", lambda nbytes, device: (asked.append(nbytes), real(nbytes, device))[1])
    with torch.no_grad():
        poison()
        out = mhla_amd.mhla_causal(q, k, v, mix, cu_seqlens=cu)
    assert not torch.isnan(out).any()
    n_chunks = None if cu is None else mhla_amd.causal_varlen_plan(cu, DEV).n_chunks
    by_kv = ops._cs_plan(B, T, Hk, K, V, 64, ops._dtype_code(q), 0, n_chunks)[0]
    by_q = ops._cs_plan(B, T, H, K, V, 64, ops._dtype_code(q), 0, n_chunks)[0]
    assert asked == [by_kv] and by_kv < by_q and abs(by_q / by_kv - H // Hk) < 0.01, (asked, by_kv, by_q)


def test_batch_slices_are_sized_by_the_query_heads(monkeypatch):
    import mhla_amd
    from mhla_amd import ops
    H, Hk = 4, 2
    q, k, v, _, mix = inputs(3, 130, H, Hk, 64, 64, torch.bfloat16)
    with torch.no_grad():
        poison()
        whole = mhla_amd.mhla_causal(q, k, v, mix)
        monkeypatch.setattr(ops, "_MAX_GRID_BH", H * 1)
        poison()
        names = launches(lambda: same_bits("sliced", mhla_amd.mhla_causal(q, k, v, mix), whole))
    assert names.get("k_csf_out4<gqa>") == 3, names


def test_against_the_fp64_oracle():
    """The grouped call itself against the fp64 operator on explicitly repeated heads, every chunk at the operator's tolerance (one
    final rounding + 1e-3): bf16 pipeline at the default summaries, and the generic fp32 kernels."""
    import mhla_amd
    for dtype, K, V in ((torch.bfloat16, 64, 128), (torch.float32, 40, 24)):
        H, Hk = 6, 2
        q, k, v, _, mix = inputs(2, T330, H, Hk, K, V, dtype)
        assert not torch.equal(q[:, :, 0], q[:, :, 1]) and not torch.equal(k[:, :, 0], k[:, :, 1])
        with torch.no_grad():
            poison()
            out = mhla_amd.mhla_causal(q, k, v, mix)
        qc, kc, vc = q.cpu(), rep(k, 3).cpu(), rep(v, 3).cpu()
        want = causal_fp64(qc, kc, vc, mix.cpu(), torch.zeros_like(vc))["out"]
        check_chunks(f"gqa out {dtype}", out, want, TOL[dtype])


def test_gradient_path():
    """With a gradient to compute, k and v are expanded inside the graph and the repeated-head nodes run: the forward's bits are the
    native grouped forward's, dk and dv come back on the k/v heads, and every gradient equals that of an explicit expand-then-call."""
    import mhla_amd
    H, Hk, G = 4, 2, 2
    q, k, v, _, mix = inputs(2, 200, H, Hk, 64, 128, torch.bfloat16)
    do = torch.randn(2, 200, H, 128, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).to(DEV)
    with torch.no_grad():
        poison()
        native = mhla_amd.mhla_causal(q, k, v, mix)

    def leaves():
        return [t.detach().clone().requires_grad_(True) for t in (q, k, v, mix)]

    q1, k1, v1, m1 = leaves()
    poison()
    names = launches(lambda: same_bits("forward with a graph", mhla_amd.mhla_causal(q1, k1, v1, m1).detach(), native))
    assert "k_csf_out4" in names and "k_csf_out4<gqa>" not in names, names
    poison()
    mhla_amd.mhla_causal(q1, k1, v1, m1).backward(do)
    q2, k2, v2, m2 = leaves()
    B, T = k2.shape[:2]
    ke = k2[:, :, :, None, :].expand(B, T, Hk, G, 64).reshape(B, T, H, 64)
    ve = v2[:, :, :, None, :].expand(B, T, Hk, G, 128).reshape(B, T, H, 128)
    poison()
    mhla_amd.mhla_causal(q2, ke, ve, m2).backward(do)
    assert k1.grad.shape == k.shape and v1.grad.shape == v.shape
    for name, a, b in (("dq", q1, q2), ("dk", k1, k2), ("dv", v1, v2), ("dmix", m1, m2)):
        same_bits(name, a.grad, b.grad)
    # grad mode on, nothing requires one: the native forward
    names = launches(lambda: same_bits("nothing requires grad", mhla_amd.mhla_causal(q, k, v, mix), native))
    assert "k_csf_out4<gqa>" in names, names


def _state_bits(name, got, want, lengths, T):
    assert got.S.shape == want.S.shape and got.seen == want.seen and got.lengths == want.lengths, name
    assert torch.equal(got.P, want.P) and torch.equal(got.Cur, want.Cur) and not torch.isnan(got.P).any() and not torch.isnan(got.Cur).any(), name
    for b, n in enumerate(lengths if lengths is not None else [T] * got.S.shape[0]):
        assert torch.equal(got.S[b, :, :n // 64], want.S[b, :, :n // 64]), f"{name}: sequence {b}: a finished chunk differs"


@pytest.mark.parametrize("form", ["uniform", "lengths", "cu_seqlens"])
def test_prefill_takes_the_kv_heads(form):
    """`o` is the repeated-head operator's, the state that of mhla_causal_state on the un-repeated k, v; no repeated-head output launch."""
    import mhla_amd
    H, Hk, G, K, V = 4, 2, 2, 64, 64
    lengths = [37, 100]
    B, T = (2, 100) if form != "cu_seqlens" else (1, CU[-1])
    q, k, v, _, mix = inputs(B, T, H, Hk, K, V, torch.bfloat16)
    kw = {"uniform": {}, "lengths": dict(lengths=lengths, left_padded=True), "cu_seqlens": dict(cu_seqlens=CU)}[form]
    got = []
    with torch.no_grad():
        poison()
        names = launches(lambda: got.extend(mhla_amd.mhla_causal_prefill(q, k, v, mix, **kw)))
        o, state = got
        poison()
        if form == "lengths":
            want = torch.zeros_like(o)
            for b, n in enumerate(lengths):
                want[b:b + 1, T - n:] = mhla_amd.mhla_causal(q[b:b + 1, T - n:], rep(k, G)[b:b + 1, T - n:], rep(v, G)[b:b + 1, T - n:], mix)
        else:
            want = mhla_amd.mhla_causal(q, rep(k, G), rep(v, G), mix, **kw)
        poison()
        want_state = mhla_amd.mhla_causal_state(k, v, mix, **kw)
    same_bits(f"prefill {form}", o, want)
    assert state.S.shape[1] == Hk
    per_seq = lengths if form == "lengths" else [b - a for a, b in zip(CU, CU[1:])] if form == "cu_seqlens" else None
    _state_bits(f"prefill {form}", state, want_state, per_seq, T)
    out_names = {n for n in names if n.startswith("k_csf_out4") or n.startswith("k_cs_out")}
    assert out_names and all("gqa" in n for n in out_names), names


def _layers(dtype):
    from mhla_amd import modules
    torch.manual_seed(5)
    mk = lambda grouped: modules.MHLA(mode="chunk", hidden_size=512, expand_k=0.5, expand_v=1.0, num_heads=4, num_kv_heads=2,
                                      feature_map="relu", norm_eps=1e-6, layer_idx=0, exact_decoding=True, grouped_state=grouped)
    plain, grouped = mk(False), mk(True)
    with torch.no_grad():
        plain.g_norm_swish_gate.weight.uniform_(0.5, 1.5)
        plain.mixing_matrix.copy_(torch.rand(32, 32).view(32, 32, 1, 1, 1, 1))
    grouped.load_state_dict(plain.state_dict())
    return plain.to(DEV).to(dtype).eval(), grouped.to(DEV).to(dtype).eval()


def test_fla_layer_exact_decoding():
    """MHLA(grouped_state=True), K = 64, V = 128: the prefill (fused norm x gate in the grouped output kernel) and three steps are
    bit for bit those of grouped_state=False, whose prefill repeats the heads."""
    from mhla_amd import modules
    plain, grouped = _layers(torch.bfloat16)
    x = torch.randn(2, 73, 512, generator=torch.Generator().manual_seed(23)).to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        cp, cg = modules.DecodeCache(), modules.DecodeCache()
        for a, b in [(0, 70), (70, 71), (71, 72), (72, 73)]:
            outs = []
            poison()
            op = plain(x[:, a:b], past_key_values=cp, use_cache=True)[0]
            poison()
            names = launches(lambda: outs.append(grouped(x[:, a:b], past_key_values=cg, use_cache=True)[0]))
            same_bits(f"tokens {a}:{b}", outs[0], op)
            if a == 0:
                assert names.get("k_csf_out4<norm,gqa>") == 1 and "k_csf_out4<norm>" not in names, names
    assert cg[0]["recurrent_state"].S.shape[1] == 2 and cp[0]["recurrent_state"].S.shape[1] == 4


def test_fla_layer_plain_forward():
    """A forward without a cache: under torch.no_grad() k and v stay on the k/v heads (grouped output kernel), with grad enabled the
    layer repeats them; the same bits."""
    plain, grouped = _layers(torch.bfloat16)
    x = torch.randn(2, 130, 512, generator=torch.Generator().manual_seed(29)).to(DEV).to(torch.bfloat16)
    for layer in (plain, grouped):
        outs = []
        poison()
        with_grad = layer(x)[0]
        assert with_grad.requires_grad
        with torch.no_grad():
            poison()
            names = launches(lambda: outs.append(layer(x)[0]))
        same_bits("no_grad forward", outs[0], with_grad.detach())
        assert names.get("k_csf_out4<norm,gqa>") == 1 and "k_csf_out4<norm>" not in names, names
        # up to 64 tokens: the reference's token-recurrent branch (naive_recurrent_mhla), norm and gate as kernels of their own
        short = []
        poison()
        want = layer(x[:, :40])[0].detach()
        with torch.no_grad():
            poison()
            names = launches(lambda: short.append(layer(x[:, :40])[0]))
        same_bits("no_grad forward, 40 tokens", short[0], want)
        assert names.get("k_csf_out4<gqa>") == 1 and "k_csf_out4" not in names, names
