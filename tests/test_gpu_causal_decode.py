"""GPU parity: decoding with the causal operator -- prefill state + single-token steps (mhla_causal_prefill / mhla_causal_step),
the fla layer's `exact_decoding` and the GPT host's cache / generate.  The reference is the chunk operator itself: it is causal,
so row t of `orc.causal_fwd` over the whole sequence is what step t must return."""
import pytest
import torch

from conftest import load_golden, rel_err, rms_ratio
from decode_util import check_state, decode_inputs, packed_views
from gpu_util import DEV, CAUSAL_CHUNK_TOL_H16, CAUSAL_TOL, TOL, check, check_chunks, poison, _fla_layer
from oracle import mhla_oracle as orc

pytestmark = pytest.mark.gpu


def _check_rows(name, o0, o1, want):
    """Prefill and step rows together, from token 0 so that the 64-token chunks of the per-chunk check are the operator's: each
    chunk of rows (a partly decoded one included) within the bound of its own maximum.  A chunk may hold rows of both kinds, so
    it gets the wider of the two per-chunk bounds: prefill rows come from the operator's default arithmetic (11-bit stored
    summaries for 16-bit tensors: CAUSAL_CHUNK_TOL_H16), step rows from the fp32 state (CAUSAL_TOL)."""
    got = o1 if o0 is None or o0.shape[1] == 0 else torch.cat([o0, o1], dim=1)
    assert got.shape[1] == want.shape[1]
    check_chunks(name, got, want, max(CAUSAL_CHUNK_TOL_H16[got.dtype], CAUSAL_TOL[got.dtype]))


def _decode(q, k, v, mix, T0, n, state=None, views=None, scale=None, **kw):
    """Prefill the first T0 tokens (unless a state is given), then n steps; returns (prefill output, stacked step outputs, state)."""
    import mhla_amd
    o0 = None
    if scale is not None:
        kw["scale"] = scale
    if state is None:
        o0, state = mhla_amd.mhla_causal_prefill(q[:, :T0], k[:, :T0], v[:, :T0], mix, scale=scale)
        assert state.seen == T0
    outs = []
    for t in range(state.seen, state.seen + n):
        qt, kt, vt = (views or (lambda *a: a))(q[:, t:t + 1], k[:, t:t + 1], v[:, t:t + 1])
        outs.append(mhla_amd.mhla_causal_step(qt, kt, vt, mix, state, **{a: (b[:, t:t + 1] if a == "gate" else b) for a, b in kw.items()}))
    return o0, (torch.cat(outs, dim=1) if outs else None), state


CASES = [  # dtype, B, H, K, V, T0, n, packed
    (torch.float32, 2, 2, 16, 24, 0, 70, False),       # empty state, first roll
    (torch.float32, 1, 2, 32, 16, 60, 10, False),      # partial tail then roll
    (torch.bfloat16, 1, 2, 64, 128, 64, 65, False),    # prefill ending on a boundary (Cur = 0), roll at 128
    (torch.bfloat16, 1, 4, 128, 256, 120, 80, False),  # C5 head, two rolls (128, 192)
    (torch.bfloat16, 1, 2, 256, 512, 63, 3, False),    # 1.3B-like head, roll on the first step
    (torch.float16, 2, 1, 64, 64, 100, 30, False),     # fp16
    (torch.bfloat16, 1, 2, 64, 64, 70, 5, True),       # strided slices of one packed projection
]
C5 = CASES[3]


def _case(case):
    dtype, B, H, K, V, T0, n, packed = case
    L = (T0 + n + 63) // 64 + 1
    q, k, v, mix, want = decode_inputs(B, T0 + n, H, K, V, L, dtype)
    return [t.to(DEV) for t in (q, k, v, mix)], want


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{str(c[0]).split('.')[-1]}-B{c[1]}H{c[2]}K{c[3]}V{c[4]}-{c[5]}+{c[6]}" + ("-packed" if c[7] else ""))
def test_steps_are_rows_of_the_full_operator(case):
    dtype, B, H, K, V, T0, n, packed = case
    (q, k, v, mix), want = _case(case)
    poison()
    o0, o1, state = _decode(q, k, v, mix, T0, n, views=packed_views if packed else None)
    assert state.seen == T0 + n and o1.dtype == dtype and o1.shape == (B, n, H, V)
    if T0:
        check("prefill rows", o0, want[:, :T0], CAUSAL_TOL[dtype])
    else:
        assert o0.shape == (B, 0, H, V)
    check("step rows", o1, want[:, T0:], CAUSAL_TOL[dtype])
    _check_rows("rows", o0, o1, want)


@pytest.mark.parametrize("tag,T0,T1", [("b", 190, 200), ("a", 64, 256), ("d", 130, 320)])
def test_steps_match_reference_fixtures(tag, T0, T1):
    g = load_golden("causal_" + tag)
    bf16 = tag == "d"
    q, k, v = ((g[n].bfloat16() if bf16 else g[n]).to(DEV) for n in ("q", "k", "v"))
    assert q.shape[1] >= T1
    mix = g["mix"].to(DEV)
    o0, o1, _ = _decode(q, k, v, mix, T0, T1 - T0)
    got = torch.cat([o0, o1], dim=1)
    want = g["out"][:, :T1]
    tol = 2 * 2.0 ** -8 + 1e-3 if bf16 else 1e-4    # the bounds test_golden_causal holds the operator to on these fixtures
    check("out rows", got, want, tol)
    check_chunks("out rows", got, want, tol if bf16 else CAUSAL_TOL[torch.float32])
    if bf16:
        r = rms_ratio(got.float().cpu(), want.float())
        assert r < 1e-3, f"rms-relative error {r:.2e} vs the reference's own bf16 result"


def test_steps_match_the_reference_recurrent_form_on_the_first_chunk():
    """Fixture c (T <= 64): the one place where the reference's own token-recurrent form is right."""
    g = load_golden("causal_c")
    q, k, v, mix = (g[n].to(DEV) for n in ("q", "k", "v", "mix"))
    T = q.shape[1]
    assert T >= 50 and "out_recurrent" in g
    o0, o1, state = _decode(q, k, v, mix, 0, 50)
    assert o0.shape[1] == 0 and state.seen == 50
    check("vs out", o1, g["out"][:, :50], 1e-4)
    check("vs out_recurrent", o1, g["out_recurrent"][:, :50], 1e-4)
    check_chunks("vs out", o1, g["out"][:, :50], 1e-4)


def test_state_contents():
    import mhla_amd
    dtype, B, H, K, V, T0, n, _ = C5
    (q, k, v, mix), _ = _case(C5)
    _, _, state = _decode(q, k, v, mix, T0, 0)
    check_state(state, q, k, v, mix, "after prefill(120)")
    _decode(q, k, v, mix, T0, 8, state=state)
    check_state(state, q, k, v, mix, "on the boundary 128")
    _decode(q, k, v, mix, T0, n - 8, state=state)
    check_state(state, q, k, v, mix, "after 80 steps")
    # prefill(T0) + n steps == prefill(T0 + n)
    _, ref = mhla_amd.mhla_causal_prefill(q, k, v, mix)
    assert ref.seen == state.seen == T0 + n
    nfull = (T0 + n) // 64
    tol = TOL[torch.float32]
    check("S: steps vs prefill", state.S[:, :, :nfull], ref.S[:, :, :nfull].cpu(), tol)
    check("P: steps vs prefill", state.P, ref.P.cpu(), tol)
    check("Cur: steps vs prefill", state.Cur, ref.Cur.cpu(), tol)
    # a prefill that ends on a boundary
    _, _, sb = _decode(q, k, v, mix, 128, 0)
    check_state(sb, q, k, v, mix, "after prefill(128)")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("gate,affine", [(True, True), (True, False), (False, True)])
def test_step_fused_norm_gate_epilogue(dtype, gate, affine):
    B, H, K, V, T0, n = 1, 2, 64, 128, 60, 6
    q, k, v, mix, want = decode_inputs(B, T0 + n, H, K, V, 3, dtype)
    gen = torch.Generator().manual_seed(7)
    g = torch.randn(B, T0 + n, H, V, generator=gen).to(dtype)
    w = torch.rand(V, generator=gen) + 0.5
    eps = 1e-5
    o_ref = orc.causal_fwd(q.float(), k.float(), v.float(), mix)[:, T0:]
    if gate:
        y_ref = orc.rms_norm_swish_gate(o_ref, g[:, T0:].float(), w if affine else None, eps)
    else:
        y_ref = o_ref * torch.rsqrt(o_ref.pow(2).mean(-1, keepdim=True) + eps) * w
    qd, kd, vd, md = (t.to(DEV) for t in (q, k, v, mix))
    kw = {}
    if gate:
        kw["gate"] = g.to(DEV)
    if affine:
        kw["norm_weight"] = w.to(DEV)
    poison()
    _, y, state = _decode(qd, kd, vd, md, T0, n, norm_eps=eps, **kw)
    assert y.dtype == dtype and state.seen == T0 + n
    check("y", y, y_ref, CAUSAL_TOL[dtype])


@pytest.mark.parametrize("scale", [1.0, 0.37])
@pytest.mark.parametrize("epilogue", [False, True], ids=["o", "fused-norm-gate"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_scale_argument_across_a_chunk_boundary(dtype, epilogue, scale):
    """`scale` other than the default K ** -0.5 = 0.125 through mhla_causal_prefill (60 tokens) and ten mhla_causal_step calls, the
    fourth of which closes the chunk: rows of the oracle at the same scale, with and without the step's fused norm x gate
    epilogue.  Behind a norm with eps << mean(o^2) y does not depend on the scale of o (2e-6 here), so the epilogue cases take
    a norm_eps of the size of mean(o^2) at the tested scale (72 / 529): the oracle's y at the default scale is then 0.5 .. 0.8 of
    the maximum away, asserted below.  mhla_causal_state takes no `scale` (the state S = k^T v does not contain it): a state
    built by it alone continues, under the same `scale`, to the same bits."""
    import mhla_amd
    B, H, K, V, T0, n = 1, 2, 64, 128, 60, 10
    assert abs(scale - K ** -0.5) > 0.1
    q, k, v, mix, want = decode_inputs(B, T0 + n, H, K, V, 3, dtype, 1234, scale)
    qd, kd, vd, md = (t.to(DEV) for t in (q, k, v, mix))
    kw = {}
    if epilogue:
        gen = torch.Generator().manual_seed(7)
        g = torch.randn(B, T0 + n, H, V, generator=gen).to(dtype)
        w = torch.rand(V, generator=gen) + 0.5
        eps = {0.37: 72.0, 1.0: 530.0}[scale]
        kw = dict(gate=g.to(DEV), norm_weight=w.to(DEV), norm_eps=eps)
        y_ref = orc.rms_norm_swish_gate(want[:, T0:], g[:, T0:].float(), w, eps)
        y_default = orc.rms_norm_swish_gate(decode_inputs(B, T0 + n, H, K, V, 3, dtype)[4][:, T0:], g[:, T0:].float(), w, eps)
        assert rel_err(y_default, y_ref) > 0.25   # the comparison can see the argument: 50 times the widest bound below
    poison()
    o0, o1, state = _decode(qd, kd, vd, md, T0, n, scale=scale, **kw)
    assert state.seen == T0 + n and o1.dtype == dtype
    check("prefill rows", o0, want[:, :T0], CAUSAL_TOL[dtype])
    check_chunks("prefill rows", o0, want[:, :T0], CAUSAL_CHUNK_TOL_H16[dtype])
    if epilogue:
        check("y", o1, y_ref, CAUSAL_TOL[dtype])
    else:
        check("step rows", o1, want[:, T0:], CAUSAL_TOL[dtype])
        _check_rows("rows", o0, o1, want)
    s2 = mhla_amd.mhla_causal_state(kd[:, :T0], vd[:, :T0], md)
    assert s2.seen == T0
    _, o2, s2 = _decode(qd, kd, vd, md, T0, n, state=s2, scale=scale, **kw)
    assert torch.equal(o2, o1) and torch.equal(s2.P, state.P) and torch.equal(s2.Cur, state.Cur) and torch.equal(s2.S[:, :, :1], state.S[:, :, :1])


def test_steps_are_deterministic():
    dtype, B, H, K, V, T0, n, _ = C5
    (q, k, v, mix), _ = _case(C5)
    _, _, s0 = _decode(q, k, v, mix, T0, 0)
    runs = []
    for _ in range(2):
        st = s0.clone()
        assert st.S.data_ptr() != s0.S.data_ptr() and st.seen == s0.seen
        _, o, st = _decode(q, k, v, mix, T0, n, state=st)
        runs.append((o, st))
    (oa, sa), (ob, sb) = runs
    assert torch.equal(oa, ob)
    nfull = sa.seen // 64
    assert torch.equal(sa.S[:, :, :nfull], sb.S[:, :, :nfull]) and torch.equal(sa.P, sb.P) and torch.equal(sa.Cur, sb.Cur)


def test_uninitialised_memory_is_never_read():
    dtype, B, H, K, V, T0, n, _ = C5
    (q, k, v, mix), _ = _case(C5)
    poison()
    o0, o1, state = _decode(q, k, v, mix, T0, n)
    nfull = state.seen // 64
    for name, t in (("prefill out", o0), ("step out", o1), ("S", state.S[:, :, :nfull]), ("P", state.P), ("Cur", state.Cur)):
        assert bool(torch.isfinite(t).all()), f"{name} holds non-finite values"
    # rows of S beyond the finished chunks are never read: NaN there changes nothing
    _, _, s2 = _decode(q, k, v, mix, T0, 0)
    s2.S[:, :, T0 // 64:] = float("nan")
    _, o2, s2 = _decode(q, k, v, mix, T0, n, state=s2)
    assert torch.equal(o2, o1)
    assert torch.equal(s2.S[:, :, :nfull], state.S[:, :, :nfull]) and torch.equal(s2.P, state.P) and torch.equal(s2.Cur, state.Cur)
    assert bool(torch.isnan(s2.S[:, :, nfull:]).all())


def test_full_state_and_errors():
    import mhla_amd
    from mhla_amd import _lib, ops
    B, H, K, V = 1, 2, 16, 24
    q, k, v, mix3, want = decode_inputs(B, 130, H, K, V, 3, torch.float32, seed=5)
    q, k, v, mix = (t.to(DEV) for t in (q, k, v, mix3[:2, :2].contiguous()))   # (rows 0, 1 of the operator read mix[:2, :2] only)
    # an [L, L] = [2, 2] matrix serves 128 tokens: the last step closes chunk 1 without a next row of mix
    o0, o1, state = _decode(q, k, v, mix, 120, 8)
    check("rows up to the capacity", torch.cat([o0, o1], 1), want[:, :128], CAUSAL_TOL[torch.float32])
    _check_rows("rows up to the capacity", o0, o1, want[:, :128])
    assert state.seen == 128 and state.capacity_chunks == 2 and state.nbytes == 4 * B * H * K * V * 4
    keep = state.clone()
    with pytest.raises(IndexError, match="needs 3 chunks but mixing_matrix has only 2 rows"):
        mhla_amd.mhla_causal_step(q[:, 128:129], k[:, 128:129], v[:, 128:129], mix, state)
    assert state.seen == 128 and all(torch.equal(a, b) for a, b in ((state.S, keep.S), (state.P, keep.P), (state.Cur, keep.Cur)))
    with pytest.raises(IndexError):
        mhla_amd.mhla_causal_prefill(q, k, v, mix)   # 130 tokens: 3 chunks

    _, _, st = _decode(q, k, v, mix, 10, 0)
    one = lambda t, i=10: t[:, i:i + 1]
    step = lambda qq, kk, vv, s=None, **kw: mhla_amd.mhla_causal_step(qq, kk, vv, mix, st if s is None else s, **kw)
    before = st.clone()
    with pytest.raises(ValueError):
        step(q[:, 10:12], k[:, 10:12], v[:, 10:12])                               # T != 1
    with pytest.raises(ValueError):
        step(one(q), one(k)[..., :8], one(v))                                     # shape
    with pytest.raises(ValueError):
        step(one(q), one(k).bfloat16(), one(v))                                   # dtype
    with pytest.raises(ValueError):
        step(one(q), one(k).cpu(), one(v))                                        # device
    with pytest.raises(ValueError):
        step(one(q), one(k), one(v), gate=one(v)[..., :8])                        # gate shape
    with pytest.raises(ValueError):
        step(one(q), one(k), one(v), s=mhla_amd.CausalState.empty(B, H, K, V + 4, 2, DEV))   # state of another V
    with pytest.raises(ValueError):
        step(one(q), one(k), one(v), s=mhla_amd.CausalState.empty(B, H, K + 4, V, 2, DEV))   # state of another K
    with pytest.raises(RuntimeError, match="inference only"):
        step(one(q).clone().requires_grad_(True), one(k), one(v))
    assert st.seen == 10 and torch.equal(st.Cur, before.Cur) and torch.equal(st.P, before.P)
    with torch.no_grad():   # the same input under no_grad is fine
        o = step(one(q).clone().requires_grad_(True), one(k), one(v))
    assert not o.requires_grad and st.seen == 11
    check("row 10", o, want[:, 10:11], CAUSAL_TOL[torch.float32])

    # the raw entry point: short workspace, position beyond the state's capacity
    lib = _lib.load()
    need = lib.mhla_causal_step_ws_bytes(B, H, K, V, _lib.F32)
    ws = torch.empty(need // 4 + 4, dtype=torch.float32, device=DEV)
    out = torch.empty(B, 1, H, V, device=DEV)
    mixf = mix.contiguous()

    def raw(pos, ws_bytes):
        return lib.mhla_causal_step(ops._view(one(q)), ops._view(one(k)), ops._view(one(v)), mixf.data_ptr(), 2, st.S.data_ptr(), 2,
                                    st.P.data_ptr(), st.Cur.data_ptr(), pos, ops._view(out), _lib.NULL_VIEW, None, 1e-5, _lib.NULL_VIEW,
                                    ws.data_ptr(), ws_bytes, B, H, K, V, 64, K ** -0.5, _lib.F32, ops._stream())
    EINVAL = -22
    snap = st.clone()
    assert raw(11, need - 4) == EINVAL and b"workspace too small" in lib.mhla_last_error()
    assert raw(128, need) == EINVAL and b"the state holds 2" in lib.mhla_last_error()
    torch.cuda.synchronize()
    assert torch.equal(st.Cur, snap.Cur) and torch.equal(st.P, snap.P)


@pytest.mark.parametrize("opts", [{}, {"num_kv_heads": 1}, {"use_output_gate": False}], ids=["default", "gqa", "no-output-gate"])
@pytest.mark.parametrize("T0,n", [(100, 40), (0, 70)], ids=["prefill100+40", "70-from-empty"])
def test_fla_layer_exact_decoding(opts, T0, n):
    import mhla_amd
    from mhla_amd import modules
    m = _fla_layer(**opts)
    x = torch.randn(2, T0 + n, 256, generator=torch.Generator().manual_seed(11))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    want = orc.fla_layer_forward(sd, x, 2, 64, 128, norm_eps=1e-6, **opts)
    m = m.to(DEV).eval()
    xd = x.to(DEV)
    cache = modules.DecodeCache()
    outs = []
    with torch.no_grad():
        if T0:
            o, attn, c = m(xd[:, :T0], past_key_values=cache, use_cache=True)
            assert attn is None and c is cache and cache.get_seq_length(0) == T0
            outs.append(o)
        for t in range(T0, T0 + n):
            outs.append(m(xd[:, t:t + 1], past_key_values=cache, use_cache=True)[0])
    got = torch.cat(outs, dim=1)
    check("o (prefill + steps)", got, want, 1e-4)
    assert cache.get_seq_length() == T0 + n and len(cache) == 1
    st = cache[0]["recurrent_state"]
    assert isinstance(st, mhla_amd.CausalState) and st.seen == T0 + n and st.S.shape == (2, 2, 32, 64, 128)


def test_fla_layer_exact_decoding_multi_token_call_and_padding():
    from mhla_amd import modules
    m = _fla_layer()
    x = torch.randn(2, 80, 256, generator=torch.Generator().manual_seed(12))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    want = orc.fla_layer_forward(sd, x, 2, 64, 128, norm_eps=1e-6)
    m = m.to(DEV).eval()
    xd = x.to(DEV)
    cache = modules.DecodeCache()
    with torch.no_grad():
        a = m(xd[:, :60], past_key_values=cache, use_cache=True, attention_mask=torch.ones(2, 60, dtype=torch.long, device=DEV))[0]
        b = m(xd[:, 60:80], past_key_values=cache, use_cache=True)[0]      # several tokens on a state: one step each
        check("o", torch.cat([a, b], dim=1), want, 1e-4)
        mask = torch.ones(2, 81, dtype=torch.long, device=DEV)
        mask[1, :3] = 0
        with pytest.raises(NotImplementedError):
            m(xd[:, :1], past_key_values=cache, use_cache=True, attention_mask=mask)
    assert cache.get_seq_length() == 80


def test_gpt_host_cached_logits_and_generate():
    from mhla_amd.hosts.gpt import GPT_MHLA
    from mhla_amd.modules import DecodeCache
    torch.manual_seed(5)
    model = GPT_MHLA(vocab_size=512, hidden_size=128, num_layers=2, num_heads=4, max_seq_len=2048, exact_decoding=True).to(DEV).eval()
    prompt = torch.randint(0, 512, (2, 20), generator=torch.Generator().manual_seed(6)).to(DEV)
    new = model.generate(prompt, 50)
    assert new.shape == (2, 50) and new.dtype == torch.long
    ids = torch.cat([prompt, new], dim=1)[:, :70]
    with torch.no_grad():
        full = model(ids)
        cache = DecodeCache()
        steps = [model(ids[:, :20], cache=cache)] + [model(ids[:, t:t + 1], cache=cache) for t in range(20, 70)]
    cached = torch.cat(steps, dim=1)
    assert cache.get_seq_length(0) == cache.get_seq_length(1) == 70
    check("logits: prefill(20) + 50 cached steps vs one forward", cached, full.cpu(), 1e-4)
    assert torch.equal(new, cached[:, 19:69].argmax(-1))
    with pytest.raises(ValueError):
        GPT_MHLA(vocab_size=64, hidden_size=128, num_layers=1, num_heads=4).to(DEV)(prompt % 64, cache=DecodeCache())
