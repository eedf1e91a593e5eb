"""GPU parity: extending a decode state of the causal operator by several tokens in one call (mhla_causal_extend), through the
fla layer's `exact_decoding` and the GPT host's cache.  The reference is the chunk operator itself, as in
test_gpu_causal_decode.py: rows state.seen .. state.seen + T - 1 of `orc.causal_fwd` over the whole sequence; states are
compared with the oracle's summaries, with the fp64 restatement of the segment formula (decode_util.extend_ref) and with
the same state advanced by single steps."""
import pytest
import torch

from conftest import load_golden, rel_err, rms_ratio
from decode_util import check_state, cpu_state, decode_inputs, extend_ref, packed_views, same_state
from gpu_util import DEV, CAUSAL_CHUNK_TOL_H16, CAUSAL_TOL, TOL, check, check_chunks, launches, poison, _fla_layer
from oracle import mhla_oracle as orc

pytestmark = pytest.mark.gpu


def _start(q, k, v, mix, T0, scale=None, **kw):
    """(prefill rows or None, state) after T0 tokens: `mhla_causal_prefill`, or an empty state for T0 = 0."""
    import mhla_amd
    B, _, H, K = q.shape
    if T0 == 0:
        return None, mhla_amd.CausalState.empty(B, H, K, v.shape[-1], kw.get("capacity_chunks") or mix.shape[0], DEV)
    o0, state = mhla_amd.mhla_causal_prefill(q[:, :T0], k[:, :T0], v[:, :T0], mix, scale=scale, **kw)
    assert state.seen == T0
    return o0, state


def _extend(q, k, v, mix, state, n, views=None, **kw):
    import mhla_amd
    t = state.seen
    qt, kt, vt = (views or (lambda *a: a))(q[:, t:t + n], k[:, t:t + n], v[:, t:t + n])
    o = mhla_amd.mhla_causal_extend(qt, kt, vt, mix, state, **{a: (b[:, t:t + n] if a == "gate" else b) for a, b in kw.items()})
    assert state.seen == t + n and o.shape == (q.shape[0], n, q.shape[2], v.shape[-1]) and o.dtype == q.dtype
    return o


def _steps(q, k, v, mix, state, n, **kw):
    import mhla_amd
    outs = []
    for t in range(state.seen, state.seen + n):
        outs.append(mhla_amd.mhla_causal_step(q[:, t:t + 1], k[:, t:t + 1], v[:, t:t + 1], mix, state, **kw))
    return torch.cat(outs, dim=1)


def _check_rows(name, o0, ext, want):
    """All rows from token 0, so that the 64-token chunks of the per-chunk check are the operator's.  Chunks that hold prefill rows
    of the default operator (11-bit stored summaries for 16-bit tensors) get the wider of the two per-chunk bounds; every chunk
    whose rows all came from a state is held to CAUSAL_TOL."""
    T0 = 0 if o0 is None else o0.shape[1]
    got = ext if T0 == 0 else torch.cat([o0, ext], dim=1)
    assert got.shape[1] == want.shape[1]
    dt = got.dtype
    check(f"{name}: extension rows", ext, want[:, T0:], CAUSAL_TOL[dt])
    n0 = (T0 + 63) // 64 * 64
    if T0:
        check_chunks(f"{name}: chunks with prefill rows", got[:, :n0], want[:, :n0], max(CAUSAL_CHUNK_TOL_H16[dt], CAUSAL_TOL[dt]))
    if got.shape[1] > n0:
        check_chunks(f"{name}: chunks from the state alone", got[:, n0:], want[:, n0:], CAUSAL_TOL[dt])


CASES = [  # dtype, B, H, K, V, T0 (prefill), extensions, packed, state checks
    (torch.float32, 2, 2, 16, 24, 0, (70,), False, False),             # extension as prefill; K, V below one tile; first roll
    (torch.float32, 1, 2, 32, 16, 60, (10, 1, 57, 64, 3), False, True),   # partial fill across a boundary; T = 1; landing on a boundary; a whole chunk; a tail
    (torch.float32, 1, 2, 80, 72, 37, (27, 200), False, False),        # K, V not multiples of 64; three new chunks in one call
    (torch.bfloat16, 1, 2, 64, 128, 64, (65, 130), False, False),      # start on a boundary (Cur = 0)
    (torch.bfloat16, 1, 4, 128, 256, 120, (200,), False, True),        # C5 head, four boundaries, ends on one (320)
    (torch.bfloat16, 1, 4, 128, 256, 120, (80,), False, True),         # ... and 80 from a fresh prefill
    (torch.bfloat16, 1, 2, 256, 512, 63, (66,), False, False),         # 1.3B-like head; the chunk closes on the first row; one whole chunk + one row
    (torch.float16, 2, 1, 64, 64, 100, (30,), False, False),           # fp16
    (torch.bfloat16, 1, 2, 64, 64, 70, (40,), True, False),            # strided slices of one packed projection
    (torch.bfloat16, 1, 2, 64, 64, 0, (200,), False, False),           # every chunk from the state alone: CAUSAL_TOL per chunk
    (torch.float32, 1, 2, 64, 64, 0, (200,), False, False),
]
C5 = CASES[4]


def _case(case):
    dtype, B, H, K, V, T0, exts = case[:7]
    T = T0 + sum(exts)
    q, k, v, mix, want = decode_inputs(B, T, H, K, V, (T + 63) // 64 + 1, dtype)
    return [t.to(DEV) for t in (q, k, v, mix)], want


def _id(c):
    return f"{str(c[0]).split('.')[-1]}-B{c[1]}H{c[2]}K{c[3]}V{c[4]}-{c[5]}+" + "+".join(map(str, c[6])) + ("-packed" if c[7] else "")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_extensions_are_rows_of_the_full_operator(case):
    dtype, B, H, K, V, T0, exts, packed, states = case
    (q, k, v, mix), want = _case(case)
    poison()
    o0, state = _start(q, k, v, mix, T0)
    outs = []
    for n in exts:
        before = state.clone()
        outs.append(_extend(q, k, v, mix, state, n, views=packed_views if packed else None))
        if states:
            name = f"after {state.seen} tokens"
            check_state(state, q, k, v, mix, name)
            sl = slice(before.seen, state.seen)
            o_ref, ref = extend_ref(cpu_state(before), q[:, sl].cpu(), k[:, sl].cpu(), v[:, sl].cpu(), mix.cpu())
            check(f"{name}: rows vs extend_ref", outs[-1], o_ref.float(), CAUSAL_TOL[dtype])
            same_state(f"{name}: vs extend_ref", cpu_state(state), ref, TOL[torch.float32])
            _steps(q, k, v, mix, before, n)
            same_state(f"{name}: vs single steps", cpu_state(state), cpu_state(before), TOL[torch.float32])
    assert state.seen == T0 + sum(exts)
    _check_rows("rows", o0, torch.cat(outs, dim=1), want)


def test_interleaved_extensions_and_steps():
    import mhla_amd
    dtype, B, H, K, V = torch.bfloat16, 1, 2, 64, 64
    q, k, v, mix, want = decode_inputs(B, 205, H, K, V, 5, dtype)
    q, k, v, mix = (t.to(DEV) for t in (q, k, v, mix))
    poison()
    o0, state = _start(q, k, v, mix, 50)
    outs = [_extend(q, k, v, mix, state, 30), _steps(q, k, v, mix, state, 20), _extend(q, k, v, mix, state, 100),
            _steps(q, k, v, mix, state, 5)]
    assert state.seen == 205
    _check_rows("rows", o0, torch.cat(outs, dim=1), want)
    ref = mhla_amd.mhla_causal_state(k, v, mix)
    same_state("vs one prefill of the whole sequence", cpu_state(state), cpu_state(ref), TOL[torch.float32])
    check_state(state, q, k, v, mix, "after 205 tokens")


@pytest.mark.parametrize("T0", [10, 63, 64], ids=["inside", "closes-the-chunk", "on-a-boundary"])
def test_one_token_is_the_step(T0):
    import mhla_amd
    dtype, B, H, K, V = torch.bfloat16, 1, 2, 64, 128
    q, k, v, mix, _ = decode_inputs(B, 70, H, K, V, 3, dtype)
    q, k, v, mix = (t.to(DEV) for t in (q, k, v, mix))
    _, sa = _start(q, k, v, mix, T0)
    sb = sa.clone()
    one = lambda t: t[:, T0:T0 + 1]
    oa = mhla_amd.mhla_causal_extend(one(q), one(k), one(v), mix, sa)
    ob = mhla_amd.mhla_causal_step(one(q), one(k), one(v), mix, sb)
    assert sa.seen == sb.seen == T0 + 1 and torch.equal(oa, ob)
    assert torch.equal(sa.P, sb.P) and torch.equal(sa.Cur, sb.Cur) and torch.equal(sa.S[:, :, :sa.seen // 64], sb.S[:, :, :sb.seen // 64])


@pytest.mark.parametrize("tag,T0,T1", [("a", 64, 256), ("b", 190, 200), ("d", 130, 320)])
def test_extension_matches_reference_fixtures(tag, T0, T1):
    g = load_golden("causal_" + tag)
    bf16 = tag == "d"
    q, k, v = ((g[n].bfloat16() if bf16 else g[n]).to(DEV) for n in ("q", "k", "v"))
    assert q.shape[1] >= T1
    mix = g["mix"].to(DEV)
    o0, state = _start(q, k, v, mix, T0)
    o1 = _extend(q, k, v, mix, state, T1 - T0)
    got = torch.cat([o0, o1], dim=1)
    want = g["out"][:, :T1]
    tol = 2 * 2.0 ** -8 + 1e-3 if bf16 else 1e-4    # the bounds test_steps_match_reference_fixtures holds the steps to
    check("out rows", got, want, tol)
    check_chunks("out rows", got, want, tol if bf16 else CAUSAL_TOL[torch.float32])
    if bf16:
        r = rms_ratio(got.float().cpu(), want.float())
        assert r < 1e-3, f"rms-relative error {r:.2e} vs the reference's own bf16 result"


@pytest.mark.parametrize("scale", [1.0, 0.37])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("gate,affine", [(True, True), (True, False), (False, True)], ids=["gate+weight", "gate", "weight"])
def test_extend_fused_norm_gate_epilogue(dtype, gate, affine, scale):
    """Prefill 20, one extension of 50 tokens across the boundary at 64 (44 rows of the open chunk, 6 of the next).  Behind a norm
    with eps << mean(o^2) y does not depend on the scale of o, so norm_eps is of the size of mean(o^2) at the tested scale (the
    values test_scale_argument_across_a_chunk_boundary derives for these inputs): the oracle's y at the default scale is then far
    outside the bound, asserted below."""
    B, H, K, V, T0, n = 1, 2, 64, 128, 20, 50
    q, k, v, mix, want = decode_inputs(B, T0 + n, H, K, V, 3, dtype, 1234, scale)
    gen = torch.Generator().manual_seed(7)
    g = torch.randn(B, T0 + n, H, V, generator=gen).to(dtype)
    w = torch.rand(V, generator=gen) + 0.5
    eps = {0.37: 72.0, 1.0: 530.0}[scale]

    def y_of(o):
        if gate:
            return orc.rms_norm_swish_gate(o, g[:, T0:].float(), w if affine else None, eps)
        return o * torch.rsqrt(o.pow(2).mean(-1, keepdim=True) + eps) * w
    y_ref = y_of(want[:, T0:])
    assert rel_err(y_of(decode_inputs(B, T0 + n, H, K, V, 3, dtype)[4][:, T0:]), y_ref) > 0.25   # the comparison can see `scale`
    qd, kd, vd, md = (t.to(DEV) for t in (q, k, v, mix))
    kw = {"norm_eps": eps, "scale": scale}
    if gate:
        kw["gate"] = g.to(DEV)
    if affine:
        kw["norm_weight"] = w.to(DEV)
    poison()
    _, state = _start(qd, kd, vd, md, T0, scale=scale)
    y = _extend(qd, kd, vd, md, state, n, **kw)
    check("y", y, y_ref, CAUSAL_TOL[dtype])
    # the plain rows at this scale from the same start: the state does not depend on the epilogue
    _, s2 = _start(qd, kd, vd, md, T0, scale=scale)
    o = _extend(qd, kd, vd, md, s2, n, scale=scale)
    check("o", o, want[:, T0:], CAUSAL_TOL[dtype])
    same_state("epilogue or not", state, s2)


def test_extensions_are_deterministic():
    (q, k, v, mix), _ = _case(C5)
    _, s0 = _start(q, k, v, mix, 120)
    runs = []
    for _ in range(2):
        st = s0.clone()
        assert st.S.data_ptr() != s0.S.data_ptr()
        runs.append((_extend(q, k, v, mix, st, 200), st))
    (oa, sa), (ob, sb) = runs
    assert torch.equal(oa, ob)
    same_state("two runs", sa, sb)


def test_long_extensions_and_large_batches_are_cut(monkeypatch):
    """A workspace cap of one token's worth cuts the extension into calls of at most 64 tokens at chunk boundaries, a (b, h) range
    of one batch entry slices the batch: the same segments through the same kernels, so the same bits as one call."""
    from mhla_amd import ops
    dtype, B, H, K, V, T0, n = torch.bfloat16, 2, 2, 64, 64, 40, 230
    q, k, v, mix, want = decode_inputs(B, T0 + n, H, K, V, 6, dtype)
    q, k, v, mix = (t.to(DEV) for t in (q, k, v, mix))
    o0, s0 = _start(q, k, v, mix, T0)
    whole = s0.clone()
    o_whole = _extend(q, k, v, mix, whole, n)
    monkeypatch.setattr(ops, "EXTEND_WS_CAP_BYTES", 1)
    monkeypatch.setattr(ops, "_MAX_GRID_BH", H)
    cut = s0.clone()
    ran = launches(lambda: _extend(q, k, v, mix, cut, n))
    assert ran["k_cx_xty_acc"] == 2 * 5, ran      # per batch entry: 24 tokens to the boundary, 64, 64, 64, 14
    _check_rows("rows", o0, o_whole, want)
    cut2 = s0.clone()
    o_cut = _extend(q, k, v, mix, cut2, n)
    assert torch.equal(o_cut, o_whole)
    same_state("cut vs one call", cut2, whole)
    same_state("cut, run twice", cut2, cut)


def test_uninitialised_memory_is_never_read():
    (q, k, v, mix), _ = _case(C5)
    poison()
    o0, state = _start(q, k, v, mix, 120)
    o1 = _extend(q, k, v, mix, state, 150)        # ends at 270: chunks 0 .. 3 finished, 14 rows in chunk 4
    nfull = state.seen // 64
    assert nfull == 4
    for name, t in (("prefill out", o0), ("extension out", o1), ("S", state.S[:, :, :nfull]), ("P", state.P), ("Cur", state.Cur)):
        assert bool(torch.isfinite(t).all()), f"{name} holds non-finite values"
    # rows of S beyond the finished chunks are never read, and those the extension does not finish are not written
    _, s2 = _start(q, k, v, mix, 120)
    s2.S[:, :, 1:] = float("nan")
    o2 = _extend(q, k, v, mix, s2, 150)
    assert torch.equal(o2, o1)
    same_state("NaN beyond the finished chunks", s2, state)
    assert bool(torch.isnan(s2.S[:, :, nfull:]).all())


def test_full_state_and_errors():
    import mhla_amd
    from mhla_amd import _lib, ops
    B, H, K, V = 1, 2, 16, 24
    q, k, v, mix3, want = decode_inputs(B, 130, H, K, V, 3, torch.float32, seed=5)
    q, k, v, mix = (t.to(DEV) for t in (q, k, v, mix3[:2, :2].contiguous()))   # (rows 0, 1 of the operator read mix[:2, :2] only)
    # an [L, L] = [2, 2] matrix serves 128 tokens: the extension closes chunk 1 without a next row of mix
    o0, state = _start(q, k, v, mix, 120)
    o1 = _extend(q, k, v, mix, state, 8)
    _check_rows("rows up to the capacity", o0, o1, want[:, :128])
    assert state.seen == 128 and state.capacity_chunks == 2
    assert float(state.P.abs().max()) == 0.0 and float(state.Cur.abs().max()) == 0.0     # the state is full
    check_state(state, q, k, v, mix, "full state")
    keep = state.clone()
    with pytest.raises(IndexError, match="needs 3 chunks but mixing_matrix has only 2 rows"):
        _extend(q, k, v, mix, state, 2)
    with pytest.raises(IndexError):
        _extend(q, k, v, mix, state, 1)
    assert state.seen == 128
    same_state("after the refused calls", state, keep)
    _, fresh = _start(q, k, v, mix, 120)
    keep = fresh.clone()
    with pytest.raises(IndexError, match="sequence of 129 tokens needs 3 chunks"):
        _extend(q, k, v, mix, fresh, 9)
    assert fresh.seen == 120 and torch.equal(fresh.S, keep.S) and torch.equal(fresh.P, keep.P) and torch.equal(fresh.Cur, keep.Cur)
    # a state with less capacity than the matrix has rows
    mix3d = mix3.to(DEV)
    _, small = _start(q, k, v, mix3d, 120, capacity_chunks=2)
    with pytest.raises(IndexError, match="but the state holds only 2"):
        _extend(q, k, v, mix3d, small, 9)
    assert small.seen == 120

    _, st = _start(q, k, v, mix, 10)
    some = lambda t, i=10, n=5: t[:, i:i + n]
    ext = lambda qq, kk, vv, s=None, **kw: mhla_amd.mhla_causal_extend(qq, kk, vv, mix, st if s is None else s, **kw)
    before = st.clone()
    with pytest.raises(ValueError):
        ext(some(q), some(k)[..., :8], some(v))                                   # shape
    with pytest.raises(ValueError):
        ext(some(q), some(k), some(v, n=4))                                       # T of q and v differ
    with pytest.raises(ValueError):
        ext(some(q), some(k).bfloat16(), some(v))                                 # dtype
    with pytest.raises(ValueError):
        ext(some(q), some(k).cpu(), some(v))                                      # device
    with pytest.raises(ValueError):
        ext(some(q), some(k), some(v), gate=some(v)[..., :8])                     # gate shape
    with pytest.raises(ValueError):
        ext(some(q), some(k), some(v), s=mhla_amd.CausalState.empty(B, H, K, V + 4, 2, DEV))   # state of another V
    with pytest.raises(TypeError):
        ext(some(q), some(k), some(v), s=(st.S, st.P, st.Cur))
    with pytest.raises(RuntimeError, match="inference only"):
        ext(some(q).clone().requires_grad_(True), some(k), some(v))
    assert st.seen == 10
    same_state("after the refused calls", st, before)
    with torch.no_grad():   # the same input under no_grad is fine
        o = ext(some(q).clone().requires_grad_(True), some(k), some(v))
    assert not o.requires_grad and st.seen == 15
    check("rows 10 .. 14", o, want[:, 10:15], CAUSAL_TOL[torch.float32])

    # the raw entry point: short workspace, pos + T beyond the state's capacity, a row of mix that ldmix does not cover
    lib = _lib.load()
    T = 60
    need = lib.mhla_causal_extend_ws_bytes(B, T, H, K, V, 15, _lib.F32)
    ws = torch.empty(need // 4 + 4, dtype=torch.float32, device=DEV)
    out = torch.empty(B, T, H, V, device=DEV)
    mixf = mix.contiguous()

    def raw(pos, n, ws_bytes, ldmix=2):
        return lib.mhla_causal_extend(ops._view(q[:, :n]), ops._view(k[:, :n]), ops._view(v[:, :n]), mixf.data_ptr(), ldmix, st.S.data_ptr(), 2,
                                      st.P.data_ptr(), st.Cur.data_ptr(), pos, n, ops._view(out[:, :n]), _lib.NULL_VIEW, None, 1e-5,
                                      _lib.NULL_VIEW, ws.data_ptr(), ws_bytes, B, H, K, V, 64, K ** -0.5, _lib.F32, ops._stream())
    EINVAL = -22
    snap = st.clone()
    assert raw(15, T, need - 4) == EINVAL and b"workspace too small" in lib.mhla_last_error()
    assert raw(100, 29, need) == EINVAL and b"need 3 chunks, the state holds 2" in lib.mhla_last_error()
    assert raw(15, T, need, ldmix=1) == EINVAL and b"ldmix=1 < 2" in lib.mhla_last_error()
    assert raw(15, 0, need) == EINVAL and b"T=0" in lib.mhla_last_error()
    torch.cuda.synchronize()
    assert torch.equal(st.S, snap.S) and torch.equal(st.Cur, snap.Cur) and torch.equal(st.P, snap.P)


@pytest.mark.parametrize("name,T", [("mhla_causal_step", 1), ("mhla_causal_extend", 5)])
def test_checks_behind_the_device_check_refuse_before_launch(name, T):
    """The argument checks of step and extend that only GPU tensors reach (tests/test_decode_validation_cpu.py holds the others):
    epilogue arguments with epilogue=False, a state that is not contiguous, a state of another chunk size.  Each is a ValueError
    naming the function called -- for the chunk size too, which the step used to leave to the library (RuntimeError) -- and
    leaves the state as it was; nothing is launched."""
    import mhla_amd
    fn = getattr(mhla_amd, name)
    B, H, K, V, cap = 1, 2, 16, 24, 3
    q, k, v = torch.zeros(B, T, H, K, device=DEV), torch.zeros(B, T, H, K, device=DEV), torch.ones(B, T, H, V, device=DEV)
    mix = torch.ones(cap, cap, device=DEV)

    def refused(state, match, **kw):
        before = [t.clone() for t in (state.S, state.P, state.Cur)]
        with pytest.raises(ValueError, match=match):
            fn(q, k, v, mix, state, **kw)
        assert state.seen == 7 and all(torch.equal(a, b) for a, b in zip(before, (state.S, state.P, state.Cur)))

    def fresh(chunk_size=64):
        s = mhla_amd.CausalState.empty(B, H, K, V, cap, DEV, chunk_size=chunk_size)
        s.seen = 7
        s.Cur.fill_(0.5)
        return s

    refused(fresh(), f"{name}: gate / norm_weight given with epilogue=False", gate=torch.ones_like(v), epilogue=False)
    strided = fresh()
    strided.S = torch.full((B, H, cap, K, 2 * V), 0.25, device=DEV)[..., ::2]
    assert strided.S.shape == (B, H, cap, K, V) and not strided.S.is_contiguous()
    refused(strided, f"{name}: state tensors must be contiguous")
    refused(fresh(chunk_size=32), f"{name}: chunk_size=32, the decode state supports 64 only")


def test_launch_count_does_not_depend_on_the_tokens():
    (q, k, v, mix), want = _case(C5)
    _, state = _start(q, k, v, mix, 100)
    ran = launches(lambda: _extend(q, k, v, mix, state, 200))
    assert ran and "k_cs_step" not in ran and "k_cx_out" in ran, ran
    assert sum(ran.values()) <= 8 < 200, ran
    _, s2 = _start(q, k, v, mix, 100)
    stepped = launches(lambda: _steps(q, k, v, mix, s2, 3))
    assert stepped.get("k_cs_step") == 3 and sum(stepped.values()) >= 6, stepped   # at least two per token


def test_fla_layer_launch_count():
    from mhla_amd import modules
    m = _fla_layer().to(DEV).eval()
    x = torch.randn(2, 300, 256, generator=torch.Generator().manual_seed(13)).to(DEV)
    cache = modules.DecodeCache()
    with torch.no_grad():
        m(x[:, :100], past_key_values=cache, use_cache=True)
        ran = launches(lambda: m(x[:, 100:300], past_key_values=cache, use_cache=True))
    assert ran and "k_cs_step" not in ran and "k_cx_out" in ran, ran
    assert sum(ran.values()) < 200, ran
    assert cache.get_seq_length() == 300 and cache[0]["recurrent_state"].seen == 300


@pytest.mark.parametrize("opts", [{}, {"num_kv_heads": 1}, {"use_output_gate": False}], ids=["default", "gqa", "no-output-gate"])
def test_fla_layer_multi_token_calls(opts):
    import mhla_amd
    from mhla_amd import modules
    m = _fla_layer(**opts)
    x = torch.randn(2, 200, 256, generator=torch.Generator().manual_seed(11))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    want = orc.fla_layer_forward(sd, x, 2, 64, 128, norm_eps=1e-6, **opts)
    m = m.to(DEV).eval()
    xd = x.to(DEV)
    cache = modules.DecodeCache()
    with torch.no_grad():
        outs = [m(xd[:, :100], past_key_values=cache, use_cache=True)[0], m(xd[:, 100:190], past_key_values=cache, use_cache=True)[0]]
        assert cache.get_seq_length() == 190
        outs += [m(xd[:, t:t + 1], past_key_values=cache, use_cache=True)[0] for t in range(190, 200)]
    check("o (prefill + one call of 90 + 10 steps)", torch.cat(outs, dim=1), want, 1e-4)
    st = cache[0]["recurrent_state"]
    assert cache.get_seq_length() == 200 and isinstance(st, mhla_amd.CausalState) and st.seen == 200


def test_gpt_host_multi_token_call_on_a_cache():
    from mhla_amd.hosts.gpt import GPT_MHLA
    from mhla_amd.modules import DecodeCache
    torch.manual_seed(5)
    model = GPT_MHLA(vocab_size=512, hidden_size=128, num_layers=2, num_heads=4, max_seq_len=2048, exact_decoding=True).to(DEV).eval()
    ids = torch.randint(0, 512, (2, 151), generator=torch.Generator().manual_seed(6)).to(DEV)
    with torch.no_grad():
        full = model(ids)
        cache = DecodeCache()
        parts = [model(ids[:, :20], cache=cache), model(ids[:, 20:150], cache=cache), model(ids[:, 150:151], cache=cache)]
    assert cache.get_seq_length(0) == cache.get_seq_length(1) == 151
    check("logits: prefill(20) + 130 tokens + 1 token vs one forward", torch.cat(parts, dim=1), full.cpu(), 1e-4)
