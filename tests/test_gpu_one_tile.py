"""GPU: the one-tile instantiations of the block-mix token kernels (blocks of at most 64 tokens: k_sp_bwd_dq and k_sp_out
without the tile loop, its second row set and its look-ahead) and k_sp_state without the third row stream, against the instantiations they
replace (mhla_set_option("recut_kernels", 0)).  The arithmetic and its order are the same -- only requests disappear -- so the claim is bit
identity of every output, every gradient and the state the forward keeps; the oracle comparison at the suite's tolerances keeps a
wrong-but-consistent pair from passing, and the per-launch hook pins the launch list to mhla_describe_dispatch's."""
import ctypes

import pytest
import torch

from gpu_util import DEV, bm_tols, check, make_blockmix_inputs, oracle_blockmix, to_dev

pytestmark = pytest.mark.gpu

# what a call can ask of the kernels: (name, keyword arguments of the problem)
VARIANTS = [("default", {}),
            ("summaries=split", {"summaries": "split"}),
            ("no normaliser", {"normalize": False}),
            ("split q/k normaliser pair", {"split": True}),          # k_sp_state's third stream is real
            ("split pair, summaries=split", {"split": True, "summaries": "split"}),
            ("relu prologue", {"relu_eps": True}),                    # the token kernels' non-WQ form
            ("gather map", {"gather": True})]
SHAPES = [(1, 2, 4), (3, 1, 5)]   # (B, H, M): B H = 2 and 3


def _inputs(B, H, M, S, D, dtype, split, relu_eps, seed=7):
    q, k, v, W, do, qd, kd = make_blockmix_inputs(B, H, M, S, D, dtype, seed, "rand", split)
    if relu_eps:   # raw projections: the kernels apply relu(x) + eps themselves
        g = torch.Generator().manual_seed(seed + 1)
        q = torch.randn(q.shape, generator=g).to(dtype)
        k = torch.randn(k.shape, generator=g).to(dtype)
    return q, k, v, W, do, qd, kd


def _run_c_abi(B, H, M, S, D, dtype, *, normalize=True, split=False, summaries="tf32", relu_eps=False, gather=False):
    """Forward + backward through the C ABI with workspaces of the caller's (filled with one byte pattern first, so that words no kernel
    writes compare equal): every result and the forward's workspace -- the state it keeps for the backward -- as integer words."""
    from mhla_amd import _lib
    from mhla_amd.ops import _bm_flags, _view
    lib = _lib.load()
    q, k, v, W, do, qd, kd = to_dev(*_inputs(B, H, M, S, D, dtype, split, relu_eps))
    N = M * S
    idx = None
    if gather:   # block-major position p lives at row idx[p]
        idx = torch.randperm(N, generator=torch.Generator().manual_seed(3)).to(torch.int32).to(DEV)
        scat = lambda t: None if t is None else torch.empty_like(t).index_copy_(1, idx.long(), t)
        q, k, v, do, qd, kd = (scat(t) for t in (q, k, v, do, qd, kd))
    dt = {torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}[dtype]
    flags = _bm_flags(relu_eps, False, True, summaries)   # (no_smalln: bf16 blocks of 16 tokens would take the single-launch path)
    st = torch.cuda.current_stream().cuda_stream
    null = _lib.NULL_VIEW
    qdv, kdv = (null, null) if not normalize else (_view(qd), _view(kd)) if split else (_view(q), _view(k))
    ip = None if idx is None else idx.data_ptr()
    pattern = lambda nbytes: torch.full((nbytes // 4 + 4,), -1, dtype=torch.int32, device=DEV)
    fws = pattern(lib.mhla_blockmix_fwd_ws_bytes(B, H, M, S, D, dt, int(split), flags))
    out = torch.empty_like(q)
    rc = lib.mhla_blockmix_fwd(_view(q), _view(k), _view(v), qdv, kdv, W.data_ptr(), M, _view(out), ip, fws.data_ptr(), fws.numel() * 4,
                               B, H, M, S, D, dt, 1e-6, flags, st)
    assert rc == 0, lib.mhla_last_error()
    keeps = lib.mhla_blockmix_fwd_keeps_state(B, H, M, S, D, dt, int(split), flags)
    state = fws.clone()
    ws = pattern(lib.mhla_blockmix_bwd_ws_bytes(B, H, M, S, D, dt, int(split), flags))
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    dqd, dkd = (torch.empty_like(q), torch.empty_like(q)) if split else (None, None)
    dW = torch.empty(M, M, device=DEV)
    rc = lib.mhla_blockmix_bwd(_view(q), _view(k), _view(v), qdv, kdv, W.data_ptr(), M, _view(out), _view(do), _view(dq), _view(dk), _view(dv),
                               _view(dqd) if split else null, _view(dkd) if split else null, dW.data_ptr(), ip, ws.data_ptr(), ws.numel() * 4,
                               fws.data_ptr() if keeps else None, B, H, M, S, D, dt, 1e-6, flags, st)
    assert rc == 0, lib.mhla_last_error()
    torch.cuda.synchronize()
    res = {"out": out, "dq": dq, "dk": dk, "dv": dv, "dW": dW, "kept state": state}
    if split:
        res.update({"dq_den": dqd, "dk_den": dkd})
    words = lambda t: t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()
    return {name: words(t) for name, t in res.items()}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 72])
@pytest.mark.parametrize("S", [16, 40, 48, 64, 80])
def test_one_tile_kernels_are_bit_identical_to_the_loop_kernels(S, D, dtype):
    """S = 16: waves 1 .. 3 have no tile; 40: a partial last tile (clamped rows); 48 / 64: one tile on three / four waves; 80: one past the
    boundary (the loop kernels either way).  D = 72: five feature tiles, the lone last one.  Every output word with "recut_kernels" 1 and 0."""
    import mhla_amd
    for B, H, M in SHAPES:
        for name, kw in VARIANTS:
            new = _run_c_abi(B, H, M, S, D, dtype, **kw)
            prev = mhla_amd.set_option("recut_kernels", 0)
            try:
                old = _run_c_abi(B, H, M, S, D, dtype, **kw)
            finally:
                mhla_amd.set_option("recut_kernels", prev)
            assert prev == 1 and new.keys() == old.keys()
            for what in new:
                differ = int((new[what] != old[what]).sum())
                assert differ == 0, f"B H = {B * H}, M = {M}, S = {S}, D = {D}, {name}: {what} differs in {differ} of {new[what].numel()} words"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("S,D,split", [(40, 64, False), (64, 64, False), (64, 72, True)])
def test_one_tile_kernels_against_the_oracle(S, D, split, dtype):
    """The path the bit-identity test compares from, against the CPU oracle at the suite's tolerances (gpu_util.bm_tols)."""
    import mhla_amd
    B, H, M = 1, 3, 5
    otol, gtol, wtol = bm_tols(dtype, "tf32")
    q, k, v, W, do, qd, kd = make_blockmix_inputs(B, H, M, S, D, dtype, 11, "rand", split)
    want, wg = oracle_blockmix(q, k, v, W, do, qd, kd, 1e-6, True)
    t = to_dev(q, k, v, W, do, qd, kd)
    leaves = [x.requires_grad_(True) for x in t[:4]] + ([x.requires_grad_(True) for x in t[5:]] if split else [])
    out = mhla_amd.mhla_blockmix(t[0], t[1], t[2], t[3], eps=1e-6, q_den=t[5], k_den=t[6], no_smalln=True)
    out.backward(t[4])
    torch.cuda.synchronize()
    check("out", out, want, otol)
    for name, leaf in zip(("dq", "dk", "dv"), leaves):
        check(name, leaf.grad, wg[name], gtol)
    check("dW", leaves[3].grad, wg["dW"], wtol)
    if split:
        check("dq_den", leaves[4].grad, wg["dq_den"], gtol)
        check("dk_den", leaves[5].grad, wg["dk_den"], gtol)


@pytest.mark.parametrize("S,D,kw", [(64, 64, {}), (40, 64, {}), (16, 72, {}), (48, 64, {"split": True})], ids=["s64", "s40", "s16_d72", "s48_pair"])
def test_one_tile_launch_list_is_the_described_one(S, D, kw):
    """The new instantiations report under the names of the kernels they stand in for: the per-launch hook's record of a forward +
    backward equals mhla_describe_dispatch's lists."""
    import mhla_amd
    lib = mhla_amd._lib.load()
    B, H, M, dt = 1, 2, 4, torch.bfloat16
    split = bool(kw.get("split"))
    want = mhla_amd.describe_dispatch(B, H, M, S, D, dt, no_smalln=True, **kw)
    q, k, v, W, do, qd, kd = make_blockmix_inputs(B, H, M, S, D, dt, 1, "rand", split)
    t = [x.requires_grad_(True) for x in to_dev(q, k, v, W)]
    den = dict(zip(("q_den", "k_den"), to_dev(qd, kd))) if split else {}
    run = lambda: mhla_amd.mhla_blockmix(*t, no_smalln=True, **den).sum().backward()
    run()   # (first call: plans, LDS opt-ins)
    torch.cuda.synchronize()
    lib.mhla_prof_enable(1)
    run()
    torch.cuda.synchronize()
    lib.mhla_prof_enable(0)
    buf = ctypes.create_string_buffer(1 << 14)
    lib.mhla_prof_report(buf, len(buf))
    ran = sorted(line.rsplit(" ", 2)[0] for line in buf.value.decode().splitlines() for _ in range(int(line.rsplit(" ", 2)[1])))
    assert ran == sorted(want["fwd"] + want["bwd"]), (want["text"], ran)
