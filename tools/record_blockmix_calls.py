"""The block-mix section of `mhla_amd/ops.py` (`_bm_plan` ... `qk_prologue`: the block-mix operators, the DiT core, LePE, the rotary
feature map and the q / k prologue) run on CPU tensors, forward and backward, against a recording stand-in for the library
(tools/fake_decode_lib.py), with the Python autograd nodes forced (the C++ ones refuse CPU tensors): every library call with every
argument, the order of allocations, every exception's type and message, and the signature and docstring hash of every public name
of the section.  Two trees whose logs are byte-identical make the same calls in the same order on the same storage and refuse the
same things with the same words: the check of a refactor of that section (profiles/blockmix_host_refactor.md).

    python tools/record_blockmix_calls.py [--tree DIR] [-o LOG]     the log (sha256 on stderr); DIR: another checkout to import
    python tools/record_blockmix_calls.py --raises                  also list the `raise` lines of the section no scenario reached
    python tools/record_blockmix_calls.py --counts                  Python function calls per public call (cProfile), no log
"""
import argparse
import cProfile
import hashlib
import inspect
import itertools
import os
import pstats
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.join(HERE, ".."))
ap.add_argument("-o", "--output")
ap.add_argument("--raises", action="store_true")
ap.add_argument("--counts", action="store_true")
opt = ap.parse_args()
sys.path.insert(0, os.path.abspath(opt.tree))

import torch  # noqa: E402

from mhla_amd import _lib, ops  # noqa: E402
from mhla_amd import build as _build  # noqa: E402
from fake_decode_lib import Session  # noqa: E402

_build.build(verbose=False)
ops._native_nodes = lambda: False
B, M, S, H, D = 3, 4, 16, 2, 32
N, C = M * S, H * D
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
PUBLIC = ("set_keep_state_limits", "describe_dispatch", "describe_causal_dispatch", "set_option", "mhla_blockmix", "mhla_blockmix_rope",
          "lepe2d", "lepe3d", "mhla_blockmix_wan", "wan_pro_supported", "mhla_blockmix_wan_pro", "mhla_dit_core", "featmap_rotary",
          "qk_prologue")


def rand(*shape, dtype=F32, seed=0, grad=False):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).requires_grad_(grad)


def toks(dtype=F32, d=D, b=B, grad=True, n=N):
    return tuple(rand(b, n, H, d, dtype=dtype, seed=i, grad=grad) for i in (1, 2, 3))


def run(s, label, fn, names, wrt=(), dout=None):
    """One scenario as one recorded call: `fn()` and, with `wrt` (the inputs to differentiate), its backward on `dout` (one per
    output that is not None; default: random, allocated inside the call).  Both halves run inside the same call, so the storage the
    forward allocates keeps its name in the backward's arguments."""
    s.name(**names)

    def both():
        out = fn()
        if not wrt:
            return out
        every = out if isinstance(out, tuple) else (out,)
        outs = [o for o in every if o is not None and o.requires_grad]
        douts = dout if dout is not None else [rand(*o.shape, dtype=o.dtype, seed=7) for o in outs]
        return (*every, *torch.autograd.grad(outs, wrt, douts, allow_unused=True))
    return s.call(label, both)


class patched:
    """`with patched(KEEP_STATE_LIMIT_BYTES=0):` -- module globals of ops the section reads at call time."""

    def __init__(self, **values):
        self.values = values

    def __enter__(self):
        self.saved = {k: getattr(ops, k) for k in self.values}
        for k, v in self.values.items():
            setattr(ops, k, v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            setattr(ops, k, v)


def blockmix(s):
    bm = ops.mhla_blockmix

    def case(label, dtype=F32, d=D, b=B, W=None, grad=True, dout=None, n=N, **kw):
        q, k, v = toks(dtype, d, b, grad, n)
        W = rand(M, M, seed=4, grad=grad) if W is None else W
        extra = {n: t for n, t in kw.items() if isinstance(t, torch.Tensor)}
        wrt = [t for t in (q, k, v, W, *extra.values()) if t.requires_grad]
        run(s, f"blockmix {label}", lambda: bm(q, k, v, W, **kw), dict(q=q, k=k, v=v, W=W, **extra), wrt, dout)

    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5)).int()
    for dtype in (F32, BF16, F16):
        case(f"{dtype}", dtype)
        case(f"{dtype} q_den k_den", dtype, q_den=rand(B, N, H, D, dtype=dtype, seed=11, grad=True), k_den=rand(B, N, H, D, dtype=dtype, seed=12, grad=True))
    case("block_index", block_index=perm)
    case("normalize=False", normalize=False)
    case("relu_eps", relu_eps=True, eps=1e-5)
    for summaries in ops.SUMMARIES:
        case(f"summaries={summaries}", BF16, summaries=summaries)
    case("force_generic", BF16, force_generic=True)
    case("no_smalln", BF16, no_smalln=True)
    case("inputs without grad", grad=False)
    with torch.no_grad():
        case("under no_grad")
    case("W [M, M, 1, 1]", W=rand(M, M, 1, 1, seed=4, grad=True))
    case("W bf16", BF16, W=rand(M, M, dtype=BF16, seed=4, grad=True))
    W = rand(M, M, seed=4, grad=True)
    for dtype in (F32, BF16):
        proj = rand(B, N, 3 * C, dtype=dtype, seed=6, grad=True)
        run(s, f"blockmix views into a packed projection {dtype}", lambda: bm(*proj.view(B, N, 3, H, D).unbind(2), W), dict(proj=proj, W=W), (proj, W))
    q, k, v = toks()
    flat = rand(B * N * H * D + 2, seed=8, grad=True)
    run(s, "blockmix q contiguous at an 8-byte aligned base", lambda: bm(flat[2:].view(B, N, H, D), k, v, W), dict(flat=flat, k=k, v=v, W=W), (flat, k, v, W))
    flat3 = rand(B * N * 3 * C + 2, seed=8, grad=True)
    run(s, "blockmix views into a packed projection at an 8-byte aligned base", lambda: bm(*flat3[2:].view(B, N, 3, H, D).unbind(2), W),
        dict(flat=flat3, W=W), (flat3, W))
    wide = rand(B, N, H, 2 * D, seed=9, grad=True)
    run(s, "blockmix k with a strided last dim", lambda: bm(q, wide[..., ::2], v, W), dict(q=q, wide=wide, v=v, W=W), (q, wide, v, W))
    for label, dout in (("bf16", rand(B, N, H, D, dtype=BF16, seed=7)), ("fp64", rand(B, N, H, D, dtype=torch.float64, seed=7)),
                        ("transposed", rand(B, H, N, D, seed=7).transpose(1, 2)), ("expanded", rand(1, 1, 1, 1, seed=7).expand(B, N, H, D)),
                        ("strided last dim", rand(B, N, H, 2 * D, seed=7)[..., ::2])):
        s.name(dout=dout)
        case(f"dout {label}", dout=[dout])
    case("blocks of 64 tokens: the forward's workspace is kept", BF16, n=M * 64)   # (blocks of 16: one launch, nothing to keep)
    with patched(KEEP_STATE_LIMIT_BYTES=0):
        case("blocks of 64 tokens, KEEP_STATE_LIMIT_BYTES=0", BF16, n=M * 64)
        case("KEEP_STATE_LIMIT_BYTES=0", BF16)
        case("KEEP_STATE_LIMIT_BYTES=0 q_den k_den", q_den=rand(B, N, H, D, seed=11, grad=True), k_den=rand(B, N, H, D, seed=12, grad=True))
    case("B=0", b=0)
    with patched(_MAX_GRID_BH=2 * H):
        case("_MAX_GRID_BH=2H")
        case("_MAX_GRID_BH=2H q_den k_den block_index", BF16, q_den=rand(B, N, H, D, dtype=BF16, seed=11, grad=True),
             k_den=rand(B, N, H, D, dtype=BF16, seed=12, grad=True), block_index=perm)
    for d in (160, 136):
        case(f"D={d}", d=d)
        case(f"D={d} bf16 block_index relu_eps", BF16, d=d, block_index=perm, relu_eps=True)
        case(f"D={d} normalize=False", d=d, normalize=False)
    case("D=160 q_den k_den", d=160, q_den=rand(B, N, H, 160, seed=11, grad=True), k_den=rand(B, N, H, 160, seed=12, grad=True))
    os.environ["MHLA_CHECK_HANDOVER"] = "1"
    try:
        case("MHLA_CHECK_HANDOVER=1")
        case("MHLA_CHECK_HANDOVER=1 q_den k_den", BF16, q_den=rand(B, N, H, D, dtype=BF16, seed=11, grad=True), k_den=rand(B, N, H, D, dtype=BF16, seed=12, grad=True))
    finally:
        del os.environ["MHLA_CHECK_HANDOVER"]


def tables(n=N, d=D, dtype=F32):
    return rand(n, d // 2, dtype=dtype, seed=13), rand(n, d // 2, dtype=dtype, seed=14)


def rope(s):
    cos, sin = tables()
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5)).int()

    def case(label, dtype=F32, grad=True, **kw):
        q, k, v = toks(dtype, grad=grad)
        W = rand(M, M, 1, 1, seed=4, grad=grad)
        run(s, f"rope {label}", lambda: ops.mhla_blockmix_rope(q, k, v, W, cos, sin, **kw), dict(q=q, k=k, v=v, W=W, cos=cos, sin=sin, block_index=perm),
            (q, k, v, W) if grad else ())
    case("kept workspace")
    with patched(KEEP_STATE_LIMIT_BYTES=0):
        case("recomputed workspace")
    case("normalize=False block_index eps", normalize=False, block_index=perm, eps=1e-4)
    case("forward only", grad=False)
    case("bf16 forward only", BF16, grad=False)
    with torch.no_grad():
        case("bf16 under no_grad", BF16)
    case("bf16 with grad: refused", BF16)
    wide = rand(N, D, seed=13)
    q, k, v = toks()
    W = rand(M, M, seed=4, grad=True)
    run(s, "rope tables sliced out of wider ones", lambda: ops.mhla_blockmix_rope(q, k, v, W, wide[:, :D // 2], wide[:, D // 2:]),
        dict(q=q, k=k, v=v, W=W, wide=wide), (q, k, v, W))


def wan(s):
    cos, sin = tables()
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5)).int()
    q, k, v = toks(grad=False)
    W, nw, gate = rand(M, M, 1, 1, seed=4), rand(D, dtype=BF16, seed=15), rand(B, N, H, D, dtype=BF16, seed=16)
    names = dict(q=q, k=k, v=v, W=W, cos=cos, sin=sin, nw=nw, gate=gate, block_index=perm)
    for t, g, n in itertools.product((False, True), repeat=3):
        run(s, f"wan tables={t} gate={g} norm_weight={n}",
            lambda: ops.mhla_blockmix_wan(q, k, v, W, cos if t else None, sin if t else None, nw if n else None, 1e-6, gate if g else None, BF16), names)
    run(s, "wan block_index normalize=False fp32 out", lambda: ops.mhla_blockmix_wan(q, k, v, W, cos, sin, nw.float(), 1e-5, None, F32, eps=1e-5,
                                                                                    normalize=False, block_index=perm), names)
    proj = rand(B, N, 3 * C, seed=6)
    run(s, "wan views into a packed projection", lambda: ops.mhla_blockmix_wan(*proj.view(B, N, 3, H, D).unbind(2), W, cos, sin, nw, 1e-6, gate, BF16),
        dict(proj=proj, **names))
    run(s, "wan with a leaf that requires grad: refused", lambda: ops.mhla_blockmix_wan(q, k, v, W.clone().requires_grad_(), cos, sin, nw, 1e-6, gate, BF16), names)
    with torch.no_grad():
        run(s, "wan with that leaf under no_grad", lambda: ops.mhla_blockmix_wan(q, k, v, W.clone().requires_grad_(), cos, sin, nw, 1e-6, gate, BF16), names)


def wan_pro(s):
    cos, sin = tables()
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5)).int()
    proj = rand(B, N, 3 * C, dtype=BF16, seed=6)
    q, k, v = proj.view(B, N, 3 * H, D).split(H, dim=2)   # each [B, N, H, D] with the heads of a token contiguous
    W, nw, gate = rand(M, M, seed=4), rand(D, seed=15), rand(B, N, H, D, dtype=BF16, seed=16)
    wq, wk = rand(C, dtype=BF16, seed=17), rand(C, seed=18)
    names = dict(proj=proj, W=W, cos=cos, sin=sin, nw=nw, gate=gate, wq=wq, wk=wk, block_index=perm)
    pro = ops.mhla_blockmix_wan_pro
    for qk_norm, w, t, g in itertools.product((True, False), repeat=4):
        run(s, f"wan_pro qk_norm={qk_norm} wq/wk={w} tables={t} gate={g}",
            lambda: pro(q, k, v, wq if w else None, wk if w else None, 1e-6, W, cos if t else None, sin if t else None, nw if g else None, 1e-6,
                        gate if g else None, qk_norm=qk_norm), names)
    run(s, "wan_pro block_index normalize=False", lambda: pro(q, k, v, wq, wk, 1e-5, W, cos, sin, nw, 1e-5, gate, eps=1e-5, normalize=False, block_index=perm), names)
    qf, kf, vf = toks(F16, grad=False)
    run(s, "wan_pro fp16 tensors of their own", lambda: pro(qf, kf, vf, None, None, 1e-6, W, None, None, None, 1e-6, None), dict(q=qf, k=kf, v=vf, **names))
    run(s, "wan_pro_supported", lambda: (ops.wan_pro_supported(q, M), ops.wan_pro_supported(q.float(), M), ops.wan_pro_supported(q, 7)), names)


def dit_core(s):
    W = rand(M, M, 1, 1, seed=4, grad=True)
    lw, lb = rand(C, 1, 3, 3, seed=20, grad=True), rand(C, seed=21, grad=True)

    def case(label, dtype=BF16, bias=True, qkv=None, grad=True, block_len=4, **kw):
        qkv = rand(B, (2 * block_len) ** 2, 3, H, D, dtype=dtype, seed=6, grad=grad) if qkv is None else qkv
        wrt = [qkv, W, lw] + ([lb] if bias else []) if grad else ()
        run(s, f"dit_core {label}", lambda: ops.mhla_dit_core(qkv, W, lw, lb if bias else None, 2, block_len, **kw), dict(qkv=qkv, W=W, lw=lw, lb=lb), wrt)
    case("bf16")
    case("blocks of 64 tokens: kept", block_len=8)
    with patched(KEEP_STATE_LIMIT_BYTES=0):
        case("blocks of 64 tokens: recomputed", block_len=8)
    case("fp32 without the LePE bias", F32, bias=False)
    with patched(KEEP_STATE_LIMIT_BYTES=0):
        case("recomputed")
    case("relu_eps=False split summaries eps", relu_eps=False, summaries="split", eps=1e-5)
    base = rand(3, B, N, H, D, dtype=BF16, seed=6, grad=True)
    s.name(base=base)
    case("non-contiguous qkv", qkv=base.permute(1, 2, 0, 3, 4))
    with torch.no_grad():
        case("under no_grad")
    case("inputs without grad", grad=False)
    lw5 = rand(C, 1, 5, 5, seed=20, grad=True)
    qkv = rand(B, N, 3, H, D, seed=6, grad=True)
    run(s, "dit_core 5 x 5 LePE", lambda: ops.mhla_dit_core(qkv, W, lw5, lb, 2, 4), dict(qkv=qkv, W=W, lw=lw5, lb=lb), (qkv, W, lw5, lb))


def subsets(xs):
    return itertools.chain.from_iterable(itertools.combinations(xs, n) for n in range(len(xs) + 1))


def lepe(s):
    for dims, k_sizes in ((2, (3, 5)), (3, (3,))):
        for K in k_sizes:
            for bias, add in itertools.product((False, True), repeat=2):
                present = ["v", "weight"] + (["bias"] if bias else []) + (["add"] if add else [])
                for req in subsets(present) if (bias and add) else (tuple(present), ()):
                    t = dict(v=rand(B, N, C, dtype=BF16, seed=1, grad="v" in req), weight=rand(C, 1, *(K,) * dims, seed=20, grad="weight" in req),
                             bias=rand(C, seed=21, grad="bias" in req) if bias else None,
                             add=rand(B, N, C, dtype=BF16, seed=22, grad="add" in req) if add else None)
                    if dims == 2:
                        fn = lambda: ops.lepe2d(t["v"], t["weight"], t["bias"], 2, 4, t["add"])
                    else:
                        fn = lambda: ops.lepe3d(t["v"], t["weight"], t["bias"], (4, 2, 8), t["add"])
                    run(s, f"lepe{dims}d K={K} bias={bias} add={add} requires grad: {', '.join(req) or 'nothing'}", fn, t, [t[n] for n in req])
    v4 = rand(B, N, H, 2 * D, dtype=BF16, seed=1, grad=True)
    w = rand(C, 1, 3, 3, seed=20, grad=True)
    run(s, "lepe2d v with strided channels", lambda: ops.lepe2d(v4[..., ::2].reshape(B, N, C), w, None, 2, 4), dict(v=v4, weight=w), (v4, w))
    packed = rand(B, N, 3 * C, seed=6, grad=True)
    w3 = rand(C, 1, 3, 3, 3, seed=20, grad=True)
    run(s, "lepe3d v a slice of a packed projection", lambda: ops.lepe3d(packed[..., 2 * C:], w3, None, (4, 4, 4), packed[..., :C]),
        dict(packed=packed, weight=w3), (packed, w3))


def featmap_rotary(s):
    T, K = N, D
    for dtype, fmap, off in itertools.product((F32, BF16), (None, "identity", "relu", "elu"), (0, 5)):
        x = rand(B, T, H, K, dtype=dtype, seed=1, grad=True)
        cos, sin = tables(T + off, K, dtype)
        run(s, f"featmap_rotary {dtype} {fmap} t_offset={off}", lambda: ops.featmap_rotary(x, cos, sin, fmap, off), dict(x=x, cos=cos, sin=sin), (x,))
    x = rand(B, T, H, K, seed=1, grad=True)
    wide = rand(T + 5, K, seed=13)
    run(s, "featmap_rotary tables sliced out of a wider one", lambda: ops.featmap_rotary(x, wide[:, :K // 2], wide[:, K // 2:], "relu", 3), dict(x=x, wide=wide), (x,))
    run(s, "featmap_rotary tables of differing row strides", lambda: ops.featmap_rotary(x, wide[:T, :K // 2], tables(T, K)[1]), dict(x=x, wide=wide), (x,))
    run(s, "featmap_rotary tables strided in their last dim", lambda: ops.featmap_rotary(x, wide[:, ::2], wide[:, 1::2]), dict(x=x, wide=wide), (x,))
    proj = rand(B, T, 3 * H * K, dtype=BF16, seed=6, grad=True)
    cos, sin = tables(T, K, BF16)
    run(s, "featmap_rotary x a view into a packed projection", lambda: ops.featmap_rotary(proj.view(B, T, 3, H, K)[:, :, 1], cos, sin, "elu"),
        dict(proj=proj, cos=cos, sin=sin), (proj,))
    with torch.no_grad():
        run(s, "featmap_rotary under no_grad", lambda: ops.featmap_rotary(x, cos.float(), sin.float()), dict(x=x))


def qk_prologue(s):
    cos, sin = tables()
    for dtype, weight in itertools.product((BF16, F32), (False, True)):
        x = rand(B, N, C, dtype=dtype, seed=1, grad=True)
        w = rand(C, dtype=dtype, seed=17, grad=True) if weight else None
        names, wrt = dict(x=x, w=w, cos=cos, sin=sin), [x] + ([w] if weight else [])
        run(s, f"qk_prologue {dtype} weight={weight}", lambda: ops.qk_prologue(x, w, 1e-5, 1e-6), names, wrt)
        run(s, f"qk_prologue {dtype} weight={weight} rope", lambda: ops.qk_prologue(x, w, rope=(cos, sin), head_dim=D), names, wrt)
        run(s, f"qk_prologue {dtype} weight={weight} rope, gradient from y alone", lambda: ops.qk_prologue(x, w, rope=(cos, sin), head_dim=D)[0], names, wrt)
        run(s, f"qk_prologue {dtype} weight={weight} rope, gradient from y_rope alone", lambda: ops.qk_prologue(x, w, rope=(cos, sin), head_dim=D)[1], names, wrt)
    x = rand(B, N, 2 * C, seed=1, grad=True)
    run(s, "qk_prologue x with a strided last dim", lambda: ops.qk_prologue(x[..., ::2], None), dict(x=x), (x,))
    run(s, "qk_prologue x [B, N, H, D] a slice of wider rows", lambda: ops.qk_prologue(x[..., :C].unflatten(2, (H, D)), None, rope=(cos, sin), head_dim=D), dict(x=x), (x,))
    with torch.no_grad():
        run(s, "qk_prologue under no_grad", lambda: ops.qk_prologue(x[..., :C], None, rope=(cos, sin), head_dim=D), dict(x=x))


def others(s):
    for dtype, kw in ((BF16, {}), (F32, {}), (BF16, dict(summaries="split")), (BF16, dict(split=True, relu_eps=True)), (F16, dict(force_generic=True, no_smalln=True))):
        s.call(f"describe_dispatch {dtype} {kw}", ops.describe_dispatch, 32, 16, 16, 16, 72, dtype, **kw)
    s.call("describe_dispatch of a refused problem", ops.describe_dispatch, 32, 16, 16, 16, 500, BF16)
    s.call("describe_dispatch summaries", ops.describe_dispatch, 32, 16, 16, 16, 72, BF16, summaries="fp8")
    s.call("describe_causal_dispatch", ops.describe_causal_dispatch, 512, 64, 128, BF16)
    s.call("describe_causal_dispatch split, chunk 32", ops.describe_causal_dispatch, 512, 64, 128, BF16, chunk_size=32, summaries="split", force_generic=True)
    q, k, v = toks(BF16)
    W = rand(M, M, seed=4, grad=True)
    names = dict(q=q, k=k, v=v, W=W)
    run(s, "a call whose plan is cached", lambda: ops.mhla_blockmix(q, k, v, W), names, (q, k, v, W))
    s.call("set_option fp32_summaries 1", ops.set_option, "fp32_summaries", 1)
    run(s, "the same call asks for its sizes again", lambda: ops.mhla_blockmix(q, k, v, W), names, (q, k, v, W))
    s.call("set_option fp32_summaries 0", ops.set_option, "fp32_summaries", 0)
    run(s, "and again", lambda: ops.mhla_blockmix(q, k, v, W), names, (q, k, v, W))
    s.call("set_option of no such option", ops.set_option, "no_such_option", 1)
    saved = ops.set_keep_state_limits()
    s.call("set_keep_state_limits()", ops.set_keep_state_limits)
    s.call("set_keep_state_limits(blockmix=0)", ops.set_keep_state_limits, blockmix=0)
    run(s, "a call under that limit recomputes", lambda: ops.mhla_blockmix(q, k, v, W), names, (q, k, v, W))
    s.call("set_keep_state_limits(causal=1 << 20)", ops.set_keep_state_limits, causal=1 << 20)
    s.call("set_keep_state_limits restored", ops.set_keep_state_limits, *saved)


def refusals(s):
    """Every `raise` of the section, once at least, and the shared checks through each public call."""
    call = lambda label, fn, *a, **kw: s.call(f"refusal: {label}", fn, *a, **kw)
    meta = torch.device("meta")
    q, k, v = toks(grad=False)
    W, cos, sin = rand(M, M, seed=4), *tables()
    perm = torch.arange(N, dtype=torch.int32)
    bm = ops.mhla_blockmix
    call("blockmix q_den alone", bm, q, k, v, W, q_den=q)
    call("blockmix rank", bm, q[0], k, v, W)
    call("blockmix block_index dtype", bm, q, k, v, W, block_index=perm.long())
    call("blockmix block_index strided", bm, q, k, v, W, block_index=torch.arange(2 * N, dtype=torch.int32)[::2])
    call("blockmix block_index elsewhere", bm, q, k, v, W, block_index=perm.to(meta))
    call("blockmix block_index length", bm, q, k, v, W, block_index=perm[:-1])
    call("blockmix summaries", bm, q, k, v, W, summaries="fp8")
    call("blockmix N not divisible", bm, q, k, v, rand(5, 5))
    call("blockmix q_den with normalize=False", bm, q, k, v, W, q_den=q, k_den=k, normalize=False)
    call("blockmix k shape", bm, q, k[:, :, :1], v, W)
    call("blockmix v dtype", bm, q, k, v.double(), W)
    call("blockmix k elsewhere", bm, q, k.to(meta), v, W)
    call("blockmix q_den shape", bm, q, k, v, W, q_den=q[:2], k_den=k)
    call("blockmix W columns", bm, q, k, v, rand(M, M + 1))
    call("blockmix W rank", bm, q, k, v, rand(M))
    call("blockmix W elsewhere", bm, q, k, v, W.to(meta))
    call("blockmix dtype", bm, q.double(), k.double(), v.double(), W)
    call("blockmix 5-D tensors passed as 4-D views", bm, q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), W)
    q160 = rand(B, N, H, 160)
    call("blockmix wide head relu_eps with q_den", bm, q160, q160, q160, W, q_den=q160, k_den=q160, relu_eps=True)
    call("blockmix wide head N not divisible", bm, q160, q160, q160, rand(5, 5))
    qg, kg, vg = toks()
    s.name(q=qg, k=kg, v=vg, W=W)
    call("blockmix backward dout shape", lambda: torch.autograd.grad(bm(qg, kg, vg, W)[:2], (qg,), rand(2, N, H, D)))
    rp = ops.mhla_blockmix_rope
    call("rope N not divisible", rp, q, k, v, rand(5, 5), cos, sin)
    call("rope k shape", rp, q, k[:, :, :1], v, W, cos, sin)
    call("rope block_index length", rp, q, k, v, W, cos, sin, block_index=perm[:-1])
    call("rope table shape", rp, q, k, v, W, cos[:-1], sin)
    call("rope table dtype", rp, q, k, v, W, cos, sin.double())
    call("rope fp32 D % 8 with grad", rp, *toks(d=36), W, *tables(d=36))
    call("rope bf16 with grad", rp, *toks(BF16), W, cos, sin)
    call("rope dtype", rp, q.double(), k.double(), v.double(), W, cos, sin)
    for dims, fn, geom, w in ((2, ops.lepe2d, (2, 4), rand(C, 1, 3, 3)), (3, ops.lepe3d, ((4, 4, 4),), rand(C, 1, 3, 3, 3))):
        x = rand(B, N, C)
        call(f"lepe{dims}d v rank", fn, x[0], w, None, *geom)
        call(f"lepe{dims}d weight rank", fn, x, w[0], None, *geom)
        call(f"lepe{dims}d weight not depthwise", fn, x, w.expand(C, 2, *w.shape[2:]), None, *geom)
        call(f"lepe{dims}d weight not cubic", fn, x, w[..., :2], None, *geom)
        call(f"lepe{dims}d N", fn, x[:, :-1], w, None, *geom)
        call(f"lepe{dims}d channels", fn, x, w[:-1], None, *geom)
        call(f"lepe{dims}d dtype", fn, x.double(), w, None, *geom)
    wn = ops.mhla_blockmix_wan
    nw, gate = rand(D), rand(B, N, H, D, dtype=BF16)
    call("wan requires grad", wn, q, k.clone().requires_grad_(), v, W, cos, sin, nw, 1e-6, gate, BF16)
    call("wan norm weight requires grad", wn, q, k, v, W, cos, sin, nw.clone().requires_grad_(), 1e-6, gate, BF16)
    call("wan bf16 tensors", wn, q.bfloat16(), k.bfloat16(), v.bfloat16(), W, cos, sin, nw, 1e-6, gate, BF16)
    call("wan N not divisible", wn, q, k, v, rand(5, 5), cos, sin, nw, 1e-6, gate, BF16)
    call("wan v shape", wn, q, k, v[:, :, :1], W, cos, sin, nw, 1e-6, gate, BF16)
    call("wan block_index dtype", wn, q, k, v, W, cos, sin, nw, 1e-6, gate, BF16, block_index=perm.long())
    call("wan table shape", wn, q, k, v, W, cos, sin[:, :-1], nw, 1e-6, gate, BF16)
    call("wan gate dtype", wn, q, k, v, W, cos, sin, nw, 1e-6, gate.float(), BF16)
    call("wan gate shape", wn, q, k, v, W, None, None, nw, 1e-6, gate[:, :-1], BF16)
    call("wan out dtype", wn, q, k, v, W, None, None, nw, 1e-6, None, torch.float64)
    pro = ops.mhla_blockmix_wan_pro
    qb, kb, vb = toks(BF16, grad=False)
    wq = rand(C)
    call("wan_pro requires grad", pro, qb, kb, vb, wq.clone().requires_grad_(), wq, 1e-6, W, cos, sin, nw, 1e-6, gate)
    call("wan_pro N not divisible", pro, qb, kb, vb, wq, wq, 1e-6, rand(5, 5), cos, sin, nw, 1e-6, gate)
    call("wan_pro k dtype", pro, qb, kb.float(), vb, wq, wq, 1e-6, W, cos, sin, nw, 1e-6, gate)
    call("wan_pro block_index length", pro, qb, kb, vb, wq, wq, 1e-6, W, cos, sin, nw, 1e-6, gate, block_index=perm[:-1])
    call("wan_pro dtype", pro, qb.double(), kb.double(), vb.double(), wq, wq, 1e-6, W, cos, sin, nw, 1e-6, gate)
    padded = rand(B, N, H, 2 * D, dtype=BF16)
    s.name(padded=padded, k=kb, v=vb)
    call("wan_pro heads of a token apart", pro, padded[..., :D], kb, vb, wq, wq, 1e-6, W, cos, sin, nw, 1e-6, gate)
    call("wan_pro heads of a token apart, qk_norm=False", pro, padded[..., :D], kb, vb, None, None, 1e-6, W, None, None, None, 1e-6, None, qk_norm=False)
    longer = rand(B, 2 * N, H, D, dtype=BF16)
    s.name(longer=longer)
    call("wan_pro k batch stride", pro, qb, longer[:, :N], vb, wq, wq, 1e-6, W, cos, sin, nw, 1e-6, gate)
    call("wan_pro table dtype", pro, qb, kb, vb, wq, wq, 1e-6, W, cos.double(), sin, nw, 1e-6, gate)
    call("wan_pro gate dtype", pro, qb, kb, vb, wq, wq, 1e-6, W, cos, sin, nw, 1e-6, gate.half())
    call("wan_pro gate shape", pro, qb, kb, vb, wq, wq, 1e-6, W, cos, sin, nw, 1e-6, gate[:2])
    dc = ops.mhla_dit_core
    qkv, lw = rand(B, N, 3, H, D), rand(C, 1, 3, 3)
    call("dit_core rank", dc, qkv[0], W, lw, None, 2, 4)
    call("dit_core not three slices", dc, qkv[:, :, :2], W, lw, None, 2, 4)
    call("dit_core N not divisible", dc, qkv, rand(5, 5), lw, None, 2, 4)
    call("dit_core block layout", dc, qkv, W, lw, None, 2, 2)
    call("dit_core summaries", dc, qkv, W, lw, None, 2, 4, summaries="fp8")
    call("dit_core dtype", dc, qkv.double(), W, lw, None, 2, 4)
    fr = ops.featmap_rotary
    x, (c16, s16) = rand(B, N, H, D), tables(N + 4)
    call("featmap_rotary rank", fr, x[0], c16, s16)
    call("featmap_rotary K % 8", fr, x[..., :12], c16[:, :6], s16[:, :6])
    call("featmap_rotary feature map", fr, x, c16, s16, "gelu")
    call("featmap_rotary table dtype", fr, x, c16.bfloat16(), s16)
    call("featmap_rotary table width", fr, x, c16[:, :-1], s16[:, :-1])
    call("featmap_rotary table rows", fr, x, c16, s16, None, 5)
    call("featmap_rotary dtype", fr, x.double(), c16.double(), s16.double())
    qp = ops.qk_prologue
    x3 = rand(B, N, C)
    call("qk_prologue channels % 8", qp, x3[..., :12], None)
    call("qk_prologue rope without head_dim", qp, x3, None, rope=(cos, sin))
    call("qk_prologue rope table dtype", qp, x3, None, rope=(cos.double(), sin), head_dim=D)
    call("qk_prologue rope table shapes", qp, x3, None, rope=(cos, sin[:-1]), head_dim=D)
    call("qk_prologue rope table width", qp, x3, None, rope=(cos, sin), head_dim=D // 2)
    call("qk_prologue head_dim not dividing", qp, x3, None, rope=tables(N, 48), head_dim=48)
    call("qk_prologue dtype", qp, x3.double(), None)


def record():
    lines = []
    for name in PUBLIC:
        obj = getattr(ops, name)
        lines.append(f"{name}{inspect.signature(obj)} doc {hashlib.sha256((obj.__doc__ or '').encode()).hexdigest()}")
    lines.append(f"SUMMARIES = {ops.SUMMARIES!r}")
    with Session(ops, _lib) as s:
        for part in (blockmix, rope, wan, wan_pro, dit_core, lepe, featmap_rotary, qk_prologue, others, refusals):
            part(s)
    return lines + s.lines


def raise_lines():
    src = open(ops.__file__).read().split("\n")
    lo = next(i for i, ln in enumerate(src) if ln.startswith("def _bm_plan"))
    hi = next(i for i, ln in enumerate(src) if ln.startswith("# causal chunk-mixing MHLA (fla)"))
    return {i + 1 for i in range(lo, hi) if src[i].lstrip().startswith("raise ")}, src


def count_calls():
    """Python function calls (cProfile, builtins included) of one public call's forward and of its backward, caches warm; the count
    does not depend on the machine."""
    out = []
    cos, sin = tables()
    W = rand(M, M, seed=4, grad=True)
    lw, lb = rand(C, 1, 3, 3, seed=20, grad=True), rand(C, seed=21, grad=True)
    lw3 = rand(C, 1, 3, 3, 3, seed=20, grad=True)
    gate, nw = rand(B, N, H, D, dtype=BF16, seed=16), rand(D, seed=15)
    with Session(ops, _lib):
        def profiled(fn):
            prof = cProfile.Profile()
            prof.enable()
            result = fn()
            prof.disable()
            return result, pstats.Stats(prof).total_calls

        def measure(label, make, backward=True):
            """`make()`: (the forward as a function of no arguments, the inputs to differentiate)"""
            for warm in (True, False):   # (warm: the cached workspace sizes)
                fwd, wrt = make()
                result, n_fwd = profiled(fwd)
                if backward:
                    outs = [o for o in (result if isinstance(result, tuple) else (result,)) if o is not None]
                    douts = [rand(*o.shape, dtype=o.dtype, seed=7) for o in outs]
                    _, n_bwd = profiled(lambda: torch.autograd.grad(outs, wrt, douts))
            out.append(f"{label} forward: {n_fwd}")
            if backward:
                out.append(f"{label} backward: {n_bwd}")

        def bm(dtype, **kw):
            def make():
                q, k, v = toks(dtype)
                extra = {n: rand(B, N, H, D, dtype=dtype, seed=11, grad=True) for n in kw.get("den", ())}
                return (lambda: ops.mhla_blockmix(q, k, v, W, **extra)), (q, k, v, W, *extra.values())
            return make
        measure("mhla_blockmix fp32", bm(F32))
        measure("mhla_blockmix bf16", bm(BF16))
        measure("mhla_blockmix bf16 q_den k_den", bm(BF16, den=("q_den", "k_den")))

        def rope_make():
            q, k, v = toks()
            return (lambda: ops.mhla_blockmix_rope(q, k, v, W, cos, sin)), (q, k, v, W)
        measure("mhla_blockmix_rope fp32", rope_make)
        q, k, v = toks(grad=False)
        measure("mhla_blockmix_wan tables, gate, norm weight", lambda: ((lambda: ops.mhla_blockmix_wan(q, k, v, W.detach(), cos, sin, nw, 1e-6, gate, BF16)), ()), False)
        measure("mhla_blockmix_wan bare", lambda: ((lambda: ops.mhla_blockmix_wan(q, k, v, W.detach(), None, None, None, 1e-6, None, BF16)), ()), False)
        qb, kb, vb = toks(BF16, grad=False)
        wq = rand(C)
        measure("mhla_blockmix_wan_pro tables, gate, norm weights",
                lambda: ((lambda: ops.mhla_blockmix_wan_pro(qb, kb, vb, wq, wq, 1e-6, W.detach(), cos, sin, nw, 1e-6, gate)), ()), False)
        measure("mhla_blockmix_wan_pro qk_norm=False, bare",
                lambda: ((lambda: ops.mhla_blockmix_wan_pro(qb, kb, vb, None, None, 1e-6, W.detach(), None, None, None, 1e-6, None, qk_norm=False)), ()), False)

        def dit_make():
            qkv = rand(B, N, 3, H, D, dtype=BF16, seed=6, grad=True)
            return (lambda: ops.mhla_dit_core(qkv, W, lw, lb, 2, 4)), (qkv, W, lw, lb)
        measure("mhla_dit_core bf16, LePE bias", dit_make)

        def lepe_make(dims):
            def make():
                x, add = rand(B, N, C, dtype=BF16, seed=1, grad=True), rand(B, N, C, dtype=BF16, seed=22, grad=True)
                if dims == 2:
                    return (lambda: ops.lepe2d(x, lw, lb, 2, 4, add)), (x, lw, lb, add)
                return (lambda: ops.lepe3d(x, lw3, lb, (4, 4, 4), add)), (x, lw3, lb, add)
            return make
        measure("lepe2d bias, add", lepe_make(2))
        measure("lepe3d bias, add", lepe_make(3))

        def fr_make():
            x = rand(B, N, H, D, seed=1, grad=True)
            return (lambda: ops.featmap_rotary(x, cos, sin, "relu")), (x,)
        measure("featmap_rotary relu", fr_make)

        def qp_make(with_rope):
            def make():
                x, w = rand(B, N, C, dtype=BF16, seed=1, grad=True), rand(C, seed=17, grad=True)
                return (lambda: ops.qk_prologue(x, w, rope=(cos, sin) if with_rope else None, head_dim=D if with_rope else None)), (x, w)
            return make
        measure("qk_prologue weight", qp_make(False))
        measure("qk_prologue weight, rope", qp_make(True))
    return out


if __name__ == "__main__":
    if opt.counts:
        print("\n".join(count_calls()))
        sys.exit(0)
    seen = set()
    if opt.raises:
        path = ops.__file__

        def tracer(frame, event, arg):
            if frame.f_code.co_filename != path:
                return None
            if event == "line":
                seen.add(frame.f_lineno)
            return tracer
        sys.settrace(tracer)
    log = "\n".join(record()) + "\n"
    sys.settrace(None)
    if opt.output:
        open(opt.output, "w").write(log)
    else:
        sys.stdout.write(log)
    print(f"sha256 {hashlib.sha256(log.encode()).hexdigest()}  {log.count(chr(10))} lines", file=sys.stderr)
    if opt.raises:
        want, src = raise_lines()
        for n in sorted(want - seen):
            print(f"never raised: {n}: {src[n - 1].strip()[:120]}", file=sys.stderr)
        print(f"{len(want & seen)} of {len(want)} raise statements of the section were reached", file=sys.stderr)
