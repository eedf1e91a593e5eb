"""Operator-level API: torch.autograd Functions over the C ABI (libmhla_hip.so).

PyTorch is plumbing here (device memory, streams, autograd graph); every FLOP of the operator
runs in the hand-written HIP kernels.  There is no eager / CPU fallback: tensors must live on
a ROCm device and the library must be built, otherwise these functions raise.
"""
from __future__ import annotations

import functools
import heapq
import os
import warnings
from typing import NamedTuple, Optional

import torch

from . import _lib, _native
from ._lib import NULL_VIEW, View

# Autograd nodes in C++ (csrc_torch/mhla_torch.cpp) for the two plain operators when libmhla_torch.so is built: the eager host
# path of a forward + backward drops from ~180 us to the cost of the allocations and two C calls.  False forces the Python nodes
# below (same C ABI); MHLA_CHECK_HANDOVER=1 (a debugging aid of the Python nodes) does too.
USE_NATIVE_NODES = True


def _native_nodes() -> bool:
    return USE_NATIVE_NODES and _native.available() and os.environ.get("MHLA_CHECK_HANDOVER") != "1"

# (batch, head) pairs one launch of the library addresses (grid.y); larger batches are sliced by the operators below
_MAX_GRID_BH = 65535

# query heads one k/v head serves in the grouped decode calls (the library's CST_GMAX)
_MAX_KV_GROUP = 8


def _kv_group(fn: str, H: int, Hkv: int) -> int:
    """G = H / Hkv of a decode call whose k, v have Hkv heads and q has H (query head h uses k/v head h // G, the layer's repeat
    order); host arithmetic, raised before the library is loaded or a state is touched."""
    if Hkv == H:
        return 1
    if Hkv < 1 or H % Hkv:
        raise ValueError(f"{fn}: q has H={H} heads and k, v have Hkv={Hkv}: H must be a multiple of Hkv (grouped-query heads)")
    if H // Hkv > _MAX_KV_GROUP:
        raise NotImplementedError(f"{fn}: H={H} query heads on Hkv={Hkv} k/v heads: at most {_MAX_KV_GROUP} per k/v head are supported")
    return H // Hkv

# Forward workspaces up to these sizes are kept alive for the backward (block / chunk summaries); beyond the limit the backward
# recomputes them.  The memory is held per LAYER between its forward and its backward: the causal pipeline's hi + lo chunk
# summaries are 0.54 GB per layer at the 340M fla shape (B = 4, T = 8192) and 1.07 GB at the 1.3B-like one (B = 2) -- 13 / 26 GB
# over 24 layers -- so the causal operator has its own limit; `set_keep_state_limits` (or the fla layer's `keep_state_limit`
# argument) lowers it where memory matters more than the ~25 % of the backward the recomputation costs.
KEEP_STATE_LIMIT_BYTES = 4 << 30
CAUSAL_KEEP_STATE_LIMIT_BYTES = 4 << 30


def set_keep_state_limits(blockmix: Optional[int] = None, causal: Optional[int] = None):
    """Largest forward workspace (bytes) each operator keeps alive for its backward; 0 = always recompute.  Returns the pair in
    force.  Process-wide defaults; `mhla_causal(..., keep_state_limit=...)` overrides per call."""
    global KEEP_STATE_LIMIT_BYTES, CAUSAL_KEEP_STATE_LIMIT_BYTES
    if blockmix is not None:
        KEEP_STATE_LIMIT_BYTES = int(blockmix)
    if causal is not None:
        CAUSAL_KEEP_STATE_LIMIT_BYTES = int(causal)
    return KEEP_STATE_LIMIT_BYTES, CAUSAL_KEEP_STATE_LIMIT_BYTES

_DTYPES = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}


def _dtype_code(t: torch.Tensor) -> int:
    try:
        return _DTYPES[t.dtype]
    except KeyError:
        raise TypeError(f"mhla_amd: unsupported dtype {t.dtype} (float32 / bfloat16 / float16)") from None


def _require_gpu(*ts: torch.Tensor):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "mhla_amd operators run only on a ROCm GPU through libmhla_hip.so; got a "
                f"{t.device} tensor (there is no CPU fallback)")


def _device_guard(fn):
    """Run `fn` with the device of its first GPU tensor argument current, so that `_stream()` is that device's stream and
    the library launches on it (a tensor on cuda:1 while cuda:0 is current would otherwise be launched on the wrong GPU)."""
    @functools.wraps(fn)
    def wrapped(*args, **kw):
        dev = next((a.device for a in args if isinstance(a, torch.Tensor) and a.is_cuda), None)
        # (the common case -- the tensor's device is already current -- costs one C call: an eager fwd+bwd of the DiT shape is
        # bound by the host, tools/host_overhead.py)
        if dev is None or dev.index == torch._C._cuda_getDevice():
            return fn(*args, **kw)
        with torch.cuda.device(dev):
            return fn(*args, **kw)
    return wrapped


def _check_like(ref: torch.Tensor, what: str, **tensors):
    """The C ABI receives raw pointers + strides: shape, dtype and device agreement is checked here, where it is cheap.
    Every named tensor must have `ref`'s dtype and device; a tuple value is (tensor, expected_shape)."""
    for name, t in tensors.items():
        shape = None
        if isinstance(t, tuple):
            t, shape = t
        if t is None:
            continue
        if t.device != ref.device:
            raise ValueError(f"{what}: {name} is on {t.device}, expected {ref.device}")
        if t.dtype != ref.dtype:
            raise TypeError(f"{what}: {name} has dtype {t.dtype}, expected {ref.dtype} (cast it: the kernels read every "
                            "token tensor with one element type)")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")


def _check_block_index(block_index: Optional[torch.Tensor], N: int, ref: torch.Tensor):
    if block_index is None:
        return
    if block_index.dtype != torch.int32 or not block_index.is_contiguous():
        raise TypeError("block_index must be a contiguous int32 tensor")
    if block_index.device != ref.device:
        raise ValueError(f"block_index is on {block_index.device}, expected {ref.device}")
    if block_index.numel() != N:
        raise ValueError(f"block_index has {block_index.numel()} entries, expected N={N}")


def _view(t: torch.Tensor) -> View:
    """[B, N, H, D] tensor -> mhla_view (element strides; D must be contiguous)."""
    s = t.stride()   # (read once: four or five views per call add up on the host-bound decode step)
    if len(s) != 4:
        raise ValueError(f"expected a [B, N, H, D] tensor, got shape {tuple(t.shape)}")
    if s[3] != 1:
        raise ValueError("last dim must be contiguous")
    return View(t.data_ptr(), s[0], s[1], s[2])


def _strided_ok(t: torch.Tensor) -> bool:
    """Addressable in place by every kernel family: 16-byte aligned base and 16-byte row pieces (strides that are multiples of
    8 elements for 16-bit types, 4 for fp32) -- what the bf16 fast paths need, so a view never lands on a slower path or on a
    workspace-size mismatch because of its alignment."""
    s = t.stride()   # (read once, as in _view: a block-mix call prepares three to five tensors)
    mult = 8 if t.element_size() == 2 else 4
    return len(s) == 4 and s[3] == 1 and not (s[0] % mult or s[1] % mult or s[2] % mult) and t.data_ptr() % 16 == 0


def _prep(t: torch.Tensor) -> torch.Tensor:
    """Use the tensor in place when the kernels can address it, otherwise make it contiguous."""
    return t if _strided_ok(t) else t.contiguous()


def _alloc_like_tokens(B, N, H, D, ref):
    return torch.empty((B, N, H, D), dtype=ref.dtype, device=ref.device)


def _stream() -> int:
    # raw handle of the current device's current stream (torch.cuda.current_stream() builds a Stream object through several
    # Python layers: 20 us per call)
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(nbytes, 16) // 4 + 4, dtype=torch.float32, device=device)


# An optional tensor as the C ABI takes it: a null pointer / null view when it is absent.
def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def _view_or_null(t: Optional[torch.Tensor]) -> View:
    return _view(t) if t is not None else NULL_VIEW


def _f32(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """A norm weight / bias as the kernels read it: detached, fp32, contiguous."""
    return t.detach().to(torch.float32).contiguous() if t is not None else None


def _mix2d(mix: torch.Tensor, cols: Optional[int] = None) -> torch.Tensor:
    """A mixing matrix [L, L(, 1, ...)] or a block-mix W [M, M(, 1, 1)] as the kernels read it: detached, fp32, contiguous
    [rows, cols] (`cols`: what the caller will tell the library, so that a matrix of another width fails here)."""
    return mix.detach().reshape(mix.shape[0], mix.shape[1] if cols is None else cols).to(torch.float32).contiguous()


def _block_len(N: int, M: int) -> int:
    if N % M:
        raise ValueError(f"N={N} tokens not divisible into M={M} blocks")
    return N // M


def _rope_tables(cos: torch.Tensor, sin: torch.Tensor, N: int, D: int):
    if cos.shape != (N, D // 2) or sin.shape != (N, D // 2) or cos.dtype != torch.float32 or sin.dtype != torch.float32:
        raise ValueError(f"rope tables must be fp32 [N={N}, D/2={D // 2}]")
    return cos.contiguous(), sin.contiguous()


def _wants_grad(*ts) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


# Workspace sizes are pure functions of the problem: one ctypes round trip per distinct problem, not per call (the eager path of a
# small operator -- the DiT shape -- is bound by the host, tools/host_overhead.py).
@functools.lru_cache(maxsize=512)
def _bm_plan(B, H, M, S, D, dt, split, flags):
    lib = _lib.load()
    return (lib.mhla_blockmix_fwd_ws_bytes(B, H, M, S, D, dt, split, flags), lib.mhla_blockmix_bwd_ws_bytes(B, H, M, S, D, dt, split, flags),
            lib.mhla_blockmix_fwd_keeps_state(B, H, M, S, D, dt, split, flags) == 1)


@functools.lru_cache(maxsize=512)
def _cs_plan(B, T, H, K, V, chunk, dt, flags, n_chunks=None):
    """(forward, backward) workspace bytes of a causal call; `n_chunks`: the chunks of a pack (None: the uniform call)."""
    lib = _lib.load()
    if n_chunks is None:
        return (lib.mhla_causal_fwd_ws_bytes(B, T, H, K, V, chunk, dt, flags), lib.mhla_causal_bwd_ws_bytes(B, T, H, K, V, chunk, dt, flags))
    return (lib.mhla_causal_varlen_fwd_ws_bytes(B, T, H, K, V, chunk, n_chunks, dt, flags),
            lib.mhla_causal_varlen_bwd_ws_bytes(B, T, H, K, V, chunk, n_chunks, dt, flags))


# ------------------------------------------------------------------------------------------
# block-mixing MHLA (DiT / ViT / Wan)
# ------------------------------------------------------------------------------------------
def _check_handover(lib, ws, B, H, M, S, D, dt, split, flags):
    """MHLA_CHECK_HANDOVER=1: after every block-mix backward, synchronise and ask the library whether a dK/dV tile of the fused
    token-gradient launch gave up waiting for its dQ tile (`mhla_blockmix_bwd_status`); raises instead of returning an invalid
    dk.  Off by default: the check is a device synchronisation (not allowed while a HIP graph is being captured)."""
    if os.environ.get("MHLA_CHECK_HANDOVER") == "1":
        rc = lib.mhla_blockmix_bwd_status(ws.data_ptr(), ws.numel() * 4, B, H, M, S, D, dt, split, flags, _stream())
        _lib.check(rc, "mhla_blockmix_bwd_status")


SUMMARIES = ("tf32", "split", "bf16")


def _bm_flags(relu_eps: bool, force_generic: bool, no_smalln: bool, summaries: str) -> int:
    if summaries not in SUMMARIES:
        raise ValueError(f"summaries={summaries!r}: 'tf32' (default: 2-byte block summaries with 11 significand bits, the precision of the "
                         "reference's TF32 matmuls), 'split' (>= 16 significand bits: 24-bit / fp32 summaries) or 'bf16' (opt-in reduced precision)")
    return ((_lib.FLAG_RELU_EPS if relu_eps else 0) | (_lib.FLAG_FORCE_GENERIC if force_generic else 0)
            | (_lib.FLAG_NO_SMALLN if no_smalln else 0) | (_lib.FLAG_BF16_SUMMARIES if summaries == "bf16" else 0)
            | (_lib.FLAG_FP32_GRADE_SUMMARIES if summaries == "split" else 0))


def describe_dispatch(B: int, H: int, M: int, S: int, D: int, dtype, *, split: bool = False, summaries: str = "tf32", relu_eps: bool = False,
                      force_generic: bool = False, no_smalln: bool = False) -> dict:
    """Which kernel family, summary format and launches serve a block-mix problem (mhla_describe_dispatch; no GPU needed):
    {"family": ..., "summaries": ..., "fwd": [...], "bwd": [...]}.  dtype: a torch dtype."""
    return _describe("mhla_describe_dispatch", B, H, M, S, D, _DTYPES[dtype], int(split), _bm_flags(relu_eps, force_generic, no_smalln, summaries))


def describe_causal_dispatch(T: int, K: int, V: int, dtype, *, chunk_size: int = 64, summaries: str = "tf32", force_generic: bool = False) -> dict:
    """The same for the causal operator (mhla_causal_describe_dispatch)."""
    return _describe("mhla_causal_describe_dispatch", T, K, V, chunk_size, _DTYPES[dtype], _causal_flags(summaries, force_generic))


def _describe(fn: str, *problem) -> dict:
    import ctypes
    buf = ctypes.create_string_buffer(1024)
    rc = getattr(_lib.load(), fn)(*problem, buf, len(buf))
    if rc < 0:
        _lib.check(rc, fn)
    txt = buf.value.decode()
    d = dict(part.split("=", 1) for part in txt.split("; "))
    d["fwd"], d["bwd"] = d["fwd"].split(" "), d["bwd"].split(" ")
    d["text"] = txt
    return d


def set_option(name: str, value: int) -> int:
    """mhla_set_option through the package: the process-wide options change what the workspace-size queries return
    ("fp32_summaries"), so the cached plans are dropped with every change.  Returns the previous value."""
    rc = _lib.load().mhla_set_option(name.encode(), int(value))
    if rc < 0:
        _lib.check(rc, "mhla_set_option")
    _bm_plan.cache_clear()
    _cs_plan.cache_clear()
    return rc


def _den_views(normalize, q_den, k_den, qv, kv):
    """The pair the normaliser reads: q_den / k_den where they are given (Wan: the un-roped q, k), otherwise q / k themselves
    (`qv`, `kv`: their views); null views without normalisation."""
    if not normalize:
        return NULL_VIEW, NULL_VIEW
    if q_den is not None:
        return _view(q_den), _view(k_den)
    return qv, kv


def _blocks(N: int, W: torch.Tensor, checked: bool = False):
    """(M, S) of a call on N tokens with the mixing matrix W [M, M(, 1, 1)]: the blocks and the tokens of one.  `checked`: the node's
    public wrapper has already refused an N that M does not divide (no second check)."""
    M = W.shape[0]
    return M, (N // M if checked or not N % M else _block_len(N, M))


def _rope_args(cos: Optional[torch.Tensor], sin: Optional[torch.Tensor]):
    """Optional rope tables as the C ABI takes them: (cos, sin, row stride); null pointers and 0 without tables."""
    return (None, None, 0) if cos is None else (cos.data_ptr(), sin.data_ptr(), cos.stride(0))


def _bm_launch(fn, head, ws, kept, prob, eps, flags):
    """fn(*head, <tail>), checked; `fn`: one of the library's block-mix entry points.  They all end in this tail: the workspace and
    its bytes; in a backward the workspace its forward kept (`kept`: a 1-tuple of the pointer or None; () in a forward); `prob`, the
    problem (B, H, M, S, D, dtype code) as the size queries take it too; eps, flags, stream."""
    rc = fn(*head, ws.data_ptr(), ws.numel() * 4, *kept, *prob, eps, flags, _stream())
    if rc:
        _lib.check(rc, fn.__name__)


def _bm_fwd(lib, tok, den, normalize, Wf, out, index_ptr, prob, eps, flags):
    """mhla_blockmix_fwd on prepared tensors (`tok` = (q, k, v), `den` = (q_den, k_den) or (None, None); `index_ptr`: the pointer
    of block_index or None) into `out`.  Returns the workspace where the backward may read the forward's block summaries out of it
    (the library keeps them there and the workspace is within KEEP_STATE_LIMIT_BYTES), otherwise None: the backward recomputes them."""
    q, k, v = tok
    fwd_bytes, _, keeps = _bm_plan(*prob, 0 if den[0] is None else 1, flags)
    ws = _ws(fwd_bytes, q.device)
    qv, kv = _view(q), _view(k)
    _bm_launch(lib.mhla_blockmix_fwd, (qv, kv, _view(v), *_den_views(normalize, *den, qv, kv), Wf.data_ptr(), prob[2], _view(out),
                                       index_ptr), ws, (), prob, eps, flags)
    return ws if keeps and ws.numel() * 4 <= KEEP_STATE_LIMIT_BYTES else None


def _bm_bwd(lib, tok, den, normalize, Wf, out, dout, grads, dW, index_ptr, fwd_ws, prob, eps, flags):
    """mhla_blockmix_bwd on a node's saved tensors (`tok`, `den`, `index_ptr` as in `_bm_fwd`; `fwd_ws`: what `_bm_fwd` returned) into
    `grads` = (dq, dk, dv, dq_den, dk_den) -- any [B, N, H, D] views, the last two None without `den` -- and dW fp32 [M, M]."""
    q, k, v = tok
    dq, dk, dv, dqd, dkd = grads
    split = 0 if den[0] is None else 1
    ws = _ws(_bm_plan(*prob, split, flags)[1], q.device)
    qv, kv = _view(q), _view(k)
    _bm_launch(lib.mhla_blockmix_bwd, (qv, kv, _view(v), *_den_views(normalize, *den, qv, kv), Wf.data_ptr(), prob[2], _view(out),
                                       _view(dout), _view(dq), _view(dk), _view(dv), NULL_VIEW if dqd is None else _view(dqd),
                                       NULL_VIEW if dkd is None else _view(dkd), dW.data_ptr(), index_ptr),
               ws, (_ptr(fwd_ws),), prob, eps, flags)
    _check_handover(lib, ws, *prob, split, flags)


def _bm_grads(q, M, den=False):
    """What a block-mix backward writes: (dq, dk, dv, dq_den, dk_den) like q and contiguous (the last two None without `den`), and
    dW fp32 [M, M]."""
    dq, dk, dv = q.new_empty(q.shape), q.new_empty(q.shape), q.new_empty(q.shape)
    dW = torch.empty((M, M), dtype=torch.float32, device=q.device)
    return (dq, dk, dv, torch.empty_like(dq) if den else None, torch.empty_like(dq) if den else None), dW


def _w_grad(dW, w_shape, w_dtype):
    """The library's fp32 [M, M] gradient as the gradient of the caller's W (its shape, its dtype)."""
    return dW.reshape(w_shape).to(w_dtype)


class _BlockMix(torch.autograd.Function):
    @staticmethod
    @_device_guard
    def forward(ctx, q, k, v, W, q_den, k_den, block_index, eps, normalize, flags):
        lib = _lib.load()
        _require_gpu(q, k, v, W, q_den, k_den, block_index)
        B, N, H, D = q.shape
        M, S = _blocks(N, W)
        split = q_den is not None
        if split and not normalize:
            raise ValueError("q_den/k_den given but normalize=False")
        _check_like(q, "mhla_blockmix", k=(k, q.shape), v=(v, q.shape), q_den=(q_den, q.shape), k_den=(k_den, q.shape))
        _check_block_index(block_index, N, q)
        if W.device != q.device or W.dim() < 2 or W.shape[1] != M:
            raise ValueError(f"W must be a [M, M] (or [M, M, 1, 1]) matrix on {q.device}, got {tuple(W.shape)} on {W.device}")
        q, k, v = _prep(q), _prep(k), _prep(v)
        if split:
            q_den, k_den = _prep(q_den), _prep(k_den)
        Wf = _mix2d(W, M)
        out = q.new_empty((B, N, H, D))
        prob, eps = (B, H, M, S, D, _dtype_code(q)), float(eps)
        fwd_ws = _bm_fwd(lib, (q, k, v), (q_den, k_den), normalize, Wf, out, _ptr(block_index), prob, eps, flags)
        ctx.save_for_backward(q, k, v, Wf, out, q_den, k_den, block_index, fwd_ws)
        ctx.cfg = (prob, eps, bool(normalize), W.shape, W.dtype, flags)
        return out

    @staticmethod
    @_device_guard
    def backward(ctx, dout):
        lib = _lib.load()
        q, k, v, Wf, out, q_den, k_den, block_index, fwd_ws = ctx.saved_tensors
        prob, eps, normalize, w_shape, w_dtype, flags = ctx.cfg
        if dout.dtype != q.dtype:
            dout = dout.to(q.dtype)
        _check_like(q, "mhla_blockmix backward", dout=(dout, q.shape))
        dout = _prep(dout)
        grads, dW = _bm_grads(q, prob[2], q_den is not None)
        _bm_bwd(lib, (q, k, v), (q_den, k_den), normalize, Wf, out, dout, grads, dW, _ptr(block_index), fwd_ws, prob, eps, flags)
        dq, dk, dv, dqd, dkd = grads
        return dq, dk, dv, _w_grad(dW, w_shape, w_dtype), dqd, dkd, None, None, None, None


def mhla_blockmix(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, W: torch.Tensor, *, eps: float = 1e-6,
                  q_den: Optional[torch.Tensor] = None, k_den: Optional[torch.Tensor] = None,
                  normalize: bool = True, block_index: Optional[torch.Tensor] = None,
                  relu_eps: bool = False, force_generic: bool = False, no_smalln: bool = False,
                  summaries: str = "tf32") -> torch.Tensor:
    """Block-mixing MHLA operator (mhla_dit/mhla/mhla.py:262-268; wan/mhla_utils.py:331-341).

    q, k, v : [B, N, H, D] token-major (any batch/token/head strides, e.g. views into a fused QKV
              projection), tokens in block-major order -- or in any order with `block_index`
              (int32[N]: block-major position -> token row).
    W       : [M, M] (or the conv weight [M, M, 1, 1]); W[i, j] mixes block j's KV summary into block i.
    q_den, k_den : optional separate pair for the normaliser (Wan: un-roped q, k).
    normalize    : False skips the division (Wan `normalize_out=False`).
    relu_eps     : apply relu(x)+eps to q and k inside the kernels (mhla.py:229-230) -- q, k are then
                   the raw projections and receive the masked gradient.
    force_generic / no_smalln: testing aids -- take the generic fp32-MFMA kernels / skip the single-launch
                   small-sequence path where they would otherwise be chosen.
    summaries    : how 16-bit problems keep what feeds a SECOND contraction (the block summaries KV, G, dG, dKV, dP = dO / n,
                   the score tiles of the 256-token path).  Operands are bf16 hi + lo pairs with fp32 accumulation in every case but
                   "bf16".  "tf32" (default): the summaries are STORED with 11 significand bits (fp16 payload x one power-of-two
                   multiplier per block row, 2 bytes) -- the precision the reference's own matmul / 1x1 conv run at under
                   allow_tf32 (mhla_dit/train.py:12-13) -- where the kernels have the format (blocks of >= 16 tokens, D <= 96,
                   M <= 128), >= 16 bits elsewhere; results within one final rounding + 1e-3 of the fp32 result (observed 4e-4).
                   "split": >= 16 significand bits everywhere (24-bit / fp32 summaries; 1e-5).  "bf16" (bf16 tensors only):
                   single bf16 values -- REDUCED PRECISION (2-3e-3 of a gradient's maximum).
    Returns [B, N, H, D] contiguous, same dtype; differentiable w.r.t. q, k, v, W (and q_den, k_den).
    """
    if (q_den is None) != (k_den is None):
        raise ValueError("q_den and k_den must be given together")
    if q.dim() != 4:
        raise ValueError(f"q: expected [B, N, H, D], got {tuple(q.shape)}")
    _check_block_index(block_index, q.shape[1], q)
    if q.shape[-1] > 128:
        return _blockmix_wide_head(q, k, v, W, eps, q_den, k_den, normalize, block_index, relu_eps, force_generic, no_smalln, summaries)
    flags = _bm_flags(relu_eps, force_generic, no_smalln, summaries)
    if not _wants_grad(q, k, v, W, q_den, k_den):
        flags |= _lib.FLAG_NO_BWD_STATE   # inference: the forward skips what only a backward would read
    if q.shape[0] == 0:   # empty batch: nothing to launch; keep the autograd graph connected (all gradients are zero)
        return torch.zeros_like(v) + 0 * (q.sum() + k.sum() + W.sum()).to(v.dtype)
    nb = _MAX_GRID_BH // q.shape[2]
    if q.shape[0] > nb:
        # more (batch, head) pairs than one launch addresses (the kernels index them with grid.y <= 65535; the C ABI returns
        # MHLA_ENOTSUP): batch slices through the same autograd node, the gradient of W accumulates over the slices
        sl = lambda t, i: None if t is None else t[i:i + nb]
        return torch.cat([_BlockMix.apply(sl(q, i), sl(k, i), sl(v, i), W, sl(q_den, i), sl(k_den, i), block_index, eps, normalize,
                                          flags) for i in range(0, q.shape[0], nb)], dim=0)
    if _native_nodes():
        return torch.ops.mhla_amd.blockmix(q, k, v, W, q_den, k_den, block_index, float(eps), bool(normalize), flags, KEEP_STATE_LIMIT_BYTES)
    return _BlockMix.apply(q, k, v, W, q_den, k_den, block_index, eps, normalize, flags)


def _wide_head_chunk(D: int) -> int:
    """Slice width for a head dim above 128: the largest divisor of D in [32, 128] that is a multiple of 8 (the kernels' head dims);
    without one (D = 132, 136, 152, 184, ...) the width in [64, 128] that needs the fewest slices and then the least zero padding."""
    for c in range(128, 31, -8):
        if D % c == 0:
            return c
    return min(range(64, 129, 8), key=lambda c: (-(-D // c), -(-D // c) * c - D))


def _blockmix_wide_head(q, k, v, W, eps, q_den, k_den, normalize, block_index, relu_eps, force_generic, no_smalln, summaries):
    """Head dims above 128 (the reference module takes any dim_head, mhla_dit/mhla/mhla.py:155-158; the kernels stop at 128, where a
    block summary is 64 KB): the D x D summary is a (D / c)^2 grid of c x c blocks, and the operator is linear in them --
        O[:, b] = sum_a Q[:, a] G[a, b],   G[a, b] = W (K[:, a]^T V[:, b])
    -- so the numerator is (D / c)^2 un-normalised calls of the operator on c-wide slices, and the normaliser, which couples all D
    features of a token (n_i[s] = sum_j W_ij q_j[s] . ksum_j + eps), a few [B, M, S, H] tensor ops.  Everything stays differentiable
    (the slices' autograd nodes and eager PyTorch); no BASELINE shape comes here."""
    B, N, H, D = q.shape
    out_dtype = v.dtype
    if relu_eps and q_den is not None:
        raise ValueError("relu_eps needs q_den / k_den to alias q / k (as for head dims up to 128: MHLA_FLAG_RELU_EPS)")
    c = _wide_head_chunk(D)
    Wm = W.reshape(W.shape[0], W.shape[1]) if W.dim() == 4 else W
    M = Wm.shape[0]
    S = _block_len(N, M)
    # (16-bit tensors: everything below runs on ONE fp32 copy of each tensor -- the partial products O_ab and the gradient pieces of the
    # slices would otherwise each carry their own 16-bit rounding into their sums -- and results / gradients are rounded once)
    q, k, v = q.float(), k.float(), v.float()
    if q_den is not None:
        q_den, k_den = q_den.float(), k_den.float()
    if relu_eps:   # (in PyTorch, before any padding: a padded column must stay 0, not become eps)
        q, k = torch.relu(q) + eps, torch.relu(k) + eps
    nc = -(-D // c)
    pad = nc * c - D   # zero columns add nothing to either product (no divisor of D among the kernels' head dims)
    qp, kp, vp = (torch.nn.functional.pad(t, (0, pad)) if pad else t for t in (q, k, v))
    qs, ks_, vs = ([t[..., a * c:(a + 1) * c].contiguous() for a in range(nc)] for t in (qp, kp, vp))   # sliced once
    kw = dict(eps=eps, normalize=False, block_index=block_index, relu_eps=False, force_generic=force_generic, no_smalln=no_smalln,
              summaries=summaries)
    cols = []
    for b in range(nc):
        acc = None
        for a in range(nc):
            o = mhla_blockmix(qs[a], ks_[a], vs[b], W, **kw)
            acc = o if acc is None else acc + o
        cols.append(acc)
    out = torch.cat(cols, dim=-1)[..., :D]
    if normalize:
        qd, kd = (q, k) if q_den is None else (q_den, k_den)
        if block_index is not None:   # block-major position p lives at row block_index[p]
            rows = block_index.long()
            qd, kd = qd[:, rows], kd[:, rows]
        ksum = kd.reshape(B, M, S, H, D).sum(2)                                  # [B, M, H, D]
        z = (qd.reshape(B, M, S, H, D) * ksum[:, :, None]).sum(-1)               # [B, M, S, H]
        n = torch.einsum("ij,bjsh->bish", Wm.float(), z) + eps                   # the quirk normaliser: same offset s in every block j
        n = n.reshape(B, N, H)
        if block_index is not None:   # back to the tensors' row order
            n = torch.zeros_like(n).index_copy(1, block_index.long(), n)
        out = out / n[..., None]
    return out.to(out_dtype)


class _BlockMixRope(torch.autograd.Function):
    """mhla_blockmix_rope_fwd / mhla_blockmix_rope_bwd: the operator with the rotation of q, k inside its kernels, both ways."""

    @staticmethod
    @_device_guard
    def forward(ctx, q, k, v, W, cos, sin, eps, normalize, block_index):
        lib = _lib.load()
        B, N, H, D = q.shape
        M, S = _blocks(N, W, checked=True)
        q, k, v = _prep(q.detach()), _prep(k.detach()), _prep(v.detach())
        Wf = _mix2d(W, M)
        out = q.new_empty((B, N, H, D))
        prob, eps, normalize = (B, H, M, S, D, _dtype_code(q)), float(eps), int(bool(normalize))
        ws = _ws(_bm_plan(*prob, 0, 0)[0], q.device)
        _bm_launch(lib.mhla_blockmix_rope_fwd, (_view(q), _view(k), _view(v), normalize, Wf.data_ptr(), M, *_rope_args(cos, sin),
                                                   _view(out), _ptr(block_index)), ws, (), prob, eps, 0)
        keep = any(ctx.needs_input_grad[:4]) and ws.numel() * 4 <= KEEP_STATE_LIMIT_BYTES   # KV, G, z, ksum, 1/n for the backward
        ctx.save_for_backward(q, k, v, Wf, out, cos, sin, block_index, ws if keep else None)
        ctx.cfg = (prob, eps, normalize, W.shape, W.dtype)
        return out

    @staticmethod
    @_device_guard
    def backward(ctx, dout):
        lib = _lib.load()
        q, k, v, Wf, out, cos, sin, block_index, fwd_ws = ctx.saved_tensors
        prob, eps, normalize, w_shape, w_dtype = ctx.cfg
        M = prob[2]
        dout = _prep(dout.to(q.dtype))
        (dq, dk, dv, _, _), dW = _bm_grads(q, M)
        ws = _ws(_bm_plan(*prob, 0, 0)[1], q.device)
        _bm_launch(lib.mhla_blockmix_rope_bwd, (_view(q), _view(k), _view(v), normalize, Wf.data_ptr(), M, *_rope_args(cos, sin),
                                                   _view(out), _view(dout), _view(dq), _view(dk), _view(dv), dW.data_ptr(),
                                                   _ptr(block_index)), ws, (_ptr(fwd_ws),), prob, eps, 0)
        return dq, dk, dv, _w_grad(dW, w_shape, w_dtype), None, None, None, None, None


def mhla_blockmix_rope(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, W: torch.Tensor, rope_cos: torch.Tensor,
                       rope_sin: torch.Tensor, *, eps: float = 1e-6, normalize: bool = True,
                       block_index: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Block-mixing operator with Wan's rotary prologue fused in (wan/mhla_utils.py:314 + :317-341), forward and backward.

    q, k are the un-rotated tensors ([B, N, H, D]); rope_cos / rope_sin are fp32 [N, D/2] (the multiplier of `rope_apply`
    per token row).  Rotated k feeds KV, rotated q the numerator, plain q / k the normaliser -- no q_rope / k_rope
    tensors are materialised, in either direction: the backward rotates q and k again where the rotated ones are needed and
    returns the gradients w.r.t. the un-rotated tensors (fp32 tensors, D % 8 == 0 for the backward).

    The forward serves fp32 tensors.  16-bit tensors are served only where their block summaries are fp32 words: head dims above
    96; head dims up to 96 where the format falls back to fp32 words (more than 128 blocks of fewer than 16 tokens or at head dims under
    32, more than 256 blocks, D * D no multiple of 64); the "fp32_summaries" process option.  The rotated q and k are fp32 values there and enter the
    products as bf16 hi + lo pairs whatever the tensor type: one final rounding + 1e-3, like the default arithmetic of
    mhla_blockmix.  On the h16 / p24 summaries that are the 16-bit default elsewhere the library refuses the call (no rotary summary
    kernel is built for them) and this raises: use fp32 tensors, or rotate on the host and call
    mhla_blockmix(q_rope, k_rope, v, W, q_den=q, k_den=k)."""
    _require_gpu(q, k, v, W, rope_cos, rope_sin, block_index)
    _, N, _, D = q.shape
    _blocks(N, W)   # (the one divisibility check of this call: the node does not repeat it)
    _check_like(q, "mhla_blockmix_rope", k=(k, q.shape), v=(v, q.shape))
    _check_block_index(block_index, N, q)
    cos, sin = _rope_tables(rope_cos, rope_sin, N, D)
    if _wants_grad(q, k, v, W) and (q.dtype != torch.float32 or D % 8):
        raise RuntimeError("the backward of mhla_blockmix_rope needs fp32 tensors with D % 8 == 0; rotate in the host and call "
                           "mhla_blockmix(q_rope, k_rope, v, W, q_den=q, k_den=k) otherwise")
    return _BlockMixRope.apply(q, k, v, W, cos, sin, eps, normalize, block_index)


# ------------------------------------------------------------------------------------------
# LePE: depthwise conv over V on the block-major token layout (DiT / ViT)
# ------------------------------------------------------------------------------------------
def _tok3(t: torch.Tensor) -> torch.Tensor:
    """[B, N, C] view with contiguous channels (copy only if the channels are strided)."""
    return t if t.stride(-1) == 1 else t.contiguous()


def _lepe_taps(weight, bias, C, taps):
    """A depthwise conv's weight [C, 1, k, k(, k)] as fp32 [taps, C], the layout the kernels read, and its bias in fp32 (or None)."""
    return weight.detach().reshape(C, taps).t().to(torch.float32).contiguous(), _f32(bias)


def _lepe_conv(dims, x, w_taps, bias, add, y, geom, transposed):
    """mhla_lepe2d / mhla_lepe3d (`dims`): y = conv(x) (+ bias) (+ add), or with `transposed` the flipped-kernel correlation that is
    the gradient w.r.t. the conv's input.  x, add, y: [B, N, C] with contiguous channels (or contiguous [B, N, H, D]: the same batch
    and token strides); `geom`: the library's geometry arguments, (pieces_len, block_len, C, K) in 2-D and (F, H, W, C) in 3-D."""
    lib = _lib.load()
    fn = lib.mhla_lepe3d if dims == 3 else lib.mhla_lepe2d
    rc = fn(x.data_ptr(), x.stride(0), x.stride(1), w_taps.data_ptr(), _ptr(bias), _ptr(add),
            add.stride(0) if add is not None else 0, add.stride(1) if add is not None else 0,
            y.data_ptr(), y.stride(0), y.stride(1), x.shape[0], *geom, int(transposed), _dtype_code(x), _stream())
    if rc:
        _lib.check(rc, f"mhla_lepe{dims}d (input gradient)" if transposed else f"mhla_lepe{dims}d")


def _lepe_wgrad(dims, v, dy, geom, w_shape, w_dtype, b_dtype):
    """mhla_lepe2d_wgrad / mhla_lepe3d_wgrad: the gradients of the conv's weight and bias in the parameters' shapes and dtypes
    (`b_dtype` None: no bias, no gradient).  v, dy: [B, N, C] with contiguous channels."""
    lib = _lib.load()
    C = v.shape[2]
    taps = w_shape.numel() // C
    dwb = torch.empty((taps + 1, C), dtype=torch.float32, device=v.device)   # one row per tap, then the bias row
    if dims == 3:
        fn, nbytes = lib.mhla_lepe3d_wgrad, lib.mhla_lepe3d_wgrad_ws_bytes(C)
    else:
        fn, nbytes = lib.mhla_lepe2d_wgrad, lib.mhla_lepe2d_wgrad_ws_bytes(C, geom[3])
    ws = _ws(nbytes, v.device)
    rc = fn(v.data_ptr(), v.stride(0), v.stride(1), dy.data_ptr(), dy.stride(0), dy.stride(1), dwb.data_ptr(),
            ws.data_ptr(), ws.numel() * 4, v.shape[0], *geom, _dtype_code(v), _stream())
    if rc:
        _lib.check(rc, f"mhla_lepe{dims}d_wgrad")
    return dwb[:taps].t().reshape(w_shape).to(w_dtype), (dwb[taps].to(b_dtype) if b_dtype is not None else None)


class _Lepe(torch.autograd.Function):
    """`lepe2d` (dims = 2) and `lepe3d` (dims = 3): the same node over the two kernel sets; `geom` as in `_lepe_conv`."""

    @staticmethod
    @_device_guard
    def forward(ctx, v, weight, bias, add, dims, geom):
        _require_gpu(v, weight, bias, add)
        B, N, C = v.shape
        v = _tok3(v)
        w_taps, b32 = _lepe_taps(weight, bias, C, 27 if dims == 3 else geom[3] ** 2)
        y = torch.empty((B, N, C), dtype=v.dtype, device=v.device)
        _lepe_conv(dims, v, w_taps, b32, _tok3(add) if add is not None else None, y, geom, False)
        ctx.save_for_backward(v, w_taps)
        ctx.cfg = (dims, geom, weight.shape, weight.dtype, bias.dtype if bias is not None else None, add is not None)
        return y

    @staticmethod
    @_device_guard
    def backward(ctx, dy):
        v, w_taps = ctx.saved_tensors
        dims, geom, w_shape, w_dtype, b_dtype, has_add = ctx.cfg
        dy = _tok3(dy.to(v.dtype))
        dv = dw = db = None
        if ctx.needs_input_grad[0]:
            dv = torch.empty(v.shape, dtype=v.dtype, device=v.device)
            _lepe_conv(dims, dy, w_taps, None, None, dv, geom, True)
        if ctx.needs_input_grad[1] or (b_dtype is not None and ctx.needs_input_grad[2]):
            dw, db = _lepe_wgrad(dims, v, dy, geom, w_shape, w_dtype, b_dtype)
        return dv, dw, db, (dy if has_add else None), None, None


def lepe2d(v: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], pieces_len: int, block_len: int,
           add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Depthwise conv of the DiT / ViT hosts' LePE branch on the operator's own token layout:
    `conv2d(v as image, weight [C,1,K,K], bias, padding=K//2, groups=C)` (+ `add`), with v, add, result [B, N, C] in
    block-major token order (N = pieces_len^2 * block_len^2).  Replaces the rearranges + nn.Conv2d at
    mhla_dit/mhla/mhla.py:246-247 and the add at :271-273.  Differentiable w.r.t. v, weight, bias, add."""
    if v.dim() != 3 or weight.dim() != 4 or weight.shape[1] != 1 or weight.shape[2] != weight.shape[3]:
        raise ValueError("v: [B, N, C]; weight: [C, 1, K, K]")
    if v.shape[1] != (pieces_len * block_len) ** 2 or weight.shape[0] != v.shape[2]:
        raise ValueError(f"N={v.shape[1]} != (pieces_len*block_len)^2 or channel mismatch")
    return _Lepe.apply(v, weight, bias, add, 2, (int(pieces_len), int(block_len), v.shape[2], weight.shape[-1]))


def lepe3d(v: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], grid, add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Depthwise 3 x 3 x 3 conv of the Wan host's LePE branch on its own token layout:
    `conv3d(v as video, weight [C,1,3,3,3], bias, padding=1, groups=C)` (+ `add`), with v, add, result [B, N, C] in raster
    token order n = (f*H + h)*W + w, grid = (F, H, W).  Replaces the rearranges + nn.Conv3d at wan/mhla_utils.py:199-201,
    349-352 and the add at :363-364.  Differentiable w.r.t. v, weight, bias, add."""
    F_, H_, W_ = (int(g) for g in grid)
    if v.dim() != 3 or weight.dim() != 5 or tuple(weight.shape[1:]) != (1, 3, 3, 3):
        raise ValueError("v: [B, N, C]; weight: [C, 1, 3, 3, 3]")
    if v.shape[1] != F_ * H_ * W_ or weight.shape[0] != v.shape[2]:
        raise ValueError(f"N={v.shape[1]} != F*H*W={F_ * H_ * W_} or channel mismatch")
    return _Lepe.apply(v, weight, bias, add, 3, (F_, H_, W_, v.shape[2]))


def _wan_tokens(fn, q, k, v, W, weights, rope_cos, rope_sin, norm_weight, gate, block_index, fp32_only=False):
    """The front mhla_blockmix_wan and mhla_blockmix_wan_pro share, first half (`fn`: the caller's name, for the messages; `weights`:
    its further differentiable tensors): the forward-only guard, the GPU requirement, the shapes, the agreement checks.  Returns q, k,
    v detached and as the kernels address them, the problem (B, H, M, S, D, dtype code) and N."""
    if _wants_grad(q, k, v, W, *weights, norm_weight, gate):
        raise RuntimeError(f"{fn} is forward-only")
    _require_gpu(q, k, v, W, *weights, rope_cos, rope_sin, norm_weight, gate, block_index)
    if fp32_only and q.dtype != torch.float32:
        raise TypeError(f"{fn} takes fp32 q, k, v (the host's .float())")
    B, N, H, D = q.shape
    M, S = _blocks(N, W)
    _check_like(q, fn, k=(k, q.shape), v=(v, q.shape))
    _check_block_index(block_index, N, q)
    q, k, v = _prep(q.detach()), _prep(k.detach()), _prep(v.detach())
    return q, k, v, (B, H, M, S, D, _dtype_code(q)), N


def _wan_operands(q, prob, N, W, rope_cos, rope_sin, norm_weight, gate, out_dtype, gate_in):
    """Second half of that front, in the order the storage is allocated: the optional rope tables, the gate (in `out_dtype`, which
    the message calls `gate_in`), the norm weight (one that `_f32` has made already passes through as it is), W, the output and the
    workspace, which both calls size by the fp32 plan.  Returns (cos, sin, gate, norm weight, Wf, out, ws)."""
    B, H, M, S, D, _ = prob
    cos = sin = None
    if rope_cos is not None:
        cos, sin = _rope_tables(rope_cos, rope_sin, N, D)
    if gate is not None:
        if gate.shape != (B, N, H, D) or gate.dtype != out_dtype:
            raise ValueError(f"gate: [B, N, H, D] in {gate_in}")
        gate = _prep(gate.detach())
    nw = _f32(norm_weight)
    Wf = _mix2d(W, M)
    out = torch.empty((B, N, H, D), dtype=out_dtype, device=q.device)
    return cos, sin, gate, nw, Wf, out, _ws(_bm_plan(B, H, M, S, D, _lib.F32, 0, 0)[0], q.device)


@_device_guard
def mhla_blockmix_wan(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, W: torch.Tensor, rope_cos: Optional[torch.Tensor],
                      rope_sin: Optional[torch.Tensor], norm_weight: Optional[torch.Tensor], norm_eps: float,
                      gate: Optional[torch.Tensor], out_dtype: torch.dtype, *, eps: float = 1e-6, normalize: bool = True,
                      block_index: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The Wan layer's operator with prologue and epilogue fused (inference): rotary prologue as `mhla_blockmix_rope`
    (tables optional) and the per-head RMSNorm (x SiLU gate) of wan/mhla_utils.py:356-362 applied before the store.
    q, k, v: fp32 [B, N, H, D]; gate: [B, N, H, D] in `out_dtype` or None; returns [B, N, H, D] in `out_dtype`."""
    lib = _lib.load()
    q, k, v, prob, N = _wan_tokens("mhla_blockmix_wan", q, k, v, W, (), rope_cos, rope_sin, norm_weight, gate, block_index, fp32_only=True)
    cos, sin, gate, nw, Wf, out, ws = _wan_operands(q, prob, N, W, rope_cos, rope_sin, norm_weight, gate, out_dtype, "out_dtype")
    _bm_launch(lib.mhla_blockmix_wan_fwd, (_view(q), _view(k), _view(v), int(bool(normalize)), Wf.data_ptr(), prob[2], *_rope_args(cos, sin),
                                              _ptr(nw), float(norm_eps), _view_or_null(gate), _view(out), _DTYPES[out_dtype], _ptr(block_index)),
               ws, (), prob, float(eps), 0)
    return out


def wan_pro_supported(q: torch.Tensor, M: int) -> bool:
    """True when `mhla_blockmix_wan_pro` serves q [B, N, H, D] with M blocks (16-bit tensors, 96 < D <= 128, at most 192 blocks)."""
    if q.dim() != 4 or q.dtype not in (torch.bfloat16, torch.float16) or not q.is_cuda or q.shape[1] % M:
        return False
    return _lib.load().mhla_blockmix_wan_pro_ok(M, q.shape[1] // M, q.shape[3], _dtype_code(q), 0) == 1


def mhla_blockmix_wan_pro(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, wq: Optional[torch.Tensor], wk: Optional[torch.Tensor],
                          qk_norm_eps: float, W: torch.Tensor, rope_cos: Optional[torch.Tensor], rope_sin: Optional[torch.Tensor],
                          norm_weight: Optional[torch.Tensor], norm_eps: float, gate: Optional[torch.Tensor], *, eps: float = 1e-6,
                          normalize: bool = True, block_index: Optional[torch.Tensor] = None, qk_norm: bool = True) -> torch.Tensor:
    """The Wan layer's inference operator with the q / k prologue folded into its loads (mhla_blockmix_wan_pro_fwd): q, k, v are the
    16-bit projection outputs [B, N, H, D] (views of [B, N, C] are fine), wq / wk the full-dim RMSNorm weights [H * D] (None: no affine),
    `qk_norm=False`: no norm at all (relu(x) + eps).  One small kernel per tensor computes the per-token rstd; the operator's kernels
    apply relu(x * rstd * w) + eps, the rotation, and the per-head norm x gate epilogue.  Same numbers as
    `mhla_blockmix_wan(qk_prologue(q), qk_prologue(k), v.float(), ...)` without the three fp32 tensors.  Forward only; returns
    [B, N, H, D] in the dtype of q."""
    lib = _lib.load()
    q, k, v, prob, N = _wan_tokens("mhla_blockmix_wan_pro", q, k, v, W, (wq, wk), rope_cos, rope_sin, norm_weight, gate, block_index)
    B, H, _, _, D, dt = prob
    wq, wk, nw = _f32(wq), _f32(wk), _f32(norm_weight)
    rq = rk = None
    if qk_norm:
        if not (q.stride(2) == D and k.stride(2) == D):
            raise ValueError("q, k: the heads of a token must be contiguous (views of the [B, N, H * D] projection)")
        rq = torch.empty(B * N, dtype=torch.float32, device=q.device)
        rk = torch.empty(B * N, dtype=torch.float32, device=q.device)
        for x, r in ((q, rq), (k, rk)):
            if x.stride(0) != N * x.stride(1):
                raise ValueError("q, k: batch stride must be N * token stride")
            _lib.check(lib.mhla_rms_rstd(x.data_ptr(), x.stride(1), r.data_ptr(), B * N, H * D, float(qk_norm_eps), dt, _stream()), "mhla_rms_rstd")
    cos, sin, gate, nw, Wf, out, ws = _wan_operands(q, prob, N, W, rope_cos, rope_sin, nw, gate, q.dtype, "the dtype of q")
    _bm_launch(lib.mhla_blockmix_wan_pro_fwd, (_view(q), _view(k), _view(v), _ptr(rq), _ptr(rk), _ptr(wq), _ptr(wk), int(bool(normalize)),
                                                  Wf.data_ptr(), prob[2], *_rope_args(cos, sin), _ptr(nw), float(norm_eps), _view_or_null(gate),
                                                  _view(out), dt, _ptr(block_index)), ws, (), prob, float(eps), 0)
    return out


class _DitCore(torch.autograd.Function):
    """Operator + LePE of the DiT / ViT module as ONE autograd node on the packed QKV projection output
    (mhla_dit/mhla/mhla.py:245-273): q, k, v are the three slices of `qkv` [B, N, 3, H, D] read in place; the backward writes
    dq, dk and dv (operator part + LePE part, summed inside the LePE kernel) straight into one [B, N, 3, H, D] gradient --
    no per-slice gradient tensors, no zero-fill and slice-adds by autograd."""

    @staticmethod
    @_device_guard
    def forward(ctx, qkv, W, lepe_w, lepe_b, pieces_len, block_len, eps, flags):
        lib = _lib.load()
        _require_gpu(qkv, W, lepe_w, lepe_b)
        B, N, _, H, D = qkv.shape
        (M, S), C, K = _blocks(N, W, checked=True), H * D, lepe_w.shape[-1]
        qkv = qkv if (qkv.is_contiguous() and _strided_ok(qkv[:, :, 0])) else qkv.contiguous()
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        Wf = _mix2d(W, M)
        prob, eps = (B, H, M, S, D, _dtype_code(qkv)), float(eps)
        attn = qkv.new_empty((B, N, H, D))
        fwd_ws = _bm_fwd(lib, (q, k, v), (None, None), True, Wf, attn, None, prob, eps, flags)
        w_taps, b32 = _lepe_taps(lepe_w, lepe_b, C, K * K)
        y = torch.empty((B, N, C), dtype=qkv.dtype, device=qkv.device)
        v3 = v.reshape(B, N, C)          # view: H and D are adjacent in the packed buffer
        _lepe_conv(2, v3, w_taps, b32, attn, y, (pieces_len, block_len, C, K), False)
        ctx.save_for_backward(qkv, Wf, attn, w_taps, fwd_ws)
        ctx.cfg = (prob, (pieces_len, block_len, C, K), eps, flags, W.shape, W.dtype, lepe_w.shape, lepe_w.dtype,
                   lepe_b.dtype if lepe_b is not None else None)
        return y

    @staticmethod
    @_device_guard
    def backward(ctx, dy):
        lib = _lib.load()
        qkv, Wf, attn, w_taps, fwd_ws = ctx.saved_tensors
        prob, geom, eps, flags, w_shape, w_dtype, lw_shape, lw_dtype, lb_dtype = ctx.cfg
        B, N, _, H, D = qkv.shape
        M, C = prob[2], geom[2]
        dy = dy.to(qkv.dtype).contiguous()
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        dqkv = torch.empty_like(qkv)
        dv_attn = qkv.new_empty((B, N, H, D))
        dW = torch.empty((M, M), dtype=torch.float32, device=qkv.device)
        _bm_bwd(lib, (q, k, v), (None, None), True, Wf, attn, dy.reshape(B, N, H, D), (dqkv[:, :, 0], dqkv[:, :, 1], dv_attn, None, None),
                dW, None, fwd_ws, prob, eps, flags)
        # dv = operator part + LePE part (flipped-kernel correlation of dy), written into the V slice of the packed gradient
        _lepe_conv(2, dy, w_taps, None, dv_attn, dqkv[:, :, 2].reshape(B, N, C), geom, True)
        dlw, dlb = _lepe_wgrad(2, v.reshape(B, N, C), dy, geom, lw_shape, lw_dtype, lb_dtype)
        return dqkv, _w_grad(dW, w_shape, w_dtype), dlw, dlb, None, None, None, None


def mhla_dit_core(qkv: torch.Tensor, W: torch.Tensor, lepe_weight: torch.Tensor, lepe_bias: Optional[torch.Tensor],
                  pieces_len: int, block_len: int, *, eps: float = 1e-6, relu_eps: bool = True, summaries: str = "tf32") -> torch.Tensor:
    """`mhla_blockmix(q, k, v, W) + LePE(v)` of the DiT / ViT module on the packed projection output `qkv` [B, N, 3, H, D]
    (block-major tokens), returning [B, N, H*D]; one autograd node whose backward emits a single packed gradient.
    `summaries`: see mhla_blockmix."""
    if qkv.dim() != 5 or qkv.shape[2] != 3:
        raise ValueError("qkv: [B, N, 3, H, D]")
    if qkv.shape[1] % W.shape[0] or qkv.shape[1] != (pieces_len * block_len) ** 2:
        raise ValueError("token count does not match the block layout")
    flags = _bm_flags(relu_eps, False, False, summaries)
    if not _wants_grad(qkv, W, lepe_weight, lepe_bias):
        flags |= _lib.FLAG_NO_BWD_STATE
    return _DitCore.apply(qkv, W, lepe_weight, lepe_bias, int(pieces_len), int(block_len), eps, flags)


_FMAPS = {None: 0, "identity": 0, "relu": 1, "elu": 2}


class _FmapRotary(torch.autograd.Function):
    @staticmethod
    @_device_guard
    def forward(ctx, x, cos, sin, fmap, t_offset):
        lib = _lib.load()
        _require_gpu(x, cos, sin)
        B, T, H, K = x.shape
        x = _prep(x)
        y = _alloc_like_tokens(B, T, H, K, x)
        rc = lib.mhla_featmap_rotary(_view(x), NULL_VIEW, *_rope_args(cos, sin), t_offset, _view(y),
                                     B, T, H, K, fmap, 0, _dtype_code(x), _stream())
        _lib.check(rc, "mhla_featmap_rotary")
        ctx.save_for_backward(x, cos, sin)
        ctx.cfg = (fmap, t_offset)
        return y

    @staticmethod
    @_device_guard
    def backward(ctx, dy):
        lib = _lib.load()
        x, cos, sin = ctx.saved_tensors
        fmap, t_offset = ctx.cfg
        B, T, H, K = x.shape
        dy = _prep(dy.to(x.dtype))
        dx = _alloc_like_tokens(B, T, H, K, x)
        rc = lib.mhla_featmap_rotary(_view(dy), _view(x), *_rope_args(cos, sin), t_offset, _view(dx),
                                     B, T, H, K, fmap, 1, _dtype_code(x), _stream())
        _lib.check(rc, "mhla_featmap_rotary (backward)")
        return dx, None, None, None, None


def featmap_rotary(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, feature_map: Optional[str] = None,
                   t_offset: int = 0) -> torch.Tensor:
    """Feature map (None / "identity", "relu", "elu" = elu + 1) followed by the NeoX-style rotary embedding, one HIP kernel
    each way (mhla_nlp/fla/layers/mhla.py:297-299 + :311).  x: [B, T, H, K]; cos, sin: [>= t_offset + T, K/2] in x's dtype."""
    if x.dim() != 4 or x.shape[-1] % 8:
        raise ValueError("x: [B, T, H, K] with K % 8 == 0")
    if feature_map not in _FMAPS:
        raise ValueError(f"feature_map {feature_map!r}: one of {sorted(k for k in _FMAPS if k)} or None")
    if cos.dtype != x.dtype or sin.dtype != x.dtype or cos.shape[-1] != x.shape[-1] // 2 or cos.shape[0] < t_offset + x.shape[1]:
        raise ValueError("cos/sin: [>= t_offset + T, K/2] tables in the dtype of x")
    if cos.stride(-1) != 1 or sin.stride(-1) != 1 or cos.stride(0) != sin.stride(0):
        cos, sin = cos.contiguous(), sin.contiguous()
    return _FmapRotary.apply(x, cos, sin, _FMAPS[feature_map], int(t_offset))


@_device_guard
def _fmrot_decode_launch(q, k, cos, sin, state, ntok, off, T, left_padded, yq, yk, B, fmap):
    """The one library call of `featmap_rotary_decode`: the state gives `pos` and, a view of a pool, its slot map and slot count."""
    view = _view if off is None else _view0
    slot = state.map if isinstance(state, CausalStateView) else None
    rc = _lib.load().mhla_featmap_rotary_decode(
        view(q), view(k), cos.data_ptr(), sin.data_ptr(), cos.stride(0), cos.shape[0], state.pos.data_ptr(),
        slot.data_ptr() if slot is not None else None, state.dims[0] if slot is not None else 0,
        ntok.data_ptr() if ntok is not None else None, off.data_ptr() if off is not None else None, T, int(bool(left_padded)),
        view(yq), view(yk), B, q.shape[2], k.shape[2], q.shape[3], fmap, _DTYPES[q.dtype], _stream())
    _lib.check(rc, "mhla_featmap_rotary_decode")


def featmap_rotary_decode(q: torch.Tensor, k: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, state: "CausalState", *,
                          feature_map: Optional[str] = None, counts=None, left_padded: bool = False, cu_seqlens=None,
                          off_dev: Optional[torch.Tensor] = None, inplace: bool = False):
    """Feature map and rotary (`featmap_rotary`) of q AND k of a decode call's new tokens in ONE HIP launch, every row at the position
    the decode state gives it: row r of sequence b's window sits at `state.pos[b] + r` (a view of a pool: at its slot's position).
    The kernel reads the positions -- and the slot map -- on the device: no host position, no gathered table rows, nothing that a
    captured graph could not replay; it never writes them, so call it ahead of the step / extend / verify that advances the state.
    Returns `(q', k')`: bit for bit `featmap_rotary(x, cos.index_select(0, p), sin.index_select(0, p), feature_map)` at those
    positions p; rows outside every window, of an inactive entry of a device slot map, or at a position beyond the tables are zeros.
    q `[B, T, H, K]`, k `[B, T, Hkv, K]` (H a multiple of Hkv, K % 8 == 0; strided views -- slices of one fused projection -- are
    addressed in place); cos, sin `[tab_rows, K/2]` in q's dtype, used as they are.  state: a ragged `CausalState` or any view of a
    pool (dense, paged fp32, paged h16); only `pos` and the slot map are read, so a stale host mirror is fine.  A uniform state is a
    ValueError: `state.to_ragged()` puts its positions on the device.
    Token layouts, as `mhla_causal_extend` takes them: all T rows of every sequence (the default); `counts` (B ints in 0 .. T, rows
    `[0, counts[b])`, or `[T - counts[b], T)` with `left_padded`); `cu_seqlens` (packed new tokens: q, k `[1, N, ...]`, sequence b's
    rows `[cu[b], cu[b + 1])`; excludes `counts` and `left_padded`).  `counts` and `cu_seqlens` are validated as that call validates
    them and go to the device in one small copy.  `off_dev`: the offsets of a pack as a device int32 `[B + 1]` tensor the caller has
    validated and uploaded -- no host read, no copy (a cache uploads a step's offsets once for all layers); excludes the other two.
    `inplace`: the results overwrite q and k (which must then be addressable in place).  Inference only."""
    fn = "featmap_rotary_decode"
    if not isinstance(state, CausalState):
        raise TypeError(f"{fn}: state must be a CausalState, got {type(state).__name__}")
    _refuse_paged_pool(fn, state)
    if q.dim() != 4 or k.dim() != 4 or q.shape[-1] % 8 or q.shape[-1] < 8:
        raise ValueError(f"{fn}: q [B, T, H, K], k [B, T, Hkv, K] with K % 8 == 0")
    B, T, H, K = q.shape
    Hkv = k.shape[2]
    if tuple(k.shape) != (B, T, Hkv, K) or Hkv < 1 or H % Hkv or k.dtype != q.dtype or k.device != q.device:
        raise ValueError(f"{fn}: k is {k.dtype} {tuple(k.shape)} on {k.device}, expected [B={B}, T={T}, Hkv, K={K}] like q ({q.dtype} on "
                         f"{q.device}) with Hkv dividing H={H}")
    if q.dtype not in _DTYPES:
        raise ValueError(f"{fn}: unsupported dtype {q.dtype} (float32 / bfloat16 / float16)")
    if feature_map not in _FMAPS:
        raise ValueError(f"{fn}: feature_map {feature_map!r}: one of {sorted(f for f in _FMAPS if f)} or None")
    if any(t.dim() != 2 or t.dtype != q.dtype or t.device != q.device or t.shape[1] != K // 2 or t.shape[0] < 1 for t in (cos, sin)) or cos.shape != sin.shape:
        raise ValueError(f"{fn}: cos/sin: [tab_rows, K/2 = {K // 2}] tables in the dtype of q ({q.dtype}) on {q.device}")
    if state.pos is None or (state.lengths is None and not isinstance(state, CausalStateView)):
        raise ValueError(f"{fn}: the state is uniform ({state!r}) and has no positions on the device: pass state.to_ragged()")
    if state.pos.device != q.device:
        raise ValueError(f"{fn}: the state is on {state.pos.device}, q on {q.device}")
    if _wants_grad(q, k):
        raise ValueError(f"{fn} is inference only: call it under torch.no_grad() (an input requires grad)")
    rows = _state_rows(state)
    ntok = off = None
    if off_dev is not None:
        if counts is not None or cu_seqlens is not None or left_padded:
            raise ValueError(f"{fn}: off_dev (offsets already on the device) excludes counts, cu_seqlens and left_padded")
        if (not isinstance(off_dev, torch.Tensor) or off_dev.dtype != torch.int32 or off_dev.dim() != 1 or off_dev.shape[0] < 2
                or off_dev.device != q.device or not off_dev.is_contiguous()):
            raise ValueError(f"{fn}: off_dev is a contiguous int32 [sequences + 1] tensor on {q.device}")
        if B != 1:
            raise ValueError(f"{fn}: off_dev takes one packed row (B = 1), got B = {B}")
        off, nseq = off_dev, off_dev.shape[0] - 1
    elif cu_seqlens is not None:
        if counts is not None or left_padded:
            raise ValueError(f"{fn}: cu_seqlens (packed new tokens) excludes counts and left_padded, which place windows in padded tensors")
        if B != 1:
            raise ValueError(f"{fn}: cu_seqlens takes one packed row (B = 1), got B = {B}")
        cu = _cu_host(cu_seqlens.cu if isinstance(cu_seqlens, CausalVarlenPlan) else cu_seqlens)
        if cu[-1] != T:
            raise ValueError(f"{fn}: cu_seqlens ends at {cu[-1]}, the pack has N = {T} tokens")
        nseq = len(cu) - 1
    else:
        nseq = B
        if counts is not None:
            counts = _int_tuple(fn, "counts", counts, B, T)
    if rows != nseq:
        raise ValueError(f"{fn}: the state holds {rows} sequences, the tokens {nseq}")
    if T > _PACK_MAX_TOKENS:
        raise ValueError(f"{fn}: T = {T} token rows, one call takes {_PACK_MAX_TOKENS}")
    _require_gpu(q, k, cos, sin)
    if inplace:
        if not (_step_view_ok(q) and _step_view_ok(k)):
            raise ValueError(f"{fn}: inplace needs q and k addressable in place (last dim contiguous, strides multiples of 4 elements, "
                             f"{4 * q.element_size()}-byte aligned)")
        yq, yk = q, k
    else:
        q, k = (t if _step_view_ok(t) else t.contiguous() for t in (q, k))
        yq, yk = torch.empty((B, T, H, K), dtype=q.dtype, device=q.device), torch.empty((B, T, Hkv, K), dtype=q.dtype, device=q.device)
    if T == 0 or nseq == 0:   # (a pack whose sequences are all empty has no row)
        return yq, yk
    if cos.stride(1) != 1 or sin.stride(1) != 1 or cos.stride(0) != sin.stride(0) or cos.stride(0) % 4:
        cos, sin = cos.contiguous(), sin.contiguous()
    # the one small copy of the call: the counts, or the offsets of a pack (off_dev: none)
    if off is None and cu_seqlens is not None:
        off = torch.tensor(cu, dtype=torch.int32).to(q.device)
    elif counts is not None:
        ntok = torch.tensor(counts, dtype=torch.int32).to(q.device)
    _fmrot_decode_launch(q, k, cos, sin, state, ntok, off, T, left_padded, yq, yk, nseq, _FMAPS[feature_map])
    return yq, yk


class _QkPrologue(torch.autograd.Function):
    @staticmethod
    @_device_guard
    def forward(ctx, x, weight, cos, sin, norm_eps, eps, head_dim):
        lib = _lib.load()
        _require_gpu(x, weight, cos, sin)
        C = x.shape[-1]
        x2 = x.detach().reshape(-1, C)
        if x2.stride(-1) != 1:
            x2 = x2.contiguous()
        rows = x2.shape[0]
        y = torch.empty((rows, C), dtype=torch.float32, device=x.device)
        w = _f32(weight)
        rope = cos is not None
        yr = torch.empty_like(y) if rope else None
        head_dim = int(head_dim) if rope else 0
        rc = lib.mhla_qk_prologue_rope(x2.data_ptr(), x2.stride(0), _ptr(w), y.data_ptr(), C, yr.data_ptr() if rope else None, C, *_rope_args(cos, sin),
                                       cos.shape[0] if rope else 0, head_dim, rows, C, int(weight is not None), float(norm_eps),
                                       float(eps), _dtype_code(x2), _stream())
        if rc:
            _lib.check(rc, "mhla_qk_prologue_rope")
        ctx.save_for_backward(x2, w, cos, sin)
        ctx.cfg = (x.shape, float(norm_eps), head_dim, weight.dtype if weight is not None else None)
        if rope:
            return y.reshape(x.shape), yr.reshape(x.shape)
        return y.reshape(x.shape), None

    @staticmethod
    @_device_guard
    def backward(ctx, dy, dyr):
        lib = _lib.load()
        x2, w, cos, sin = ctx.saved_tensors
        shape, norm_eps, head_dim, w_dtype = ctx.cfg
        rows, C = x2.shape
        f32 = lambda t: None if t is None else t.reshape(rows, C).to(torch.float32).contiguous()
        dy, dyr = f32(dy), f32(dyr)
        if dy is None and dyr is None:
            return None, None, None, None, None, None, None
        dx = torch.empty((rows, C), dtype=x2.dtype, device=x2.device)
        dwp = None
        if w is not None:
            dwp = torch.empty((lib.mhla_qk_prologue_dw_rows(rows), C), dtype=torch.float32, device=x2.device)
        rope = dyr is not None
        if not rope:   # no gradient arrived for the rotated output: the call is the one of a forward without tables
            cos, sin, head_dim = None, None, 0
        rc = lib.mhla_qk_prologue_bwd(x2.data_ptr(), x2.stride(0), _ptr(w), _ptr(dy), C, dyr.data_ptr() if rope else None, C,
                                      *_rope_args(cos, sin), cos.shape[0] if rope else 0, head_dim, dx.data_ptr(), C, _ptr(dwp), rows, C,
                                      int(w is not None), norm_eps, _dtype_code(x2), _stream())
        if rc:
            _lib.check(rc, "mhla_qk_prologue_bwd")
        dw = dwp.sum(0).to(w_dtype) if dwp is not None else None
        return dx.reshape(shape), dw, None, None, None, None, None


def qk_prologue(x: torch.Tensor, weight: Optional[torch.Tensor], norm_eps: float = 1e-5, eps: float = 1e-6,
                rope=None, head_dim: Optional[int] = None):
    """relu(rmsnorm(x) * weight) + eps over the last dim, fp32 output -- the q / k prologue of Wan's MHLA_Video_Uni
    (wan/mhla_utils.py:268-272 after the .float() at :308) as one HIP kernel each way.  weight None: relu(x) + eps.
    With `rope=(cos, sin)` (fp32 [N, head_dim/2] tables, token = row % N) a second tensor, the output rotated as by
    `rope_apply` (:314), is produced in the same pass and `(y, y_rope)` is returned.  Differentiable w.r.t. x and weight."""
    if x.shape[-1] % 8:
        raise ValueError("channel dim must be a multiple of 8")
    if rope is not None:
        cos, sin = rope
        if head_dim is None or cos.dtype != torch.float32 or sin.dtype != torch.float32 or cos.shape != sin.shape or \
                cos.shape[1] != head_dim // 2 or x.shape[-1] % head_dim:
            raise ValueError("rope: fp32 [N, head_dim/2] cos/sin tables and head_dim dividing the channel dim")
        y, yr = _QkPrologue.apply(x, weight, cos.contiguous(), sin.contiguous(), norm_eps, eps, head_dim)
        return y, yr
    return _QkPrologue.apply(x, weight, None, None, norm_eps, eps, 0)[0]


# ------------------------------------------------------------------------------------------
# causal chunk-mixing MHLA (fla)
# ------------------------------------------------------------------------------------------
def _causal_check(what, q, k, v, mix, chunk_size, gate=None):
    """The forward checks of the causal nodes: a row of the mixing matrix for every chunk of the sequence; k, v, gate like q.
    Returns the number of chunks."""
    B, T, H, _ = q.shape
    n = (T + chunk_size - 1) // chunk_size
    L = mix.shape[0]
    if n > L:
        raise IndexError(f"sequence of {T} tokens needs {n} chunks but mixing_matrix has only {L} rows")
    _check_like(q, what, k=(k, q.shape), v=(v, (B, T, H, v.shape[-1])), gate=(gate, (B, T, H, v.shape[-1])))
    return n


def _causal_call(name, plan, *args):
    """mhla_causal_<name>(*args), checked; for a pack mhla_causal_varlen_<name>, whose two extra arguments -- the pack's chunk count
    and chunk table -- stand before the last four (scale, dtype, flags, stream)."""
    if plan is not None:
        name, args = "varlen_" + name, args[:-4] + (plan.n_chunks, plan.table.data_ptr()) + args[-4:]
    _lib.check(getattr(_lib.load(), "mhla_causal_" + name)(*args), "mhla_causal_" + name)


def _causal_bwd(q, k, v, mixf, dout, fwd_ws, chunk_size, scale, flags, plan=None):
    """mhla_causal_bwd on a node's saved tensors (`fwd_ws`: the forward's chunk summaries, None to recompute them):
    (dq, dk, dv, dmix), dmix fp32 in the shape of mixf.  `plan`: packed sequences -- mhla_causal_varlen_bwd over the plan's chunk
    table, mixf the plan's effective matrix [n, n]."""
    B, T, H, K = q.shape
    V = v.shape[-1]
    dq = _alloc_like_tokens(B, T, H, K, q)
    dk = _alloc_like_tokens(B, T, H, K, q)
    dv = q.new_empty((B, T, H, V))
    # the library writes every entry of the leading [n, n] block (zeros above the diagonal)
    n_chunks = (T + chunk_size - 1) // chunk_size if plan is None else plan.n_chunks
    dmix = (torch.empty if tuple(mixf.shape) == (n_chunks, n_chunks) else torch.zeros)(mixf.shape, dtype=torch.float32, device=q.device)
    dt = _dtype_code(q)
    ws = _ws(_cs_plan(B, T, H, K, V, chunk_size, dt, flags, None if plan is None else n_chunks)[1], q.device)
    _causal_call("bwd", plan, _view(q), _view(k), _view(v), mixf.data_ptr(), mixf.shape[1], _view(dout), _view(dq), _view(dk), _view(dv),
                 dmix.data_ptr(), dmix.shape[1], ws.data_ptr(), ws.numel() * 4, _ptr(fwd_ws), B, T, H, K, V, chunk_size, scale, dt, flags,
                 _stream())
    return dq, dk, dv, dmix


class _Causal(torch.autograd.Function):
    """`plan`: None, or the CausalVarlenPlan of a pack -- `mix` is then the plan's effective matrix [n, n] (a differentiable function
    of the mixing matrix) and the gradient returned for it is the library's dmix_eff."""

    @staticmethod
    @_device_guard
    def forward(ctx, q, k, v, mix, chunk_size, scale, flags, keep_limit, plan):
        _lib.load()   # (a missing library is reported before anything else)
        table, n_chunks = (None, None) if plan is None else (plan.table, plan.n_chunks)
        _require_gpu(q, k, v, mix, table)
        B, T, H, K = q.shape
        V = v.shape[-1]
        n = _causal_check("mhla_causal", q, k, v, mix, chunk_size)
        if plan is None and (mix.device != q.device or mix.dim() < 2 or mix.shape[1] < n):
            raise ValueError(f"mixing_matrix must be [L, L(, 1, 1, 1, 1)] with L >= {n} on {q.device}")
        q, k, v = _prep(q), _prep(k), _prep(v)
        mixf = _mix2d(mix, n_chunks)
        out = q.new_empty((B, T, H, V))
        ws = _ws(_cs_plan(B, T, H, K, V, chunk_size, _dtype_code(q), flags, n_chunks)[0], q.device)
        _causal_call("fwd", plan, _view(q), _view(k), _view(v), mixf.data_ptr(), mixf.shape[1], _view(out), ws.data_ptr(), ws.numel() * 4,
                     B, T, H, K, V, chunk_size, float(scale), _dtype_code(q), flags, _stream())
        # keep the chunk summaries (S_j and their prefix mixes) for the backward unless they are very large
        keep = ws.numel() * 4 <= keep_limit and any(ctx.needs_input_grad[:4])
        ctx.save_for_backward(q, k, v, mixf, ws if keep else None)
        ctx.cfg = (chunk_size, float(scale), mix.shape, mix.dtype, flags, plan)
        return out

    @staticmethod
    @_device_guard
    def backward(ctx, dout):
        q, k, v, mixf, fwd_ws = ctx.saved_tensors
        chunk_size, scale, mix_shape, mix_dtype, flags, plan = ctx.cfg
        dq, dk, dv, dmix = _causal_bwd(q, k, v, mixf, _prep(dout.to(q.dtype)), fwd_ws, chunk_size, scale, flags, plan)
        return dq, dk, dv, dmix if plan is not None else dmix.reshape(mix_shape).to(mix_dtype), None, None, None, None, None


class CausalVarlenPlan:
    """Packed sequences for the causal operator: every sequence of `cu` (cumulative lengths, as fla's `cu_seqlens`) cut into
    its own chunks -- a ragged last chunk per sequence, none for an empty one -- numbered c = 0 .. n_chunks - 1 along the pack.
    Built once per batch (`causal_varlen_plan`) and shared by every layer.

    cu        host tuple of the cumulative lengths
    n_chunks  chunks of the pack; max_chunks: of its longest sequence (rows of the mixing matrix it reads)
    table     device int32 [n_chunks, 2]: first token row and rows (1 .. chunk_size) of every chunk -- what the kernels read
    loc, seq  device int64 [n_chunks]: the chunk's index within its sequence, and its sequence
    dst       device int32 [n_chunks, 2]: (seq, loc) of every chunk -- where the packed prefill puts the chunk's K^T V in the ragged
              decode state (`mhla_causal_state(cu_seqlens=)`)"""

    def __init__(self, cu, device, chunk_size: int = 64):
        self.cu = tuple(cu)
        self.chunk_size = int(chunk_size)
        starts, counts, loc, seq = [], [], [], []
        for s in range(len(self.cu) - 1):
            for j, p in enumerate(range(self.cu[s], self.cu[s + 1], self.chunk_size)):
                starts.append(p)
                counts.append(min(self.chunk_size, self.cu[s + 1] - p))
                loc.append(j)
                seq.append(s)
        self.n_chunks = len(starts)
        self.max_chunks = max(loc) + 1 if loc else 0
        self.table = torch.tensor([starts, counts], dtype=torch.int32).t().contiguous().to(device)
        self.loc = torch.tensor(loc, dtype=torch.int64).to(device)
        self.seq = torch.tensor(seq, dtype=torch.int64).to(device)
        self.dst = torch.tensor([seq, loc], dtype=torch.int32).t().contiguous().to(device)
        c = torch.arange(self.n_chunks, device=self.table.device)
        self._mask = ((self.seq[:, None] == self.seq[None, :]) & (c[None, :] <= c[:, None])).to(torch.float32)

    @property
    def lengths(self):
        return tuple(b - a for a, b in zip(self.cu, self.cu[1:]))

    def mix_eff(self, mixing_matrix: torch.Tensor) -> torch.Tensor:
        """fp32 [n_chunks, n_chunks]: mix_eff[c, c'] = mixing_matrix[loc[c], loc[c']] where c and c' belong to the same sequence
        and c' <= c, exact zeros elsewhere -- the operator over the pack's chunks with this matrix is the operator over every
        sequence alone.  Differentiable: autograd's index backward sums a gradient of it into `mixing_matrix`."""
        if mixing_matrix.device != self.table.device:
            raise ValueError(f"mixing_matrix is on {mixing_matrix.device}, the plan on {self.table.device}")
        m = mixing_matrix.reshape(mixing_matrix.shape[0], mixing_matrix.shape[1]).to(torch.float32)
        return m[self.loc[:, None], self.loc[None, :]] * self._mask

    def __repr__(self):
        return f"CausalVarlenPlan(sequences={len(self.cu) - 1}, tokens={self.cu[-1]}, n_chunks={self.n_chunks}, device={self.table.device})"


def causal_varlen_plan(cu_seqlens, device=None, chunk_size: int = 64) -> CausalVarlenPlan:
    """The `CausalVarlenPlan` of `cu_seqlens` (a sequence of ints or a 1-D integer tensor; reading a device tensor synchronises,
    once -- build the plan once per batch and pass it to every layer as `cu_seqlens=`).  ValueError unless cu_seqlens is 1-D,
    starts at 0 and never decreases; empty sequences are allowed.  `device` defaults to the tensor's."""
    if isinstance(cu_seqlens, torch.Tensor) and device is None:
        device = cu_seqlens.device
    if int(chunk_size) <= 0:
        _cu_host(cu_seqlens, False)   # (its refusals of the argument's form come first)
        raise ValueError(f"chunk_size must be positive, got {chunk_size}")
    return CausalVarlenPlan(_cu_host(cu_seqlens), device if device is not None else "cpu", chunk_size)


def _cu_host(cu_seqlens, values=True):
    """`cu_seqlens` (a sequence of ints or a 1-D integer tensor, read once) as a host tuple: ValueError unless it is 1-D and -- with
    `values` -- starts at 0 and never decreases."""
    if isinstance(cu_seqlens, torch.Tensor):
        if cu_seqlens.dim() != 1 or cu_seqlens.is_floating_point() or cu_seqlens.is_complex():
            raise ValueError(f"cu_seqlens must be a 1-D integer tensor, got shape {tuple(cu_seqlens.shape)} of {cu_seqlens.dtype}")
        cu = cu_seqlens.tolist()
    else:
        cu = list(cu_seqlens)
        if any(isinstance(x, (list, tuple, torch.Tensor)) or int(x) != x for x in cu):
            raise ValueError(f"cu_seqlens must be a 1-D sequence of ints, got {cu_seqlens!r}")
    cu = tuple(int(x) for x in cu)
    if values and (len(cu) < 1 or cu[0] != 0):
        raise ValueError(f"cu_seqlens must start at 0, got {cu}")
    if values and any(b < a for a, b in zip(cu, cu[1:])):
        raise ValueError(f"cu_seqlens must be non-decreasing, got {cu}")
    return cu


def _causal_varlen_args(what, q, mixing_matrix, cu_seqlens, chunk_size) -> CausalVarlenPlan:
    """The checks of a packed call, all before the library is loaded or anything is launched; returns the plan."""
    if q.shape[0] != 1:
        raise ValueError(f"{what}: cu_seqlens takes one packed row (B = 1), got B = {q.shape[0]}")
    plan = cu_seqlens if isinstance(cu_seqlens, CausalVarlenPlan) else causal_varlen_plan(cu_seqlens, q.device, chunk_size)
    if plan.chunk_size != int(chunk_size):
        raise ValueError(f"{what}: the plan was built for chunk_size={plan.chunk_size}, the call has chunk_size={chunk_size}")
    if plan.cu[-1] != q.shape[1]:
        raise ValueError(f"{what}: cu_seqlens ends at {plan.cu[-1]}, the pack has T = {q.shape[1]} tokens")
    if plan.table.device != q.device:
        raise ValueError(f"{what}: the plan is on {plan.table.device}, expected {q.device}")
    L = mixing_matrix.shape[0]
    if plan.max_chunks > L:
        long = [i for i, n in enumerate(plan.lengths) if n > chunk_size * L]
        raise IndexError(f"{what}: sequences {long} of lengths {[plan.lengths[i] for i in long]} need more than the {L} rows of "
                         f"mixing_matrix ({chunk_size * L} tokens)")
    return plan


def _causal_group(fn, q, k, v, gate=None) -> int:
    """G = H / Hkv of an operator call whose k, v have fewer heads than q (grouped-query heads, the decode calls' convention:
    `_kv_group`); with G > 1 also the shapes -- k, v on the same Hkv heads, gate on q's H.  Host arithmetic, raised before the
    library is loaded."""
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        return 1   # (the operator's own shape errors)
    B, T, H, K = q.shape
    G = _kv_group(fn, H, k.shape[2])
    if G > 1:
        _check_like(q, fn, k=(k, (B, T, k.shape[2], K)), v=(v, (B, T, k.shape[2], v.shape[-1])), gate=(gate, (B, T, H, v.shape[-1])))
    return G


def _expand_kv(t: torch.Tensor, G: int) -> torch.Tensor:
    """[B, T, Hkv, D] -> [B, T, Hkv G, D], every head G times in a row (the layer's '(h g)' order, `repeat_interleave(G, 2)`), as a
    differentiable expand + reshape: autograd sums the G gradients of a head back onto it."""
    B, T, Hkv, D = t.shape
    return t[:, :, :, None, :].expand(B, T, Hkv, G, D).reshape(B, T, Hkv * G, D)


@_device_guard
def _causal_fwd_gqa(q, k, v, mix, gate, weight, chunk_size, scale, norm_eps, flags, plan, epi):
    """The grouped-query forward without a graph (mhla_causal_fwd_gqa and its kin): q [B, T, H, K] on k, v of Hkv heads, un-repeated.
    The chunk summaries, their mixes and the workspace exist once per k/v head; `epi`: the fused norm x gate output.  `plan`, `mix`:
    as _Causal takes them."""
    _lib.load()
    table, n_chunks = (None, None) if plan is None else (plan.table, plan.n_chunks)
    _require_gpu(q, k, v, mix, gate, weight, table)
    B, T, H, K = q.shape
    Hkv, V = k.shape[2], v.shape[-1]
    n = (T + chunk_size - 1) // chunk_size
    if n > mix.shape[0]:
        raise IndexError(f"sequence of {T} tokens needs {n} chunks but mixing_matrix has only {mix.shape[0]} rows")
    if plan is None and (mix.device != q.device or mix.dim() < 2 or mix.shape[1] < n):
        raise ValueError(f"mixing_matrix must be [L, L(, 1, 1, 1, 1)] with L >= {n} on {q.device}")
    q, k, v = _prep(q.detach()), _prep(k.detach()), _prep(v.detach())
    mixf = _mix2d(mix, n_chunks)
    dt = _dtype_code(q)
    out = q.new_empty((B, T, H, V))
    ws = _ws(_cs_plan(B, T, Hkv, K, V, chunk_size, dt, flags, n_chunks)[0], q.device)   # (by the k/v heads: 1 / G of the repeated call's)
    tail = (ws.data_ptr(), ws.numel() * 4, B, T, H, Hkv, K, V, chunk_size, float(scale), dt, flags, _stream())
    if not epi:
        _causal_call("fwd_gqa", plan, _view(q), _view(k), _view(v), mixf.data_ptr(), mixf.shape[1], _view(out), *tail)
    else:
        gate = _prep(gate.detach()) if gate is not None else None
        wf = _f32(weight)
        _causal_call("normgate_fwd_gqa", plan, _view(q), _view(k), _view(v), mixf.data_ptr(), mixf.shape[1], NULL_VIEW, _view_or_null(gate),
                     _ptr(wf), float(norm_eps), _view(out), *tail)
    return out


def _causal_keep_limit(keep_state_limit: Optional[int]) -> int:
    return CAUSAL_KEEP_STATE_LIMIT_BYTES if keep_state_limit is None else int(keep_state_limit)


def _causal_flags(summaries: str, force_generic: bool) -> int:
    if summaries not in SUMMARIES:
        raise ValueError(f"summaries={summaries!r}: 'tf32' / 'split' (bf16 hi + lo pairs, the reference's fp32 arithmetic) or 'bf16'")
    return ((_lib.CAUSAL_BF16_SUMMARIES if summaries == "bf16" else 0) | (_lib.CAUSAL_FP32_GRADE_SUMMARIES if summaries == "split" else 0)
            | (_lib.CAUSAL_FORCE_GENERIC if force_generic else 0))


def mhla_causal(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mixing_matrix: torch.Tensor,
                chunk_size: int = 64, scale: Optional[float] = None, *, summaries: str = "tf32",
                force_generic: bool = False, keep_state_limit: Optional[int] = None, cu_seqlens=None) -> torch.Tensor:
    """Causal chunk-mixing MHLA operator (naive_chunk_simple_mhla_fixed,
    mhla_nlp/fla/ops/mhla/naive.py:10-83).  q, k: [B, T, H, K]; v: [B, T, H, V];
    mixing_matrix: [L, L] or [L, L, 1, 1, 1, 1], L >= ceil(T / chunk_size).  fp32 compute, output in
    the dtype of q; `scale` defaults to K**-0.5 as in the reference (naive.py:42).
    summaries: how bf16 problems keep the chunk summaries S, P, dP, dS between their two contractions (score tiles and operands are
    bf16 hi + lo pairs with fp32 accumulation in every case but "bf16") -- "tf32" (default): STORED with 11 significand bits (fp16
    payload x one power-of-two multiplier per 16-row strip of a chunk tile, 2 bytes per element), the precision of the reference's
    matmuls under allow_tf32; within one final rounding + 1e-3 of the fp32 result (observed 4e-4); "split": bf16 hi + lo pairs,
    >= 16 significand bits (naive.py:39, :60-78; 4 bytes per element); "bf16": one bf16 value each, score tiles too -- REDUCED
    PRECISION (2-3e-3 of the result's maximum).
    force_generic: testing aid -- the generic fp32-MFMA kernels for every shape.
    keep_state_limit: largest forward workspace (bytes: the chunk summaries S, P -- 4 B T H K V / 64 bytes at the default, 8 with hi + lo pairs)
    kept alive for the backward; above it the backward recomputes them.  Default: ops.CAUSAL_KEEP_STATE_LIMIT_BYTES
    (set_keep_state_limits).
    cu_seqlens: packed sequences, the fla convention (B = 1) -- a `CausalVarlenPlan` (`causal_varlen_plan`: build it once per
    batch), a sequence of ints or a 1-D tensor (read once: a device tensor synchronises), starting at 0, non-decreasing, ending at
    T.  Every sequence is computed exactly as if it were alone in a call of its own: its chunks are cut from its own first token
    and see rows 0.. of the mixing matrix and nothing of their neighbours.  Empty sequences are allowed; IndexError, before
    anything is launched, names the sequences longer than 64 L tokens.
    Grouped-query heads: k [B, T, Hkv, K], v [B, T, Hkv, V] with H = G Hkv, G <= 8; query head h uses k/v head h // G.  The result
    is, bit for bit, that of the call on `k.repeat_interleave(G, 2)`, `v.repeat_interleave(G, 2)`.  With no gradient to compute
    (grad mode off, or nothing that requires one) the forward runs natively on the un-repeated heads: chunk summaries, their
    mixes and the workspace once per k/v head, no copy of k or v.  When a gradient is needed, k and v are expanded to H heads
    inside the graph and today's nodes run -- the backward still works on repeated heads, because the group sums of dk / dv
    belong in a token kernel that has no registers left for them and the group-summed dP in the summary kernel -- and autograd
    returns dk, dv on Hkv heads."""
    if q.dim() != 4 or v.dim() != 4:
        raise ValueError("q, k: [B, T, H, K], v: [B, T, H, V]")
    if int(chunk_size) <= 0:
        raise ValueError(f"chunk_size must be positive, got {chunk_size}")
    keep_limit = _causal_keep_limit(keep_state_limit)
    flags = _causal_flags(summaries, force_generic)
    if scale is None:
        scale = q.shape[-1] ** -0.5
    G = _causal_group("mhla_causal", q, k, v)
    plan = _causal_varlen_args("mhla_causal", q, mixing_matrix, cu_seqlens, chunk_size) if cu_seqlens is not None else None
    if G > 1 and _wants_grad(q, k, v, mixing_matrix):   # the backward's kernels take repeated heads: today's nodes on expanded k, v
        k, v = _expand_kv(k, G), _expand_kv(v, G)
    elif G > 1:
        B, T, H, _ = q.shape
        if B == 0 or T == 0:
            return torch.zeros((B, T, H, v.shape[-1]), dtype=v.dtype, device=v.device)
        mix = mixing_matrix if plan is None else plan.mix_eff(mixing_matrix)
        nb = max(1, min(B, _MAX_GRID_BH // H))   # (slices sized by the query heads: they are what the output launch's grid counts)
        outs = [_causal_fwd_gqa(q[i:i + nb], k[i:i + nb], v[i:i + nb], mix, None, None, int(chunk_size), scale, 0.0, flags, plan, False)
                for i in range(0, B, nb)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
    if plan is not None and q.shape[1] > 0:
        return _Causal.apply(q, k, v, plan.mix_eff(mixing_matrix), int(chunk_size), scale, flags, keep_limit, plan)
    if q.shape[0] == 0 or q.shape[1] == 0:   # empty batch / sequence
        return torch.zeros_like(v) + 0 * (q.sum() + k.sum() + mixing_matrix.sum()).to(v.dtype)
    nb = _MAX_GRID_BH // q.shape[2]
    if q.shape[0] > nb:   # see mhla_blockmix
        return torch.cat([_Causal.apply(q[i:i + nb], k[i:i + nb], v[i:i + nb], mixing_matrix, int(chunk_size), scale, flags, keep_limit, None)
                          for i in range(0, q.shape[0], nb)], dim=0)
    if _native_nodes():
        return torch.ops.mhla_amd.causal(q, k, v, mixing_matrix, int(chunk_size), float(scale), flags, keep_limit)
    return _Causal.apply(q, k, v, mixing_matrix, int(chunk_size), scale, flags, keep_limit, None)


def naive_chunk_simple_mhla_fixed(q, k, v, mixing_matrix, output_final_state: bool = False, chunk_size: int = 64,
                                  *args, **kwargs):
    """Drop-in for the reference op function of the same name (naive.py:11): same arguments,
    returns only `o` (the reference discards the state, naive.py:80)."""
    return mhla_causal(q, k, v, mixing_matrix, chunk_size)


class _CausalNormGate(torch.autograd.Function):
    """Causal operator + per-head RMSNorm x swish gate as ONE node: the forward applies the epilogue inside the operator's
    output kernel (mhla_causal_normgate_fwd); the backward is the norm's backward kernel followed by the operator's backward.
    `plan`: as _Causal takes it."""

    @staticmethod
    @_device_guard
    def forward(ctx, q, k, v, mix, gate, weight, chunk_size, scale, norm_eps, flags, keep_limit, plan):
        _lib.load()
        table, n_chunks = (None, None) if plan is None else (plan.table, plan.n_chunks)
        _require_gpu(q, k, v, mix, gate, weight, table)
        B, T, H, K = q.shape
        V = v.shape[-1]
        _causal_check("mhla_causal_normgate", q, k, v, mix, chunk_size, gate)
        q, k, v = _prep(q), _prep(k), _prep(v)
        gate = _prep(gate) if gate is not None else None
        mixf = _mix2d(mix, n_chunks)
        wf = _f32(weight)
        need_grad = any(ctx.needs_input_grad[:6])
        out = q.new_empty((B, T, H, V)) if need_grad else None
        y = q.new_empty((B, T, H, V))
        ws = _ws(_cs_plan(B, T, H, K, V, chunk_size, _dtype_code(q), flags, n_chunks)[0], q.device)
        _causal_call("normgate_fwd", plan, _view(q), _view(k), _view(v), mixf.data_ptr(), mixf.shape[1], _view_or_null(out),
                     _view_or_null(gate), _ptr(wf), float(norm_eps), _view(y), ws.data_ptr(), ws.numel() * 4, B, T, H, K, V, chunk_size,
                     float(scale), _dtype_code(q), flags, _stream())
        keep = ws.numel() * 4 <= keep_limit and need_grad
        ctx.save_for_backward(q, k, v, mixf, out, gate, wf, ws if keep else None)
        ctx.cfg = (chunk_size, float(scale), float(norm_eps), mix.shape, mix.dtype, weight.dtype if weight is not None else None, flags, plan)
        return y

    @staticmethod
    @_device_guard
    def backward(ctx, dy):
        q, k, v, mixf, out, gate, wf, fwd_ws = ctx.saved_tensors
        chunk_size, scale, norm_eps, mix_shape, mix_dtype, w_dtype, flags, plan = ctx.cfg
        do, dg, dw = _rmsnorm_gate_bwd(out, gate.contiguous() if gate is not None else None, wf, dy, norm_eps, w_dtype)
        dq, dk, dv, dmix = _causal_bwd(q, k, v, mixf, do, fwd_ws, chunk_size, scale, flags, plan)
        return dq, dk, dv, dmix if plan is not None else dmix.reshape(mix_shape).to(mix_dtype), dg, dw, None, None, None, None, None, None


def causal_normgate_fusable(q: torch.Tensor, v: torch.Tensor, chunk_size: int = 64, flags: int = 0, cu_seqlens=None) -> bool:
    """Shapes the fused epilogue covers (the library's own answer, mhla_causal_normgate_fusable: bf16, K % 64 == 0, K <= 256,
    V % 64 == 0, V <= 256 or V = 384 / 512, at most 256 chunks) within one launch's (batch, head) range.  cu_seqlens (as
    mhla_causal takes it): the answer for the pack, by its chunk count."""
    if q.dtype not in _DTYPES or not (q.shape[0] > 0 and q.shape[1] > 0 and q.shape[0] * q.shape[2] <= _MAX_GRID_BH):
        return False
    fn, pack = "mhla_causal_normgate_fusable", ()
    if cu_seqlens is not None:
        plan = cu_seqlens if isinstance(cu_seqlens, CausalVarlenPlan) else causal_varlen_plan(cu_seqlens, q.device, chunk_size)
        fn, pack = "mhla_causal_varlen_normgate_fusable", (plan.n_chunks,)
    return getattr(_lib.load(), fn)(q.shape[1], q.shape[-1], v.shape[-1], chunk_size, *pack, _DTYPES[q.dtype], flags) == 1


def mhla_causal_normgate(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mixing_matrix: torch.Tensor,
                         gate: Optional[torch.Tensor], weight: Optional[torch.Tensor], norm_eps: float = 1e-5,
                         chunk_size: int = 64, scale: Optional[float] = None, *, summaries: str = "tf32",
                         keep_state_limit: Optional[int] = None, cu_seqlens=None) -> torch.Tensor:
    """`rmsnorm_gate(mhla_causal(q, k, v, mix), gate, weight, norm_eps)` -- the fla layer's operator + FusedRMSNormGated
    (mhla_nlp/fla/layers/mhla.py:330-355).  Where the fused epilogue applies (bf16, K, V multiples of 64, K <= 256, V <= 256 or
    384 / 512, at most 256 chunks) the norm x gate runs inside the operator's output kernel; other shapes compose the two HIP operators.
    `summaries`, `keep_state_limit`, `cu_seqlens`, grouped-query heads (k, v on Hkv heads; gate, like q, on H): see mhla_causal."""
    if int(chunk_size) <= 0:
        raise ValueError(f"chunk_size must be positive, got {chunk_size}")
    flags = _causal_flags(summaries, False)
    if scale is None:
        scale = q.shape[-1] ** -0.5
    plan = None
    if cu_seqlens is not None:
        if q.dim() != 4 or v.dim() != 4:
            raise ValueError("q, k: [B, T, H, K], v: [B, T, H, V]")
        plan = _causal_varlen_args("mhla_causal_normgate", q, mixing_matrix, cu_seqlens, chunk_size)
    G = _causal_group("mhla_causal_normgate", q, k, v, gate)
    if not causal_normgate_fusable(q, v, chunk_size, flags, plan):
        return rmsnorm_gate(mhla_causal(q, k, v, mixing_matrix, chunk_size, scale, summaries=summaries, keep_state_limit=keep_state_limit,
                                        cu_seqlens=plan), gate, weight, norm_eps)
    if G > 1 and _wants_grad(q, k, v, mixing_matrix, gate, weight):
        k, v = _expand_kv(k, G), _expand_kv(v, G)
    elif G > 1:
        return _causal_fwd_gqa(q, k, v, mixing_matrix if plan is None else plan.mix_eff(mixing_matrix), gate, weight, int(chunk_size), scale,
                               norm_eps, flags, plan, True)
    return _CausalNormGate.apply(q, k, v, mixing_matrix if plan is None else plan.mix_eff(mixing_matrix), gate, weight, int(chunk_size), scale,
                                 norm_eps, flags, _causal_keep_limit(keep_state_limit), plan)


def naive_recurrent_mhla(q, k, v, mixing_matrix, chunk_size: int = 64, scale: Optional[float] = None,
                         initial_state: Optional[torch.Tensor] = None, output_final_state: bool = True):
    """Drop-in for the reference's token-recurrent form (mhla_nlp/fla/ops/mhla/naive.py:88-142), which the fla layer calls
    when T <= 64 (layers/mhla.py:247): same arguments, returns `(o, S)`.

    For T <= chunk_size (the only case the layer uses it for) the recurrence is exactly the single-chunk case of the chunk
    operator, which is what runs here (one HIP launch chain instead of a T-step Python loop).  Documented deviations, both
    from defects of the reference rather than from its intent: (1) beyond the first chunk the reference prepends a zero state
    and so reads every earlier chunk's state shifted by one (naive.py:124-127, 133); this function computes the chunk operator
    `naive_chunk_simple_mhla_fixed` instead; (2) the reference ignores `scale` (naive.py:101 overwrites it with K**-0.5) and
    `initial_state` only seeds the returned tensor `S`, never the output (naive.py:113-116) -- both reproduced: `scale` is
    ignored, and `S` is `initial_state` (or zeros) [B, H, K, V] in fp32, `None` when `output_final_state` is False."""
    if scale is not None and abs(float(scale) - q.shape[-1] ** -0.5) > 1e-12:
        warnings.warn("naive_recurrent_mhla ignores `scale` (the reference overwrites it with K**-0.5, naive.py:101)", stacklevel=2)
    if q.shape[1] > chunk_size:
        warnings.warn(f"naive_recurrent_mhla on T={q.shape[1]} > chunk_size={chunk_size} tokens runs the chunk operator; the reference's "
                      "recurrent form reads every earlier chunk's state shifted by one there (naive.py:124-133, not replicated)", stacklevel=2)
    o = mhla_causal(q, k, v, mixing_matrix, chunk_size, None)
    S = None
    if output_final_state:
        B, _, H, K = q.shape
        S = torch.zeros(B, H, K, v.shape[-1], dtype=torch.float32, device=q.device)
        if initial_state is not None:
            S = S + initial_state
    return o, S


# ------------------------------------------------------------------------------------------
# causal operator, decoding: prefill state + single-token step
# ------------------------------------------------------------------------------------------
class CausalState:
    """Decode state of the causal operator, fp32 whatever the tensor dtype: `S [B, H, cap, K, V]` (K_j^T V_j of every finished
    chunk), `P [B, H, K, V]` (prefix mix of the open chunk), `Cur [B, H, K, V]` (the open chunk's running K^T V), `seen` tokens
    so far.  Every row of the mixing matrix weighs the finished chunks differently, so all of them are kept: 4 K V bytes per
    chunk and head (128 KB at K = 128, V = 256) -- `nbytes` reports the total.  A UNIFORM state (`lengths is None`): all sequences
    of the batch share `seen`.  A RAGGED state (built with `lengths=`, and ragged from then on even if the lengths are equal): sequence
    b has seen `lengths[b]` tokens and behaves exactly as if it lived alone in a batch of one.  `lengths` (a tuple of B ints) is the
    host mirror every check and the boundary decision read; `pos` (int32 [B] on the state's device) holds the same numbers for the
    kernels, which advance it themselves -- a step costs no copy and no synchronisation; `seen` is kept equal to `max(lengths)`.
    Device-positioned steps (`mhla_causal_step_dev`) move `pos` alone and leave the mirror behind: the state is then `stale`, every
    call that reads the mirror refuses it, and `sync()` reads `pos` back.  `full` (int32 [B] on the state's device, zeros, created on
    first use) is where those steps flag a sequence they found beyond the capacity.
    Grouped-query heads: the state is a function of k and v alone, so its head count is that of k and v (Hkv), whatever the number
    of query heads -- every decode call, and the operator that computes a prefill's output rows (`mhla_causal`), takes q
    `[B, T, H, K]` with k, v `[B, T, Hkv, .]` and a state of Hkv heads, H = G Hkv, G <= 8."""

    __slots__ = ("S", "P", "Cur", "seen", "chunk_size", "lengths", "pos", "stale", "_full")
    pages = None   # (a paged pool and its views hold the finished chunks as pages instead of S: `PagedCausalState`)
    page_mult = None   # (the multipliers of a paged pool of h16 pages: None for every other state)

    def __init__(self, S: torch.Tensor, P: torch.Tensor, Cur: torch.Tensor, seen: int = 0, chunk_size: int = 64, *, lengths=None,
                 pos: Optional[torch.Tensor] = None):
        self.S, self.P, self.Cur, self.seen, self.chunk_size = S, P, Cur, int(seen), int(chunk_size)
        self.lengths = self.pos = self._full = None
        self.stale = False
        if lengths is not None:
            lengths = _int_tuple("CausalState", "lengths", lengths, S.shape[0], None)
            if pos is None:
                pos = torch.tensor(lengths, dtype=torch.int32, device=S.device)
            elif pos.dtype != torch.int32 or tuple(pos.shape) != (len(lengths),):
                raise ValueError(f"CausalState: pos must be an int32 tensor of shape ({len(lengths)},), got {pos.dtype} {tuple(pos.shape)}")
            self.lengths, self.pos, self.seen = lengths, pos, max(lengths)
        elif pos is not None:
            raise ValueError("CausalState: pos given without lengths")

    @classmethod
    def empty(cls, B: int, H: int, K: int, V: int, capacity_chunks: int, device="cuda", chunk_size: int = 64) -> "CausalState":
        if min(B, H, K, V, capacity_chunks) <= 0:
            raise ValueError(f"CausalState.empty: non-positive size B={B} H={H} K={K} V={V} capacity_chunks={capacity_chunks}")
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
        return cls(z(B, H, capacity_chunks, K, V), z(B, H, K, V), z(B, H, K, V), 0, chunk_size)

    # what the checks and launches read of a state's geometry, so that a pool whose finished chunks are pages (`PagedCausalState`),
    # which has no dense S, answers them too
    @property
    def dims(self):
        """(batch rows, k/v heads, capacity in chunks, K, V)."""
        return tuple(self.S.shape)

    @property
    def device(self):
        return self.S.device

    @property
    def _chunks(self) -> torch.Tensor:
        """The tensor that holds the finished chunks: S, or the pages of a paged pool."""
        return self.S

    @property
    def capacity_chunks(self) -> int:
        return self.S.shape[2]

    @property
    def nbytes(self) -> int:
        return 4 * (self.S.numel() + self.P.numel() + self.Cur.numel() + sum(t.numel() for t in (self.pos, self._full) if t is not None))

    @property
    def full(self) -> torch.Tensor:
        """int32 [B] zeros on the state's device, created on first use: a device-positioned step sets `full[b] = 1` when it finds
        sequence b beyond the capacity (and leaves that sequence as it is); nothing but the caller clears it."""
        if self._full is None:
            self._full = torch.zeros(self.dims[0], dtype=torch.int32, device=self.device)
        return self._full

    def to_ragged(self) -> "CausalState":
        """A ragged state on the SAME storage (S, P, Cur are shared, not copied), every length equal to `seen` -- what
        `mhla_causal_step_dev` takes.  A ragged state returns itself."""
        if self.lengths is not None:
            return self
        return CausalState(self.S, self.P, self.Cur, 0, self.chunk_size, lengths=(self.seen,) * self.S.shape[0])

    def sync(self) -> "CausalState":
        """Bring the host mirror up to the device after device-positioned steps: `pos` and `full` are read back in one copy --
        the one device-to-host copy of that path, and it synchronises --, `lengths` and `seen` are refreshed and the state is no
        longer stale.  Then, if any `full` flag is set, IndexError naming those sequences: they were stepped beyond the
        capacity, their rows from then on were zeros and their state stopped at the capacity.  A uniform state has nothing on
        the device to read."""
        if self.lengths is None:
            return self
        host = (self.pos if self._full is None else torch.stack((self.pos, self._full))).tolist()
        pos, full = (host, ()) if self._full is None else host
        self.lengths, self.seen, self.stale = tuple(int(n) for n in pos), max(int(n) for n in pos), False
        over = [b for b, f in enumerate(full) if f]
        if over:
            raise IndexError(f"{type(self).__name__}.sync: sequences {over} were stepped beyond the capacity of {self.capacity_chunks} chunks "
                             f"({64 * self.capacity_chunks} tokens){self._sync_cause}: their rows from there on are zeros "
                             f"(lengths={self.lengths})")
        return self

    _sync_cause = ""   # (what else sets a `full` flag: a paged pool names a chunk without a page)

    def _refuse_stale(self, fn: str):
        if self.stale:
            raise ValueError(f"{fn}: the state was advanced by mhla_causal_step_dev and its host mirror (lengths, seen) is stale: "
                             "call state.sync() first")

    def clone(self) -> "CausalState":
        c = CausalState(self.S.clone(), self.P.clone(), self.Cur.clone(), self.seen, self.chunk_size, lengths=self.lengths,
                        pos=self.pos.clone() if self.pos is not None else None)
        c.stale = self.stale
        if self._full is not None:
            c._full = self._full.clone()
        return c

    @classmethod
    def cat(cls, states) -> "CausalState":
        """The states of separately prefilled requests as one batch (copies; the inputs stay usable).  Uniform inputs that have all
        seen the same number of tokens give a uniform state; differing lengths, or any ragged input, give a ragged one.  ValueError
        when H, K, V, capacity, chunk size or device differ."""
        states = list(states)
        if not states or not all(isinstance(s, CausalState) for s in states):
            raise ValueError("CausalState.cat: a non-empty sequence of CausalState")
        for s in states:
            _refuse_paged_pool("CausalState.cat", s)
        states = [s.compact() if isinstance(s, CausalStateView) else s for s in states]   # (a view: copies of its slots)
        a = states[0]
        for s in states[1:]:
            if tuple(s.S.shape[1:]) != tuple(a.S.shape[1:]) or s.chunk_size != a.chunk_size or s.S.device != a.S.device:
                raise ValueError(f"CausalState.cat: {s!r} does not go with {a!r} (H, K, V, capacity, chunk size and device must agree)")
        for s in states:
            s._refuse_stale("CausalState.cat")
        S, P, Cur = (torch.cat([getattr(s, n) for s in states], dim=0) for n in ("S", "P", "Cur"))
        if all(s.lengths is None and s.seen == a.seen for s in states):
            return cls(S, P, Cur, a.seen, a.chunk_size)
        lengths = [n for s in states for n in (s.lengths if s.lengths is not None else (s.seen,) * s.S.shape[0])]
        out = cls(S, P, Cur, 0, a.chunk_size, lengths=lengths)
        if any(s._full is not None for s in states):
            out._full = torch.cat([s.full for s in states])
        return out

    # ---- a ragged state as a POOL of slots: requests stay in their batch row (slot) while the set of live ones changes
    def at(self, slots) -> "CausalStateView":
        """The batch rows `slots` of this ragged state (a pool of `B` slots), in that order, as a state of `len(slots)` sequences on the
        SAME storage: nothing is copied, and every decode call that takes a state takes the view and reads and writes the pool
        in place -- see `CausalStateView`.  slots: a sequence of distinct ints in 0 .. B - 1 (ValueError naming the offenders
        otherwise), or an int32 tensor `[n]` on the state's device, which only `mhla_causal_step_dev` takes.  A uniform state is
        refused: call `to_ragged()` first."""
        return CausalStateView(self, slots)

    def _pool_slots(self, fn: str, slots):
        """What `reset` and `fork` check: a ragged state that is not stale, and `slots` as `at` takes a list."""
        if self.lengths is None:
            raise ValueError(f"{fn}: the state is uniform ({self!r}): a pool of slots is a ragged state, call to_ragged() first")
        self._refuse_stale(fn)
        return _slot_tuple(fn, slots, self.dims[0])

    def _set_lengths(self, slots, values):
        lengths = list(self.lengths)
        for s, n in zip(slots, values):
            lengths[s] = int(n)
        self.lengths, self.seen = tuple(lengths), max(lengths)

    def reset(self, slots) -> "CausalState":
        """Empty the slots `slots` of a pool for new requests: P, Cur, pos, full and the host mirror of those rows become zero (plain
        tensor operations, no kernel).  S needs no clearing: rows beyond a sequence's finished chunks are never read."""
        slots = self._pool_slots("CausalState.reset", slots)
        idx = torch.tensor(slots, dtype=torch.int64).to(self.S.device)
        for t in (self.P, self.Cur, self.pos, self._full):
            if t is not None:
                t[idx] = 0
        self._set_lengths(slots, (0,) * len(slots))
        return self

    def fork(self, src: int, dst: int) -> "CausalState":
        """Copy slot `src` of a pool over slot `dst` (a shared prompt prefix, beams): the finished chunks of S, P, Cur, pos, full
        and the host mirror -- plain tensor copies, no kernel.  Rows of S beyond the finished chunks are not copied: nothing reads
        them."""
        src, dst = self._pool_slots("CausalState.fork", (src, dst))
        n = self.lengths[src]
        self.S[dst, :, :n // 64] = self.S[src, :, :n // 64]
        for t in (self.P, self.Cur, self.pos, self._full):
            if t is not None:
                t[dst] = t[src]
        self._set_lengths((dst,), (n,))
        return self

    def __repr__(self):
        B, H, cap, K, V = self.S.shape
        seen = f"seen={self.seen}" if self.lengths is None else f"lengths={self.lengths}"
        return f"CausalState(B={B}, H={H}, K={K}, V={V}, capacity_chunks={cap}, {seen}, device={self.S.device})"


def _slot_tuple(fn, slots, n_slots):
    """`slots` as a tuple of distinct ints in 0 .. n_slots - 1, at least one; ValueError naming the offenders otherwise."""
    slots = list(slots)
    bad = [s for s in slots if isinstance(s, bool) or not isinstance(s, int)]
    if bad:
        raise ValueError(f"{fn}: slots must be ints, got {bad}")
    if not slots:
        raise ValueError(f"{fn}: no slot given (at least one)")
    out = [s for s in slots if not 0 <= s < n_slots]
    if out:
        raise ValueError(f"{fn}: slots {out} are outside 0 .. {n_slots - 1} (the pool has {n_slots})")
    dup = sorted({s for s in slots if slots.count(s) > 1})
    if dup:
        raise ValueError(f"{fn}: slots {dup} are given more than once (rows of a call that share a slot would race)")
    return tuple(slots)


class CausalStateView(CausalState):
    """`pool.at(slots)`: the rows `slots` of a ragged `CausalState` (the pool), in that order, as a state of B = len(slots) sequences.
    It owns nothing: S, P, Cur, pos, full, the host mirror and `stale` are the pool's.  The decode calls -- `mhla_causal_step`,
    `mhla_causal_step_dev`, `mhla_causal_extend` (with and without `counts`), `mhla_causal_verify`, `mhla_causal_commit` -- take it where
    they take a state, and the pack prefill takes it as `into=`: row b of the call then reads and writes slot `slots[b]` of the pool
    in place (the library's `*_slots` entry points), and gives bit for bit what the call gives on `view.compact()`, a compact state
    holding copies of those slots.  Slots the view does not name keep every bit.  Nothing is gathered, scattered or concatenated.
    slots as a sequence of ints: HOST-POSITIONED.  `lengths` is `tuple(pool.lengths[s] for s in slots)`; after a call the pool's
    mirror has advanced at exactly those slots; the small device copy of the map is made once and kept on the view.
    slots as an int32 tensor `[B]` on the pool's device: DEVICE-POSITIONED, for `mhla_causal_step_dev` alone (every other call
    raises ValueError).  Its contents are never read by the host and may be rewritten in place between calls or replays of a captured
    graph: an entry outside 0 .. n_slots - 1, -1 for instance, makes that row INACTIVE -- its row of the result is zeros and no slot,
    position or flag is touched; entries that name a slot must be distinct (rows that share one race).  The step marks the POOL
    stale, and `pool.sync()` refreshes it.
    Not covered: `DecodeCache` builds its states as before (the fla layer and `hosts/gpt.py` run on a PAGED pool through
    `modules.PagedDecodeCache`); a slot of a dense pool reserves all `capacity_chunks` chunks (`PagedCausalState`: a pool whose
    finished chunks are pages)."""

    __slots__ = ("pool", "slots", "_map", "_mirror", "dims", "pages")

    def __init__(self, pool: CausalState, slots):
        self._mirror = (None, None)   # (the pool's lengths tuple the view's were last taken from, the view's lengths)
        fn = "CausalState.at"
        if isinstance(pool, CausalStateView):
            raise ValueError(f"{fn}: a view of a view; take the slots from the pool")
        if pool.lengths is None:
            raise ValueError(f"{fn}: the state is uniform ({pool!r}): a pool of slots is a ragged state, call to_ragged() first")
        self.pool, self.dims, self.pages = pool, pool.dims, pool.pages   # (neither changes while the pool lives: kept, not looked up per call)
        if isinstance(slots, torch.Tensor):
            if slots.dtype != torch.int32 or slots.dim() != 1 or slots.shape[0] < 1 or slots.device != pool.device or not slots.is_contiguous():
                raise ValueError(f"{fn}: a slot map on the device is a contiguous int32 [B >= 1] tensor on {pool.device}, got "
                                 f"{slots.dtype} {tuple(slots.shape)} on {slots.device}")
            self.slots, self._map = None, slots
        else:
            self.slots, self._map = _slot_tuple(fn, slots, pool.dims[0]), None

    S = property(lambda self: self.pool.S)
    capacity_chunks = property(lambda self: self.dims[2])
    device = property(lambda self: self.pool.device)
    _chunks = property(lambda self: self.pool._chunks)
    P = property(lambda self: self.pool.P)
    Cur = property(lambda self: self.pool.Cur)
    pos = property(lambda self: self.pool.pos)
    chunk_size = property(lambda self: self.pool.chunk_size)
    stale = property(lambda self: self.pool.stale, lambda self, x: setattr(self.pool, "stale", x))
    _full = property(lambda self: self.pool._full, lambda self, x: setattr(self.pool, "_full", x))

    @property
    def rows(self) -> int:
        """B: the sequences of a call on this view."""
        return len(self.slots) if self.slots is not None else self._map.shape[0]

    @property
    def map(self) -> torch.Tensor:
        """int32 [B] on the pool's device: slot of every row -- the caller's tensor, or the copy of the list made on first use."""
        if self._map is None:
            self._map = torch.tensor(self.slots, dtype=torch.int32).to(self.pool.device)
        return self._map

    @property
    def lengths(self):
        """The pool's host mirror at the view's slots (None for a map on the device, which the host never reads)."""
        if self.slots is None:
            return None
        src = self.pool.lengths   # (a tuple, replaced whenever a length changes: its identity says whether the selection is current)
        if self._mirror[0] is not src:
            self._mirror = (src, tuple(src[s] for s in self.slots))
        return self._mirror[1]

    @lengths.setter
    def lengths(self, values):
        self.pool._set_lengths(self.slots, values)
        self._mirror = (self.pool.lengths, tuple(values))

    @property
    def seen(self) -> int:
        return self.pool.seen if self.slots is None else max(self.lengths)

    @seen.setter
    def seen(self, _):   # (the pool's `seen` follows its lengths: `_set_lengths`)
        pass

    def to_ragged(self) -> "CausalStateView":
        return self

    def sync(self) -> "CausalStateView":
        self.pool.sync()
        return self

    def _host_slots(self, fn: str):
        if self.slots is None:
            raise ValueError(f"{fn}: the view's slot map lives on the device, which only mhla_causal_step_dev takes: make the view from "
                             "a list of slots")
        self.pool._refuse_stale(fn)

    def compact(self) -> CausalState:
        """A fresh ragged `CausalState` holding COPIES of the view's slots in call order (plain tensor operations): what a call on
        the view is defined against."""
        self._host_slots("CausalStateView.compact")
        idx = self.map.to(torch.int64)
        out = CausalState(self.S[idx], self.P[idx], self.Cur[idx], 0, self.chunk_size, lengths=self.lengths, pos=self.pos[idx])
        if self.pool._full is not None:
            out._full = self.pool._full[idx]
        return out

    clone = compact

    def at(self, slots):
        raise ValueError("CausalState.at: a view of a view; take the slots from the pool")

    def reset(self, slots):
        raise ValueError("CausalState.reset: slots are reset on the pool, not on a view of it")

    def fork(self, src, dst):
        raise ValueError("CausalState.fork: slots are forked on the pool, not on a view of it")

    def __repr__(self):
        return f"CausalStateView(slots={self.slots if self.slots is not None else 'on the device'}, B={self.rows}, of {self.pool!r})"


def _state_rows(state) -> int:
    """The sequences a call on `state` has: its batch rows, or the rows a view selects."""
    return state.rows if isinstance(state, CausalStateView) else state.S.shape[0]


class PoolExhausted(RuntimeError):
    """A call on a `PagedCausalState` needs more pages than the pool has free.  Raised before anything is changed."""


def _page_table(fn, table, n_slots, n_pages):
    """`table` as n_slots lists of equally many ints in -1 .. n_pages - 1 (-1: no page); ValueError naming the offenders otherwise."""
    rows = [list(r) for r in (table.tolist() if isinstance(table, torch.Tensor) else table)]
    if len(rows) != n_slots:
        raise ValueError(f"{fn}: the table has {len(rows)} rows, the pool {n_slots} slots (one row of capacity_chunks entries per slot)")
    cap = len(rows[0])
    ragged = [s for s, r in enumerate(rows) if len(r) != cap]
    if cap < 1 or ragged:
        raise ValueError(f"{fn}: table rows {ragged or [0]} do not have the {cap} entries of row 0 (capacity_chunks >= 1 entries per slot)")
    bad = sorted({repr(p) for r in rows for p in r if isinstance(p, bool) or not isinstance(p, int)})
    if bad:
        raise ValueError(f"{fn}: table entries must be ints, got [{', '.join(bad)}]")
    out = sorted({p for r in rows for p in r if not -1 <= p < n_pages})
    if out:
        raise ValueError(f"{fn}: table entries {out} are outside -1 .. {n_pages - 1} (the pool has {n_pages} pages, -1 is no page)")
    dup = sorted({p for r in rows for p in r if p >= 0 and r.count(p) > 1})
    if dup:
        raise ValueError(f"{fn}: pages {dup} are named more than once within one slot (two chunks of a sequence never share a page)")
    return rows


class SwappedSlots:
    """What `PagedCausalState.swap_out` returns and `swap_in` takes: the state of `n_seqs` sequences lifted out of a paged pool, in one
    contiguous byte buffer (`buffer`, uint8, which it owns; the layout is the library's: mhla_hip.h, `mhla_causal_swap_ws_bytes`) --
    per sequence P, Cur, pos and full, then every finished page once (an h16 page as payload and multipliers, never decoded).
    `lengths`: tokens of every sequence; `page_format` and `dims` = (Hkv, K, V): what a pool must share to take it; `seq_pages`: per
    sequence, the blob pages of its finished chunks 0, 1, ... -- sequences that shared a page in the pool name the same blob page;
    `n_pages`, `nbytes`.  `host`: the buffer is host memory (pinned where a GPU is present), which a swap stages through the
    device; otherwise it lives on the pool's device.  The kernels that fill a blob are stream-ordered and nothing synchronises: whoever
    reads the bytes of a host blob (`buffer`, `to`) on another stream or from the host synchronises first."""

    __slots__ = ("buffer", "lengths", "page_format", "dims", "seq_pages", "n_pages", "host")

    def __init__(self, buffer, lengths, page_format, dims, seq_pages, n_pages, host):
        self.buffer, self.lengths, self.page_format, self.dims = buffer, tuple(lengths), page_format, tuple(dims)
        self.seq_pages, self.n_pages, self.host = tuple(tuple(r) for r in seq_pages), int(n_pages), bool(host)

    n_seqs = property(lambda self: len(self.lengths))
    nbytes = property(lambda self: self.buffer.numel())
    device = property(lambda self: self.buffer.device)

    @staticmethod
    def _buffer(nbytes: int, device, host: bool) -> torch.Tensor:
        if host:   # (pinned, so that the copies of a swap are asynchronous; a machine without a GPU -- a recorded session -- has nothing to pin for)
            return torch.empty(nbytes, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        return torch.empty(nbytes, dtype=torch.uint8, device=device)

    def to(self, device) -> "SwappedSlots":
        """A copy of the blob on `device` ("cpu": pinned host memory), stream-ordered on the current stream."""
        device = torch.device(device)
        buf = self._buffer(self.nbytes, device, device.type == "cpu")
        buf.copy_(self.buffer, non_blocking=True)
        return SwappedSlots(buf, self.lengths, self.page_format, self.dims, self.seq_pages, self.n_pages, device.type == "cpu")

    def __repr__(self):
        Hkv, K, V = self.dims
        return (f"SwappedSlots(lengths={self.lengths}, n_pages={self.n_pages}, page_format={self.page_format}, Hkv={Hkv}, K={K}, V={V}, "
                f"nbytes={self.nbytes}, {'host' if self.host else self.buffer.device})")


class PagedCausalState(CausalState):
    """A pool of decode slots whose FINISHED CHUNKS ARE PAGES: `pages [n_pages, Hkv, K, V]` (fp32; one page holds K_j^T V_j of one chunk
    of one sequence, all k/v heads) and, per slot, a page table of `capacity_chunks` entries -- `table` on the host (lists of ints, -1:
    no page) and `table_dev` (int32 [n_slots, capacity_chunks]) for the kernels.  `P`, `Cur` `[n_slots, Hkv, K, V]`, `pos`, `full`,
    `lengths` and `stale` are those of a dense ragged pool (`CausalState`); there is no dense `S` (None).  A dense pool reserves
    `capacity_chunks` chunks per slot whatever the requests' lengths; this one costs memory for the tokens it holds, and slots share
    finished pages by reference count (`refs`), so that `fork` copies no chunk.  Always ragged.
    Calls go through `pool.at(slots)`, a `PagedStateView`, which every call that takes a `CausalStateView` takes (the library's
    `*_paged` entry points); each gives bit for bit what the un-slotted call gives on `view.compact()`.  The pool itself is refused
    where a state is expected.
    Page rule: before its launch a host-positioned call (step, extend, verify, commit, pack prefill `into=`) gives a page to every
    chunk that holds a token of the slot afterwards, chunks 0 .. ceil(n_after / 64) - 1, lowest free page first.  All or nothing:
    `PoolExhausted` before anything changes when the free list is too short.  Changed rows of the table go to `table_dev` with a
    stream-ordered copy (no synchronisation).  `mhla_causal_step_dev` never assigns: `reserve(slots, tokens)` applies the rule ahead
    of it, and a sequence that reaches a chunk without a page is frozen like one at the capacity (`full`, `sync()`).
    Swapping: `swap_out(slots, device)` lifts the state of slots -- finished pages (a shared one once), P, Cur, pos, full -- into one
    contiguous `SwappedSlots` blob, in pinned host memory (preemption) or on the device, and `swap_in(blob, slots)` puts it back bit
    for bit into empty slots of this or another pool of the same Hkv, K, V and page format, by the page rule.  The pool never evicts on
    its own: swapping is the caller's decision, and `PoolExhausted` is still raised before anything changes.
    Through a model: `modules.PagedDecodeCache` holds one fp32 pool per layer, and the fla layer and `hosts/gpt.py` run packed scheduler
    steps on it.  Not covered: `DecodeCache` keeps states of its own; dense pools have no swap.
    Page format `"h16"` (`empty(..., page_format="h16")`, or a float16 `pages` together with `page_mult [n_pages, Hkv, K V / 64]`,
    float32): a page takes 2 bytes an element -- an fp16 payload times one power-of-two multiplier per 64 adjacent elements of a
    head's flattened `[K, V]` chunk (K V % 64 == 0), 11 significand bits relative to the group's largest element: the precision of
    the forward's default chunk summaries -- so the pool holds 1.94 times the tokens in the same memory.  A finished chunk is written,
    and so rounded, once; `P` and `Cur` stay fp32.  The chunk a sequence finishes with is the fp32 pool's, bit for bit, and its page
    the encoding of it; every prefix mix sums DECODED pages, so `P` is a function of the pages alone and a prefilled slot holds
    the bits of one stepped to the same tokens.  `mhla_causal_step`, `mhla_causal_step_dev` and the pack prefill `into=` take a view
    of such a pool (the library's `*_paged_h16` entry points); `mhla_causal_extend`, `mhla_causal_verify` and `mhla_causal_commit`
    raise NotImplementedError before anything is launched or any page assigned.  `compact()` decodes into the usual fp32 state.
    The page rule, `reserve`, `fork`, `trim`, `reset` and `PoolExhausted` do not depend on the format."""

    __slots__ = ("pages", "page_mult", "table", "table_dev", "refs", "free", "have")
    _sync_cause = " or onto a chunk that has no page (pool.reserve(slots, tokens) assigns them)"

    def __init__(self, pages: torch.Tensor, P: torch.Tensor, Cur: torch.Tensor, table, *, lengths=None, chunk_size: int = 64,
                 page_mult: Optional[torch.Tensor] = None):
        fn = "PagedCausalState"
        if pages.dim() != 4 or P.dim() != 4 or tuple(P.shape[1:]) != tuple(pages.shape[1:]) or P.shape != Cur.shape:
            raise ValueError(f"{fn}: pages [n_pages, Hkv, K, V] and P, Cur [n_slots, Hkv, K, V], got {tuple(pages.shape)}, {tuple(P.shape)}, "
                             f"{tuple(Cur.shape)}")
        h16 = page_mult is not None or pages.dtype == torch.float16
        if h16:
            self._check_h16(fn, pages, page_mult)
        if any(t.dtype != torch.float32 or t.device != pages.device or not t.is_contiguous() for t in ((P, Cur) if h16 else (pages, P, Cur))):
            raise ValueError(f"{fn}: pages, P and Cur must be contiguous float32 tensors on one device")
        n_slots, n_pages = P.shape[0], pages.shape[0]
        if min(n_slots, n_pages) < 1:
            raise ValueError(f"{fn}: n_slots={n_slots} and n_pages={n_pages} must be positive")
        rows = _page_table(fn, table, n_slots, n_pages)
        lengths = _int_tuple(fn, "lengths", (0,) * n_slots if lengths is None else lengths, n_slots, None)
        over = [s for s, n in enumerate(lengths) if n > 64 * len(rows[0])]
        if over:
            raise IndexError(f"{fn}: slots {over} (lengths {lengths}) exceed the capacity of {len(rows[0])} chunks")
        bare = {s: [j for j in range(-(-n // 64)) if rows[s][j] < 0] for s, n in enumerate(lengths)}
        bare = {s: js for s, js in bare.items() if js}
        if bare:
            raise ValueError(f"{fn}: slots {sorted(bare)} hold tokens in chunks that have no page: {bare} (lengths {lengths})")
        self.S, self.P, self.Cur, self.chunk_size, self.pages, self.page_mult = None, P, Cur, int(chunk_size), pages, page_mult
        self.lengths, self.seen, self.stale, self._full = lengths, max(lengths), False, None
        self.pos = torch.tensor(lengths, dtype=torch.int32, device=pages.device)
        self.table = rows
        self.refs = [0] * n_pages
        for r in rows:
            for p in r:
                if p >= 0:
                    self.refs[p] += 1
        self.free = [p for p in range(n_pages) if not self.refs[p]]   # (a heap: the lowest free page goes first)
        self.have = [self._leading(r) for r in rows]   # per slot: its leading chunks that have pages -- the page rule's quick test
        self.table_dev = torch.tensor(rows, dtype=torch.int32, device=pages.device)

    @staticmethod
    def _check_h16(fn, pages, page_mult):
        """h16 pages: a contiguous float16 payload with its multipliers, one per 64 elements of a head's chunk."""
        n_pages, Hkv, K, V = pages.shape
        if (K * V) % 64:
            raise ValueError(f"{fn}: h16 pages need K V % 64 == 0 (one multiplier per 64 elements of a head's [K, V] chunk), got K={K} V={V}")
        if pages.dtype != torch.float16 or page_mult is None or page_mult.dtype != torch.float32 or tuple(page_mult.shape) != (n_pages, Hkv, K * V // 64):
            raise ValueError(f"{fn}: h16 pages are a float16 `pages` [n_pages, Hkv, K, V] together with a float32 `page_mult` "
                             f"[n_pages, Hkv, K V / 64] = {(n_pages, Hkv, K * V // 64)}, got {pages.dtype} and "
                             + ("no page_mult" if page_mult is None else f"{page_mult.dtype} {tuple(page_mult.shape)}"))
        if page_mult.device != pages.device or not (pages.is_contiguous() and page_mult.is_contiguous()):
            raise ValueError(f"{fn}: pages and page_mult must be contiguous tensors on one device")

    @classmethod
    def empty(cls, n_slots: int, Hkv: int, K: int, V: int, capacity_chunks: int, n_pages: int, device="cuda",
              page_format: str = "fp32") -> "PagedCausalState":
        if min(n_slots, Hkv, K, V, capacity_chunks, n_pages) <= 0:
            raise ValueError(f"PagedCausalState.empty: non-positive size n_slots={n_slots} Hkv={Hkv} K={K} V={V} "
                             f"capacity_chunks={capacity_chunks} n_pages={n_pages}")
        if page_format not in ("fp32", "h16"):
            raise ValueError(f"PagedCausalState.empty: page_format {page_format!r}: 'fp32' or 'h16'")
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
        table = [[-1] * capacity_chunks for _ in range(n_slots)]
        if page_format == "h16":
            if (K * V) % 64:
                raise ValueError(f"PagedCausalState.empty: h16 pages need K V % 64 == 0, got K={K} V={V}")
            return cls(torch.zeros(n_pages, Hkv, K, V, dtype=torch.float16, device=device), z(n_slots, Hkv, K, V), z(n_slots, Hkv, K, V), table,
                       page_mult=z(n_pages, Hkv, K * V // 64))
        return cls(z(n_pages, Hkv, K, V), z(n_slots, Hkv, K, V), z(n_slots, Hkv, K, V), table)

    @property
    def page_format(self) -> str:
        return "fp32" if self.page_mult is None else "h16"

    dims = property(lambda self: (self.P.shape[0], self.P.shape[1], len(self.table[0]), self.P.shape[2], self.P.shape[3]))
    capacity_chunks = property(lambda self: len(self.table[0]))
    device = property(lambda self: self.pages.device)
    _chunks = property(lambda self: self.pages)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size()
                   for t in (self.pages, self.page_mult, self.P, self.Cur, self.pos, self._full, self.table_dev) if t is not None)

    @property
    def pages_free(self) -> int:
        return len(self.free)

    @property
    def pages_used(self) -> int:
        return len(self.refs) - len(self.free)

    def at(self, slots) -> "PagedStateView":
        """The slots `slots` of the pool as a state of `len(slots)` sequences on the same storage: `CausalState.at`, paged."""
        return PagedStateView(self, slots)

    def to_ragged(self) -> "PagedCausalState":
        return self

    def clone(self):
        raise ValueError("PagedCausalState.clone: a paged pool is not copied as a whole; pool.at(slots).compact() copies slots")

    # ---- pages
    def _release(self, page: int):
        self.refs[page] -= 1
        if not self.refs[page]:
            heapq.heappush(self.free, page)

    @staticmethod
    def _leading(row) -> int:
        return next((j for j, p in enumerate(row) if p < 0), len(row))

    def _push(self, slots):
        """Rows `slots` of the host table, which changed, to `table_dev`: one small stream-ordered copy per row, no synchronisation."""
        for s in slots:
            self.have[s] = self._leading(self.table[s])
            self.table_dev[s].copy_(torch.tensor(self.table[s], dtype=torch.int32), non_blocking=True)

    def _assign(self, fn: str, slots, n_after, fresh: bool = False):
        """The page rule for the slots `slots`: a page for every chunk 0 .. ceil(n_after[b] / 64) - 1 of slot b that has none.  fresh
        (a prefill): the slot starts anew, its pages are released first (a shared one stays with its other holders).  All or nothing."""
        have = self.have
        if not fresh and all(n <= 64 * have[s] for s, n in zip(slots, n_after)):   # (the usual call: every page is there)
            return
        cap = self.capacity_chunks
        want = [min(cap, -(-int(n) // 64)) for n in n_after]
        released = 0
        if fresh:
            gone = [p for s in slots for p in self.table[s] if p >= 0]
            released = sum(1 for p in set(gone) if self.refs[p] == gone.count(p))
            missing = {s: list(range(w)) for s, w in zip(slots, want) if w}
        else:
            missing = {s: [j for j in range(w) if self.table[s][j] < 0] for s, w in zip(slots, want)}
            missing = {s: js for s, js in missing.items() if js}
        need = sum(len(js) for js in missing.values())
        if need > len(self.free) + released:
            raise PoolExhausted(f"{fn}: slots {sorted(missing)} need {need} more pages, the pool has {len(self.free) + released} free "
                                f"(of {len(self.refs)}; pool.trim / pool.reset release pages)")
        changed = set(missing)
        if fresh:
            for s in slots:
                for j, p in enumerate(self.table[s]):
                    if p >= 0:
                        self._release(p)
                        self.table[s][j] = -1
                        changed.add(s)
        for s, js in missing.items():
            for j in js:
                p = heapq.heappop(self.free)
                self.refs[p] = 1
                self.table[s][j] = p
        if changed:
            self._push(sorted(changed))

    def reserve(self, slots, tokens) -> "PagedCausalState":
        """Pages for the first `tokens` tokens (an int, or one per slot) of every slot of `slots`, by the page rule -- what a caller of
        `mhla_causal_step_dev`, which never assigns pages, does ahead of the steps.  It reads the table alone, not the positions, so a
        stale pool is fine.  IndexError beyond the capacity; `PoolExhausted` before anything changes."""
        fn = "PagedCausalState.reserve"
        slots = _slot_tuple(fn, slots, self.dims[0])
        tokens = _int_tuple(fn, "tokens", (tokens,) * len(slots) if isinstance(tokens, int) else tokens, len(slots), None)
        over = [s for s, n in zip(slots, tokens) if n > 64 * self.capacity_chunks]
        if over:
            raise IndexError(f"{fn}: slots {over} would hold more than the capacity of {self.capacity_chunks} chunks "
                             f"({64 * self.capacity_chunks} tokens)")
        self._assign(fn, slots, tokens)
        return self

    def trim(self, slots) -> "PagedCausalState":
        """Release the pages of every slot of `slots` beyond its ceil(length / 64) chunks, for instance after a commit that accepted less
        than was verified."""
        slots = self._pool_slots("PagedCausalState.trim", slots)
        changed = []
        for s in slots:
            for j in range(-(-self.lengths[s] // 64), self.capacity_chunks):
                if self.table[s][j] >= 0:
                    self._release(self.table[s][j])
                    self.table[s][j] = -1
                    changed.append(s)
        self._push(sorted(set(changed)))
        return self

    def reset(self, slots) -> "PagedCausalState":
        """Empty the slots `slots` for new requests: every page they hold is released (a shared one stays with its other holders), P,
        Cur, pos, full and the host mirror of those rows become zero."""
        slots = self._pool_slots("PagedCausalState.reset", slots)
        self._set_lengths(slots, (0,) * len(slots))
        self.trim(slots)
        idx = torch.tensor(slots, dtype=torch.int64).to(self.device)
        for t in (self.P, self.Cur, self.pos, self._full):
            if t is not None:
                t[idx] = 0
        return self

    def fork(self, src: int, dst: int) -> "PagedCausalState":
        """Slot `dst` becomes a copy of slot `src` (a shared prompt prefix, beams) without copying a chunk: `dst`'s pages are released,
        then it SHARES `src`'s pages of finished chunks (`length // 64` of them, reference count + 1); P, Cur, pos, full and the host
        mirror are copied.  A finished chunk is never written again, so both go on independently."""
        src, dst = self._pool_slots("PagedCausalState.fork", (src, dst))
        n = self.lengths[src]
        self._set_lengths((dst,), (0,))
        self.trim((dst,))
        for j in range(n // 64):
            p = self.table[src][j]
            self.refs[p] += 1
            self.table[dst][j] = p
        self._push((dst,))
        for t in (self.P, self.Cur, self.pos, self._full):
            if t is not None:
                t[dst] = t[src]
        self._set_lengths((dst,), (n,))
        return self

    # ---- swapping: the caller's decision, never the pool's
    def swap_out(self, slots, device="cpu", release: bool = True) -> "SwappedSlots":
        """Lift the state of the slots `slots` out of the pool into a `SwappedSlots` blob on `device`: "cpu" (pinned host memory:
        preemption; staged through a device buffer of at most `SWAP_STAGE_CAP_BYTES` in slices of whole items) or the pool's own
        device (also: None), for a migration into another pool or a compaction.  Per slot, in call order: its `length // 64` finished
        pages -- a page that several of the slots share after a `fork` once --, P, Cur, pos and full.  Pages beyond the finished chunks
        (the open chunk's, pages from `reserve`, a verify's scratch) are not saved: their content is outside the state's contract.
        release=True: the slots are then emptied exactly as `reset` empties them (a page shared with a slot that stays loses one
        reference); release=False: the pool keeps every bit -- a snapshot.  Everything is enqueued on the current stream and nothing
        synchronises: synchronise before the host reads the bytes of a host blob.  The pool must be host-positioned and not stale."""
        fn = "PagedCausalState.swap_out"
        slots = self._pool_slots(fn, slots)
        host = device is not None and torch.device(device).type == "cpu"
        device = self.device if device is None else torch.device(device)
        if not host and device != self.device and (device.index is not None or device.type != self.device.type):
            raise ValueError(f"{fn}: device {device}: 'cpu' or the pool's device {self.device} (SwappedSlots.to(device) copies a blob anywhere)")
        seq_pages, blob_page = [], {}   # (pool page -> blob page, in order of first use)
        for s in slots:
            seq_pages.append([blob_page.setdefault(self.table[s][j], len(blob_page)) for j in range(self.lengths[s] // 64)])
        Hkv, K, V = self.dims[1], self.dims[3], self.dims[4]
        nbytes = _swap_bytes(len(slots), len(blob_page), Hkv, K, V, self.page_format)
        blob = SwappedSlots(SwappedSlots._buffer(nbytes, self.device, host), [self.lengths[s] for s in slots], self.page_format, (Hkv, K, V),
                            seq_pages, len(blob_page), host)
        _swap_launch("out", self, blob, list(slots) + list(blob_page))
        if release:
            self.reset(slots)
        return blob

    def swap_in(self, blob: "SwappedSlots", slots) -> "PagedCausalState":
        """Put the sequences of `blob` into the EMPTY slots `slots` (as many as it has sequences; length 0 and no page in the table
        row, ValueError naming the others) of this pool -- any pool with the blob's Hkv, K, V and page format (ValueError), whatever its
        n_slots, n_pages and capacity (IndexError for a sequence beyond 64 capacity_chunks).  Page rule: every sequence gets
        ceil(length / 64) pages, lowest free page first; a blob page that several sequences hold gets ONE pool page, its reference
        count their number.  All or nothing: `PoolExhausted` before anything changes.  Then the changed table rows go to `table_dev`,
        the scatter writes the finished pages, P, Cur, pos and full -- bit for bit what `swap_out` read -- and the host mirror follows.
        A host blob is staged through the device in slices; a blob may be swapped in more than once (a `fork` across pools).  Stream-
        ordered, no synchronisation."""
        fn = "PagedCausalState.swap_in"
        if not isinstance(blob, SwappedSlots):
            raise TypeError(f"{fn}: blob must be the SwappedSlots of a swap_out, got {type(blob).__name__}")
        slots = self._pool_slots(fn, slots)
        if len(slots) != blob.n_seqs:
            raise ValueError(f"{fn}: {len(slots)} slots for the {blob.n_seqs} sequences of the blob")
        mine = (self.dims[1], self.dims[3], self.dims[4])
        if blob.dims != mine or blob.page_format != self.page_format:
            raise ValueError(f"{fn}: the blob holds (Hkv, K, V) = {blob.dims}, page_format={blob.page_format!r}; the pool "
                             f"{mine}, page_format={self.page_format!r} (nothing is converted on the way)")
        if not blob.host and blob.buffer.device != self.device:
            raise ValueError(f"{fn}: the blob lives on {blob.buffer.device}, the pool on {self.device}: blob.to(device) copies it")
        busy = [s for s in slots if self.lengths[s] or any(p >= 0 for p in self.table[s])]
        if busy:
            raise ValueError(f"{fn}: slots {busy} are not empty (length 0 and no page: pool.reset(slots) empties them)")
        cap = self.capacity_chunks
        over = [s for s, n in zip(slots, blob.lengths) if n > 64 * cap]
        if over:
            raise IndexError(f"{fn}: slots {over} would hold more than the capacity of {cap} chunks ({64 * cap} tokens; lengths {blob.lengths})")
        need = blob.n_pages + sum(-(-n // 64) - n // 64 for n in blob.lengths)   # (shared pages once, and a page for every open chunk)
        if need > len(self.free):
            raise PoolExhausted(f"{fn}: slots {sorted(slots)} need {need} pages, the pool has {len(self.free)} free (of {len(self.refs)}; "
                                "pool.trim / pool.reset release pages)")
        placed = {}   # blob page -> pool page
        for s, n, row in zip(slots, blob.lengths, blob.seq_pages):
            for j in range(-(-n // 64)):
                b = row[j] if j < len(row) else None   # (None: the open chunk's page, which holds nothing yet)
                if b in placed:
                    p = placed[b]
                    self.refs[p] += 1
                else:
                    p = heapq.heappop(self.free)
                    self.refs[p] = 1
                    if b is not None:
                        placed[b] = p
                self.table[s][j] = p
        self._push([s for s, n in zip(slots, blob.lengths) if n])
        self.full   # (the scatter restores the flags)
        _swap_launch("in", self, blob, list(slots) + [placed[b] for b in range(blob.n_pages)])
        self._set_lengths(slots, blob.lengths)
        return self

    def __repr__(self):
        n_slots, H, cap, K, V = self.dims
        return (f"PagedCausalState(n_slots={n_slots}, H={H}, K={K}, V={V}, capacity_chunks={cap}, pages={self.pages_used}/{len(self.refs)} used, "
                + ("" if self.page_mult is None else "page_format=h16, ") + f"lengths={self.lengths}, device={self.device})")


class PagedStateView(CausalStateView):
    """`paged_pool.at(slots)`: a `CausalStateView` of a `PagedCausalState`.  Everything said there holds; the finished chunks are read
    and written through the pool's page table (the library's `*_paged` entry points), and `compact()` gathers them into an ordinary
    dense ragged `CausalState` -- what every call on the view is defined against, bit for bit.  There is no dense `S`."""

    __slots__ = ()

    @property
    def S(self):
        raise AttributeError("a view of a PagedCausalState has no dense S: pool.pages and pool.table hold the finished chunks, "
                             "view.compact() gathers them")

    table_dev = property(lambda self: self.pool.table_dev)
    page_mult = property(lambda self: self.pool.page_mult)

    def compact(self) -> CausalState:
        """A fresh dense ragged `CausalState` holding COPIES of the view's slots in call order, each chunk gathered from its page
        (zeros where the table names none), h16 pages decoded (payload x multiplier, exact in fp32): plain tensor operations."""
        self._host_slots("PagedStateView.compact")
        pool = self.pool
        idx = self.map.to(torch.int64)
        tab = torch.tensor([pool.table[s] for s in self.slots], dtype=torch.int64).to(pool.device)   # [B, cap]
        S = pool.pages[tab.clamp_min(0)]   # [B, cap, H, K, V]
        if pool.page_mult is not None:
            m = pool.page_mult[tab.clamp_min(0)]   # [B, cap, H, K V / 64]
            S = (S.float().reshape(*m.shape, 64) * m[..., None]).reshape(S.shape)
        S[tab < 0] = 0
        out = CausalState(S.permute(0, 2, 1, 3, 4).contiguous(), pool.P[idx], pool.Cur[idx], 0, self.chunk_size, lengths=self.lengths,
                          pos=pool.pos[idx])
        if pool._full is not None:
            out._full = pool._full[idx]
        return out

    clone = compact

    def __repr__(self):
        return f"PagedStateView(slots={self.slots if self.slots is not None else 'on the device'}, B={self.rows}, of {self.pool!r})"


def _refuse_paged_pool(fn, state):
    if isinstance(state, PagedCausalState):
        raise TypeError(f"{fn}: a PagedCausalState is a pool, not a state: pass pool.at(slots), the view of the slots the call works on")


def _refuse_h16(fn, state):
    """What has no form on h16 pages, refused before anything is launched or any page is assigned: a verify uses the rows of S beyond
    the finished chunks as scratch and reads them back, which rounded pages would change."""
    if state.page_mult is not None:
        raise NotImplementedError(f"{fn}: the pool's pages are h16 (page_format='h16'): mhla_causal_step, mhla_causal_step_dev and the pack "
                                  "prefill (mhla_causal_state(..., into=view)) run on them; extend, verify and commit need an fp32 pool")


def _page_rule(fn, state, counts):
    """The page rule of a host-positioned call that adds `counts[b]` tokens to sequence b of a view of a paged pool
    (`PagedCausalState`): after every refusal, before the first launch.  Any other state (`state.pages is None`, which the callers
    on a hot path test themselves): nothing."""
    if state.pages is not None:
        state.pool._assign(fn, state.slots, [p + n for p, n in zip(state.lengths, counts)])


def _int_tuple(fn, name, xs, B, hi):
    """`xs` (a list or a tensor; reading a device tensor synchronises) as B ints in 0 .. hi: the `lengths` of a ragged state (its
    host mirror; `hi` = T, or None for no upper bound), the `counts` of a call (T), the `accept` of a commit (`hi`: the draft's
    counts, a tuple -- one bound per sequence)."""
    xs = tuple(int(n) for n in (xs.tolist() if isinstance(xs, torch.Tensor) else xs))
    per_seq = isinstance(hi, tuple)
    if len(xs) != B:
        raise ValueError(f"{fn}: {name} has {len(xs)} entries, " + (f"the draft B={B}" if per_seq else f"expected B={B}"))
    if any(n < 0 or n > h for n, h in zip(xs, hi)) if per_seq else B and (min(xs) < 0 or (hi is not None and max(xs) > hi)):
        raise ValueError(f"{fn}: {name}={xs} must be in 0 .." + ("" if hi is None else f" counts={hi} of the draft" if per_seq else f" T={hi}"))
    return xs


def _runs(lengths, nb):
    """(first, end, length) of every run of adjacent sequences with equal length, none longer than `nb` sequences."""
    i = 0
    while i < len(lengths):
        j = i + 1
        while j < len(lengths) and j - i < nb and lengths[j] == lengths[i]:
            j += 1
        yield i, j, lengths[i]
        i = j


class _StateRows:
    """Rows [i, j) of a state as a launch takes them -- the one form for every kind.  A state of its own: views of S, P, Cur and no
    slot map.  A view of a pool, dense or paged: the pool's tensors whole and that piece of the view's slot map."""

    __slots__ = ("S", "pages", "page_mult", "table_dev", "P", "Cur", "chunk_size", "map", "dims")

    def __init__(self, state, i, j):
        pool = getattr(state, "pool", None)
        self.chunk_size, self.dims = state.chunk_size, state.dims
        if pool is None:
            self.S, self.P, self.Cur, self.map = state.S[i:j], state.P[i:j], state.Cur[i:j], None
            self.pages = self.page_mult = self.table_dev = None
        else:
            self.S, self.P, self.Cur, self.map = pool.S, pool.P, pool.Cur, state.map[i:j]
            self.pages, self.page_mult, self.table_dev = pool.pages, pool.page_mult, getattr(pool, "table_dev", None)


def _rows_of(state, i, j, *along):
    """What one launch chain takes of a call's per-sequence objects when it serves sequences [i, j) only: (`_StateRows`, x[i:j] for
    every x of `along`).  A view of a pool: its slot map is sliced with the tokens, while the pool's `pos` and `full`, which the
    launches address through the map, pass whole."""
    pooled = (state.pos, state._full) if isinstance(state, CausalStateView) else ()
    return (_StateRows(state, i, j),) + tuple(x if any(x is t for t in pooled) else x[i:j] for x in along)


def _batch_slices(state: CausalState, nb, prepared=None, *along):
    """One launch addresses `nb` sequences (`_MAX_GRID_BH // H`; batches beyond that range: see mhla_blockmix).  Yields, for every
    batch slice [i, j) of at most `nb`: (`_StateRows`, `prepared.part(i, j)`, x[i:j] for every x of `along`: `_rows_of`).  B <= nb,
    the usual case, is one launch chain on the objects themselves."""
    B = _state_rows(state)
    if B <= nb:
        yield (state, prepared) + along
        return
    for i in range(0, B, nb):
        j = min(B, i + nb)
        rows = _rows_of(state, i, j, *along)
        yield (rows[0], prepared.part(i, j) if prepared is not None else None) + rows[1:]


def _run_slices(state: CausalState, lengths, nb):
    """`_batch_slices` cut further where adjacent lengths differ: (i, j, the length, the state's rows) of every run of `_runs`; a run
    that is the whole batch: the state itself."""
    for i, j, n in _runs(lengths, nb):
        yield i, j, n, state if j - i == len(lengths) else _StateRows(state, i, j)


# The library's entry point for every kind of decode call (the key) by the kind of state: a state of its own, a view of a dense pool,
# of a pool of fp32 pages, of a pool of h16 pages (None: there is none, and the call was refused on its way here).  Last, how the first
# takes the heads: H alone (False), H alone with a grouped-query twin `_gqa` that takes H, Hkv (True: `_gqa_call` picks), or H, Hkv
# like every entry point for a view (None).
_ENTRY = {
    "state_init": ("mhla_causal_state_init", None, None, None, False),
    "prefill": ("mhla_causal_varlen_state_init", "mhla_causal_varlen_state_init_slots", "mhla_causal_varlen_state_init_paged",
                "mhla_causal_varlen_state_init_paged_h16", False),
    "step_uniform": ("mhla_causal_step", None, None, None, False),
    "extend_uniform": ("mhla_causal_extend", None, None, None, False),
    "step": ("mhla_causal_step_ragged", "mhla_causal_step_slots", "mhla_causal_step_paged", "mhla_causal_step_paged_h16", True),
    "step_dev": ("mhla_causal_step_dev", "mhla_causal_step_dev_slots", "mhla_causal_step_dev_paged", "mhla_causal_step_dev_paged_h16", True),
    "extend": ("mhla_causal_extend_ragged", "mhla_causal_extend_slots", "mhla_causal_extend_paged", None, True),
    "verify": ("mhla_causal_verify_ragged", "mhla_causal_verify_slots", "mhla_causal_verify_paged", None, True),
    "commit": ("mhla_causal_commit_ragged", "mhla_causal_commit_slots", "mhla_causal_commit_paged", None, False),
    "extend_packed": ("mhla_causal_extend_packed", "mhla_causal_extend_packed", "mhla_causal_extend_packed", None, None),
    "verify_packed": ("mhla_causal_verify_packed", "mhla_causal_verify_packed", "mhla_causal_verify_packed", None, None),
    "commit_packed": ("mhla_causal_commit_packed", "mhla_causal_commit_packed", "mhla_causal_commit_packed", None, False),
}


def _state_args(call, mixf, state, pos=(), packed=False):
    """The one place that tells the kinds of state apart for the library: (the entry point of `call`, a key of `_ENTRY`, for this
    state; how it takes the heads, `_ENTRY`'s last column; the state's part of its argument list, in its order).  `state`: a state,
    a view, or `_StateRows` of either.  `pos`: what the entry point takes between Cur and the slot map, its positions last.
    Padded:  mix, ldmix, S | pages, n_pages, table | pages, page_mult, n_pages, table; capacity, P, Cur, *pos; a view: slot map, n_slots.
    Packed (one entry point for every kind): mix, ldmix, S, 0, null | pages, n_pages, table; capacity, P, Cur, *pos, slot map | null, n_slots | 0."""
    row = _ENTRY[call]
    slot = getattr(state, "map", None)
    if slot is None:   # (a state of its own, the usual call, spelt out: this is on the path of every step)
        S = state.S
        if packed:
            return row[0], None, (mixf.data_ptr(), mixf.shape[1], S.data_ptr(), 0, None, S.shape[2], state.P.data_ptr(), state.Cur.data_ptr(), *pos, None, 0)
        return row[0], row[4], (mixf.data_ptr(), mixf.shape[1], S.data_ptr(), S.shape[2], state.P.data_ptr(), state.Cur.data_ptr(), *pos)
    pages, mult = state.pages, state.page_mult
    if pages is None:
        name, chunks = row[1], (state.S.data_ptr(), 0, None) if packed else (state.S.data_ptr(),)
    elif mult is None:
        name, chunks = row[2], (pages.data_ptr(), pages.shape[0], state.table_dev.data_ptr())
    else:   # (h16 pages: the multipliers follow the payload)
        name, chunks = row[3], (pages.data_ptr(), mult.data_ptr(), pages.shape[0], state.table_dev.data_ptr())
    dims = state.dims
    return name, None, (mixf.data_ptr(), mixf.shape[1], *chunks, dims[2], state.P.data_ptr(), state.Cur.data_ptr(), *pos, slot.data_ptr(), dims[0])


@functools.lru_cache(maxsize=64)
def _step_ws_bytes(B, H, K, V, dt):
    return _lib.load().mhla_causal_step_ws_bytes(B, H, K, V, dt)


@functools.lru_cache(maxsize=64)
def _swap_bytes(n_seqs, n_pages, Hkv, K, V, page_format):
    """Bytes of a blob of `n_seqs` sequence items and `n_pages` page items: the library's layout (pure host arithmetic)."""
    return _lib.load().mhla_causal_swap_ws_bytes(n_seqs, n_pages, Hkv, K, V, 1 if page_format == "h16" else 0)


def _swap_launch(direction, pool, blob, items):
    """Both directions of a swap ("out": pool -> blob, "in": blob -> pool): the one place that marshals a paged pool and an item list
    (`items`: the pool slot of every sequence of the blob, then the pool page of every blob page) for mhla_causal_swap_{out,in}_paged.
    The list goes to the device in one small copy.  A blob on the pool's device: one call on the whole list, on the blob itself.  A
    host blob: the list is cut into slices of whole items whose bytes fit a device staging buffer of at most `SWAP_STAGE_CAP_BYTES`
    (one item, where a single item is larger), reused across the slices -- stream order makes that safe --, each slice gathered into
    the stage and copied to the blob, or copied to the stage and scattered; nothing synchronises."""
    fn = getattr(_lib.load(), f"mhla_causal_swap_{direction}_paged")
    Hkv, K, V = blob.dims
    n_seqs, n_moved = blob.n_seqs, blob.n_pages
    seq_b, page_b = (_swap_bytes(*n, Hkv, K, V, blob.page_format) for n in ((1, 0), (0, 1)))
    at = lambda i: i * seq_b if i < n_seqs else n_seqs * seq_b + (i - n_seqs) * page_b   # where item i begins
    items_dev = torch.tensor(items, dtype=torch.int32).to(pool.device)
    head = (pool.pages.data_ptr(), _ptr(pool.page_mult), pool.pages.shape[0], pool.P.data_ptr(), pool.Cur.data_ptr(), pool.pos.data_ptr(),
            _ptr(pool._full), pool.dims[0], items_dev.data_ptr(), n_seqs, n_moved)
    what = f"mhla_causal_swap_{direction}_paged"
    if not blob.host:
        _lib.check(fn(*head, 0, len(items), blob.buffer.data_ptr(), Hkv, K, V, _stream()), what)
        return
    cuts = [0]
    for i in range(1, len(items) + 1):   # (greedy: a slice grows while its bytes fit the cap, and holds at least one item)
        if at(i) - at(cuts[-1]) > SWAP_STAGE_CAP_BYTES and i - 1 > cuts[-1]:
            cuts.append(i - 1)
    cuts.append(len(items))
    stage = torch.empty(max(at(j) - at(i) for i, j in zip(cuts, cuts[1:])), dtype=torch.uint8, device=pool.device)
    for i, j in zip(cuts, cuts[1:]):
        piece, staged = blob.buffer[at(i):at(j)], stage[:at(j) - at(i)]
        if direction == "in":
            staged.copy_(piece, non_blocking=True)
        _lib.check(fn(*head, i, j, stage.data_ptr(), Hkv, K, V, _stream()), what)
        if direction == "out":
            piece.copy_(staged, non_blocking=True)


def _gqa_call(lib, name, H, Hkv):
    """(entry point, its head arguments) of a ragged decode call: `name` itself with H, or -- k, v and the state having fewer heads
    than q -- its grouped form `name_gqa` with H, Hkv."""
    return (getattr(lib, name), (H,)) if Hkv == H else (getattr(lib, name + "_gqa"), (H, Hkv))


def _extend_ragged_ws_bytes(lib, B, T, H, Hkv, K, V, max_later, dt):
    if Hkv == H:
        return lib.mhla_causal_extend_ragged_ws_bytes(B, T, H, K, V, max_later, dt)
    return lib.mhla_causal_extend_ragged_gqa_ws_bytes(B, T, H, Hkv, K, V, max_later, dt)


@_device_guard
def _causal_state_init(k, v, mix, state: CausalState):
    lib = _lib.load()
    B, T, H, K = k.shape
    k, v = _prep(k), _prep(v)
    mixf = _mix2d(mix)
    name, _, head = _state_args("state_init", mixf, state)
    rc = getattr(lib, name)(_view(k), _view(v), *head, B, T, H, K, v.shape[-1], state.chunk_size, _dtype_code(k), _stream())
    _lib.check(rc, name)


def mhla_causal_prefill(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mixing_matrix: torch.Tensor, chunk_size: int = 64,
                        scale: Optional[float] = None, *, summaries: str = "tf32", capacity_chunks: Optional[int] = None,
                        lengths=None, left_padded: bool = False, cu_seqlens=None, into=None):
    """`(o, state)`: `o = mhla_causal(q, k, v, mixing_matrix, chunk_size, scale, summaries=summaries)` and the `CausalState`
    after these T tokens, from which `mhla_causal_step` continues one token at a time (T = 0: an empty state).  The state is
    built from k, v in exact fp32 products, independently of `summaries`; no autograd passes through it.
    capacity_chunks: chunks the state can hold (64 tokens each), default and at most the rows L of the mixing matrix.
    lengths, left_padded: a padded batch, as `mhla_causal_state` takes it -- the state is ragged, every sequence's rows of `o` are
    those of `mhla_causal` over that sequence alone (one call per run of adjacent sequences of equal length), padding rows zero.
    cu_seqlens: a pack (B = 1), as `mhla_causal` takes it -- `o` is the packed output `mhla_causal(..., cu_seqlens=)`, the state
    the ragged one of `mhla_causal_state(..., cu_seqlens=)`, one sequence of the pack per batch entry; one plan serves both.
    Grouped-query heads (k, v `[B, T, Hkv, .]`, H = G Hkv, G <= 8): `o` is `mhla_causal` on the un-repeated k, v -- bit for bit the
    output on k, v repeated G times per head, as the fla layer repeats them, without the copies; the state is built from the same
    k, v and has Hkv heads (`CausalState`).
    into (a host-positioned `CausalStateView`; with cu_seqlens only): the state half goes into the view's slots of its pool, as
    `mhla_causal_state(..., into=)`, and the view is returned as `state`."""
    if into is not None and cu_seqlens is None:
        raise ValueError("mhla_causal_prefill: into= takes a pack (cu_seqlens=)")
    if q.dim() != 4 or v.dim() != 4:
        raise ValueError("q, k: [B, T, H, K], v: [B, T, H, V]")
    if int(chunk_size) != 64:
        raise ValueError(f"mhla_causal_prefill: chunk_size={chunk_size}, the decode state supports 64 only")
    # grouped-query heads: the operator that computes `o` and the state both take the un-repeated k, v
    if k.dim() == 4:
        _kv_group("mhla_causal_prefill", q.shape[2], k.shape[2])
    if cu_seqlens is not None:
        # every refusal of the state half first, so that nothing is launched for a call that is refused
        plan = _causal_state_pack_args("mhla_causal_prefill", k, v, mixing_matrix, cu_seqlens, lengths, left_padded, capacity_chunks, into)[0]
        o = mhla_causal(q, k, v, mixing_matrix, chunk_size, scale, summaries=summaries, cu_seqlens=plan)
        return o, mhla_causal_state(k, v, mixing_matrix, capacity_chunks=capacity_chunks, cu_seqlens=plan, into=into)
    if lengths is None:
        o = mhla_causal(q, k, v, mixing_matrix, chunk_size, scale, summaries=summaries)
        return o, mhla_causal_state(k, v, mixing_matrix, capacity_chunks=capacity_chunks)
    B, T, H, _ = q.shape
    lengths = _int_tuple("mhla_causal_prefill", "lengths", lengths, B, T)
    state = mhla_causal_state(k, v, mixing_matrix, capacity_chunks=capacity_chunks, lengths=lengths, left_padded=left_padded)
    o = torch.zeros((B, T, H, v.shape[-1]), dtype=q.dtype, device=q.device)
    for i, j, n in _runs(lengths, B):
        if n:
            t0 = T - n if left_padded else 0
            o[i:j, t0:t0 + n] = mhla_causal(q[i:j, t0:t0 + n], k[i:j, t0:t0 + n], v[i:j, t0:t0 + n], mixing_matrix, chunk_size, scale,
                                            summaries=summaries)
    return o, state


def _causal_state_pack_args(fn, k, v, mixing_matrix, cu_seqlens, lengths, left_padded, capacity_chunks, into=None):
    """The checks of a packed prefill state, all before the library is loaded or anything is launched; returns (plan, capacity).
    into: the view whose slots take the pack's sequences -- the capacity is then its pool's."""
    if k.dim() != 4 or v.dim() != 4:
        raise ValueError("k: [B, T, H, K], v: [B, T, H, V]")
    if lengths is not None or left_padded:
        raise ValueError(f"{fn}: cu_seqlens (a pack) excludes lengths= and left_padded= (a padded batch)")
    B, T, H, K = k.shape
    _check_like(k, fn, v=(v, (B, T, H, v.shape[-1])))
    plan = _causal_varlen_args(fn, k, mixing_matrix, cu_seqlens, 64)
    L = mixing_matrix.shape[0]
    n_seqs = len(plan.cu) - 1
    if into is not None:
        if not isinstance(into, CausalStateView):
            raise TypeError(f"{fn}: into must be a CausalStateView (pool.at(slots)), got {type(into).__name__}")
        into._host_slots(fn)
        if capacity_chunks is not None:
            raise ValueError(f"{fn}: capacity_chunks={capacity_chunks} given together with into=: the capacity is the pool's "
                             f"({into.capacity_chunks} chunks)")
        if n_seqs != into.rows:
            raise ValueError(f"{fn}: the pack holds {n_seqs} sequences, the view selects {into.rows} slots {into.slots}")
        capacity_chunks = into.capacity_chunks
        if into.dims[1:] != (H, capacity_chunks, K, v.shape[-1]) or into.device != k.device:
            raise ValueError(f"{fn}: into is {into!r}, the pack has H={H} K={K} V={v.shape[-1]} on {k.device}")
    cap = L if capacity_chunks is None else int(capacity_chunks)
    if not 0 < cap <= L:
        raise ValueError(f"capacity_chunks={cap} must be in 1 .. {L} (rows of mixing_matrix)")
    if n_seqs < 1:
        raise ValueError(f"{fn}: cu_seqlens holds no sequence")
    if n_seqs * H > _MAX_GRID_BH:
        raise ValueError(f"{fn}: {n_seqs} sequences x H={H} heads exceed one launch's range of {_MAX_GRID_BH} (sequence, head) pairs: "
                         "split the pack")
    if plan.max_chunks > cap:
        long = [i for i, n in enumerate(plan.lengths) if n > 64 * cap]
        raise IndexError(f"{fn}: sequences {long} of lengths {[plan.lengths[i] for i in long]} need more than the {cap} chunks the "
                         f"state holds ({64 * cap} tokens)")
    if mixing_matrix.device != k.device or mixing_matrix.dim() < 2 or mixing_matrix.shape[1] < cap:
        raise ValueError(f"mixing_matrix must be [L, L(, 1, 1, 1, 1)] with L >= {cap} on {k.device}")
    return plan, cap


@_device_guard
def _causal_state_init_pack(k, v, mix, state: CausalState, plan: CausalVarlenPlan, seq_len: torch.Tensor):
    """One launch chain of `mhla_causal_varlen_state_init`: the state of every sequence of the pack k, v into the ragged `state`;
    `seq_len`: the sequences' lengths on the device (the state's `pos`).  A view: sequence s into slot s of the view, of its pool."""
    lib = _lib.load()
    _, T, H, K = k.shape
    k, v = _prep(k), _prep(v)
    mixf = _mix2d(mix)
    name, _, head = _state_args("prefill", mixf, state, (len(plan.lengths), seq_len.data_ptr()))
    ws = ()
    if state.page_mult is not None:   # h16 pages: the chunks' fp32 K^T V are staged, in slices of the chunk list beyond the cap
        V, dt = v.shape[-1], _dtype_code(k)
        need = lib.mhla_causal_varlen_state_init_paged_h16_ws_bytes(plan.n_chunks, H, K, V, dt)
        buf = _ws(min(need, max(EXTEND_WS_CAP_BYTES, lib.mhla_causal_varlen_state_init_paged_h16_ws_bytes(1, H, K, V, dt))), k.device)
        ws = (buf.data_ptr(), buf.numel() * 4)
    rc = getattr(lib, name)(_view(k), _view(v), *head, max(plan.lengths), T, H, K, v.shape[-1], state.chunk_size, plan.n_chunks,
                            plan.table.data_ptr(), plan.dst.data_ptr(), *ws, _dtype_code(k), _stream())
    _lib.check(rc, name)


def mhla_causal_state(k: torch.Tensor, v: torch.Tensor, mixing_matrix: torch.Tensor, *, lengths=None, left_padded: bool = False,
                      capacity_chunks: Optional[int] = None, cu_seqlens=None, into=None) -> CausalState:
    """The `CausalState` after the T tokens of k `[B, T, H, K]`, v `[B, T, H, V]` (the state half of `mhla_causal_prefill`;
    chunk 64).  T = 0: an empty state.
    lengths (a list or a tensor of B ints in 0 .. T; a device tensor is read once, which synchronises): a padded batch -- the tokens
    of sequence b are rows `[0, lengths[b])`, or `[T - lengths[b], T)` with `left_padded`, and the state is ragged (`CausalState`):
    every sequence as if prefilled alone, `lengths[b] = 0` an empty one.  Built run by run of adjacent sequences of equal length.
    cu_seqlens (a `CausalVarlenPlan`, a list or a tensor, as `mhla_causal` takes it; B = 1): a pack -- the ragged state of B =
    number of sequences, in `cu` order, empty ones included, bit for bit what every sequence prefilled alone gives, in ONE launch
    chain whatever their number (`mhla_causal_varlen_state_init`).  Excludes `lengths` / `left_padded` (ValueError); IndexError
    names the sequences longer than `64 capacity_chunks` tokens; ValueError when sequences x heads exceed 65535.
    into (a host-positioned `CausalStateView`, `pool.at(slots)`; with cu_seqlens only): sequence s of the pack is prefilled into slot
    `slots[s]` of the pool, in the same single launch chain (`mhla_causal_varlen_state_init_slots`), and the view is returned: those
    slots -- finished chunks of S, P, Cur, pos, a cleared `full` flag and the host mirror -- then hold bit for bit what the call
    without `into` returns, and every other slot keeps every bit.  The capacity is the pool's: `capacity_chunks` together with
    `into` is a ValueError, as is a pack whose number of sequences is not the view's."""
    if into is not None and cu_seqlens is None:
        raise ValueError("mhla_causal_state: into= takes a pack (cu_seqlens=)")
    if cu_seqlens is not None:
        plan, cap = _causal_state_pack_args("mhla_causal_state", k, v, mixing_matrix, cu_seqlens, lengths, left_padded, capacity_chunks, into)
        _, T, H, K = k.shape
        if T:
            _require_gpu(k, v, mixing_matrix, plan.table)
        if into is not None:
            pool = into.pool
            with torch.no_grad():
                seq_len = torch.tensor(plan.lengths, dtype=torch.int32).to(k.device)   # the one small copy of the call
                idx = into.map.to(torch.int64)
                if into.pages is not None:   # (a paged pool: the slots start anew, their pages released first; before anything changes)
                    pool._assign("mhla_causal_state", into.slots, plan.lengths, True)
                if T:
                    _causal_state_init_pack(k.detach(), v.detach(), mixing_matrix, into, plan, seq_len)
                else:   # (an all-empty pack launches nothing: empty slots)
                    pool.P[idx] = 0
                    pool.Cur[idx] = 0
                pool.pos[idx] = seq_len
                if pool._full is not None:
                    pool._full[idx] = 0
            into.lengths = plan.lengths
            return into
        with torch.no_grad():
            state = CausalState.empty(len(plan.lengths), H, K, v.shape[-1], cap, k.device, 64)
            # (the launch chain writes P and Cur of every sequence, the empty ones included: nothing to zero first)
            P, Cur = (state.P, state.Cur) if not T else (torch.empty_like(state.P), torch.empty_like(state.Cur))
            state = CausalState(state.S, P, Cur, 0, 64, lengths=plan.lengths)
            if T:
                _causal_state_init_pack(k.detach(), v.detach(), mixing_matrix, state, plan, state.pos)
        return state
    if k.dim() != 4 or v.dim() != 4:
        raise ValueError("k: [B, T, H, K], v: [B, T, H, V]")
    B, T, H, K = k.shape
    V = v.shape[-1]
    _check_like(k, "mhla_causal_state", v=(v, (B, T, H, V)))
    if lengths is not None:
        lengths = _int_tuple("mhla_causal_state", "lengths", lengths, B, T)
        T = max(lengths)
    L = mixing_matrix.shape[0]
    cap = L if capacity_chunks is None else int(capacity_chunks)
    if not 0 < cap <= L:
        raise ValueError(f"capacity_chunks={cap} must be in 1 .. {L} (rows of mixing_matrix)")
    if (T + 63) // 64 > cap:
        raise IndexError(f"sequence of {T} tokens needs {(T + 63) // 64} chunks but the state holds only {cap}")
    if mixing_matrix.device != k.device or mixing_matrix.dim() < 2 or mixing_matrix.shape[1] < cap:
        raise ValueError(f"mixing_matrix must be [L, L(, 1, 1, 1, 1)] with L >= {cap} on {k.device}")
    _require_gpu(k, v, mixing_matrix)
    nb = _MAX_GRID_BH // H
    with torch.no_grad():
        state = CausalState.empty(B, H, K, V, cap, k.device, 64)
        # a uniform batch is one run of T tokens per slice; T = 0 launches nothing
        t_pad = k.shape[1]
        for i, j, n, part in _run_slices(state, lengths if lengths is not None else (T,) * B, nb):
            if n:
                t0 = t_pad - n if left_padded and lengths is not None else 0
                _causal_state_init(k[i:j, t0:t0 + n].detach(), v[i:j, t0:t0 + n].detach(), mixing_matrix, part)
        if lengths is not None:
            return CausalState(state.S, state.P, state.Cur, 0, 64, lengths=lengths)
        state.seen = T
    return state


def _step_view_ok(t: torch.Tensor) -> bool:
    # what the step kernels address in place: 4-element pieces (8 bytes for 16-bit types, 16 for fp32)
    sb, sn, sh, sd = t.stride()
    return sd == 1 and (sb | sn | sh) % 4 == 0 and t.data_ptr() % (4 * t.element_size()) == 0


class _Prepared(NamedTuple):
    """What `_decode_prepare` returns and every launcher below takes as its first nine arguments (`*prepared`): the token tensors
    addressable in place or as contiguous copies, the mixing matrix and the norm weight in fp32, the position of the first token
    (None when the call is not host-positioned), the scale, and whether the rows go through the norm x gate epilogue."""
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    gate: Optional[torch.Tensor]
    mixf: torch.Tensor
    wf: Optional[torch.Tensor]
    pos: Optional[int]
    scale: float
    want_y: bool

    def part(self, i, j, t0=None, t1=None, pos=None) -> "_Prepared":
        """The same call for sequences [i, j) and tokens [t0, t1) (None: no bound) only; `pos`: the position of its first token,
        where that is another."""
        q, k, v, gate = (x if x is None else x[i:j, t0:t1] for x in self[:4])
        return self._replace(q=q, k=k, v=v, gate=gate, pos=self.pos if pos is None else pos)


def _decode_entry(fn, state, q, k, v, one_token, refuse_stale, packed=False):
    """The first refusals of every decode call, in this order: the state's type, a stale host mirror (not for
    `mhla_causal_step_dev`, which never reads it), the tensors' rank, the token count."""
    if not isinstance(state, CausalState):
        raise TypeError(f"{fn}: state must be a CausalState, got {type(state).__name__}")
    if isinstance(state, PagedCausalState):
        _refuse_paged_pool(fn, state)
    if refuse_stale and isinstance(state, CausalStateView):   # (a slot map on the device: the device-positioned step alone)
        state._host_slots(fn)
    if refuse_stale and state.stale:
        state._refuse_stale(fn)
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        t = "1" if one_token else "T"
        raise ValueError(f"q, k: [B, {t}, H, K], v: [B, {t}, H, V]")
    T = q.shape[1]
    if one_token and T != 1:
        raise ValueError(f"{fn} takes one token per call (T = 1), got T = {T}")
    if T < 1 and not packed:   # (a pack whose sequences are all empty has no row: nothing is launched)
        raise ValueError(f"{fn} takes at least one token per call, got T = {T}")


def _decode_prepare(fn, q, k, v, mixing_matrix, state, scale, gate, norm_weight, epilogue, positioned=True, seqs=None) -> _Prepared:
    """What `mhla_causal_step` and `mhla_causal_extend` (`fn`: the one called, for the messages) check after `_decode_entry`'s
    tests of the state's type, the tensors' rank and T, and the tensors they launch with.  The C ABI receives raw pointers, so
    everything is refused here, in an order callers rely on -- the head counts (k, v and the state may have Hkv heads that divide
    q's H: `_kv_group`), tensors like q, dtype, state shapes, devices, norm_weight, requires-grad, GPU,
    matrix shape, chunk size, rows / capacity (IndexError), epilogue arguments, state contiguity -- before anything is launched
    or `state` is touched.  Returns a `_Prepared`; its position is that of the first token (of the furthest sequence
    of a ragged state, whose `seen` is `max(lengths)`: rows and capacity are checked against it).  `positioned=False`
    (`mhla_causal_step_dev`, which made its own check of the matrix against the capacity): the host position is neither read nor
    checked -- a stale mirror is fine -- and the position returned is None.  `seqs` (packed new tokens, `cu_seqlens=`): the
    sequences the state must hold, where the tokens are one row [1, N, ...] and say nothing about it."""
    B, T, H, K = q.shape
    V = v.shape[-1]
    Hk = k.shape[2]   # grouped-query heads: k, v and the state have Hkv heads, q, gate and the rows H = G Hkv
    dims = state.dims
    nrow, cap = dims[0], dims[2]   # the state's batch rows (B, or -- a view -- the slots of the pool, B of which the call selects); its capacity
    _kv_group(fn, H, Hk)
    try:
        _check_like(q, fn, k=(k, (B, T, Hk, K)), v=(v, (B, T, Hk, V)), gate=(gate, (B, T, H, V)))
    except TypeError as e:
        raise ValueError(str(e)) from None
    if seqs is not None:
        B = seqs
    if q.dtype not in _DTYPES:
        raise ValueError(f"{fn}: unsupported dtype {q.dtype} (float32 / bfloat16 / float16)")
    chunks = state._chunks
    if (state.rows if isinstance(state, CausalStateView) else nrow) != B or dims != (nrow, Hk, cap, K, V) or tuple(state.P.shape) != (nrow, Hk, K, V) or tuple(state.Cur.shape) != (nrow, Hk, K, V):
        raise ValueError(f"{fn}: state is {state!r}, the {'token has' if T == 1 else 'tokens have'} B={B} H={H if Hk == H else Hk} K={K} V={V}"
                         + ("" if Hk == H else f" (k/v heads; q has {H})"))
    dev = q.device
    for name, t in (("state.S", chunks), ("state.P", state.P), ("state.Cur", state.Cur), ("mixing_matrix", mixing_matrix), ("norm_weight", norm_weight)):
        if t is not None and t.device != dev:
            raise ValueError(f"{fn}: {name} is on {t.device}, expected {dev}")
    if norm_weight is not None and norm_weight.numel() != V:
        raise ValueError(f"{fn}: norm_weight has {norm_weight.numel()} entries, expected V={V}")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (q, k, v, gate)):
        raise RuntimeError(f"{fn} is inference only: call it under torch.no_grad() (an input requires grad)")
    _require_gpu(q, k, v, mixing_matrix)
    L = mixing_matrix.shape[0]
    if mixing_matrix.dim() < 2 or mixing_matrix.shape[1] < min(L, cap):
        raise ValueError(f"mixing_matrix must be [L, L(, 1, 1, 1, 1)], got {tuple(mixing_matrix.shape)}")
    if int(state.chunk_size) != 64:
        raise ValueError(f"{fn}: chunk_size={state.chunk_size}, the decode state supports 64 only")
    pos = None
    if positioned:
        pos = state.seen
        n = (pos + T + 63) // 64
        if n > L:
            raise IndexError(f"sequence of {pos + T} tokens needs {n} chunks but mixing_matrix has only {L} rows")
        if n > cap:
            raise IndexError(f"sequence of {pos + T} tokens needs {n} chunks but the state holds only {cap}")
    if scale is None:
        scale = K ** -0.5
    want_y = bool(epilogue) if epilogue is not None else (gate is not None or norm_weight is not None)
    if not want_y and (gate is not None or norm_weight is not None):
        raise ValueError(f"{fn}: gate / norm_weight given with epilogue=False")
    if not (chunks.is_contiguous() and state.P.is_contiguous() and state.Cur.is_contiguous()):
        raise ValueError(f"{fn}: state tensors must be contiguous")
    # (a view whose slot map is on the device has no host lengths; its positions are the pool's all the same)
    if (state.lengths is not None or isinstance(state, CausalStateView)) and (
            (state.lengths is not None and len(state.lengths) != B) or state.pos is None or state.pos.device != dev
            or state.pos.dtype != torch.int32 or tuple(state.pos.shape) != (nrow,) or not state.pos.is_contiguous()):
        raise ValueError(f"{fn}: a ragged state carries B={B} lengths and `pos`, a contiguous int32 [B] tensor on {dev}")
    # (nothing from here to the end of the call is recorded for autograd, with or without torch.no_grad(): grad mode is off or no
    # token tensor requires grad, both matrices are detached, and the launch reads and writes through raw pointers)
    q, k, v = (t if _step_view_ok(t) else t.contiguous() for t in (q, k, v))
    if gate is not None and not _step_view_ok(gate):
        gate = gate.contiguous()
    wf = norm_weight.detach().reshape(V).to(torch.float32).contiguous() if norm_weight is not None else None
    # (built without the generated `__new__`: one Python call less on a path that is bound by the host)
    return tuple.__new__(_Prepared, (q, k, v, gate, _mix2d(mixing_matrix), wf, pos, scale, want_y))


@_device_guard
def _launch_rows(q, k, v, gate, mixf, wf, scale, want_y, call, state, pos, middle, ws_bytes, res, norm_eps, B, packed=False):
    """The one library call of the decode entry points that compute rows: `call` (a key of `_ENTRY`) on what `_decode_prepare`
    returned (the first eight arguments; the guard finds its tensor at once), for the sequences `state` -- the batch or a slice of it
    -- holds.  All of them take the token views and the state's part (`_state_args`, with the positions `pos`), then arguments of
    their own (`middle`), then one tail: the rows into `res` (through the norm x gate epilogue with `want_y`), a workspace of
    `ws_bytes`, the sizes (`B` sequences), scale, dtype and stream.  `packed`: the tokens are one row [1, N, ...] -- views with a zero
    batch stride (`_view0`) and the packed form of the state's part; that is all the difference."""
    lib = _lib.load()
    _, _, H, K = q.shape
    view = _view0 if packed else _view
    name, twin, head = _state_args(call, mixf, state, pos, packed)
    fn, heads = _gqa_call(lib, name, H, k.shape[2]) if twin else (getattr(lib, name), (H,) if twin is False else (H, k.shape[2]))
    ws = _ws(ws_bytes, q.device)
    # (the two optional arguments spelt out, not through `_view_or_null` / `_ptr`: two Python calls on a host-bound path)
    rc = fn(view(q), view(k), view(v), *head, *middle, NULL_VIEW if want_y else view(res), view(gate) if gate is not None else NULL_VIEW,
            wf.data_ptr() if wf is not None else None, float(norm_eps), view(res) if want_y else NULL_VIEW, ws.data_ptr(), ws.numel() * 4,
            B, *heads, K, v.shape[-1], state.chunk_size, float(scale), _DTYPES[q.dtype], _stream())
    _lib.check(rc, name)


def _causal_decode(q, k, v, gate, mixf, wf, pos, scale, want_y, state, res, norm_eps, extend=False):
    """One launch chain of `mhla_causal_step` (one token) or, with `extend`, of `mhla_causal_extend` (T tokens) on what
    `_decode_prepare` returned (the first nine arguments): the tokens at positions pos .. of the uniform `state`, the rows into `res`."""
    B, T, H, K = q.shape
    V, dt = v.shape[-1], _DTYPES[q.dtype]
    if extend:
        call, middle, ws_bytes = "extend_uniform", (pos, T), _lib.load().mhla_causal_extend_ws_bytes(B, T, H, K, V, pos, dt)
    else:
        call, middle, ws_bytes = "step_uniform", (pos,), _step_ws_bytes(B, H, K, V, dt)
    _launch_rows(q, k, v, gate, mixf, wf, scale, want_y, call, state, (), middle, ws_bytes, res, norm_eps, B)


def _causal_step_ragged(q, k, v, gate, mixf, wf, _, scale, want_y, state, pos, lengths, res, norm_eps):
    """One launch chain of `mhla_causal_step_ragged` on what `_decode_prepare` returned, for the sequences `state` (a batch slice)
    holds: `pos` their device positions, which the chain advances, `lengths` the host mirror of the same numbers."""
    B, _, H, K = q.shape
    _launch_rows(q, k, v, gate, mixf, wf, scale, want_y, "step", state, (pos.data_ptr(),),
                 (max(lengths), int(any(n % 64 == 63 for n in lengths))), _step_ws_bytes(B, H, K, v.shape[-1], _DTYPES[q.dtype]), res, norm_eps, B)


def mhla_causal_step(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mixing_matrix: torch.Tensor, state: CausalState, *,
                     scale: Optional[float] = None, gate: Optional[torch.Tensor] = None, norm_weight: Optional[torch.Tensor] = None,
                     norm_eps: float = 1e-5, epilogue: Optional[bool] = None) -> torch.Tensor:
    """One decoding step of the causal operator: q, k `[B, 1, H, K]`, v `[B, 1, H, V]` of the token at position `state.seen`;
    returns row `state.seen` of `mhla_causal` over the whole sequence, `[B, 1, H, V]`, updates `state` in place and advances
    `state.seen`.  Strided views (slices of a packed projection) are read in place.  With `gate` and / or `norm_weight` (or
    `epilogue=True` for the bare norm) the result is `rmsnorm_gate(o, gate, norm_weight, norm_eps)` applied in the same
    launch chain.  Inference only: nothing is recorded for autograd, and an input that requires grad while grad mode is on
    raises.  The step that would open chunk L of an [L, L] matrix (or exceed the state's capacity) raises IndexError and
    leaves the state untouched.  Cost per token: P and Cur read, Cur written (12 K V bytes per (b, h)); every 64th step also
    closes the chunk and re-mixes the finished ones (4 K V bytes per finished chunk).
    On a ragged state (`state.lengths`) the token of sequence b is at position `lengths[b]`, the row returned is that of
    `mhla_causal` over that sequence's own tokens, and each sequence closes its chunk where its own position says so -- one
    launch chain for the batch, the positions advanced on the device (no copy, no synchronisation); every entry of `lengths`
    and `seen` grow by one.  The IndexError is raised when the longest sequence would not fit.
    Grouped-query heads: k, v `[B, 1, Hkv, .]` with a state of Hkv heads and q of H = G Hkv (G <= 8; query head h uses k/v head
    h // G): the bits of this call on k, v repeated G times and a state of H heads, with P and Cur moved once per k/v head.  A
    uniform grouped state takes the ragged launch chain, its positions filled on the device; `step_dev`, `extend`, `verify` and
    `commit` take the same shapes."""
    _decode_entry("mhla_causal_step", state, q, k, v, True, True)
    prepared = _decode_prepare("mhla_causal_step", q, k, v, mixing_matrix, state, scale, gate, norm_weight, epilogue)
    B, _, H, _ = q.shape
    res = q.new_empty((B, 1, H, v.shape[-1]))
    if state.lengths is None and k.shape[2] == H:
        _causal_decode(*prepared, state, res, norm_eps)
        state.seen += 1
        return res
    lengths, pos = state.lengths, state.pos
    if lengths is None:   # grouped heads have no uniform kernels: the ragged chain, its positions filled on the device (no copy, no synchronisation)
        lengths, pos = (state.seen,) * B, torch.full((B,), state.seen, dtype=torch.int32, device=q.device)
    nb = _MAX_GRID_BH // H
    # What the library checks per launch, for every slice before the first launch (a refusal after an earlier slice had run would
    # leave its device positions ahead of `lengths`): a slice with a sequence on a boundary needs the row after its furthest
    # sequence's chunk, unless that chunk is the state's last.  (Not `_slices` with counts of one, which asks for less.)
    cols = prepared.mixf.shape[1]
    for i in range(0, B, nb):
        part = lengths[i:i + nb]
        need = max(part) // 64 + 1 + (any(n % 64 == 63 for n in part) and max(part) // 64 + 1 < state.capacity_chunks)
        if cols < need:
            raise IndexError(f"mhla_causal_step: a sequence of lengths {part} closes its chunk: row {need - 1} of mixing_matrix is read, "
                             f"which has only {cols} columns")
    if state.pages is not None:   # (the page rule, `_page_rule`, on the lengths already at hand)
        state.pool._assign("mhla_causal_step", state.slots, [n + 1 for n in lengths])
    for part, p, pos_, lengths_, out in _batch_slices(state, nb, prepared, pos, lengths, res):
        _causal_step_ragged(*p, part, pos_, lengths_, out, norm_eps)
    if state.lengths is not None:
        state.lengths = tuple(n + 1 for n in state.lengths)
    state.seen += 1
    return res


def _causal_step_dev(q, k, v, gate, mixf, wf, _, scale, want_y, state, pos, full, rotary, fmap, res, norm_eps):
    """One launch chain of `mhla_causal_step_dev` on what `_decode_prepare` returned, for the sequences `state` (a batch slice)
    holds; `rotary`: the tables as the library takes them, (cos, sin, row stride, rows), nulls and zeros without.  Nothing here reads
    a position or synchronises: legal under stream capture."""
    B, _, H, K = q.shape
    _launch_rows(q, k, v, gate, mixf, wf, scale, want_y, "step_dev", state, (pos.data_ptr(),), (full.data_ptr(), *rotary, fmap),
                 _step_ws_bytes(B, H, K, v.shape[-1], _DTYPES[q.dtype]), res, norm_eps, B)


def mhla_causal_step_dev(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mixing_matrix: torch.Tensor, state: CausalState, *,
                         feature_map: Optional[str] = None, rotary=None, scale: Optional[float] = None,
                         gate: Optional[torch.Tensor] = None, norm_weight: Optional[torch.Tensor] = None, norm_eps: float = 1e-5,
                         epilogue: Optional[bool] = None) -> torch.Tensor:
    """`mhla_causal_step` on a ragged state with the positions on the device only: the same rows and the same state, bit for bit,
    from a call that reads no host position, advances none and never synchronises -- the launch chain (always three launches) and
    every argument are the same token after token, so the call may be captured in `torch.cuda.graph` and replayed once per token
    with new q, k, v (and gate) copied into the captured tensors.  It marks the state `stale`: `state.lengths` / `seen` stay where
    they were until `state.sync()`, and `mhla_causal_step`, `mhla_causal_extend` and `CausalState.cat` refuse the state until then.
    state: a ragged one (ValueError otherwise: `state.to_ragged()` makes one on the same storage).  mixing_matrix: at least
    `capacity_chunks` rows and columns (IndexError otherwise) -- the bound is the capacity, not the current length.
    A sequence at or beyond the capacity (64 capacity_chunks tokens) is FROZEN, not an error: its state and position stay, its row
    of the result is zeros, and `state.full[b]` becomes 1 -- `state.sync()` raises the IndexError the host-positioned step
    would have raised, after the fact.
    feature_map (None / "identity", "relu", "elu") and rotary = (cos, sin) -- tables `[>= 64 capacity_chunks, K/2]` in the dtype
    of q -- fuse the fla layer's q / k prologue into the step: q and k are then the projections' outputs, and sequence b is
    rotated by row `pos[b]` of the tables, with the arithmetic and the rounding of `featmap_rotary` (K % 8 == 0).
    scale, gate, norm_weight, norm_eps, epilogue, strided views, inference only: as `mhla_causal_step`."""
    fn = "mhla_causal_step_dev"
    _decode_entry(fn, state, q, k, v, True, False)   # (a stale mirror is what this call leaves: not refused)
    B, _, H, K = q.shape
    if state.lengths is None and not isinstance(state, CausalStateView):   # (a view is of a ragged pool, whatever its map)
        raise ValueError(f"{fn}: the state is uniform ({state!r}); the positions must live on the device: pass state.to_ragged()")
    cap = state.capacity_chunks
    if mixing_matrix.dim() < 2 or mixing_matrix.shape[0] < cap or mixing_matrix.shape[1] < cap:
        raise IndexError(f"{fn}: mixing_matrix {tuple(mixing_matrix.shape)} has fewer rows or columns than the state's capacity of "
                         f"{cap} chunks, which bounds what a step may read")
    cos = sin = None
    if rotary is not None:
        cos, sin = rotary
        for name, t in (("cos", cos), ("sin", sin)):
            if t.dim() != 2 or t.shape[0] < 64 * cap:
                raise ValueError(f"{fn}: rotary {name} has shape {tuple(t.shape)}, expected at least {64 * cap} rows (64 per chunk of "
                                 f"capacity) of K/2={K // 2} entries")
            if t.dtype != q.dtype or t.device != q.device:
                raise ValueError(f"{fn}: rotary {name} is {t.dtype} on {t.device}, expected {q.dtype} on {q.device}")
            if t.shape[1] != K // 2:
                raise ValueError(f"{fn}: rotary {name} has shape {tuple(t.shape)}, expected K/2={K // 2} entries per row")
    if (rotary is not None or feature_map is not None) and K % 8:
        raise ValueError(f"{fn}: K={K}: the fused prologue (feature_map / rotary) needs K % 8 == 0")
    if feature_map not in _FMAPS:
        raise ValueError(f"{fn}: feature_map {feature_map!r}: one of {sorted(k for k in _FMAPS if k)} or None")
    prepared = _decode_prepare(fn, q, k, v, mixing_matrix, state, scale, gate, norm_weight, epilogue, positioned=False)
    rot = (None, None, 0, 0)
    if cos is not None:
        if (cos.stride(1) != 1 or sin.stride(1) != 1 or cos.stride(0) != sin.stride(0) or cos.stride(0) % 4
                or (cos.data_ptr() | sin.data_ptr()) % (4 * cos.element_size())):
            cos, sin = cos.contiguous(), sin.contiguous()
        rot = (cos.data_ptr(), sin.data_ptr(), cos.stride(0), cos.shape[0])
    if state._full is None and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{fn}: state.full does not exist yet and a tensor created while capturing would belong to the graph "
                           "(cleared by every replay): run one eager step first, or touch state.full before the capture")
    full = state.full
    res = q.new_empty((B, 1, H, v.shape[-1]))
    state.stale = True
    for part, p, pos, full_, out in _batch_slices(state, _MAX_GRID_BH // H, prepared, state.pos, full, res):
        _causal_step_dev(*p, part, pos, full_, rot, _FMAPS[feature_map], out, norm_eps)
    return res


# Largest workspace one launch chain of `mhla_causal_extend` takes: a longer extension is cut into consecutive calls.  Per (b, h)
# the chain needs 4 K V bytes per chunk touched after the first and 4 V bytes per token (mhla_hip.h).
EXTEND_WS_CAP_BYTES = 256 << 20
SWAP_STAGE_CAP_BYTES = EXTEND_WS_CAP_BYTES   # the device staging buffer of a swap to or from a host blob (`_swap_launch`)


def _counts_prepare(fn, q, k, v, mixing_matrix, state, counts, left_padded, cu_seqlens, scale, gate, norm_weight, epilogue):
    """What a call with per-sequence token counts checks, in the order callers rely on, before anything is launched or `state` is
    touched: the counts given (`mhla_causal_extend(counts=)`, `mhla_causal_verify`; padded tokens [B, T, ...]) or those of packed new
    tokens (`cu_seqlens=`; one row [1, N, ...], which says nothing about the number of sequences).  Returns (cu as a tuple, or None
    without `cu_seqlens`; every sequence's token count; what `_decode_prepare` returns)."""
    if cu_seqlens is None:
        cu, B = None, q.shape[0]
        counts = _int_tuple(fn, "counts", counts, B, q.shape[1])
    else:
        if counts is not None or left_padded:
            raise ValueError(f"{fn}: cu_seqlens (packed new tokens) excludes counts and left_padded, which place windows in padded tensors")
        if q.shape[0] != 1:
            raise ValueError(f"{fn}: cu_seqlens takes one packed row (B = 1), got B = {q.shape[0]}")
        cu = _cu_host(cu_seqlens.cu if isinstance(cu_seqlens, CausalVarlenPlan) else cu_seqlens)   # (of a plan: its host `cu` alone)
        if cu[-1] != q.shape[1]:
            raise ValueError(f"{fn}: cu_seqlens ends at {cu[-1]}, the pack has N = {q.shape[1]} tokens")
        B = len(cu) - 1
    if state.lengths is None:
        raise ValueError(f"{fn}: {'counts' if cu is None else 'cu_seqlens'} needs a ragged state and this one is uniform ({state!r}); the "
                         "positions must live on the device: pass state.to_ragged()")
    if len(state.lengths) != B:
        raise ValueError(f"{fn}: the state holds {len(state.lengths)} sequences, "
                         + (f"the tokens B={B}" if cu is None else f"cu_seqlens has {len(cu)} entries ({B} sequences)"))
    if cu is not None:
        counts = tuple([b - a for a, b in zip(cu, cu[1:])])
    _counts_fit(fn, mixing_matrix, state, counts)
    return cu, counts, _decode_prepare(fn, q, k, v, mixing_matrix, state, scale, gate, norm_weight, epilogue, positioned=False,
                                       seqs=None if cu is None else B)


def _counts_fit(fn, mixing_matrix, state, counts):
    """The IndexErrors of a call with per-sequence counts, naming the sequences: every sequence's end within the rows of the mixing
    matrix and the state's capacity."""
    if mixing_matrix.dim() < 2:
        raise ValueError(f"mixing_matrix must be [L, L(, 1, 1, 1, 1)], got {tuple(mixing_matrix.shape)}")
    L, cap = mixing_matrix.shape[0], state.capacity_chunks
    need = [(p + n + 63) // 64 if n else 0 for p, n in zip(state.lengths, counts)]
    if max(need, default=0) <= min(L, cap):   # (the usual call: no words to put together)
        return
    for limit, what in ((L, f"mixing_matrix has only {L} rows"), (cap, f"the state holds only {cap}")):
        over = [b for b, c in enumerate(need) if c > limit]
        if over:
            raise IndexError(f"{fn}: sequences {over} (lengths {tuple(state.lengths[b] for b in over)} + counts "
                             f"{tuple(counts[b] for b in over)}) need up to {max(need)} chunks but {what}")


def _ragged_plan(lengths, counts, cap):
    """What `mhla_causal_extend_ragged` is told about the device arrays of one batch slice: (max_end, max_later, any_close, the
    last row of the mixing matrix it may read)."""
    live = [(p, n) for p, n in zip(lengths, counts) if n]
    if not live:
        return 0, 0, False, 0
    # (lists, not generators: a handful of sequences, on the path of every extend, verify and commit)
    max_end = max([p + n for p, n in live])
    max_later = max([(p + n - 1) // 64 - p // 64 for p, n in live])
    any_close = any([p % 64 + n >= 64 for p, n in live])
    return max_end, max_later, any_close, (min(max_end // 64, cap - 1) if any_close else (max_end - 1) // 64)


# ---- packed new tokens (`cu_seqlens=` of extend and verify, the draft's `cu` of a commit): the tokens of all sequences in one row
_PACK_MAX_TOKENS = 65535   # tokens of one library call: its last launch puts them on a grid dimension


def _slices(fn, state, counts, H, mixf, cu=None, ws_dims=None, rows=False):
    """The launch chains of one call with per-sequence `counts`, (first sequence, end, `_ragged_plan`) each, after what the library
    checks per launch was checked for every one of them before the first launch (see mhla_causal_step): the columns of the matrix and
    -- `rows`, a commit, whose `counts` are the accepted ones and have not been held against the matrix -- its rows.
    Padded tokens: batch slices of one launch's (b, h) range, `_MAX_GRID_BH // H` sequences.  Packed (`cu`): `_packed_cut`."""
    B, lengths = len(counts), state.lengths
    if cu is None:
        nb, cap = min(B, _MAX_GRID_BH // H), state.capacity_chunks
        slices = [(i, min(B, i + nb), _ragged_plan(lengths[i:i + nb], counts[i:i + nb], cap)) for i in range(0, B, nb)]
    else:
        slices = _packed_cut(fn, state, cu, counts, H, ws_dims)
    for i, j, plan in slices:
        if plan[0] and mixf.shape[1] < plan[3] + 1:
            raise IndexError(f"{fn}: sequences {list(range(i, j))} (lengths {lengths[i:j]}, counts {counts[i:j]}): row {plan[3]} of "
                             f"mixing_matrix is read, which has only {mixf.shape[1]} columns")
    if rows and any(plan[0] and mixf.shape[0] < plan[3] + 1 for _, _, plan in slices):
        raise IndexError(f"{fn}: mixing_matrix has only {mixf.shape[0]} rows, fewer than the accepted tokens read (lengths "
                         f"{lengths}, accept {counts})")
    return slices


def _packed_cut(fn, state, cu, counts, H, ws_dims):
    """Where a pack is cut: the whole pack, or -- beyond `_PACK_MAX_TOKENS`, one launch's (b, h) range (`_MAX_GRID_BH // H`) or, with
    `ws_dims` = (H, Hkv, K, V, dtype code) of a call that computes rows, `EXTEND_WS_CAP_BYTES` -- consecutive runs of whole sequences,
    each as long as fits.  Sequences are independent, so a cut changes no bit; there is no cut inside a sequence: one that alone
    exceeds a limit is a ValueError."""
    B, cap, nb = len(counts), state.capacity_chunks, max(1, _MAX_GRID_BH // H)
    lib = _lib.load()

    def fits(i, j, plan=None):
        n = cu[j] - cu[i]
        if j - i > nb or n > _PACK_MAX_TOKENS:
            return False
        if ws_dims is None or not n:
            return True
        Hq, Hk, K, V, dt = ws_dims
        later = (plan or _ragged_plan(state.lengths[i:j], counts[i:j], cap))[1]
        return lib.mhla_causal_extend_packed_ws_bytes(j - i, n, Hq, Hk, K, V, later, dt) <= EXTEND_WS_CAP_BYTES

    whole = _ragged_plan(state.lengths, counts, cap)
    slices, i = ([(0, B, whole)], B) if fits(0, B, whole) else ([], 0)   # (the usual call: one chain)
    while i < B:
        j = B
        if not fits(i, B):
            j = i + 1
            if not fits(i, j):
                raise ValueError(f"{fn}: sequence {i} alone brings {cu[j] - cu[i]} new tokens, more than one call takes ({_PACK_MAX_TOKENS} "
                                 f"tokens, a workspace of EXTEND_WS_CAP_BYTES={EXTEND_WS_CAP_BYTES}): a pack is cut between sequences "
                                 "only, pass the sequence in pieces")
            while j < B and fits(i, j + 1):
                j += 1
        slices.append((i, j, _ragged_plan(state.lengths[i:j], counts[i:j], cap)))
        i = j
    return slices


def _causal_extend_ragged(q, k, v, gate, mixf, wf, _, scale, want_y, state, pos, ntok, plan, left_padded, res, norm_eps, call="extend"):
    """One launch chain of `mhla_causal_extend_ragged` on what `_decode_prepare` returned, for the sequences `state` (a batch slice)
    holds: `pos` their device positions, which the chain advances, `ntok` their token counts on the device, `plan` the host
    values of `_ragged_plan`.  call="verify" (`mhla_causal_verify_ragged`): the same arguments and rows, nothing committed."""
    B, T, H, K = q.shape
    max_end, max_later, any_close, _ = plan
    ws_bytes = _extend_ragged_ws_bytes(_lib.load(), B, T, H, k.shape[2], K, v.shape[-1], max_later, _DTYPES[q.dtype])
    _launch_rows(q, k, v, gate, mixf, wf, scale, want_y, call, state, (pos.data_ptr(),),
                 (ntok.data_ptr(), T, max_end, max_later, int(any_close), int(bool(left_padded))), ws_bytes, res, norm_eps, B)


def _causal_packed(q, k, v, gate, mixf, wf, _, scale, want_y, state, pos, off, B, plan, res, norm_eps, call):
    """One launch chain of `mhla_causal_extend_packed` (`call`: "extend_packed"; or "verify_packed") on what `_decode_prepare`
    returned, cut to the chain's tokens, for the B sequences `state` (a batch slice) holds: `pos` their device positions, `off` their
    B + 1 offsets on the device, `plan` the host values of `_ragged_plan`; the rows into `res`."""
    _, N, H, K = q.shape
    max_end, max_later, any_close, _ = plan
    ws_bytes = _lib.load().mhla_causal_extend_packed_ws_bytes(B, N, H, k.shape[2], K, v.shape[-1], max_later, _DTYPES[q.dtype])
    _launch_rows(q, k, v, gate, mixf, wf, scale, want_y, call, state, (pos.data_ptr(),), (off.data_ptr(), N, max_end, max_later, int(any_close)),
                 ws_bytes, res, norm_eps, B, True)


def _packed_offsets(cu, slices, device, accept=None):
    """The one small copy of a packed call: for every chain of `slices` its sequences' offsets from the chain's first token (j - i + 1
    ints), one after the other, then -- a commit -- `accept`; returns (the device tensor, where each chain's offsets begin)."""
    host, at = [], []
    for i, j, _ in slices:
        at.append(len(host))
        host.extend([c - cu[i] for c in cu[i:j + 1]])
    if accept is not None:
        host.extend(accept)
    return torch.tensor(host, dtype=torch.int32).to(device), at


def _view0(t: torch.Tensor) -> View:
    """A tensor of a pack, [1, N, H, D], as the packed entry points take it: the batch stride 0."""
    s = t.stride()
    return View(t.data_ptr(), 0, s[1], s[2])


def _chains(state, slices, skip_empty=True):
    """The one pairing of launch chains (`_slices`) with the state's rows, for extend, verify and commit, padded and packed: (the
    chain's number, first sequence, end, plan, the state's rows, their positions: `_rows_of`) of every chain.  One chain, the usual
    call: the state itself, no views built.  `skip_empty`: a chain none of whose sequences has a token is left out."""
    if len(slices) == 1:
        return ((0,) + slices[0] + (state, state.pos),)
    return [(n, i, j, plan) + _rows_of(state, i, j, state.pos) for n, (i, j, plan) in enumerate(slices) if plan[0] or not skip_empty]


def _rows_chains(call, fn, prepared, state, slices, counts, left_padded, res, norm_eps, cu=None):
    """The rows of an extend or a verify (`call`: the key of `_ENTRY`) with per-sequence `counts` into `res`, one launch chain per
    slice of `slices`: the page rule, the one copy (the counts; packed, `cu`: the offsets), then `_causal_extend_ragged` or
    `_causal_packed` per chain.  Returns `res`."""
    if state.pages is not None:
        _page_rule(fn, state, counts)
    if res is None:   # (a padded verify takes its rows after the page rule, every other call before it: the order of allocations stays)
        res = prepared.q.new_empty(prepared.q.shape[:3] + prepared.v.shape[3:])
    # the one small copy of the call: the counts, or the offsets of a pack
    cnt, at = (torch.tensor(counts, dtype=torch.int32).to(res.device), None) if cu is None else _packed_offsets(cu, slices, res.device)
    several = len(slices) > 1
    p, c, out = prepared, cnt, res   # (one chain, the usual call: the caller's objects themselves)
    for n, i, j, plan, rows, pos in _chains(state, slices, cu is not None):   # (a padded chain runs without a token too)
        if cu is None:
            if several:
                p, c, out = prepared.part(i, j), cnt[i:j], res[i:j]
            _causal_extend_ragged(*p, rows, pos, c, plan, left_padded, out, norm_eps, call)
        else:
            if several:
                p, c, out = prepared.part(None, None, cu[i], cu[j]), cnt[at[n]:at[n] + j - i + 1], res[:, cu[i]:cu[j]]
            _causal_packed(*p, rows, pos, c, j - i, plan, out, norm_eps, call)
    return res


def _advance(state, counts):
    """The host mirror after every sequence took `counts[b]` tokens (the device positions were advanced by the launch chains)."""
    lengths = tuple([p + n for p, n in zip(state.lengths, counts)])
    state.lengths, state.seen = lengths, max(lengths)


def _extend_run(prepared, part, res, norm_eps, i, j, p, t_lo, t_hi, step_t):
    """Tokens [t_lo, t_hi) of the padded tensors as the next tokens of sequences i .. j - 1 (whose state `part` is), all at position
    p: the uniform launch chain, cut into consecutive calls of at most `step_t` tokens at chunk boundaries."""
    t0 = t_lo
    while t0 < t_hi:
        # the first piece fills the open chunk, so that every later one starts on a boundary
        t1 = min(t_hi, t0 + step_t - (p + t0 - t_lo) % 64)
        _causal_decode(*prepared.part(i, j, t0, t1, p + t0 - t_lo), part, res[i:j, t0:t1], norm_eps, True)
        t0 = t1


def _extend_step_t(nb, H, K, V):
    # tokens per call: whole chunks, so that nb H (K V / 64 + V) 4 bytes per token stay under the cap (and under the C ABI's 65535)
    per_tok = nb * H * (K * V // 64 + V) * 4
    return min(max(64, EXTEND_WS_CAP_BYTES // per_tok // 64 * 64), 65472)


def _extend_counts(fn, prepared, state, counts, left_padded, res, norm_eps):
    """Sequence b of a ragged state takes `counts[b]` of the T padded tokens: one ragged launch chain per batch slice.  A slice whose
    workspace would exceed `EXTEND_WS_CAP_BYTES` is not cut per sequence: the whole call then runs the uniform chain sequence by
    sequence (which cuts at chunk boundaries), and writes the padding rows itself."""
    B, T, H, K = prepared.q.shape
    V = prepared.v.shape[-1]
    Hk = prepared.k.shape[2]
    slices = _slices(fn, state, counts, H, prepared.mixf)
    lib = _lib.load()
    dt = _DTYPES[prepared.q.dtype]
    over = any(_extend_ragged_ws_bytes(lib, j - i, T, H, Hk, K, V, plan[1], dt) > EXTEND_WS_CAP_BYTES for i, j, plan in slices)
    if over and Hk != H:
        # grouped heads have no uniform chain to fall back to: the ragged chain window by window of whole chunks of tokens, every
        # sequence taking what it has in the window (this function again, on views; each window fits the cap)
        nb = min(B, _MAX_GRID_BH // H)
        step_t = _extend_step_t(nb, H, K, V)
        if T <= step_t:
            raise ValueError(f"{fn}: {nb} sequences x {T} tokens need a workspace beyond EXTEND_WS_CAP_BYTES={EXTEND_WS_CAP_BYTES} with "
                             "grouped heads: extend fewer sequences per call")
        for t0 in range(0, T, step_t):
            t1 = min(T, t0 + step_t)
            lo = [T - n if left_padded else 0 for n in counts]
            part = tuple(max(0, min(t1, a + n) - max(t0, a)) for a, n in zip(lo, counts))
            if any(part):
                _extend_counts(fn, prepared.part(None, None, t0, t1), state, part, left_padded, res[:, t0:t1], norm_eps)
            else:
                res[:, t0:t1].zero_()
        return res
    if over and isinstance(state, CausalStateView):
        raise ValueError(f"{fn}: {B} sequences x {T} tokens need a workspace beyond EXTEND_WS_CAP_BYTES={EXTEND_WS_CAP_BYTES}, and a view "
                         "of a pool has no sequential fallback: extend fewer tokens or sequences per call")
    if over:
        res.zero_()
        step_t = _extend_step_t(1, H, K, V)
        for b, _, p, part in _run_slices(state, state.lengths, 1):   # (sequence by sequence)
            n = counts[b]
            if n:
                t_lo = T - n if left_padded else 0
                _extend_run(prepared, part, res, norm_eps, b, b + 1, p, t_lo, t_lo + n, step_t)
        state.pos += torch.tensor(counts, dtype=torch.int32).to(state.pos.device, non_blocking=False)
    else:
        _rows_chains("extend", fn, prepared, state, slices, counts, left_padded, res, norm_eps)
    _advance(state, counts)
    return res


def mhla_causal_extend(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mixing_matrix: torch.Tensor, state: CausalState, *,
                       scale: Optional[float] = None, gate: Optional[torch.Tensor] = None, norm_weight: Optional[torch.Tensor] = None,
                       norm_eps: float = 1e-5, epilogue: Optional[bool] = None, counts=None, left_padded: bool = False,
                       cu_seqlens=None) -> torch.Tensor:
    """T >= 1 new tokens on an existing decode state in one call: q, k `[B, T, H, K]`, v (and `gate`) `[B, T, H, V]` of the tokens
    at positions `state.seen .. state.seen + T - 1`; returns those rows of `mhla_causal` over the whole sequence, `[B, T, H, V]`,
    updates `state` in place as T calls of `mhla_causal_step` would and adds T to `state.seen` -- the next turn of a
    conversation, a chunk of a long prompt, a draft to verify, in a number of launches that does not depend on T (at most seven).
    Exact fp32 products on the fp32 state (rows of the step's grade, never the stored 11-bit summaries), so `extend` and `step`
    may alternate freely; an empty state makes it a prefill in exact fp32.  T = 1 is `mhla_causal_step` itself (the same bits).
    Epilogue arguments, strided views, inference only and the IndexError of a sequence beyond the mixing matrix or the state's
    capacity (raised before anything is launched, the state untouched): as `mhla_causal_step`.  The workspace holds one fp32
    [K, V] tile per (b, h) and chunk touched after the first, plus the T fp32 output rows; an extension that would need more than
    `EXTEND_WS_CAP_BYTES` (256 MiB) is cut into consecutive calls at chunk boundaries.
    On a ragged state every sequence gets T new tokens, at positions `lengths[b] ..`.  Equal lengths: the uniform launch chain.
    Differing lengths: ONE ragged launch chain (at most six launches whatever B and the lengths), whose kernels read every
    sequence's position from `state.pos` and give each sequence the bits it would get alone in a batch of one; then T is added to the
    device positions (by the chain) and to `lengths`.
    counts (a list or a tensor of B ints in 0 .. T; a device tensor is read once, which synchronises; needs a ragged state --
    `state.to_ragged()` makes one -- that is not stale): sequence b takes `counts[b]` tokens only, rows `[0, counts[b])` of the
    padded tensors, or `[T - counts[b], T)` with `left_padded` -- a decoding slot beside a 256-token slice of a long prompt, drafts of
    different lengths, a slot that sits this call out (0: its state stays bit for bit).  The same single ragged chain, whatever
    the counts; one small host-to-device copy (the counts).  Rows outside a sequence's window are never read and come back as
    zeros; `state.pos` advances on the device, `lengths` by `counts`, `seen` to `max(lengths)`.  A count of 1 is that sequence's
    `mhla_causal_step` (the same bits as in a batch of one).  IndexError, before anything is launched and naming the
    sequences, when one would exceed the mixing matrix or the capacity.  All counts 0: nothing is launched, zeros are returned.
    Batches beyond one launch's (b, h) range are sliced; a ragged call whose workspace would exceed `EXTEND_WS_CAP_BYTES` is not cut
    per sequence but falls back to the uniform chain sequence by sequence (which cuts at chunk boundaries): the same rows and
    state within fp32 rounding, more launches.
    Grouped-query heads (k, v and the state on Hkv heads, as `mhla_causal_step`): always the ragged chain, on a uniform state too;
    beyond `EXTEND_WS_CAP_BYTES` it runs window by window of whole chunks of tokens instead of sequence by sequence.
    cu_seqlens (B + 1 ints as a sequence, a 1-D tensor -- read once -- or a `CausalVarlenPlan`, of which only the host `cu` is used;
    starts at 0, never decreases, ends at N; excludes `counts` and `left_padded`: ValueError): PACKED new tokens, the layout of a
    scheduler step of continuous batching and of the pack prefill.  q, k are `[1, N, H, K]`, v (and `gate`) `[1, N, H(kv), V]`, the
    state holds B sequences (ragged, not stale; a `CausalState`, or a view of a dense or an fp32 paged pool), and sequence b takes
    tokens `[cu[b], cu[b + 1])` at its own position -- none (equal neighbours): its state keeps every bit.  Returns `[1, N, H, V]`.
    No padding row is allocated, staged or written: the same ragged chain (at most six launches) with the fp32 rows staged
    `[H, N, V]`; every sequence's rows and state are BIT FOR BIT those of the padded call with `counts=` the pack's lengths.  One
    small host-to-device copy (the offsets).  Checks, IndexErrors and the page rule come before the first launch, in the order of
    `counts=`; all sequences empty: nothing is launched, zeros are returned.  A pack beyond one call's 65535 tokens, one launch's
    (b, h) range or `EXTEND_WS_CAP_BYTES` is cut BETWEEN sequences into consecutive chains (no bit changes); a single sequence
    beyond the token bound or the cap is a ValueError -- there is no cut inside a sequence.  Not on h16 pages (NotImplementedError,
    as the padded call)."""
    fn = "mhla_causal_extend"
    _decode_entry(fn, state, q, k, v, False, True, cu_seqlens is not None)
    if state.page_mult is not None:
        _refuse_h16(fn, state)
    B, T, H, K = q.shape
    V = v.shape[-1]
    if cu_seqlens is not None or counts is not None:
        cu, counts, prepared = _counts_prepare(fn, q, k, v, mixing_matrix, state, counts, left_padded, cu_seqlens, scale, gate, norm_weight,
                                               epilogue)
        if not any(counts):
            return torch.zeros((B, T, H, V), dtype=q.dtype, device=q.device)
        res = q.new_empty((B, T, H, V))
        if cu is None:   # (padded: the three strategies of `_extend_counts`)
            return _extend_counts(fn, prepared, state, counts, left_padded, res, norm_eps)
        slices = _slices(fn, state, counts, H, prepared.mixf, cu, (H, k.shape[2], K, V, _DTYPES[prepared.q.dtype]))
        _rows_chains("extend_packed", fn, prepared, state, slices, counts, False, res, norm_eps, cu)
        _advance(state, counts)
        return res
    if T == 1:
        return mhla_causal_step(q, k, v, mixing_matrix, state, scale=scale, gate=gate, norm_weight=norm_weight, norm_eps=norm_eps,
                                epilogue=epilogue)
    prepared = _decode_prepare(fn, q, k, v, mixing_matrix, state, scale, gate, norm_weight, epilogue)
    pos = prepared.pos
    res = q.new_empty((B, T, H, V))
    # (a view of a pool: always the ragged chain, which addresses through the slot map)
    if state.lengths is not None and (k.shape[2] != H or any(n != state.lengths[0] for n in state.lengths) or isinstance(state, CausalStateView)):
        return _extend_counts(fn, prepared, state, (T,) * B, False, res, norm_eps)
    if k.shape[2] != H:   # grouped heads have no uniform kernels: the ragged chain on the same storage, its positions filled on the device
        rag = CausalState(state.S, state.P, state.Cur, 0, 64, lengths=(pos,) * B,
                          pos=torch.full((B,), pos, dtype=torch.int32, device=q.device))
        _extend_counts(fn, prepared, rag, (T,) * B, False, res, norm_eps)
        state.seen = pos + T
        return res
    nb = min(B, _MAX_GRID_BH // H)
    step_t = _extend_step_t(nb, H, K, V)
    # (a uniform state: runs of the one length, `nb` sequences each)
    for i, j, p, part in _run_slices(state, state.lengths if state.lengths is not None else (pos,) * B, nb):
        _extend_run(prepared, part, res, norm_eps, i, j, p, 0, T, step_t)
    if state.lengths is not None:
        state.pos += T
        state.lengths = tuple(n + T for n in state.lengths)
    state.seen = pos + T
    return res


class CausalDraft:
    """What `mhla_causal_verify` hands to `mhla_causal_commit`: the draft's prepared `k`, `v` (REFERENCES to the tensors the verify
    read, or to their contiguous copies -- not copies of their own), `counts` (B ints), `left_padded`, and `lengths`, the state's
    lengths when the draft was verified, which a commit holds the state to; `view`, the `CausalStateView` the draft was verified on
    (None: a state of its own), which a commit holds the state to as well -- the same pool and the same slots; `cu`, the offsets of a
    draft verified with `cu_seqlens=` (None: padded) -- k, v are then the pack `[1, N, Hkv, *]` and sequence b's window is rows
    `[cu[b], cu[b + 1])`, `counts` their differences."""

    __slots__ = ("k", "v", "counts", "left_padded", "lengths", "view", "cu")

    def __init__(self, k, v, counts, left_padded, lengths, view=None, cu=None):
        self.k, self.v, self.counts, self.left_padded, self.lengths = k, v, tuple(counts), bool(left_padded), tuple(lengths)
        self.view = view
        self.cu = None if cu is None else tuple(cu)

    def __repr__(self):
        return (f"CausalDraft(counts={self.counts}, left_padded={self.left_padded}, lengths={self.lengths}"
                + ("" if self.cu is None else ", packed") + ")")


def mhla_causal_verify(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mixing_matrix: torch.Tensor, state: CausalState, *,
                       counts=None, left_padded: bool = False, scale: Optional[float] = None, gate: Optional[torch.Tensor] = None,
                       norm_weight: Optional[torch.Tensor] = None, norm_eps: float = 1e-5, epilogue: Optional[bool] = None,
                       cu_seqlens=None):
    """`(o, draft)`: the rows `mhla_causal_extend(q, k, v, mixing_matrix, state, counts=counts, left_padded=left_padded, ...)` would
    return, bit for bit, WITHOUT committing a token -- a draft of speculative, lookup or multi-token-prediction decoding to verify.
    `state` is untouched: `P`, `Cur`, `pos`, the finished chunks of `S`, `lengths` and `seen` are as before, so any call on it gives
    what it would have given (rows of `S` beyond a sequence's finished chunks are scribbled on; they are outside the state's
    contract, nothing reads them before a later call finishes them).  No copy of the state is made.
    state: a ragged one that is not stale (ValueError otherwise: `state.to_ragged()` makes one on the same storage).  counts (B ints
    in 0 .. T, default T for every sequence), left_padded, the epilogue arguments, strided views, inference only and the
    IndexErrors: as `mhla_causal_extend(counts=)` -- the WHOLE draft must fit the mixing matrix and the capacity.  The same six
    launches at most; all counts 0: nothing is launched.  Batches beyond one launch's (b, h) range are sliced; a call whose workspace
    would exceed `EXTEND_WS_CAP_BYTES` raises ValueError (drafts are short: there is no sequential fallback).
    `draft` (a `CausalDraft`) is what `mhla_causal_commit` takes to advance the state by an accepted prefix.  It holds references to
    k and v (or to the contiguous copies the call made), not copies: the caller must not overwrite k, v before the commit.
    cu_seqlens: PACKED drafts, as `mhla_causal_extend(cu_seqlens=)` -- tokens `[1, N, ...]`, sequence b's draft rows
    `[cu[b], cu[b + 1])`, rows `[1, N, H, V]`, bit for bit the padded verify's; the draft remembers the pack (`draft.cu`) and
    `mhla_causal_commit` reads it from there, `accept[b]` the accepted prefix of sequence b's window.  A pack beyond one call's limits
    is cut between sequences; a single sequence beyond them is a ValueError."""
    fn = "mhla_causal_verify"
    _decode_entry(fn, state, q, k, v, False, True, cu_seqlens is not None)
    if state.page_mult is not None:
        _refuse_h16(fn, state)
    B, T, H, K = q.shape
    V = v.shape[-1]
    packed = cu_seqlens is not None
    cu, counts, prepared = _counts_prepare(fn, q, k, v, mixing_matrix, state, (T,) * B if counts is None and not packed else counts, left_padded,
                                           cu_seqlens, scale, gate, norm_weight, epilogue)
    draft = CausalDraft(prepared.k, prepared.v, counts, left_padded, state.lengths, state if isinstance(state, CausalStateView) else None, cu)
    if not any(counts):
        return torch.zeros((B, T, H, V), dtype=q.dtype, device=q.device), draft
    if packed:
        slices = _slices(fn, state, counts, H, prepared.mixf, cu, (H, k.shape[2], K, V, _DTYPES[q.dtype]))
        return _rows_chains("verify_packed", fn, prepared, state, slices, counts, False, q.new_empty((B, T, H, V)), norm_eps, cu), draft
    slices = _slices(fn, state, counts, H, prepared.mixf)
    lib = _lib.load()
    need = max([_extend_ragged_ws_bytes(lib, j - i, T, H, k.shape[2], K, V, plan[1], _DTYPES[q.dtype]) for i, j, plan in slices])
    if need > EXTEND_WS_CAP_BYTES:
        raise ValueError(f"{fn}: a draft of T={T} tokens for {B} sequences needs a workspace of {need} bytes, more than "
                         f"EXTEND_WS_CAP_BYTES={EXTEND_WS_CAP_BYTES}: verify fewer tokens or sequences per call")
    return _rows_chains("verify", fn, prepared, state, slices, counts, left_padded, None, norm_eps), draft   # (None: the rows, taken after the page rule)


@_device_guard
def _launch_commit(k, v, mixf, state, pos, cnt, acc, B, plan, left_padded):
    """The one library call of a commit, one launch chain for the B sequences `state` (a batch slice) holds: `pos` their device
    positions, which the chain advances, `acc` the accepted counts on the device, `plan` the host values of `_ragged_plan` for them.
    Padded (the draft's k, v [B, T, ...]): `cnt` the draft's counts on the device, and `left_padded`.  Packed (`left_padded` None;
    k, v the chain's tokens of the draft's pack [1, N, ...]): `cnt` the sequences' B + 1 offsets, views with a zero batch stride."""
    lib = _lib.load()
    _, T, H, K = k.shape
    packed = left_padded is None
    view, dt = _view0 if packed else _view, _dtype_code(k)
    max_end, max_later, any_close, _ = plan
    ws = _ws(lib.mhla_causal_commit_ragged_ws_bytes(B, dt), k.device)
    name, _, head = _state_args("commit_packed" if packed else "commit", mixf, state, (pos.data_ptr(),), packed)
    rc = getattr(lib, name)(view(k), view(v), *head, cnt.data_ptr(), acc.data_ptr(), T, max_end, max_later, int(any_close),
                            *(() if packed else (int(bool(left_padded)),)), ws.data_ptr(), ws.numel() * 4, B, H, K, v.shape[-1],
                            state.chunk_size, dt, _stream())
    _lib.check(rc, name)


def mhla_causal_commit(draft: CausalDraft, mixing_matrix: torch.Tensor, state: CausalState, accept) -> CausalState:
    """Advance `state` by the first `accept[b]` tokens of every sequence's verified draft (`draft`: what `mhla_causal_verify`
    returned for this state); returns `state`.  Afterwards the state -- every sequence's finished chunks, `P`, `Cur`, `pos`, `lengths`,
    `seen` -- is bit for bit the one `mhla_causal_extend(..., counts=accept)` leaves when called instead of the verify.  At most four
    launches, which read the draft's k and v only; no rows are computed.
    accept: B ints, or a tensor (read once, which synchronises a device tensor), 0 <= accept[b] <= draft.counts[b]; anything else is
    a ValueError, as is a state that moved since the verify (`state.lengths != draft.lengths`), a uniform or a stale state.  All
    zeros (every draft rejected): nothing is launched and the state is bit for bit as before."""
    fn = "mhla_causal_commit"
    if not isinstance(draft, CausalDraft):
        raise TypeError(f"{fn}: draft must be a CausalDraft (what mhla_causal_verify returns), got {type(draft).__name__}")
    if not isinstance(state, CausalState):
        raise TypeError(f"{fn}: state must be a CausalState, got {type(state).__name__}")
    if isinstance(state, PagedCausalState):
        _refuse_paged_pool(fn, state)
    if state.page_mult is not None:
        _refuse_h16(fn, state)
    if isinstance(state, CausalStateView):
        state._host_slots(fn)
    if state.stale:
        state._refuse_stale(fn)
    if state.lengths is None:
        raise ValueError(f"{fn}: the state is uniform ({state!r}); a draft is verified on, and committed to, a ragged state")
    seen_on, given = ((x.pool, x.slots) if isinstance(x, CausalStateView) else None for x in (draft.view, state))
    if seen_on != given:   # (pools compare by identity)
        raise ValueError(f"{fn}: the draft was verified on {draft.view if draft.view is not None else 'a state of its own'!r}, "
                         f"the commit is given {state!r}: pass the view (the same pool and slots) the verify took")
    B = len(draft.counts)
    accept = _int_tuple(fn, "accept", accept, B, draft.counts)
    if tuple(state.lengths) != draft.lengths:
        raise ValueError(f"{fn}: the state moved since the verify: lengths {state.lengths}, the draft was verified at {draft.lengths}")
    if not any(accept):
        return state
    k, v = draft.k, draft.v
    _, T, H, K = k.shape
    dims = state.dims
    if (state.rows if isinstance(state, CausalStateView) else dims[0]) != B or dims[1:] != (H, dims[2], K, v.shape[-1]) or state.device != k.device:
        raise ValueError(f"{fn}: state is {state!r}, the draft has B={B} H={H} K={K} V={v.shape[-1]} on {k.device}")
    if mixing_matrix.dim() < 2 or mixing_matrix.device != k.device:
        raise ValueError(f"{fn}: mixing_matrix must be [L, L(, 1, 1, 1, 1)] on {k.device}, got {tuple(mixing_matrix.shape)} on "
                         f"{mixing_matrix.device}")
    _require_gpu(k, v, mixing_matrix)
    mixf = _mix2d(mixing_matrix)
    cu = draft.cu
    slices = _slices(fn, state, accept, H, mixf, cu, rows=True)
    if state.pages is not None:
        _page_rule(fn, state, accept)
    # the one small copy of the call: the draft's counts over `accept`, or the offsets of a pack followed by `accept`
    if cu is None:
        both = torch.tensor((draft.counts, accept), dtype=torch.int32).to(k.device)
        cnt, acc = both[0], both[1]
    else:
        cnt, at = _packed_offsets(cu, slices, k.device, accept)
        acc = cnt[len(cnt) - B:]
    several, left = len(slices) > 1, draft.left_padded if cu is None else None
    k_, v_, c, a = k, v, cnt, acc   # (one chain, the usual call: the caller's objects themselves)
    for n, i, j, plan, rows, pos in _chains(state, slices):   # (a slice of which nothing was accepted is left alone)
        if several and cu is None:
            k_, v_, c, a = k[i:j], v[i:j], cnt[i:j], acc[i:j]
        elif several:
            k_, v_, c, a = k[:, cu[i]:cu[j]], v[:, cu[i]:cu[j]], cnt[at[n]:at[n] + j - i + 1], acc[i:j]
        _launch_commit(k_, v_, mixf, rows, pos, c, a, j - i, plan, left)
    _advance(state, accept)
    return state


# ------------------------------------------------------------------------------------------
# per-head RMSNorm x swish gate
# ------------------------------------------------------------------------------------------
def _rmsnorm_gate_bwd(x, g, wf, dy, eps, w_dtype):
    """mhla_rmsnorm_gate_bwd over the rows of x [..., D] (x and the gate g contiguous, g / the fp32 weight wf may be None):
    (dx, dg, dw), dw summed from the kernel's fp32 partial rows and cast to the weight's dtype."""
    lib = _lib.load()
    D = x.shape[-1]
    rows = x.numel() // D
    dyc = dy.contiguous().to(x.dtype)
    dx = torch.empty_like(x)
    dg = torch.empty_like(x) if g is not None else None
    dwp = torch.empty((lib.mhla_rmsnorm_gate_dw_rows(rows), D), dtype=torch.float32, device=x.device)
    rc = lib.mhla_rmsnorm_gate_bwd(x.data_ptr(), D, _ptr(g), D, _ptr(wf), dyc.data_ptr(), D, dx.data_ptr(), D, _ptr(dg), D,
                                   dwp.data_ptr(), rows, D, eps, _dtype_code(x), _stream())
    _lib.check(rc, "mhla_rmsnorm_gate_bwd")
    return dx, dg, (dwp.sum(0).to(w_dtype) if wf is not None else None)


class _RmsNormGate(torch.autograd.Function):
    @staticmethod
    @_device_guard
    def forward(ctx, x, g, weight, eps):
        lib = _lib.load()
        _require_gpu(x, g, weight)
        D = x.shape[-1]
        xc = x.contiguous()
        gc = g.contiguous().to(x.dtype) if g is not None else None
        wf = _f32(weight)
        rows = xc.numel() // D
        y = torch.empty_like(xc)
        rc = lib.mhla_rmsnorm_gate_fwd(xc.data_ptr(), D, _ptr(gc), D, _ptr(wf), y.data_ptr(), D, None, rows, D,
                                       float(eps), _dtype_code(xc), _stream())
        _lib.check(rc, "mhla_rmsnorm_gate_fwd")
        ctx.save_for_backward(xc, gc, wf)
        ctx.cfg = (float(eps), weight.dtype if weight is not None else None)
        return y

    @staticmethod
    @_device_guard
    def backward(ctx, dy):
        xc, gc, wf = ctx.saved_tensors
        eps, w_dtype = ctx.cfg
        return (*_rmsnorm_gate_bwd(xc, gc, wf, dy, eps, w_dtype), None)


def rmsnorm_gate(x: torch.Tensor, g: Optional[torch.Tensor], weight: Optional[torch.Tensor],
                 eps: float = 1e-5) -> torch.Tensor:
    """y = x * rsqrt(mean(x^2, -1) + eps) * weight [* g * sigmoid(g)] over the last dim (<= 512).
    FusedRMSNormGated math (mhla_nlp/fla/modules/fused_norm_gate.py:77-99); with g=None it is Wan's
    per-head g_norm (wan/model.py:181-196)."""
    return _RmsNormGate.apply(x, g, weight, eps)
