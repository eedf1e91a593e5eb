"""Drop-in for the fla attention layer `MHLA` (mhla_nlp/fla/layers/mhla.py:29-365).

Same constructor, `forward(hidden_states, attention_mask, past_key_values, use_cache,
output_attentions, **kw) -> (o, None, past_key_values)` and parameter names
(`q_proj/k_proj/v_proj/g_proj/o_proj.weight`, `mixing_matrix [32,32,1,1,1,1]` (side = `max_chunks`),
`g_norm_swish_gate.weight`).  The causal operator and the per-head RMSNorm x swish gate run as HIP
kernels; rotary is plain tensor math (NeoX half rotation, rotary.py:20-32) -- no Triton.

Deviations, all documented in SURVEY.md: sequences of <= 64 tokens use the single-chunk case of the
chunk operator (the reference's token-recurrent form equals it only on the first chunk and ignores
its initial state); `exact_decoding=True` (not in the reference) replaces that branch, under `use_cache`, by a prefill that
keeps a `CausalState` and exact single-token steps.  `use_short_conv=True` (off in the shipped configuration; the reference's
ShortConvolution is a sibling fla module outside the MHLA hot path) is served by a plain-PyTorch
`ShortConvolution` with the reference's parameters and cache protocol (no HIP kernel: not on the path).
"""
import warnings
from typing import Dict, NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from ..ops import (CausalState, PagedCausalState, _counts_fit, _cu_host, _mix2d, _runs, _slot_tuple, causal_varlen_plan, mhla_causal_prefill, featmap_rotary, featmap_rotary_decode, mhla_causal, mhla_causal_commit, mhla_causal_extend, mhla_causal_normgate, mhla_causal_state, mhla_causal_step, mhla_causal_verify,
                   mhla_causal_step_dev, naive_recurrent_mhla, rmsnorm_gate)
from ..weights import causal_mixing_init


class FusedRMSNormGated(nn.Module):
    """Parameter holder + HIP kernel call (fused_norm_gate.py:997-1058)."""

    def __init__(self, hidden_size, elementwise_affine=True, eps=1e-5, activation="swish"):
        super().__init__()
        if activation not in ("swish", "silu"):
            raise ValueError(f"Unsupported activation: {activation}")
        self.hidden_size = hidden_size
        self.eps = eps
        self.activation = activation
        if elementwise_affine:
            self.weight = nn.Parameter(torch.ones(hidden_size))
        else:
            self.register_parameter("weight", None)
        self.register_parameter("bias", None)

    def forward(self, x, g):
        return rmsnorm_gate(x, g, self.weight, self.eps)


class RotaryEmbedding(nn.Module):
    """NeoX-style rotary, non-interleaved, base 10000 (rotary.py:330-431): fp32 inv_freq, cos/sin cached
    in the activation dtype."""

    def __init__(self, dim: int, base: float = 10000.0):
        super().__init__()
        self.dim = dim
        self.base = base
        self._cache: Optional[Tuple] = None

    def _tables(self, seqlen: int, device, dtype):
        c = self._cache
        if c is None or c[0] < seqlen or c[1] != device or c[2] != dtype:
            inv_freq = 1.0 / (self.base ** (torch.arange(0, self.dim, 2, device=device, dtype=torch.float32) / self.dim))
            t = torch.arange(seqlen, device=device, dtype=torch.float32)
            fr = torch.outer(t, inv_freq)
            c = (seqlen, device, dtype, torch.cos(fr).to(dtype), torch.sin(fr).to(dtype))
            self._cache = c
        return c[3], c[4]

    def forward(self, q, k, seqlen_offset: int = 0, max_seqlen: Optional[int] = None, cu_seqlens=None, positions=None):
        """`positions` [T] (long): the rotary position of every token row -- packed sequences restart per sequence
        (rotary.py:68-72 with cu_seqlens), padded decoding adds each sequence's own offset (layers/mhla.py:305-309)."""
        T = q.shape[1]
        if positions is not None:
            cos, sin = self._tables(max(max_seqlen or 0, T + int(seqlen_offset if isinstance(seqlen_offset, int) else 0)), q.device, q.dtype)
            cos, sin = cos.index_select(0, positions)[None, :, None, :], sin.index_select(0, positions)[None, :, None, :]
        else:
            cos, sin = self._tables(max(max_seqlen or 0, T + seqlen_offset), q.device, q.dtype)
            cos = cos[seqlen_offset:seqlen_offset + T][None, :, None, :]
            sin = sin[seqlen_offset:seqlen_offset + T][None, :, None, :]

        def rot(x):
            x1, x2 = x.chunk(2, dim=-1)
            return torch.cat((x1 * cos - x2 * sin, x2 * cos + x1 * sin), dim=-1)

        return rot(q), rot(k)


class ShortConvolution(nn.Conv1d):
    """Depthwise causal 1-D convolution (+ SiLU) of `fla/modules/convolution.py:794-1010` in plain PyTorch: parameters
    `weight [D, 1, W]` (+ `bias`), `forward(x [B, T, D], residual, mask, cache [N, D, W], output_final_state, cu_seqlens)
    -> (y, cache)`.  y_t = act(sum_i w[i] x[t - (W - 1) + i] + b); positions before a sequence start read the cache's last
    W - 1 columns (zeros without a cache); with `cu_seqlens` (B = 1) the convolution does not cross sequence boundaries; a
    single new token per sequence (B T == N) is the decoding step, which rolls the cache in place (:963-1002).  Outside the
    MHLA hot path (SURVEY.md 2.3 marks it OUT), hence no HIP kernel."""

    def __init__(self, hidden_size: int, kernel_size: int, bias: bool = False, activation: Optional[str] = "silu", **kwargs):
        super().__init__(hidden_size, hidden_size, kernel_size, groups=hidden_size, bias=bias, padding=kernel_size - 1)
        self.hidden_size = hidden_size
        if activation is not None and activation not in ("silu", "swish"):
            raise ValueError(f"Activation `{activation}` not supported yet.")
        self.activation = activation

    def _act(self, y):
        return F.silu(y) if self.activation is not None else y

    def forward(self, x, residual=None, mask=None, cache=None, output_final_state=False, cu_seqlens=None, **kwargs):
        B, T, D = x.shape
        W = self.kernel_size[0]
        N = B if cu_seqlens is None else len(cu_seqlens) - 1
        if mask is not None:
            if cu_seqlens is not None:
                raise ValueError("`mask` and `cu_seqlens` cannot be provided at the same time")
            x = x * mask.unsqueeze(-1)
        w = self.weight.squeeze(1)                                           # [D, W]
        if B * T == N:                                                       # decoding step (:927-935)
            xt = x.reshape(N, D)
            if cache is None:
                cache = x.new_zeros(N, D, W)
            cache.copy_(torch.cat([cache[..., 1:], xt.unsqueeze(-1)], dim=-1))
            y = (cache * w).sum(-1)
            if self.bias is not None:
                y = y + self.bias
            y = self._act(y).reshape(x.shape)
            return (y + residual if residual is not None else y), cache

        def one(seq, init):                                                  # seq [b, t, D], init [b, D, W] or None
            hist = init[..., 1:] if init is not None else seq.new_zeros(seq.shape[0], D, W - 1)
            xin = torch.cat([hist.to(seq.dtype), seq.transpose(1, 2)], dim=-1)
            y = F.conv1d(xin, self.weight, self.bias, groups=D).transpose(1, 2)
            full = torch.cat([init.to(seq.dtype) if init is not None else seq.new_zeros(seq.shape[0], D, W), seq.transpose(1, 2)], dim=-1)
            return self._act(y), full[..., -W:]

        if cu_seqlens is None:
            y, final = one(x, cache)
        else:
            ys, finals = [], []
            cu = [int(c) for c in cu_seqlens]
            for i in range(N):
                yi, fi = one(x[:, cu[i]:cu[i + 1]], None if cache is None else cache[i:i + 1])
                ys.append(yi)
                finals.append(fi)
            y, final = torch.cat(ys, dim=1), torch.cat(finals, dim=0)
        if residual is not None:
            y = y + residual
        return y, (final if output_final_state else None)

    @property
    def state_size(self) -> int:
        return self.hidden_size * self.kernel_size[0]


class DecodeCache:
    """Minimal list-backed cache with the protocol the layer uses (`fla.models.utils.Cache` has the same one): `len(cache)`
    layers hold a state, `cache[i]` is layer i's `{"recurrent_state", "conv_state"}`, `get_seq_length(i)` the tokens layer i
    has seen, `update(...)` stores a layer's state and adds `offset` tokens to its count.
    `device_positions=True` (layers built with `exact_decoding=True`): after the prefill every one-token call is a
    device-positioned step (`mhla_causal_step_dev`: the q / k prologue and the norm x gate epilogue inside its three launches) that
    reads no host position and never synchronises, so a whole decode step can be captured in `torch.cuda.graph` and replayed
    once per token.  The prefill leaves a ragged state plus, in the layer's entry, what the steps read: the clamped,
    lower-triangular fp32 mixing matrix and the rotary tables of 64 x capacity rows.  Neither the states' host mirrors nor this
    cache's token counts move during such steps (a replay runs no Python): `sync()` brings both up, with the one device-to-host
    copy per layer of the whole generation.
    `packed_prefill=True` (layers built with `exact_decoding=True` and `isolate_sequences=True`): the call on the empty cache may
    carry `cu_seqlens` (B = 1) or an `attention_mask`, which the layer unpads to a pack -- a packed exact prefill: the operator
    over the pack, every sequence alone, and the ragged decode state of all of them from one launch chain
    (`mhla_causal_state(cu_seqlens=)`); later calls are `[sequences, T', D]` on that state.  Off (the default), such a call is
    refused as before.
    Speculative calls (`MHLA.forward(..., speculative=True)`) leave a verified draft in every layer's entry (`"draft"`) and move
    neither the states nor the token counts: `commit(accept)` advances every layer by the accepted prefix, `discard()` drops the
    drafts; until one of them, any other call on those layers is refused."""

    def __init__(self, device_positions: bool = False, packed_prefill: bool = False):
        self.states, self._seen = [], []
        self.device_positions = bool(device_positions)
        self.packed_prefill = bool(packed_prefill)

    def sync(self):
        """After device-positioned steps: `CausalState.sync()` on every layer's state and the tokens they advanced by added to
        this cache's counts.  Raises the first IndexError of a state that was stepped beyond its capacity, after all are synced."""
        err = None
        for i, entry in enumerate(self.states):
            st = entry.get("recurrent_state")
            if isinstance(st, CausalState) and st.stale:
                before = st.seen
                try:
                    st.sync()
                except IndexError as e:
                    err = err or e
                self._seen[i] += st.seen - before
        if err is not None:
            raise err
        return self

    def commit(self, accept):
        """After a speculative call: `mhla_causal_commit` of every layer that holds a draft with the first `accept[b]` tokens of
        sequence b's draft (B ints, or a tensor read once here for all layers), what the furthest sequence grew added to the
        layer's token count, and the drafts dropped."""
        accept = tuple(int(n) for n in (accept.tolist() if isinstance(accept, torch.Tensor) else accept))
        for i, entry in enumerate(self.states):
            if entry.get("draft") is not None:
                st = entry["recurrent_state"]
                before = st.seen
                mhla_causal_commit(entry["draft"], entry["draft_mix"], st, accept)
                self._seen[i] += st.seen - before
        return self.discard()

    def discard(self):
        """Drop every layer's pending draft: the states are as they were before the speculative call."""
        for entry in self.states:
            entry.pop("draft", None)
            entry.pop("draft_mix", None)
        return self

    def __len__(self):
        return len(self.states)

    def __getitem__(self, layer_idx):
        return self.states[layer_idx]

    def get_seq_length(self, layer_idx=0):
        layer_idx = layer_idx or 0
        return self._seen[layer_idx] if layer_idx < len(self._seen) else 0

    def update(self, recurrent_state=None, conv_state=None, layer_idx=0, offset=1, **kwargs):
        layer_idx = layer_idx or 0
        while len(self.states) <= layer_idx:
            self.states.append(dict(recurrent_state=None, conv_state=None))
            self._seen.append(0)
        self.states[layer_idx] = dict(recurrent_state=recurrent_state, conv_state=conv_state)
        self._seen[layer_idx] += int(offset)
        return self.states[layer_idx]


class _PoolStep(NamedTuple):
    """What `PagedDecodeCache.schedule` declared for the next model step."""
    slots: Tuple[int, ...]               # the request (slot of every layer's pool) of every sequence of the pack
    cu: Tuple[int, ...]                  # the pack's offsets, validated
    counts: Tuple[int, ...]              # tokens per sequence
    off_dev: torch.Tensor                # `cu` on the device (int32), uploaded once for all layers
    map_dev: torch.Tensor                # `slots` on the device (int32), likewise
    ran: set                             # the layers that have run the step


class PagedDecodeCache:
    """The cache of a model that serves requests by CONTINUOUS BATCHING (layers built with `exact_decoding=True`): one fp32-paged
    `PagedCausalState` of `n_slots` slots, `capacity_chunks` chunks a slot and `n_pages` pages per layer -- created on the layer's
    first call from its `(num_kv_heads with grouped_state, else num_heads; head_k_dim; head_v_dim)` --, and a request lives in the
    same slot of every layer's pool.  A model step is a PACK of new tokens, `hidden_states [1, N, D]`:
        cache.schedule(slots, cu_seqlens)   # request slots[b] takes rows cu[b] .. cu[b + 1] of the next pack (none: it sits the step out)
        model(input_ids [1, N], cache=cache)
    and every layer then runs `featmap_rotary_decode` (one launch: feature map and rotary of q and k at the positions its pool holds on
    the device) and `mhla_causal_extend(cu_seqlens=)` on `pool.at(slots)` in place -- a decoding request's one token beside a slice of
    a long prompt beside a fresh request, which is simply an empty slot.  `schedule` validates (ValueError, no state moves: distinct
    slots in range; offsets from 0 that never decrease, one more than slots; their end is held against N when the model is called) and
    uploads offsets and slot map ONCE for all layers.  Every layer runs exactly once between two `schedule` calls: a layer that runs
    twice or without a schedule, and a `schedule` while only some layers have run the last one, are ValueErrors.
    Every pool gets the same page-rule calls, so all layers' page tables are equal; what the operators refuse (`PoolExhausted`, the
    IndexError of a slot beyond the capacity or the mixing matrix) is raised by layer 0 before anything of the step is launched.
    `lengths`: tokens per slot (the host mirror of layer 0's pool); `pages_free`; `pool(i)`: layer i's pool (`swap_out` and the
    like stay available there); `release(slots)` empties slots of every layer for new requests; `fork(src, dst)` copies a slot
    (a shared prompt prefix) in every layer without copying a page.  h16 pages are refused: the extend has no form on them."""

    def __init__(self, n_slots: int, capacity_chunks: int, n_pages: int, device="cuda", page_format: str = "fp32"):
        if page_format != "fp32":
            raise ValueError(f"PagedDecodeCache: page_format {page_format!r}: the layer step is an extend, which runs on fp32 pages only")
        if min(int(n_slots), int(capacity_chunks), int(n_pages)) < 1:
            raise ValueError(f"PagedDecodeCache: non-positive size n_slots={n_slots} capacity_chunks={capacity_chunks} n_pages={n_pages}")
        self.n_slots, self.capacity_chunks, self.n_pages, self.device = int(n_slots), int(capacity_chunks), int(n_pages), torch.device(device)
        self._pools, self._rotary, self._step = [], [], None

    def schedule(self, slots, cu_seqlens) -> "PagedDecodeCache":
        fn = "PagedDecodeCache.schedule"
        slots = _slot_tuple(fn, slots, self.n_slots)
        cu = _cu_host(cu_seqlens)
        if len(cu) != len(slots) + 1:
            raise ValueError(f"{fn}: cu_seqlens has {len(cu)} entries for {len(slots)} slots (one more than slots)")
        last = self._step
        if last is not None and last.ran and last.ran != set(range(len(self._pools))):
            raise ValueError(f"{fn}: layers {sorted(set(range(len(self._pools))) - last.ran)} have not run the last scheduled step (every "
                             "layer runs exactly once between two schedule calls)")
        both = torch.tensor(cu + slots, dtype=torch.int32).to(self.device)   # (one small copy for the step, all layers)
        self._step = _PoolStep(slots, cu, tuple(b - a for a, b in zip(cu, cu[1:])), both[:len(cu)], both[len(cu):], set())
        return self

    def _layer_step(self, layer_idx: int, n_tokens: int, dims):
        """Layer `layer_idx`'s turn in the scheduled step (checked: a schedule, whose end is the pack's token count, and which this
        layer has not run): (the step, the view of this layer's pool -- created on first use with `dims` = (heads, K, V))."""
        fn, step = "MHLA.forward on a PagedDecodeCache", self._step
        if step is None:
            raise ValueError(f"{fn}: no step is scheduled: cache.schedule(slots, cu_seqlens) declares every model step")
        if layer_idx in step.ran:
            raise ValueError(f"{fn}: layer {layer_idx} has already run the scheduled step (every layer runs exactly once between two schedule calls)")
        if step.cu[-1] != n_tokens:
            raise ValueError(f"{fn}: the scheduled cu_seqlens ends at {step.cu[-1]}, the pack has N = {n_tokens} tokens")
        while len(self._pools) <= layer_idx:
            self._pools.append(None)
            self._rotary.append(None)
        if self._pools[layer_idx] is None:
            self._pools[layer_idx] = PagedCausalState.empty(self.n_slots, *dims, self.capacity_chunks, self.n_pages, self.device)
        view = self._pools[layer_idx].at(step.slots)
        view._map = step.map_dev   # (the step's upload, not one per layer)
        return step, view

    def _tables(self, layer_idx: int, rotary, like):
        """Layer `layer_idx`'s rotary tables of 64 x capacity rows in the dtype of `like`, built once and kept."""
        kept = self._rotary[layer_idx]
        if kept is None or kept[0].dtype != like.dtype or kept[0].device != like.device:
            rows = 64 * self.capacity_chunks
            cos, sin = rotary._tables(rows, like.device, like.dtype)
            kept = self._rotary[layer_idx] = (cos[:rows], sin[:rows])
        return kept

    @property
    def lengths(self) -> Tuple[int, ...]:
        return self._pools[0].lengths if self._pools and self._pools[0] is not None else (0,) * self.n_slots

    @property
    def pages_free(self) -> int:
        return self._pools[0].pages_free if self._pools and self._pools[0] is not None else self.n_pages

    def pool(self, layer_idx: int) -> PagedCausalState:
        return self._pools[layer_idx]

    def release(self, slots) -> "PagedDecodeCache":
        """`PagedCausalState.reset(slots)` on every layer's pool: the slots are empty, their pages free."""
        slots = _slot_tuple("PagedDecodeCache.release", slots, self.n_slots)
        for p in self._pools:
            if p is not None:
                p.reset(slots)
        return self

    def fork(self, src: int, dst: int) -> "PagedDecodeCache":
        """`PagedCausalState.fork(src, dst)` on every layer's pool."""
        _slot_tuple("PagedDecodeCache.fork", (src, dst), self.n_slots)
        for p in self._pools:
            if p is not None:
                p.fork(src, dst)
        return self

    def __len__(self):
        return sum(p is not None for p in self._pools)

    def get_seq_length(self, layer_idx=0):
        return max(self.lengths)

    def __repr__(self):
        return (f"PagedDecodeCache(n_slots={self.n_slots}, capacity_chunks={self.capacity_chunks}, n_pages={self.n_pages}, layers={len(self)}, "
                f"lengths={self.lengths}, pages_free={self.pages_free})")


def _elu1(x):
    return F.elu(x) + 1


class _Call(NamedTuple):
    """The kind of a `MHLA.forward` call, as `_classify_call` finds it."""
    exact: bool                          # exact_decoding with use_cache and a cache: a prefill, or a step / extension on `state`
    state: Optional[CausalState]         # the decode state this layer's cache entry holds (exact calls only)
    ragged: bool                         # a left-padded prefill, or a call on a ragged state: every sequence at positions of its own
    lengths: Optional[list]              # the left-padded prefill: tokens per sequence ...
    keep: Optional[torch.Tensor]         # ... and its [B, T] mask of real tokens
    token_counts: Optional[Tuple[int, ...]]   # validated; only on a cached ragged state
    seen: int                            # tokens `state` held before the call
    packed: bool = False                 # the packed exact prefill (DecodeCache(packed_prefill=True)): a pack in, a ragged state out


class _RotaryRows(NamedTuple):
    """Where `MHLA._rotary_rows` puts every token row of a call."""
    positions: Optional[torch.Tensor]    # the rotary position of every row (long, flattened), None: seqlen_offset .. seqlen_offset + T
    table_len: int                       # rows of the cos / sin tables the call needs
    seqlen_offset: int
    keep: Optional[torch.Tensor]         # token_counts: [B, T] mask of the rows each sequence takes


class MHLA(nn.Module):
    def __init__(self, mode: str = "chunk", hidden_size: int = 1024, expand_k: float = 0.5, expand_v: float = 1.0,
                 num_heads: int = 4, num_kv_heads: Optional[int] = None, feature_map: Optional[str] = None,
                 use_short_conv: bool = False, conv_size: int = 4, conv_bias: bool = False,
                 use_output_gate: bool = True, gate_fn: str = "swish", elementwise_affine: Optional[bool] = True,
                 norm_eps: float = 1e-5, gate_logit_normalizer: int = 16, gate_low_rank_dim: int = 16,
                 clamp_min: Optional[float] = None, fuse_norm: bool = True, layer_idx: int = None, max_chunks: int = 32,
                 summaries: str = "tf32", exact_decoding: bool = False, isolate_sequences: bool = False,
                 grouped_state: bool = False):
        """`max_chunks` (not in the reference, default = its hard-coded 32): side of the mixing matrix, i.e. the longest
        sequence is 64 * max_chunks tokens -- 128 for the 8192-token configuration of BASELINE.json configs[4], which the
        reference layer itself cannot run (layers/mhla.py:196-200); the operator accepts any [n, n] matrix (naive.py:55).
        `summaries` (not in the reference): "tf32" (default) stores the operator's chunk summaries with 11 significand bits in 2
        bytes (the precision of the reference's TF32 matmuls), "split" with >= 16 bits in 4 bytes (bf16 hi + lo pairs, naive.py:39);
        "bf16" opts into the reduced-precision variant (2-3e-3 of the output's maximum) -- see mhla_amd.mhla_causal.
        `exact_decoding` (not in the reference, default off: nothing changes): with `use_cache=True` and a cache
        (`past_key_values`, e.g. `DecodeCache`; `layer_idx` set), a call on an empty cache -- of any length -- is a prefill: the
        chunk operator as otherwise, plus a `CausalState` (ops.py: 4 K V bytes per finished chunk and head, fp32) stored as the
        cache's `recurrent_state`; a later call of one token runs `mhla_causal_step` (norm x gate fused when
        `fuse_norm_and_gate`) and returns exactly the row the chunk operator over the whole sequence would.  A later call of
        several tokens runs `mhla_causal_extend` once (the same epilogue; launches independent of the token count).
        Padding: the prefill (the call on an empty cache) may carry a LEFT-padded `attention_mask` (each row zeros, then ones;
        anything else, or `use_short_conv`, raises NotImplementedError).  Every sequence then runs alone -- its own rotary
        positions, the operator over its real tokens only, zeros at the padding rows of the output; sequences never mix, unlike
        the packed batch of the non-exact path -- and the state is ragged (`CausalState.lengths`): later calls step all sequences
        together, each at its own position, and do not read the mask beyond its shape.  An all-ones mask gives a uniform state,
        and a padding mask on a call whose cached state is uniform raises NotImplementedError.  Steps and extensions are
        inference only (call under `torch.no_grad()`).  Adds no parameters.
        On a cached ragged state `forward(..., token_counts=[n_0, ...])` (through `**kwargs`; B ints in 0 .. T, ignored anywhere
        else) gives every sequence its own number of the call's tokens, RIGHT-aligned as the left-padded prefill: sequence b takes
        rows `[T - n_b, T)` at positions `pos_b ..` (its own rotary rows), in one `mhla_causal_extend(counts=, left_padded=True)`
        launch chain whatever the counts; the output is zero at padding rows, n_b = 0 leaves that sequence's state untouched, and
        the cache's token count grows by what the longest sequence grew.  `use_short_conv` raises NotImplementedError.
        On a cached decode state `forward(..., speculative=True)` (through `**kwargs`; ignored without `exact_decoding`) is a VERIFY
        of a draft: the output of the same call without the flag (rotary rows and `token_counts` handled alike), from
        `mhla_causal_verify` -- neither the state nor the cache's token count moves, and the draft stays in the layer's cache entry
        until `DecodeCache.commit(accept)` advances the state by each sequence's accepted prefix or `DecodeCache.discard()` drops
        it.  A uniform cached state is replaced by `state.to_ragged()` (the same storage).  A new speculative call replaces a
        pending draft; any other call on an entry with one raises ValueError.  `use_short_conv`, a
        `DecodeCache(device_positions=True)` and an empty cache raise NotImplementedError.
        With a `DecodeCache(device_positions=True)` the one-token calls after the prefill are device-positioned steps (see
        `DecodeCache`; capturable in a graph); they do not reassign `mixing_matrix.data` -- generation does not change the weights
        -- and calls of several tokens on such a cache, `use_short_conv` and `head_k_dim % 8 != 0` raise NotImplementedError.
        `isolate_sequences` (not in the reference, default off: nothing changes): a call with `cu_seqlens`, given or made by
        unpadding an `attention_mask`, runs the operator over every sequence of the pack alone (`mhla_causal(cu_seqlens=)`:
        each sequence's chunks cut from its own start, rows 0.. of the mixing matrix, nothing of its neighbours -- what
        `exact_decoding` evaluates) instead of over the pack as one sequence; calls of <= 64 tokens then use the chunk operator
        too and return no recurrent state.  `varlen_plan=` (through `**kwargs`): a `CausalVarlenPlan` built once for all layers.
        With `use_cache` a call that carries an `attention_mask` or `cu_seqlens` raises NotImplementedError -- the `exact_decoding`
        prefill of a padded batch included -- unless the layer has `exact_decoding` too and the cache is a
        `DecodeCache(packed_prefill=True)`: the call on the empty cache is then a packed exact prefill (`cu_seqlens` with B = 1, or
        an `attention_mask`, unpadded to a pack and re-padded on the way out): the operator over the pack, the ragged decode state
        of every sequence from one launch chain, rotary rows per sequence, and the cache counts the longest sequence; later calls
        are `[sequences, T', D]` on that state and read no mask.  `use_short_conv` there, and `cu_seqlens` on a cache that already
        holds a state, raise NotImplementedError.
        With a `PagedDecodeCache` (recognised by its type alone; `exact_decoding` and `use_cache`, ValueError otherwise) a call is one
        SCHEDULER STEP of continuous batching: `hidden_states [1, N, D]` is the pack `cache.schedule(slots, cu_seqlens)` declared, and
        the layer runs one `featmap_rotary_decode` launch and one `mhla_causal_extend(cu_seqlens=)` on its pool's slots in place (see
        `_pool_step`).  An `attention_mask` is a ValueError; `cu_seqlens`, `token_counts` or `speculative` as arguments,
        `use_short_conv` and `head_k_dim % 8 != 0` raise NotImplementedError.
        `grouped_state` (not in the reference, default off: nothing changes; needs `exact_decoding`, ValueError otherwise): with
        `num_kv_heads < num_heads` every exact call -- the prefill's state, steps, extensions with or without `token_counts`,
        speculative verify / commit, device-positioned steps, the packed exact prefill -- keeps k and v un-repeated: feature map and
        rotary run on `num_kv_heads` heads, and the cached `CausalState` has `num_kv_heads` heads, 1 / `num_kv_groups` of the memory
        and of the per-token state traffic (the state is a function of k and v alone, so the repeated heads of a group held equal
        copies).  The outputs are bit for bit those of `grouped_state=False`; the operator of the prefill's output takes the
        un-repeated heads too (`mhla_causal`: natively when there is no gradient to compute).  Whatever `grouped_state`, a forward
        without a cache under `torch.no_grad()` leaves k and v un-repeated as well."""
        super().__init__()
        self.mode = mode
        self.hidden_size = hidden_size
        self.expand_k = expand_k
        self.expand_v = expand_v
        self.num_heads = num_heads
        self.num_kv_heads = num_kv_heads if num_kv_heads is not None else num_heads
        self.num_kv_groups = self.num_heads // self.num_kv_heads
        self.key_dim = int(hidden_size * expand_k)
        self.value_dim = int(hidden_size * expand_v)
        self.key_dim_per_group = self.key_dim // self.num_kv_groups
        self.value_dim_per_group = self.value_dim // self.num_kv_groups
        self.clamp_min = clamp_min
        self.layer_idx = layer_idx
        if summaries not in ("tf32", "split", "bf16"):
            raise ValueError(f"summaries={summaries!r}: 'tf32', 'split' or 'bf16'")
        self.summaries = summaries
        self.exact_decoding = bool(exact_decoding)
        self.isolate_sequences = bool(isolate_sequences)
        if grouped_state and not exact_decoding:
            raise ValueError("MHLA(grouped_state=True) needs exact_decoding=True: the grouped state is the exact decode state")
        self.grouped_state = bool(grouped_state)
        self.use_output_gate = use_output_gate
        assert mode in ["chunk", "fused_recurrent", "fused_chunk"], f"Not supported mode `{mode}`."
        assert self.key_dim % num_heads == 0, f"key dim must be divisible by num_heads of {num_heads}"
        assert self.value_dim % num_heads == 0, f"value dim must be divisible by num_heads of {num_heads}"
        self.head_k_dim = self.key_dim // num_heads
        self.head_v_dim = self.value_dim // num_heads

        self._fmap_name = feature_map
        if feature_map == "relu":
            self.feature_map_q = self.feature_map_k = nn.ReLU()
        elif feature_map == "identity":
            self.feature_map_q = self.feature_map_k = nn.Identity()
        elif feature_map == "elu":
            self.feature_map_q = self.feature_map_k = _elu1
        else:
            raise NotImplementedError(f"Not supported feature map `{feature_map}`.")
        self.use_short_conv = use_short_conv
        self.conv_size = conv_size
        self.conv_bias = conv_bias

        self.q_proj = nn.Linear(hidden_size, self.key_dim, bias=False)
        self.k_proj = nn.Linear(hidden_size, self.key_dim_per_group, bias=False)
        self.v_proj = nn.Linear(hidden_size, self.value_dim_per_group, bias=False)
        if self.use_output_gate:
            self.g_proj = nn.Linear(hidden_size, self.value_dim, bias=False)
        if use_short_conv:                                                   # layers/mhla.py:175-194
            self.q_conv1d = ShortConvolution(self.key_dim, conv_size, bias=conv_bias, activation="silu")
            self.k_conv1d = ShortConvolution(self.key_dim_per_group, conv_size, bias=conv_bias, activation="silu")
            self.v_conv1d = ShortConvolution(self.value_dim_per_group, conv_size, bias=conv_bias, activation="silu")
        self.max_chunks = int(max_chunks)
        self.mixing_matrix = nn.Parameter(causal_mixing_init(self.max_chunks))   # layers/mhla.py:196-200 (32 there)
        self.o_proj = nn.Linear(self.value_dim, hidden_size, bias=False)
        self.fuse_norm_and_gate = gate_fn == "swish" and fuse_norm and use_output_gate
        if self.fuse_norm_and_gate:
            self.g_norm_swish_gate = FusedRMSNormGated(self.head_v_dim, elementwise_affine, norm_eps)
        else:
            self.g_norm = FusedRMSNormGated(self.head_v_dim, elementwise_affine, norm_eps)
            self.gate_fn = {"swish": F.silu, "silu": F.silu, "sigmoid": torch.sigmoid, "relu": F.relu,
                            "gelu": F.gelu}[gate_fn]
        self.gate_logit_normalizer = gate_logit_normalizer
        assert self.head_k_dim <= 256, "head_k_dim must be less than or equal to 256"
        self.rotary = RotaryEmbedding(dim=self.head_k_dim)

    def forward(self, hidden_states: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                past_key_values=None, use_cache: Optional[bool] = False, output_attentions: Optional[bool] = False,
                **kwargs: Dict):
        if isinstance(past_key_values, PagedDecodeCache):   # (recognised by the cache's type alone: nothing below changes)
            return self._pool_step(hidden_states, attention_mask, past_key_values, use_cache, kwargs), None, past_key_values
        if self.exact_decoding and bool(use_cache) and getattr(past_key_values, "device_positions", False):
            if kwargs.get("speculative", False):
                raise NotImplementedError("MHLA: speculative=True on a DecodeCache(device_positions=True) (a verify reads the host positions)")
            entry = self._device_positioned_entry(hidden_states, past_key_values)
            if entry is not None:
                return self._device_positioned_step(hidden_states, entry), None, past_key_values
        # clamp + tril of the mixing weights at the start of every forward, on .data (layers/mhla.py:237)
        self.mixing_matrix.data = torch.clamp(self.mixing_matrix.data, 1e-5, 1).tril()
        if attention_mask is not None:
            assert len(attention_mask.shape) == 2, (
                "Expected attention_mask as a 0-1 matrix with shape [batch_size, seq_len] for padding purposes "
                "(0 indicating padding). Arbitrary attention masks of shape [batch_size, seq_len, seq_len] are not allowed.")
        if (self.isolate_sequences and use_cache and (attention_mask is not None or kwargs.get("cu_seqlens", None) is not None)
                and not (self.exact_decoding and getattr(past_key_values, "packed_prefill", False))):
            # (before the exact_decoding prefill drops the mask: that path is refused too, not taken silently)
            raise NotImplementedError("MHLA(isolate_sequences=True): an attention_mask or cu_seqlens with use_cache -- a decode state per "
                                      "packed sequence, and the exact_decoding prefill of a padded batch, are not implemented for it")
        batch_size, q_len, _ = hidden_states.shape
        last_state = None
        if past_key_values is not None and self.layer_idx is not None and len(past_key_values) > self.layer_idx:
            last_state = past_key_values[self.layer_idx]                      # :249-251
        speculative = self._speculative_call(past_key_values, use_cache, last_state, kwargs)
        call = self._classify_call(hidden_states, attention_mask, past_key_values, use_cache, last_state, kwargs)
        # (an exact call's mask has become the prefill's lengths, or is not read: a ragged state carries them)
        attention_mask = None if call.exact and not call.packed else attention_mask
        indices, cu_seqlens = None, kwargs.get("cu_seqlens", None)
        if attention_mask is not None:
            hidden_states, indices, cu_seqlens = self._unpad(hidden_states, attention_mask)
        plan = None               # isolate_sequences: the pack's chunk table, handed to the operator as cu_seqlens=
        if self.isolate_sequences and cu_seqlens is not None:
            plan = kwargs.get("varlen_plan", None)
            if plan is None:
                plan = causal_varlen_plan(cu_seqlens, hidden_states.device)
        # (grouped_state: the exact paths keep the k/v heads un-repeated.  So does, with grad mode off, every call whose operator is the
        # reference protocol's -- mhla_causal / mhla_causal_normgate / naive_recurrent_mhla take grouped-query heads, and the state the
        # last one returns has q's heads; an exact call without grouped_state keeps its repeated heads: its cached state has them)
        reference = call.state is None and not call.exact
        grouped = self.num_kv_groups > 1 and ((self.grouped_state and call.exact) or (reference and not torch.is_grad_enabled()))
        q, k, v, conv_states = self._project(hidden_states, last_state, use_cache, cu_seqlens, repeat=not grouped)
        rows = self._rotary_rows(call, q, q_len, cu_seqlens, attention_mask, past_key_values)
        q, k = self._featmap_rotary(q, k, rows, flat=call.ragged)
        fused = self.use_output_gate and self.fuse_norm_and_gate and (q_len > 64 or call.packed)
        if call.state is not None:
            o, recurrent_state, fused = self._decode(q, k, v, hidden_states, call.state, call.token_counts, speculative)
        elif call.exact:
            o, recurrent_state, fused = self._exact_prefill(q, k, v, hidden_states, call.lengths, fused, plan if call.packed else None)
        else:
            initial_state = last_state["recurrent_state"] if last_state is not None else None
            o, recurrent_state, fused = self._reference_operator(q, k, v, hidden_states, plan, fused, (batch_size, q_len), initial_state, use_cache)
        if speculative:   # (the verified draft, not a state: neither the state nor the cache's token count moves)
            last_state.update(draft=recurrent_state, draft_mix=self.mixing_matrix.detach())
        else:
            self._update_cache(past_key_values, use_cache, call, recurrent_state, conv_states, q_len, q)
        o = self._gate_and_project(o, hidden_states, fused)
        if call.keep is not None:                                            # zeros at padding rows, as pad_input leaves them
            o = o.masked_fill(~call.keep.unsqueeze(-1), 0)
        if rows.keep is not None:
            o = o.masked_fill(~rows.keep.unsqueeze(-1), 0)
        if indices is not None:                                              # pad_input, :362-363
            full = o.new_zeros(batch_size * q_len, o.shape[-1])
            full.index_copy_(0, indices, o.squeeze(0))
            o = full.reshape(batch_size, q_len, -1)
        return o, None, past_key_values

    def _speculative_call(self, past_key_values, use_cache, last_state, kwargs) -> bool:
        """Whether the call is a speculative one (`speculative=True` through **kwargs; ignored without `exact_decoding`, `use_cache` and
        a cache) -- a verify on the cached decode state, which must exist and is made ragged on the same storage -- and the refusals
        around a pending draft: a new speculative call replaces it, any other call is refused until `commit` or `discard`."""
        exact = self.exact_decoding and bool(use_cache) and past_key_values is not None and hasattr(past_key_values, "update")
        speculative = exact and bool(kwargs.get("speculative", False))
        if not speculative:
            if exact and last_state is not None and last_state.get("draft") is not None:
                raise ValueError("MHLA(exact_decoding=True): the cache holds a pending draft of a speculative call: commit or discard first "
                                 "(DecodeCache.commit(accept) / DecodeCache.discard())")
            return False
        if self.use_short_conv:
            raise NotImplementedError("MHLA(exact_decoding=True): use_short_conv with speculative=True (the convolution's state has no verify)")
        state = last_state["recurrent_state"] if last_state is not None else None
        if not isinstance(state, CausalState):
            raise NotImplementedError("MHLA(exact_decoding=True): speculative=True on an empty cache: a draft is verified on the decode state "
                                      "a prefill left")
        last_state["recurrent_state"] = state.to_ragged()   # (shares storage; a ragged state returns itself)
        return True

    def _classify_call(self, hidden_states, attention_mask, past_key_values, use_cache, last_state, kwargs) -> _Call:
        """Which kind of call this is (see `_Call`), and every refusal that depends on the kind."""
        batch_size, q_len, _ = hidden_states.shape
        exact = self.exact_decoding and bool(use_cache) and past_key_values is not None and hasattr(past_key_values, "update")
        cached = last_state["recurrent_state"] if last_state is not None else None
        state = cached if exact and isinstance(cached, CausalState) else None
        ragged = state is not None and state.lengths is not None
        lengths = keep = None
        if exact:
            if self.layer_idx is None:
                raise ValueError("MHLA(exact_decoding=True): the cache is indexed by layer_idx, which is None")
            cu_seqlens = kwargs.get("cu_seqlens", None)
            if self.isolate_sequences and getattr(past_key_values, "packed_prefill", False):
                # DecodeCache(packed_prefill=True): the call on the empty cache that carries a pack (or a mask, unpadded to one) is the
                # packed exact prefill; on a state, a mask is not read (as on any ragged state) and a pack is refused
                if state is not None and cu_seqlens is not None:
                    raise NotImplementedError("MHLA(isolate_sequences=True): cu_seqlens on a cache that already holds a decode state -- "
                                              "packed new tokens are not implemented: pass them padded, [sequences, T, D], with token_counts=")
                if state is None and (cu_seqlens is not None or attention_mask is not None):
                    if self.use_short_conv:
                        raise NotImplementedError("MHLA(isolate_sequences=True): use_short_conv with a packed exact prefill (a convolution "
                                                  "state per packed sequence is not implemented)")
                    if cu_seqlens is not None and batch_size != 1:
                        raise ValueError(f"MHLA: cu_seqlens takes one packed row (B = 1), got B = {batch_size}")
                    return _Call(True, None, False, None, None, None, 0, True)
            # (a ragged state carries the lengths: the mask is not read)
            if attention_mask is not None and not ragged and not bool(attention_mask.all()):
                if state is not None:
                    raise NotImplementedError("MHLA(exact_decoding=True): the cached decode state is uniform (all sequences share "
                                              "one length); a padding attention_mask goes with the prefill")
                keep = attention_mask[:, -q_len:].to(hidden_states.device) != 0
                if self.use_short_conv:
                    raise NotImplementedError("MHLA(exact_decoding=True): use_short_conv with a padding attention_mask")
                if keep.shape != (batch_size, q_len) or bool((keep[:, :-1] & ~keep[:, 1:]).any()):
                    raise NotImplementedError("MHLA(exact_decoding=True): a padding attention_mask must be left-padded, each row "
                                              f"zeros then ones over the {q_len} tokens of the call")
                lengths, ragged = keep.sum(-1).tolist(), True
        # token_counts (not in the reference; through **kwargs, so its signature is kept): B ints in 0 .. q_len, honoured only on a
        # cached ragged decode state -- sequence b takes the LAST token_counts[b] rows of the call (right-aligned, as the left-padded
        # prefill), through mhla_causal_extend(counts=, left_padded=True): one launch chain whatever the counts
        token_counts = kwargs.get("token_counts", None) if ragged and state is not None else None
        if token_counts is not None:
            if self.use_short_conv:
                raise NotImplementedError("MHLA(exact_decoding=True): use_short_conv with token_counts")
            token_counts = tuple(int(n) for n in (token_counts.tolist() if isinstance(token_counts, torch.Tensor) else token_counts))
            if len(token_counts) != batch_size or any(n < 0 or n > q_len for n in token_counts):
                raise ValueError(f"MHLA: token_counts={token_counts} must be {batch_size} ints in 0 .. {q_len}")
        return _Call(exact, state, ragged, lengths, keep, token_counts, state.seen if state is not None else 0)

    @staticmethod
    def _unpad(hidden_states, attention_mask):
        """layers/mhla.py:253-256 (get_unpad_data): the real tokens of a padded batch as one packed sequence `[1, tokens, D]`, their
        rows in the `[B * T]` layout and the pack's `cu_seqlens`."""
        batch_size, q_len, _ = hidden_states.shape
        m = attention_mask[:, -q_len:]
        indices = torch.nonzero(m.flatten(), as_tuple=False).flatten()
        cu_seqlens = F.pad(m.sum(-1, dtype=torch.int32).cumsum(0, dtype=torch.int32), (1, 0))
        return hidden_states.reshape(batch_size * q_len, -1).index_select(0, indices).unsqueeze(0), indices, cu_seqlens

    def _repeat_kv(self, k, v):
        """k, v of `num_kv_heads` heads with every head repeated `num_kv_groups` times (repeat '(h g) d', :290-292)."""
        B, T = k.shape[:2]
        k = k.unsqueeze(3).expand(-1, -1, -1, self.num_kv_groups, -1).reshape(B, T, self.num_heads, self.head_k_dim)
        v = v.unsqueeze(3).expand(-1, -1, -1, self.num_kv_groups, -1).reshape(B, T, self.num_heads, self.head_v_dim)
        return k, v

    def _project(self, hidden_states, last_state=None, use_cache=False, cu_seqlens=None, repeat=True):
        """q, k, v as `[B, T, H, .]` (through the short convolutions with `use_short_conv`, :258-279; grouped k / v heads
        expanded, :290-292 -- `repeat=False`: left as `[B, T, num_kv_heads, .]`) and the convolutions' states (None without them)."""
        B, T, _ = hidden_states.shape
        conv_states = None
        if self.use_short_conv:
            cq = ck = cv = None
            if last_state is not None and last_state.get("conv_state") is not None:
                cq, ck, cv = last_state["conv_state"]
            q, cq = self.q_conv1d(x=self.q_proj(hidden_states), cache=cq, output_final_state=use_cache, cu_seqlens=cu_seqlens)
            k, ck = self.k_conv1d(x=self.k_proj(hidden_states), cache=ck, output_final_state=use_cache, cu_seqlens=cu_seqlens)
            v, cv = self.v_conv1d(x=self.v_proj(hidden_states), cache=cv, output_final_state=use_cache, cu_seqlens=cu_seqlens)
            conv_states = (cq, ck, cv)
        else:
            q, k, v = self.q_proj(hidden_states), self.k_proj(hidden_states), self.v_proj(hidden_states)
        q = q.reshape(B, T, self.num_heads, self.head_k_dim)
        k, v = k.reshape(B, T, self.num_kv_heads, self.head_k_dim), v.reshape(B, T, self.num_kv_heads, self.head_v_dim)
        if self.num_kv_groups > 1 and repeat:
            k, v = self._repeat_kv(k, v)
        return q, k, v, conv_states

    def _rotary_rows(self, call, q, q_len, cu_seqlens, attention_mask, past_key_values) -> _RotaryRows:
        """The rotary position of every token row (see `_RotaryRows`): packed sequences restart at every sequence start
        (rotary.py:68-72 with cu_seqlens); with a padding mask AND a cache offset every sequence continues from its own length
        (prepare_lens_from_mask, :305-309)."""
        B, T = q.shape[:2]
        seqlen_offset = 0
        if past_key_values is not None and hasattr(past_key_values, "get_seq_length"):
            seqlen_offset = past_key_values.get_seq_length(self.layer_idx)    # :301-303
        if cu_seqlens is None and not call.ragged:
            return _RotaryRows(None, T + seqlen_offset, seqlen_offset, None)
        tpos = torch.arange(T, device=q.device)
        if call.ragged:
            # every sequence at positions of its own, in the [B, T] layout: row (b, t) is token t - pad_b of a padded prefill (padding
            # rows: position 0, their output is dropped), token pos_b + t of a later call (the state's device positions: no sync).
            # The tables are gathered per row, so q and k go through the rotary as one sequence of B T rows.
            if call.lengths is not None:
                pads = T - torch.tensor(call.lengths, device=q.device)
                return _RotaryRows((tpos[None, :] - pads[:, None]).clamp_(min=0).flatten(), T, 0, None)
            if call.token_counts is None:
                return _RotaryRows((call.state.pos.long()[:, None] + tpos[None, :]).flatten(), call.state.seen + T, 0, None)
            # row t of sequence b is its token pos_b + (t - (T - n_b)); padding rows (t < T - n_b) are clamped: their output is dropped
            pads = T - torch.tensor(call.token_counts, device=q.device)
            rel = (tpos[None, :] - pads[:, None]).clamp_(min=0)
            return _RotaryRows((call.state.pos.long()[:, None] + rel).flatten(), call.state.seen + T, 0, tpos[None, :] >= pads[:, None])
        cu = cu_seqlens.to(q.device).long()
        seq = torch.searchsorted(cu, tpos, right=True) - 1
        if attention_mask is None or seqlen_offset <= 0:
            return _RotaryRows(tpos - cu[seq] + seqlen_offset, T + seqlen_offset, seqlen_offset, None)
        offs = (attention_mask.sum(-1).to(q.device).long() - q_len)[seq]
        return _RotaryRows(tpos - cu[seq] + offs, int(attention_mask.shape[1]), seqlen_offset, None)

    def _featmap_rotary(self, q, k, rows, flat):
        """Feature map (:297-299) and rotary (:311) of q and k at `rows`; `flat`: as one sequence of B T rows (ragged calls)."""
        shape, kshape = q.shape, k.shape   # (grouped_state: k has the k/v heads)
        if flat:
            q, k = q.reshape(1, shape[0] * shape[1], *shape[2:]), k.reshape(1, shape[0] * shape[1], *kshape[2:])
        if self.head_k_dim % 8 == 0:
            # feature map + rotary in one HIP kernel per tensor and direction
            cos, sin = self.rotary._tables(rows.table_len, q.device, q.dtype)
            t_off = rows.seqlen_offset
            if rows.positions is not None:   # per-token rows of the tables, gathered once
                cos, sin, t_off = cos.index_select(0, rows.positions), sin.index_select(0, rows.positions), 0
            q, k = featmap_rotary(q, cos, sin, self._fmap_name, t_off), featmap_rotary(k, cos, sin, self._fmap_name, t_off)
        else:
            if not getattr(self, "_warned_eager_rotary", False):
                warnings.warn(f"MHLA: head_k_dim={self.head_k_dim} is not a multiple of 8: feature map and rotary run as eager "
                              "PyTorch ops (about ten elementwise passes per tensor) instead of the fused HIP kernel", stacklevel=3)
                self._warned_eager_rotary = True
            q, k = self.feature_map_q(q), self.feature_map_k(k)              # :297-299
            q, k = self.rotary(q, k, seqlen_offset=rows.seqlen_offset, max_seqlen=rows.table_len, positions=rows.positions)   # :311
        return (q.reshape(shape), k.reshape(kshape)) if flat else (q, k)

    def _fused_gate(self, hidden_states):
        """`(g [B, T, H, V], the norm module)` for an operator that applies norm x gate itself; `(None, None)` unless `fuse_norm_and_gate`."""
        if not self.fuse_norm_and_gate:
            return None, None
        return self.g_proj(hidden_states).reshape(*hidden_states.shape[:2], self.num_heads, self.head_v_dim), self.g_norm_swish_gate

    def _decode(self, q, k, v, hidden_states, state, token_counts, speculative=False):
        """Decoding on the state the prefill (or the calls before) left: one exact step for one token, one extension for several.
        `speculative`: a verify -- the same rows, the state untouched, and the `CausalDraft` returned in the state's place."""
        B, T = q.shape[:2]
        g, gn = self._fused_gate(hidden_states)
        advance = mhla_causal_verify if speculative else mhla_causal_step if T == 1 and token_counts is None else mhla_causal_extend
        counted = {} if token_counts is None else {"counts": token_counts, "left_padded": True}
        o = advance(q, k, v, self.mixing_matrix, state, gate=g, norm_weight=gn.weight if gn is not None else None,
                    norm_eps=gn.eps if gn is not None else 1e-5, epilogue=gn is not None, **counted)
        if speculative:
            o, state = o
        return (o.reshape(B, T, self.value_dim) if gn is not None else o), state, gn is not None

    def _exact_prefill(self, q, k, v, hidden_states, lengths, fused, plan=None):
        """Prefill: the chunk operator for the output (any length: the single-chunk case for <= 64 tokens), and the decode state.
        `lengths` (a left-padded batch): the operator (and the fused epilogue) over every sequence's real tokens alone, zeros
        elsewhere -- run by run of adjacent sequences of equal length, as mhla_causal_prefill(lengths=, left_padded=True) does.
        `plan` (the packed exact prefill): the `isolate_sequences` operator over the pack, and the ragged state of every sequence
        of it from one launch chain."""
        B, T = q.shape[:2]
        mix = self.mixing_matrix
        # (grouped_state: the state and the operator both take the k/v heads as they are)
        ko, vo = k, v
        if plan is not None:
            o, _, fused = self._reference_operator(q, ko, vo, hidden_states, plan, fused, (B, T), None, True)
            return o, mhla_causal_state(k, v, mix, cu_seqlens=plan), fused
        if not fused and lengths is not None:
            return (*mhla_causal_prefill(q, k, v, mix, summaries=self.summaries, lengths=lengths, left_padded=True), False)
        if not fused:
            return mhla_causal(q, ko, vo, mix, summaries=self.summaries), mhla_causal_state(k, v, mix), False
        g, gn = self._fused_gate(hidden_states)
        if lengths is None:
            o = mhla_causal_normgate(q, ko, vo, mix, g, gn.weight, gn.eps, summaries=self.summaries)
            return o.reshape(B, T, self.value_dim), mhla_causal_state(k, v, mix), True
        o = q.new_zeros(B, T, self.num_heads, self.head_v_dim)
        for i, j, n in _runs(lengths, B):
            if n:
                o[i:j, T - n:] = mhla_causal_normgate(q[i:j, T - n:], ko[i:j, T - n:], vo[i:j, T - n:], mix, g[i:j, T - n:],
                                                      gn.weight, gn.eps, summaries=self.summaries)
        return o.reshape(B, T, self.value_dim), mhla_causal_state(k, v, mix, lengths=lengths, left_padded=True), True

    def _reference_operator(self, q, k, v, hidden_states, plan, fused, padded_shape, initial_state, use_cache):
        """The reference layer's operator call, and the `isolate_sequences` one (`plan`): a recurrent state only from the
        token-recurrent form."""
        B, T = q.shape[:2]
        if fused:
            # operator + per-head RMSNorm x swish gate (:330-337 + :351-355) as one node: the epilogue runs in the operator's
            # output kernel where the shape allows, otherwise as the separate HIP kernel (mhla_causal_normgate decides)
            g, gn = self._fused_gate(hidden_states)
            o = mhla_causal_normgate(q, k, v, self.mixing_matrix, g, gn.weight, gn.eps, summaries=self.summaries, cu_seqlens=plan)
            return o.reshape(B, T, self.value_dim), None, True
        if plan is not None:                                                 # (isolate_sequences: the chunk operator whatever q_len)
            return mhla_causal(q, k, v, self.mixing_matrix, summaries=self.summaries, cu_seqlens=plan), None, False
        batch_size, q_len = padded_shape
        if q_len > 64:                                                       # :330-337
            return mhla_causal(q, k, v, self.mixing_matrix, summaries=self.summaries), None, False
        if T > 64 and not getattr(self, "_warned_recurrent_packed", False):   # :247, :318-327: the token-recurrent form
            warnings.warn(f"MHLA: a padded batch of {batch_size} x {q_len} tokens unpads to one packed sequence of {T} > 64 tokens; "
                          "the recurrent branch then runs the multi-chunk chunk operator (the reference's recurrent form reads "
                          "shifted states beyond the first chunk -- not replicated, see naive_recurrent_mhla)", stacklevel=3)
            self._warned_recurrent_packed = True
        return (*naive_recurrent_mhla(q, k, v, self.mixing_matrix, initial_state=initial_state, output_final_state=bool(use_cache)), False)

    def _update_cache(self, cache, use_cache, call, recurrent_state, conv_states, q_len, like):
        """:339-345; on a `DecodeCache(device_positions=True)` the state is stored ragged, with what the device-positioned steps read."""
        if cache is None or not hasattr(cache, "update"):
            return
        dev = self.exact_decoding and bool(use_cache) and getattr(cache, "device_positions", False) and isinstance(recurrent_state, CausalState)
        recurrent_state = recurrent_state.to_ragged() if dev else recurrent_state
        # (with token_counts the furthest sequence may have grown by fewer than q_len tokens, and a packed prefill's q_len is the
        # pack's: the cache counts what the state does -- after a packed prefill, the longest sequence)
        entry = cache.update(recurrent_state=recurrent_state, conv_state=conv_states, layer_idx=self.layer_idx,
                             offset=q_len if call.token_counts is None and not call.packed else recurrent_state.seen - call.seen)
        if dev:
            # what the device-positioned steps read, made once: the matrix as this forward clamped it (generation does not change
            # the weights), the tables of a row per position the state can reach, the norm weight in fp32
            cap = recurrent_state.capacity_chunks
            cos, sin = self.rotary._tables(64 * cap, like.device, like.dtype)
            gn = self.g_norm_swish_gate if self.fuse_norm_and_gate else None
            entry.update(dev_mix=_mix2d(self.mixing_matrix), dev_cos=cos[:64 * cap], dev_sin=sin[:64 * cap],
                         dev_norm_weight=gn.weight.detach().float().contiguous() if gn is not None and gn.weight is not None else None)

    def _gate_and_project(self, o, hidden_states, fused_epilogue):
        """Norm and output gate (unless the operator's launch chain applied them already: `fused_epilogue`), then o_proj."""
        B, T, _ = hidden_states.shape
        if fused_epilogue:
            pass
        elif self.use_output_gate:
            g = self.g_proj(hidden_states)
            if self.fuse_norm_and_gate:
                o = self.g_norm_swish_gate(o, g.reshape(B, T, self.num_heads, self.head_v_dim))   # :351-355
                o = o.reshape(B, T, self.value_dim)
            else:
                o = self.g_norm(o, None).reshape(B, T, self.value_dim) * self.gate_fn(g)
        else:
            o = self.g_norm(o, None).reshape(B, T, self.value_dim)
        return self.o_proj(o)

    def _pool_step(self, hidden_states, attention_mask, cache, use_cache, kwargs):
        """A scheduler step on a `PagedDecodeCache`: `hidden_states [1, N, D]` is the pack `cache.schedule(slots, cu_seqlens)` declared.
        Projections (k, v left on `num_kv_heads` with `grouped_state`); ONE `featmap_rotary_decode` launch on this layer's
        `pool.at(slots)` -- q and k in place, every row at the position its slot holds on the device, from the layer's tables of 64 x
        capacity rows: no host position, no gathered table rows --; `mhla_causal_extend(cu_seqlens=)` on the same view (norm x gate as
        `_decode` passes them; a fresh request is an empty slot, whose extend is the exact fp32 prefill); output gate and projection.
        Everything the configuration cannot do is refused before anything runs, and what the extend would refuse (`PoolExhausted`,
        the IndexError of a slot beyond the capacity or the mixing matrix) before this layer's first launch, its pages assigned by
        the page rule the extend would apply."""
        fn = "MHLA.forward on a PagedDecodeCache"
        if not self.exact_decoding:
            raise ValueError(f"{fn} needs a layer built with exact_decoding=True (the pool holds exact decode states)")
        if not use_cache:
            raise ValueError(f"{fn} needs use_cache=True: the call advances the pool")
        if hidden_states.dim() != 3 or hidden_states.shape[0] != 1:
            raise ValueError(f"{fn}: hidden_states is the step's pack [1, N, D], got {tuple(hidden_states.shape)}")
        if attention_mask is not None:
            raise ValueError(f"{fn}: no attention_mask: a pack has no padding")
        given = [n for n in ("cu_seqlens", "token_counts") if kwargs.get(n, None) is not None] + (["speculative"] if kwargs.get("speculative", False) else [])
        if given:
            raise NotImplementedError(f"{fn}: {', '.join(given)} as an argument: cache.schedule(slots, cu_seqlens) carries the step's layout, "
                                      "and speculative calls are not implemented on this cache")
        if self.use_short_conv:
            raise NotImplementedError(f"{fn}: use_short_conv (a convolution state per slot is not implemented)")
        if self.head_k_dim % 8:
            raise NotImplementedError(f"{fn} needs head_k_dim % 8 == 0 (the fused q / k prologue), got {self.head_k_dim}")
        if self.layer_idx is None:
            raise ValueError("MHLA(exact_decoding=True): the cache is indexed by layer_idx, which is None")
        heads = self.num_kv_heads if self.grouped_state else self.num_heads
        step, view = cache._layer_step(self.layer_idx, hidden_states.shape[1], (heads, self.head_k_dim, self.head_v_dim))
        self.mixing_matrix.data = torch.clamp(self.mixing_matrix.data, 1e-5, 1).tril()   # (as every forward: layers/mhla.py:237)
        _counts_fit("mhla_causal_extend", self.mixing_matrix, view, step.counts)
        view.pool.reserve(step.slots, [p + n for p, n in zip(view.lengths, step.counts)])
        q, k, v, _ = self._project(hidden_states, repeat=not self.grouped_state)
        cos, sin = cache._tables(self.layer_idx, self.rotary, q)
        q, k = featmap_rotary_decode(q, k, cos, sin, view, feature_map=self._fmap_name, off_dev=step.off_dev, inplace=True)
        g, gn = self._fused_gate(hidden_states)
        o = mhla_causal_extend(q, k, v, self.mixing_matrix, view, cu_seqlens=step.cu, gate=g, norm_weight=gn.weight if gn is not None else None,
                               norm_eps=gn.eps if gn is not None else 1e-5, epilogue=gn is not None)
        step.ran.add(self.layer_idx)
        return self._gate_and_project(o.reshape(*hidden_states.shape[:2], self.value_dim) if gn is not None else o, hidden_states, gn is not None)

    def _device_positioned_entry(self, hidden_states, cache):
        """`DecodeCache(device_positions=True)`: what the configuration cannot do is refused on every call, the prefill included;
        returns this layer's cache entry once the prefill has left a state (None before: the call is the prefill)."""
        if self.layer_idx is None:
            raise ValueError("MHLA(exact_decoding=True): the cache is indexed by layer_idx, which is None")
        if self.use_short_conv:
            raise NotImplementedError("MHLA: DecodeCache(device_positions=True) with use_short_conv (the convolution's state is host-positioned)")
        if self.head_k_dim % 8:
            raise NotImplementedError(f"MHLA: DecodeCache(device_positions=True) needs head_k_dim % 8 == 0 (the fused q / k prologue), got {self.head_k_dim}")
        entry = cache[self.layer_idx] if len(cache) > self.layer_idx else None
        if entry is None or not isinstance(entry.get("recurrent_state"), CausalState):
            return None
        if hidden_states.shape[1] != 1:
            raise NotImplementedError(f"MHLA: a call of {hidden_states.shape[1]} tokens on a DecodeCache(device_positions=True) that holds a "
                                      "state: device-positioned decoding takes one token per call (there is no device-positioned extend)")
        return entry

    def _device_positioned_step(self, hidden_states, entry):
        """One token on a `DecodeCache(device_positions=True)`: projections, `mhla_causal_step_dev` (feature map, rotary at each
        sequence's device position, the step, and norm x gate when `fuse_norm_and_gate`, in three launches), output projection.
        Nothing here depends on a position or synchronises, the cache is not updated (the state advances in place, on the device),
        and `mixing_matrix.data` is NOT reassigned: the matrix the prefill clamped is read, since generation does not change the
        weights.  The whole call may be captured in a graph."""
        q, k, v, _ = self._project(hidden_states, repeat=not self.grouped_state)
        g, gn = self._fused_gate(hidden_states)
        o = mhla_causal_step_dev(q, k, v, entry["dev_mix"], entry["recurrent_state"], feature_map=self._fmap_name,
                                 rotary=(entry["dev_cos"], entry["dev_sin"]), gate=g, norm_weight=entry["dev_norm_weight"],
                                 norm_eps=gn.eps if gn is not None else 1e-5, epilogue=gn is not None)
        return self._gate_and_project(o.reshape(*hidden_states.shape[:2], self.value_dim) if gn is not None else o, hidden_states, gn is not None)
