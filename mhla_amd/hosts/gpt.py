"""A minimal GPT-style host around the fla `MHLA` drop-in: token embedding, pre-norm blocks of
[RMSNorm -> MHLA layer -> residual -> RMSNorm -> gated MLP -> residual], final norm and a tied-free LM head -- the shape of the
reference's GLA-family language model (mhla_nlp/fla/models/gla/modeling_gla.py:83-100 builds the attention the same way).
Plumbing for step-level numbers; stock PyTorch besides the attention layer.  The reference layer's mixing matrix has 32 chunks
(layers/mhla.py:196-200: 2048 tokens at chunk 64); `max_seq_len` sizes it for longer sequences (8192 -> 128 chunks, the
BASELINE.json configs[4] sequence length, through the drop-in layer's `max_chunks`).  With `exact_decoding=True` the layers
keep a decode state in a cache (`forward(..., cache=DecodeCache())`: prefill on the first call, one exact step per later
token, one extension per later call of several tokens) and `generate` decodes greedily on top of it -- with `graph=True` by
replaying one captured whole-model step per token (device-positioned steps: `DecodeCache(device_positions=True)`).  With a
`PagedDecodeCache` a forward is one scheduler step of continuous batching -- a pack of new tokens of the requests the cache's slots
hold -- and `serve` runs requests to completion on top of it (`serve_schedule`: the policy, a pure function)."""
import heapq

import torch
import torch.nn.functional as F
from torch import nn

from ..modules import MHLA, DecodeCache, PagedDecodeCache
from ..ops import causal_varlen_plan


class RMSNorm(nn.Module):
    def __init__(self, dim, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.eps = eps

    def forward(self, x):
        xf = x.float()
        return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + self.eps)).to(x.dtype) * self.weight


class GatedMLP(nn.Module):
    def __init__(self, dim, hidden_ratio=4):
        super().__init__()
        inter = 256 * ((int(dim * hidden_ratio * 2 / 3) + 255) // 256)
        self.gate_proj = nn.Linear(dim, inter * 2, bias=False)
        self.down_proj = nn.Linear(inter, dim, bias=False)

    def forward(self, x):
        g, y = self.gate_proj(x).chunk(2, dim=-1)
        return self.down_proj(F.silu(g) * y)


class Block(nn.Module):
    def __init__(self, dim, heads, expand_k, expand_v, layer_idx, max_chunks=32, exact_decoding=False, isolate_sequences=False,
                 num_kv_heads=None, grouped_state=False):
        super().__init__()
        self.attn_norm = RMSNorm(dim)
        self.attn = MHLA(mode="chunk", hidden_size=dim, expand_k=expand_k, expand_v=expand_v, num_heads=heads,
                         feature_map="relu", layer_idx=layer_idx, max_chunks=max_chunks, exact_decoding=exact_decoding,
                         isolate_sequences=isolate_sequences, num_kv_heads=num_kv_heads, grouped_state=grouped_state)
        self.mlp_norm = RMSNorm(dim)
        self.mlp = GatedMLP(dim)

    def forward(self, x, cache=None, attention_mask=None, token_counts=None, cu_seqlens=None, varlen_plan=None, speculative=False):
        kw = {}
        if cu_seqlens is not None or varlen_plan is not None:   # packed sequences: training (no cache), or the packed prefill
            kw = dict(cu_seqlens=cu_seqlens, varlen_plan=varlen_plan)
        if cache is not None:
            kw.update(past_key_values=cache, use_cache=True)
            if token_counts is not None:
                kw["token_counts"] = token_counts
            if speculative:
                kw["speculative"] = True
        x = x + self.attn(self.attn_norm(x), attention_mask=attention_mask, **kw)[0]
        return x + self.mlp(self.mlp_norm(x))


class GPT_MHLA(nn.Module):
    def __init__(self, vocab_size=32000, hidden_size=1024, num_layers=24, num_heads=4, expand_k=0.5, expand_v=1.0,
                 max_seq_len=2048, exact_decoding=False, isolate_sequences=False, num_kv_heads=None, grouped_state=False):
        """`num_kv_heads`, `grouped_state`: passed to every layer (`MHLA`): grouped-query heads, and -- with `exact_decoding` -- decode
        states of `num_kv_heads` heads instead of `num_heads` equal copies per group."""
        super().__init__()
        self.exact_decoding = bool(exact_decoding)
        self.isolate_sequences = bool(isolate_sequences)
        self.embeddings = nn.Embedding(vocab_size, hidden_size)
        max_chunks = max(32, (max_seq_len + 63) // 64)     # 32 = the reference layer's matrix; 128 for seq_len 8192 (config 5)
        self.layers = nn.ModuleList([Block(hidden_size, num_heads, expand_k, expand_v, i, max_chunks, exact_decoding, isolate_sequences, num_kv_heads, grouped_state)
                                     for i in range(num_layers)])
        self.norm = RMSNorm(hidden_size)
        self.lm_head = nn.Linear(hidden_size, vocab_size, bias=False)
        for m in self.modules():
            if isinstance(m, (nn.Linear, nn.Embedding)):
                nn.init.normal_(m.weight, std=0.02)

    def forward(self, input_ids, labels=None, cache=None, attention_mask=None, token_counts=None, cu_seqlens=None, speculative=False):
        """`cache` (a `DecodeCache`, model built with `exact_decoding=True`): `input_ids` are the tokens AFTER the ones the cache
        has seen -- the whole prompt on an empty cache, then one token per call, or several (the next turn, a piece of a long
        prompt, a draft to verify): on a non-empty cache those take the layer's `mhla_causal_extend` path, one launch chain per
        layer whatever their number.
        `attention_mask` [B, T] (0 = padding) is handed to every layer.  With a cache it belongs to the prefill and must be
        left-padded: every sequence is then decoded as if alone in the batch, at its own position (the layer's ragged decode
        state), and later calls need no mask.  Logits at padding rows are unspecified.
        `token_counts` (B ints in 0 .. T, a list or a tensor; with a cache whose decode state is ragged, i.e. after a masked
        prefill): sequence b takes only the LAST `token_counts[b]` tokens of `input_ids[b]` (right-aligned, as the prefill's
        padding) -- one slot decoding a token beside another taking a slice of a long prompt, a slot that sits the call out (0) -- in
        one launch chain per layer; handed to every layer.  The layers' outputs at padding rows are zeros, the logits there unspecified.
        `cu_seqlens` (`input_ids` [1, T]): packed sequences, handed to every layer.  A model built with
        `isolate_sequences=True` runs every sequence of the pack (or of a padded batch with `attention_mask`) alone; the
        operator's chunk table (`causal_varlen_plan`, one host read of the lengths) is built here once for all layers.  With a
        cache, `cu_seqlens` is the packed prefill: a model built with both `exact_decoding` and `isolate_sequences`, an EMPTY
        `DecodeCache(packed_prefill=True)`; the logits are the pack's, [1, T], and later calls are [sequences, T'] on the ragged
        state.  On a cache that holds a state it raises NotImplementedError.
        `speculative=True` (a cache that holds a state): `input_ids` are a draft to VERIFY -- the logits of the same call without
        the flag, but no layer's state and no token count moves; `cache.commit(accept)` then advances every layer by the first
        `accept[b]` tokens of sequence b's window, `cache.discard()` by none.  Handed to every layer.
        `cache` a `PagedDecodeCache`: one scheduler step of continuous batching.  `cache.schedule(slots, cu_seqlens)` declared which
        request takes which rows of the pack, `input_ids` [1, N] is that pack, the logits are [1, N, vocab], and every layer has
        advanced its pool's slots.  `cu_seqlens=` as an argument stays refused (the schedule carries it); `attention_mask`,
        `token_counts` and `speculative` are refused by the layers."""
        if cache is not None and not self.exact_decoding:
            raise ValueError("GPT_MHLA.forward(cache=...) needs a model built with exact_decoding=True")
        # a model built with exact_decoding and isolate_sequences prefills a pack into an EMPTY DecodeCache(packed_prefill=True):
        # the layers' packed exact prefill (`input_ids` [1, T] with cu_seqlens, or a padded batch with attention_mask)
        prefill = cache is not None and len(cache) == 0
        packed = prefill and self.isolate_sequences and getattr(cache, "packed_prefill", False)
        if cu_seqlens is not None and cache is not None and not packed:
            raise NotImplementedError("GPT_MHLA.forward: cu_seqlens with a cache" + (
                " that already holds a state" if not prefill else
                " needs a model built with exact_decoding and isolate_sequences and a DecodeCache(packed_prefill=True)"))
        plan = None
        if self.isolate_sequences and (cache is None or packed) and (cu_seqlens is not None or attention_mask is not None):
            lens = cu_seqlens if cu_seqlens is not None else F.pad(
                attention_mask[:, -input_ids.shape[1]:].sum(-1, dtype=torch.int32).cumsum(0, dtype=torch.int32), (1, 0))
            plan = causal_varlen_plan(lens, input_ids.device)
        if token_counts is not None and isinstance(token_counts, torch.Tensor):
            token_counts = token_counts.tolist()   # (read once for all layers)
        x = self.embeddings(input_ids)
        for blk in self.layers:
            x = blk(x, cache, attention_mask, token_counts, cu_seqlens, plan, speculative)
        logits = self.lm_head(self.norm(x))
        if labels is None:
            return logits
        return F.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]).float(), labels[:, 1:].reshape(-1))

    @torch.no_grad()
    def generate(self, input_ids, max_new_tokens, attention_mask=None, graph=False, return_logits=False, draft=None, draft_len=4):
        """Greedy decoding: one prefill over `input_ids` [B, T], then one cached step per new token.  Returns the
        `max_new_tokens` new ids [B, max_new_tokens]; T + max_new_tokens must fit the mixing matrix (`max_seq_len`).
        `attention_mask` [B, T]: prompts of different lengths, left-padded to T (0 = padding); every sequence continues from
        its own length.  A model built with `exact_decoding` and `isolate_sequences` prefills them as a pack
        (`DecodeCache(packed_prefill=True)`); the prompts stay left-padded, since the next token is read from `logits[:, -1]`.
        `graph=True`: the steps are device-positioned (`DecodeCache(device_positions=True)`) -- an eager prefill, one eager step
        that loads every kernel, then ONE whole-model step captured in a graph (static id and logits buffers, a single stream: a
        linear graph without parallel branches) and replayed once per token, and one `cache.sync()` at the end, which raises
        IndexError if a sequence was stepped beyond `max_seq_len` (its logits from there on came from zero attention rows).
        `return_logits=True`: `(ids, logits [B, max_new_tokens, vocab])`, the logits every id was picked from.
        `draft=fn, draft_len=k`: greedy SPECULATIVE decoding, the same ids in fewer model calls.  `fn(histories)` takes the list of B
        1-D id tensors (every prompt without its padding, plus the tokens emitted so far) and returns `[B, k]` proposed ids.  Per
        round ONE model call verifies `[last token, d_1 .. d_k]` (`speculative=True`: no state moves), sequence b accepts the
        longest prefix with `d_j == argmax(logits_{j-1})`, emits those m_b drafts plus the bonus token `argmax(logits_{m_b})`, and
        `cache.commit(m_b + 1)` advances every layer -- one host read of the acceptance per round for all of them.  A sequence that
        has its `max_new_tokens` sits the later rounds out (`token_counts` 0); near the end the window is clipped so that nothing is
        verified beyond `T + max_new_tokens`.  `graph=True` with it raises NotImplementedError."""
        n = int(max_new_tokens)
        if draft is not None:
            if graph:
                raise NotImplementedError("GPT_MHLA.generate: draft= with graph=True (a verify reads the host positions)")
            return self._generate_speculative(input_ids, n, attention_mask, return_logits, draft, int(draft_len))
        # (both flags: a padded batch is prefilled as a pack -- no padding row through the operator, one state chain per layer)
        cache = DecodeCache(device_positions=bool(graph), packed_prefill=self.exact_decoding and self.isolate_sequences)
        new, kept = [], []

        def pick(logits):
            kept.append(logits[:, -1:]) if return_logits else None
            new.append(logits[:, -1:].argmax(-1))
            return new[-1]

        ids = input_ids
        for _ in range(min(n, 1) if graph else n):   # (graph: the prefill alone)
            ids = pick(self.forward(ids, cache=cache, attention_mask=attention_mask))
            attention_mask = None   # (the prefill's: the decode state carries the lengths from here on)
        if graph and n > 1:
            # the warm-up step (a real token) on a side stream, as a capture wants it: kernel code objects and the GEMM library's
            # per-stream workspaces exist before anything is recorded
            side = torch.cuda.Stream(device=ids.device)
            side.wait_stream(torch.cuda.current_stream(ids.device))
            with torch.cuda.stream(side):
                ids = pick(self.forward(ids, cache=cache))
            torch.cuda.current_stream(ids.device).wait_stream(side)
        if graph and n > 2:
            static_ids = ids.clone()
            step = torch.cuda.CUDAGraph()
            with torch.cuda.graph(step):   # (one capture stream, nothing forks from it: a linear graph)
                static_logits = self.forward(static_ids, cache=cache)
            for _ in range(n - 2):
                step.replay()
                static_ids.copy_(pick(static_logits.clone()))
        if graph:
            cache.sync()
        ids = torch.cat(new, dim=1) if new else input_ids[:, :0]
        return (ids, torch.cat(kept, dim=1) if kept else None) if return_logits else ids

    def _generate_speculative(self, input_ids, n, attention_mask, return_logits, draft, k):
        """`generate(draft=, draft_len=k)`: the prefill, then rounds of draft, verify, accept, commit (see `generate`)."""
        if k < 1:
            raise ValueError(f"GPT_MHLA.generate: draft_len={k} must be at least 1")
        B, T = input_ids.shape
        dev = input_ids.device
        empty = input_ids[:, :0]
        if n < 1:
            return (empty, None) if return_logits else empty
        cache = DecodeCache(packed_prefill=self.exact_decoding and self.isolate_sequences)
        logits = self.forward(input_ids, cache=cache, attention_mask=attention_mask)[:, -1]
        keep = attention_mask[:, -T:].to(dev) != 0 if attention_mask is not None else None
        hist = [input_ids[b, keep[b]] if keep is not None else input_ids[b] for b in range(B)]
        out = [[t] for t in logits.argmax(-1).tolist()]          # emitted ids per sequence
        kept = [[logits[b]] for b in range(B)]                    # the logits each was picked from
        last = logits.argmax(-1)
        hist = [torch.cat([h, last[b:b + 1]]) for b, h in enumerate(hist)]
        while any(len(o) < n for o in out):
            # sequence b verifies [last, d_1 .. d_kb], kb = min(k, what it may still emit - 1): right-aligned in k + 1 columns
            room = [n - len(o) for o in out]
            counts = [min(k, r - 1) + 1 if r > 0 else 0 for r in room]
            d = draft(hist).to(dev)
            if tuple(d.shape) != (B, k):
                raise ValueError(f"GPT_MHLA.generate: draft returned {tuple(d.shape)}, expected [B, draft_len] = {(B, k)}")
            window = torch.zeros(B, k + 1, dtype=input_ids.dtype, device=dev)
            for b, c in enumerate(counts):
                if c:
                    window[b, k + 1 - c] = last[b]
                    window[b, k + 2 - c:] = d[b, :c - 1]
            logits = self.forward(window, cache=cache, token_counts=counts, speculative=True)
            # column j + 1 of the window is checked against the argmax at column j; the one host read of the round
            top_host, win_host = torch.stack([logits.argmax(-1), window]).tolist()
            agree = [[t == w for t, w in zip(tr[:-1], wr[1:])] for tr, wr in zip(top_host, win_host)]
            accept = []
            for b, c in enumerate(counts):
                if not c:
                    accept.append(0)
                    continue
                c0, m = k + 1 - c, 0
                while m < c - 1 and agree[b][c0 + m]:
                    m += 1
                accept.append(m + 1)
                new = top_host[b][c0:c0 + m + 1]                  # the m accepted drafts (equal to the argmax) and the bonus token
                out[b].extend(new)
                kept[b].extend(logits[b, c0:c0 + m + 1]) if return_logits else None
                add = torch.tensor(new, dtype=input_ids.dtype, device=dev)
                hist[b] = torch.cat([hist[b], add])
                last[b] = add[-1]
            cache.commit(accept)
        ids = torch.tensor(out, dtype=torch.long, device=dev)
        return (ids, torch.stack([torch.stack(r) for r in kept])) if return_logits else ids


    @torch.no_grad()
    def serve(self, prompts, max_new_tokens, *, n_slots, n_pages, step_tokens=256, return_logits=False, cache=None):
        """Greedy CONTINUOUS BATCHING of `prompts` (a list of 1-D id tensors or lists, any lengths) to `max_new_tokens` new ids each, no
        EOS and no preemption, on a `PagedDecodeCache(n_slots, capacity of the mixing matrix, n_pages)`: every model call is one step
        of `serve_schedule` (the policy; see there) -- the decoding requests' one token each beside slices of the prompts being
        prefilled, packed, at most `step_tokens` tokens --, a finished request's slot is released at once and the next request
        moves in.  The schedule depends on the lengths alone, so nothing is read back from the device between steps.  Returns the list
        of every request's ids (1-D, `max_new_tokens` long); `return_logits=True`: `(ids, logits)`, per request the
        `[max_new_tokens, vocab]` logits every id was picked from.  `cache`: an empty `PagedDecodeCache` of these sizes to run on (its
        pools are reused; by default a new one is made); every slot is released again when `serve` returns."""
        if not self.exact_decoding:
            raise ValueError("GPT_MHLA.serve needs a model built with exact_decoding=True")
        dev = self.embeddings.weight.device
        prompts = [torch.as_tensor(p, dtype=torch.long).reshape(-1).to(dev) for p in prompts]
        n = int(max_new_tokens)
        cap = self.layers[0].attn.max_chunks
        steps = serve_schedule([len(p) for p in prompts], n, n_slots, n_pages, cap, step_tokens)
        if cache is None:
            cache = PagedDecodeCache(n_slots, cap, n_pages, dev)
        elif (cache.n_slots, cache.capacity_chunks, cache.n_pages) != (n_slots, cap, n_pages) or any(cache.lengths):
            raise ValueError(f"GPT_MHLA.serve: cache is {cache!r}, expected an empty one of n_slots={n_slots}, capacity_chunks={cap}, n_pages={n_pages}")
        fed = [0] * len(prompts)
        ids, kept = [[] for _ in prompts], [[] for _ in prompts]
        for slots, cu, kinds in steps:
            pack = []
            for (req, kind), a, b in zip(kinds, cu, cu[1:]):
                pack.append(ids[req][-1] if kind == "decode" else prompts[req][fed[req]:fed[req] + b - a])
                fed[req] += b - a
            cache.schedule(slots, cu)
            logits = self.forward(torch.cat(pack)[None], cache=cache)[0]
            done = []
            for (req, kind), slot, b in zip(kinds, slots, cu[1:]):
                if kind != "prompt":   # (the request's last row of the step: its prompt ended here, or it decoded a token)
                    ids[req].append(logits[b - 1].argmax(-1, keepdim=True))
                    kept[req].append(logits[b - 1]) if return_logits else None
                    if len(ids[req]) == n:
                        done.append(slot)
            if done:
                cache.release(done)
        empty = torch.zeros(0, dtype=torch.long, device=dev)
        out = [torch.cat(r) if r else empty for r in ids]
        return (out, [torch.stack(r) if r else None for r in kept]) if return_logits else out


def serve_schedule(prompt_lens, max_new_tokens, n_slots, n_pages, capacity_chunks, step_tokens):
    """The steps of `GPT_MHLA.serve`, a pure function of the lengths: a list of `(slots, cu, kinds)` -- what
    `PagedDecodeCache.schedule(slots, cu)` takes, and per sequence of the pack `(request, kind)`, kind "prompt" (a slice of the prompt
    that does not end it: no id), "first" (the slice that ends the prompt: the request's first id comes from its last row) or "decode"
    (the id emitted last goes in, the next comes out).  A request is fed its prompt and its first `max_new_tokens - 1` ids.
    Policy: admission is FIFO -- the oldest waiting request moves in when a slot is free and the pool can hold
    ceil((prompt + max_new_tokens) / 64) pages for it beside those promised to the running requests, so no step can exhaust the
    pool; no request overtakes it.  Within a step every decoding request takes its one token first, and what is left of
    `step_tokens` goes to prompt slices in admission order (a request that gets none sits the step out).  A request that has its
    `max_new_tokens` ids leaves after the step, and its slot and pages are free for the next step's admission.
    ValueError: an empty prompt, a request beyond the capacity of 64 `capacity_chunks` tokens or beyond `n_pages` pages on its own,
    `step_tokens < n_slots` (the decoding requests alone could exceed a step)."""
    fn = "serve_schedule"
    lens, n = [int(p) for p in prompt_lens], int(max_new_tokens)
    if n < 1 or not lens:
        return []
    if min(int(n_slots), int(n_pages), int(capacity_chunks)) < 1 or step_tokens < n_slots:
        raise ValueError(f"{fn}: n_slots={n_slots}, n_pages={n_pages}, capacity_chunks={capacity_chunks} must be positive and "
                         f"step_tokens={step_tokens} at least n_slots (every decoding request takes a token of every step)")
    need = [-(-(p + n) // 64) for p in lens]
    bad = [r for r, p in enumerate(lens) if p < 1 or p + n - 1 > 64 * capacity_chunks or need[r] > n_pages]
    if bad:
        raise ValueError(f"{fn}: requests {bad} (prompts {[lens[r] for r in bad]} + {n} new tokens) are empty, exceed the capacity of "
                         f"{64 * capacity_chunks} tokens or need more than the pool's {n_pages} pages")
    waiting, free, pages = list(range(len(lens))), list(range(n_slots)), int(n_pages)
    running, steps = [], []   # running: [request, slot, tokens fed, ids emitted] in admission order
    while waiting or running:
        while waiting and free and need[waiting[0]] <= pages:
            r = waiting.pop(0)
            pages -= need[r]
            running.append([r, heapq.heappop(free), 0, 0])
        budget = step_tokens - sum(1 for run in running if run[2] >= lens[run[0]])
        slots, cu, kinds = [], [0], []
        for decode in (True, False):
            for run in running:
                r, slot, fed, _ = run
                if (fed >= lens[r]) != decode:
                    continue
                take = 1 if decode else min(budget, lens[r] - fed)
                if not take:
                    continue
                budget -= 0 if decode else take
                run[2] += take
                run[3] += run[2] >= lens[r]
                slots.append(slot)
                cu.append(cu[-1] + take)
                kinds.append((r, "decode" if decode else "first" if run[2] == lens[r] else "prompt"))
        steps.append((tuple(slots), tuple(cu), tuple(kinds)))
        for run in [run for run in running if run[3] == n]:
            running.remove(run)
            heapq.heappush(free, run[1])
            pages += need[run[0]]
    return steps


def GPT_configs():
    return {"340M": dict(hidden_size=1024, num_layers=24, num_heads=4), "1.3B": dict(hidden_size=2048, num_layers=24, num_heads=4)}
