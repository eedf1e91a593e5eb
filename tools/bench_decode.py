#!/usr/bin/env python
"""Per-token latency of the causal operator's decoding step (mhla_causal_step) at the two C5 head shapes of bench_configs.py
(H = 4, K = 128, V = 256 and H = 4, K = 256, V = 512; bf16 tokens, fp32 state, L = 128 chunks), B = 1 and 32, early (pos ~ 100)
and late (pos ~ 8000) in the sequence.  Per configuration, alternating within one run and repeated `--reps` times:
  * `--steps` (>= 200) ordinary steps at a fixed position (the state's `seen` is put back before every call, so every call is the
    same step: no chunk boundary), HIP events around the batch, ending in a synchronise;
  * the same number of BOUNDARY steps (pos % 64 == 63: the step plus k_cs_roll over the i + 1 finished chunks), separately;
  * what the token costs without a decode state: `mhla_causal` forward over all pos + 1 tokens.
Each JSON line carries the median and the min / max over the repetitions (us per token), the device time of each kernel from the
library's per-launch event hook (the event-timed batch includes the Python host path of a call, which at B = 1 is the larger
part), the bytes a step must move -- 3 B H K V 4 (P and Cur read, Cur written) plus the token rows -- and the resulting GB/s.

`--extend`: an extension of T in {16, 64, 256, 1024} tokens by ONE `mhla_causal_extend` call at pos 100 and pos 8000, for the same
configurations, against (a) the same T tokens as single steps (real ones: the boundaries they cross included) and (b) a full
`mhla_causal` forward over pos + T tokens -- all three timed in the same run, alternating, `--reps` times; us per token, the
ratios and the device time of each kernel of the extension.  `--extend --workload`: a prefill of 8000 tokens and one extension
of 1024 at B = 1, H = 4, K = 128, V = 256, for a trace of its own.

`--ragged`: the step on a RAGGED state (one position per sequence, `mhla_causal_step_ragged`) against the uniform step at the same B, at
the C5 head (H = 4, K = 128, V = 256), B = 8 and 32: the ragged lengths lie in four different chunks around chunk 15 (offsets -2, -1,
+1, +2, so that the boundary kernel reads as many finished chunks on average as the uniform one at chunk 15), every sequence at another
place in its chunk.  Alternating in the same run, `--reps` times, non-boundary and boundary steps separately; per variant the wall time
of a call (events around `--steps` calls) and the DEVICE time of its kernels (the per-launch event hook, 20 calls per repetition), each
with median, min and max.  Every call must be the same step, so the host side of the state (`seen`, `lengths`) is put back before
every call as above, and so are the device positions of the ragged state, which the launch chain itself advances: a 4 B-byte device
copy before every call, so that host mirror and device array agree at every launch, as they do in use.  The uniform variants are given
the same copy (into a spare tensor), so that all four wall times include that one extra launch; the device times count the library's
kernels only.  The ragged step moves the uniform step's bytes plus 4 B.

`--graph`: the device-positioned step (`mhla_causal_step_dev`: positions on the device only, a launch chain that depends on none of
them) at the C5 head (H = 4, K = 128, V = 256, bf16, L = 128), B = 8 and 32, lengths as for `--ragged`, non-boundary steps: (a) the eager
ragged step, (b) the eager device-positioned step, (c) ONE captured device-positioned step replayed (`torch.cuda.graph`); then the same
three with the fla layer's q / k prologue (relu + rotary) -- for (a) the chain the layer runs today: two `index_select`s of the tables
at the device positions, two `featmap_rotary` launches, the ragged step; for (b), (c) the prologue fused into the step.  Every variant
(the graph too) starts with the 4 B-byte copy that puts the device positions back, so that every call is the same step.  Alternating in
one run, `--reps` times: wall time per call (events around `--steps` calls or replays) with median, min, max; device time of the
library's kernels for the eager variants (the per-launch event hook cannot see inside a replay, whose wall time is GPU-side).
Then a GPT 340M decode step (24 layers, bf16, B = 8, prompt 100): eager on an ordinary cache, eager device-positioned, and the captured
whole-model step replayed; the positions advance (a boundary every 64th step is part of the average).  Last line: the GPU kernels one
layer's decode step launches before and after (torch.profiler; null where the profiler gives no device events).

`--mixed`: a mixed serving batch at the C5 head (H = 4, K = 128, V = 256, bf16, L = 128), B = 8: seven sequences at positions of their
own (chunks 13 .. 17, every one at another place in its chunk, none on a boundary) decode ONE token each while the eighth takes a
256-token slice of a long prompt (from position 1000: it closes four chunks).  (a) ONE `mhla_causal_extend(counts=, left_padded=True)`
call -- the ragged launch chain -- against (b) what such a batch costs without it: one `mhla_causal_extend` per sequence on its B = 1
slice of the same state (for one token that is the step).  Alternating in one run, `--reps` times, `--steps` calls each: wall time per
call with median, min and max, the device time of the library's kernels and the launches per call (the per-launch event hook).  The
state is put back before every call -- host mirror and a 32-byte device copy of the positions, given to both variants -- so that every
call is the same work.

`--packed-prefill`: the same eight prompts (100 .. 2048 tokens, all different) prefilled two ways at the C5 head (H = 4, K = 128,
V = 256, bf16, L = 128, a state of 40 chunks per sequence): (a) left-padded to [8, 2048] through `mhla_causal_prefill(lengths=,
left_padded=True)` -- one operator call and one state chain per run of equal lengths, here per prompt -- and (b) packed to [1, sum]
through `mhla_causal_prefill(cu_seqlens=plan)` -- one operator call over the pack, one state chain (`mhla_causal_varlen_state_init`).
Alternating in one run, `--reps` times, `--steps` calls each (at most 20): wall time per call with median, min and max, the device time
of the library's kernels and its launches per call (the per-launch event hook); the same for the state half alone
(`mhla_causal_state`).  The plan is built once, outside the timed calls, as a server builds it once per batch for all layers.

`--speculative`: one round of speculative decoding at the 340M layer shape (H = 4, K = 128, V = 256, bf16, L = 128), a history of 2048
tokens, a draft of k = 4 (the verify sees 5 tokens: the last one and the draft), B = 1 and 8: (a) `mhla_causal_verify` + `mhla_causal_commit`
of all 5, (b) the same with 2 of 5 accepted, (c) the round without them -- `CausalState.clone()` (4 K V bytes per chunk and head of S),
`mhla_causal_extend(counts=)` on the clone -- and (d) five exact steps (`mhla_causal_step` on the uniform state; 2048 .. 2052: no
boundary).  Alternating in one run, `--reps` times, `--steps` calls each: wall time per call with median, min and max, the device time of
the library's kernels and its launches per call (the per-launch event hook).  The state is put back before every call -- host mirror and
a 4 B-byte device copy of the positions, given to every variant -- so that every call is the same work.

`--gqa`: grouped-query heads (`mhla_causal_step` with k, v and the state on Hkv heads, q on H) beside the repeated-head step on a
state of H heads, at B = 8, H = 16, Hkv = 4 and 2, K = 128, V = 256, 32 chunks seen: the ordinary step and the one that closes a chunk,
alternating in one run, `--reps` times, `--steps` calls each -- wall and device time per call (median, min, max), the kernels' device
times, the bytes of state a step moves and the state's size.

`--gqa-prefill`: the grouped-query prefill operator (`mhla_causal` / `mhla_causal_normgate` on k, v of Hkv heads, no graph) beside the
repeated-head path it replaces (`repeat_interleave` of k and v, then the operator on H heads) at B = 1, T = 8192, H = 16, Hkv = 8, 4, 2,
K = 128, V = 256, bf16, `summaries="tf32"`, plain and with the fused norm x gate epilogue.  Both paths run in one process, alternating,
`--reps` times, `--steps` calls each after a warm-up of both: device-event time per call (median, min, max: the spread of repeated
identical runs), the kernels' device times, the workspace each path asks for and the peak of `torch.cuda.max_memory_allocated` over
one call above what the inputs hold.

`--slots`: the step on chosen slots of a state pool (`CausalState.at`) at the C5 head (H = 4, K = 128, V = 256, bf16, L = 128), B = 8 and
32, lengths as for `--ragged`, non-boundary steps: (a) the un-slotted ragged step and device-positioned step on a compact state of B
rows, (b) the same batch through a permuted view of a pool of 2 B slots (the host-positioned view for the step, a map on the device for
the device-positioned step), (c) what a pool costs without views: `index_select` the live rows of S, P, Cur and pos into a fresh
state, step it, `index_copy_` P, Cur and pos back (S does not change off a boundary: the cheapest honest form of it).  Alternating in
one run, `--reps` times (at least four), `--steps` calls each (a quarter of them for (c)): wall time per call and, for (a) and (b), the
device time of the library's kernels, each with median, min and max.  Positions and host mirror are put back before every call, for
every variant, so that every call is the same step.  On a tree without `CausalState.at` the same command times (a) alone: the
figure to hold the un-slotted path of a later tree against.

`--paged`: the step on a PAGED pool (`PagedCausalState`) beside the dense pool and the compact state, at the shape, batches and lengths of
`--slots`, and at two places: "off" (the lengths of `--slots`, no sequence on a boundary) and "boundary" (every sequence at
pos % 64 == 63, the one case in which a step reads S through the page table: its roll closes the chunk and mixes the finished ones).
Variants, alternating in one run, `--reps` times, `--steps` calls each: (a) `compact_*`, the un-slotted step and device-positioned step
on a compact state of B rows, (b) `view_*`, the same through a permuted view of a dense pool of 2 B slots, (c) `paged_*`, through the
same view of a paged pool whose table is a random permutation of its pages (every page the steps touch assigned beforehand).  Wall and
device time per call (median, min, max), the kernels' device times, and the bytes of the dense and the paged pool.  Positions and host
mirror are put back before every call.  On a tree without `PagedCausalState` the same command times (a) and (b): the figures to hold
the un-paged paths of a later tree against.

`--paged-h16`: `--paged` at B = 4 and 32 with a fourth variant, (d) `h16_*`: the same view of a paged pool of h16 pages
(`PagedCausalState(..., page_mult=)`: 2 bytes an element and one multiplier per 64, the same table) -- off a boundary, where the step
reads P and Cur alone, and on one, where the roll encodes the closing chunk and mixes the decoded pages.  Then the PACK PREFILL into
the slots (`mhla_causal_state(k, v, mix, cu_seqlens=plan, into=view)`, the B sequences at the "off" lengths, about 1000 tokens each)
into the fp32 paged pool and into the h16 pool (state kernel into a staging area, `k_cs_page_encode`, roll): wall and device time per
call, the kernels' device times, and the bytes of both pools.

`--packed`: PACKED new tokens (`mhla_causal_extend(cu_seqlens=)`) beside the padded ragged call, at the C5 head (H = 4, K = 128,
V = 256, bf16, L = 128), B = 8 and 32, on the mixed step of continuous batching: B - 1 decoders at positions of their own take ONE
token each and the last sequence a 256-token slice of a prompt (from position 1000: it closes four chunks).  Variants, alternating
in one run, `--reps` times, `--steps` calls each: `padded_extend` (`counts=`, tokens padded to [B, 256]), `padded_verify`,
`ragged_step` (the single-token step of the same B sequences) -- the EXISTING paths, which the same command times on a tree
without `cu_seqlens` too: the figures to hold them against --, then `packed_extend` ([1, B + 255] tokens), `padded_from_pack` (what a
caller who holds a pack pays today: scatter the pack into zeroed padded tensors, the padded call, gather the rows back) and, at EQUAL
tokens (every sequence 64 tokens from position 1000), `equal_padded` / `equal_packed`.  Wall and device time per call (median, min,
max), the kernels' device times, launches per call, and the bytes of workspace and token tensors (q, k, v and the rows) of both
layouts.  Positions and host mirror are put back before every call, for every variant.  `--packed --existing-only` times the existing
paths alone on a tree that has `cu_seqlens` as well: the process then does exactly the work of the older tree's, which is what a
comparison of the two builds needs (a process that also runs the packed variants differs in more than its library).

`--pool-layer`: a scheduler step of continuous batching through the fla LAYER on a `PagedDecodeCache` (a bf16 layer of the 340M shape:
hidden 1024, 4 heads, K = 128, V = 256, 32 chunks), at two mixes -- `decode`: 32 requests x 1 token; `mixed`: 31 x 1 token + one
256-token slice of a prompt (from position 1000: it closes four chunks) --, every sequence at a position of its own around 1000,
positions and host mirrors put back before every call.  Three tables, alternating variants, `--reps` times, `--steps` calls each:
the PROLOGUE alone, `featmap_rotary_decode` (one `k_fr_decode` launch reading positions and slot map on the device) against today's
sequence for the same pack (position arithmetic with torch ops -- arange, searchsorted, adds --, two `index_select`s of the tables, two
`k_fmap_rotary` launches): wall time from HIP events and the device time of the library's kernels from the per-launch hook (the torch
kernels of today's path are in its wall time only); the whole LAYER step on the pool against the existing padded `DecodeCache` call
with `token_counts` ([32, 1, D] / [32, 256, D]); and the HOST's share of a model step across 24 layers -- `schedule` once, then per
layer the view of the pool, the capacity check and the page rule, timed with the host clock and no launch -- in the steady state
and on a step in which every request opens a new chunk (a page and a table row pushed per request and layer): the figure a
follow-up on one page table shared by all layers would rest on.  Also the prologue kernel on a pack of 32 x 512 tokens with its
rows on and off 16-byte boundaries: 16-byte against 8-byte pieces.

`--swap`: `PagedCausalState.swap_out` / `swap_in` on the pools of `--paged` / `--paged-h16` (H = 4, K = 128, V = 256, 2 B slots, 19 pages a
slot, a random table), the B sequences at the "off" lengths (about 1000 tokens, 13 .. 17 finished pages each), B = 4 and 32, fp32 and
h16 pages.  Device blob: wall time per call (events around `--steps` calls, at most 100) and the device time of the swap kernel (the
per-launch event hook), beside the torch expressions that move the same bytes -- `pages[idx]`, `P[idx]`, `Cur[idx]` (what `compact()`
does) and the indexed assignments back -- and a plain device `copy_` of the blob's byte count: the session's copy rate.  Host blob:
wall time of a swap out and of a swap in (after a `reset` of the target slots) with a synchronise, beside a pinned `copy_` of the
same byte count in each direction, the link's ceiling.  GB/s counts the blob's bytes once.  Last, for context: the device time of
the state half of a re-prefill of the same sequences (`mhla_causal_state(..., cu_seqlens=plan, into=view)`), a lower bound on what
losing the state costs, since a real re-prefill runs the whole model.

`--workload`: no timing, just a prefill and 192 real steps (three boundaries) at B = 1, H = 4, K = 128, V = 256 -- the program to put
after `rocprofv3 --kernel-trace --stats -d <dir> --` for a trace of its own."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench_configs import kernel_times  # noqa: E402
import mhla_amd  # noqa: E402
from mhla_amd import causal_mixing_init  # noqa: E402

DEV = "cuda"
L = 128


def batch_us(fn, iters, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def spread(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def token(B, H, K, V, g):
    mk = lambda D: torch.randn(B, 1, H, D, generator=g).to(torch.bfloat16).to(DEV)
    return mk(K), mk(K), mk(V)


def config(B, H, K, V, pos, steps, reps, parent_iters):
    g = torch.Generator().manual_seed(1)
    mix = causal_mixing_init(L).reshape(L, L).to(DEV)
    q, k, v = token(B, H, K, V, g)
    i = pos // 64
    state = mhla_amd.CausalState.empty(B, H, K, V, L, DEV)
    state.S[:, :, :i + 1].normal_(0, 0.1)        # finished chunks the boundary step reads
    state.P.normal_(0, 0.1)
    T = pos + 1
    qT, kT = (torch.randn(B, T, H, K, generator=g).to(torch.bfloat16).to(DEV) for _ in range(2))
    vT = torch.randn(B, T, H, V, generator=g).to(torch.bfloat16).to(DEV)
    roll_pos = i * 64 + 63

    def step():
        state.seen = pos
        mhla_amd.mhla_causal_step(q, k, v, mix, state)

    def roll():
        state.seen = roll_pos
        mhla_amd.mhla_causal_step(q, k, v, mix, state)

    def parent():
        mhla_amd.mhla_causal(qT, kT, vT, mix)

    t_step, t_roll, t_parent = [], [], []
    with torch.no_grad():
        for _ in range(reps):
            t_step.append(batch_us(step, steps))
            t_roll.append(batch_us(roll, steps))
            t_parent.append(batch_us(parent, parent_iters, warm=2))
            state.Cur.zero_()                     # (the repeated step keeps adding the same k (x) v: keep it small)
        ks = {n: round(us, 2) for n, us in kernel_times(step, iters=20).items()}
        kr = {n: round(us, 2) for n, us in kernel_times(roll, iters=20).items()}
    nbytes = 3 * B * H * K * V * 4 + B * H * (2 * K + 2 * V) * 2
    dev_step = ks.get("k_cs_step", 0.0) + ks.get("k_cs_step_finish", 0.0)
    rec = {"B": B, "H": H, "K": K, "V": V, "pos": pos, "chunk": i, "steps_per_batch": steps, "reps": reps,
           "step_us": spread(t_step), "roll_step_us": spread(t_roll), "roll_pos": roll_pos,
           "parent_fwd_us": spread(t_parent), "parent_tokens": T,
           "step_kernels_us": ks, "roll_step_kernels_us": kr,
           "step_bytes": nbytes, "step_GBps_wall": round(nbytes / (statistics.median(t_step) * 1e-6) / 1e9, 1),
           "step_GBps_device": round(nbytes / (dev_step * 1e-6) / 1e9, 1) if dev_step else None,
           "roll_bytes": (i + 1) * B * H * K * V * 4 + 3 * B * H * K * V * 4,
           "state_MB": round(state.nbytes / 2 ** 20, 1)}
    print(json.dumps(rec), flush=True)
    return rec


def roll_sweep(B, H, K, V, steps):
    """How the boundary step grows with the number of finished chunks: k_cs_roll reads (i + 1) K V 4 bytes per (b, h)."""
    g = torch.Generator().manual_seed(1)
    mix = causal_mixing_init(L).reshape(L, L).to(DEV)
    q, k, v = token(B, H, K, V, g)
    state = mhla_amd.CausalState.empty(B, H, K, V, L, DEV)
    state.S.normal_(0, 0.1)
    out = {}
    with torch.no_grad():
        for i in (0, 1, 7, 15, 31, 63, 95, 125):
            def roll():
                state.seen = i * 64 + 63
                mhla_amd.mhla_causal_step(q, k, v, mix, state)
            wall = batch_us(roll, steps)
            out[i] = {"wall_us": round(wall, 2), "k_cs_roll_us": round(kernel_times(roll, iters=20).get("k_cs_roll", 0.0), 2),
                      "roll_bytes": (i + 1) * B * H * K * V * 4 + 3 * B * H * K * V * 4}
    print(json.dumps({"roll_sweep": {"B": B, "H": H, "K": K, "V": V}, "by_chunk": out}), flush=True)


def ragged_config(B, H, K, V, steps, reps):
    g = torch.Generator().manual_seed(1)
    mix = causal_mixing_init(L).reshape(L, L).to(DEV)
    q, k, v = token(B, H, K, V, g)
    i0 = 15
    chunks = [i0 + (-2, -1, 1, 2)[b % 4] for b in range(B)]

    def make(lengths):
        st = mhla_amd.CausalState.empty(B, H, K, V, L, DEV)
        st.S[:, :, :i0 + 3].normal_(0, 0.1)
        st.P.normal_(0, 0.1)
        return st if lengths is None else mhla_amd.CausalState(st.S, st.P, st.Cur, lengths=lengths)

    len_step = tuple(c * 64 + (7 * b) % 63 for b, c in enumerate(chunks))
    len_roll = tuple(c * 64 + 63 for c in chunks)
    uni, rag = make(None), make(len_step)
    pos_step, pos_roll = (torch.tensor(x, dtype=torch.int32, device=DEV) for x in (len_step, len_roll))
    spare = torch.empty_like(pos_roll)

    def put_back(lengths):
        rag.lengths, rag.seen = lengths, max(lengths)

    def u_step():
        uni.seen = i0 * 64 + 36
        spare.copy_(pos_step)
        mhla_amd.mhla_causal_step(q, k, v, mix, uni)

    def r_step():
        put_back(len_step)
        rag.pos.copy_(pos_step)
        mhla_amd.mhla_causal_step(q, k, v, mix, rag)

    def u_roll():
        uni.seen = i0 * 64 + 63
        spare.copy_(pos_roll)
        mhla_amd.mhla_causal_step(q, k, v, mix, uni)

    def r_roll():
        put_back(len_roll)
        rag.pos.copy_(pos_roll)
        mhla_amd.mhla_causal_step(q, k, v, mix, rag)

    wall = {n: [] for n in ("uniform_step", "ragged_step", "uniform_roll", "ragged_roll")}
    dev = {n: [] for n in wall}
    kern = {}
    fns = {"uniform_step": u_step, "ragged_step": r_step, "uniform_roll": u_roll, "ragged_roll": r_roll}
    with torch.no_grad():
        for _ in range(reps):
            for n, fn in fns.items():
                wall[n].append(batch_us(fn, steps))
            for n, fn in fns.items():
                kern[n] = kernel_times(fn, iters=20)
                dev[n].append(sum(kern[n].values()))
            uni.Cur.zero_()
            rag.Cur.zero_()
    nbytes = 3 * B * H * K * V * 4 + B * H * (2 * K + 2 * V) * 2
    rec = {"ragged": {"B": B, "H": H, "K": K, "V": V, "chunks": sorted(set(chunks)), "uniform_chunk": i0}, "steps_per_batch": steps, "reps": reps,
           "wall_us": {n: spread(x) for n, x in wall.items()}, "device_us": {n: spread(x) for n, x in dev.items()},
           "kernels_us": {n: {kn: round(us, 2) for kn, us in ks.items()} for n, ks in kern.items()},
           "step_bytes": {"uniform": nbytes, "ragged": nbytes + 4 * B},
           "ragged_step_device_within_uniform_spread": min(dev["uniform_step"]) <= statistics.median(dev["ragged_step"]) <= max(dev["uniform_step"])}
    print(json.dumps(rec), flush=True)
    return rec


def gqa_config(B, H, Hkv, K, V, steps, reps, chunks_seen=32):
    """Grouped-query heads: the ragged step on a state of Hkv heads (k, v un-repeated) beside the repeated-head step on a state of H
    heads (what a layer without `grouped_state` runs), every sequence `chunks_seen` chunks in; the ordinary step and the one that
    closes a chunk, alternating in one run."""
    g = torch.Generator().manual_seed(1)
    mix = causal_mixing_init(L).reshape(L, L).to(DEV)
    G = H // Hkv
    q = torch.randn(B, 1, H, K, generator=g).to(torch.bfloat16).to(DEV)
    k = torch.randn(B, 1, Hkv, K, generator=g).to(torch.bfloat16).to(DEV)
    v = torch.randn(B, 1, Hkv, V, generator=g).to(torch.bfloat16).to(DEV)
    kr, vr = k.repeat_interleave(G, 2), v.repeat_interleave(G, 2)
    len_step, len_roll = (chunks_seen * 64 + 36,) * B, (chunks_seen * 64 + 63,) * B
    pos_step, pos_roll = (torch.tensor(x, dtype=torch.int32, device=DEV) for x in (len_step, len_roll))

    def make(heads):
        st = mhla_amd.CausalState.empty(B, heads, K, V, L, DEV)
        st.S[:, :, :chunks_seen + 1].normal_(0, 0.1)
        st.P.normal_(0, 0.1)
        return mhla_amd.CausalState(st.S, st.P, st.Cur, lengths=len_step)

    grouped, repeated = make(Hkv), make(H)

    def run(state, kk, vv, lengths, pos):
        def fn():
            state.lengths, state.seen = lengths, max(lengths)
            state.pos.copy_(pos)
            mhla_amd.mhla_causal_step(q, kk, vv, mix, state)
        return fn

    fns = {"repeated_step": run(repeated, kr, vr, len_step, pos_step), "grouped_step": run(grouped, k, v, len_step, pos_step),
           "repeated_roll": run(repeated, kr, vr, len_roll, pos_roll), "grouped_roll": run(grouped, k, v, len_roll, pos_roll)}
    wall, dev, kern = {n: [] for n in fns}, {n: [] for n in fns}, {}
    with torch.no_grad():
        for _ in range(reps):
            for n, fn in fns.items():
                wall[n].append(batch_us(fn, steps))
            for n, fn in fns.items():
                kern[n] = kernel_times(fn, iters=20)
                dev[n].append(sum(kern[n].values()))
            grouped.Cur.zero_()
            repeated.Cur.zero_()
    state_bytes = lambda heads: 3 * B * heads * K * V * 4
    rec = {"gqa": {"B": B, "H": H, "Hkv": Hkv, "G": G, "K": K, "V": V, "chunks_seen": chunks_seen}, "steps_per_batch": steps, "reps": reps,
           "wall_us": {n: spread(x) for n, x in wall.items()}, "device_us": {n: spread(x) for n, x in dev.items()},
           "kernels_us": {n: {kn: round(us, 2) for kn, us in ks.items()} for n, ks in kern.items()},
           "step_state_traffic_bytes": {"repeated": state_bytes(H), "grouped": state_bytes(Hkv)},
           "state_MB_at_chunks_seen": {"repeated": round((chunks_seen + 2) * B * H * K * V * 4 / 2 ** 20, 1),
                                       "grouped": round((chunks_seen + 2) * B * Hkv * K * V * 4 / 2 ** 20, 1)},
           "state_MB_allocated": {"repeated": round(repeated.nbytes / 2 ** 20, 1), "grouped": round(grouped.nbytes / 2 ** 20, 1)}}
    print(json.dumps(rec), flush=True)
    return rec


def graph_config(B, H, K, V, steps, reps):
    g = torch.Generator().manual_seed(1)
    mix = causal_mixing_init(L).reshape(L, L).to(DEV)
    q, k, v = token(B, H, K, V, g)
    i0 = 15
    chunks = [i0 + (-2, -1, 1, 2)[b % 4] for b in range(B)]
    lengths = tuple(c * 64 + (7 * b) % 63 for b, c in enumerate(chunks))
    pos0 = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    inv = 1.0 / (10000.0 ** (torch.arange(0, K, 2, dtype=torch.float32) / K))
    fr = torch.outer(torch.arange(64 * L, dtype=torch.float32), inv)
    cos, sin = torch.cos(fr).to(torch.bfloat16).to(DEV), torch.sin(fr).to(torch.bfloat16).to(DEV)

    def make():
        st = mhla_amd.CausalState.empty(B, H, K, V, L, DEV)
        st.S[:, :, :i0 + 3].normal_(0, 0.1)
        st.P.normal_(0, 0.1)
        st = mhla_amd.CausalState(st.S, st.P, st.Cur, lengths=lengths)
        st.full
        return st

    rag, dev, rep, rep_pro = make(), make(), make(), make()

    def ragged():
        rag.lengths, rag.seen = lengths, max(lengths)
        rag.pos.copy_(pos0)
        mhla_amd.mhla_causal_step(q, k, v, mix, rag)

    def ragged_pro():   # the layer's chain today: tables gathered at the device positions, two prologue launches, the ragged step
        rag.lengths, rag.seen = lengths, max(lengths)
        rag.pos.copy_(pos0)
        p = rag.pos.long()
        c, s = cos.index_select(0, p), sin.index_select(0, p)
        qq = mhla_amd.featmap_rotary(q.reshape(1, B, H, K), c, s, "relu", 0).reshape(B, 1, H, K)
        kk = mhla_amd.featmap_rotary(k.reshape(1, B, H, K), c, s, "relu", 0).reshape(B, 1, H, K)
        mhla_amd.mhla_causal_step(qq, kk, v, mix, rag)

    def dev_step(st=dev, **kw):
        st.pos.copy_(pos0)
        return mhla_amd.mhla_causal_step_dev(q, k, v, mix, st, **kw)

    dev_pro = lambda st=dev: dev_step(st, feature_map="relu", rotary=(cos, sin))
    graphs = {}
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            dev_step(rep), dev_pro(rep_pro)
        torch.cuda.current_stream().wait_stream(side)
        for name, fn, st in (("replay", dev_step, rep), ("replay_pro", dev_pro, rep_pro)):
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                fn(st)
    fns = {"ragged": ragged, "dev": dev_step, "replay": graphs["replay"].replay,
           "ragged_pro": ragged_pro, "dev_pro": dev_pro, "replay_pro": graphs["replay_pro"].replay}
    wall = {n: [] for n in fns}
    devt = {n: [] for n in fns if not n.startswith("replay")}
    kern = {}
    with torch.no_grad():
        for _ in range(reps):
            for n, fn in fns.items():
                wall[n].append(batch_us(fn, steps))
            for n in devt:
                kern[n] = kernel_times(fns[n], iters=20)
                devt[n].append(sum(kern[n].values()))
            for st in (rag, dev, rep, rep_pro):
                st.Cur.zero_()
    rec = {"graph": {"B": B, "H": H, "K": K, "V": V, "chunks": sorted(set(chunks))}, "steps_per_batch": steps, "reps": reps,
           "wall_us": {n: spread(x) for n, x in wall.items()}, "device_us": {n: spread(x) for n, x in devt.items()},
           "kernels_us": {n: {kn: round(us, 2) for kn, us in ks.items()} for n, ks in kern.items()},
           "replay_median_below_min_eager_ragged": statistics.median(wall["replay"]) < min(wall["ragged"]),
           "replay_pro_median_below_min_eager_ragged_pro": statistics.median(wall["replay_pro"]) < min(wall["ragged_pro"])}
    print(json.dumps(rec), flush=True)
    return rec


def slots_config(B, H, K, V, steps, reps):
    g = torch.Generator().manual_seed(1)
    mix = causal_mixing_init(L).reshape(L, L).to(DEV)
    q, k, v = token(B, H, K, V, g)
    i0 = 15
    chunks = [i0 + (-2, -1, 1, 2)[b % 4] for b in range(B)]
    lengths = tuple(c * 64 + (7 * b) % 63 for b, c in enumerate(chunks))
    n_slots = 2 * B
    slots = torch.randperm(n_slots, generator=g)[:B].tolist()

    def make(rows, lens):
        st = mhla_amd.CausalState.empty(rows, H, K, V, L, DEV)
        st.S[:, :, :i0 + 3].normal_(0, 0.1)
        st.P.normal_(0, 0.1)
        st = mhla_amd.CausalState(st.S, st.P, st.Cur, lengths=lens)
        st.full
        return st

    rag = make(B, lengths)
    pos0 = torch.tensor(lengths, dtype=torch.int32, device=DEV)

    def put_back(st, lens, pos):
        st.lengths, st.seen, st.stale = lens, max(lens), False
        st.pos.copy_(pos)

    def compact_step():
        put_back(rag, lengths, pos0)
        mhla_amd.mhla_causal_step(q, k, v, mix, rag)

    def compact_dev():
        put_back(rag, lengths, pos0)
        mhla_amd.mhla_causal_step_dev(q, k, v, mix, rag)

    fns = {"compact_step": compact_step, "compact_dev": compact_dev}
    states = [rag]
    if hasattr(mhla_amd.CausalState, "at"):
        pool_lengths = [0] * n_slots
        for s_, n in zip(slots, lengths):
            pool_lengths[s_] = n
        pool_lengths = tuple(pool_lengths)
        pool = make(n_slots, pool_lengths)
        pool_pos0 = torch.tensor(pool_lengths, dtype=torch.int32, device=DEV)
        idx = torch.tensor(slots, dtype=torch.int64, device=DEV)
        view, dev_view = pool.at(slots), pool.at(idx.to(torch.int32))
        states.append(pool)

        def view_step():
            put_back(pool, pool_lengths, pool_pos0)
            mhla_amd.mhla_causal_step(q, k, v, mix, view)

        def view_dev():
            put_back(pool, pool_lengths, pool_pos0)
            mhla_amd.mhla_causal_step_dev(q, k, v, mix, dev_view)

        def gather_scatter():
            put_back(pool, pool_lengths, pool_pos0)
            live = mhla_amd.CausalState(pool.S.index_select(0, idx), pool.P.index_select(0, idx), pool.Cur.index_select(0, idx), lengths=lengths,
                                        pos=pool.pos.index_select(0, idx))
            mhla_amd.mhla_causal_step(q, k, v, mix, live)
            pool.P.index_copy_(0, idx, live.P)
            pool.Cur.index_copy_(0, idx, live.Cur)
            pool.pos.index_copy_(0, idx, live.pos)

        fns.update(view_step=view_step, view_dev=view_dev, gather_scatter=gather_scatter)
    wall = {n: [] for n in fns}
    dev = {n: [] for n in fns if n != "gather_scatter"}
    kern = {}
    with torch.no_grad():
        for _ in range(max(4, reps)):
            for n, fn in fns.items():
                wall[n].append(batch_us(fn, max(10, steps // 4) if n == "gather_scatter" else steps))
            for n in dev:
                kern[n] = kernel_times(fns[n], iters=20)
                dev[n].append(sum(kern[n].values()))
            for st in states:
                st.Cur.zero_()
    med = {n: statistics.median(x) for n, x in wall.items()}
    rec = {"slots": {"B": B, "H": H, "K": K, "V": V, "n_slots": n_slots, "slots": slots, "chunks": sorted(set(chunks))}, "steps_per_batch": steps,
           "reps": max(4, reps), "wall_us": {n: spread(x) for n, x in wall.items()}, "device_us": {n: spread(x) for n, x in dev.items()},
           "kernels_us": {n: {kn: round(us, 2) for kn, us in ks.items()} for n, ks in kern.items()}}
    if "view_step" in fns:
        rec["view_over_compact_device"] = {h: round(statistics.median(dev["view_" + h]) / statistics.median(dev["compact_" + h]), 3) for h in ("step", "dev")}
        rec["view_over_compact_wall"] = {h: round(med["view_" + h] / med["compact_" + h], 3) for h in ("step", "dev")}
        rec["gather_scatter_over_compact_wall"] = round(med["gather_scatter"] / med["compact_step"], 2)
        rec["pool_MB"] = round(pool.nbytes / 2 ** 20, 1)
    print(json.dumps(rec), flush=True)
    return rec


def paged_config(B, H, K, V, steps, reps, h16=False):
    g = torch.Generator().manual_seed(1)
    mix = causal_mixing_init(L).reshape(L, L).to(DEV)
    q, k, v = token(B, H, K, V, g)
    i0 = 15
    chunks = [i0 + (-2, -1, 1, 2)[b % 4] for b in range(B)]
    places = {"off": tuple(c * 64 + (7 * b) % 63 for b, c in enumerate(chunks)), "boundary": tuple(c * 64 + 63 for c in chunks)}
    n_slots = 2 * B
    slots = torch.randperm(n_slots, generator=g)[:B].tolist()
    idx = torch.tensor(slots, dtype=torch.int64, device=DEV)
    held = i0 + 4   # chunks a slot holds pages for: every one a step here reads or closes, and the one it opens

    def spread_over_pool(lens):
        out = [0] * n_slots
        for s_, n in zip(slots, lens):
            out[s_] = n
        return tuple(out)

    def dense(rows):
        st = mhla_amd.CausalState.empty(rows, H, K, V, L, DEV)
        st.S[:, :, :held].normal_(0, 0.1)
        st.P.normal_(0, 0.1)
        st = mhla_amd.CausalState(st.S, st.P, st.Cur, lengths=(0,) * rows)
        st.full
        return st

    rag, pool = dense(B), dense(n_slots)
    states = {"compact": (rag, rag, rag, lambda lens: lens), "view": (pool, pool.at(slots), pool.at(idx.to(torch.int32)), spread_over_pool)}
    nbytes = {"dense_pool_MB": round(pool.nbytes / 2 ** 20, 1)}
    if hasattr(mhla_amd, "PagedCausalState"):
        n_pages = n_slots * held
        perm = torch.randperm(n_pages, generator=g).tolist()
        table = [perm[s_ * held:(s_ + 1) * held] + [-1] * (L - held) for s_ in range(n_slots)]
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=DEV)
        paged = mhla_amd.PagedCausalState(z(n_pages, H, K, V).normal_(0, 0.1), z(n_slots, H, K, V).normal_(0, 0.1), z(n_slots, H, K, V), table)
        paged.full
        states["paged"] = (paged, paged.at(slots), paged.at(idx.to(torch.int32)), spread_over_pool)
        nbytes["paged_pool_MB"] = round(paged.nbytes / 2 ** 20, 1)
        if h16:   # the same table over 2-byte pages: a payload at the fp16 range's upper end, every multiplier 2^-17
            pay = (z(n_pages, H, K, V).normal_(0, 0.1) * 2.0 ** 17).half()
            hp = mhla_amd.PagedCausalState(pay, z(n_slots, H, K, V).normal_(0, 0.1), z(n_slots, H, K, V), table,
                                           page_mult=torch.full((n_pages, H, K * V // 64), 2.0 ** -17, dtype=torch.float32, device=DEV))
            hp.full
            states["h16"] = (hp, hp.at(slots), hp.at(idx.to(torch.int32)), spread_over_pool)
            nbytes["h16_pool_MB"] = round(hp.nbytes / 2 ** 20, 1)
    fns = {}
    for place, lens in places.items():
        for name, (st, host_view, dev_view, over) in states.items():
            lens_ = over(lens)
            pos0 = torch.tensor(lens_, dtype=torch.int32, device=DEV)

            def step(st=st, view=host_view, lens_=lens_, pos0=pos0):
                st.lengths, st.seen, st.stale = lens_, max(lens_), False
                st.pos.copy_(pos0)
                mhla_amd.mhla_causal_step(q, k, v, mix, view)

            def dev(st=st, view=dev_view, lens_=lens_, pos0=pos0):
                st.lengths, st.seen, st.stale = lens_, max(lens_), False
                st.pos.copy_(pos0)
                mhla_amd.mhla_causal_step_dev(q, k, v, mix, view)

            fns[f"{name}_step@{place}"], fns[f"{name}_dev@{place}"] = step, dev
    wall, devt, kern = {n: [] for n in fns}, {n: [] for n in fns}, {}
    with torch.no_grad():
        for _ in range(reps):
            for n, fn in fns.items():
                wall[n].append(batch_us(fn, steps))
            for n, fn in fns.items():
                kern[n] = kernel_times(fn, iters=20)
                devt[n].append(sum(kern[n].values()))
            for st, *_ in states.values():
                st.Cur.zero_()
    prefill = {}
    if "h16" in states:   # last: a prefill starts its slots anew and takes the lowest free pages, which ends the random table
        lens = places["off"]
        cu = [0]
        for n in lens:
            cu.append(cu[-1] + n)
        plan = mhla_amd.causal_varlen_plan(cu, DEV)
        kc = torch.randn(1, cu[-1], H, K, generator=g).to(torch.bfloat16).to(DEV)
        vc = torch.randn(1, cu[-1], H, V, generator=g).to(torch.bfloat16).to(DEV)
        pf = {}
        for name in ("paged", "h16"):
            st, view = states[name][:2]

            def fill(st=st, view=view):
                st.stale = False
                mhla_amd.mhla_causal_state(kc, vc, mix, cu_seqlens=plan, into=view)

            pf[name] = fill
        pw, pd, pk = {n: [] for n in pf}, {n: [] for n in pf}, {}
        with torch.no_grad():
            for _ in range(reps):
                for n, fn in pf.items():
                    pw[n].append(batch_us(fn, min(20, steps), warm=2))
                for n, fn in pf.items():
                    pk[n] = kernel_times(fn, iters=5)
                    pd[n].append(sum(pk[n].values()))
        prefill = {"prefill": {"tokens": cu[-1], "pack_chunks": plan.n_chunks, "wall_us": {n: spread(x) for n, x in pw.items()},
                               "device_us": {n: spread(x) for n, x in pd.items()},
                               "kernels_us": {n: {kn: round(us, 2) for kn, us in ks.items()} for n, ks in pk.items()}}}
    rec = {"paged": {"B": B, "H": H, "K": K, "V": V, "n_slots": n_slots, "slots": slots, "chunks": sorted(set(chunks)), "pages_per_slot": held},
           "steps_per_batch": steps, "reps": reps, **nbytes, "wall_us": {n: spread(x) for n, x in wall.items()},
           "device_us": {n: spread(x) for n, x in devt.items()},
           "kernels_us": {n: {kn: round(us, 2) for kn, us in ks.items()} for n, ks in kern.items()}, **prefill}
    print(json.dumps(rec), flush=True)
    return rec


def swap_config(B, H, K, V, steps, reps):
    import time
    g = torch.Generator().manual_seed(1)
    mix = causal_mixing_init(L).reshape(L, L).to(DEV)
    i0 = 15
    chunks = [i0 + (-2, -1, 1, 2)[b % 4] for b in range(B)]
    lens = tuple(c * 64 + (7 * b) % 63 for b, c in enumerate(chunks))   # the "off" lengths of --paged: about 1000 tokens each
    n_slots, held = 2 * B, i0 + 4
    slots = torch.randperm(n_slots, generator=g)[:B].tolist()
    n_pages = n_slots * held
    perm = torch.randperm(n_pages, generator=g).tolist()
    table = [perm[s_ * held:(s_ + 1) * held] + [-1] * (L - held) for s_ in range(n_slots)]
    lengths = [0] * n_slots
    for s_, n in zip(slots, lens):
        lengths[s_] = n
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=DEV)

    def make(fmt, filled=True):
        tab, lng = (table, lengths) if filled else ([[-1] * L for _ in range(n_slots)], None)
        if fmt == "h16":
            pool = mhla_amd.PagedCausalState((z(n_pages, H, K, V).normal_(0, 0.1) * 2.0 ** 17).half(), z(n_slots, H, K, V).normal_(0, 0.1), z(n_slots, H, K, V), tab,
                                             lengths=lng, page_mult=torch.full((n_pages, H, K * V // 64), 2.0 ** -17, dtype=torch.float32, device=DEV))
        else:
            pool = mhla_amd.PagedCausalState(z(n_pages, H, K, V).normal_(0, 0.1), z(n_slots, H, K, V).normal_(0, 0.1), z(n_slots, H, K, V), tab, lengths=lng)
        pool.full
        return pool

    def wall_sync_us(fn, iters=5):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e6

    idx = torch.tensor(slots, dtype=torch.int64, device=DEV)
    out = {}
    for fmt in ("fp32", "h16"):
        src, dst = make(fmt), make(fmt, filled=False)
        blob = src.swap_out(slots, device=DEV, release=False)
        pidx = torch.tensor([p for s_ in slots for p in src.table[s_][:src.lengths[s_] // 64]], dtype=torch.int64, device=DEV)
        nbytes = blob.nbytes
        flat = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        host_blob = src.swap_out(slots, release=False)
        targets = list(range(B))

        def torch_gather():   # the expressions of compact(): the same bytes into fresh tensors
            got = [src.pages[pidx], src.P[idx], src.Cur[idx]]
            if src.page_mult is not None:
                got.append(src.page_mult[pidx])
            return got

        parts = torch_gather()
        didx = torch.arange(len(pidx), device=DEV)

        def torch_scatter():
            dst.pages[didx] = parts[0]
            dst.P[idx] = parts[1]
            dst.Cur[idx] = parts[2]
            if src.page_mult is not None:
                dst.page_mult[didx] = parts[3]

        def swap_in(b):
            dst.reset(targets)
            dst.swap_in(b, targets)

        dev_fns = {"swap_out": lambda: src.swap_out(slots, device=DEV, release=False), "swap_in": lambda: swap_in(blob), "torch_gather": torch_gather,
                   "torch_scatter": torch_scatter, "device_copy": lambda: flat.copy_(blob.buffer)}
        host_fns = {"swap_out_host": lambda: src.swap_out(slots, release=False), "swap_in_host": lambda: swap_in(host_blob),
                    "pinned_copy_d2h": lambda: pinned.copy_(flat, non_blocking=True), "pinned_copy_h2d": lambda: flat.copy_(pinned, non_blocking=True)}
        wall, devt, host = {n: [] for n in dev_fns}, {"swap_out": [], "swap_in": []}, {n: [] for n in host_fns}
        with torch.no_grad():
            for _ in range(reps):
                for n, fn in dev_fns.items():
                    wall[n].append(batch_us(fn, steps))
                for n in devt:
                    devt[n].append(sum(kernel_times(dev_fns[n], iters=20).values()))
                for n, fn in host_fns.items():
                    host[n].append(wall_sync_us(fn))
        gbs = lambda us: round(nbytes / statistics.median(us) / 1e3, 1)
        out[fmt] = {"blob_MB": round(nbytes / 2 ** 20, 2), "pages_moved": blob.n_pages, "wall_us": {n: spread(x) for n, x in wall.items()},
                    "device_us": {n: spread(x) for n, x in devt.items()}, "host_wall_us": {n: spread(x) for n, x in host.items()},
                    "GBps": {**{f"{n}_device": gbs(x) for n, x in devt.items()}, **{f"{n}_wall": gbs(x) for n, x in wall.items()},
                             **{n: gbs(x) for n, x in host.items()}}}
    # what the alternative costs at the least: the state half of a re-prefill of the same sequences (a real one runs the whole model)
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    plan = mhla_amd.causal_varlen_plan(cu, DEV)
    kc = torch.randn(1, cu[-1], H, K, generator=g).to(torch.bfloat16).to(DEV)
    vc = torch.randn(1, cu[-1], H, V, generator=g).to(torch.bfloat16).to(DEV)
    pre = {}
    with torch.no_grad():
        for fmt in ("fp32", "h16"):
            pool = make(fmt, filled=False)
            view = pool.at(slots)
            fill = lambda: mhla_amd.mhla_causal_state(kc, vc, mix, cu_seqlens=plan, into=view)
            fill()
            pre[fmt] = spread([sum(kernel_times(fill, iters=5).values()) for _ in range(reps)])
    rec = {"swap": {"B": B, "H": H, "K": K, "V": V, "n_slots": n_slots, "tokens": cu[-1]}, "steps_per_batch": steps, "reps": reps, **out,
           "reprefill_state_device_us": pre}
    print(json.dumps(rec), flush=True)
    return rec


def pool_layer_config(steps, reps, layers=24):
    import time
    from mhla_amd import modules, ops
    B, D, H, K, V, CAP, SLICE = 32, 1024, 4, 128, 256, 32, 256
    torch.manual_seed(1)
    g = torch.Generator().manual_seed(1)
    m = modules.MHLA(mode="chunk", hidden_size=D, num_heads=H, feature_map="relu", layer_idx=0, max_chunks=CAP, exact_decoding=True)
    m = m.to(DEV).to(torch.bfloat16).eval()
    lens = tuple(960 + (7 * b) % 63 for b in range(B - 1)) + (1000,)
    slots = torch.randperm(2 * B, generator=g)[:B].tolist()
    mixes = {"decode": (1,) * B, "mixed": (1,) * (B - 1) + (SLICE,)}
    cos, sin = m.rotary._tables(64 * CAP, DEV, torch.bfloat16)
    cos, sin = cos[:64 * CAP], sin[:64 * CAP]
    rec = {"pool_layer": {"B": B, "hidden": D, "H": H, "K": K, "V": V, "capacity_chunks": CAP, "lengths": lens, "slots": slots},
           "steps_per_batch": steps, "reps": reps}
    with torch.no_grad():
        for mix, counts in mixes.items():
            cu = [0]
            for n in counts:
                cu.append(cu[-1] + n)
            N, T = cu[-1], max(counts)
            # ---- the states: a pool behind a PagedDecodeCache, a ragged state behind a DecodeCache, both at `lens`
            cache = modules.PagedDecodeCache(2 * B, CAP, 2 * B * 21, DEV)
            cache.schedule(slots, list(range(B + 1)))
            m(torch.randn(1, B, D, generator=g).to(torch.bfloat16).to(DEV), past_key_values=cache, use_cache=True)   # (creates the pool)
            pool = cache.pool(0)
            pool.reserve(slots, [n + c for n, c in zip(lens, counts)])
            pool.pages.normal_(0, 0.1)
            pool.P.normal_(0, 0.1)
            pool_lens = [0] * (2 * B)
            for s_, n in zip(slots, lens):
                pool_lens[s_] = n
            pool_lens = tuple(pool_lens)
            pool_pos = torch.tensor(pool_lens, dtype=torch.int32, device=DEV)
            st = mhla_amd.CausalState.empty(B, H, K, V, CAP, DEV)
            st.S.normal_(0, 0.1)
            st.P.normal_(0, 0.1)
            st = mhla_amd.CausalState(st.S, st.P, st.Cur, lengths=lens)
            own = modules.DecodeCache()
            own.update(recurrent_state=st, layer_idx=0, offset=max(lens))
            st_pos = torch.tensor(lens, dtype=torch.int32, device=DEV)
            x_pack = torch.randn(1, N, D, generator=g).to(torch.bfloat16).to(DEV)
            x_pad = torch.randn(B, T, D, generator=g).to(torch.bfloat16).to(DEV)
            q = torch.randn(1, N, H, K, generator=g).to(torch.bfloat16).to(DEV)
            k = torch.randn(1, N, H, K, generator=g).to(torch.bfloat16).to(DEV)
            view = pool.at(slots)
            off = torch.tensor(cu, dtype=torch.int32, device=DEV)
            cu_dev, map64 = off.long(), view.map.long()

            def put_back():
                pool.lengths, pool.seen = pool_lens, max(pool_lens)
                pool.pos.copy_(pool_pos)
                st.lengths, st.seen = lens, max(lens)
                st.pos.copy_(st_pos)
                own._seen[0] = max(lens)

            def prologue_new():
                mhla_amd.featmap_rotary_decode(q, k, cos, sin, view, feature_map="relu", off_dev=off)

            def prologue_today():   # the layer's `_rotary_rows` + `_featmap_rotary` for a pack: positions with torch ops, gathered table rows
                tpos = torch.arange(N, device=DEV)
                seq = torch.searchsorted(cu_dev, tpos, right=True) - 1
                p = pool.pos.long()[map64][seq] + tpos - cu_dev[seq]
                c, s_ = cos.index_select(0, p), sin.index_select(0, p)
                mhla_amd.featmap_rotary(q, c, s_, "relu"), mhla_amd.featmap_rotary(k, c, s_, "relu")

            def layer_pool():
                put_back()
                cache.schedule(slots, cu)
                m(x_pack, past_key_values=cache, use_cache=True)

            def layer_padded():   # the existing DecodeCache call: padded [B, T, D], right-aligned windows
                put_back()
                m(x_pad, past_key_values=own, use_cache=True, token_counts=counts)

            fns = {"prologue_k_fr_decode": prologue_new, "prologue_today": prologue_today, "layer_pool_step": layer_pool,
                   "layer_padded_token_counts": layer_padded}
            wall, devt, kern = {n: [] for n in fns}, {n: [] for n in fns}, {}
            for _ in range(reps):
                for n, fn in fns.items():
                    wall[n].append(batch_us(fn, steps))
                for n, fn in fns.items():
                    kern[n] = kernel_times(fn, iters=20)
                    devt[n].append(sum(kern[n].values()))
            rec[mix] = {"tokens": N, "padded_rows": B * T, "wall_us": {n: spread(x) for n, x in wall.items()},
                        "library_device_us": {n: spread(x) for n, x in devt.items()},
                        "kernels_us": {n: {kn: round(us, 2) for kn, us in ks.items()} for n, ks in kern.items()}}
        # ---- the prologue's piece width: a pack large enough to be bound by memory (32 x 512 tokens, q and k rotated in place), its rows
        # on 16-byte boundaries (16-byte pieces) and 8 bytes off them (the 8-byte pieces of k_fmap_rotary); the bits are the same
        NB = 32 * 512
        big = torch.randn(1, NB, 2 * H * K + 8, generator=g).to(torch.bfloat16).to(DEV)
        first = mhla_amd.CausalState.empty(32, 1, 8, 8, 1, DEV).to_ragged()
        off_big = torch.arange(0, NB + 1, 512, dtype=torch.int32, device=DEV)
        width = {}
        for name, at in (("16_byte_pieces", 0), ("8_byte_pieces", 4)):
            qv, kv = big[..., at:at + H * K].view(1, NB, H, K), big[..., at + H * K:at + 2 * H * K].view(1, NB, H, K)
            fn = lambda qv=qv, kv=kv: mhla_amd.featmap_rotary_decode(qv, kv, cos, sin, first, feature_map="relu", off_dev=off_big, inplace=True)
            width[name] = {"wall_us": spread([batch_us(fn, steps) for _ in range(reps)]),
                           "device_us": spread([sum(kernel_times(fn, iters=20).values()) for _ in range(reps)])}
        rec["piece_width"] = {"tokens": NB, "bytes_moved_MB": round(2 * 2 * NB * 2 * H * K / 2 ** 20, 1), **width}
        # ---- the host's share of a model step: per layer the view, the capacity check and the page rule (no launch), `layers` pools
        cache = modules.PagedDecodeCache(2 * B, CAP, 2 * B * 21, DEV)
        dims = (1, 8, 8)   # (the host's work does not depend on the size of a page: small ones, 24 pools)
        cache.schedule(slots, list(range(B + 1)))
        for i in range(layers):
            cache._layer_step(i, B, dims)
            cache._step.ran.add(i)
        host = {}
        for place, at in (("steady", lens), ("every_request_opens_a_chunk", tuple(64 * (15 + b % 3) for b in range(B)))):
            full = [0] * (2 * B)
            for s_, n in zip(slots, at):
                full[s_] = n
            full = tuple(full)
            for i in range(layers):
                cache.pool(i).reserve(slots, list(at))
            times = []
            for _ in range(max(20, steps // 4)):
                for i in range(layers):   # (put back: lengths, and the pages the last round assigned)
                    pl = cache.pool(i)
                    pl.lengths, pl.seen = full, max(full)
                    pl.trim(slots)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                cache.schedule(slots, list(range(B + 1)))
                for i in range(layers):
                    step, view = cache._layer_step(i, B, dims)
                    ops._counts_fit("bench", m.mixing_matrix, view, step.counts)
                    view.pool.reserve(step.slots, [p + n for p, n in zip(view.lengths, step.counts)])
                    step.ran.add(i)
                times.append((time.perf_counter() - t0) * 1e6)
                torch.cuda.synchronize()
            host[place] = {"per_step_us": spread(times), "per_layer_us": round(statistics.median(times) / layers, 2)}
        rec["host_share"] = {"layers": layers, "sequences": B, **host}
    print(json.dumps(rec), flush=True)
    return rec


def launch_counts(fn):
    """{kernel: launches} of one call of `fn` (the library's per-launch hook)."""
    import ctypes
    lib = mhla_amd._lib.load()
    buf = ctypes.create_string_buffer(1 << 14)
    torch.cuda.synchronize()
    lib.mhla_prof_report(buf, len(buf))
    lib.mhla_prof_enable(1)
    fn()
    torch.cuda.synchronize()
    lib.mhla_prof_enable(0)
    lib.mhla_prof_report(buf, len(buf))
    return {ln.rsplit(" ", 2)[0]: int(ln.rsplit(" ", 2)[1]) for ln in buf.value.decode().splitlines() if ln.strip()}


def mixed_config(H, K, V, steps, reps, slice_tokens=256):
    B = 8
    g = torch.Generator().manual_seed(1)
    mix = causal_mixing_init(L).reshape(L, L).to(DEV)
    lengths = tuple((13 + b % 5) * 64 + 5 + (9 * b) % 50 for b in range(B - 1)) + (1000,)
    counts = (1,) * (B - 1) + (slice_tokens,)
    T = slice_tokens
    q, k = (torch.randn(B, T, H, K, generator=g).to(torch.bfloat16).to(DEV) for _ in range(2))
    v = torch.randn(B, T, H, V, generator=g).to(torch.bfloat16).to(DEV)
    st = mhla_amd.CausalState.empty(B, H, K, V, L, DEV)
    st.S[:, :, :24].normal_(0, 0.1)
    st.P.normal_(0, 0.1)
    rag = mhla_amd.CausalState(st.S, st.P, st.Cur, lengths=lengths)
    ones = [mhla_amd.CausalState(st.S[b:b + 1], st.P[b:b + 1], st.Cur[b:b + 1], lengths[b]) for b in range(B)]
    pos0 = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    spare = torch.empty_like(pos0)
    toks = [tuple(t[b:b + 1, T - n:] for t in (q, k, v)) for b, n in enumerate(counts)]   # right-aligned, as the ragged call reads them

    def ragged():
        rag.lengths, rag.seen = lengths, max(lengths)
        rag.pos.copy_(pos0)
        mhla_amd.mhla_causal_extend(q, k, v, mix, rag, counts=counts, left_padded=True)

    def per_sequence():
        spare.copy_(pos0)
        for b in range(B):
            ones[b].seen = lengths[b]
            mhla_amd.mhla_causal_extend(*toks[b], mix, ones[b])

    fns = {"ragged_chain": ragged, "per_sequence": per_sequence}
    wall = {n: [] for n in fns}
    dev = {n: [] for n in fns}
    kern = {}
    with torch.no_grad():
        for _ in range(reps):
            for n, fn in fns.items():
                wall[n].append(batch_us(fn, steps))
            for n, fn in fns.items():
                kern[n] = kernel_times(fn, iters=20)
                dev[n].append(sum(kern[n].values()))
            st.Cur.zero_()
        launches = {n: launch_counts(fn) for n, fn in fns.items()}
    med = {n: statistics.median(x) for n, x in wall.items()}
    rec = {"mixed": {"B": B, "H": H, "K": K, "V": V, "lengths": lengths, "counts": counts}, "steps_per_batch": steps, "reps": reps,
           "wall_us": {n: spread(x) for n, x in wall.items()}, "device_us": {n: spread(x) for n, x in dev.items()},
           "per_sequence_over_ragged_wall": round(med["per_sequence"] / med["ragged_chain"], 2),
           "per_sequence_over_ragged_device": round(statistics.median(dev["per_sequence"]) / statistics.median(dev["ragged_chain"]), 2),
           "launches": {n: {"total": sum(c.values()), "by_kernel": c} for n, c in launches.items()},
           "kernels_us": {n: {kn: round(us, 2) for kn, us in ks.items()} for n, ks in kern.items()},
           "ragged_wall_median_below_per_sequence_min": med["ragged_chain"] < min(wall["per_sequence"])}
    print(json.dumps(rec), flush=True)
    return rec


def packed_config(B, H, K, V, steps, reps, slice_tokens=256, existing_only=False):
    import inspect
    has_packed = "cu_seqlens" in inspect.signature(mhla_amd.mhla_causal_extend).parameters and not existing_only
    g = torch.Generator().manual_seed(1)
    mix = causal_mixing_init(L).reshape(L, L).to(DEV)
    lengths = tuple((13 + b % 5) * 64 + 5 + (9 * b) % 50 for b in range(B - 1)) + (1000,)
    counts = (1,) * (B - 1) + (slice_tokens,)
    T, N = slice_tokens, B - 1 + slice_tokens
    cu = [0]
    for n in counts:
        cu.append(cu[-1] + n)
    mk = lambda rows, D: torch.randn(1, rows, H, D, generator=g).to(torch.bfloat16).to(DEV)
    qp, kp, vp = mk(N, K), mk(N, K), mk(N, V)                        # the pack
    q, k, v = (torch.zeros(B, T, H, t.shape[-1], dtype=t.dtype, device=DEV) for t in (qp, kp, vp))   # the same tokens, right-padded
    rows = torch.cat([torch.arange(n) + b * T for b, n in enumerate(counts)]).to(DEV)   # row of the padded tensors of every pack row
    for t, tp in ((q, qp), (k, kp), (v, vp)):
        t.view(B * T, H, -1)[rows] = tp[0]
    q1, k1, v1 = (t[:, :1].contiguous() for t in (q, k, v))         # one token per sequence
    Te = 64                                                          # equal tokens: every sequence 64 from position 1000
    qe, ke, ve = (torch.randn(B, Te, H, D, generator=g).to(torch.bfloat16).to(DEV) for D in (K, K, V))
    qep, kep, vep = (t.reshape(1, B * Te, H, -1) for t in (qe, ke, ve))
    cue = [b * Te for b in range(B + 1)]
    st = mhla_amd.CausalState.empty(B, H, K, V, L, DEV)
    st.S[:, :, :24].normal_(0, 0.1)
    st.P.normal_(0, 0.1)
    rag = mhla_amd.CausalState(st.S, st.P, st.Cur, lengths=lengths)
    pos0 = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    pos_e = torch.full((B,), 1000, dtype=torch.int32, device=DEV)

    def put_back(ls=lengths, p=pos0):
        rag.lengths, rag.seen = tuple(ls), max(ls)
        rag.pos.copy_(p)

    def padded_extend():
        put_back()
        return mhla_amd.mhla_causal_extend(q, k, v, mix, rag, counts=counts)

    def padded_verify():
        put_back()
        return mhla_amd.mhla_causal_verify(q, k, v, mix, rag, counts=counts)[0]

    def ragged_step():
        put_back()
        return mhla_amd.mhla_causal_step(q1, k1, v1, mix, rag)

    def equal_padded():
        put_back((1000,) * B, pos_e)
        return mhla_amd.mhla_causal_extend(qe, ke, ve, mix, rag, counts=(Te,) * B)

    def packed_extend():
        put_back()
        return mhla_amd.mhla_causal_extend(qp, kp, vp, mix, rag, cu_seqlens=cu)

    def padded_from_pack():
        put_back()
        pad = []
        for tp in (qp, kp, vp):
            t = torch.zeros(B * T, H, tp.shape[-1], dtype=tp.dtype, device=DEV)
            t[rows] = tp[0]
            pad.append(t.view(B, T, H, -1))
        o = mhla_amd.mhla_causal_extend(*pad, mix, rag, counts=counts)
        return o.view(B * T, H, V)[rows].unsqueeze(0)

    def equal_packed():
        put_back((1000,) * B, pos_e)
        return mhla_amd.mhla_causal_extend(qep, kep, vep, mix, rag, cu_seqlens=cue)

    fns = {"padded_extend": padded_extend, "padded_verify": padded_verify, "ragged_step": ragged_step, "equal_padded": equal_padded}
    if has_packed:
        fns.update(packed_extend=packed_extend, padded_from_pack=padded_from_pack, equal_packed=equal_packed)
    wall = {n: [] for n in fns}
    dev = {n: [] for n in fns}
    kern = {}
    with torch.no_grad():
        for _ in range(reps):
            for n, fn in fns.items():
                wall[n].append(batch_us(fn, steps))
            for n, fn in fns.items():
                kern[n] = kernel_times(fn, iters=20)
                dev[n].append(sum(kern[n].values()))
            st.Cur.zero_()
        launches = {n: launch_counts(fn) for n, fn in fns.items()}
    lib = mhla_amd._lib.load()
    later = max((p + n - 1) // 64 - p // 64 for p, n in zip(lengths, counts))
    tok = lambda r: r * H * (2 * K + 2 * V) * 2   # q, k, v and the rows, bf16
    nbytes = {"padded": {"workspace": lib.mhla_causal_extend_ragged_ws_bytes(B, T, H, K, V, later, 1), "tokens": tok(B * T)}}
    if has_packed:
        nbytes["packed"] = {"workspace": lib.mhla_causal_extend_packed_ws_bytes(B, N, H, H, K, V, later, 1), "tokens": tok(N)}
    rec = {"packed": {"B": B, "H": H, "K": K, "V": V, "tokens": N, "padded_rows": B * T, "lengths": lengths, "counts": counts,
                      "equal_tokens": Te, "tree_has_cu_seqlens": has_packed},
           "steps_per_batch": steps, "reps": reps,
           "wall_us": {n: spread(x) for n, x in wall.items()}, "device_us": {n: spread(x) for n, x in dev.items()},
           "launches": {n: {"total": sum(c.values()), "by_kernel": c} for n, c in launches.items()},
           "kernels_us": {n: {kn: round(us, 2) for kn, us in ks.items()} for n, ks in kern.items()}, "bytes": nbytes}
    print(json.dumps(rec), flush=True)
    return rec


def speculative_config(B, H, K, V, steps, reps, pos=2048, k=4):
    g = torch.Generator().manual_seed(1)
    mix = causal_mixing_init(L).reshape(L, L).to(DEV)
    T = k + 1
    q, kk = (torch.randn(B, T, H, K, generator=g).to(torch.bfloat16).to(DEV) for _ in range(2))
    v = torch.randn(B, T, H, V, generator=g).to(torch.bfloat16).to(DEV)
    st = mhla_amd.CausalState.empty(B, H, K, V, L, DEV)
    st.S[:, :, :pos // 64].normal_(0, 0.1)
    st.P.normal_(0, 0.1)
    lengths = (pos,) * B
    rag = mhla_amd.CausalState(st.S, st.P, st.Cur, lengths=lengths)
    uni = mhla_amd.CausalState(st.S, st.P, st.Cur, pos)
    pos0 = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    spare = torch.empty_like(pos0)
    counts = (T,) * B

    def put_back():
        rag.lengths, rag.seen = lengths, pos
        rag.pos.copy_(pos0)

    def round_of(accept):
        def fn():
            put_back()
            _, draft = mhla_amd.mhla_causal_verify(q, kk, v, mix, rag, counts=counts)
            mhla_amd.mhla_causal_commit(draft, mix, rag, accept)
        return fn

    def clone_extend():
        put_back()
        mhla_amd.mhla_causal_extend(q, kk, v, mix, rag.clone(), counts=counts)

    def five_steps():
        spare.copy_(pos0)
        uni.seen = pos
        for t in range(T):
            mhla_amd.mhla_causal_step(q[:, t:t + 1], kk[:, t:t + 1], v[:, t:t + 1], mix, uni)

    fns = {"verify_commit_all": round_of((T,) * B), "verify_commit_2_of_5": round_of((2,) * B), "clone_extend": clone_extend,
           "five_steps": five_steps}
    wall = {n: [] for n in fns}
    dev = {n: [] for n in fns}
    kern = {}
    with torch.no_grad():
        for _ in range(reps):
            for n, fn in fns.items():
                wall[n].append(batch_us(fn, steps))
            for n, fn in fns.items():
                kern[n] = kernel_times(fn, iters=20)
                dev[n].append(sum(kern[n].values()))
            st.Cur.zero_()
        launches = {n: launch_counts(fn) for n, fn in fns.items()}
    med = {n: statistics.median(x) for n, x in wall.items()}
    rec = {"speculative": {"B": B, "H": H, "K": K, "V": V, "pos": pos, "draft_len": k, "verify_tokens": T}, "steps_per_batch": steps, "reps": reps,
           "wall_us": {n: spread(x) for n, x in wall.items()}, "device_us": {n: spread(x) for n, x in dev.items()},
           "launches": {n: {"total": sum(c.values()), "by_kernel": c} for n, c in launches.items()},
           "five_steps_over_round_wall": round(med["five_steps"] / med["verify_commit_all"], 2),
           "clone_extend_over_round_wall": round(med["clone_extend"] / med["verify_commit_all"], 2),
           "state_MB": round(rag.nbytes / 2 ** 20, 1),
           "kernels_us": {n: {kn: round(us, 2) for kn, us in ks.items()} for n, ks in kern.items()}}
    print(json.dumps(rec), flush=True)
    return rec


def packed_prefill_config(H, K, V, iters, reps, cap=40):
    lengths = (100, 333, 517, 777, 1024, 1300, 1701, 2048)
    B, T = len(lengths), max(lengths)
    g = torch.Generator().manual_seed(1)
    mix = causal_mixing_init(L).reshape(L, L).to(DEV)
    mk = lambda n, D: torch.randn(1, n, H, D, generator=g).to(torch.bfloat16)
    seqs = [(mk(n, K), mk(n, K), mk(n, V)) for n in lengths]
    pad = [torch.zeros(B, T, H, D, dtype=torch.bfloat16) for D in (K, K, V)]
    for b, n in enumerate(lengths):
        for dst, src in zip(pad, seqs[b]):
            dst[b, T - n:] = src[0]
    qp, kp, vp = (t.to(DEV) for t in pad)
    qc, kc, vc = (torch.cat([s[i] for s in seqs], dim=1).to(DEV) for i in range(3))
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    plan = mhla_amd.causal_varlen_plan(cu, DEV)
    fns = {"padded_prefill": lambda: mhla_amd.mhla_causal_prefill(qp, kp, vp, mix, lengths=lengths, left_padded=True, capacity_chunks=cap),
           "packed_prefill": lambda: mhla_amd.mhla_causal_prefill(qc, kc, vc, mix, cu_seqlens=plan, capacity_chunks=cap),
           "padded_state": lambda: mhla_amd.mhla_causal_state(kp, vp, mix, lengths=lengths, left_padded=True, capacity_chunks=cap),
           "packed_state": lambda: mhla_amd.mhla_causal_state(kc, vc, mix, cu_seqlens=plan, capacity_chunks=cap)}
    wall = {n: [] for n in fns}
    dev = {n: [] for n in fns}
    kern = {}
    with torch.no_grad():
        for _ in range(reps):
            for n, fn in fns.items():
                wall[n].append(batch_us(fn, iters, warm=2))
            for n, fn in fns.items():
                kern[n] = kernel_times(fn, iters=5)
                dev[n].append(sum(kern[n].values()))
        launches = {n: launch_counts(fn) for n, fn in fns.items()}
    med = {n: statistics.median(x) for n, x in wall.items()}
    rec = {"packed_prefill": {"H": H, "K": K, "V": V, "lengths": lengths, "tokens": cu[-1], "padded_rows": B * T, "capacity_chunks": cap,
                              "pack_chunks": plan.n_chunks},
           "calls_per_batch": iters, "reps": reps,
           "wall_us": {n: spread(x) for n, x in wall.items()}, "device_us": {n: spread(x) for n, x in dev.items()},
           "launches": {n: {"total": sum(c.values()), "by_kernel": c} for n, c in launches.items()},
           "padded_over_packed_wall": {h: round(med["padded_" + h] / med["packed_" + h], 2) for h in ("prefill", "state")},
           "padded_over_packed_device": {h: round(statistics.median(dev["padded_" + h]) / statistics.median(dev["packed_" + h]), 2)
                                         for h in ("prefill", "state")},
           "kernels_us": {n: {kn: round(us, 2) for kn, us in ks.items()} for n, ks in kern.items()}}
    print(json.dumps(rec), flush=True)
    return rec


def gqa_prefill_config(H, Hkv, K, V, T, fused, iters, reps):
    from mhla_amd import ops
    G = H // Hkv
    g = torch.Generator().manual_seed(1)
    mk = lambda h, D: torch.randn(1, T, h, D, generator=g).to(torch.bfloat16).to(DEV)
    q, k, v, gate = mk(H, K), mk(Hkv, K), mk(Hkv, V), mk(H, V)
    w = torch.ones(V, device=DEV)
    mix = causal_mixing_init(L).reshape(L, L).to(DEV)
    op = (lambda kk, vv: mhla_amd.mhla_causal_normgate(q, kk, vv, mix, gate, w)) if fused else (lambda kk, vv: mhla_amd.mhla_causal(q, kk, vv, mix))
    fns = {"grouped": lambda: op(k, v), "repeated": lambda: op(k.repeat_interleave(G, 2), v.repeat_interleave(G, 2))}
    dev = {n: [] for n in fns}
    kern, peak = {}, {}
    with torch.no_grad():
        for fn in fns.values():   # warm-up of both paths before either is timed
            batch_us(fn, 3, warm=3)
        for _ in range(reps):
            for n, fn in fns.items():
                dev[n].append(batch_us(fn, iters, warm=2))
        for n, fn in fns.items():
            kern[n] = kernel_times(fn, iters=5)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peak[n] = torch.cuda.max_memory_allocated() - base
    dt = ops._dtype_code(q)
    ws = {"grouped": ops._cs_plan(1, T, Hkv, K, V, 64, dt, 0)[0], "repeated": ops._cs_plan(1, T, H, K, V, 64, dt, 0)[0]}
    med = {n: statistics.median(x) for n, x in dev.items()}
    rec = {"gqa_prefill": {"B": 1, "T": T, "H": H, "Hkv": Hkv, "K": K, "V": V, "fused_epilogue": fused, "summaries": "tf32"},
           "calls_per_batch": iters, "reps": reps, "event_us": {n: spread(x) for n, x in dev.items()},
           "repeated_over_grouped": round(med["repeated"] / med["grouped"], 3),
           "workspace_bytes": ws, "workspace_ratio": round(ws["repeated"] / ws["grouped"], 3), "peak_bytes_over_inputs": peak,
           "kernels_us": {n: {kn: round(us, 2) for kn, us in ks.items()} for n, ks in kern.items()}}
    print(json.dumps(rec), flush=True)
    return rec


def gpu_kernel_count(fn):
    """GPU kernels one call of `fn` launches, or None where the profiler reports no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower())
        return n or None
    except Exception:   # noqa: BLE001
        return None


def gpt_graph(steps, reps, B=8, T0=100):
    from mhla_amd.hosts.gpt import GPT_MHLA, GPT_configs
    from mhla_amd.modules import DecodeCache
    torch.manual_seed(0)
    model = GPT_MHLA(**GPT_configs()["340M"], exact_decoding=True).to(DEV).to(torch.bfloat16).eval()
    prompt = torch.randint(0, 32000, (B, T0), device=DEV)
    steps = min(steps, (2048 - T0 - 8) // (reps + 1))   # every cache stays inside the matrix (2048 tokens) over all repetitions
    ids = torch.randint(0, 32000, (B, 1), device=DEV)
    with torch.no_grad():
        caches = {n: DecodeCache(device_positions=n != "eager") for n in ("eager", "dev", "replay")}
        for c in caches.values():
            model(prompt, cache=c)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(ids, cache=caches["replay"])
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            model(ids, cache=caches["replay"])
        fns = {"eager": lambda: model(ids, cache=caches["eager"]), "dev": lambda: model(ids, cache=caches["dev"]), "replay": graph.replay}
        wall = {n: [] for n in fns}
        for _ in range(reps):
            for n, fn in fns.items():
                wall[n].append(batch_us(fn, steps, warm=2))
        layer, x = model.layers[0].attn, torch.randn(B, 1, 1024, device=DEV, dtype=torch.bfloat16)
        counts = {n: gpu_kernel_count(lambda n=n: layer(x, past_key_values=caches[n], use_cache=True)) for n in ("eager", "dev")}
        for n in ("dev", "replay"):
            caches[n].sync()
    rec = {"gpt_340M_decode_step": {"B": B, "prompt": T0, "layers": 24, "dtype": "bf16"}, "steps_per_batch": steps, "reps": reps,
           "wall_us": {n: spread(x) for n, x in wall.items()}, "layer_step_gpu_kernels": counts,
           "tokens_seen": {n: c.get_seq_length(0) for n, c in caches.items()}}
    print(json.dumps(rec), flush=True)
    return rec


def extend_config(B, H, K, V, pos, T, reps, parent_iters):
    g = torch.Generator().manual_seed(1)
    Lx = L + 16                                   # pos 8000 + 1024 tokens: 141 chunks
    mix = causal_mixing_init(Lx).reshape(Lx, Lx).to(DEV)
    i = pos // 64
    state = mhla_amd.CausalState.empty(B, H, K, V, Lx, DEV)
    state.S[:, :, :i].normal_(0, 0.1)
    state.P.normal_(0, 0.1)
    n = pos + T
    qT, kT = (torch.randn(B, n, H, K, generator=g).to(torch.bfloat16).to(DEV) for _ in range(2))
    vT = torch.randn(B, n, H, V, generator=g).to(torch.bfloat16).to(DEV)
    qe, ke, ve = qT[:, pos:], kT[:, pos:], vT[:, pos:]

    def reset():
        state.seen = pos
        state.Cur.zero_()

    def extend():
        reset()
        mhla_amd.mhla_causal_extend(qe, ke, ve, mix, state)

    def steps():
        reset()
        for t in range(T):
            mhla_amd.mhla_causal_step(qe[:, t:t + 1], ke[:, t:t + 1], ve[:, t:t + 1], mix, state)

    def parent():
        mhla_amd.mhla_causal(qT, kT, vT, mix)

    t_ext, t_step, t_parent = [], [], []
    with torch.no_grad():
        for _ in range(reps):
            t_ext.append(batch_us(extend, 20, warm=3))
            t_step.append(batch_us(steps, max(1, 256 // T), warm=1))
            t_parent.append(batch_us(parent, parent_iters, warm=2))
        ks = {nm: round(us, 2) for nm, us in kernel_times(extend, iters=10).items()}
    ext, stp, par = (statistics.median(x) for x in (t_ext, t_step, t_parent))
    touched = (pos + T - 1) // 64 - i
    rec = {"extend": {"B": B, "H": H, "K": K, "V": V, "pos": pos, "T": T}, "reps": reps,
           "extend_us": spread(t_ext), "steps_us": spread(t_step), "parent_fwd_us": spread(t_parent),
           "extend_us_per_token": round(ext / T, 3), "steps_us_per_token": round(stp / T, 3), "parent_us_per_token": round(par / T, 3),
           "steps_over_extend": round(stp / ext, 2), "parent_over_extend": round(par / ext, 2),
           "extend_kernels_us": ks, "extend_device_us": round(sum(ks.values()), 2),
           # P, Cur read, Cur / S written, the prefix tiles written and read back, S[0 .. ] read once per eight new chunks, token rows
           "extend_bytes": B * H * (K * V * 4 * (3 + 3 * touched + (i + touched) * ((touched + 7) // 8)) + T * (2 * K + 2 * V) * 2)}
    print(json.dumps(rec), flush=True)
    return rec


def extend_workload():
    B, H, K, V, T0, n = 1, 4, 128, 256, 8000, 1024
    g = torch.Generator().manual_seed(1)
    mix = causal_mixing_init(L + 16).reshape(L + 16, L + 16).to(DEV)
    q, k = (torch.randn(B, T0 + n, H, K, generator=g).to(torch.bfloat16).to(DEV) for _ in range(2))
    v = torch.randn(B, T0 + n, H, V, generator=g).to(torch.bfloat16).to(DEV)
    with torch.no_grad():
        _, state = mhla_amd.mhla_causal_prefill(q[:, :T0], k[:, :T0], v[:, :T0], mix)
        for _ in range(10):
            state.seen = T0
            state.Cur.zero_()
            mhla_amd.mhla_causal_extend(q[:, T0:], k[:, T0:], v[:, T0:], mix, state)
    torch.cuda.synchronize()
    print(json.dumps({"workload": "prefill + 10 x extend", "B": B, "H": H, "K": K, "V": V, "prefill": T0, "extend": n, "seen": state.seen}))


def workload():
    B, H, K, V, T0, n = 1, 4, 128, 256, 8000, 192
    g = torch.Generator().manual_seed(1)
    mix = causal_mixing_init(L).reshape(L, L).to(DEV)
    q, k = (torch.randn(B, T0 + n, H, K, generator=g).to(torch.bfloat16).to(DEV) for _ in range(2))
    v = torch.randn(B, T0 + n, H, V, generator=g).to(torch.bfloat16).to(DEV)
    with torch.no_grad():
        _, state = mhla_amd.mhla_causal_prefill(q[:, :T0], k[:, :T0], v[:, :T0], mix)
        for t in range(T0, T0 + n):
            mhla_amd.mhla_causal_step(q[:, t:t + 1], k[:, t:t + 1], v[:, t:t + 1], mix, state)
    torch.cuda.synchronize()
    print(json.dumps({"workload": "prefill + steps", "B": B, "H": H, "K": K, "V": V, "prefill": T0, "steps": n, "seen": state.seen}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-iters", type=int, default=5)
    ap.add_argument("--workload", action="store_true")
    ap.add_argument("--extend", action="store_true")
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--mixed", action="store_true")
    ap.add_argument("--packed-prefill", action="store_true")
    ap.add_argument("--speculative", action="store_true")
    ap.add_argument("--gqa", action="store_true")
    ap.add_argument("--gqa-prefill", action="store_true")
    ap.add_argument("--slots", action="store_true")
    ap.add_argument("--paged", action="store_true")
    ap.add_argument("--paged-h16", action="store_true")
    ap.add_argument("--packed", action="store_true")
    ap.add_argument("--existing-only", action="store_true")
    ap.add_argument("--swap", action="store_true")
    ap.add_argument("--pool-layer", action="store_true")
    a = ap.parse_args()
    if a.pool_layer:
        pool_layer_config(max(100, a.steps), a.reps)
    elif a.swap:
        for B in (4, 32):
            swap_config(B, 4, 128, 256, min(100, a.steps), a.reps)
    elif a.packed:
        for B in (8, 32):
            packed_config(B, 4, 128, 256, max(100, a.steps), a.reps, existing_only=a.existing_only)
    elif a.paged_h16:
        for B in (4, 32):
            paged_config(B, 4, 128, 256, max(200, a.steps), a.reps, h16=True)
    elif a.paged:
        for B in (8, 32):
            paged_config(B, 4, 128, 256, max(200, a.steps), a.reps)
    elif a.slots:
        for B in (8, 32):
            slots_config(B, 4, 128, 256, max(200, a.steps), a.reps)
    elif a.gqa_prefill:
        for fused in (False, True):
            for Hkv in (8, 4, 2):
                gqa_prefill_config(16, Hkv, 128, 256, 8192, fused, min(20, a.steps), a.reps)
    elif a.gqa:
        for Hkv in (4, 2):
            gqa_config(8, 16, Hkv, 128, 256, max(200, a.steps), a.reps)
    elif a.speculative:
        for B in (1, 8):
            speculative_config(B, 4, 128, 256, max(100, a.steps), a.reps)
    elif a.packed_prefill:
        packed_prefill_config(4, 128, 256, min(20, a.steps), a.reps)
    elif a.mixed:
        mixed_config(4, 128, 256, max(100, a.steps), a.reps)
    elif a.graph:
        for B in (8, 32):
            graph_config(B, 4, 128, 256, max(200, a.steps), a.reps)
        gpt_graph(a.steps, a.reps)
    elif a.ragged:
        for B in (8, 32):
            ragged_config(B, 4, 128, 256, max(200, a.steps), a.reps)
    elif a.extend and a.workload:
        extend_workload()
    elif a.extend:
        for H, K, V in ((4, 128, 256), (4, 256, 512)):
            for B in (1, 32):
                for pos in (100, 8000):
                    for T in (16, 64, 256, 1024):
                        extend_config(B, H, K, V, pos, T, a.reps, a.parent_iters)
    elif a.workload:
        workload()
    else:
        for H, K, V in ((4, 128, 256), (4, 256, 512)):
            for B in (1, 32):
                for pos in (100, 8000):
                    config(B, H, K, V, pos, max(200, a.steps), a.reps, a.parent_iters)
        roll_sweep(1, 4, 128, 256, max(200, a.steps))
        roll_sweep(32, 4, 128, 256, max(200, a.steps))
