"""Shared by the state-pool tests (test_gpu_state_slots.py, test_gpu_state_paged.py, test_gpu_state_paged_h16.py, test_gpu_state_swap.py,
test_gpu_extend_packed.py, test_state_paged_h16_cpu.py, test_state_swap_cpu.py): the cases and the one generator of their inputs, the
pool builders (a NaN-poisoned dense, paged or h16 pool filled from a compact state by plain tensor operations: no setup depends on
what is tested), the h16 reference (codec, fp64 rows), the pool of the host-layer tests, and ONE snapshot and ONE isolation check for
every kind of pool: each byte a call does not name is compared as bits against what it held, poison included.  A sibling of
decode_util.py with the same rule: nothing here is used by one file alone.  `mhla_amd` is imported only inside the helpers that call
it; every helper takes its device from its arguments (`tokens`: `device=`), so all of it runs on CPU tensors --
tests/test_pool_util_cpu.py holds the checkers themselves to what they must catch and must let pass."""
import functools
from collections import namedtuple

import torch

from gpu_util import DEV
from decode_util import signed_features

N_SLOTS, CAP, L = 5, 4, 4
VIEW = [3, 0, 4]                  # call row -> slot: not monotonic
LENGTHS = (63, 5, 130)            # on a chunk boundary, inside chunk 0, in chunk 2
COUNTS, ACCEPT, T = (1, 70, 0), (1, 33, 0), 70
POISON = 0x7FC00000               # pos of a slot nobody prefilled: a NaN's bits, outside every capacity
NAN = float("nan")
N_PAGES = 10
# slot -> pages of its chunks 0, 1, ...: descending within a slot, interleaved across slots; pages 0, 1, 3, 8, 9 start free
TABLE = {4: [7, 5, 2], 3: [6], 0: [4]}

# (dtype, H, Hkv, K, V); the last shape has h16 groups that straddle rows (V = 72)
CASES = [(torch.float32, 2, 2, 64, 64), (torch.bfloat16, 2, 2, 64, 64), (torch.float32, 4, 2, 64, 64), (torch.bfloat16, 4, 2, 64, 64),
         (torch.float32, 2, 2, 40, 72)]
IDS = ["fp32", "bf16", "fp32-G2", "bf16-G2", "fp32-K40V72"]


def bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()]) if t.is_floating_point() else t


def same_bits(name, a, b):
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), f"{name}: bits differ"


def windows(x, counts, left):
    """x [B, T, ...] with NaN outside every row's window of counts[b] tokens."""
    out = torch.full_like(x, NAN)
    for b, n in enumerate(counts):
        t0 = x.shape[1] - n if left else 0
        out[b, t0:t0 + n] = x[b, t0:t0 + n]
    return out


@functools.lru_cache(maxsize=None)
def tokens(dtype, H, Hkv, K, V, B=3, device=DEV):
    """One set per shape and device, shared by the cases and never written, drawn on the CPU: hk, hv (the pack that fills the pool), q, k,
    v, gate of T padded tokens per call row (NaN outside the windows of COUNTS is put in by the cases that have windows), norm weight, mix."""
    g = torch.Generator().manual_seed(4321)
    n = sum(LENGTHS)
    hk, hv = signed_features(g, 1, n, Hkv, K).to(dtype), torch.randn(1, n, Hkv, V, generator=g).to(dtype)
    q, k = signed_features(g, B, T, H, K).to(dtype), signed_features(g, B, T, Hkv, K).to(dtype)
    v, gate = torch.randn(B, T, Hkv, V, generator=g).to(dtype), torch.randn(B, T, H, V, generator=g).to(dtype)
    w = torch.rand(V, generator=g) + 0.5
    mix = torch.tril(torch.rand(L, L, generator=g).clamp(1e-5, 1))
    return tuple(t.to(device) for t in (hk, hv, q, k, v, gate, w, mix))


# -------------------------------------------------------------------------------------------------
# the h16 reference: the codec, and the fp64 rows of every request of `tokens` alone
# -------------------------------------------------------------------------------------------------
GROUP = 64
ROW_EXTRA = 1e-3   # the row bound beyond the final rounding of a row: CAUSAL_TOL[dtype] - u for 16-bit tensors, the whole bound for fp32


def encode(x):
    """x [..., K, V] fp32 -> (payload [..., K, V] fp16, multipliers [..., K V / 64] fp32): group g of a chunk is elements
    [64 g, 64 g + 64) of the flattened [K, V]; its multiplier is 2^(e - 14) for the exponent field e of the group's largest magnitude
    (compared as bit patterns; the field of the multiplier clamped to 1 .. 240), its payload half(x * 2^-(e - 14))."""
    assert x.dtype == torch.float32 and (x.shape[-1] * x.shape[-2]) % GROUP == 0
    g = x.contiguous().reshape(*x.shape[:-2], -1, GROUP)
    mx = (g.view(torch.int32) & 0x7FFFFFFF).amax(-1)
    e = (mx >> 23) & 0xFF
    f = torch.where(e < 15, torch.ones_like(e), torch.where(e > 254, torch.full_like(e, 240), e - 14))
    mult = (f << 23).view(torch.float32)
    inv = (0x7F000000 - (f << 23)).view(torch.float32)   # 1 / mult, exact
    return (g * inv[..., None]).half().reshape(x.shape), mult


def decode(pay, mult):
    """payload x multiplier, exact in fp32."""
    return (pay.float().reshape(*mult.shape, GROUP) * mult[..., None]).reshape(pay.shape)


def sequence(case, b):
    """Request b of `tokens` alone, on the CPU in fp64: (q, k, v [1, m + T, H, .] with k, v repeated to the query heads and zeros as
    the queries of the m prefilled tokens, gate [1, T, H, V], w, mix, m)."""
    dtype, H, Hkv, K, V = case
    hk, hv, q, k, v, gate, w, mix = tokens(*case, device="cpu")
    t0, m = sum(LENGTHS[:b]), LENGTHS[b]
    rep = lambda t: t.double().repeat_interleave(H // Hkv, dim=2)
    kk = torch.cat([rep(hk[:, t0:t0 + m]), rep(k[b:b + 1])], dim=1)
    vv = torch.cat([rep(hv[:, t0:t0 + m]), rep(v[b:b + 1])], dim=1)
    qq = torch.cat([torch.zeros(1, m, H, K, dtype=torch.float64), q[b:b + 1].double()], dim=1)
    return qq, kk, vv, gate[b:b + 1].double(), w.double(), mix.double(), m


def rows_fp64(q, k, v, mix, store=None):
    """The causal operator in fp64, [1, T, H, V]; `store`: what a finished chunk's K^T V [1, H, K, V] becomes before anything reads it."""
    T, K = q.shape[1], q.shape[-1]
    qh, kh, vh = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    S, out = [], []
    for i in range(-(-T // 64)):
        r = slice(64 * i, min(T, 64 * i + 64))
        Q, Kc, Vc = qh[:, :, r], kh[:, :, r], vh[:, :, r]
        P = sum((mix[i, j] * S[j] for j in range(i)), torch.zeros_like(Kc.transpose(-1, -2) @ Vc))
        out.append(K ** -0.5 * (Q @ P + mix[i, i] * (torch.tril(Q @ Kc.transpose(-1, -2)) @ Vc)))
        Sj = Kc.transpose(-1, -2) @ Vc
        S.append(Sj if store is None else store(Sj))
    return torch.cat(out, dim=2).permute(0, 2, 1, 3)


def gate_norm(o, gate, w, eps=1e-5):
    return o * torch.rsqrt(o.square().mean(-1, keepdim=True) + eps) * w * gate * torch.sigmoid(gate)


# -------------------------------------------------------------------------------------------------
# pool builders
# -------------------------------------------------------------------------------------------------
def fill_pool(kind, src, slots, *, n_slots, table=None, n_pages=None):
    """A pool of `n_slots` slots -- kind "dense" (`CausalState`), "paged" (`PagedCausalState`, fp32 pages) or "h16" (the same, the pages
    through the reference codec) -- whose every byte of state is poison but for `slots`, which hold copies of the rows of the compact
    ragged `CausalState` `src`, in order: P, Cur, pos and the finished chunks, in the dense S or in the pages `table` (slot -> pages of
    its chunks 0, 1, ...; of `n_pages`) names.  pos of every other slot is POISON; `full` is created (zeros: a flag is a finding)."""
    from mhla_amd import CausalState, PagedCausalState
    _, Hkv, cap, K, V = src.S.shape
    nan = lambda *s: torch.full(s, NAN, dtype=torch.float32, device=src.S.device)
    P, Cur, host = nan(n_slots, Hkv, K, V), nan(n_slots, Hkv, K, V), [0] * n_slots
    for b, s in enumerate(slots):
        P[s], Cur[s], host[s] = src.P[b], src.Cur[b], src.lengths[b]
    if kind == "dense":
        S = nan(n_slots, Hkv, cap, K, V)
        for b, s in enumerate(slots):
            S[s, :, :host[s] // 64] = src.S[b, :, :host[s] // 64]
        pool = CausalState(S, P, Cur, 0, 64, lengths=host)
    else:
        pages, rows = nan(n_pages, Hkv, K, V), [[-1] * cap for _ in range(n_slots)]
        for b, s in enumerate(slots):
            rows[s][:len(table[s])] = table[s]
            for j in range(host[s] // 64):
                pages[rows[s][j]] = src.S[b, :, j]
        kw = {}
        if kind == "h16":   # (the encoding of the fp32 pages; NaN too in the multipliers of every page no slot names)
            pages, mult = encode(pages)
            for p in set(range(n_pages)) - {p for s in slots for p in table[s]}:
                mult[p] = NAN
            kw = dict(page_mult=mult)
        pool = PagedCausalState(pages, P, Cur, rows, lengths=host, **kw)
        assert pool.table_dev.tolist() == rows and pool.pages_used == sum(len(table[s]) for s in slots)
        assert pool.page_format == ("h16" if kind == "h16" else "fp32")
    pool.pos.fill_(POISON)
    for s in slots:
        pool.pos[s] = host[s]
    pool.full
    return pool


def make_pool(kind, shape, slots=VIEW, lengths=LENGTHS, table=TABLE):
    """The family's pool of N_SLOTS slots (and N_PAGES pages through the scrambled TABLE: an identity mapping would hide a wrong index):
    poison but for `slots`, which hold what the existing un-slotted, un-paged pack prefill gives for `lengths`."""
    import mhla_amd
    hk, hv, *_, mix = tokens(*shape)
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    src = mhla_amd.mhla_causal_state(hk[:, :cu[-1]], hv[:, :cu[-1]], mix, cu_seqlens=cu, capacity_chunks=CAP)
    return fill_pool(kind, src, slots, n_slots=N_SLOTS, table=table, n_pages=N_PAGES)


# the pool of the host-layer tests (no GPU, no poison): LENGTHS at VIEW through TABLE, H = 2 heads of K x V = 8 x 16, NINE pages
HOST_DIMS = (2, 8, 16, 9)
HOST_LENGTHS = tuple(dict(zip(VIEW, LENGTHS)).get(s, 0) for s in range(N_SLOTS))
HOST_ROWS = [(TABLE.get(s, []) + [-1] * CAP)[:CAP] for s in range(N_SLOTS)]


def host_pool(fmt="h16"):
    from mhla_amd import PagedCausalState
    H, K, V, n_pages = HOST_DIMS
    z = lambda *s: torch.zeros(s)
    pages, kw = z(n_pages, H, K, V), {}
    if fmt == "h16":
        pages, kw = pages.half(), dict(page_mult=z(n_pages, H, K * V // GROUP))
    return PagedCausalState(pages, z(N_SLOTS, H, K, V), z(N_SLOTS, H, K, V), [list(r) for r in HOST_ROWS], lengths=HOST_LENGTHS, **kw)


def host_state(pool):
    return [list(r) for r in pool.table], list(pool.refs), sorted(pool.free), pool.lengths, pool.pos.tolist(), pool.table_dev.tolist()


# -------------------------------------------------------------------------------------------------
# the snapshot and the checks
# -------------------------------------------------------------------------------------------------
Snapshot = namedtuple("Snapshot", "chunks page_mult P Cur pos full table_dev table lengths")


def snapshot(pool):
    """Clones of every device tensor of a pool of any kind (`chunks`: S, or the pages), copies of its host table and lengths; None for
    what the kind does not have."""
    paged = pool.pages is not None
    c = lambda t: None if t is None else t.clone()
    return Snapshot(c(pool.pages if paged else pool.S), c(pool.page_mult), pool.P.clone(), pool.Cur.clone(), pool.pos.clone(), pool.full.clone(),
                    c(pool.table_dev) if paged else None, [list(r) for r in pool.table] if paged else None, tuple(pool.lengths))


def _settle(pool):
    if pool.P.is_cuda:
        torch.cuda.synchronize()


def check_untouched(name, pool, before, touched, reach=None, pages=None, flagged=()):
    """Nothing the call does not name changed a bit since the snapshot `before`.  Every slot outside `touched` keeps every bit of P, Cur,
    pos and full (`flagged`: slots whose `full` flag the call may set), its host length, its dense S or its table row; the device
    table is the host's; a page keeps every bit of payload and multipliers unless it is WRITABLE: one of `pages`, or else a chunk of a
    touched slot from the one open `before` to the last one its `reach` tokens touch (`reach`: tokens per slot of `touched`) -- every
    such chunk must have a page.  With neither, no page is writable."""
    _settle(pool)
    for s in range(pool.dims[0]):
        if s in touched:
            continue
        rest = f"of slot {s}, which the call does not name or leaves alone"
        for part in ("P", "Cur", "pos", "full"):
            if part != "full" or s not in flagged:
                same_bits(f"{name}: {part} {rest}", getattr(pool, part)[s], getattr(before, part)[s])
        assert pool.lengths[s] == before.lengths[s], f"{name}: the host lengths entry {rest}: {pool.lengths[s]}, was {before.lengths[s]}"
        if before.table is None:
            same_bits(f"{name}: S {rest}", pool.S[s], before.chunks[s])
        else:
            assert pool.table[s] == before.table[s], f"{name}: the table row {rest}"
    if before.table is None:
        return
    off = [s for s, (dev, host) in enumerate(zip(pool.table_dev.tolist(), pool.table)) if dev != host]
    assert not off, f"{name}: table_dev is not the host table at the rows of slots {off}"
    n_pages = pool.pages.shape[0]
    writable = set(pages or ())
    if pages is None and reach is not None:
        for s, n in zip(touched, reach):
            for j in range(before.lengths[s] // 64, -(-n // 64)):
                assert 0 <= pool.table[s][j] < n_pages, f"{name}: chunk {j} of slot {s}, which the call reaches, has no page"
                writable.add(pool.table[s][j])
    for p in set(range(n_pages)) - writable:
        same_bits(f"{name}: payload of page {p}, which the call must not write", pool.pages[p], before.chunks[p])
        if pool.page_mult is not None:
            same_bits(f"{name}: multipliers of page {p}, which the call must not write", pool.page_mult[p], before.page_mult[p])


def check_pool(name, pool, before, ref, slots, lengths_after, touched=None, flagged=(), reach=None):
    """Slots `slots` of the pool hold the bits of the compact state `ref` -- the finished chunks (of S, or through the page table, h16
    pages decoded), P, Cur, and pos == ref.pos == lengths_after --; every other slot, and of `slots` those not in `touched`, hold every
    bit they held `before`, and so does every page a touched slot may not write (`check_untouched`; `reach`: tokens per slot of
    `slots`, default `lengths_after`)."""
    _settle(pool)
    touched = [s for s in slots if touched is None or s in touched]
    reach = lengths_after if reach is None else reach
    for b, s in enumerate(slots):
        n = lengths_after[b]
        if s not in touched:
            continue
        if pool.pages is None:
            same_bits(f"{name}: S of slot {s}", pool.S[s, :, :n // 64], ref.S[b, :, :n // 64])
        for j in range(n // 64) if pool.pages is not None else ():
            p = pool.table[s][j]
            assert 0 <= p < pool.pages.shape[0], f"{name}: finished chunk {j} of slot {s} has no page"
            chunk = pool.pages[p] if pool.page_mult is None else decode(pool.pages[p], pool.page_mult[p])
            same_bits(f"{name}: chunk {j} of slot {s} (page {p})", chunk, ref.S[b, :, j])
        same_bits(f"{name}: P of slot {s}", pool.P[s], ref.P[b])
        same_bits(f"{name}: Cur of slot {s}", pool.Cur[s], ref.Cur[b])
        assert int(pool.pos[s]) == int(ref.pos[b]) == n, f"{name}: pos of slot {s} is {int(pool.pos[s])}, the compact state's {int(ref.pos[b])}, expected {n}"
    check_untouched(name, pool, before, touched, [reach[list(slots).index(s)] for s in touched], flagged=flagged)
