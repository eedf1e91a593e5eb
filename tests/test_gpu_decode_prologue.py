"""GPU: `featmap_rotary_decode` -- feature map and rotary of q and k of a call's new tokens in one launch, at positions read from the
decode state on the device.  Every comparison is `torch.equal`: the reference is today's layer path, `mhla_amd.featmap_rotary` on
`cos.index_select(0, p)` / `sin.index_select(0, p)` with the expected positions p, and rows that must be zero are compared to zeros."""
import pytest
import torch

from gpu_util import DEV, launches, poison

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(1, 1, 8), (4, 2, 64), (3, 3, 40)]    # (H, Hkv, K): one 4 + 4 piece; 16-byte pieces for 16-bit tensors; a half row that is no multiple of 8
FMAPS = [None, "relu", "elu"]
ROWS, V, CAP = 256, 8, 4
POS = [0, 63, 64, 200, 254, 5]                  # six slots of a pool


def tokens(B, T, H, Hkv, K, dtype, seed=7):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, H, K, generator=g).to(dtype).to(DEV), torch.randn(B, T, Hkv, K, generator=g).to(dtype).to(DEV))


def tables(K, dtype):
    t = torch.arange(ROWS, dtype=torch.float32)
    fr = torch.outer(t, 1.0 / (10000.0 ** (torch.arange(0, K, 2, dtype=torch.float32) / K)))
    return torch.cos(fr).to(dtype).to(DEV), torch.sin(fr).to(dtype).to(DEV)


def pool_at(pos, Hkv, K, kind="dense"):
    """A pool whose slots have seen `pos` tokens (no chunk is read by the prologue: only the positions and the slot map)."""
    import mhla_amd
    n = len(pos)
    if kind == "dense":
        z = lambda *s: torch.zeros(s, device=DEV)
        return mhla_amd.CausalState(z(n, Hkv, CAP, K, V), z(n, Hkv, K, V), z(n, Hkv, K, V), 0, 64, lengths=pos)
    pool = mhla_amd.PagedCausalState.empty(n, Hkv, K, V, CAP, 4 * n, DEV, page_format="h16" if kind == "h16" else "fp32")
    pool.reserve(list(range(n)), list(pos))
    pool._set_lengths(range(n), pos)
    pool.pos.copy_(torch.tensor(pos, dtype=torch.int32))
    return pool


def reference(q, k, cos, sin, p, fmap):
    """Rows [N, ...] at positions p (long [N]; -1: a row that must be zero) through today's path."""
    import mhla_amd
    live = (p >= 0) & (p < ROWS)
    idx = p.clamp(0, ROWS - 1).to(DEV)
    c, s = cos.index_select(0, idx), sin.index_select(0, idx)
    out = []
    for x in (q, k):
        y = mhla_amd.featmap_rotary(x.reshape(1, -1, *x.shape[2:]).contiguous(), c, s, fmap)
        out.append(torch.where(live.to(DEV)[None, :, None, None], y, torch.zeros_like(y)).reshape(x.shape))
    return out


def packed_positions(slots, cu, pos):
    p = torch.full((cu[-1],), -1, dtype=torch.long)
    for s, a, b in zip(slots, cu, cu[1:]):
        p[a:b] = pos[s] + torch.arange(b - a)
    return p


def padded_positions(pos, counts, T, left):
    p = torch.full((len(pos), T), -1, dtype=torch.long)
    for b, (p0, n) in enumerate(zip(pos, counts)):
        t0 = T - n if left else 0
        p[b, t0:t0 + n] = p0 + torch.arange(n)
    return p.flatten()


def same(name, got, want):
    for g, w, which in zip(got, want, "qk"):
        assert g.shape == w.shape and g.dtype == w.dtype
        assert torch.equal(g, w), f"{name}: {which}' differs in {int((g != w).sum())} of {g.numel()} elements"


@pytest.mark.parametrize("fmap", FMAPS, ids=["identity", "relu", "elu"])
@pytest.mark.parametrize("H,Hkv,K", SHAPES, ids=["H1K8", "H4Hkv2K64", "H3K40"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_packed_on_a_pool(dtype, H, Hkv, K, fmap):
    import mhla_amd
    poison()
    cos, sin = tables(K, dtype)
    slots = [4, 1, 5, 2, 0]
    for kind in ("dense", "fp32", "h16") if (K * V) % 64 == 0 else ("dense", "fp32"):
        pool = pool_at(POS, Hkv, K, kind)
        view = pool.at(slots)
        # slot 4: positions 254, 255, then 256 beyond the tables (zeros); slot 1 crosses 63 -> 64; slot 5 takes none; slot 2 takes 67
        # tokens across 128; slot 0 one token at 0.  Then empty sequences first and in the middle.
        for cu in ([0, 3, 6, 6, 73, 74], [0, 0, 3, 3, 70, 71]):
            q, k = tokens(1, cu[-1], H, Hkv, K, dtype)
            want = reference(q, k, cos, sin, packed_positions(slots, cu, POS), fmap)
            got = mhla_amd.featmap_rotary_decode(q, k, cos, sin, view, feature_map=fmap, cu_seqlens=cu)
            same(f"{kind} pool, cu_seqlens={cu}", got, want)
            off = torch.tensor(cu, dtype=torch.int32, device=DEV)
            same(f"{kind} pool, off_dev={cu}", mhla_amd.featmap_rotary_decode(q, k, cos, sin, view, feature_map=fmap, off_dev=off), want)
            if cu[1] == 3:
                assert float(want[0][0, 2].abs().max()) == 0.0 and float(want[0][0, 1].abs().max()) > 0.0, "position 256 is zeros, 255 is not"
        assert pool.lengths == tuple(POS) and pool.pos.tolist() == POS, "the positions are read, never written"


@pytest.mark.parametrize("left", [False, True], ids=["right-padded", "left-padded"])
@pytest.mark.parametrize("fmap", FMAPS, ids=["identity", "relu", "elu"])
@pytest.mark.parametrize("H,Hkv,K", SHAPES, ids=["H1K8", "H4Hkv2K64", "H3K40"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_padded_with_counts(dtype, H, Hkv, K, fmap, left):
    import mhla_amd
    poison()
    cos, sin = tables(K, dtype)
    pos, counts, T = (63, 200, 7), (5, 2, 0), 5
    state = pool_at(pos, Hkv, K)
    q, k = tokens(3, T, H, Hkv, K, dtype)
    want = reference(q, k, cos, sin, padded_positions(pos, counts, T, left), fmap)
    same("a state of its own", mhla_amd.featmap_rotary_decode(q, k, cos, sin, state, feature_map=fmap, counts=counts, left_padded=left), want)
    assert float(want[0][2].abs().max()) == 0.0 and float(want[1][1, 3 if left else 1].abs().max()) > 0.0, "rows outside a window are zeros"
    # the same windows through a slot map: the call's rows 0, 1, 2 are slots 3, 0, 2 of a pool
    pool = pool_at((200, 9, 7, 63), Hkv, K, "fp32")
    same("a view of a paged pool", mhla_amd.featmap_rotary_decode(q, k, cos, sin, pool.at([3, 0, 2]), feature_map=fmap, counts=counts,
                                                                  left_padded=left), want)


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("H,Hkv,K", SHAPES, ids=["H1K8", "H4Hkv2K64", "H3K40"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_no_counts_on_a_state_of_its_own(dtype, H, Hkv, K, T):
    import mhla_amd
    poison()
    cos, sin = tables(K, dtype)
    pos = (0, 63, 254, 130)
    state = pool_at(pos, Hkv, K)
    q, k = tokens(4, T, H, Hkv, K, dtype)
    for fmap in FMAPS:
        want = reference(q, k, cos, sin, padded_positions(pos, (T,) * 4, T, False), fmap)
        same(f"T={T} {fmap}", mhla_amd.featmap_rotary_decode(q, k, cos, sin, state, feature_map=fmap), want)
    # a device slot map with an inactive entry: that row is zeros
    pool = pool_at(pos, Hkv, K)
    view = pool.at(torch.tensor([3, -1, 0, 2], dtype=torch.int32, device=DEV))
    live = padded_positions((130, 0, 0, 254), (T, 0, T, T), T, False)
    same("a device slot map", mhla_amd.featmap_rotary_decode(q, k, cos, sin, view, feature_map="relu"), reference(q, k, cos, sin, live, "relu"))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_a_stale_state_gives_the_same_bits(dtype):
    """Only the device positions are read: a state whose host mirror is behind (device-positioned steps moved `pos`) gives the rows
    of the positions on the device."""
    import mhla_amd
    poison()
    H, Hkv, K = 4, 2, 64
    cos, sin = tables(K, dtype)
    state = pool_at((0, 63, 100), Hkv, K)
    state.pos += 7           # what device-positioned steps do: the mirror stays
    state.stale = True
    q, k = tokens(3, 2, H, Hkv, K, dtype)
    want = reference(q, k, cos, sin, padded_positions((7, 70, 107), (2, 2, 2), 2, False), "relu")
    same("stale", mhla_amd.featmap_rotary_decode(q, k, cos, sin, state, feature_map="relu"), want)
    assert state.lengths == (0, 63, 100) and state.stale


@pytest.mark.parametrize("H,Hkv,K", SHAPES, ids=["H1K8", "H4Hkv2K64", "H3K40"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_strided_and_in_place(dtype, H, Hkv, K):
    """q and k as slices of one fused projection, rotated in place: the result of the out-of-place call, and the rest of the buffer
    keeps every bit."""
    import mhla_amd
    poison()
    cos, sin = tables(K, dtype)
    slots, cu = [4, 1, 5, 2, 0], [0, 3, 6, 6, 73, 74]
    view = pool_at(POS, Hkv, K, "fp32").at(slots)
    N, pad = cu[-1], 8
    ld = (H + Hkv) * K + 2 * pad
    g = torch.Generator().manual_seed(9)
    fused = torch.randn(1, N, ld, generator=g).to(dtype).to(DEV)
    before = fused.clone()
    q = fused[..., pad:pad + H * K].view(1, N, H, K)
    k = fused[..., pad + H * K:pad + (H + Hkv) * K].view(1, N, Hkv, K)
    want = mhla_amd.featmap_rotary_decode(q, k, cos, sin, view, feature_map="elu", cu_seqlens=cu)
    assert torch.equal(fused, before), "the out-of-place call writes neither q nor k"
    same("strided, out of place", want, reference(q.contiguous(), k.contiguous(), cos, sin, packed_positions(slots, cu, POS), "elu"))
    yq, yk = mhla_amd.featmap_rotary_decode(q, k, cos, sin, view, feature_map="elu", cu_seqlens=cu, inplace=True)
    assert yq is q and yk is k
    same("in place", (q, k), want)
    assert torch.equal(fused[..., :pad], before[..., :pad]) and torch.equal(fused[..., ld - pad:], before[..., ld - pad:]), "the rest of the buffer"


def test_one_launch_per_call():
    import mhla_amd
    poison()
    H, Hkv, K, dtype = 4, 2, 64, torch.bfloat16
    cos, sin = tables(K, dtype)
    view = pool_at(POS, Hkv, K, "fp32").at([4, 1, 5, 2, 0])
    cu = [0, 3, 6, 6, 73, 74]
    q, k = tokens(1, cu[-1], H, Hkv, K, dtype)
    off = torch.tensor(cu, dtype=torch.int32, device=DEV)
    assert launches(lambda: mhla_amd.featmap_rotary_decode(q, k, cos, sin, view, feature_map="relu", off_dev=off)) == {"k_fr_decode": 1}
    assert launches(lambda: mhla_amd.featmap_rotary_decode(q, k, cos, sin, view, feature_map="relu", cu_seqlens=cu)) == {"k_fr_decode": 1}
    q3, k3 = tokens(6, 3, H, Hkv, K, dtype)
    ran = launches(lambda: mhla_amd.featmap_rotary_decode(q3, k3, cos, sin, pool_at(POS, Hkv, K), counts=(3, 0, 1, 2, 3, 3), left_padded=True, inplace=True))
    assert ran == {"k_fr_decode": 1} and "k_fmap_rotary" not in ran
