"""The fp64 references of tests/neighbour_refs.py against the oracle, on small fp32 inputs at 1e-6 (no GPU needed): what
test_gpu_neighbours.py compares the HIP kernels with is the operation the oracle (and through the golden fixtures the reference
implementation) defines."""
import pytest
import torch

import neighbour_refs as nr
from conftest import load_golden, rel_err
from oracle import mhla_oracle as orc

TOL = 1e-6


@pytest.mark.parametrize("D", [8, 24, 100])
def test_rmsnorm_gate_ref_matches_oracle(D):
    g_ = torch.Generator().manual_seed(D)
    x, g = torch.randn(5, 3, D, generator=g_), torch.randn(5, 3, D, generator=g_)
    w = torch.rand(D, generator=g_) + 0.5
    assert rel_err(nr.rmsnorm_gate_ref(x, g, w, 1e-5), orc.rms_norm_swish_gate(x, g, w, 1e-5)) < TOL
    assert rel_err(nr.rmsnorm_gate_ref(x, g, None, 1e-5), orc.rms_norm_swish_gate(x, g, None, 1e-5)) < TOL
    assert rel_err(nr.rmsnorm_gate_ref(x, None, w, 1e-5), orc.rms_norm(x, w, 1e-5)) < TOL
    assert rel_err(nr.rmsnorm_gate_ref(x, None, None, 1e-5), orc.rms_norm(x, None, 1e-5)) < TOL


def test_rmsnorm_gate_ref_matches_golden():
    g = load_golden("fla_neighbours")
    assert rel_err(nr.rmsnorm_gate_ref(g["o"], g["g"], g["w"], 1e-5), g["gated"]) < TOL
    assert rel_err(nr.rmsnorm_gate_ref(g["o"], None, g["w"], 1e-5), g["normed"]) < TOL


def _neox_tables(rows, K, dtype=torch.float32):
    inv = 1.0 / (10000.0 ** (torch.arange(0, K, 2, dtype=torch.float32) / K))
    fr = torch.outer(torch.arange(rows, dtype=torch.float32), inv)
    return torch.cos(fr).to(dtype), torch.sin(fr).to(dtype)


@pytest.mark.parametrize("K,off", [(8, 0), (24, 5), (64, 31)])
@pytest.mark.parametrize("fmap", [None, "relu", "elu"])
def test_featmap_rotary_ref_matches_oracle(K, off, fmap):
    import torch.nn.functional as F
    g_ = torch.Generator().manual_seed(K + off)
    B, T, H = 2, 9, 3
    x = torch.randn(B, T, H, K, generator=g_)
    x.view(-1)[::7] = 0.0
    cos, sin = _neox_tables(off + T, K)
    f = {None: lambda t: t, "relu": torch.relu, "elu": lambda t: F.elu(t) + 1}[fmap]
    assert rel_err(nr.featmap_rotary_ref(x, cos, sin, fmap, off), orc.neox_rotary(f(x), offset=off)) < TOL


def test_featmap_rotary_ref_matches_golden():
    g = load_golden("fla_neighbours")
    x = g["x"]
    cos, sin = _neox_tables(x.shape[1], x.shape[-1])
    assert rel_err(nr.featmap_rotary_ref(x, cos, sin, None, 0), g["rot"]) < TOL


@pytest.mark.parametrize("C,D,norm", [(48, 8, True), (48, 24, True), (256, 128, True), (48, 24, False)])
def test_qk_prologue_ref_matches_oracle(C, D, norm):
    from mhla_amd.modules.wan import _rope_table
    g_ = torch.Generator().manual_seed(C + D)
    B, grid = 2, (2, 3, 5)
    N, H = 30, C // D
    x = torch.randn(B, N, C, generator=g_)
    w = (torch.rand(C, generator=g_) + 0.5) if norm else None
    freqs = orc.wan_freqs(D)
    cos, sin = _rope_table(freqs, grid, "cpu")
    y, yr = nr.qk_prologue_ref(x, w, 1e-5, 1e-6, rope=(cos, sin), head_dim=D)
    want = orc.relu_eps(orc.rms_norm(x, w, 1e-5) if norm else x, 1e-6)
    assert rel_err(y, want) < TOL
    assert rel_err(yr, orc.wan_rope_apply(want.reshape(B, N, H, D), grid, freqs).reshape(B, N, C)) < TOL
    y1, none = nr.qk_prologue_ref(x, w, 1e-5, 1e-6)
    assert none is None and torch.equal(y1, y)
    # token = row % ntok on the flattened rows
    y2, yr2 = nr.qk_prologue_ref(x.reshape(B * N, C), w, 1e-5, 1e-6, rope=(cos, sin), head_dim=D)
    assert torch.equal(yr2.reshape(yr.shape), yr)


def test_rms_rstd_ref_matches_oracle():
    x = torch.randn(7, 40, generator=torch.Generator().manual_seed(3))
    r = nr.rms_rstd_ref(x, 1e-5)
    assert r.shape == (7,)
    assert rel_err(x.double() * r[:, None], orc.rms_norm(x, None, 1e-5)) < TOL


@pytest.mark.parametrize("pl,bl", [(1, 1), (3, 4), (2, 7), (1, 6)])
def test_lepe2d_layout_maps_round_trip(pl, bl):
    B, C, N = 2, 3, (pl * bl) ** 2
    t = torch.arange(B * N * C, dtype=torch.float64).reshape(B, N, C)
    img = nr.blocks_to_image(t, pl, bl)
    assert img.shape == (B, C, pl * bl, pl * bl)
    assert torch.equal(nr.image_to_blocks(img, pl, bl), t)
    # the same permutation as the oracle's raster -> block-major gather map
    raster = img.permute(0, 2, 3, 1).reshape(B, N, C)
    assert torch.equal(raster[:, orc.block_index_2d(pl, bl)], t)
    # a delta filter that picks the right-hand neighbour: pixel (y, x) receives pixel (y, x + 1)
    w = torch.zeros(C, 1, 3, 3)
    w[:, 0, 1, 2] = 1.0
    got = nr.blocks_to_image(nr.lepe2d_ref(t, w, None, None, pl, bl), pl, bl)
    want = torch.zeros_like(img)
    want[..., :-1] = img[..., 1:]
    assert torch.equal(got, want)


@pytest.mark.parametrize("grid", [(1, 1, 1), (2, 9, 11), (3, 4, 2)])
def test_lepe3d_layout_maps_round_trip(grid):
    B, C, N = 2, 3, grid[0] * grid[1] * grid[2]
    t = torch.arange(B * N * C, dtype=torch.float64).reshape(B, N, C)
    vid = nr.raster_to_video(t, grid)
    assert vid.shape == (B, C, *grid)
    assert torch.equal(nr.video_to_raster(vid), t)
    f, h, w_ = (g - 1 for g in grid)
    assert torch.equal(vid[1, :, f, h, w_], t[1, (f * grid[1] + h) * grid[2] + w_])
    w = torch.zeros(C, 1, 3, 3, 3)
    w[:, 0, 2, 1, 1] = 1.0   # the next frame's pixel
    got = nr.raster_to_video(nr.lepe3d_ref(t, w, None, t, grid), grid)
    want = vid.clone()
    want[:, :, :-1] += vid[:, :, 1:]
    assert torch.equal(got, want)
