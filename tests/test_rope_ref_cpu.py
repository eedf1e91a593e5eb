"""The fp64 reference of the rotary block-mix operator (gpu_util.rope_blockmix_fp64), checked without a GPU: its rotation against the
oracle's Wan rotation, its autograd gradients against the oracle's closed-form backward, and its own conditioning
(the same function in fp32) at every shape the GPU parity test holds the kernels to."""
import pytest
import torch

from conftest import rel_err
from gpu_util import ROPE_CASES, TOL, make_rope_inputs, rope_blockmix_fp64, rope_case_seed, rope_rotate
from oracle import mhla_oracle as orc


@pytest.mark.parametrize("D", [64, 128])
def test_rope_rotate_matches_wan_rope_apply(D):
    """rope_rotate with the Wan layer's cos / sin tables == the oracle's complex multiplication (wan_rope_apply), to 1e-6."""
    from mhla_amd.modules.wan import _rope_table
    grid = (4, 6, 10)
    N = grid[0] * grid[1] * grid[2]
    freqs = orc.wan_freqs(D)
    cos, sin = _rope_table(freqs, grid, "cpu")
    assert cos.shape == sin.shape == (N, D // 2) and cos.dtype == torch.float32
    x = torch.randn(2, N, 3, D, generator=torch.Generator().manual_seed(D))
    want = orc.wan_rope_apply(x, grid, freqs)
    for dt in (torch.float32, torch.float64):
        got = rope_rotate(x.to(dt), cos.to(dt), sin.to(dt))
        assert got.dtype == dt and got.shape == x.shape
        assert rel_err(got, want) < 1e-6
    # tables of another float dtype than x are taken to x's
    assert torch.equal(rope_rotate(x.double(), cos, sin), rope_rotate(x.double(), cos.double(), sin.double()))


def _unrotate(g, cos, sin):
    """The transposed rotation: the gradient w.r.t. x of <rope_rotate(x), g>."""
    return rope_rotate(g, cos, -sin)


@pytest.mark.parametrize("case", [(2, 2, 5, 12, 24, True, True), (1, 3, 7, 9, 16, True, False), (2, 1, 4, 6, 8, False, True), (1, 2, 1, 10, 16, True, False)],
                         ids=lambda c: "-".join(str(int(x)) for x in c))
def test_reference_gradients_match_closed_form(case):
    """Autograd through rotation + gather + operator + scatter == the oracle's hand-derived backward on the rotated pair with the
    un-rotated pair as the normaliser's: dq = R^T dq_num + dq_den, dk = R^T dk_num + dk_den (block-major, scattered back), to 1e-10."""
    B, H, M, S, D, normalize, gather = case
    q, k, v, W, do, cos, sin, perm = make_rope_inputs(B, H, M, S, D, torch.float64, seed=rope_case_seed(case), gather=gather)
    out, dq, dk, dv, dW = rope_blockmix_fp64(q, k, v, W, do, cos, sin, perm, normalize)
    rows = torch.arange(M * S) if perm is None else perm.long()
    bm = lambda t: t[:, rows]
    cb, sb = cos.double()[rows], sin.double()[rows]   # the angles of the block-major rows
    qr, kr = rope_rotate(bm(q), cb, sb), rope_rotate(bm(k), cb, sb)
    assert torch.equal(qr, bm(rope_rotate(q, cos, sin)))   # rotating and gathering commute: the tables are indexed by token row
    Wd = W.double()
    den = dict(q_den=bm(q), k_den=bm(k)) if normalize else {}
    want_out = orc.blockmix_fwd(qr, kr, bm(v), Wd, 1e-6, normalize=normalize, **den)
    g = orc.blockmix_bwd(qr, kr, bm(v), Wd, bm(do), 1e-6, normalize=normalize, **den)
    want_dq, want_dk = _unrotate(g["dq"], cb, sb), _unrotate(g["dk"], cb, sb)
    if normalize:
        want_dq, want_dk = want_dq + g["dq_den"], want_dk + g["dk_den"]

    def scat(t):
        r = torch.empty_like(t)
        r[:, rows] = t
        return r
    for name, got, want in (("out", out, scat(want_out)), ("dq", dq, scat(want_dq)), ("dk", dk, scat(want_dk)), ("dv", dv, scat(g["dv"])), ("dW", dW, g["dW"])):
        assert got.dtype == torch.float64 and got.shape == want.shape, name
        if M == 1 and name == "dW":   # W cancels between numerator and normaliser up to eps: dW ~ eps-sized, a difference of large terms
            assert (got - want).abs().max() < 1e-10 and want.abs().max() < 1e-3
            continue
        assert rel_err(got, want) < 1e-10, f"{name}: {rel_err(got, want):.3e}"


@pytest.mark.parametrize("case", ROPE_CASES, ids=lambda c: "-".join(str(int(x)) for x in c))
def test_reference_conditioning(case):
    """The reference evaluated in fp32 stays within a tenth of the fp32 tolerance (2e-4) of its fp64 value at every GPU case, so
    that bound measures the kernels and not the reference's own sensitivity to rounding (measured: at most 1.3e-6)."""
    B, H, M, S, D, normalize, gather = case
    q, k, v, W, do, cos, sin, perm = make_rope_inputs(B, H, M, S, D, torch.float32, seed=rope_case_seed(case), gather=gather)
    r64 = rope_blockmix_fp64(q, k, v, W, do, cos, sin, perm, normalize)
    r32 = rope_blockmix_fp64(q, k, v, W, do, cos, sin, perm, normalize, dtype=torch.float32)
    for name, a, b in zip(("out", "dq", "dk", "dv", "dW"), r32, r64):
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        if M == 1 and name == "dW":   # ~ 0 (W cancels up to eps): the GPU test holds it to an absolute 1e-3 -- a tenth of that here
            assert (a.double() - b).abs().max() < 1e-4 and b.abs().max() < 1e-3
            continue
        e = rel_err(a, b)
        print(f"{name}: fp32 vs fp64 {e:.2e}")
        assert e < TOL[torch.float32] / 10, f"{name}: the fp32 evaluation of the reference is {e:.3e} from fp64"
