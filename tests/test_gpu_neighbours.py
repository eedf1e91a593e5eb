"""The kernels around the two operators -- per-head RMSNorm x gate, feature map + rotary, the Wan q / k prologue (+ rope, both
directions), mhla_rms_rstd, the 2-D and 3-D LePE convolutions and their weight gradients (csrc/epilogue.hpp, lepe.hpp,
capi_misc.hip) -- against the plain fp64 references of neighbour_refs.py, at every launch shape of their dispatch: each template
instantiation, the interior and the edges of each kernel family, the second trip of every capped grid-stride loop (with the
per-workgroup dw accumulators that persist across trips), strided views addressed in place, the decode shape, and the alignment
fallbacks of the LePE dispatch.  Each case is the smallest shape that reaches its code path.

Tolerances are the derived ones of gpu_util, not fitted: all these kernels do fp32 math on the given
values and round once, so 16-bit results keep TOL[dtype] = u + 1e-3 (check() also holds the part beyond the final rounding to
1e-3), fp32 results of 16-bit problems (dw with an fp32 weight, y of the prologue, rstd) keep DW_TOL = 1e-3, fp32 problems keep
TOL[float32].  The references see the rounded 16-bit inputs; an fp32 evaluation of the norm x gate rounded to 16 bits stays 2.3e-7
beyond the final rounding of fp64 at the largest row counts used here, so the references leave the whole 1e-3 to the kernels.

Not covered: the FORWARD grid caps of 2^20 workgroups (norm_fwd_grid) -- a second trip there needs over 4 M rows, too slow
against a CPU reference."""
import functools

import pytest
import torch

import neighbour_refs as nr
from gpu_util import DEV, DW_TOL, TOL, check, launches, poison

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAN = float("nan")


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _leaf(t):
    return None if t is None else t.detach().cpu().double().clone().requires_grad_(True)


def _dev(t, grad=True):
    return None if t is None else t.detach().to(DEV).requires_grad_(grad)


def _f32tol(dtype):
    """fp32-stored result of a problem in `dtype`."""
    return DW_TOL[dtype]


def _lib():
    from mhla_amd import _lib as L
    return L.load()


# -------------------------------------------------------------------------------------------------
# per-head RMSNorm x gate
# -------------------------------------------------------------------------------------------------
NORM_D = [4, 24, 64, 68, 100, 128, 132, 256, 260, 508, 512]   # <.,16> | <.,32> | NV = 1 | NV = 2: interiors and both edges
NORM_ROWS = [1, 3, 17, 37 * 4 + 1]
NORM_FAMILY_D = [24, 100, 132, 508]                           # one D strictly inside each family
EPS = 1e-5


def _norm_rows_per_workgroup(D):
    """Rows a workgroup of the backward covers per grid-stride trip: 4 waves x 64 / LPR rows (narrow rows) or x 1."""
    return 16 if D <= 64 else 8 if D <= 128 else 4


def _norm_inputs(rows, D, dtype, gate, weight, seed=0):
    g_ = torch.Generator().manual_seed(1000 * D + rows % 1000 + seed)
    x = torch.randn(rows, D, generator=g_).to(dtype)
    g = torch.randn(rows, D, generator=g_).to(dtype) if gate else None
    w = None if weight is None else (torch.rand(D, generator=g_) + 0.5).to(weight)
    dy = torch.randn(rows, D, generator=g_).to(dtype)
    return x, g, w, dy


def _norm_ref(x, g, w, dy):
    xr, gr, wr = _leaf(x), _leaf(g), _leaf(w)
    y = nr.rmsnorm_gate_ref(xr, gr, wr, EPS)
    y.backward(dy.double())
    return {"y": y.detach(), "dx": xr.grad, "dg": None if g is None else gr.grad, "dw": None if w is None else wr.grad}


def _norm_hip(x, g, w, dy):
    import mhla_amd
    xd, gd, wd = _dev(x), _dev(g), _dev(w)
    poison()
    y = mhla_amd.rmsnorm_gate(xd, gd, wd, EPS)
    assert y.dtype == x.dtype and y.shape == x.shape
    poison()
    y.backward(dy.to(DEV))
    return {"y": y.detach(), "dx": xd.grad, "dg": None if g is None else gd.grad, "dw": None if w is None else wd.grad}


def _norm_check(tag, got, want, dtype):
    check(f"y {tag}", got["y"], want["y"], TOL[dtype])
    check(f"dx {tag}", got["dx"], want["dx"], TOL[dtype])
    if want["dg"] is not None:
        check(f"dg {tag}", got["dg"], want["dg"], TOL[dtype])
    if want["dw"] is not None:
        wd = got["dw"].dtype
        check(f"dw {tag}", got["dw"], want["dw"], TOL[wd] if wd != F32 else _f32tol(dtype))
    else:
        assert got["dw"] is None


def _norm_case(rows, D, dtype, gate, weight=F32):
    inp = _norm_inputs(rows, D, dtype, gate, weight)
    got, want = _norm_hip(*inp), _norm_ref(*inp)
    _norm_check(f"rows={rows} D={D}", got, want, dtype)
    return inp, got, want


@pytest.mark.parametrize("gate", [True, False])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
@pytest.mark.parametrize("D", NORM_D)
def test_rmsnorm_gate_family_interiors_and_edges(D, dtype, gate):
    """Every kernel family at its first, an interior (dead tail lanes) and its last D; rows below, at and beyond one workgroup."""
    for rows in NORM_ROWS:
        _norm_case(rows, D, dtype, gate)


@pytest.mark.parametrize("gate", [True, False])
@pytest.mark.parametrize("D", NORM_FAMILY_D)
def test_rmsnorm_gate_fp16(D, gate):
    for rows in (3, 37 * 4 + 1):
        _norm_case(rows, D, F16, gate)


@pytest.mark.parametrize("gate", [True, False])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
@pytest.mark.parametrize("D", NORM_FAMILY_D)
def test_rmsnorm_gate_without_weight(D, dtype, gate):
    """weight=None: the a.w == nullptr branches of the four kernels; no weight gradient."""
    for rows in (3, 37 * 4 + 1):
        _norm_case(rows, D, dtype, gate, weight=None)


def test_rmsnorm_gate_weight_stored_in_bf16():
    """A bf16 weight parameter: dw is rounded to bf16 and held to TOL[bf16]."""
    _, got, _ = _norm_case(37 * 4 + 1, 100, BF16, True, weight=BF16)
    assert got["dw"].dtype == BF16


@functools.lru_cache(maxsize=1)
def _norm_big_case():
    inp = _norm_inputs(131072 + 5, 24, BF16, True, F32)
    return inp, _norm_ref(*inp)


@pytest.mark.parametrize("rows,D,dtype", [(131072 + 5, 24, BF16), (65536 + 3, 100, BF16), (32768 + 3, 132, BF16), (32768 + 3, 260, BF16),
                                          (131072 + 5, 24, F32), (65536 + 3, 100, F32)], ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_rmsnorm_gate_second_grid_stride_trip(rows, D, dtype):
    """Rows past the backward's workgroup cap: some workgroups take a second trip (ragged: not all of them), and their dw
    accumulators carry over from the first."""
    assert _lib().mhla_rmsnorm_gate_dw_rows(rows) * _norm_rows_per_workgroup(D) < rows
    if (rows, D, dtype) == (131072 + 5, 24, BF16):
        inp, want = _norm_big_case()
        _norm_check(f"rows={rows} D={D}", _norm_hip(*inp), want, dtype)
    else:
        _norm_case(rows, D, dtype, True)


def test_rmsnorm_gate_is_deterministic():
    inp, _ = _norm_big_case()
    a, b = _norm_hip(*inp), _norm_hip(*inp)
    for k in ("y", "dx", "dg", "dw"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("D", NORM_FAMILY_D)
def test_rmsnorm_gate_dw_partial_rows_are_all_summed(D):
    """Below the cap: dw of the whole equals the sum of the dw of its two halves (another split of the rows over the per-workgroup
    partial rows), and the reference."""
    rows = 37 * 4 + 1
    assert _lib().mhla_rmsnorm_gate_dw_rows(rows) * _norm_rows_per_workgroup(D) >= rows
    (x, g, w, dy), got, _ = _norm_case(rows, D, BF16, True)
    h = rows // 2
    lo, hi = _norm_hip(x[:h], g[:h], w, dy[:h]), _norm_hip(x[h:], g[h:], w, dy[h:])
    check("dw halves", got["dw"], (lo["dw"].double() + hi["dw"].double()).cpu(), _f32tol(BF16))


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
def test_rmsnorm_gate_views_of_a_packed_buffer(dtype):
    """x and g as the two slices of one packed [rows, 2, D] buffer: the op copies them, the gradients arrive in the buffer."""
    import mhla_amd
    rows, D = 37, 100
    x, g, w, dy = _norm_inputs(rows, D, dtype, True, F32, seed=7)
    want = _norm_ref(x, g, w, dy)
    pk = torch.stack((x, g), dim=1).to(DEV).requires_grad_(True)
    wd = _dev(w)
    poison()
    y = mhla_amd.rmsnorm_gate(pk[:, 0], pk[:, 1], wd, EPS)
    poison()
    y.backward(dy.to(DEV))
    got = {"y": y.detach(), "dx": pk.grad[:, 0], "dg": pk.grad[:, 1], "dw": wd.grad}
    _norm_check("packed", got, want, dtype)


# -------------------------------------------------------------------------------------------------
# feature map + rotary
# -------------------------------------------------------------------------------------------------
def _fm_inputs(B, T, H, K, dtype, fmap, table_rows, seed=0):
    g_ = torch.Generator().manual_seed(100 * K + T + seed)
    x = torch.randn(B, T, H, K, generator=g_)
    flat = x.view(-1)
    if fmap == "elu":
        flat[1::3] = -(5.0 + 15.0 * torch.rand(flat[1::3].shape, generator=g_))      # deep in the exp branch: [-20, -5]
    if fmap is not None:
        flat[::7] = 0.0                                                               # the tie of the mask / the branch
    if fmap == "elu" and T >= 4:
        x[:, :2] = -(5.0 + 15.0 * torch.rand(x[:, :2].shape, generator=g_))           # two tokens wholly in [-20, -5]
    dy = torch.randn(B, T, H, K, generator=g_)
    ang = torch.rand(table_rows, K // 2, generator=g_) * 6.2831853
    return x.to(dtype), dy.to(dtype), torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)


def _fm_ref(x, dy, cos, sin, fmap, off):
    xr = _leaf(x)
    y = nr.featmap_rotary_ref(xr, cos, sin, fmap, off)
    y.backward(dy.double())
    return y.detach(), xr.grad


def _fm_case(B, T, H, K, dtype, fmap, off=0, table_rows=None, sliced=False):
    import mhla_amd
    rows = table_rows or off + T
    x, dy, cos, sin = _fm_inputs(B, T, H, K, dtype, fmap, rows)
    want, wdx = _fm_ref(x, dy, cos, sin, fmap, off)
    cd, sd = cos.to(DEV), sin.to(DEV)
    if sliced:   # tables cut out of wider ones: row stride K, the rest NaN
        wide = torch.full((2, rows, K), NAN, dtype=dtype, device=DEV)
        wide[0, :, :K // 2], wide[1, :, :K // 2] = cd, sd
        cd, sd = wide[0, :, :K // 2], wide[1, :, :K // 2]
        assert cd.stride(0) == K and not cd.is_contiguous()
    xd = _dev(x)
    poison()
    y = mhla_amd.featmap_rotary(xd, cd, sd, fmap, off)
    assert y.dtype == dtype
    poison()
    y.backward(dy.to(DEV))
    tag = f"B={B} T={T} H={H} off={off}"
    check(f"y {tag}", y, want, TOL[dtype])
    check(f"dx {tag}", xd.grad, wdx, TOL[dtype])
    if fmap == "elu" and T >= 4:   # normalised by the small values of the exp branch alone
        check(f"y exp-branch tokens {tag}", y[:, :2], want[:, :2], TOL[dtype])
        check(f"dx exp-branch tokens {tag}", xd.grad[:, :2], wdx[:, :2], TOL[dtype])


@pytest.mark.parametrize("fmap", [None, "relu", "elu"])
@pytest.mark.parametrize("K,dtype", [(K, dt) for K in (8, 24, 64, 256) for dt in (F32, BF16)] + [(64, F16)],
                         ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_featmap_rotary_shapes(K, dtype, fmap):
    """(2, 77, 3): more than one workgroup and a ragged last one (462 K / 8 threads: 462, 1386, 3696, 14784, none a multiple of
    256), with and without a table offset; (1, 1, 1): a single thread group; the decode shape: one token at the last row of a
    4096-row table."""
    threads = 2 * 77 * 3 * K // 8
    assert threads > 256 and threads % 256
    _fm_case(2, 77, 3, K, dtype, fmap)
    _fm_case(2, 77, 3, K, dtype, fmap, off=5)
    _fm_case(1, 1, 1, K, dtype, fmap)
    _fm_case(2, 1, 3, K, dtype, fmap, off=4095, table_rows=4096)


@pytest.mark.parametrize("fmap", [None, "elu"])
@pytest.mark.parametrize("K,dtype", [(8, BF16), (24, F32), (64, F16), (256, BF16)], ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_featmap_rotary_tables_sliced_out_of_wider_ones(K, dtype, fmap):
    _fm_case(2, 9, 3, K, dtype, fmap, off=3, sliced=True)
    _fm_case(1, 1, 2, K, dtype, fmap, off=4095, table_rows=4096, sliced=True)


@pytest.mark.parametrize("fmap", [None, "relu", "elu"])
@pytest.mark.parametrize("K,dtype", [(8, BF16), (24, F32), (64, BF16), (256, F16)], ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_featmap_rotary_views_of_a_packed_buffer(K, dtype, fmap):
    """q and k as the two slices of a packed [B, T, 2, H, K] buffer, addressed in place; the gradient lands in the buffer."""
    import mhla_amd
    from mhla_amd import ops
    B, T, H, off = 2, 13, 3, 2
    xq, dyq, cos, sin = _fm_inputs(B, T, H, K, dtype, fmap, off + T, seed=1)
    xk, dyk, _, _ = _fm_inputs(B, T, H, K, dtype, fmap, off + T, seed=2)
    wq, wdq = _fm_ref(xq, dyq, cos, sin, fmap, off)
    wk, wdk = _fm_ref(xk, dyk, cos, sin, fmap, off)
    cd, sd = cos.to(DEV), sin.to(DEV)
    for both in (True, False):
        pk = torch.stack((xq, xk), dim=2).to(DEV).requires_grad_(True)
        q, k = pk[:, :, 0], pk[:, :, 1]
        assert ops._strided_ok(q) and ops._strided_ok(k) and not q.is_contiguous()
        poison()
        yq = mhla_amd.featmap_rotary(q, cd, sd, fmap, off)
        loss = (yq.float() * dyq.to(DEV).float()).sum()
        check(f"y q both={both}", yq, wq, TOL[dtype])
        if both:
            yk = mhla_amd.featmap_rotary(k, cd, sd, fmap, off)
            loss = loss + (yk.float() * dyk.to(DEV).float()).sum()
            check("y k", yk, wk, TOL[dtype])
        poison()
        loss.backward()
        if both:
            check("dx packed", pk.grad, torch.stack((wdq, wdk), dim=2), TOL[dtype])
        else:
            check("dx q", pk.grad[:, :, 0], wdq, TOL[dtype])
            assert float(pk.grad[:, :, 1].abs().max()) == 0.0


# -------------------------------------------------------------------------------------------------
# q / k prologue (+ rope), mhla_rms_rstd
# -------------------------------------------------------------------------------------------------
NTOK = 30
PRO_FWD_ROWS_PER_TRIP = 16384 * 4    # k_qk_prologue, k_rms_rstd: at most 16384 workgroups of 4 rows


def _pro_inputs(lead, C, hd, dtype, norm, seed=0):
    g_ = torch.Generator().manual_seed(10 * C + (hd or 0) + seed)
    x = torch.randn(*lead, C, generator=g_).to(dtype)
    w = (torch.rand(C, generator=g_) + 0.5) if norm else None
    dy, dyr = torch.randn(*lead, C, generator=g_), torch.randn(*lead, C, generator=g_)
    rope = None
    if hd:
        ang = torch.rand(NTOK, hd // 2, generator=g_) * 6.2831853
        rope = (torch.cos(ang), torch.sin(ang))
    return x, w, dy, dyr, rope


def _pro_ref(x, w, dy, dyr, rope, hd, use=("y", "yr")):
    xr, wr = _leaf(x), _leaf(w)
    y, yr = nr.qk_prologue_ref(xr, wr, 1e-5, 1e-6, rope=rope, head_dim=hd)
    loss = 0.0
    if "y" in use:
        loss = loss + (y * dy.double()).sum()
    if "yr" in use and yr is not None:
        loss = loss + (yr * dyr.double()).sum()
    if use:
        loss.backward()
    return {"y": y.detach(), "yr": None if yr is None else yr.detach(), "dx": xr.grad, "dw": None if w is None else wr.grad}


def _pro_hip(x, w, dy, dyr, rope, hd, use=("y", "yr"), xd=None):
    import mhla_amd
    xd = _dev(x) if xd is None else xd
    wd = _dev(w)
    poison()
    if rope is not None:
        y, yr = mhla_amd.qk_prologue(xd, wd, 1e-5, 1e-6, rope=tuple(t.to(DEV) for t in rope), head_dim=hd)
    else:
        y, yr = mhla_amd.qk_prologue(xd, wd, 1e-5, 1e-6), None
    assert y.dtype == F32 and y.shape == x.shape
    loss = 0.0
    if "y" in use:
        loss = loss + (y * dy.to(DEV)).sum()
    if "yr" in use and yr is not None:
        loss = loss + (yr * dyr.to(DEV)).sum()
    if use:
        poison()
        loss.backward()
    return {"y": y.detach(), "yr": None if yr is None else yr.detach(), "dx": xd.grad if xd.is_leaf else None,
            "dw": None if w is None else wd.grad}


def _pro_check(tag, got, want, dtype, grads=True):
    check(f"y {tag}", got["y"], want["y"], _f32tol(dtype))
    if want["yr"] is not None:
        check(f"y rope {tag}", got["yr"], want["yr"], _f32tol(dtype))
    if grads:
        if got["dx"] is not None:
            check(f"dx {tag}", got["dx"], want["dx"], TOL[dtype])
        if want["dw"] is not None:
            check(f"dw {tag}", got["dw"], want["dw"], _f32tol(dtype))


PRO_C_HD = [(C, hd) for C in (8, 72, 1024, 1032, 1152, 2048) for hd in (8, 24, 128) if C % hd == 0]


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=_name)
@pytest.mark.parametrize("C,hd", PRO_C_HD)
def test_qk_prologue_with_rope(C, hd, dtype):
    """NV = 2 (C <= 1024) and NV = 4 (C <= 2048) at their first, an interior and their last C; one lane = one head (head_dim 8),
    a head over three lanes (24) and over sixteen (128); norm on and off; one and three batches of 30 tokens."""
    for norm in (True, False):
        for B in (1, 3):
            inp = _pro_inputs((B, NTOK), C, hd, dtype, norm, seed=B)
            _pro_check(f"C={C} hd={hd} norm={norm} B={B}", _pro_hip(*inp, hd), _pro_ref(*inp, hd), dtype)


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=_name)
@pytest.mark.parametrize("C", [8, 72, 1024, 1032, 1152, 2048])
def test_qk_prologue_single_output(C, dtype):
    for norm in (True, False):
        for B in (1, 3):
            x, w, dy, dyr, _ = _pro_inputs((B, NTOK), C, None, dtype, norm, seed=B)
            _pro_check(f"C={C} norm={norm} B={B}", _pro_hip(x, w, dy, dyr, None, None), _pro_ref(x, w, dy, dyr, None, None), dtype)


@pytest.mark.parametrize("use", [("y",), ("yr",), ("y", "yr")], ids=lambda u: "+".join(u))
@pytest.mark.parametrize("C,hd,dtype", [(72, 24, BF16), (1152, 128, F32)], ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_qk_prologue_gradient_from_either_output(C, hd, dtype, use):
    inp = _pro_inputs((3, NTOK), C, hd, dtype, True, seed=5)
    _pro_check(f"C={C} from {'+'.join(use)}", _pro_hip(*inp, hd, use=use), _pro_ref(*inp, hd, use=use), dtype)


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=_name)
@pytest.mark.parametrize("C", [2056, 4096])
def test_qk_prologue_wide_rows_are_forward_only(C, dtype):
    """NV = 8 (2048 < C <= 4096): forward with and without rope; its backward is not built and says so."""
    for norm in (True, False):
        inp = _pro_inputs((3, NTOK), C, 8, dtype, norm)
        _pro_check(f"C={C} norm={norm}", _pro_hip(*inp, 8, use=()), _pro_ref(*inp, 8, use=()), dtype, grads=False)
    import mhla_amd
    x, w = inp[0], torch.ones(C)
    xd = _dev(x)
    y = mhla_amd.qk_prologue(xd, _dev(w), 1e-5, 1e-6)
    with pytest.raises(RuntimeError, match="C <= 2048"):
        y.sum().backward()


def test_qk_prologue_refuses_rows_wider_than_4096():
    import mhla_amd
    with pytest.raises(RuntimeError, match="C <= 4096"):
        mhla_amd.qk_prologue(torch.zeros(2, 4104, device=DEV), None)


@pytest.mark.parametrize("C", [8, 72])
def test_qk_prologue_forward_second_grid_stride_trip(C):
    rows = 65536 + 3
    assert PRO_FWD_ROWS_PER_TRIP < rows
    inp = _pro_inputs((rows,), C, 8, BF16, True)
    _pro_check(f"rows={rows} C={C}", _pro_hip(*inp, 8, use=()), _pro_ref(*inp, 8, use=()), BF16, grads=False)


@pytest.mark.parametrize("C,hd", [(64, 8), (1152, None)])
def test_qk_prologue_backward_second_grid_stride_trip(C, hd):
    """Rows past the backward's cap of 2048 workgroups: a second trip for the first of them, dw accumulators carried over."""
    rows = 8192 + 3
    assert _lib().mhla_qk_prologue_dw_rows(rows) * 4 < rows
    inp = _pro_inputs((rows,), C, hd, BF16, True)
    _pro_check(f"rows={rows} C={C}", _pro_hip(*inp, hd), _pro_ref(*inp, hd), BF16)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
def test_qk_prologue_view_with_a_mergeable_batch_stride(dtype):
    """x = the middle slice of a packed [B, N, 3, C] projection: rows of stride 3 C read in place, gradient in the buffer."""
    B, C, hd = 3, 72, 24
    x, w, dy, dyr, rope = _pro_inputs((B, NTOK), C, hd, dtype, True, seed=9)
    pk = torch.full((B, NTOK, 3, C), NAN, dtype=dtype)
    pk[:, :, 1] = x
    pk = pk.to(DEV).requires_grad_(True)
    xv = pk[:, :, 1]
    assert xv.reshape(-1, C).data_ptr() == xv.data_ptr() and xv.reshape(-1, C).stride(0) == 3 * C
    got = _pro_hip(x, w, dy, dyr, rope, hd, xd=xv)
    got["dx"] = pk.grad[:, :, 1]
    _pro_check("view", got, _pro_ref(x, w, dy, dyr, rope, hd), dtype)
    assert float(pk.grad[:, :, 0].abs().max()) == 0.0 and float(pk.grad[:, :, 2].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [BF16, F32, F16], ids=_name)
@pytest.mark.parametrize("wide", [False, True], ids=["ldx=C", "ldx=3C"])
@pytest.mark.parametrize("rows", [5, 65536 + 3])
@pytest.mark.parametrize("C", [8, 520, 1536])
def test_rms_rstd(C, rows, wide, dtype):
    """mhla_rms_rstd (no Python entry of its own: through the C ABI as mhla_blockmix_wan_pro calls it): one and two trips of its
    channel loop (C <= 512 < C), rows past its grid cap, dense rows and rows inside a packed buffer whose other slices are NaN."""
    from mhla_amd import _lib as L, ops
    if rows > 5:
        assert PRO_FWD_ROWS_PER_TRIP < rows
    gen = torch.Generator(device=DEV).manual_seed(C + rows)
    buf = torch.full((rows, 3 if wide else 1, C), NAN, dtype=dtype, device=DEV)
    x = buf[:, 1 if wide else 0]
    x.copy_(torch.randn(rows, C, generator=gen, device=DEV))
    assert x.stride(0) == (3 * C if wide else C)
    poison()
    r = torch.empty(rows, dtype=F32, device=DEV)
    L.check(L.load().mhla_rms_rstd(x.data_ptr(), x.stride(0), r.data_ptr(), rows, C, 1e-5, ops._dtype_code(x), ops._stream()), "mhla_rms_rstd")
    want = torch.cat([nr.rms_rstd_ref(t.cpu(), 1e-5) for t in x.split(8192)])
    check(f"y rstd rows={rows} C={C}", r, want, _f32tol(dtype))


# -------------------------------------------------------------------------------------------------
# LePE
# -------------------------------------------------------------------------------------------------
def _conv_by_taps(t, weight):
    """Zero-padded depthwise correlation of [B, C, *spatial] with weight [C, 1, *k], one shifted slice per tap: each output
    touches the values inside its own window and nothing else (what an inf / NaN locality expectation needs)."""
    nd = t.dim() - 2
    ks = weight.shape[2:]
    out = torch.zeros_like(t)
    for tap in torch.cartesian_prod(*[torch.arange(k) for k in ks]).reshape(-1, nd).tolist():
        src, dst = [slice(None)] * 2, [slice(None)] * 2
        for ax, (d, k) in enumerate(zip(tap, ks)):
            sh, n = d - k // 2, t.shape[2 + ax]           # out[p] += w[d] in[p + sh]
            lo, hi = max(0, -sh), min(n, n - sh)
            dst.append(slice(lo, hi))
            src.append(slice(lo + sh, hi + sh))
        if any(s.stop <= s.start for s in dst[2:]):
            continue
        w = weight[(slice(None), 0) + tuple(tap)].reshape(1, -1, *([1] * nd))
        out[tuple(dst)] += w * t[tuple(src)]
    return out


def _same_class(got, want):
    """Non-finite values agree in kind (+inf, -inf, NaN) and place."""
    g, w = got.float().cpu(), want.float()
    return (torch.equal(torch.isnan(g), torch.isnan(w)) and torch.equal(torch.isposinf(g), torch.isposinf(w))
            and torch.equal(torch.isneginf(g), torch.isneginf(w)))


def _lepe_inputs(B, N, C, wshape, dtype, seed):
    g_ = torch.Generator().manual_seed(seed)
    v = torch.randn(B, N, C, generator=g_).to(dtype)
    w = torch.randn(C, 1, *wshape, generator=g_) * 0.3          # fp32 parameters: dw, dbias are fp32 results
    bias = torch.randn(C, generator=g_)
    add = torch.randn(B, N, C, generator=g_).to(dtype)
    dy = torch.randn(B, N, C, generator=g_).to(dtype)
    return v, w, bias, add, dy


def _embed(t, view):
    """[B, N, C] as a slice of a NaN-filled buffer on the device; (leaf buffer, view of it).
    packed: [B, N, 3, C][:, :, 2]; pad4: [B, N, C + 4][..., :C] (row stride 4 mod 8 elements); off4: [B, N, C + 8][..., 4:4 + C]
    (base 4 elements off).  Every address stays a multiple of 4 elements."""
    B, N, C = t.shape
    if view == "packed":
        buf = torch.full((B, N, 3, C), NAN, dtype=t.dtype)
        buf[:, :, 2] = t
        sl = (slice(None), slice(None), 2)
    elif view == "pad4":
        buf = torch.full((B, N, C + 4), NAN, dtype=t.dtype)
        buf[:, :, :C] = t
        sl = (slice(None), slice(None), slice(0, C))
    else:
        buf = torch.full((B, N, C + 8), NAN, dtype=t.dtype)
        buf[:, :, 4:4 + C] = t
        sl = (slice(None), slice(None), slice(4, 4 + C))
    buf = buf.to(DEV).requires_grad_(True)
    return buf, sl


def _lepe_case(kind, geom, C, dtype, B=3, view="packed", seed=0, expect=None):
    """kind "2d": geom = (K, pl, bl); "3d": geom = (F, H, W).  Forward + every gradient against the fp64 convolution; `expect`:
    the kernel name the forward and the input gradient must launch."""
    import mhla_amd
    if kind == "2d":
        K, pl, bl = geom
        N, wshape = (pl * bl) ** 2, (K, K)
        ref = lambda v, w, b, a: nr.lepe2d_ref(v, w, b, a, pl, bl)
        hip = lambda v, w, b, a: mhla_amd.lepe2d(v, w, b, pl, bl, add=a)
    else:
        N, wshape = geom[0] * geom[1] * geom[2], (3, 3, 3)
        ref = lambda v, w, b, a: nr.lepe3d_ref(v, w, b, a, geom)
        hip = lambda v, w, b, a: mhla_amd.lepe3d(v, w, b, geom, add=a)
    v, w, bias, add, dy = _lepe_inputs(B, N, C, wshape, dtype, 1000 * C + 10 * N + seed)
    rv, rw, rb, ra = _leaf(v), _leaf(w), _leaf(bias), _leaf(add)
    want = ref(rv, rw, rb, ra)
    want.backward(dy.double())
    buf, sl = _embed(v, view)
    wd, bd, ad = _dev(w), _dev(bias), _dev(add)
    dyd = dy.to(DEV)
    if view != "packed":   # the upstream gradient as the same kind of view: the input-gradient launch sees it too
        dyd = _embed(dy, view)[0].detach()[sl]
    out = []
    poison()
    ran = launches(lambda: out.append(hip(buf[sl], wd, bd, ad)))
    got = out[0]
    assert got.dtype == dtype
    poison()
    ran_b = launches(lambda: got.backward(dyd))
    if expect:
        assert expect in ran and expect in ran_b, (expect, ran, ran_b)
        other = {"k_lepe2d": "k_lepe2d_run4", "k_lepe2d_run4": "k_lepe2d"}.get(expect)
        assert other not in ran and other not in ran_b, (expect, ran, ran_b)
    tag = f"{geom} C={C} B={B} {view}"
    check(f"y {tag}", got, want.detach(), TOL[dtype])
    check(f"dv {tag}", buf.grad[sl], rv.grad, TOL[dtype])
    rest = buf.grad.clone()
    rest[sl] = 0
    assert float(rest.abs().max()) == 0.0
    check(f"dw {tag}", wd.grad, rw.grad, _f32tol(dtype))
    check(f"dbias {tag}", bd.grad, rb.grad, _f32tol(dtype))
    assert torch.equal(ad.grad, dyd.contiguous())
    return (v, w, bias, add, dy), wd.grad, bd.grad


LEPE2D_RUN4 = [(1, 4), (3, 4), (2, 8)]
LEPE2D_FALLBACK = [(2, 6), (2, 7), (1, 1)]


@pytest.mark.parametrize("dtype", [BF16, F16], ids=_name)
@pytest.mark.parametrize("C", [8, 264])
@pytest.mark.parametrize("pl,bl", LEPE2D_RUN4 + LEPE2D_FALLBACK)
def test_lepe2d_3x3_16bit_dispatch(pl, bl, C, dtype):
    """Runs of four tokens (block_len % 4 == 0) and the per-token kernel (block_len 6, 7, 1); C = 264: past one workgroup of
    the weight gradient (256 channels) with a tail."""
    _lepe_case("2d", (3, pl, bl), C, dtype, expect="k_lepe2d_run4" if bl % 4 == 0 else "k_lepe2d")


@pytest.mark.parametrize("pl,bl,C", [(3, 4, 8), (2, 7, 264)])
def test_lepe2d_3x3_fp32(pl, bl, C):
    """fp32 tensors never take the runs of four: the per-token kernel and the 8-channel weight gradient in fp32."""
    _lepe_case("2d", (3, pl, bl), C, F32, expect="k_lepe2d")


@pytest.mark.parametrize("view", ["pad4", "off4"])
def test_lepe2d_alignment_fallbacks(view):
    """block_len % 4 == 0 but rows that are only 8-byte aligned (row stride 4 mod 8 elements; base 8 bytes off): the per-token
    kernel, in the forward and -- with the upstream gradient laid out the same way -- in the input gradient."""
    _lepe_case("2d", (3, 3, 4), 8, BF16, view=view, expect="k_lepe2d")


@pytest.mark.parametrize("C", [8, 136])
@pytest.mark.parametrize("pl,bl,dtype", [(2, 7, F32), (3, 4, BF16), (1, 2, F16)], ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_lepe2d_5x5(pl, bl, dtype, C):
    """K = 5: always the per-token kernel; C = 136: past one workgroup of its weight gradient (128 channels) with a tail."""
    _lepe_case("2d", (5, pl, bl), C, dtype, expect="k_lepe2d")


def test_lepe2d_weight_gradient_is_deterministic():
    a = _lepe_case("2d", (3, 3, 4), 264, BF16)
    b = _lepe_case("2d", (3, 3, 4), 264, BF16)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def _nonfinite_case(kind, geom, C, dtype, marks, expect=None):
    """One token of v is inf, another NaN (`marks`: their spatial coordinates; the first at a corner, the second on an edge), and
    the same for dy in the backward.  Every output whose window holds no marked token is bit-identical to the run without the
    marks -- a filler row that enters with weight zero by multiplication instead of a select would leak -- and the others are
    +inf / -inf / NaN exactly where a tap-by-tap evaluation of the convolution says."""
    import mhla_amd
    if kind == "2d":
        K, pl, bl = geom
        side = pl * bl
        N, wshape, space = side * side, (K, K), (side, side)
        hip = lambda v, w: mhla_amd.lepe2d(v, w, None, pl, bl)
        to_sp = lambda t: nr.blocks_to_image(t, pl, bl)
        from_sp = lambda t: nr.image_to_blocks(t, pl, bl)
    else:
        K = 3
        N, wshape, space = geom[0] * geom[1] * geom[2], (3, 3, 3), tuple(geom)
        hip = lambda v, w: mhla_amd.lepe3d(v, w, None, geom)
        to_sp = lambda t: nr.raster_to_video(t, geom)
        from_sp = nr.video_to_raster
    B = 2
    v, w, _, _, dy = _lepe_inputs(B, N, C, wshape, dtype, 77 + C)

    def mark(t):
        sp = to_sp(t.clone())
        sp[(0, slice(None)) + tuple(marks[0])] = float("inf")
        sp[(1, slice(None)) + tuple(marks[1])] = float("inf")
        sp[(0, slice(None)) + tuple(marks[1])] = NAN
        return from_sp(sp).contiguous()

    vm, dym = mark(v), mark(dy)
    touched = torch.zeros(B, 1, *space)
    touched[(0, 0) + tuple(marks[0])] = touched[(0, 0) + tuple(marks[1])] = touched[(1, 0) + tuple(marks[1])] = 1.0
    pool = torch.nn.functional.max_pool2d if kind == "2d" else torch.nn.functional.max_pool3d
    touched = from_sp(pool(touched, K, 1, K // 2))[:, :, 0] > 0                         # [B, N]: a marked token inside the window
    assert 0 < int(touched.sum()) < touched.numel() // 2
    wd = w.to(DEV)
    res = {}
    for name, vv, dd in (("clean", v, dy), ("marked", vm, dym)):
        vd = _dev(vv)
        poison()
        ran = launches(lambda: res.__setitem__(name + " y", hip(vd, wd)))
        poison()
        ran_b = launches(lambda: res[name + " y"].backward(dd.to(DEV)))
        res[name + " dv"] = vd.grad
        if expect:
            assert expect in ran and expect in ran_b, (ran, ran_b)
    want_y = from_sp(_conv_by_taps(to_sp(vm.double()), w.double()))
    want_dv = from_sp(_conv_by_taps(to_sp(dym.double()), w.double().flip(*range(2, w.dim()))))
    for q, want in (("y", want_y), ("dv", want_dv)):
        clean, marked = res["clean " + q].detach().cpu(), res["marked " + q].detach().cpu()
        assert bool(torch.isfinite(clean).all())
        assert torch.equal(marked[~touched], clean[~touched]), f"{q}: an inf / NaN token reached outputs outside its window"
        assert not bool(torch.isfinite(want[touched]).any())
        assert _same_class(marked, want), f"{q}: inf / NaN pattern differs from the convolution's"


@pytest.mark.parametrize("pl,bl,K,dtype,expect", [(3, 4, 3, BF16, "k_lepe2d_run4"), (2, 6, 3, BF16, "k_lepe2d"), (2, 7, 5, F32, "k_lepe2d")],
                         ids=["run4", "fallback", "5x5"])
def test_lepe2d_non_finite_values_stay_inside_their_window(pl, bl, K, dtype, expect):
    side = pl * bl
    # (0, 0): the first token of a run at the top edge; (side - 1, bl): the first token of a run at the bottom edge
    _nonfinite_case("2d", (K, pl, bl), 16, dtype, marks=[(0, 0), (side - 1, bl)], expect=expect)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=_name)
@pytest.mark.parametrize("C", [8, 136])
@pytest.mark.parametrize("grid", [(1, 1, 1), (1, 1, 5), (2, 9, 11), (3, 4, 2)], ids=lambda g: "x".join(map(str, g)))
def test_lepe3d_grids(grid, C, dtype, B):
    """A single token, a line, planes that no power of two divides, and a small box; B N below the 128 slices of the weight
    gradient (empty slices), not a multiple of them, and (see below) beyond 8 tokens per slice."""
    _lepe_case("3d", grid, C, dtype, B=B, expect="k_lepe3d")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
def test_lepe3d_more_than_eight_tokens_per_weight_gradient_slice(dtype):
    """B N = 6 x 198 = 1188 > 8 x 128: every token lane of a slice walks more than one token."""
    _lepe_case("3d", (2, 9, 11), 136, dtype, B=6, expect="k_lepe3d")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
def test_lepe3d_non_finite_values_stay_inside_their_window(dtype):
    _nonfinite_case("3d", (3, 4, 5), 16, dtype, marks=[(0, 0, 0), (2, 2, 4)], expect="k_lepe3d")
