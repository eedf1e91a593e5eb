"""The block-mix cases with a signed / sparse mixing matrix and a visible eps (gpu_util.MIX_CASES, MIX_RELU_CASES), proved without a GPU:
every row reaches the kernels it names (mhla_amd.describe_dispatch), its inputs are well conditioned (conditions on the fp64 reference,
not measurements of a kernel), the fp32 oracle the GPU test compares with is within a tenth of the tolerance of fp64, and the checks of
tests/test_gpu_blockmix_weights.py REJECT the results of an operator that

 (a) uses eps = 1e-6 everywhere,
 (b) uses it in the backward only (dP = dO / n and dn = -(dO . O) / n with an n that lacks eps),
 (c) mixes with |W| ("signed" only),
 (d) adds 1e-6 in the relu prologue while the normaliser keeps eps (relu rows),
 (e) divides the all-zero row of a "sparse" W by n - eps + 1e-6 (the forward stays exactly 0; dW's zero row does not),

each evaluated in fp64 and rounded to the result's dtype -- which is what shows that the GPU tests can fail.  Mutant (e) changes dW
alone: the row's G is exactly 0, so dq = dP G^T + dz ksum keeps its value whatever dP is, and W's zero row hands nothing to dKV or dz."""
import functools

import pytest
import torch

from conftest import rel_err
from gpu_util import (MIX_CASE, MIX_CASES, MIX_KINDS, MIX_RELU_CASES, OBSERVED, ROPE_CASES, TOL, bm_tols, bm_tols_signed, check, check_chunks,
                      check_dw_rows, make_mix_case, make_mix_relu_case, make_mix_rope_case, make_mix_weights, mix_case_per_block,
                      mix_case_reference, mix_conditioning, mix_extra_checks, mix_relu_reference, rope_blockmix_fp64, rope_rotate, visible_eps,
                      zero_rows_and_columns)
from oracle import mhla_oracle as orc

ALL = [(c, kind) for c in MIX_CASES for kind in MIX_KINDS]
RELU = [(c, kind) for c in MIX_RELU_CASES for kind in MIX_KINDS]
_ids = lambda p: f"{p[0][0]}-{p[1]}"
TOKEN = ("out", "dq", "dk", "dv", "dq_den", "dk_den")


@functools.lru_cache(maxsize=None)
def _case(cid, kind):
    """(tensors, fp64 reference, fp32 oracle as the GPU test computes it, conditioning, tolerances) of a row; the results as name -> tensor."""
    relu = cid.startswith("R")
    case = next(c for c in MIX_RELU_CASES if c[0] == cid) if relu else MIX_CASE[cid]
    t = (make_mix_relu_case if relu else make_mix_case)(case, kind)
    ref = mix_relu_reference if relu else mix_case_reference
    r64, r32 = (_named(*ref(t, dtype=dt)) for dt in (torch.float64, torch.float32))
    pos = lambda x: torch.relu(x.double()) + t["eps"] if relu else x
    cond = mix_conditioning(pos(t["q"]), pos(t["k"]), t["v"], t["W"], t["do"], t["eps"], t["qd"], t["kd"])
    summ = case[7].get("summaries", "tf32")
    tols = bm_tols_signed(case[1], summ, cond["kappa_n"]) if kind == "signed" else bm_tols(case[1], summ)
    return case, t, r64, r32, cond, tols


def _named(out, grads):
    return dict(grads, out=out)


def _tol(name, tols):
    return tols[0] if name == "out" else tols[2] if name == "dW" else tols[1]


def _closed_form(t, W=None, eps=None, n_bwd=lambda n: n):
    """The oracle's forward and its closed-form backward in fp64, with the normaliser the BACKWARD divides by as a
    function of the forward's: the identity gives orc.blockmix_bwd (asserted below), anything else a mutant."""
    f = lambda x: None if x is None else x.double()
    q, k, v, do, qd, kd = (f(t[n]) for n in ("q", "k", "v", "do", "qd", "kd"))
    W = f(t["W"] if W is None else W)
    eps = t["eps"] if eps is None else eps
    B, N, H, D = q.shape
    M = W.shape[0]
    out, aux = orc.blockmix_fwd(q, k, v, W, eps, qd, kd, True, return_aux=True)
    qb, kb, vb, dob, ob = (orc._to_blocks(x, M) for x in (q, k, v, do, out))
    n = n_bwd(aux["n"]).unsqueeze(-1)
    dP = dob / n
    dn = -(dob * ob).sum(-1, keepdim=True) / n
    dG = torch.matmul(qb.transpose(-2, -1), dP)
    dKV = torch.einsum("ij,bixy->bjxy", W, dG)
    dz = torch.einsum("ij,bixy->bjxy", W, dn)
    qdb = qb if qd is None else orc._to_blocks(qd, M)
    dq_num, dq_den = torch.matmul(dP, aux["g"].transpose(-2, -1)), dz * aux["ksum"].unsqueeze(-2)
    dk_num, dk_den = torch.matmul(vb, dKV.transpose(-2, -1)), (dz * qdb).sum(-2, keepdim=True).expand_as(kb)
    back = lambda x: orc._from_blocks(x.contiguous(), B, H)
    res = {"out": out, "dv": back(torch.matmul(kb, dKV)),
           "dW": torch.einsum("bixy,bjxy->ij", dG, aux["kv"]) + torch.einsum("bixy,bjxy->ij", dn, aux["z"].unsqueeze(-1))}
    if qd is None:
        res.update(dq=back(dq_num + dq_den), dk=back(dk_num + dk_den))
    else:
        res.update(dq=back(dq_num), dk=back(dk_num), dq_den=back(dq_den), dk_den=back(dk_den))
    return res


def _rejected(name, got, want, W, tol, S, per_block):
    """The GPU test's checks of one tensor, applied to `got`: True if the global one raises (and, where the row has it, the per-block one
    too -- each alone must catch the mutant)."""
    n0 = len(OBSERVED)

    def raises(fn):
        try:
            fn()
        except AssertionError:
            return True
        return False
    try:
        if name == "dW":
            return raises(lambda: check_dw_rows(got, want, W, tol))
        glob = raises(lambda: check(name, got, want, tol))
        return glob and (not per_block or raises(lambda: check_chunks(name, got, want, tol, chunk=S)))
    finally:
        del OBSERVED[n0:]   # (planted errors are no parity observations)


def _assert_rejected(case, t, r32, tols, mutant, names, what):
    for name in names:
        if name not in r32:
            continue
        got = mutant[name].to(torch.float32 if name == "dW" else case[1])
        assert _rejected(name, got, r32[name], t["W"], _tol(name, tols), case[5], mix_case_per_block(case)), f"{what}: {name} passes the checks"


@pytest.mark.parametrize("case", MIX_CASES + MIX_RELU_CASES, ids=lambda c: c[0])
def test_each_row_reaches_the_kernels_it_names(case):
    import mhla_amd
    from mhla_amd import ops
    cid, dtype, B, H, M, S, D, opt, (family, fmt, fwd, bwd) = case
    flags = {k: v for k, v in opt.items() if k in ("summaries", "split", "no_smalln", "force_generic")}
    wide = D > 128
    if wide:   # ops._blockmix_wide_head: un-normalised calls on slices of this width
        assert cid == "K1" and ops._wide_head_chunk(D) == 72
        D = 72
    d = mhla_amd.describe_dispatch(B, H, M, S, D, dtype, relu_eps=cid.startswith("R"), **flags)
    assert d["family"].startswith(family) and d["summaries"].startswith(fmt), d["text"]
    assert all(n in d["fwd"] for n in fwd) and all(n in d["bwd"] for n in bwd), d["text"]
    if family == "split-operand" and not wide:   # the normaliser's product is its own launch exactly where the row says so
        assert ("k_wz<0>" in d["fwd"]) == ("k_wz<0>" in fwd), d["text"]
    if cid == "E2":   # the same blocks as E1 with too few (b, h) pairs for the recut kernel
        assert "k_sp_mixh2<0>" not in d["fwd"], d["text"]


def test_weight_kinds_are_what_they_say():
    for M in (3, 5, 16, 130):
        g = lambda: torch.Generator().manual_seed(M)
        W = make_mix_weights("signed", M, g())
        R = W - torch.eye(M)
        assert torch.equal(torch.diagonal(W), torch.ones(M)) and (W < 0).any() and torch.allclose(R.abs().sum(1), torch.full((M,), 0.5), atol=1e-6)
        W = make_mix_weights("sparse", M, g())
        zr, zc = zero_rows_and_columns(W)
        assert M // 2 in zr and M // 3 in zc and (W >= 0).all()
        keep = [i for i in range(M) if i != M // 2]
        assert ((W[keep] != 0).sum(1) >= 2).all() and ((W[keep] != 0).sum(1) <= 3).all()
        nz = W[(W != 0) & ~torch.eye(M, dtype=torch.bool)]
        assert (nz >= 0.25).all() and (nz <= 1).all()
        assert torch.equal(make_mix_weights("sparse", M, g()), W)   # seeded
        F = make_mix_weights("signed_full", M, g())
        assert F.min() < -0.5 and F.max() > 0.5 and F.abs().max() <= 1
    with pytest.raises(ValueError):
        make_mix_weights("rand", 4, g())


@pytest.mark.parametrize("p", ALL + RELU, ids=_ids)
def test_conditions_of_the_inputs_and_of_the_reference(p):
    """Conditions, not measurements: n > 0; "signed": kappa_n <= 4, kappa_G and kappa_dKV <= 2.5; "sparse": kappa_n == 1, the zero row's
    out and the zero column's dk, dv exactly 0 in the reference; the visible eps is a power of two a quarter of the median z; the fp32
    oracle within tol / 10 of fp64, over the tensor and block by block."""
    case, t, r64, r32, cond, tols = _case(p[0][0], p[1])
    cid, dtype, B, H, M, S, D = case[:7]
    print(f"{cid}-{p[1]}: eps {t['eps']:g} " + " ".join(f"{k} {v:.3g}" for k, v in cond.items()))
    assert cond["n_min"] > 0
    if p[1] == "signed":
        assert cond["kappa_n"] <= 4 and cond["kappa_G"] <= 2.5 and cond["kappa_dKV"] <= 2.5, cond
    else:
        assert abs(cond["kappa_n"] - 1) < 1e-12, cond
        zr, zc = zero_rows_and_columns(t["W"])
        blocks = lambda x: x.reshape(B, M, S, H, D)
        for r in (r64, r32):
            assert not blocks(r["out"])[:, zr].any()
            assert not any(blocks(r[n])[:, zc].any() for n in ("dk", "dv", "dk_den") if n in r)
            assert r["dW"][zr].abs().max() > r["dW"].abs().max() * 0.999   # (why dW is checked in two pieces)
    if not cid.startswith("R"):
        z = torch.matmul(orc._to_blocks((t["q"] if t["qd"] is None else t["qd"]).double(), M),
                         orc._to_blocks((t["k"] if t["kd"] is None else t["kd"]).double(), M).sum(-2).unsqueeze(-1))
        assert t["eps"] == visible_eps(t["q"], t["k"], M, t["qd"], t["kd"]) and 2 ** -0.5 <= 4 * t["eps"] / z.median().item() <= 2 ** 0.5
        assert torch.tensor(t["eps"]).frexp()[0] == 0.5
    for name, want in r64.items():
        tol = _tol(name, bm_tols(dtype, "split")) / 10   # (the tightest tolerance any row of this dtype is held to)
        got = r32[name]
        assert got.dtype == torch.float32 and want.dtype == torch.float64
        e = rel_err(got, want)
        assert e < tol, f"{name}: fp32 oracle {e:.2e} from fp64"
        if name in TOKEN:
            gb, wb = (x.double().reshape(B, M, S, H, D).transpose(1, 0).reshape(M, -1) for x in (got, want))
            den = wb.abs().amax(1)
            eb = ((gb - wb).abs().amax(1) / den.masked_fill(den == 0, 1.0)).max().item()
            assert eb < tol, f"{name}: fp32 oracle {eb:.2e} of a block's own maximum from fp64"


@pytest.mark.parametrize("p", ALL, ids=_ids)
def test_the_checks_reject_wrong_eps_wrong_sign_and_a_wrong_zero_row(p):
    case, t, r64, r32, cond, tols = _case(p[0][0], p[1])
    names = list(r64)
    grads = [n for n in names if n != "out"]
    same = _closed_form(t)
    for name in names:   # the knobbed closed form is the oracle's when no knob is turned ...
        assert rel_err(same[name], r64[name]) < 1e-12, name
    _assert_rejected(case, t, r32, tols, _closed_form(t, eps=1e-6), names, "(a) eps = 1e-6 everywhere")
    stale = _closed_form(t, n_bwd=lambda n: n - t["eps"] + 1e-6)
    assert torch.equal(stale["out"], r64["out"])
    _assert_rejected(case, t, r32, tols, stale, grads, "(b) eps = 1e-6 in the backward only")
    if p[1] == "signed":
        _assert_rejected(case, t, r32, tols, _closed_form(t, W=t["W"].abs()), names, "(c) |W|")
    else:
        zr, _ = zero_rows_and_columns(t["W"])

        def n_zero_row(n):
            n = n.clone()
            n[:, zr] = n[:, zr] - t["eps"] + 1e-6
            return n
        bad = _closed_form(t, n_bwd=n_zero_row)
        assert torch.equal(bad["out"], r64["out"]) and all(torch.equal(bad[n], r64[n]) for n in grads if n != "dW")
        n0 = len(OBSERVED)
        with pytest.raises(AssertionError, match="rows of W that are zero"):
            check_dw_rows(bad["dW"].float(), r32["dW"], t["W"], _tol("dW", tols))
        del OBSERVED[n0:]
    # ... and the untouched fp64 results, rounded to the result's dtype, pass every check the GPU test makes
    n0 = len(OBSERVED)
    got = {name: r64[name].to(torch.float32 if name == "dW" else case[1]) for name in names}
    for name in names:
        if name == "dW":
            check_dw_rows(got[name], r32[name], t["W"], _tol(name, tols))
        else:
            check(name, got[name], r32[name], _tol(name, tols))
    mix_extra_checks(got, r32, t["W"], case[5], tols, mix_case_per_block(case))
    del OBSERVED[n0:]


@pytest.mark.parametrize("p", RELU, ids=_ids)
def test_the_checks_reject_a_wrong_prologue_constant(p):
    case, t, r64, r32, cond, tols = _case(p[0][0], p[1])
    names = list(r64)
    _assert_rejected(case, t, r32, tols, _named(*mix_relu_reference(t, torch.float64, eps=1e-6)), names, "(a) eps = 1e-6 everywhere")
    _assert_rejected(case, t, r32, tols, _named(*mix_relu_reference(t, torch.float64, prologue=1e-6)), names, "(d) relu(x) + 1e-6, n keeps eps")
    if p[1] == "signed":
        bad = dict(t, W=t["W"].abs())
        _assert_rejected(case, t, r32, tols, _named(*mix_relu_reference(bad, torch.float64)), names, "(c) |W|")


@pytest.mark.parametrize("cid", ["D1", "C1"])
def test_conditions_hold_at_eps_1e_6_where_the_stale_eps_test_starts(cid):
    """The first call of the GPU module's stale-eps test: the same tensors and signed W with eps = 1e-6.  The normaliser stays positive;
    without eps in it kappa_n is a little larger than in the table's cases (4.1) -- it enters C1's bound through bm_tols_signed, as there."""
    t = make_mix_case(MIX_CASE[cid], "signed", eps=1e-6)
    cond = mix_conditioning(t["q"], t["k"], t["v"], t["W"], t["do"], t["eps"], t["qd"], t["kd"])
    assert cond["n_min"] > 0 and cond["kappa_n"] <= 4.5 and cond["kappa_G"] <= 2.5 and cond["kappa_dKV"] <= 2.5, cond


@pytest.mark.parametrize("n", [0, 5])
def test_conditions_of_the_rotary_cases(n):
    """ROPE_CASES[n] with a signed W and the visible eps of the un-rotated pair: the same conditions (the rotated pair feeds KV and the
    numerator), eps moves every result far outside the fp32 tolerance, and the reference in fp32 stays within a tenth of it."""
    case = ROPE_CASES[n]
    (q, k, v, W, do, cos, sin, perm), eps = make_mix_rope_case(case)
    rows = torch.arange(q.shape[1]) if perm is None else perm.long()
    bm = lambda x: x[:, rows]
    cond = mix_conditioning(bm(rope_rotate(q.double(), cos, sin)), bm(rope_rotate(k.double(), cos, sin)), bm(v), W, bm(do), eps, bm(q), bm(k))
    print(f"rope {n}: eps {eps:g} {cond}")
    assert cond["n_min"] > 0 and cond["kappa_n"] <= 4 and cond["kappa_G"] <= 2.5 and cond["kappa_dKV"] <= 2.5, cond
    r64 = rope_blockmix_fp64(q, k, v, W, do, cos, sin, perm, case[5], eps=eps)
    r32 = rope_blockmix_fp64(q, k, v, W, do, cos, sin, perm, case[5], eps=eps, dtype=torch.float32)
    stale = rope_blockmix_fp64(q, k, v, W, do, cos, sin, perm, case[5], eps=1e-6)
    for name, a, b, c in zip(("out", "dq", "dk", "dv", "dW"), r32, r64, stale):
        assert rel_err(a, b) < TOL[torch.float32] / 10, name
        assert rel_err(c, b) > 10 * TOL[torch.float32], name


@pytest.mark.parametrize("cid,kind", [("D5", "signed"), ("A3", "sparse"), ("G3", "sparse"), ("J2", "signed")])
def test_closed_form_backward_matches_autograd_at_the_visible_eps(cid, kind):
    """The oracle's hand-derived gradients against autograd through its forward, in fp64, with a signed W, a W with an empty row and
    column, a separate normaliser pair, and eps a quarter of the normaliser (tests/test_oracle_golden.py ties them at eps = 1e-6)."""
    case, t, r64, _, _, _ = _case(cid, kind)
    leaves = {n: t[n].double().requires_grad_(True) for n in ("q", "k", "v", "W", "qd", "kd") if t[n] is not None}
    out = orc.blockmix_fwd(leaves["q"], leaves["k"], leaves["v"], leaves["W"], t["eps"], leaves.get("qd"), leaves.get("kd"))
    (out * t["do"].double()).sum().backward()
    assert rel_err(out.detach(), r64["out"]) < 1e-12
    for leaf, name in (("q", "dq"), ("k", "dk"), ("v", "dv"), ("W", "dW"), ("qd", "dq_den"), ("kd", "dk_den")):
        if leaf in leaves:
            assert rel_err(leaves[leaf].grad, r64[name]) < 1e-10, name
