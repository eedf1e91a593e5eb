"""GPU parity of the block-mixing operator with what its other tests never feed it: a mixing matrix with NEGATIVE entries ("signed"), one
with an all-zero row and an all-zero column ("sparse"), and an eps that is a quarter of the normaliser instead of 1e-6 of it -- at one
shape per kernel family, summary format and mixing / dW kernel (gpu_util.MIX_CASES lists what each row reaches;
tests/test_blockmix_weights_cpu.py asserts it from the dispatcher's description, shows the inputs to be well conditioned, and shows that
these checks reject an operator with a dropped, stale or one-sided eps, with |W| for W, or with a wrong all-zero row).

Every case is one forward + backward through mhla_amd.mhla_blockmix against the oracle (test_gpu_blockmix.run_case: NaN-poisoned memory
before both): check() on out, dq, dk, dv (dq_den, dk_den), dW in two pieces, everything finite, exact zeros where W's zero row / column
makes the reference exactly zero, and block by block (check_chunks, chunk = S) on the rows whose arithmetic keeps >= 16 bits.
Tolerances: gpu_util.bm_tols, but (1 + K kappa) u for summaries="bf16" with a signed W (gpu_util.bm_tols_signed; derived there)."""
import pytest
import torch

from gpu_util import (DEV, DW_TOL, MIX_CASE, MIX_CASES, MIX_KINDS, MIX_RELU_CASES, ROPE_CASES, TOL, bm_tols, check, check_dw_rows, make_mix_case,
                      make_mix_relu_case, make_mix_rope_case, mix_case_per_block, mix_case_seed, mix_extra_checks, mix_relu_reference, poison,
                      rope_blockmix_fp64)
from test_gpu_blockmix import run_case

pytestmark = pytest.mark.gpu

NAMES = ("out", "dq", "dk", "dv", "dW", "dq_den", "dk_den")


def _run(cid, kind, eps=None, normalize=True):
    """A MIX_CASES row with a W of `kind` through run_case; eps: the visible one unless given."""
    case = MIX_CASE[cid]
    _, dtype, B, H, M, S, D, opt, _ = case
    t = make_mix_case(case, kind, eps)   # (W, the gather map and eps; run_case draws the same q, k, v, dO from the same seed)
    flags = {k: v for k, v in opt.items() if k in ("no_smalln", "force_generic")}
    return run_case(B, H, M, S, D, dtype, normalize=normalize, split=opt.get("split", False) and normalize, w="rand", idx=t["idx"],
                    seed=mix_case_seed(case), summaries=opt.get("summaries", "tf32"), W=t["W"], eps=t["eps"], per_block=mix_case_per_block(case), **flags)


def _same(a, b, what):
    for name in NAMES:
        if name in a:
            assert torch.equal(a[name], b[name]), f"{name}: {what}"


@pytest.mark.parametrize("kind", MIX_KINDS)
@pytest.mark.parametrize("cid", [c[0] for c in MIX_CASES])
def test_signed_and_sparse_w_with_a_visible_eps(cid, kind):
    """Every family applies eps itself, the h16 mixing kernels size a row's multiplier from |w| and rescale the weights into fp16
    pairs, and an all-zero row (n = eps exactly, multiplier bound 0) or column (nothing to store but zeros) is where a 0 / 0, an
    unset multiplier or a skipped store would show.  No path needs an exception from the exact zeros: a zero weight multiplies finite
    summaries in every mixing kernel and in the score tiles of the small-sequence kernels, and 0 x (1 / n) = 0."""
    _run(cid, kind)


@pytest.mark.parametrize("cid", ["D1", "C1", "A1", "G1"])
def test_without_the_normaliser_eps_changes_nothing(cid):
    """normalize=False with weights uniform in [-1, 1] and eps = 1: the reference ignores eps, and so must the kernels -- bit for bit
    the results of the same call with eps = 1e-6 (h16, fast path, small-sequence and fp32-word kernels)."""
    a = _run(cid, "signed_full", eps=1.0, normalize=False)
    b = _run(cid, "signed_full", eps=1e-6, normalize=False)
    _same(a, b, "depends on eps without a normaliser")


@pytest.mark.parametrize("kind", MIX_KINDS)
@pytest.mark.parametrize("case", MIX_RELU_CASES, ids=lambda c: c[0])
def test_relu_prologue_adds_the_eps_of_the_call(case, kind):
    """relu(x) + eps inside the kernels with eps = 0.25 on raw randn q, k (the same number is the normaliser's): against the oracle on
    relu(x) + eps, the gradients masked by x > 0.

    The bf16 rows are what found that the split-operand kernels took a bf16 tensor's token operands to BE their bf16 hi part also under
    the prologue, where relu(x) + 0.25 is an fp32 value: dq sat 1.7e-3 .. 2.6e-3 beyond the final rounding (bound 1e-3) at R2 and R3, the
    single-bf16 class of arithmetic, reaching dq through dn -> dz -> dz ksum.  k_sp_state, k_sp_out and k_sp_bwd_dkv now have a variant
    that keeps the lo part (StateVar / OutVar / DkvVar `.lo`, picked by the launch for bf16 tensors with MHLA_FLAG_RELU_EPS): 2.8e-4 .. 4.0e-4."""
    import mhla_amd
    _, dtype, B, H, M, S, D, opt, _ = case
    t = make_mix_relu_case(case, kind)
    want, wg = mix_relu_reference(t)
    summaries = opt.get("summaries", "tf32")
    tols = bm_tols(dtype, summaries)
    leaves = [t[n].to(DEV).requires_grad_(True) for n in ("q", "k", "v", "W")]
    poison()
    out = mhla_amd.mhla_blockmix(*leaves, eps=t["eps"], relu_eps=True, summaries=summaries)
    poison()
    out.backward(t["do"].to(DEV))
    torch.cuda.synchronize()
    got = dict(zip(("out", "dq", "dk", "dv", "dW"), [out.detach()] + [x.grad for x in leaves]))
    wg = dict(wg, out=want)
    for name in ("out", "dq", "dk", "dv"):
        assert got[name].dtype == dtype
        check(name, got[name], wg[name], tols[0] if name == "out" else tols[1])
    check_dw_rows(got["dW"], wg["dW"], t["W"], tols[2])
    mix_extra_checks(got, wg, t["W"], S, tols, mix_case_per_block(case))


@pytest.mark.parametrize("cid,python_nodes", [("D1", False), ("F1", False), ("G2", False), ("D1", True)])
def test_recomputed_state_takes_the_eps_of_the_call(cid, python_nodes, monkeypatch):
    """The backward is handed eps a second time: with the forward's kept 1 / n and when it recomputes the summaries and the normaliser
    (KEEP_STATE_LIMIT_BYTES = 0) -- both against the reference with a signed W and the visible eps, bit-identical to each other; h16 also
    through the Python autograd nodes."""
    from mhla_amd import ops
    if python_nodes:
        monkeypatch.setattr(ops, "_native_nodes", lambda: False)
    res = []
    for limit in (1 << 30, 0):
        monkeypatch.setattr(ops, "KEEP_STATE_LIMIT_BYTES", limit)
        res.append(_run(cid, "signed"))
    _same(res[0], res[1], "kept and recomputed state differ")


@pytest.mark.parametrize("n", [0, 5], ids=["rope0", "rope5"])
def test_rotary_operator_with_a_signed_w_and_a_visible_eps(n):
    """mhla_blockmix_rope (its own entry points hand eps to k_sp_state<rope>, the mixing and both token kernels) against the fp64
    operator at the fp32 tolerances."""
    import mhla_amd
    case = ROPE_CASES[n]
    (q, k, v, W, do, cos, sin, perm), eps = make_mix_rope_case(case)
    want = rope_blockmix_fp64(q, k, v, W, do, cos, sin, perm, case[5], eps=eps)
    t = [x.to(DEV).requires_grad_(True) for x in (q, k, v, W)]
    poison()
    out = mhla_amd.mhla_blockmix_rope(*t, cos.to(DEV), sin.to(DEV), eps=eps, normalize=case[5], block_index=None if perm is None else perm.to(DEV))
    poison()
    out.backward(do.to(DEV))
    torch.cuda.synchronize()
    for name, g, w in zip(("out", "dq", "dk", "dv"), [out.detach()] + [x.grad for x in t[:3]], want):
        check(name, g, w, TOL[torch.float32])
    check("dW", t[3].grad, want[4], DW_TOL[torch.float32])


@pytest.mark.parametrize("cid", ["D1", "C1"])
def test_second_call_of_a_shape_takes_its_own_eps(cid):
    """Plans and workspaces are cached per shape and flags, not per eps: the same shape first with eps = 1e-6, then with the visible
    one -- each against its own reference."""
    _run(cid, "signed", eps=1e-6)
    _run(cid, "signed")
