"""GPU: the block-mix token kernels that multiply a token row against the PAYLOAD of an h16 summary (split.hpp sp_payop: k_sp_bwd_dq's dO
rows, the row dots of k_sp_state<1>) -- the row travels as an fp16 operand scaled by a power of two of its own (common.hpp tok16_operands),
the summary's multiplier, the row's scale and 1 / n meet the accumulator in fp32.  Forward + backward through mhla_blockmix against the CPU
oracle at the suite's tolerances (gpu_util.bm_tols), on the shapes at which the kernels take another path and on token rows built to break a
missing or wrong row scale.

Row extremes used.  Two things bound what can be asked.  The oracle must stay finite and agree with its own fp64 evaluation (every case
asserts that for its inputs, and test_oracle_is_sound_on_the_extreme_rows does nothing else): with q, k, v and dO of one token all x 2^30, dW
overflows fp32 without the normaliser, and a token whose key is 2^30 above the others takes every output to its own value row, so that dW is
the cancelled remainder of two equal terms and the fp32 oracle misses it by several times its maximum.  And the inputs must not ask more of
the 11-bit summary format than it has: an fp64 model of the format alone (tools/sim_h16.py, run on these inputs) stays at 2.5e-4 (out),
6.1e-4 (dq), 4.2e-4 (dk), 2.3e-4 (dv), 3.6e-4 (dW) of a result's maximum on the rows below -- what it shows on ordinarily drawn inputs
(2.8e-4, 4.6e-4, 5.1e-4, 2.4e-4, 3.3e-4) -- but reaches 2.6e-3 (dW) and 1.7e-3 (dk) as soon as ONE token or a few features of a row dominate
a block, because a result then is a handful of rounded products with nothing to average over.  So:
  * bf16: a token whose q, k, v and dO are all below 2^-30 (x 2^-34); the large rows are a whole (batch, head) slice, q, k, v and dO x 2^24
    (2^30 scaled down until dW stays finite in fp32 without the normaliser, with two binades to spare) -- every token of it is "near 2^24",
    none dominates its block, and the maximum-normalised comparison then looks at that slice; a token whose features run over 2^33 within
    the row, downwards from its drawn size (x 2^-33 .. 2^0);
  * fp16 cannot hold 2^-30 or 2^30: the small token is x 2^-20 (fp16 subnormals), there is no large slice, and the spanning row runs over
    2^24 (x 2^-24 .. 2^0, the low end subnormal or zero);
  * both: one dO row and one v row of exact zeros.
No result may be inf or NaN anywhere."""
import functools

import pytest
import torch

from gpu_util import DEV, bm_tols, check, make_blockmix_inputs, oracle_blockmix, to_dev
from oracle import mhla_oracle as orc

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 4), (3, 1, 5)]   # (B, H, M)
DTYPES = [torch.bfloat16, torch.float16]
# the oracle in fp32 against itself in fp64, relative to a result's maximum: 1 % of the tightest bound the reference is used for here
# (1e-3); on ordinarily drawn inputs it is below 3e-6 on every shape of this file
ORACLE_SELF_TOL = 1e-5


def _extreme_rows(t, S, dtype):
    """q, k, v, dO with the rows of the module docstring; the tokens in different blocks and, at S = 40, one in the clamped partial tile."""
    q, k, v, do = (x.float().clone() for x in t)
    D = q.shape[-1]
    bf = dtype == torch.bfloat16
    small, zdo, zv, span = 1, 2 * S + 5, 2 * S + 6, 4 * S - 1
    ramp = torch.exp2(torch.linspace(-33 if bf else -24, 0, D).round())
    for x in (q, k, v, do):
        x[:, small] *= 2.0 ** (-34 if bf else -20)
        x[:, span] *= ramp
        if bf:
            x[-1, :, -1] *= 2.0 ** 24   # the last (batch, head) slice
    do[:, zdo] = 0
    v[:, zv] = 0
    out = [x.to(dtype) for x in (q, k, v, do)]
    if bf:
        assert all(x[0, small, 0].float().abs().max() < 2.0 ** -30 and x[-1, :, -1].float().abs().max() > 2.0 ** 24 for x in out)
    return out


@functools.lru_cache(maxsize=None)
def _problem(B, H, M, S, D, dtype, normalize, extreme, split=False, relu_eps=False):
    """Inputs and the oracle's results (computed once per problem, never modified); the oracle's fp32 / fp64 agreement asserted."""
    q, k, v, W, do, qd, kd = make_blockmix_inputs(B, H, M, S, D, dtype, 100 + S + D, "rand", split)
    if relu_eps:   # raw projections: the kernels apply relu(x) + eps themselves
        g = torch.Generator().manual_seed(5)
        q, k = torch.randn(q.shape, generator=g).to(dtype), torch.randn(k.shape, generator=g).to(dtype)
    if extreme:
        q, k, v, do = _extreme_rows((q, k, v, do), S, dtype)
    oq, ok = (torch.relu(q.float()) + 1e-6, torch.relu(k.float()) + 1e-6) if relu_eps else (q, k)
    want, wg = oracle_blockmix(oq, ok, v, W, do, qd, kd, 1e-6, normalize)
    d = lambda x: None if x is None else x.double()
    want64 = orc.blockmix_fwd(d(oq), d(ok), d(v), W.double(), 1e-6, d(qd), d(kd), normalize)
    wg64 = orc.blockmix_bwd(d(oq), d(ok), d(v), W.double(), d(do), 1e-6, d(qd), d(kd), normalize)
    for name, a, b in [("out", want, want64)] + [(n, wg[n], wg64[n]) for n in wg]:
        assert torch.isfinite(a).all(), f"oracle {name} is not finite"
        e = ((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()
        assert e < ORACLE_SELF_TOL, f"oracle {name}: fp32 and fp64 differ by {e:.2e} of the maximum"
    if relu_eps:   # the gradient w.r.t. the raw projections: masked where relu cut
        wg = dict(wg)
        wg["dq"] = wg["dq"] * (q.float() > 0)
        wg["dk"] = wg["dk"] * (k.float() > 0)
    return (q, k, v, W, do, qd, kd), want, wg


def _run(B, H, M, S, D, dtype, normalize=True, extreme=False, split=False, relu_eps=False, summaries="tf32"):
    import mhla_amd
    t, want, wg = _problem(B, H, M, S, D, dtype, normalize, extreme, split, relu_eps)
    otol, gtol, wtol = bm_tols(dtype, summaries)
    q, k, v, W, do, qd, kd = to_dev(*(None if x is None else x.clone() for x in t))
    leaves = [x.requires_grad_(True) for x in (q, k, v, W)] + ([x.requires_grad_(True) for x in (qd, kd)] if split else [])
    out = mhla_amd.mhla_blockmix(q, k, v, W, eps=1e-6, q_den=qd, k_den=kd, normalize=normalize, relu_eps=relu_eps, no_smalln=True,
                                 summaries=summaries)
    out.backward(do)
    torch.cuda.synchronize()
    names = ["dq", "dk", "dv", "dW"] + (["dq_den", "dk_den"] if split else [])
    got = {"out": out.detach(), **{n: x.grad for n, x in zip(names, leaves)}}
    for n, x in got.items():
        assert torch.isfinite(x).all(), f"{n} has {int((~torch.isfinite(x)).sum())} inf / NaN"
    tag = f"B H = {B * H}, M = {M}: "
    check(tag + "out", got["out"], want, otol)
    for n in names:
        check(tag + n, got[n], wg[n], wtol if n == "dW" else gtol)


@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "nonorm"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [32, 48, 64])
@pytest.mark.parametrize("S", [16, 40, 64, 80])
def test_payload_operand_kernels_against_the_oracle(S, D, dtype, normalize):
    """D = 32 / 48 / 64: two, three and four feature tiles, one and two reduction steps.  S = 16: waves without a tile; 40: a clamped partial
    tile; 64: the full one-tile form; 80: the loop kernels."""
    for B, H, M in SHAPES:
        _run(B, H, M, S, D, dtype, normalize)


@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "nonorm"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [32, 48, 64])
@pytest.mark.parametrize("S", [16, 40, 64, 80])
def test_row_scaling_on_extreme_token_rows(S, D, dtype, normalize):
    """The same shapes with the extreme rows of the module docstring: nothing inf or NaN, and the oracle comparison holds."""
    for B, H, M in SHAPES:
        _run(B, H, M, S, D, dtype, normalize, extreme=True)


@pytest.mark.parametrize("kw", [{"relu_eps": True}, {"split": True}, {"summaries": "split"}], ids=["relu_prologue", "rotated_pair", "summaries_split"])
def test_variants_that_keep_the_hi_lo_form(kw):
    """The relu prologue, a rotated numerator pair beside the plain normaliser pair (how 16-bit tensors carry rope: rotated in the host) and
    the >= 16-bit summaries still run and pass."""
    _run(3, 1, 5, 40, 64, torch.bfloat16, **kw)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_oracle_is_sound_on_the_extreme_rows(dtype):
    """(needs no kernel: the reference the extreme-row cases compare with is finite and agrees with its fp64 self)"""
    for normalize in (True, False):
        _problem(1, 2, 4, 40, 64, dtype, normalize, True)
