"""CPU: the per-chunk parity check (gpu_util.check_chunks) proved on the oracle's own numbers -- errors that the globally
normalised check() lets through, planted where the causal operator's magnitudes are small by construction (the last chunk of dk,
the first chunk of out), must raise; the untouched oracle tensors pass both.  And the fp64 model of the h16 summary format that
the per-chunk tolerance of the default arithmetic is derived from."""
import functools

import pytest
import torch

from gpu_util import (CAUSAL_CHUNK_TOL_H16, CAUSAL_TOL, H16_CHUNK_MODEL_ERR, OBSERVED, causal_fp64, check, check_chunks,
                      chunk_errors)
from oracle import mhla_oracle as orc
from test_gpu_causal import causal_inputs

TOL = 4.9e-3      # the bf16 tolerance of the global check, u + 1e-3


@functools.lru_cache(maxsize=None)
def _oracle(T, K, V, seed):
    q, k, v, mix, do = causal_inputs(1, T, 2, K, V, max(6, (T + 63) // 64), torch.float32, seed=seed)
    out = orc.causal_fwd(q, k, v, mix)
    return out, orc.causal_bwd(q, k, v, mix, do)


@pytest.mark.parametrize("T,K,V,seed", [(321, 64, 64, 385), (8200, 192, 192, 8392)])
def test_a_wrong_last_chunk_of_dk_passes_check_and_fails_check_chunks(T, K, V, seed):
    out, grads = _oracle(T, K, V, seed)
    dk = grads["dk"]
    for name, t in (("out", out), ("dq", grads["dq"]), ("dk", dk), ("dv", grads["dv"])):
        check(name, t.clone(), t, TOL)
        assert check_chunks(name, t.clone(), t, TOL) == 0.0
    last = 64 * ((T - 1) // 64)
    bad = dk.clone()
    bad[:, last:] *= 0.7
    check("dk", bad, dk, TOL)
    n0 = len(OBSERVED)
    with pytest.raises(AssertionError, match=f"dk: chunk {last // 64} of"):
        check_chunks("dk", bad, dk, TOL)
    rec = OBSERVED[n0]
    assert len(OBSERVED) == n0 + 1 and len(rec) == 7 and rec[1] == f"dk per-chunk (worst: {last // 64})" and rec[1].split(" ")[0] == "dk"
    assert abs(rec[3] - 0.3) < 1e-6 and rec[5] == TOL


def test_a_wrong_first_chunk_of_out_passes_check_and_fails_check_chunks():
    out, grads = _oracle(8192, 64, 64, 8256)
    check("out", out.clone(), out, TOL)
    check_chunks("out", out.clone(), out, TOL)
    check_chunks("dv", grads["dv"].clone(), grads["dv"], TOL)
    bad = out.clone()
    bad[:, :64] *= 0.95
    check("out", bad, out, TOL)
    with pytest.raises(AssertionError, match="out: chunk 0 of 128"):
        check_chunks("out", bad, out, TOL)


def test_an_all_zero_chunk_must_be_exactly_zero():
    out, _ = _oracle(321, 64, 64, 385)
    want = out.clone()
    want[:, 64:128] = 0.0
    got = want.clone()
    check_chunks("out", got, want, TOL)
    got[0, 100, 1, 3] = 1e-30
    check("out", got, want, TOL)
    with pytest.raises(AssertionError, match=r"chunks \[1\] must be exactly zero"):
        check_chunks("out", got, want, TOL)
    got[0, 100, 1, 3] = float("nan")
    with pytest.raises(AssertionError):
        check_chunks("out", got, want, TOL)


def test_rounding_rms_nan_and_other_dims():
    out, _ = _oracle(321, 64, 64, 385)
    # a bf16-rounded result costs u per element and nothing beyond it: inside u + 1e-3 in every chunk, the one-token tail included
    check_chunks("out", out.bfloat16(), out, CAUSAL_TOL[torch.bfloat16])
    with pytest.raises(AssertionError):
        check_chunks("out", out.bfloat16(), out, 2.0 ** -9)
    # the error beyond the final rounding: 3e-3 of one chunk's maximum on one element of it
    bad = out.clone()
    c = out[:, 128:192].abs().max().item()
    bad[0, 130, 0, 0] += 3e-3 * c
    with pytest.raises(AssertionError, match="out: chunk 2 of 6"):
        check_chunks("out", bad.bfloat16(), out, CAUSAL_TOL[torch.bfloat16])
    # noise of 0.4 % rms on a chunk whose largest single error stays inside the bound: the rms criterion
    noise = torch.randn(out[:, 192:256].shape, generator=torch.Generator().manual_seed(1)).sign() * 0.0045 * c
    bad = out.clone()
    bad[:, 192:256] = out[:, 192:256] + noise * (out[:, 192:256].abs().max() / c)
    with pytest.raises(AssertionError, match="rms ratio"):
        check_chunks("out", bad, out, TOL)
    bad = out.clone()
    bad[0, 320, 1, 5] = float("nan")
    with pytest.raises(AssertionError, match="out: chunk 5 of 6"):
        check_chunks("out", bad, out, TOL)
    # the token axis elsewhere, another chunk length
    t = out.permute(0, 2, 1, 3).contiguous()
    check_chunks("out", t.clone(), t, TOL, dim=2)
    bad = t.clone()
    bad[:, :, 320:] *= 0.9
    with pytest.raises(AssertionError, match="out: chunk 10 of 11"):
        check_chunks("out", bad, t, TOL, chunk=32, dim=2)
    with pytest.raises(AssertionError, match="shape"):
        check_chunks("out", out[:, :320], out, TOL)


def test_256_chunks_in_one_pass_agree_with_a_loop_over_the_chunks():
    """The pad-and-reshape form against check()'s own figures chunk by chunk, at 256 chunks with a ragged last one."""
    from conftest import rel_err, rms_ratio
    g = torch.Generator().manual_seed(0)
    T = 255 * 64 + 9
    want = torch.randn(2, T, 2, 16, generator=g) * torch.linspace(0.01, 3.0, T).view(1, T, 1, 1)
    got = (want * (1 + 2e-3 * torch.randn(2, T, 2, 16, generator=g))).bfloat16()
    n0 = len(OBSERVED)
    check_chunks("out", got, want, 0.05)
    _, name, dtype, e, r, tol, x = OBSERVED[n0]
    per = [(rel_err(a.float(), b), rms_ratio(a.float(), b)) for a, b in zip(got.split(64, 1), want.split(64, 1))]
    assert len(per) == 256 and dtype == "bfloat16" and tol == 0.05
    worst = max(range(256), key=lambda c: per[c][0])
    assert name == f"out per-chunk (worst: {worst})"
    assert abs(e - per[worst][0]) < 1e-12 and abs(r - max(p[1] for p in per)) < 1e-12 and 0 < x < e


@pytest.mark.parametrize("T,K,V", [(321, 64, 64), (449, 128, 256), (8192, 64, 64), (8200, 192, 192)])
def test_h16_model_stays_under_the_figure_the_bound_is_derived_from(T, K, V):
    """The fp64 model of the 2-byte summary format (four of the six shapes of tools/causal_per_chunk_model.py, the two long ones
    that set the figure among them): with the format off it IS the oracle; with it on, every chunk of every result stays within
    H16_CHUNK_MODEL_ERR of its own maximum -- which T = 8192 reaches to within 2 %, so the constant is the model's figure and
    not a looser one -- and the bound derived from it is the one written down."""
    args = causal_inputs(1, T, 2, K, V, max(4, (T + 63) // 64), torch.bfloat16, seed=T + K)
    ref, mod = causal_fp64(*args), causal_fp64(*args, h16=True)
    f = [t.float() for t in args]
    want = dict(orc.causal_bwd(*f), out=orc.causal_fwd(*f[:4]))
    worst = 0.0
    for n in ("out", "dq", "dk", "dv"):
        check_chunks(n, ref[n].float(), want[n], 2e-5)
        per, glob = chunk_errors(mod[n], ref[n])
        assert 5e-5 < glob <= per <= H16_CHUNK_MODEL_ERR, (n, per, glob)
        worst = max(worst, per)
    if T == 8192:
        assert worst > 0.98 * H16_CHUNK_MODEL_ERR, worst
    check("dmix", ref["dmix"].float(), want["dmix"][:ref["dmix"].shape[0], :ref["dmix"].shape[1]], 2e-5)
    assert CAUSAL_CHUNK_TOL_H16[torch.bfloat16] == 2.0 ** -8 + max(1e-3, 2 * H16_CHUNK_MODEL_ERR)
    # a non-default scale goes through the model like through the oracle
    s = causal_fp64(*args, scale=0.37)
    check_chunks("out", s["out"].float(), orc.causal_fwd(*f[:4], scale=0.37), 2e-5)
    check_chunks("dk", s["dk"].float(), orc.causal_bwd(*f, scale=0.37)["dk"], 2e-5)
