#!/usr/bin/env python3
"""Per-chunk error of the h16 chunk-summary storage format of the causal operator, from an fp64 model (CPU only).

tests/gpu_util.causal_fp64(..., h16=True) stores S, P, dP and dS as DESIGN.md section 3e describes the format (fp16 payload x one
power-of-two multiplier per 16-row strip of a 64 x 64 chunk tile) and computes everything else in fp64.  This prints, for the six
shapes the per-chunk tolerance of the default arithmetic is derived from, the largest error of a chunk relative to that chunk's
own maximum and the error relative to the whole tensor's maximum, against the fp64 operator on the same bf16-rounded inputs.
The maximum of the per-chunk column is tests/gpu_util.H16_CHUNK_MODEL_ERR.

    python tools/causal_per_chunk_model.py
    python tools/causal_per_chunk_model.py --walk   # instead: the inputs of tests/test_gpu_causal_walk.py (profiles/causal_walk_parity.md)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from gpu_util import causal_fp64, chunk_errors  # noqa: E402
from test_gpu_causal import causal_inputs  # noqa: E402

SHAPES = [(321, 64, 64), (449, 128, 256), (1000, 128, 256), (2100, 256, 256), (8192, 64, 64), (8200, 192, 192)]


def pooled_chunk_errors(q, k, v, mix, do, pieces, chunk=64):
    """{name: worst per-chunk error} of the model over `pieces` -- (batch row, first token, behind-last token) slices, each the
    operator on its own -- with every chunk index pooled over the pieces, the normalisation of gpu_util.check_chunks on the whole
    batch (max over the pieces of |model - fp64| by the max over the pieces of |fp64|); and the figure per piece for the packed
    case, where check_chunks runs per sequence."""
    names = ("out", "dq", "dk", "dv")
    err, ref, alone = {n: {} for n in names}, {n: {} for n in names}, {n: 0.0 for n in names}
    for b, t0, t1 in pieces:
        args = [t[b:b + 1, t0:t1] for t in (q, k, v)] + [mix, do[b:b + 1, t0:t1]]
        f64, mod = causal_fp64(*args), causal_fp64(*args, h16=True)
        for n in names:
            alone[n] = max(alone[n], chunk_errors(mod[n], f64[n])[0])
            for c, (a, w) in enumerate(zip(mod[n].split(chunk, 1), f64[n].split(chunk, 1))):
                err[n][c] = max(err[n].get(c, 0.0), (a - w).abs().max().item())
                ref[n][c] = max(ref[n].get(c, 0.0), w.abs().max().item())
    return {n: max(err[n][c] / ref[n][c] for c in err[n] if ref[n][c] > 0) for n in names}, alone


def walk_shapes():
    """The inputs of tests/test_gpu_causal_walk.py: T = 1157, H = 11, B = 3 / 5 / 8, seed T + K; the pack at H = 32, seed 66."""
    from test_gpu_causal_walk import CONTROL, H, N_CHUNKS, PACK_CHUNKS, PACK_H, T, WALKS, pack_cu
    worst = 0.0
    print("| B, T, H, K, V | " + " | ".join(f"{n} per-chunk" for n in ("out", "dq", "dk", "dv")) + " |")
    print("|---|---|---|---|---|")
    shapes = [(B, K, V) for K, V in ((64, 64), (64, 128), (128, 128), (192, 192)) for B, _, _ in WALKS] + [(CONTROL[0], CONTROL[1], CONTROL[2])]
    for B, K, V in shapes:
        args = causal_inputs(B, T, H, K, V, N_CHUNKS, torch.bfloat16, seed=T + K)
        per, _ = pooled_chunk_errors(*args, [(b, 0, T) for b in range(B)])
        worst = max(worst, *per.values())
        print(f"| {B}, {T}, {H}, {K}, {V} | " + " | ".join(f"{per[n]:.2e}" for n in ("out", "dq", "dk", "dv")) + " |", flush=True)
    cu, _ = pack_cu()
    args = causal_inputs(1, cu[-1], PACK_H, 64, 64, 4, torch.bfloat16, seed=PACK_CHUNKS)
    _, alone = pooled_chunk_errors(*args, [(0, a, b) for a, b in zip(cu, cu[1:])])
    worst = max(worst, *alone.values())
    print(f"| pack of {len(cu) - 1} sequences ({PACK_CHUNKS} chunks), {cu[-1]}, {PACK_H}, 64, 64: per sequence | "
          + " | ".join(f"{alone[n]:.2e}" for n in ("out", "dq", "dk", "dv")) + " |")
    print(f"maximum per-chunk error: {worst:.3e}")


def main():
    if "--walk" in sys.argv[1:]:
        return walk_shapes()
    worst = 0.0
    print("| T, K, V | " + " | ".join(f"{n} per-chunk / global" for n in ("out", "dq", "dk", "dv")) + " |")
    print("|---|---|---|---|---|")
    for T, K, V in SHAPES:
        args = causal_inputs(1, T, 2, K, V, max(4, (T + 63) // 64), torch.bfloat16, seed=T + K)
        ref, mod = causal_fp64(*args), causal_fp64(*args, h16=True)
        cells = []
        for n in ("out", "dq", "dk", "dv"):
            per, glob = chunk_errors(mod[n], ref[n])
            worst = max(worst, per)
            cells.append(f"{per:.2e} / {glob:.2e}")
        print(f"| {T}, {K}, {V} | " + " | ".join(cells) + " |", flush=True)
    print(f"maximum per-chunk error: {worst:.3e}")


if __name__ == "__main__":
    main()
