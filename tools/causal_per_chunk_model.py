#!/usr/bin/env python3
"""Per-chunk error of the h16 chunk-summary storage format of the causal operator, from an fp64 model (CPU only).

tests/gpu_util.causal_fp64(..., h16=True) stores S, P, dP and dS as DESIGN.md section 3e describes the format (fp16 payload x one
power-of-two multiplier per 16-row strip of a 64 x 64 chunk tile) and computes everything else in fp64.  This prints, for the six
shapes the per-chunk tolerance of the default arithmetic is derived from, the largest error of a chunk relative to that chunk's
own maximum and the error relative to the whole tensor's maximum, against the fp64 operator on the same bf16-rounded inputs.
The maximum of the per-chunk column is tests/gpu_util.H16_CHUNK_MODEL_ERR.

    python tools/causal_per_chunk_model.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from gpu_util import causal_fp64, chunk_errors  # noqa: E402
from test_gpu_causal import causal_inputs  # noqa: E402

SHAPES = [(321, 64, 64), (449, 128, 256), (1000, 128, 256), (2100, 256, 256), (8192, 64, 64), (8200, 192, 192)]


def main():
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
