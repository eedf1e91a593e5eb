#!/usr/bin/env python
"""Where the host time of an eager operator call goes (cProfile over many un-synchronised fwd+bwd calls of the C3 shape):
python tools/host_overhead.py [iters] [--python-nodes] [--causal | --dit-core]
--python-nodes: the autograd nodes of ops.py (ops.USE_NATIVE_NODES = False) instead of the C++ ones, where those are built.
--causal: the same loop on mhla_causal (B = 2, T = 512, H = 2, K = 64, V = 128, bf16) instead of mhla_blockmix.
--dit-core: the same loop on mhla_dit_core at the DiT shape (packed qkv [32, 256, 3, 16, 72] bf16, M = 16, pieces_len = block_len = 4,
a 3 x 3 LePE weight with bias): the node has no C++ twin, so this is what the DiT module pays on every call."""
import argparse
import cProfile
import os
import pstats
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import mhla_amd  # noqa: E402
from mhla_amd import ops  # noqa: E402
from mhla_amd.weights import block_distance_weights  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("iters", nargs="?", type=int, default=300)
ap.add_argument("--python-nodes", action="store_true")
ap.add_argument("--causal", action="store_true")
ap.add_argument("--dit-core", action="store_true")
a = ap.parse_args()
iters = a.iters
if a.python_nodes:
    ops.USE_NATIVE_NODES = False
g = torch.Generator().manual_seed(0)
if a.causal:
    B, T, H, K, V = 2, 512, 2, 64, 128
    mk = lambda D: torch.randn(B, T, H, D, generator=g).to(torch.bfloat16).cuda().requires_grad_(True)
    q, k, v = mk(K), mk(K), mk(V)
    W = mhla_amd.causal_mixing_init(T // 64).reshape(T // 64, T // 64).cuda().requires_grad_(True)
    do = torch.randn(B, T, H, V, generator=g).to(torch.bfloat16).cuda()
    op = mhla_amd.mhla_causal
elif a.dit_core:
    B, N, H, D, M = 32, 256, 16, 72, 16
    qkv = (torch.rand(B, N, 3, H, D, generator=g) + 0.01).to(torch.bfloat16).cuda().requires_grad_(True)
    W = block_distance_weights((4, 4), "linear").cuda().requires_grad_(True)
    lepe_w = (0.1 * torch.randn(H * D, 1, 3, 3, generator=g)).cuda().requires_grad_(True)
    lepe_b = (0.1 * torch.randn(H * D, generator=g)).cuda().requires_grad_(True)
    do = torch.randn(B, N, H * D, generator=g).to(torch.bfloat16).cuda()
    op = ops.mhla_dit_core
else:
    B, N, H, D, M = 32, 256, 16, 72, 16
    mk = lambda: (torch.rand(B, N, H, D, generator=g) + 0.01).to(torch.bfloat16).cuda().requires_grad_(True)
    q, k, v = mk(), mk(), mk()
    W = block_distance_weights((4, 4), "linear").cuda().requires_grad_(True)
    do = torch.randn(B, N, H, D, generator=g).to(torch.bfloat16).cuda()
    op = mhla_amd.mhla_blockmix
print(f"{op.__name__}, {'C++' if ops._native_nodes() and not a.dit_core else 'Python'} autograd nodes")


def step():
    out = op(qkv, W, lepe_w, lepe_b, 4, 4) if a.dit_core else op(q, k, v, W)
    out.backward(do)


for _ in range(20):
    step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(iters):
    step()
t1 = time.perf_counter()
torch.cuda.synchronize()
t2 = time.perf_counter()
print(f"host time per step (launch side) {1e6 * (t1 - t0) / iters:.1f} us; with final sync {1e6 * (t2 - t0) / iters:.1f} us")
pr = cProfile.Profile()
pr.enable()
for _ in range(iters):
    step()
pr.disable()
torch.cuda.synchronize()
pstats.Stats(pr).sort_stats("tottime").print_stats(32)
