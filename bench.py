#!/usr/bin/env python
"""MHLA operator bench: fwd+bwd tokens/s at (B, N, H, D) on MI355X, with roofline and CPU baseline.

  python bench.py --gpus N --steps K --warmup W        (N > 1: launched by torch.distributed.run)
  python bench.py ... --full                           (everything else the bench measures, see below)
  python bench.py ... --dump-outputs DIR               (what the last timed step computed, as DIR/<name>.npy)

A "step" is one forward + backward of the block-mixing MHLA operator over one synthetic batch
resident in HBM.  Workload at every N (weak scaling, per GPU): BASELINE.json configs[1]
"Synthetic MHLA op micro-bench B=8 N=4096 H=16 D=64 bf16" with M = 64 blocks of S = 64 tokens.
Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line (headline figure and the roofline
fraction that follows from it by arithmetic).  `--full` adds every other measurement after the timed
steps: GPU-event time of the step, per-kernel durations, PMC traffic and MFMA figures, the reduced-precision
step, the measured peaks, the CPU baselines, the other BASELINE.json shapes, the DiT / GPT / Wan step
benches and the `targets` block, with the full record written to bench_full.json.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.29 TB/s measured float4 copy)
MFMA_BF16_PEAK_TFLOPS = 2500.0


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--B", type=int, default=8)
    p.add_argument("--N", type=int, default=4096)
    p.add_argument("--H", type=int, default=16)
    p.add_argument("--D", type=int, default=64)
    p.add_argument("--M", type=int, default=64)
    p.add_argument("--dtype", default="bf16", choices=["bf16", "f32", "f16"])
    p.add_argument("--summaries", default="tf32", choices=["tf32", "split", "bf16"],
                   help="arithmetic on 16-bit tensors: tf32 = the library's default and the number of record (bf16 hi + lo operands, fp32 "
                        "accumulation, block summaries stored with 11 significand bits in 2 bytes: the precision of the reference's own TF32 "
                        "matmuls, mhla_dit/train.py:12-13); split = summaries with >= 16 significand bits (24-bit floats: round 5's default); "
                        "bf16 = the opt-in reduced-precision form (single-bf16 block summaries)")
    p.add_argument("--no-step-benches", action="store_true",
                   help="skip the step-level measurements of BASELINE.json configs[3] / [4] (Wan2.1-1.3B forward, GPT training steps)")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-extra-configs", action="store_true",
                   help="skip the other BASELINE.json shapes (C3 / C4 / C5 / C2 variants) reported as `extra_configs` at N = 1")
    p.add_argument("--no-graph", dest="graph", action="store_false",
                   help="launch every step eagerly through Python autograd instead of replaying the captured HIP graph")
    p.set_defaults(graph=True)
    p.add_argument("--preheat-steps", type=int, default=100,
                   help="one GPU, graph launches: steps replayed untimed during set-up, right after the capture (uploads the graph and brings the "
                        "clocks up, so that a 20-step and a 200-step run report the same ms/step); the W warm-up steps follow")
    p.add_argument("--step-benches", action="store_true", help="N > 1: also run the GPT-1.3B DDP training step (always on at N = 1)")
    p.add_argument("--graph-steps", type=int, default=10, help="whole steps captured per HIP graph on one GPU (1: one step per replay)")
    p.add_argument("--dit-step-timeout", type=float, default=240.0, help="seconds after which the DiT training-step measurement is abandoned")
    p.add_argument("--no-dit-step", action="store_true",
                   help="skip the second measurement: the DiT-XL/2 256^2 training step of the thin host (DDP over RCCL when N > 1)")
    p.add_argument("--full", action="store_true",
                   help="after the timed steps, run every other measurement and check of the bench (see the module docstring; the --no-* "
                        "options trim it) and write the full record to bench_full.json; off by default")
    p.add_argument("--dump-outputs", metavar="DIR",
                   help="after the timed steps, write what the last timed step computed (out, dq, dk, dv, dW; rank 0) as DIR/<name>.npy "
                        "in float32: token tensors larger than 2^21 values as a fixed, seeded sample of their (b, n) token rows")
    return p.parse_args()


def make_inputs(a, device, seed):
    from mhla_amd import block_distance_weights
    dt = {"bf16": torch.bfloat16, "f32": torch.float32, "f16": torch.float16}[a.dtype]
    g = torch.Generator().manual_seed(seed)
    shape = (a.B, a.N, a.H, a.D)
    q = (torch.relu(torch.randn(shape, generator=g)) + 1e-6).to(dt).to(device)
    k = (torch.relu(torch.randn(shape, generator=g)) + 1e-6).to(dt).to(device)
    v = torch.randn(shape, generator=g).to(dt).to(device)
    do = torch.randn(shape, generator=g).to(dt).to(device)
    side = int(round(a.M ** 0.5))
    W = block_distance_weights((side, side) if side * side == a.M else (a.M,), "linear").to(device)
    return q, k, v, W, do


DUMP_VALUES_PER_TENSOR = 1 << 21   # 8 MiB of float32 per token tensor: the four of them and dW stay well under 64 MB


def dump_outputs(d, outs):
    """Write one step's results (out, dq, dk, dv: [B, N, H, D]; dW: [M, M]) to d/<name>.npy as float32.  A token tensor of more
    than DUMP_VALUES_PER_TENSOR values is written as a sample of its B*N token rows, [rows, H, D]: the same rows for every tensor,
    drawn from a fixed seed, so two runs with the same arguments write the same positions."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    rows = None
    total = 0
    for name, t in zip(("out", "dq", "dk", "dv", "dW"), outs):
        t = t.detach()
        if t.dim() == 4 and t.numel() > DUMP_VALUES_PER_TENSOR:
            t = t.reshape(-1, t.shape[2], t.shape[3])
            if rows is None:
                n = max(1, DUMP_VALUES_PER_TENSOR // t[0].numel())
                rows = torch.randperm(t.shape[0], generator=torch.Generator().manual_seed(0))[:n].sort().values.to(t.device)
            t = t.index_select(0, rows)
        arr = t.float().cpu().numpy()
        total += arr.nbytes
        assert total <= 64_000_000, f"--dump-outputs: {total} bytes"
        np.save(os.path.join(d, name + ".npy"), arr)


def cpu_baseline(a, budget_s=15.0, Bs=None):
    """The oracle (eager PyTorch restatement of the reference op sequence, fp32) timed on the host cores
    on a bounded sample: fwd+bwd over B_s samples of the same (N, H, D, M) workload -- by default the whole per-GPU batch
    of the step (B = 8 at C2: ~0.6 s per iteration on 64 threads, at least 5 iterations)."""
    Bs = Bs or a.B
    from oracle import mhla_oracle as orc
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    torch.set_num_threads(max(1, min(ncpu, 64)))
    g = torch.Generator().manual_seed(1234)
    shape = (Bs, a.N, a.H, a.D)
    q = (torch.relu(torch.randn(shape, generator=g)) + 1e-6).requires_grad_(True)
    k = (torch.relu(torch.randn(shape, generator=g)) + 1e-6).requires_grad_(True)
    v = torch.randn(shape, generator=g).requires_grad_(True)
    do = torch.randn(shape, generator=g)
    side = int(round(a.M ** 0.5))
    W = orc.block_distance_weights((side, side) if side * side == a.M else (a.M,), "linear").requires_grad_(True)

    def it():
        out = orc.blockmix_fwd(q, k, v, W, 1e-6)
        (out * do).sum().backward()
        q.grad = k.grad = v.grad = W.grad = None

    it()   # warm-up
    times = []
    t_end = time.perf_counter() + budget_s
    while len(times) < 5 or (time.perf_counter() < t_end and len(times) < 20):
        t0 = time.perf_counter()
        it()
        times.append(time.perf_counter() - t0)
    times.sort()
    med = times[len(times) // 2]
    return {"value": Bs * a.N / med, "unit": "tokens/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"oracle (eager PyTorch fp32, autograd bwd) fwd+bwd on B={Bs} x N={a.N} x H={a.H} x D={a.D}, "
                      f"M={a.M}; median of {len(times)} iterations ({med * 1e3:.0f} ms each)"}


def measured_peaks(dev):
    """the two peaks measured on this box in this run (under a second together), listed beside the nominal
    `peak` that `frac` is priced against: a 1 GiB fp32 device copy (read + write bytes over time) and one 8192^3 bf16 GEMM
    through torch.matmul (hipBLASLt / rocBLAS)."""
    def ev(fn, n):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e-3
    x = torch.empty(1 << 28, dtype=torch.float32, device=dev).normal_()
    y = torch.empty_like(x)
    t_copy = ev(lambda: y.copy_(x), 10)
    del x, y
    a_ = torch.randn(8192, 8192, device=dev, dtype=torch.bfloat16)
    b_ = torch.randn(8192, 8192, device=dev, dtype=torch.bfloat16)
    t_mm = ev(lambda: torch.matmul(a_, b_), 5)
    return {"hbm_copy_GBps": 2 * (1 << 30) / t_copy / 1e9, "bf16_gemm_TFLOPS": 2 * 8192 ** 3 / t_mm / 1e12,
            "how": "1 GiB fp32 copy_ (r+w); 8192^3 bf16 matmul"}


def targets_block(res, world):
    """north_star's four target figures, as far as this run measured them (BASELINE.json `north_star`, last sentence)."""
    import glob
    import hashlib
    t = {}
    ns = res.get("north_star_c3")
    t["ge_10x_cpu_eager_on_dit_xl2_256_tokens_1gpu"] = (
        {"measured": False, "note": "needs the default one-GPU run (extra_configs + cpu_baseline)"} if not ns else
        {"measured": True, "gpu_over_cpu_graph_replay": ns.get("gpu_over_cpu_graph_replay"), "gpu_over_cpu_eager": ns.get("gpu_over_cpu_eager"),
         "cpu_cores": ns["cpu_baseline"]["cores"], "met": bool((ns.get("gpu_over_cpu_eager") or 0) >= 10)})
    # parity: the summary of the last `pytest -m gpu` session committed under profiles/, tagged with the hash of the kernel sources
    par = {"measured": False, "note": "no profiles/r*_parity_summary.json"}
    hsh = hashlib.sha256()
    for fn in sorted(glob.glob(os.path.join(ROOT, "mhla_amd", "csrc", "*"))):
        hsh.update(open(fn, "rb").read())
    for pj in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_parity_summary.json")), reverse=True):
        try:
            rep = json.load(open(pj))
        except Exception:   # noqa: BLE001
            continue
        fam = rep.get("by_baseline_config", {})
        par = {"measured": True, "source": os.path.relpath(pj, ROOT), "same_kernel_sources": rep.get("csrc_sha16") == hsh.hexdigest()[:16],
               "comparisons": rep.get("comparisons"), "per_config_full_size": fam,
               "note": "per BASELINE.json configuration at its full size, HIP path vs the CPU oracle. fp32 results (fp32 tensors, and the "
                       "fp32-stored dW / dmix of bf16 runs): max|got - want| / max|want|. 16-bit results: the part of that error beyond the "
                       "one rounding of the stored value (u = 2^-8 per element for bf16, unavoidable). Causal op (the reference computes "
                       "in fp32, naive.py:39): chunk summaries and score tiles as bf16 hi + lo pairs. Block-mix op on bf16 tensors (round 5): "
                       "fp32 block summaries / bf16 hi + lo operands and score tiles, and an fp32-grade O in the backward's row dots -- "
                       "the reference's fp32 arithmetic (mhla_dit/train.py:12-13); the opt-in summaries='bf16' form is listed as its own "
                       "'[reduced precision]' family and is not what `met` refers to"}
        worst = lambda ks: max([max(fam[k]["results_16bit_max_beyond_final_rounding"], fam[k]["results_fp32_max_rel_err"]) for k in fam if k.split("/")[0] in ks] or [None])
        par["fp32_tensors_c3_c4"] = {"worst": max([max(v["results_16bit_max_beyond_final_rounding"], v["results_fp32_max_rel_err"]) for k, v in fam.items() if "fp32 tensors" in k] or [None])}
        par["causal_bf16_c5"] = {"worst": worst(("c5", "c5_1p3b_like"))}
        par["blockmix_bf16_c2_c3"] = {"worst": max([max(v["results_16bit_max_beyond_final_rounding"], v["results_fp32_max_rel_err"]) for k, v in fam.items() if k.endswith("bf16 tensors") and k[:2] in ("c2", "c3")] or [None])}
        for k in ("fp32_tensors_c3_c4", "causal_bf16_c5", "blockmix_bf16_c2_c3"):
            par[k]["met"] = par[k]["worst"] is not None and par[k]["worst"] <= 1e-3
        break
    t["within_1e-3_rel_err_of_reference"] = par
    rf = res.get("roofline", {})
    module_level = {"measured": False, "note": "no profiles/r*_module_dit.json (tools/prof_module_mfma.sh)"}
    for pj in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_module_dit.json")), reverse=True):
        try:
            mj = json.load(open(pj))
            module_level = {"measured": True, "source": os.path.relpath(pj, ROOT),
                            "what": "DiT-XL/2 attention module (LayerNorm -> QKV GEMM -> operator + LePE -> out GEMM) fwd+bwd, B=32 x 256 tokens, bf16",
                            "ms": mj["module_timing"].get("ms"),
                            "mfma_flop_frac_of_bf16_dense_peak": mj["module_timing"].get("mfma_flop_frac_of_bf16_dense_peak"),
                            "mfma_busy_over_sq_busy_time_weighted": mj.get("module_time_weighted_mfma_busy_over_sq_busy"),
                            "same_ratio_for_a_lone_8192_cubed_hipblaslt_gemm": mj.get("calibration_gemm_mfma_busy_over_sq_busy"),
                            "relative_to_that_gemm": mj.get("module_mfma_busy_relative_to_calibration_gemm"),
                            "gemm_share_of_gpu_time": mj.get("gemm_share_of_gpu_time"), "mhla_share_of_gpu_time": mj.get("mhla_share_of_gpu_time")}
            break
        except Exception:   # noqa: BLE001
            continue
    t["ge_40pct_mfma_utilisation"] = {
        "measured": True, "mfma_flop_frac_of_bf16_dense_peak": rf.get("mfma_frac_of_bf16_peak"),
        "mfma_pipe_busy_frac_pmc": rf.get("mfma_busy_frac_pmc"), "module_level": module_level, "met": False,
        "note": "the operator is HBM-bound at 48 FLOP/B against a ridge of ~300 FLOP/B: at the HBM roofline its MFMA FLOP utilisation "
                "tops out near 15 % (SURVEY.md 8(d)); 40 % is only reachable at module level with the projections"}
    t["ge_6x_at_8_gpus_vs_1"] = {"measured": False, "n_gpus_of_this_line": world,
                                 "note": "one line per N: the driver forms the ratio from its N = 1, 2, 4, 8 runs (weak scaling, dW all-reduce "
                                         "only on this line; `dit_xl2_train_step` carries the DDP step)"}
    return t


LINE_LIMIT = 4000   # bytes; the driver keeps a bounded tail of stdout and parses the last line (round 5's 20.6 KB line did not parse)


def _finite(x):
    """Strict-JSON sanitiser: NaN / inf -> None (json.dumps(allow_nan=False) would raise), floats rounded to 6 significant digits."""
    if isinstance(x, float):
        return float(f"{x:.6g}") if x == x and abs(x) != float("inf") else None
    if isinstance(x, dict):
        return {str(k_): _finite(v_) for k_, v_ in x.items()}
    if isinstance(x, (list, tuple)):
        return [_finite(v_) for v_ in x]
    return x


def compact_line(res):
    """The ONE stdout line: the contract keys only, built from the full record.  Everything else
    (per-kernel durations, extra_configs, step benches, parity families) lives in bench_full.json / on stderr."""
    rf = res.get("roofline") or {}
    dk = rf.get("dominant_kernel") or {}
    cfg = res.get("config") or {}
    line = {k_: res.get(k_) for k_ in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                       "scaling", "vs_baseline", "dtype", "data")}
    line["config"] = {k_: cfg[k_] for k_ in ("workload", "global_batch", "parallelism", "launch", "arithmetic", "shared_gpu_harness") if k_ in cfg}
    line["roofline"] = {k_: rf.get(k_) for k_ in ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_over_algorithmic",
                                                  "algorithmic_bytes_per_step", "gpu_us_per_step", "frac_from_gpu_events")}
    line["roofline"]["dominant_kernel"] = {k_: dk.get(k_) for k_ in ("name", "avg_us", "algorithmic_bytes", "frac")} if dk else None
    if rf.get("peak_measured"):
        line["roofline"]["peak_measured"] = rf["peak_measured"]
    if res.get("cpu_baseline"):
        line["cpu_baseline"] = res["cpu_baseline"]
        line["gpu_over_cpu"] = res.get("gpu_over_cpu")
    rp = res.get("reduced_precision_bf16_summaries")
    if rp:
        line["reduced_precision"] = {"ms": rp.get("ms_per_step"), "tokens_per_s": rp.get("tokens_per_s")} if "error" not in rp else {"error": rp["error"][:80]}
    t = res.get("targets") or {}
    if t:
        c3, par, mf = (t.get("ge_10x_cpu_eager_on_dit_xl2_256_tokens_1gpu") or {}, t.get("within_1e-3_rel_err_of_reference") or {},
                       t.get("ge_40pct_mfma_utilisation") or {})
        fams = [par.get(k_, {}).get("worst") for k_ in ("fp32_tensors_c3_c4", "causal_bf16_c5", "blockmix_bf16_c2_c3")]
        line["targets"] = {
            "ge_10x_cpu_on_dit_xl2_256": {"met": c3.get("met"), "gpu_over_cpu": c3.get("gpu_over_cpu_eager")},
            "within_1e-3_of_reference": {"met": (all(par.get(k_, {}).get("met") for k_ in ("fp32_tensors_c3_c4", "causal_bf16_c5", "blockmix_bf16_c2_c3"))
                                                 if par.get("measured") else None),
                                         "worst": max([f_ for f_ in fams if f_ is not None] or [None]) if any(f_ is not None for f_ in fams) else None,
                                         "source": par.get("source"), "same_kernel_sources": par.get("same_kernel_sources")},
            "ge_40pct_mfma": {"met": mf.get("met"), "op_flop_frac": mf.get("mfma_flop_frac_of_bf16_dense_peak"),
                              "module_flop_frac": (mf.get("module_level") or {}).get("mfma_flop_frac_of_bf16_dense_peak")},
            "ge_6x_at_8_gpus": {"met": None, "note": "driver forms the ratio from its N=1,2,4,8 runs"}}
    for k_ in ("dit_xl2_train_step", "gpt_1p3b_train_step"):
        st = res.get(k_)
        if isinstance(st, dict):
            line[k_] = {kk: st.get(kk) for kk in ("ms_per_step", "tokens_per_s", "error") if st.get(kk) is not None}
    line["full_record"] = res.get("full_record")
    line = _finite(line)
    out = json.dumps(line, allow_nan=False, separators=(",", ":"))
    # belt and braces: shed optional blocks, least important first, until the line fits
    for drop in ("gpt_1p3b_train_step", "dit_xl2_train_step", "targets", "reduced_precision"):
        if len(out) <= LINE_LIMIT:
            break
        line.pop(drop, None)
        out = json.dumps(line, allow_nan=False, separators=(",", ":"))
    if len(out) > LINE_LIMIT:
        for k_ in ("launch", "arithmetic"):
            line["config"][k_] = str(line["config"].get(k_))[:120]
        if "cpu_baseline" in line:
            line["cpu_baseline"]["sample"] = line["cpu_baseline"]["sample"][:160]
        out = json.dumps(line, allow_nan=False, separators=(",", ":"))
    assert len(out) <= LINE_LIMIT, len(out)
    return out


def emit(res):
    """Full record -> bench_full.json beside this file (and gpurun_out/ when it exists; fallback $TMPDIR); a short per-kernel
    digest -> stderr; the compact line -> stdout, last.  stderr stays small on purpose: a harness that keeps one bounded tail of
    both streams must still see the whole stdout line."""
    full = json.dumps(_finite(res), allow_nan=False)
    where = None
    for d in (ROOT, os.path.join(ROOT, "gpurun_out"), os.environ.get("TMPDIR", "/tmp")):
        try:
            if not os.path.isdir(d):
                continue
            with open(os.path.join(d, "bench_full.json"), "w") as f:
                f.write(full + "\n")
            where = where or os.path.join(d, "bench_full.json")
        except OSError:
            continue
    res["full_record"] = (os.path.relpath(where, ROOT) if where and where.startswith(ROOT) else where) or "not written (no writable directory)"
    kern = (res.get("roofline") or {}).get("kernels") or {}
    digest = ", ".join(f"{n_} {kv['avg_us']:.1f}" for n_, kv in sorted(kern.items(), key=lambda x: -x[1]["us_per_step"]))
    print(f"[bench] full record: {res['full_record']} ({len(full)} bytes); kernel avg us: {digest[:1500]}", file=sys.stderr, flush=True)
    print(compact_line(res), flush=True)


def _config_name(a):
    shape = (a.B, a.N, a.H, a.D, a.M, a.dtype)
    if shape == (8, 4096, 16, 64, 64, "bf16"):
        return "BASELINE.json configs[1]"
    if shape[1:] == (256, 16, 72, 16, "bf16"):
        return "operator shape of BASELINE.json configs[2], DiT-XL/2 256x256"
    return "custom shape"


def main():
    a = parse()
    from mhla_amd import dist as mdist
    if a.gpus > 1 and not mdist.launched_by_rendezvous():
        # `python bench.py --gpus N` without torch.distributed.run: this parent starts the N ranks as fresh child processes
        # BEFORE it touches the GPU (device_count() does not initialise it) and only relays their exit status
        ngpu = torch.cuda.device_count()
        extra = {}
        if ngpu < a.gpus:
            extra = {"MHLA_DIST_BACKEND": "gloo", "MHLA_SHARED_GPU_HARNESS": "1"}
            print(f"[bench] --gpus {a.gpus} with {ngpu} visible GPU(s): ranks share devices and exchange over gloo -- a test of "
                  "the multi-rank harness, not a scaling measurement", file=sys.stderr)
        sys.exit(mdist.spawn_local_ranks(a.gpus, [sys.executable, os.path.abspath(__file__)] + sys.argv[1:], extra))
    rank, local, world = mdist.init_from_env()
    if world != a.gpus:
        raise SystemExit(f"[bench] --gpus {a.gpus} but the job has WORLD_SIZE={world} ranks")
    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback for the product path)"
    shared = os.environ.get("MHLA_SHARED_GPU_HARNESS") == "1" or world > torch.cuda.device_count()
    if world > 1:
        import torch.distributed as dist
        assert dist.get_world_size() == a.gpus
        if not shared:
            assert dist.get_backend() == "nccl", f"multi-GPU ranks must exchange over RCCL, got {dist.get_backend()}"
    local = local % torch.cuda.device_count()   # ranks > GPUs only in the shared-GPU harness test (MHLA_DIST_BACKEND=gloo)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    import mhla_amd
    lib = mhla_amd._lib.load()

    q, k, v, W, do = make_inputs(a, dev, 1234 + rank)
    for t in (q, k, v, W):
        t.requires_grad_(True)

    reducer = mdist.OverlappedGradAllReduce()

    def fwd_bwd(keep=False):
        """One forward + backward; keep=True returns what it computed: (out, dq, dk, dv, dW)."""
        out = mhla_amd.mhla_blockmix(q, k, v, W, eps=1e-6, summaries=a.summaries)
        out.backward(do)
        return (out, q.grad, k.grad, v.grad, W.grad) if keep else None

    eager_outs = [None]

    def step():
        eager_outs[0] = None   # the previous step's results go back to the allocator before this step allocates
        eager_outs[0] = fwd_bwd(keep=True)
        # the one real exchange of a data-parallel step on this path: the mean all-reduce of dW, scheduled like DDP's
        # reducer (asynchronous, consumed at the next step / the closing synchronisation of the timed region)
        reducer.issue(W.grad)
        q.grad = k.grad = v.grad = W.grad = None

    sync = torch.cuda.synchronize
    eager_step = step
    step_group, group = None, 1
    launch_mode = "eager (Python autograd)"
    # the results of the last single step and of the last step of a `step_group` call (for --dump-outputs)
    step_outs, group_outs = (lambda: eager_outs[0]), None
    if a.graph:
        # Whole-step capture: the forward + backward (both autograd calls, their workspace allocations, every launch) is
        # recorded once in a HIP graph and replayed -- the same work with no Python on the launch path, so the number does
        # not depend on the host's speed.  Falls back to eager launches if the capture is refused.
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    mhla_amd.mhla_blockmix(q, k, v, W, eps=1e-6, summaries=a.summaries).backward(do)
            torch.cuda.current_stream().wait_stream(side)
            q.grad = k.grad = v.grad = W.grad = None
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                graph_outs = fwd_bwd(keep=True)

            def step():   # noqa: F811
                graph.replay()
                reducer.issue(W.grad)

            launch_mode = "hipGraph replay of the captured fwd+bwd step"
            step_outs = lambda: graph_outs   # noqa: E731
            if world > 1:
                # N ranks: every step is one replay followed by the all-reduce of its dW.  The gradient lives in the graph's static
                # buffer, so two graphs alternate, each ending with "its" copy of dW / N: the collective of step k runs while
                # graph (k + 1) % 2 computes, and a buffer is rewritten only after its previous collective was waited for
                q.grad = k.grad = v.grad = W.grad = None
                gbufs = [torch.empty_like(W, dtype=torch.float32) for _ in range(2)]
                graphs, alt_outs = [], []
                for gb_ in gbufs:
                    g_ = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g_):
                        o_ = fwd_bwd(keep=True)
                        gb_.copy_(W.grad).div_(world)
                        q.grad = k.grad = v.grad = W.grad = None
                    graphs.append(g_)
                    alt_outs.append(o_[:4] + (gb_,))   # dW: the all-reduced mean, once the step's collective was waited for
                phase = [0]

                def step():   # noqa: F811
                    i = phase[0]
                    phase[0] = i ^ 1
                    graphs[i].replay()
                    reducer.issue(gbufs[i], prescaled=True)

                launch_mode = "hipGraph replay of the captured fwd+bwd step (+ dW / N), then its all-reduce; two graphs alternate"
                step_outs = lambda: alt_outs[phase[0] ^ 1]   # noqa: E731
            if world == 1 and a.graph_steps > 1:
                # one GPU: no per-step exchange, so several whole steps go into one graph (each replay costs ~15 us of device-side
                # start-up whatever it holds); every captured step is the complete forward + backward on the same inputs
                q.grad = k.grad = v.grad = W.grad = None
                graph_g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph_g):
                    for i_ in range(a.graph_steps):
                        group_outs = fwd_bwd(keep=i_ == a.graph_steps - 1)
                        q.grad = k.grad = v.grad = W.grad = None
                # the first launch of an instantiated graph uploads it to the device (~0.5 ms, seen as +10 % on a 20-step run): one
                # untimed replay right after the capture, besides the W warm-up steps (which use the one-step graph when W is
                # not a multiple of the group)
                for _ in range(max(1, a.preheat_steps // a.graph_steps)):
                    graph_g.replay()
                sync()
                step_group, group = graph_g.replay, a.graph_steps
                launch_mode = (f"hipGraph replay, {a.graph_steps} captured fwd+bwd steps per replay (remainder: one step per replay); "
                               f"set-up replays the captured graph {max(1, a.preheat_steps // a.graph_steps)}x untimed (graph upload, clock ramp) "
                               "before the W warm-up steps")
        except Exception as e:   # noqa: BLE001
            if rank == 0:
                print(f"[bench] graph capture failed ({type(e).__name__}: {e}); eager launches", file=sys.stderr)
            q.grad = k.grad = v.grad = W.grad = None
            step, step_group, group = eager_step, None, 1
            step_outs, group_outs = (lambda: eager_outs[0]), None

    def sync_all():
        reducer.wait()
        sync()

    el = mdist.timed_steps(step, a.steps, a.warmup, sync_all, step_group, group)
    ms_per_step = el / a.steps * 1e3
    tokens_per_step = a.B * a.N * world
    value = tokens_per_step / (el / a.steps)
    if a.dump_outputs and rank == 0:
        # the last timed step was a `step_group` call when K is a multiple of the group, else a single step
        dump_outputs(a.dump_outputs, group_outs if step_group is not None and group > 1 and a.steps % group == 0 else step_outs())

    esz = {"bf16": 2, "f16": 2, "f32": 4}[a.dtype]
    nde = a.B * a.H * a.N * a.D * esz                         # one token tensor of this rank's batch
    alg_bytes = 12 * nde                                      # fwd 4 NDe + bwd 8 NDe per (b, h)
    # the roofline figure of the line comes from the ONE timed number, ms_per_step (wall clock of the timed region, launch
    # overheads included); with --full the GPU-time bracket of the second pass is listed beside it
    achieved = alg_bytes / (ms_per_step * 1e-3) / 1e9
    res = None
    if rank == 0:
        res = {
            "metric": "MHLA fwd+bwd tokens/sec at (B,N,H,D)",
            "value": value, "unit": "tokens/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": a.dtype, "data": "synthetic",
            "config": {"workload": f"block-mix MHLA op fwd+bwd, per GPU B={a.B} N={a.N} H={a.H} D={a.D} "
                                   f"M={a.M} S={a.N // a.M} {a.dtype} ({_config_name(a)})",
                       "global_batch": a.B * world, "parallelism": f"dp{world} (batch shards, dW all-reduce only)",
                       "launch": launch_mode,
                       "arithmetic": {"tf32": "library default: bf16 hi + lo operands, fp32 accumulation, block summaries stored as fp16 payload x a power-of-two "
                                              "multiplier per block row (11 significand bits, 2 bytes) = the precision the reference's matmul / 1x1 conv run at "
                                              "(mhla_dit/mhla/mhla.py:262-263 under allow_tf32, mhla_dit/train.py:12-13); within 1e-3 of the fp32 result (observed 3e-4)",
                                      "split": "block summaries as 24-bit floats (>= 16 significand bits; opt-in MHLA_FLAG_FP32_GRADE_SUMMARIES, round 5's default)",
                                      "bf16": "REDUCED PRECISION (--summaries bf16, opt-in MHLA_FLAG_BF16_SUMMARIES): single-bf16 block summaries"}[a.summaries if a.dtype != "f32" else "split"],
                       "autograd_nodes": "C++ (libmhla_torch.so)" if mhla_amd.ops._native_nodes() else "Python (ops.py)",
                       **({"shared_gpu_harness": f"{world} ranks on {torch.cuda.device_count()} GPU(s), gloo: harness test, "
                                                  "not a scaling measurement"} if shared else {})},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS if achieved else None, "algorithmic_bytes_per_step": alg_bytes},
        }
    if not a.full:
        if rank == 0:
            print(compact_line(res), flush=True)
        _close(world)
        return

    # ---- GPU time of the whole step: HIP events on the launch stream around K more steps (the library's side-stream work
    # is joined back into this stream before each backward returns, so the bracket covers it) ----
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    sync_all()
    ev0.record()
    mdist.run_steps(step, a.steps, step_group, group)
    ev1.record()
    sync_all()
    step_gpu_us = ev0.elapsed_time(ev1) / a.steps * 1e3

    # ---- per-kernel durations, measured live with HIP events on the launch stream ----
    lib.mhla_prof_enable(1)
    step = eager_step   # per-kernel event timing needs the eager launches
    for _ in range(a.steps):
        step()
    sync()
    lib.mhla_prof_enable(0)
    import ctypes
    buf = ctypes.create_string_buffer(1 << 16)
    lib.mhla_prof_report(buf, len(buf))
    kernels = {}
    for line in buf.value.decode().splitlines():
        name, cnt, tot = line.rsplit(" ", 2)
        kernels[name] = {"launches_per_step": int(cnt) / a.steps, "avg_us": float(tot) / int(cnt) * 1e3,
                         "us_per_step": float(tot) / a.steps * 1e3}
    gpu_us = sum(kv["us_per_step"] for kv in kernels.values())
    # share of the algorithmic token traffic each kernel is responsible for: the dominant kernel's own
    # roofline fraction is its share / its duration
    share = {"k_t16_bwd": 7, "k_t16_bwd_dkv": 4, "k_t16_bwd_dq": 3, "k_t16_out": 2,
             "k_fs_state_fwd": 2, "k_fs_state<1>": 3,
             "k_sp_state": 2, "k_sp_out": 2, "k_sp_state<1>": 3, "k_sp_bwd_dq": 1, "k_sp_bwd_dkv": 4,   # (mixing / dW kernels: summaries only)
             "k_bm_bwd_tok": 7, "k_bm_state<0>": 2, "k_bm_state<1>": 3, "k_bm_out": 2}
    # the dominant kernel: the longest one; the four token kernels of the backward are within a few per cent of each other, so among the
    # kernels within 5 % of the longest the one responsible for the most token traffic is named (a stable choice from run to run)
    dom = None
    if kernels:
        top = max(v["us_per_step"] for v in kernels.values())
        dom = max((n for n in kernels if kernels[n]["us_per_step"] >= 0.95 * top), key=lambda n: (share.get(n, 0), kernels[n]["us_per_step"]))
    # HBM bytes per step: PMC counters cannot be read from inside this process, so the figure comes from the rocprofv3 PMC
    # passes of this same command (tools/prof_all.sh + tools/collect_profiles.py -> profiles/r*_pmc_traffic.json) -- and only when that file was made
    # from the kernel sources this library was built from (it records their hash); otherwise null
    traffic, traffic_src, mfma_busy = None, None, None
    if (a.B, a.N, a.H, a.D, a.M, a.dtype) == (8, 4096, 16, 64, 64, "bf16"):
        import glob
        import hashlib
        hsh = hashlib.sha256()
        for fn in sorted(glob.glob(os.path.join(ROOT, "mhla_amd", "csrc", "*"))):
            hsh.update(open(fn, "rb").read())
        for pj in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")), reverse=True):
            try:
                rec = json.load(open(pj))
                if rec.get("csrc_sha16") == hsh.hexdigest()[:16]:
                    rec = rec.get("shapes", {}).get("c2", rec)   # round 3: one file for every shape; rounds 1-2: C2 only
                    traffic, traffic_src = rec["hbm_bytes_per_step"], os.path.relpath(pj, ROOT)
                    # share of a wave's life in which the matrix pipe was busy for it (SQ_VALU_MFMA_BUSY_CYCLES per wave over
                    # SQ_WAVE_CYCLES per wave), per kernel: the counter-based "MFMA utilisation" of the same PMC passes
                    mfma_busy = {kr["kernel"]: kr["mfma_busy_cycles_per_wave"] / (kr["us_per_wave"] * 2.4e3)
                                 for kr in rec["kernels"] if kr.get("us_per_wave")}
                    break
            except Exception:   # noqa: BLE001
                pass
    # ---- second, separately named measurement: the DiT-XL/2 256^2 training step of the thin host.  With N > 1 this is the
    # step whose exchange is worth measuring (DDP's bucketed all-reduce of 2.7 GB of fp32 gradients over RCCL, overlapped with
    # the backward); the operator line above only exchanges the 16 KB dW.  Every rank takes part.
    dit_step = None
    run_dit = not a.no_dit_step and _config_name(a) == "BASELINE.json configs[1]" and not shared
    alg_flops = a.B * a.H * (12 * a.N * a.D * a.D + 6 * a.M * a.M * a.D * a.D)
    achieved_gpu = alg_bytes / (step_gpu_us * 1e-6) / 1e9 if step_gpu_us else None

    if rank == 0:
        res["roofline"].update({
                "traffic": traffic,
                "traffic_over_algorithmic": traffic / alg_bytes if traffic else None,
                "frac_from_gpu_events": achieved_gpu / HBM_PEAK_GBS if achieved_gpu else None,
                "mfma_busy_frac_pmc": mfma_busy,
                "traffic_source": traffic_src or "none for these kernel sources: run tools/prof_all.sh, then tools/collect_profiles.py (rocprofv3 PMC passes)",
                "scope": "whole fwd+bwd step: `achieved` / `frac` = algorithmic bytes 12*B*H*N*D*e over ms_per_step (the timed "
                         "region); `frac_from_gpu_events` = the same bytes over the GPU time of one step (HIP events on the launch "
                         "stream around K more steps); `dominant_kernel` carries that kernel's own algorithmic share over its own "
                         "average duration; `kernels` lists every kernel's average duration (library per-launch event hook, separate "
                         "eager pass); `mfma_busy_frac_pmc`: matrix-pipe-busy share of a wave's life per kernel from the PMC passes",
                "algorithmic_bytes_per_step": alg_bytes, "gpu_us_per_step": step_gpu_us, "sum_of_kernel_us_per_step": gpu_us,
                "dominant_kernel": None if dom is None else {
                    "name": dom, "avg_us": kernels[dom]["avg_us"],
                    "algorithmic_bytes": share.get(dom, 0) * nde or None,
                    "achieved_GBps": (share.get(dom, 0) * nde / (kernels[dom]["avg_us"] * 1e-6) / 1e9) if share.get(dom) else None,
                    "frac": (share.get(dom, 0) * nde / (kernels[dom]["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS) if share.get(dom) else None},
                "kernels": kernels,
                "mfma_frac_of_bf16_peak": alg_flops / (step_gpu_us * 1e-6) / 1e12 / MFMA_BF16_PEAK_TFLOPS if step_gpu_us else None,
        })
        if world == 1 and a.summaries == "tf32" and a.dtype == "bf16" and not a.no_extra_configs:
            # the opt-in reduced-precision form of the same step (single-bf16 block summaries: rounds 1-4's arithmetic and kernels),
            # for comparison only -- `value` above is the number of record
            try:
                for t_ in (q, k, v, W):
                    t_.grad = None
                g2 = torch.cuda.CUDAGraph()
                side2 = torch.cuda.Stream()
                side2.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side2):
                    for _ in range(3):
                        mhla_amd.mhla_blockmix(q, k, v, W, eps=1e-6, summaries="bf16").backward(do)
                        q.grad = k.grad = v.grad = W.grad = None
                torch.cuda.current_stream().wait_stream(side2)
                with torch.cuda.graph(g2):
                    for _ in range(a.graph_steps):
                        mhla_amd.mhla_blockmix(q, k, v, W, eps=1e-6, summaries="bf16").backward(do)
                        q.grad = k.grad = v.grad = W.grad = None
                for _ in range(3):
                    g2.replay()
                sync()
                e0_, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0_.record()
                for _ in range(10):
                    g2.replay()
                e1_.record()
                sync()
                ms_rp = e0_.elapsed_time(e1_) / (10 * a.graph_steps)
                res["reduced_precision_bf16_summaries"] = {
                    "what": "the same step with summaries='bf16' (MHLA_FLAG_BF16_SUMMARIES): single-bf16 block summaries on the bf16 fast "
                            "path -- REDUCED PRECISION (2-3e-3 of a gradient's maximum beyond the final rounding), not the number of record",
                    "ms_per_step": ms_rp, "tokens_per_s": a.B * a.N / (ms_rp * 1e-3), "hbm_frac": alg_bytes / (ms_rp * 1e-3) / 1e9 / HBM_PEAK_GBS}
                del g2
            except Exception as e:   # noqa: BLE001
                res["reduced_precision_bf16_summaries"] = {"error": f"{type(e).__name__}: {e}"}
        try:
            res["roofline"]["peak_measured"] = measured_peaks(dev)
        except Exception as e:   # noqa: BLE001
            res["roofline"]["peak_measured"] = {"error": f"{type(e).__name__}: {e}"[:120]}
        if world == 1 and not a.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(a)
            res["gpu_over_cpu"] = value / res["cpu_baseline"]["value"]
        if world == 1 and not a.no_extra_configs and _config_name(a) == "BASELINE.json configs[1]":
            # the other BASELINE.json shapes, measured after (outside) the timed region of the main line
            try:
                sys.path.insert(0, os.path.join(ROOT, "tools"))
                import bench_configs
                res["extra_configs"] = bench_configs.run_extra_configs()
                if not a.no_cpu_baseline:
                    # north_star's target shape (DiT-XL/2 256^2 tokens, BASELINE.json configs[2]) against the oracle on the host
                    # cores in this same run: the whole per-GPU batch of 32 samples
                    c3 = argparse.Namespace(B=32, N=256, H=16, D=72, M=16)
                    cb = cpu_baseline(c3, budget_s=10.0, Bs=32)
                    g3 = next(r for r in res["extra_configs"] if r["shape"].startswith("C3") and "bf16" in r["shape"])
                    res["north_star_c3"] = {
                        "shape": g3["shape"], "gpu_tokens_per_s_eager": g3["tokens_per_s"],
                        "gpu_tokens_per_s_graph_replay": 32 * 256 / (g3["ms_graph_replay"] * 1e-3) if g3.get("ms_graph_replay") else None,
                        "cpu_baseline": cb, "gpu_over_cpu_eager": g3["tokens_per_s"] / cb["value"],
                        "gpu_over_cpu_graph_replay": (32 * 256 / (g3["ms_graph_replay"] * 1e-3) / cb["value"]) if g3.get("ms_graph_replay") else None,
                        "target": ">= 10x the CPU-eager reference on DiT-XL/2 256^2 tokens at 1 GPU"}
            except Exception as e:   # noqa: BLE001
                res["extra_configs"] = {"error": f"{type(e).__name__}: {e}"}
    if run_dit:
        # Every rank takes part (DDP collectives).  The operator line must survive whatever happens here: a watchdog on every
        # rank prints the line without this measurement (rank 0) and leaves the process if the step has not finished in time.
        import threading

        printed = threading.Lock()   # the line is printed once: by the watchdog or by the main thread, whoever takes this first

        def give_up():
            if not printed.acquire(blocking=False):
                return               # the main thread is already printing: the step did finish
            if rank == 0:
                res["dit_xl2_train_step"] = {"error": f"not finished within {a.dit_step_timeout} s: abandoned"}
                emit(res)
            os._exit(3)              # a process that abandoned GPU / RCCL work does not report success

        dog = threading.Timer(a.dit_step_timeout, give_up)
        dog.daemon = True
        dog.start()
        try:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import bench_dit_step
            q = k = v = do = None
            torch.cuda.empty_cache()
            dit_step = bench_dit_step.run_dit_step(rank, local, world, "DiT-XL/2", 32, 256, steps=8, warmup=3)
            if isinstance(dit_step, dict):
                dit_step["rccl_env"] = {k_: os.environ.get(k_) for k_ in ("NCCL_ALGO", "NCCL_PROTO", "NCCL_MIN_NCHANNELS", "NCCL_MAX_NCHANNELS", "NCCL_BUFFSIZE")}
                dit_step["bucket_cap_mb"] = 25
        except Exception as e:   # noqa: BLE001
            dit_step = {"error": f"{type(e).__name__}: {e}"}
        # BASELINE.json configs[4] / [3] at step level (tools/bench_steps.py): the GPT-1.3B-shaped training step on every rank (DDP over
        # RCCL when N > 1); at N = 1 also the 340M model the reference ships a config for and the Wan2.1-1.3B 30-block forward
        if not a.no_step_benches and (world == 1 or a.step_benches):
            try:
                import bench_steps
                gpt13 = bench_steps.gpt_step(rank, local, world, "1.3B", batch=1, seq=8192, steps=3, warmup=2)
                if rank == 0:
                    res["gpt_1p3b_train_step"] = gpt13
                if world == 1:
                    res["gpt_340m_train_step"] = bench_steps.gpt_step(rank, local, world, "340M", batch=2, seq=8192, steps=3, warmup=2)
                    res["wan_1p3b_forward"] = bench_steps.wan_forward(dev, layers=30, iters=2, warm=1)
            except Exception as e:   # noqa: BLE001
                if rank == 0:
                    res["step_benches_error"] = f"{type(e).__name__}: {e}"
        dog.cancel()
        if not printed.acquire(blocking=False):
            time.sleep(3600)         # the watchdog fired a moment ago and is printing: it ends the process
        if rank == 0:
            res["dit_xl2_train_step"] = dit_step
    if rank == 0:
        res["targets"] = targets_block(res, world)
        emit(res)
    _close(world)


def _close(world):
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
