import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def load_golden(name):
    """tests/golden/<name>.npz and, for a fixture too large for one committed file, its parts <name>.part1.npz, .part2.npz, ..."""
    import torch

    out, i, path = {}, 0, os.path.join(GOLDEN, name + ".npz")
    while i == 0 or os.path.exists(path):
        z = np.load(path)
        out.update({k: (z[k] if k == "meta" else torch.from_numpy(z[k])) for k in z.files})
        i += 1
        path = os.path.join(GOLDEN, f"{name}.part{i}.npz")
    return out


def rel_err(a, b):
    """max|a-b| / max|b| -- the rel-err the north_star tolerance (1e-3) is stated in."""
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rms_ratio(a, b):
    """fla's RMS error ratio (mhla_nlp/fla/utils.py:76-79)."""
    a, b = a.double(), b.double()
    return ((a - b).square().mean().sqrt() / b.square().mean().sqrt().clamp_min(1e-30)).item()


@pytest.fixture(scope="session")
def golden():
    return load_golden


@pytest.fixture(autouse=True)
def _poison_free_gpu_memory(request):
    """GPU tests: fill a slab of device memory with NaN and hand it back to the caching allocator, so that the workspaces
    and outputs the ops allocate next start as NaN -- a kernel that reads workspace it never wrote (or skips part of an
    output) then fails the parity check instead of passing on lucky zeros."""
    if request.node.get_closest_marker("gpu") is None:
        yield
        return
    import torch

    if torch.cuda.is_available():
        slabs = [torch.full((n,), float("nan"), dtype=torch.float32, device="cuda") for n in (1 << 26, 1 << 24, 1 << 22, 1 << 20)]
        del slabs
    yield


def pytest_sessionfinish(session, exitstatus):
    """After a -m gpu session: the observed parity errors, per (dtype, quantity class), to gpurun_out/parity_report.json."""
    try:
        import gpu_util
    except Exception:
        return
    obs = getattr(gpu_util, "OBSERVED", [])
    if not obs:
        return
    import json
    agg = {}
    for test, name, dtype, e, r, tol, x in obs:
        kind = "output" if name.split(" ")[0] in ("out", "y", "o", "out_nonorm", "o_short") else "gradient"
        key = f"{dtype}/{kind}"
        a = agg.setdefault(key, {"n": 0, "max_rel_err": 0.0, "max_rms_ratio": 0.0, "worst": None, "loosest_tol": 0.0,
                                 "max_beyond_final_rounding": 0.0, "worst_beyond_final_rounding": None})
        if x >= a["max_beyond_final_rounding"]:
            a["max_beyond_final_rounding"], a["worst_beyond_final_rounding"] = x, f"{test} :: {name}"
        a["n"] += 1
        a["max_rms_ratio"] = max(a["max_rms_ratio"], r)
        a["loosest_tol"] = max(a["loosest_tol"], tol)
        if e >= a["max_rel_err"]:
            a["max_rel_err"], a["worst"] = e, f"{test} :: {name} (tol {tol:g})"
    # per BASELINE.json configuration, from the full-size tests (tests named test_full_size_<config>...): what bench.py's `targets`
    # block quotes (north_star: within 1e-3 of the reference).  16-bit results: the error BEYOND the one final rounding of the
    # stored value; fp32 results (fp32 tensors; fp32-stored dW / dmix of bf16 runs): the error itself.
    fam = {}
    for test, name, dtype, e, r, tol, x in obs:
        tl = test.lower()
        if "full_size_" not in tl or name == "linearity":
            continue
        cfg = tl.split("full_size_")[1][:2]                                   # c2 / c3 / c4 / c5
        tens = "fp32 tensors" if cfg == "c4" or (cfg == "c3" and "dtype1" in tl) else "bf16 tensors"
        if cfg == "c5" and "1p3b" in tl:
            cfg = "c5_1p3b_like"
        if tl.endswith("[bf16]") or "[bf16-" in tl or "-bf16]" in tl:             # the opt-in summaries="bf16" parametrisation: its own family
            tens += " [reduced precision: summaries=bf16]"
        elif tl.endswith("[split]") or "[split-" in tl or "-split]" in tl:        # the opt-in summaries="split" parametrisation (>= 16-bit summaries)
            tens += " [summaries=split: 24-bit / fp32 summaries]"
        a = fam.setdefault(f"{cfg}/{tens}", {"n": 0, "results_16bit_max_beyond_final_rounding": 0.0, "results_fp32_max_rel_err": 0.0, "worst": None})
        a["n"] += 1
        key = "results_fp32_max_rel_err" if dtype == "float32" else "results_16bit_max_beyond_final_rounding"
        val = e if dtype == "float32" else x
        if val >= a[key]:
            a[key] = val
            a["worst"] = f"{test.split('::')[-1]} :: {name}" if val >= max(a["results_16bit_max_beyond_final_rounding"], a["results_fp32_max_rel_err"]) else a["worst"]
    import glob
    import hashlib
    hsh = hashlib.sha256()
    for fn in sorted(glob.glob(os.path.join(ROOT, "mhla_amd", "csrc", "*"))):
        hsh.update(open(fn, "rb").read())
    out = os.path.join(ROOT, "gpurun_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "parity_report.json"), "w") as f:
        json.dump({"comparisons": len(obs), "csrc_sha16": hsh.hexdigest()[:16], "by_baseline_config": fam, "by_dtype_and_kind": agg,
                   "all": [dict(test=t, name=n, dtype=d, rel_err=e, rms_ratio=r, tol=tol, beyond_final_rounding=x)
                           for t, n, d, e, r, tol, x in obs]}, f, indent=1)
