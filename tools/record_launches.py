#!/usr/bin/env python
"""Record the launch sequences of the block-mix C ABI on the host, without a GPU, to compare two trees (a refactor of the host layer
must leave them identical):
  python tools/record_launches.py build TREE OUT_DIR   # copies TREE's csrc + include to OUT_DIR, replaces capi_common.hpp's launch() by a
                                                       # logger that returns MHLA_OK, builds OUT_DIR/librec.so from the block-mix units
  python tools/record_launches.py run OUT_DIR/librec.so 2> log   # drives the entry points with never-dereferenced aligned pointers
Every launch is one line on stderr: name string, the kernel's own symbol (dladdr: the exact template instantiation), grid, block, dynamic
LDS size, stream and a hash of the argument bytes; every call's return code and message too.  `diff` the logs of the two trees.  The
argument hash covers struct padding: build with RECORD_ZERO_INIT=1 (host pass with -ftrivial-auto-var-init=zero, which reaches named
locals only) to compare it."""
import ctypes
import itertools
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

LOGGER = '''template <typename K>
int launch(K kernel, dim3 grid, dim3 block, size_t smem, hipStream_t stream, const char* name, auto... args) {
    unsigned long h = 1469598103934665603UL;
    auto mix = [&](const auto& a) { const unsigned char* p = (const unsigned char*)&a; for (size_t i = 0; i < sizeof(a); ++i) h = (h ^ p[i]) * 1099511628211UL; };
    (mix(args), ...);
    Dl_info di{};
    dladdr(reinterpret_cast<const void*>(kernel), &di);
    fprintf(stderr, "LAUNCH %s %s grid=%u,%u,%u block=%u,%u,%u smem=%zu st=%p args=%016lx\\n", name, di.dli_sname ? di.dli_sname : "?", grid.x, grid.y, grid.z,
            block.x, block.y, block.z, smem, (void*)stream, h);
    return MHLA_OK;
}

'''
UNITS = ["capi", "capi_bm_f32", "capi_bm_bf16", "capi_bm_bf16hl", "capi_bm_f16", "capi_bm_wanpro"]


def build(tree, out):
    shutil.copytree(os.path.join(tree, "mhla_amd", "csrc"), os.path.join(out, "mhla_amd", "csrc"))
    shutil.copytree(os.path.join(tree, "include"), os.path.join(out, "include"))
    hdr = os.path.join(out, "mhla_amd", "csrc", "capi_common.hpp")
    s = open(hdr).read()
    a, b = s.index("template <typename K>\nint launch("), s.index("// debugging aid: per-workgroup phase timestamps")
    open(hdr, "w").write((s[:a] + LOGGER + s[b:]).replace("#include <algorithm>", "#include <dlfcn.h>\n#include <algorithm>", 1))
    zero = ["-Xarch_host", "-ftrivial-auto-var-init=zero"] if os.environ.get("RECORD_ZERO_INIT") == "1" else []
    base = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++20", "-fPIC", '-DMHLA_BUILD_FLAGS="rec"', "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"] + zero
    objs = [os.path.join(out, u + ".o") for u in UNITS]
    with ThreadPoolExecutor(len(UNITS)) as ex:
        list(ex.map(lambda u: subprocess.run(base + ["-c", os.path.join(out, "mhla_amd", "csrc", u + ".hip"), "-o", os.path.join(out, u + ".o")], check=True, capture_output=True), UNITS))
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", os.path.join(out, "librec.so"), "-ldl"], check=True)


def run(path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from mhla_amd import _lib as L
    lib = ctypes.CDLL(path)
    for name in ("mhla_last_error", "mhla_blockmix_fwd_ws_bytes", "mhla_blockmix_bwd_ws_bytes", "mhla_blockmix_fwd", "mhla_blockmix_bwd",
                 "mhla_blockmix_rope_fwd", "mhla_blockmix_rope_bwd", "mhla_blockmix_wan_fwd", "mhla_blockmix_wan_pro_fwd"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    V = L.View
    P = 1 << 32
    def say(s):
        sys.stderr.write(s + "\n"); sys.stderr.flush()
    def view(base, H, D, off=0):
        return V(base + off, 1 << 24, H * D, D)
    n = 0
    grid = itertools.product((2, 128), (2, 4, 16, 17, 32, 33, 64, 65, 128, 129, 192, 193, 256, 257), (8, 16, 21, 64), (32, 36, 64, 72, 96, 104, 128), (L.F32, L.BF16, L.F16),
                             (0, L.FLAG_FP32_GRADE_SUMMARIES, L.FLAG_BF16_SUMMARIES), (0, L.FLAG_NO_SMALLN, L.FLAG_FORCE_GENERIC, L.FLAG_NO_BWD_STATE, L.FLAG_RELU_EPS))
    for BH, M, S, D, dt, summ, fl in grid:
        flags = summ | fl
        for mode in ("norm", "nonorm", "split", "misaligned", "nofwdws"):
            if mode != "norm" and (BH == 128 or S == 8):
                continue   # (the variants on a thinner grid)
            off = 8 if mode == "misaligned" else 0
            q, k, v, o, do, dq, dk, dv = (view(P + i * (1 << 28), BH, D, off) for i in range(8))
            qd, kd = (q, k) if mode != "split" else (view(P + 9 * (1 << 28), BH, D), view(P + 10 * (1 << 28), BH, D))
            if mode == "nonorm":
                qd = kd = L.NULL_VIEW
            dqd, dkd = (L.NULL_VIEW, L.NULL_VIEW) if mode != "split" else (view(P + 11 * (1 << 28), BH, D), view(P + 12 * (1 << 28), BH, D))
            split = int(mode == "split")
            fws, bws = lib.mhla_blockmix_fwd_ws_bytes(1, BH, M, S, D, dt, split, flags), lib.mhla_blockmix_bwd_ws_bytes(1, BH, M, S, D, dt, split, flags)
            say(f"CALL BH={BH} M={M} S={S} D={D} dt={dt} flags={flags} mode={mode}")
            rc = lib.mhla_blockmix_fwd(q, k, v, qd, kd, P + (20 << 28), M, o, None, P + (21 << 28), fws, 1, BH, M, S, D, dt, 1e-6, flags, 0x1000)
            say(f"FWD rc={rc} {lib.mhla_last_error().decode() if rc else ''}")
            rc = lib.mhla_blockmix_bwd(q, k, v, qd, kd, P + (20 << 28), M, o, do, dq, dk, dv, dqd, dkd, P + (22 << 28), None, P + (23 << 28), bws,
                                       None if mode == "nofwdws" else P + (21 << 28), 1, BH, M, S, D, dt, 1e-6, flags, 0x1000)
            say(f"BWD rc={rc} {lib.mhla_last_error().decode() if rc else ''}")
            n += 1
    # rotary prologue (fp32 and bf16 forward, fp32 backward), Wan epilogue, Wan prologue-on-load
    for M, S, D, dt in itertools.product((16, 33, 64, 150, 192, 193), (16, 21), (64, 72, 128), (L.F32, L.BF16)):
        BH = 2
        q, k, v, o, do, dq, dk, dv = (view(P + i * (1 << 28), BH, D) for i in range(8))
        cos, sin, W, ws = P + (13 << 28), P + (14 << 28), P + (20 << 28), P + (21 << 28)
        fws, bws = lib.mhla_blockmix_fwd_ws_bytes(1, BH, M, S, D, dt, 0, 0), lib.mhla_blockmix_bwd_ws_bytes(1, BH, M, S, D, dt, 0, 0)
        say(f"ROPE M={M} S={S} D={D} dt={dt}")
        for norm in (0, 1):
            rc = lib.mhla_blockmix_rope_fwd(q, k, v, norm, W, M, cos, sin, 64, o, None, ws, fws, 1, BH, M, S, D, dt, 1e-6, 0, 0x1000)
            say(f"ROPE_FWD rc={rc} {lib.mhla_last_error().decode() if rc else ''}")
            for fw in (None, ws):
                rc = lib.mhla_blockmix_rope_bwd(q, k, v, norm, W, M, cos, sin, 64, o, do, dq, dk, dv, P + (22 << 28), None, P + (23 << 28), bws, fw, 1, BH, M, S, D, dt, 1e-6, 0, 0x1000)
                say(f"ROPE_BWD rc={rc} {lib.mhla_last_error().decode() if rc else ''}")
            for od in (0, 1, 2):
                for c, s in ((None, None), (cos, sin)):
                    rc = lib.mhla_blockmix_wan_fwd(q, k, v, norm, W, M, c, s, 64, P + (15 << 28), 1e-6, view(P + (16 << 28), BH, D), o, od, None, ws, fws, 1, BH, M, S, D, dt, 1e-6, 0, 0x1000)
                    say(f"WAN_FWD rc={rc} {lib.mhla_last_error().decode() if rc else ''}")
                    for S2 in (S, 128, 130):
                        f32ws = lib.mhla_blockmix_fwd_ws_bytes(1, 64, M, S2, D, L.F32, 0, 0)
                        rc = lib.mhla_blockmix_wan_pro_fwd(q, k, v, P + (17 << 28), P + (18 << 28), P + (19 << 28), P + (24 << 28), norm, W, M, c, s, 64, P + (15 << 28), 1e-6,
                                                           view(P + (16 << 28), 64, D), o, od, None, ws, f32ws, 1, 64, M, S2, D, dt, 1e-6, 0, 0x1000)
                        say(f"WAN_PRO rc={rc} {lib.mhla_last_error().decode() if rc else ''}")
    print("calls", n)


if __name__ == "__main__":
    build(sys.argv[2], sys.argv[3]) if sys.argv[1] == "build" else run(sys.argv[2])
