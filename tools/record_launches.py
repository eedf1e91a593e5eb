#!/usr/bin/env python
"""Record the launch sequences of the block-mix and causal C ABI on the host, without a GPU, to compare two trees (a refactor of the host
layer must leave them identical):
  python tools/record_launches.py build TREE OUT_DIR   # copies TREE's csrc + include to OUT_DIR, replaces capi_common.hpp's launch() by a
                                                       # logger that returns MHLA_OK, builds OUT_DIR/librec.so from the block-mix and causal units
  python tools/record_launches.py run OUT_DIR/librec.so [blockmix|causal|decode ...] 2> log   # drives the entry points (default: all three
                                                       # sections) with never-dereferenced aligned pointers
Every launch is one line on stderr: name string, the kernel's own symbol (dladdr: the exact template instantiation), grid, block, dynamic
LDS size, stream and a hash of the argument bytes; every call's return code and message and every size / capability query's answer too.
In the two causal units (the operator: the twelve mhla_causal_* / mhla_causal_varlen_* calls and queries; the decode state: every launching
entry point and size query of capi_causal_state.hip, DECODE_ENTRIES, and the decode prologue of capi_misc.hip) hipMemsetAsync is a logger as
well -- one MEMSET line -- so the launches behind a memset are recorded.
`diff` the logs of the two trees.  The argument hash covers struct padding: build with RECORD_ZERO_INIT=1 (host pass with
-ftrivial-auto-var-init=zero, which reaches named locals only) to compare it."""
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
inline hipError_t rec_memset(void* p, int value, size_t bytes, hipStream_t stream) {
    fprintf(stderr, "MEMSET %p value=%d bytes=%zu st=%p\\n", p, value, bytes, (void*)stream);
    return hipSuccess;
}
#ifdef RECORD_MEMSET
#define hipMemsetAsync rec_memset
#endif

'''
UNITS = ["capi", "capi_bm_f32", "capi_bm_bf16", "capi_bm_bf16hl", "capi_bm_f16", "capi_bm_wanpro", "capi_causal", "capi_causal_gqa", "capi_causal_state", "capi_misc"]
CAUSAL_ENTRIES = ("mhla_causal_fwd_ws_bytes", "mhla_causal_bwd_ws_bytes", "mhla_causal_normgate_fusable", "mhla_causal_fwd", "mhla_causal_normgate_fwd",
                  "mhla_causal_bwd", "mhla_causal_varlen_fwd_ws_bytes", "mhla_causal_varlen_bwd_ws_bytes", "mhla_causal_varlen_normgate_fusable",
                  "mhla_causal_varlen_fwd", "mhla_causal_varlen_normgate_fwd", "mhla_causal_varlen_bwd")
DECODE_ENTRIES = ("mhla_causal_step_ws_bytes", "mhla_causal_state_init", "mhla_causal_step", "mhla_causal_step_ragged", "mhla_causal_step_dev",
                  "mhla_causal_extend_ws_bytes", "mhla_causal_extend", "mhla_causal_extend_ragged_ws_bytes", "mhla_causal_extend_ragged",
                  "mhla_causal_verify_ragged", "mhla_causal_commit_ragged_ws_bytes", "mhla_causal_commit_ragged", "mhla_causal_extend_ragged_gqa_ws_bytes",
                  "mhla_causal_extend_packed_ws_bytes", "mhla_causal_varlen_state_init", "mhla_causal_varlen_state_init_slots",
                  "mhla_causal_varlen_state_init_paged", "mhla_causal_varlen_state_init_paged_h16", "mhla_causal_varlen_state_init_paged_h16_ws_bytes",
                  "mhla_causal_swap_ws_bytes", "mhla_causal_swap_out_paged", "mhla_causal_swap_in_paged", "mhla_featmap_rotary_decode") + tuple(
    f"mhla_causal_{name}_{form}" for name, forms in (("step", ("ragged_gqa", "slots", "paged", "paged_h16")), ("step_dev", ("gqa", "slots", "paged", "paged_h16")),
                                                     ("extend", ("ragged_gqa", "slots", "paged", "packed")), ("verify", ("ragged_gqa", "slots", "paged", "packed")),
                                                     ("commit", ("slots", "paged", "packed"))) for form in forms)


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
        list(ex.map(lambda u: subprocess.run(base + (["-DRECORD_MEMSET"] if u.startswith("capi_causal") else []) + ["-c", os.path.join(out, "mhla_amd", "csrc", u + ".hip"), "-o", os.path.join(out, u + ".o")],
                                             check=True, capture_output=True), UNITS))
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", os.path.join(out, "librec.so"), "-ldl"], check=True)


def say(s):
    sys.stderr.write(s + "\n"); sys.stderr.flush()


def run(path, sections):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from mhla_amd import _lib as L
    lib = ctypes.CDLL(path)
    for name in ("mhla_last_error", "mhla_blockmix_fwd_ws_bytes", "mhla_blockmix_bwd_ws_bytes", "mhla_blockmix_fwd", "mhla_blockmix_bwd",
                 "mhla_blockmix_rope_fwd", "mhla_blockmix_rope_bwd", "mhla_blockmix_wan_fwd", "mhla_blockmix_wan_pro_fwd") + CAUSAL_ENTRIES + DECODE_ENTRIES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    for sec in sections or ("blockmix", "causal", "decode"):
        print(sec, "calls", {"blockmix": run_blockmix, "causal": run_causal, "decode": run_decode}[sec](lib, L))


P = 1 << 32   # fake device addresses: region i is P + (i << 28), 16-byte aligned, never dereferenced


def at(i, off=0):
    return P + (i << 28) + off


def run_blockmix(lib, L):
    V = L.View
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
    return n


class Calls:
    """Calls an entry point and logs `TAG rc=... message`; counts the calls."""
    def __init__(self, lib):
        self.lib, self.n = lib, 0

    def __call__(self, tag, fn, *args):
        rc = getattr(self.lib, fn)(*args)
        say(f"{tag} rc={rc} {self.lib.mhla_last_error().decode() if rc else ''}")
        self.n += 1


def run_causal(lib, L):
    """The causal operator: uniform and packed forward, fused norm x gate forward and backward, with their size / capability queries."""
    call = Calls(lib)
    def view(i, H, D, off=0):
        return L.View(at(i, off), 1 << 24, H * D, D)
    NV = L.NULL_VIEW
    FG, BF, FP = L.CAUSAL_FORCE_GENERIC, L.CAUSAL_BF16_SUMMARIES, L.CAUSAL_FP32_GRADE_SUMMARIES
    mix, dmix, ws, bws, tab, nw = at(20), at(22), at(21), at(23), at(24), at(25)
    grid = itertools.product((2, 256), (1, 63, 64, 65, 321, 8200, 16448), (4, 64, 128, 192, 256, 320), (4, 64, 192, 256, 384, 512, 576),
                             (L.F32, L.BF16, L.F16), (0, FG, BF, FP, BF | FP, 64), (64, 32))
    for H, T, K, Vd, dt, fl, chunk in grid:
        n = (T + chunk - 1) // chunk
        thin = H == 2 and chunk == 64 and fl in (0, FG)   # (the variants of a call on a thinner grid)
        for mode in ("plain", "misaligned", "shortws", "smallld") if thin else ("plain",):
            off = 8 if mode == "misaligned" else 0
            q, k, do, dq, dk = (view(i, H, K, off) for i in (0, 1, 4, 5, 6))
            v, o, y, g, dv = (view(i, H, Vd, off) for i in (2, 3, 8, 9, 7))
            short, ld = int(mode == "shortws"), n - int(mode == "smallld")
            fws, bwsz = lib.mhla_causal_fwd_ws_bytes(1, T, H, K, Vd, chunk, dt, fl), lib.mhla_causal_bwd_ws_bytes(1, T, H, K, Vd, chunk, dt, fl)
            say(f"CAUSAL H={H} T={T} K={K} V={Vd} dt={dt} flags={fl} chunk={chunk} mode={mode} fws={fws} bws={bwsz} "
                f"fusable={lib.mhla_causal_normgate_fusable(T, K, Vd, chunk, dt, fl)}")
            tail = (1, T, H, K, Vd, chunk, 0.125, dt, fl, 0x1000)
            call("FWD", "mhla_causal_fwd", q, k, v, mix, ld, o, ws, fws - short, *tail)
            for gate, out in ((g, o), (g, NV), (NV, o), (NV, NV)):
                call("NORMGATE", "mhla_causal_normgate_fwd", q, k, v, mix, ld, out, gate, nw, 1e-6, y, ws, fws - short, *tail)
            call("NORMGATE_NOY", "mhla_causal_normgate_fwd", q, k, v, mix, ld, o, g, nw, 1e-6, NV, ws, fws, *tail)
            for fw in (ws, None):
                call("BWD", "mhla_causal_bwd", q, k, v, mix, ld, do, dq, dk, dv, dmix, ld, bws, bwsz - short, fw, *tail)
            # packed sequences: the table's row count at, inside and outside its bounds; tables that are refused on the thinner grid
            for nc in (n, n + 3, T, n - 1, T + 1) if thin else (n, n + 3):
                for tb in (tab, None, tab + 4) if thin and mode == "plain" else (tab,):
                    ld = nc - int(mode == "smallld")
                    fws = lib.mhla_causal_varlen_fwd_ws_bytes(1, T, H, K, Vd, chunk, nc, dt, fl)
                    bwsz = lib.mhla_causal_varlen_bwd_ws_bytes(1, T, H, K, Vd, chunk, nc, dt, fl)
                    say(f"PACKED nc={nc} tab={tb and hex(tb)} fws={fws} bws={bwsz} fusable={lib.mhla_causal_varlen_normgate_fusable(T, K, Vd, chunk, nc, dt, fl)}")
                    tail = (1, T, H, K, Vd, chunk, nc, tb, 0.125, dt, fl, 0x1000)
                    call("VFWD", "mhla_causal_varlen_fwd", q, k, v, mix, ld, o, ws, fws - short, *tail)
                    for gate, out in ((g, o), (NV, NV)):
                        call("VNORMGATE", "mhla_causal_varlen_normgate_fwd", q, k, v, mix, ld, out, gate, nw, 1e-6, y, ws, fws - short, *tail)
                    for fw in (ws, None):
                        call("VBWD", "mhla_causal_varlen_bwd", q, k, v, mix, ld, do, dq, dk, dv, dmix, ld, bws, bwsz - short, fw, *tail)
    return call.n


def run_decode(lib, L):
    """The decode state: init, the three steps and the two extensions, then (decode_forms) their forms, the commit, the pack prefill and
    the swap.  Every call is made from one dict of arguments; a variant overrides some of them (a null or misaligned pointer, a short
    workspace, every ldmix from 0 to past the capacity)."""
    call = Calls(lib)
    NV = L.NULL_VIEW
    for (B, H), K, Vd, dt, cap in itertools.product(((2, 2), (4, 64)), (64, 128, 100, 6), (64, 192), (L.F32, L.BF16, L.F16), (1, 3, 5)):
        def view(i, D, off=0):
            return L.View(at(i, off), 1 << 24, H * D, D)
        say(f"DECODE B={B} H={H} K={K} V={Vd} dt={dt} cap={cap} step_ws={lib.mhla_causal_step_ws_bytes(B, H, K, Vd, dt)}")
        base = dict(q=view(0, K), k=view(1, K), v=view(2, Vd), out=view(3, Vd), y=view(8, Vd), gate=view(9, Vd), nw=at(25), mix=at(20), ld=cap + 1,
                    S=at(10), P=at(11), Cur=at(12), pos_dev=at(13), full_dev=at(14), ntok_dev=at(15), cos=None, sin=None, ld_tab=K // 2, rows=64 * cap,
                    fmap=0, ws=at(21), short=0, chunk=64)
        variants = [("", {})]
        if H == 2:   # (the variants on the smaller batch)
            variants += [(f"{name}={'null' if o is None else 'off' + str(o)}", {name: None if o is None else base[name] + o})
                         for name, offs in (("S", (None, 8)), ("P", (None, 8)), ("Cur", (None, 8)), ("pos_dev", (None, 2)), ("full_dev", (None, 2)),
                                            ("ntok_dev", (None, 2)), ("ws", (None, 8)), ("mix", (None,))) for o in offs]
            variants += [(f"out={int(o)} y={int(y)} gate={int(g)} nw={int(w)}", dict(out=base["out"] if o else NV, y=base["y"] if y else NV,
                                                                                     gate=base["gate"] if g else NV, nw=base["nw"] if w else None))
                         for o, y, g, w in itertools.product((0, 1), repeat=4) if not (o and y and g and w)]
            variants += [("views+8", {n_: view(i, D, 8) for n_, i, D in (("q", 0, K), ("k", 1, K), ("v", 2, Vd), ("out", 3, Vd), ("y", 8, Vd), ("gate", 9, Vd))}),
                         ("ws-1", dict(short=1)), ("chunk=32", dict(chunk=32))]
            variants += [(f"ldmix={ld}", dict(ld=ld)) for ld in range(cap + 1)]
        positions = sorted({-1, 0, 62, 63, 64, 127, 64 * cap - 1, 64 * cap})
        for vname, over in variants:
            a = dict(base, **over)
            say(f"VARIANT {vname}")
            state, epi = (a["mix"], a["ld"], a["S"], cap, a["P"], a["Cur"]), (a["out"], a["gate"], a["nw"], 1e-6, a["y"], a["ws"])
            dims, step_ws = (B, H, K, Vd, a["chunk"], 0.125, dt, 0x1000), lib.mhla_causal_step_ws_bytes(B, H, K, Vd, dt) - a["short"]
            for T in (0, 1, 63, 64, 65, 130, 64 * cap, 64 * cap + 1):
                call(f"INIT T={T}", "mhla_causal_state_init", a["k"], a["v"], *state, B, T, H, K, Vd, a["chunk"], dt, 0x1000)
            for pos in positions:
                call(f"STEP pos={pos}", "mhla_causal_step", a["q"], a["k"], a["v"], *state, pos, *epi, step_ws, *dims)
                for anyb in (0, 1):
                    call(f"STEP_RAGGED max_pos={pos} any_boundary={anyb}", "mhla_causal_step_ragged", a["q"], a["k"], a["v"], *state, a["pos_dev"], pos, anyb,
                         *epi, step_ws, *dims)
            cs = at(16), at(17)
            ropes = [("none", None, None, K // 2, 64 * cap), ("both", *cs, K // 2, 64 * cap), ("cos only", cs[0], None, K // 2, 64 * cap),
                     ("sin only", None, cs[1], K // 2, 64 * cap), ("off8", cs[0] + 8, cs[1], K // 2, 64 * cap), ("off4", cs[0], cs[1] + 4, K // 2, 64 * cap),
                     ("ld short", *cs, K // 2 - 4, 64 * cap), ("ld odd", *cs, K // 2 + 2, 64 * cap), ("rows short", *cs, K // 2, 64 * cap - 1),
                     ("rows wide", *cs, K // 2 + 4, 1 << 31)]
            for fmap, (rname, cos, sin, ldt, rows) in itertools.product((0, 1, 2, 3), ropes):
                call(f"STEP_DEV fmap={fmap} rope={rname}", "mhla_causal_step_dev", a["q"], a["k"], a["v"], *state, a["pos_dev"], a["full_dev"], cos, sin, ldt, rows,
                     fmap, *epi, step_ws, *dims)
            for T in (1, 2, 63, 64, 65, 130, 65536):
                for pos in positions:
                    xws = lib.mhla_causal_extend_ws_bytes(B, T, H, K, Vd, pos, dt)
                    call(f"EXTEND pos={pos} T={T} ws={xws}", "mhla_causal_extend", a["q"], a["k"], a["v"], *state, pos, T, *epi, xws - a["short"], *dims)
                most = (T + 62) // 64
                for max_end, later, close, left in itertools.product((-1, 0, 1, 63, 64, 65, 64 * cap, 64 * cap + 1), sorted({0, 1, most, most + 1}), (0, 1), (0, 1)):
                    xws = lib.mhla_causal_extend_ragged_ws_bytes(B, T, H, K, Vd, later, dt)
                    call(f"EXTEND_RAGGED T={T} max_end={max_end} max_later={later} any_close={close} left={left} ws={xws}", "mhla_causal_extend_ragged",
                         a["q"], a["k"], a["v"], *state, a["pos_dev"], a["ntok_dev"], T, max_end, later, close, left, *epi, xws - a["short"], *dims)
        decode_forms(call, lib, L, base, B, H, K, Vd, dt, cap)
    return call.n


def decode_forms(call, lib, L, base, B, H, K, Vd, dt, cap):
    """The forms of the ragged entry points at one (shape, dtype, capacity) -- grouped-query, slots, pages, h16 pages, packed tokens -- the
    commit, the pack prefill and the swap, on a thinner grid of positions and token counts than the calls above.  A variant names the
    forms it bears on: a null slot map is tried on the forms that take one."""
    NV = L.NULL_VIEW
    base = dict(base, Hkv=H, slot_dev=at(26), n_slots=B + 3, table_dev=at(27), pages=at(28), n_pages=B * cap + 2, page_mult=at(29), off_dev=at(30),
                accept_dev=at(31), seq_len_dev=at(32), chunk_tab_dev=at(33), chunk_dst_dev=at(34), items_dev=at(35), blob=at(36), n_seqs=B, n_chunks=None)
    POOLS, ALL = ("slots", "paged", "paged_h16", "packed"), ("gqa", "slots", "paged", "paged_h16", "packed", "init", "swap", "rotary")
    variants = [("", {}, ALL), ("packed dense", dict(table_dev=None), ("packed",)), ("packed rows", dict(table_dev=None, slot_dev=None), ("packed", "rotary")),
                ("packed pages, no slots", dict(slot_dev=None), ("packed",)), ("Hkv=H/2", dict(Hkv=max(1, H // 2)), ALL[:5] + ("rotary",))]
    if H == 64:
        variants += [("Hkv=3", dict(Hkv=3), ALL[:5] + ("rotary",)), ("Hkv=4", dict(Hkv=4), ALL[:5])]   # (Hkv not dividing H; G = 16 above the 8 a group holds)
    if H == 2:   # (the variants on the smaller batch)
        on = dict(slot_dev=POOLS + ("init", "rotary"), table_dev=POOLS[1:] + ("init",), pages=POOLS[1:] + ("init", "swap"), page_mult=("paged_h16", "init", "swap"),
                  off_dev=("packed", "rotary"), accept_dev=ALL[1:5], seq_len_dev=("init",), chunk_tab_dev=("init",), chunk_dst_dev=("init",), items_dev=("swap",),
                  blob=("swap",), S=("gqa", "slots", "packed", "init"), P=ALL[:7], Cur=ALL[:7], pos_dev=ALL, full_dev=ALL[:4] + ("swap",), ntok_dev=ALL[:3] + ("rotary",),
                  ws=ALL[:6], mix=ALL[:6])
        variants += [(f"{name}={'null' if o is None else 'off' + str(o)}", {name: None if o is None else base[name] + o}, kinds)
                     for name, kinds in on.items() for o in ((None,) if name == "mix" else (None, 4) if name == "chunk_tab_dev" else (None, 8) if name in ("S", "P", "Cur", "pages", "blob", "ws") else (None, 2))]
        variants += [(f"{name}=0", {name: 0}, kinds) for name, kinds in (("n_slots", POOLS + ("init", "swap", "rotary")), ("n_pages", POOLS[1:] + ("init", "swap")),
                                                                        ("n_seqs", ("init", "swap")), ("n_chunks", ("init",)))]
        variants += [("Hkv=3", dict(Hkv=3), ALL[:5] + ("rotary",)), ("no y", dict(y=NV, gate=NV, nw=None), ALL[:5]), ("no out", dict(out=NV), ALL[:5]),
                     ("ws-1", dict(short=1), ALL[:6]), ("chunk=32", dict(chunk=32), ALL[:6]), ("ldmix=cap-1", dict(ld=cap - 1), ALL[:6])]
    positions = sorted({-1, 0, 63, 64 * cap - 1, 64 * cap})
    cs = at(16), at(17)
    for vname, over, kinds in variants:
        a = dict(base, **over)
        Hkv = a["Hkv"]
        say(f"FORMS {vname}")
        q, k, v = a["q"], a["k"], a["v"]
        ragged = (a["mix"], a["ld"], a["S"], cap, a["P"], a["Cur"], a["pos_dev"])
        paged_at = lambda *pages: (a["mix"], a["ld"], *pages, a["n_pages"], a["table_dev"], cap, a["P"], a["Cur"])   # noqa: E731
        slot = (a["slot_dev"], a["n_slots"])
        states = dict(gqa=ragged, slots=ragged + slot, paged=paged_at(a["pages"]) + (a["pos_dev"],) + slot,
                      paged_h16=paged_at(a["pages"], a["page_mult"]) + (a["pos_dev"],) + slot, packed=paged_at(a["S"] if a["table_dev"] is None else a["pages"]) + (a["pos_dev"],) + slot)
        names = dict(gqa=("step_ragged_gqa", "step_dev_gqa", "extend_ragged_gqa", "verify_ragged_gqa", "commit_ragged"), slots=("step_slots", "step_dev_slots", "extend_slots", "verify_slots", "commit_slots"),
                     paged=("step_paged", "step_dev_paged", "extend_paged", "verify_paged", "commit_paged"), paged_h16=("step_paged_h16", "step_dev_paged_h16", None, None, None),
                     packed=(None, None, "extend_packed", "verify_packed", "commit_packed"))
        epi = (a["out"], a["gate"], a["nw"], 1e-6, a["y"], a["ws"])
        dims, step_ws = (B, H, Hkv, K, Vd, a["chunk"], 0.125, dt, 0x1000), lib.mhla_causal_step_ws_bytes(B, H, K, Vd, dt) - a["short"]
        for kind in (kd for kd in ALL[:5] if kd in kinds):
            state, (step, step_dev, extend, verify, commit) = states[kind], names[kind]
            if step:
                for pos, anyb in itertools.product(positions, (0, 1)):
                    call(f"{step} max_pos={pos} any_boundary={anyb}", "mhla_causal_" + step, q, k, v, *state, pos, anyb, *epi, step_ws, *dims)
                for fmap, cos, sin in ((0, None, None), (2, None, None), (1, *cs), (0, cs[0], None), (3, None, None)):
                    call(f"{step_dev} fmap={fmap} rope={int(bool(cos))}{int(bool(sin))}", "mhla_causal_" + step_dev, q, k, v, *state, a["full_dev"], cos, sin, K // 2, 64 * cap, fmap,
                         *epi, step_ws, *dims)
            if not extend:
                continue
            pk = kind == "packed"
            for T in (0, 1, 130, 65536):
                most = (T + 62) // 64
                for max_end, later, close, left in itertools.product((-1, 0, 65, 64 * cap, 64 * cap + 1), sorted({0, most, most + 1}), (0, 1), (0,) if pk else (0, 1)):
                    if pk:
                        xws, tok = lib.mhla_causal_extend_packed_ws_bytes(B, T, H, Hkv, K, Vd, later, dt), (a["off_dev"], T, max_end, later, close)
                    else:
                        xws, tok = lib.mhla_causal_extend_ragged_gqa_ws_bytes(B, T, H, Hkv, K, Vd, later, dt), (a["ntok_dev"], T, max_end, later, close, left)
                    tag = f"T={T} max_end={max_end} max_later={later} any_close={close} left={left} ws={xws}"
                    call(f"{extend} {tag}", "mhla_causal_" + extend, q, k, v, *state, *tok, *epi, xws - a["short"], *dims)
                    call(f"{verify} {tag}", "mhla_causal_" + verify, q, k, v, *state, *tok, *epi, xws - a["short"], *dims)
                    if kind == "gqa" and Hkv != H:
                        continue   # (the commit has no grouped form of its own: it runs on the k/v heads)
                    cws = lib.mhla_causal_commit_ragged_ws_bytes(B, dt)
                    call(f"{commit} {tag} cws={cws}", "mhla_causal_" + commit, k, v, *state, tok[0], a["accept_dev"], *tok[1:], a["ws"], cws - a["short"],
                         *((B, Hkv) if pk else (B, H)), K, Vd, a["chunk"], dt, 0x1000)
        if "init" in kinds:   # the pack prefill: a pack of T tokens in n_chunks chunks (default: as few as hold them)
            for T, max_len in ((0, 0), (1, 1), (130, 65), (130, 131), (64 * cap + 64, 64 * cap), (64 * cap + 64, 64 * cap + 1)):
                for nc in ((a["n_chunks"],) if a["n_chunks"] is not None else sorted({(T + 63) // 64, (T + 63) // 64 + 1, (T + 63) // 64 - 1, T + 1})):
                    tail = (max_len, T, H, K, Vd, a["chunk"], nc, a["chunk_tab_dev"], a["chunk_dst_dev"])
                    seqs, dense = (a["n_seqs"], a["seq_len_dev"]), (a["mix"], a["ld"], a["S"], cap, a["P"], a["Cur"])
                    tag = f"T={T} max_len={max_len} n_chunks={nc}"
                    call(f"varlen_state_init {tag}", "mhla_causal_varlen_state_init", k, v, *dense, *seqs, *tail, dt, 0x1000)
                    call(f"varlen_state_init_slots {tag}", "mhla_causal_varlen_state_init_slots", k, v, *dense, *seqs, *slot, *tail, dt, 0x1000)
                    call(f"varlen_state_init_paged {tag}", "mhla_causal_varlen_state_init_paged", k, v, *paged_at(a["pages"]), *seqs, *slot, *tail, dt, 0x1000)
                    for hws in sorted({lib.mhla_causal_varlen_state_init_paged_h16_ws_bytes(n_, H, K, Vd, dt) for n_ in (nc, 1, 2)}):
                        call(f"varlen_state_init_paged_h16 {tag} ws={hws}", "mhla_causal_varlen_state_init_paged_h16", k, v, *paged_at(a["pages"], a["page_mult"]), *seqs, *slot,
                             *tail, a["ws"], hws - a["short"], dt, 0x1000)
        if "swap" in kinds:   # item ranges inside, empty and outside a list of n_seqs sequences and 3 pages; fp32 pages (no multipliers) and h16
            n_seqs, moved = a["n_seqs"], 3
            for mult, (i0, i1) in itertools.product((None, a["page_mult"]), ((0, n_seqs + moved), (0, 1), (n_seqs, n_seqs + 1), (1, n_seqs + 1), (2, 2), (-1, 1), (2, 1), (0, n_seqs + moved + 1))):
                for fd in (a["full_dev"], None):
                    say(f"SWAP ws={lib.mhla_causal_swap_ws_bytes(n_seqs, moved, Hkv, K, Vd, 0 if mult is None else 1)}")
                    for d in ("out", "in"):
                        call(f"swap_{d} mult={int(mult is not None)} full={int(fd is not None)} items=[{i0},{i1})", f"mhla_causal_swap_{d}_paged", a["pages"], mult, a["n_pages"], a["P"],
                             a["Cur"], a["pos_dev"], fd, a["n_slots"], a["items_dev"], n_seqs, moved, i0, i1, a["blob"], Hkv, K, Vd, 0x1000)
        if "rotary" in kinds:   # the decode prologue (capi_misc.hip): padded windows and packed tokens, with and without a slot map
            yq, yk = L.View(at(37), 1 << 24, H * K, K), L.View(at(38), 1 << 24, Hkv * K, K)
            for T, fmap, (ntok, off, left) in itertools.product((0, 1, 130), (0, 2, 3), ((a["ntok_dev"], None, 0), (a["ntok_dev"], None, 1), (None, None, 0), (None, a["off_dev"], 0),
                                                                                       (a["ntok_dev"], a["off_dev"], 0), (None, a["off_dev"], 1))):
                for cos, sin, ldt in ((*cs, K // 2), (cs[0], None, K // 2), (cs[0] + 8, cs[1], K // 2), (*cs, K // 2 + 2), (*cs, K // 2 + 4)):
                    call(f"rotary_decode T={T} fmap={fmap} ntok={int(bool(ntok))} off={int(bool(off))} left={left} cos={cos and hex(cos)} sin={int(bool(sin))} ld_tab={ldt}",
                         "mhla_featmap_rotary_decode", q, k, cos, sin, ldt, 64 * cap, a["pos_dev"], a["slot_dev"], a["n_slots"], ntok, off, T, left, yq, yk, B, H, Hkv, K, fmap, dt, 0x1000)


if __name__ == "__main__":
    build(sys.argv[2], sys.argv[3]) if sys.argv[1] == "build" else run(sys.argv[2], sys.argv[3:])
