// Shared host-side helpers of the C ABI translation units (capi*.hip): error string, launch wrapper with the per-launch event
// hook, argument checks, workspace carving, dtype / head-dim dispatch.  The library is built from several translation units
// compiled in parallel (mhla_amd/build.py); state that must be one per library is an inline variable here.
#pragma once
#include "../../include/mhla_hip.h"

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"

namespace mhla {
namespace capi {


inline thread_local char g_err[512] = "";

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

inline size_t al4(size_t n) { return (n + 3) & ~(size_t)3; }

// Optional per-launch timing (mhla_prof_*): hipEvents recorded on the launch stream around every
// kernel, so bench.py can report each kernel's average duration live (not only rocprof offline).
struct ProfRec { const char* name; hipEvent_t e0, e1; };
inline std::mutex g_prof_mu;
inline std::atomic<bool> g_prof_on{false};
inline std::vector<ProfRec> g_prof;

template <typename K>
int launch(K kernel, dim3 grid, dim3 block, size_t smem, hipStream_t stream, const char* name, auto... args) {
    if (smem > 48 * 1024) {
        // opt in to > 48 KB of dynamic LDS once per (kernel, device); the driver call is kept off the steady-state launch path
        static std::mutex mu;
        static std::map<std::pair<const void*, int>, size_t> done;
        int dev = 0;
        (void)hipGetDevice(&dev);
        const std::pair<const void*, int> key(reinterpret_cast<const void*>(kernel), dev);
        std::lock_guard<std::mutex> lk(mu);
        auto it = done.find(key);
        if (it == done.end() || it->second < smem) {
            hipError_t e = hipFuncSetAttribute(key.first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
            if (e != hipSuccess) return fail(MHLA_ELAUNCH, "%s: hipFuncSetAttribute(%zu B LDS): %s", name, smem, hipGetErrorString(e));
            done[key] = smem;
        }
    }
    ProfRec rec{name, nullptr, nullptr};
    const bool prof = g_prof_on;
    if (prof) {
        (void)hipEventCreate(&rec.e0);
        (void)hipEventCreate(&rec.e1);
        (void)hipEventRecord(rec.e0, stream);
    }
    hipLaunchKernelGGL(kernel, grid, block, smem, stream, args...);
    if (prof) {
        (void)hipEventRecord(rec.e1, stream);
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_prof.push_back(rec);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MHLA_ELAUNCH, "%s: launch failed: %s", name, hipGetErrorString(e));
    return MHLA_OK;
}

// debugging aid: per-workgroup phase timestamps of the tile kernels (mhla_debug_set_trace)
inline std::atomic<unsigned long long*> g_trace{nullptr};

// h16 summaries of 129 .. 256 blocks: the re-cut resident mixing kernel (mixh2.hpp k_sp_mixh2: the rescaled weights kept per (b, h)) serves
// launches whose workgroups get at least this many 64-element slices each -- fewer do not pay for its rebuilds (bm_plan below)
#ifndef SP_MIXH2_MIN_SLICES
#define SP_MIXH2_MIN_SLICES 8
#endif
#ifndef SP_MIXH2_TE
#define SP_MIXH2_TE 64   // slice width of k_sp_mixh2 in summary elements
#endif
// (mhla_set_option("recut_kernels", 0): the kernels they replaced -- k_sp_mixh at twelve / sixteen waves, the block-per-workgroup Wan output
// kernel, the loop forms of the one-tile token kernels (bm_one_tile below), k_sp_state with the stand-in third stream -- for A/B timing and for the bit-equality tests; MHLA_WAN_FLAT=0 / MHLA_RECUT=0 in the environment set the start value)
inline std::atomic<int> g_recut{[] { const char* e = getenv("MHLA_RECUT"); const char* f = getenv("MHLA_WAN_FLAT"); return ((e && e[0] == '0') || (f && f[0] == '0')) ? 0 : 1; }()};
inline bool sp_mixh2_applies(int M, long E, long BH, long S = 0) {
    if (M <= 128 || M > 256 || !g_recut.load()) return false;
    // (its buffer descriptors address 32-bit byte offsets: the (b, h)'s summary rows -- E / 2 + 288 floats each -- and normaliser rows must fit)
    if (BH * M * (E / 2 + 288) * 4 >= (1L << 31) || BH * M * S * 4 >= (1L << 31)) return false;
    const long total = BH * ((E + SP_MIXH2_TE - 1) / SP_MIXH2_TE), wgs = std::min<long>(total, 256);
    return wgs > 0 && (total + wgs - 1) / wgs >= SP_MIXH2_MIN_SLICES;
}
// The split-operand token kernels walk a block's 16-token tiles four waves abreast: with at most 64 tokens per block a wave has one tile
// at the most, and the instantiations without the tile loop and its look-ahead serve the launch ("recut_kernels" 0: the loop kernels)
inline bool bm_one_tile(int S) { return S <= 64 && g_recut.load(); }
// mhla_set_option("fp32_summaries") / MHLA_FP32_SUMMARIES=1 (read once): the resident-mixing pipeline keeps its summaries as fp32 instead of 24-bit floats
inline std::atomic<int> g_no_p24{[] { const char* e = getenv("MHLA_FP32_SUMMARIES"); return (e && e[0] == '1') ? 1 : 0; }()};

inline View cv(const mhla_view& v) { return View{v.ptr, (long)v.sb, (long)v.sn, (long)v.sh}; }
inline MView cmv(const mhla_mview& v) { return MView{v.ptr, (long)v.sb, (long)v.sn, (long)v.sh}; }

inline int check_view(const char* name, const void* ptr, int64_t sb, int64_t sn, int64_t sh, int dtype) {
    if (!ptr) return fail(MHLA_EINVAL, "%s: null pointer", name);
    const int esz = dtype == MHLA_F32 ? 4 : 2;
    if (((uintptr_t)ptr) % (4 * esz) != 0) return fail(MHLA_EINVAL, "%s: pointer not %d-byte aligned", name, 4 * esz);
    if ((sb | sn | sh) & 3) return fail(MHLA_EINVAL, "%s: strides (%lld, %lld, %lld) must be multiples of 4 elements", name,
                                        (long long)sb, (long long)sn, (long long)sh);
    return MHLA_OK;
}
#define CHECK_VIEW(v) do { int rc_ = check_view(#v, (v).ptr, (v).sb, (v).sn, (v).sh, dtype); if (rc_) return rc_; } while (0)
#define RC(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

// E-slices of the dW GEMM so that the launch has ~1000+ workgroups (at most 16 slices, slices >= 256 columns)
constexpr int DW_MAX_SPLIT = 16;
inline int dw_splits(long wgs, long E) {
    long ns = (1024 + wgs - 1) / wgs;
    if (ns > DW_MAX_SPLIT) ns = DW_MAX_SPLIT;
    while (ns > 1 && E / ns < 256) --ns;
    return (int)(ns < 1 ? 1 : ns);
}

inline int dt_for(int D) { return D <= 32 ? 2 : D <= 64 ? 4 : D <= 80 ? 5 : D <= 96 ? 6 : D <= 128 ? 8 : 0; }

// dispatch on (dtype, DT)
#define DISPATCH_T(dtype, ...)                                                   \
    switch (dtype) {                                                             \
        case MHLA_F32: { using ET = float; __VA_ARGS__; break; }                  \
        case MHLA_BF16: { using ET = bf16_t; __VA_ARGS__; break; }                \
        case MHLA_F16: { using ET = f16_t; __VA_ARGS__; break; }                  \
        default: return fail(MHLA_EINVAL, "unknown dtype %d", dtype);            \
    }
#define DISPATCH_DT(dt, ...)                                                     \
    switch (dt) {                                                                \
        case 2: { constexpr int DT = 2; __VA_ARGS__; break; }                    \
        case 4: { constexpr int DT = 4; __VA_ARGS__; break; }                    \
        case 5: { constexpr int DT = 5; __VA_ARGS__; break; }                    \
        case 6: { constexpr int DT = 6; __VA_ARGS__; break; }                    \
        case 8: { constexpr int DT = 8; __VA_ARGS__; break; }                    \
        default: return fail(MHLA_ENOTSUP, "head dim tile %d not supported", dt);\
    }

// (the summary format of a call: the SF_* values of common.hpp, picked by bm_sumfmt below)
struct BmWs {
    float *kv, *g, *z, *ksum, *ninv, *dg, *dkv, *dn, *dz, *dks, *dwp;
    unsigned short* olo;   // forward region: O - fl(O) as bf16 [bh][M S][D] (16-bit tensors at the default arithmetic), or null
    size_t total_fwd, total_bwd;
    long es;   // from one block's D x D summary to the next, in floats (SF_BF16: in 16-bit elements): the format's row + padding
    int fmt;   // SF_*
};
// sum16: the D x D block summaries (KV, G, dG, dKV) are stored as bf16 (split-operand path on bf16 tensors): half the floats
// padded (split-operand path): every summary row carries 1152 bytes of padding.  The mixing and dW kernels read the same 128-byte
// piece of EVERY block's summary at once, i.e. at the row stride: at a power-of-two stride (8 KB at D = 64 bf16, 64 KB at D = 128
// fp32) those requests fall on a fraction of the HBM channels -- k_sp_dwr ran at 3.7 TB/s at D = 64 and at 4.9 / 5.4 TB/s at
// D = 56 / 72 (the causal pipeline met the same effect, causal_bf16.hpp).  The generic fp32-MFMA kernels keep dense rows.
inline long bm_row_elems(int D, int fmt, bool padded) {
    const long E = (long)D * D;
    switch (fmt) {
        case SF_BF16: return E + (padded ? 576 : 0);        // (16-bit elements)
        case SF_P24: return 3 * E / 4 + 288;                // two planes: E x u16, E x u8
        case SF_H16: return E / 2 + 288;                    // E x fp16; the row's multiplier is the first word of the padding.  (Rows must start on
                                                            // 128-byte lines: with 16 bytes more every 256-byte slice piece of the mixing kernels
                                                            // straddled three lines instead of two -- 1.67x the reads, 1.23x the writes in the counters)
        default: return E + (padded ? 288 : 0);
    }
}
inline BmWs bm_carve(void* ws, int B, int H, int M, int S, int D, int fmt, bool padded, bool olo = false) {
    const size_t es = (size_t)bm_row_elems(D, fmt, padded);
    // (every region starts on a 128-byte line -- 32 floats -- so that the summary rows, whose stride is a whole number of lines, do too)
    auto al32 = [](size_t n) { return (n + 31) & ~(size_t)31; };
    const size_t bh = (size_t)B * H, st = al32(fmt == SF_BF16 ? (bh * M * es + 1) / 2 : bh * M * es), zs = al32(bh * M * S), ks = al32(bh * M * D);
    float* p = (float*)ws;
    BmWs w;
    w.fmt = fmt;
    w.es = (long)es;
    w.kv = p; p += st;
    w.g = p; p += st;
    w.z = p; p += zs;
    w.ksum = p; p += ks;
    w.ninv = p; p += zs;
    w.olo = nullptr;
    if (olo) { w.olo = (unsigned short*)p; p += al32((bh * M * S * D + 1) / 2); }
    w.total_fwd = (size_t)(p - (float*)ws) * 4;
    w.dg = p; p += st;
    w.dkv = p; p += st;
    w.dn = p; p += zs;
    w.dz = p; p += zs;
    w.dks = p; p += ks;
    // dW partials: (b, h) x E-slices of k_sp_dw / k_dw, or one per workgroup of the fused mixing + dW kernel (<= 512; <= 1024 of up to 32 x 32 at two waves) + one per (b, h)
    w.dwp = p; p += al4(std::max(bh * DW_MAX_SPLIT, M <= 32 ? bh + 1024 : M <= 128 ? bh + 512 : (size_t)0) * M * M);
    w.total_bwd = (size_t)(p - (float*)ws) * 4;
    return w;
}

inline bool view_ok16(const mhla_view& v) { return v.ptr && ((uintptr_t)v.ptr % 16) == 0 && ((v.sb | v.sn | v.sh) & 7) == 0; }
// split-bf16 MFMA kernels (split.hpp): head dims that are multiples of 8, any dtype
inline bool sp_shape_ok(int D, unsigned flags) { return (D & 7) == 0 && !(flags & MHLA_FLAG_FORCE_GENERIC); }
inline bool view_ok16m(const mhla_mview& v) { return v.ptr && ((uintptr_t)v.ptr % 16) == 0 && ((v.sb | v.sn | v.sh) & 7) == 0; }
// bf16 block summaries (and single-bf16 intermediate operands): only when the caller asked for them (MHLA_FLAG_BF16_SUMMARIES)
inline bool bm_sum16(int D, int dtype, unsigned flags) { return dtype == MHLA_BF16 && sp_shape_ok(D, flags) && (flags & MHLA_FLAG_BF16_SUMMARIES); }
// The summary format of a block-mix call on the generic / split-operand path.  h16 and p24 live on the resident-mixing pipeline
// (split.hpp k_sp_mixr: up to 256 blocks, summaries of whole 64-element slices):
//   h16: 16-bit tensors, head dims 32 .. 96, 4 .. 256 blocks (up to 128: dW fused into the mixing; beyond: k_sp_dwr) of at least 16 tokens (11-bit summaries lean on averaging
//        over the block, the head dim and the blocks: in the model, tools/sim_h16.py, 2 blocks reach 5e-3 in dW -- a difference
//        of nearly equal terms there -- head dim 8 reaches 7e-4, a 2 x 1-token case 1.4e-3; inside the rule: <= 6e-4) -- unless
//        the caller asks for >= 16 significand bits
//        (MHLA_FLAG_FP32_GRADE_SUMMARIES) or the process keeps fp32 words ("fp32_summaries");
//   p24: the same 16-bit shapes when h16 is declined, and fp32 tensors at head dims 97 .. 128 with up to 192 blocks (the Wan shape).
inline int bm_sumfmt(int M, int S, int D, int dtype, unsigned flags) {
    if (!sp_shape_ok(D, flags)) return SF_F32;
    if (bm_sum16(D, dtype, flags)) return SF_BF16;
    const bool mixr = M <= 256 && ((long)D * D) % 64 == 0;
    if (!mixr || g_no_p24.load()) return SF_F32;
    if (dtype != MHLA_F32 && D <= 96 && S >= 16 && M >= 4 && D >= 32 && !(flags & MHLA_FLAG_FP32_GRADE_SUMMARIES)) return SF_H16;   // (M <= 256: mixr)
    if (dtype != MHLA_F32 && D <= 96 && M <= 128) return SF_P24;
    if (dtype == MHLA_F32 && D > 96 && M <= 192) return SF_P24;
    return SF_F32;
}
// 16-bit tensors on the h16 / p24 pipeline with head dims up to 64: the backward forms its row dots dO . O from G_i itself --
// dO' . (Q_i G_i), one more small product in k_sp_state<1> -- and reads neither the stored output nor a residual of it
inline bool bm_rowdots_from_g(int M, int S, int D, int dtype, unsigned flags) {
    const int f = bm_sumfmt(M, S, D, dtype, flags);
    return dtype != MHLA_F32 && (f == SF_H16 || f == SF_P24) && D <= 64;
}
// other 16-bit tensors at the default arithmetic: the forward keeps what its store of O rounded away (BmWs::olo) for the backward
inline bool bm_olo(int M, int S, int D, int dtype, unsigned flags) { return dtype != MHLA_F32 && !bm_sum16(D, dtype, flags) && !bm_rowdots_from_g(M, S, D, dtype, flags); }
// (MHLA_FLAG_NO_BWD_STATE: the forward neither writes nor carves the O-residual region)
inline bool bm_fwd_olo(int M, int S, int D, int dtype, unsigned flags) { return bm_olo(M, S, D, dtype, flags) && !(flags & MHLA_FLAG_NO_BWD_STATE); }
// the workspace of the generic / split-operand family: the forward's view of it (`fwd`: without a residual region the forward was told not to keep) or the backward's
inline BmWs bm_carve_for(void* ws, int B, int H, int M, int S, int D, int dtype, unsigned flags, bool fwd) {
    return bm_carve(ws, B, H, M, S, D, bm_sumfmt(M, S, D, dtype, flags), sp_shape_ok(D, flags), fwd ? bm_fwd_olo(M, S, D, dtype, flags) : bm_olo(M, S, D, dtype, flags));
}
// the bf16-summary fast path (fused.hpp): its summaries are single bf16 values, so it serves the opt-in arithmetic only
inline bool fast_shape_ok(int M, int D, int dtype, bool split, unsigned flags) {
    return dtype == MHLA_BF16 && D == 64 && M <= 64 && !split && (flags & MHLA_FLAG_BF16_SUMMARIES);
}
// small-sequence single-launch path (smalln.hpp: bf16 tensors; smalln_f32.hpp: fp32 tensors as hi + lo bf16 operands): S = 16 tokens per block, at most 16 blocks, D <= 80
inline bool sn_shape_ok(int M, int S, int D, bool split) { return S == 16 && M <= 16 && D <= 80 && (D & 7) == 0 && !split; }

// ---- The route: the kernel family a block-mix problem is eligible for.  Every entry point, size query and the description ask
// this one function -- the only place where MHLA_FLAG_FORCE_GENERIC and MHLA_FLAG_NO_SMALLN are held against the families -- so that a
// forward, the backward that reuses its workspace, the workspace bounds and the dispatch table cannot disagree.
enum BmRoute { BM_SNF,     // small-sequence fp32
               BM_SN,      // small-sequence bf16
               BM_FAST,    // bf16 fast path
               BM_TYPED }; // split-operand or generic (capi_bm_typed.hpp; BmPlan below)
inline BmRoute bm_route(int M, int S, int D, int dtype, bool split, unsigned flags) {
    const bool generic = (flags & MHLA_FLAG_FORCE_GENERIC) != 0, smalln = !generic && !(flags & MHLA_FLAG_NO_SMALLN) && sn_shape_ok(M, S, D, split);
    if (smalln && dtype == MHLA_F32) return BM_SNF;
    if (smalln && dtype == MHLA_BF16) return BM_SN;
    return !generic && fast_shape_ok(M, D, dtype, split, flags) ? BM_FAST : BM_TYPED;
}
// the problem may leave or find the fast path's workspace layout and error word (also where the small-sequence family wins: the bounds cover both)
inline bool bm_fast_layout(int M, int S, int D, int dtype, bool split, unsigned flags) { return bm_route(M, S, D, dtype, split, flags | MHLA_FLAG_NO_SMALLN) == BM_FAST; }

inline int ws_too_small(size_t have, size_t need) { return fail(MHLA_EINVAL, "workspace too small: %zu < %zu bytes", have, need); }
// the rotary tables of the four entry points that take them (`required`: the rope pair; the Wan pair takes none or both)
inline int check_rope(const float* rcos, const float* rsin, int64_t ld, int D, bool required) {
    if (required && (!rcos || !rsin)) return fail(MHLA_EINVAL, "rope tables null");
    if ((rcos == nullptr) != (rsin == nullptr)) return fail(MHLA_EINVAL, "rope_cos and rope_sin must be given together");
    if (rcos && (ld < D / 2 || (ld & 3) || ((uintptr_t)rcos | (uintptr_t)rsin) % 16))
        return fail(MHLA_EINVAL, "rope tables: ld=%lld must be >= D/2, a multiple of 4, and the tables 16-byte aligned", (long long)ld);
    return MHLA_OK;
}
inline int check_gate(const mhla_view& gate) {
    if (gate.ptr && (((uintptr_t)gate.ptr) % 8 || ((gate.sb | gate.sn | gate.sh) & 3))) return fail(MHLA_EINVAL, "gate: pointer must be 8-byte aligned, strides multiples of 4");
    return MHLA_OK;
}

inline int bm_check(int B, int H, int M, int S, int D, int dtype, unsigned flags, bool split) {
    if (B <= 0 || H <= 0 || M <= 0 || S <= 0 || D <= 0) return fail(MHLA_EINVAL, "non-positive dimension B=%d H=%d M=%d S=%d D=%d", B, H, M, S, D);
    if (D % 4) return fail(MHLA_EINVAL, "D=%d must be a multiple of 4", D);
    if (!dt_for(D)) return fail(MHLA_ENOTSUP, "block-mix head dim D=%d > 128 not supported", D);
    if (dtype < 0 || dtype > 2) return fail(MHLA_EINVAL, "unknown dtype %d", dtype);
    if (flags & ~(MHLA_FLAG_RELU_EPS | MHLA_FLAG_FORCE_GENERIC | MHLA_FLAG_NO_SMALLN | MHLA_FLAG_BF16_SUMMARIES | MHLA_FLAG_NO_BWD_STATE | MHLA_FLAG_FP32_GRADE_SUMMARIES)) return fail(MHLA_EINVAL, "unknown flags 0x%x", flags);
    if ((flags & MHLA_FLAG_BF16_SUMMARIES) && (flags & MHLA_FLAG_FP32_GRADE_SUMMARIES)) return fail(MHLA_EINVAL, "MHLA_FLAG_BF16_SUMMARIES and MHLA_FLAG_FP32_GRADE_SUMMARIES exclude each other");
    if ((flags & MHLA_FLAG_BF16_SUMMARIES) && dtype == MHLA_F16) return fail(MHLA_EINVAL, "MHLA_FLAG_BF16_SUMMARIES (single-bf16 summaries) serves bf16 tensors only");
    if ((flags & MHLA_FLAG_RELU_EPS) && split) return fail(MHLA_EINVAL, "MHLA_FLAG_RELU_EPS needs q_den/k_den to alias q_num/k_num");
    if ((size_t)B * H > 65535) return fail(MHLA_ENOTSUP, "B*H=%zu exceeds grid limit 65535", (size_t)B * H);
    return MHLA_OK;
}

// One block-mix call: what capi.hip's entry points validated, handed to the family that serves it -- the small-sequence and fast paths
// in capi.hip, the generic / split-operand path in the per-dtype translation units (capi_bm_f32.hip, capi_bm_bf16.hip, capi_bm_f16.hip
// instantiate bm_fwd_typed / bm_bwd_typed for their element type).
struct BmCall {
    mhla_view q_num, k_num, v, q_den, k_den, outv, dout, gate;
    mhla_mview out, dq_num, dk_num, dv, dq_den, dk_den;
    const float* W; int ldw; float* dW;
    const int32_t* block_index;
    BmWs w;
    int B, H, M, S, D, dtype; float eps; unsigned flags;
    bool normalize, split, reuse, epi;
    hipStream_t st;
    const float *rcos, *rsin; long ldr;
    const float* nw; float neps; int out_dtype;
    unsigned short* olo_own;   // backward: the O-residual region of the backward's OWN workspace (w.olo may point into the kept forward workspace)
    int relu() const { return (flags & MHLA_FLAG_RELU_EPS) ? 1 : 0; }
};
// the 16-byte view test of the families that load whole 16-byte pieces: the forward's view set, or the backward's
inline bool bm_views_ok16(const BmCall& c, bool bwd) {
    if (!(view_ok16(c.q_num) && view_ok16(c.k_num) && view_ok16(c.v))) return false;
    if (!bwd) return view_ok16m(c.out);
    return view_ok16(c.dout) && (!c.normalize || view_ok16(c.outv)) && view_ok16m(c.dq_num) && view_ok16m(c.dk_num) && view_ok16m(c.dv);
}
// the family this CALL takes: the route's, when its views allow it (a rotary prologue or fused epilogue excludes the special families)
inline BmRoute bm_call_route(const BmCall& c, bool bwd) {
    const BmRoute r = bm_route(c.M, c.S, c.D, c.dtype, c.split, c.flags);
    return r != BM_TYPED && !c.rcos && !c.epi && bm_views_ok16(c, bwd) ? r : BM_TYPED;
}
// kernel names as launch() reports them and mhla_describe_dispatch prints them: one table per family
inline const char* bm_sn_name(BmRoute r, bool bwd, int D, bool hl) {
    static const char* const snf[2][2] = {{"k_snf_fwd<4>", "k_snf_fwd<5>"}, {"k_snf_bwd<4>", "k_snf_bwd<5>"}};
    static const char* const sn[2][2][2] = {{{"k_sn_fwd<4>", "k_sn_fwd<5>"}, {"k_sn_bwd<4>", "k_sn_bwd<5>"}}, {{"k_sn_fwd<4,hl>", "k_sn_fwd<5,hl>"}, {"k_sn_bwd<4,hl>", "k_sn_bwd<5,hl>"}}};
    return r == BM_SNF ? snf[bwd][D > 64] : sn[hl][bwd][D > 64];
}
constexpr const char* N_SN_DW_REDUCE = "k_sn_dw_reduce";
// the bf16 fast path (one fused token-gradient launch; its two-launch form reports k_t16_bwd_dq / k_t16_bwd_dkv)
constexpr const char *N_FS_STATE[2] = {"k_fs_state_fwd", "k_fs_state<1>"}, *N_FS_WZ = "k_fs_wz<0>", *N_T16_OUT = "k_t16_out", *N_FS_DW = "k_fs_dw", *N_T16_BWD = "k_t16_bwd";
constexpr const char* N_WZ[2] = {"k_wz<0>", "k_wz<1>"};
constexpr const char* N_DNZ = "k_dw";   // the <dn_i, z_j> term of dW as a launch of its own
constexpr const char* N_DW_REDUCE = "k_dw_reduce";

// ---- The plan of the generic / split-operand family: every decision between the kernels of capi_bm_typed.hpp, made once per call from
// the problem (and the process options behind bm_sumfmt and sp_mixh2_applies).  bm_fwd_typed / bm_bwd_typed execute it -- their only
// branching is plan field -> template instantiation -- and mhla_describe_dispatch prints it, names included.
enum BmKern { K_NONE, K_BM_STATE, K_SP_STATE, K_S16_STATE, K_MIX, K_SP_MIX, K_SP_MIXR, K_SP_MIXR_DMA, K_SP_MIXH, K_SP_MIXH2,
              K_SP_DWR, K_SP_DW, K_SP_DWT, K_DW, K_BM_OUT, K_SP_OUT, K_S16_OUT, K_BM_TOK, K_SP_TOK, K_S16_TOK };
constexpr int mixr_slice(bool s16) { return s16 ? 128 : 64; }   // sp::mixr_te<4, FMT>() (asserted in capi_bm_typed.hpp): the slice the resident mixing needs whole
struct BmPlan {
    int fmt;             // SF_*
    bool sp;             // split-operand kernels (false: the generic fp32-MFMA ones, dense rows, nothing kept for the backward)
    bool rope, wave16;   // wave16: blocks of exactly 16 tokens, bf16, D = 64: the wave-per-block kernels of split16.hpp replace the token kernels
    BmKern state, mix[2], dw, out, tok;   // [direction]: 0 forward (KV -> G), 1 backward (dG -> dKV)
    int nw;              // waves of the resident mixing kernels (k_sp_mixr / k_sp_mixh; k_sp_mixh2: the output row tiles, 12 or 16)
    bool wz_fused;       // the normaliser's product rides in the mixing kernel
    bool wz_kernel;      // the normaliser's product is a k_wz launch of its own
    bool wz1_first;      // the backward launches that k_wz<1> before the mixing (false: behind the dW producer)
    bool dw_fused;       // dW's products ride in the backward's mixing kernel (dw == K_NONE)
    int dw_v;            // K_SP_DWR: 64-row tiles per side (2, 3, 4); K_SP_DW: the 16 / 32 block variant or 0
    bool dnz;            // the <dn_i, z_j> term of dW needs a k_dw launch of its own
    bool reduce16;       // k_dw_reduce<0, 16> whatever the number of parts
    const char *n_state[2], *n_mix[2], *n_dw, *n_out, *n_olo, *n_tok[2];
};
inline BmPlan bm_plan(long BH, int M, int S, int D, int dtype, unsigned flags, bool normalize, bool split, bool rope, bool epi, bool views16) {
    BmPlan p{};
    const long E = (long)D * D;
    p.fmt = bm_sumfmt(M, S, D, dtype, flags);
    p.sp = sp_shape_ok(D, flags);
    p.rope = rope;
    if (!p.sp) {   // (no state is kept: the backward recomputes KV, G, 1 / n)
        p.state = K_BM_STATE; p.n_state[0] = "k_bm_state<0>"; p.n_state[1] = "k_bm_state<1>";
        p.mix[0] = p.mix[1] = K_MIX; p.n_mix[0] = "k_mix<0,0>"; p.n_mix[1] = "k_mix<1,0>";
        p.wz_kernel = normalize; p.wz1_first = true;
        p.dw = K_DW; p.n_dw = "k_dw";
        p.out = K_BM_OUT; p.n_out = "k_bm_out"; p.n_olo = "k_bm_out<olo>";
        p.tok = K_BM_TOK; p.n_tok[0] = "k_bm_bwd_tok";
        return p;
    }
    const bool s16 = p.fmt == SF_BF16, h16 = p.fmt == SF_H16, p24 = h16 || p.fmt == SF_P24;
    p.wave16 = s16 && S == 16 && D == 64 && !split && !rope && !epi && views16;
    p.state = p.wave16 ? K_S16_STATE : K_SP_STATE;
    p.n_state[0] = p.wave16 ? "k_s16_state<0>" : rope ? "k_sp_state<rope>" : "k_sp_state";
    p.n_state[1] = p.wave16 ? "k_s16_state<1>" : rope ? "k_sp_state<1,rope>" : "k_sp_state<1>";
    // Resident-sequence mixing (k_sp_mixr, k_sp_mixh): up to 256 blocks (bf16 summaries: 33 and more), summaries in whole 256-byte row pieces;
    // otherwise the tiled kernel k_sp_mix.  (h16 / p24: bm_sumfmt admits resident shapes only)
    const bool mixr = (M > 32 || !s16) && M <= 256 && E % mixr_slice(s16) == 0;
    p.nw = (M <= 32 && !s16) ? 2 : M <= 64 ? 4 : M <= 128 ? 8 : M <= 192 ? 12 : 16;   // (fp32-grade summaries: two waves for up to 32 blocks)
    if (h16) {   // the mixing on the fp16 payload; up to 128 blocks with dW riding along, beyond them the re-cut kernel where it pays
        p.mix[0] = p.mix[1] = sp_mixh2_applies(M, E, BH, S) ? K_SP_MIXH2 : K_SP_MIXH;
        p.dw_fused = M <= 128;
    } else if (mixr && s16 && M > 192) {   // eight waves x 32 output blocks, LDS-DMA staging with three slices in flight
        p.mix[0] = p.mix[1] = K_SP_MIXR_DMA;
    } else if (mixr) {   // fp32 / 24-bit summaries, up to 128 blocks: dW's products ride in the backward's mixing kernel (twelve waves have no registers for them)
        p.mix[0] = p.mix[1] = K_SP_MIXR;
        p.dw_fused = !s16 && M <= 128;
    } else {
        p.mix[0] = p.mix[1] = K_SP_MIX;
    }
    const bool m2 = p.mix[0] == K_SP_MIXH2;
    p.n_mix[0] = h16 ? (m2 ? "k_sp_mixh2<0>" : "k_sp_mixh<0>") : p.mix[0] == K_SP_MIXR_DMA ? "k_sp_mixr_dma<0>" : mixr ? "k_sp_mixr<0>" : "k_sp_mix<0>";
    p.n_mix[1] = h16 ? (p.dw_fused ? "k_sp_mixh<1,dw>" : m2 ? "k_sp_mixh2<1>" : "k_sp_mixh<1>")
                     : p.mix[1] == K_SP_MIXR_DMA ? "k_sp_mixr_dma<1>" : mixr ? (p.dw_fused ? "k_sp_mixr<1,dw>" : "k_sp_mixr<1>") : "k_sp_mix<1>";
    // the normaliser's product (k_wz) rides along in the LDS-DMA mixing kernel (same weights, at most 16 values per block) and in the
    // register-staged kernels at fp32 / 24-bit / h16 summaries, as extra slices (blocks of an even number of tokens: 16- or 8-byte pieces)
    p.wz_fused = mixr && (s16 ? (M > 192 && S <= 16) : S % 2 == 0);
    p.wz_kernel = normalize && !p.wz_fused;
    p.wz1_first = !p24;
    p.reduce16 = p24;
    // dW: fused (with the <dn, z> term when the normaliser rides too); the whole-matrix kernel k_sp_dwr on 16-bit payloads of 65 .. 256
    // blocks (the <dn, z> term is one of its stages); k_sp_dwt on 24-bit summaries beyond 128 blocks; k_sp_dw otherwise
    if (p.dw_fused) {
        p.dnz = normalize && !p.wz_fused;
    } else if ((h16 || s16) && M > 64 && M <= 256 && E % 64 == 0) {
        static const char* const dwr[2][3] = {{"k_sp_dwr<2>", "k_sp_dwr<3>", "k_sp_dwr<4>"}, {"k_sp_dwr<2,h16>", "k_sp_dwr<3,h16>", "k_sp_dwr<4,h16>"}};
        p.dw = K_SP_DWR; p.dw_v = M <= 128 ? 2 : M <= 192 ? 3 : 4; p.n_dw = dwr[h16][p.dw_v - 2];
    } else if (p24) {
        p.dw = K_SP_DWT; p.n_dw = "k_sp_dwt"; p.dnz = normalize;
    } else {
        p.dw = K_SP_DW; p.dw_v = M <= 16 ? 16 : M <= 32 ? 32 : 0; p.n_dw = M <= 16 ? "k_sp_dw<16>" : M <= 32 ? "k_sp_dw<32>" : "k_sp_dw"; p.dnz = normalize;
    }
    p.out = p.wave16 ? K_S16_OUT : K_SP_OUT; p.n_out = epi ? "k_sp_out<norm>" : p.wave16 ? "k_s16_out" : "k_sp_out"; p.n_olo = "k_sp_out<olo>";
    p.tok = p.wave16 ? K_S16_TOK : K_SP_TOK;
    p.n_tok[0] = rope ? "k_sp_bwd_dq<rope>" : p.wave16 ? "k_s16_bwd_dq" : "k_sp_bwd_dq";
    p.n_tok[1] = rope ? "k_sp_bwd_dkv<rope>" : p.wave16 ? "k_s16_bwd_dkv" : "k_sp_bwd_dkv";
    return p;
}
inline BmPlan bm_plan(const BmCall& c, bool bwd) {
    return bm_plan((long)c.B * c.H, c.M, c.S, c.D, c.dtype, c.flags, c.normalize, c.split, c.rcos != nullptr, c.epi, bm_views_ok16(c, bwd) && (!bwd || view_ok16(c.outv)));
}
template <typename ET, bool S16> int bm_fwd_typed(const BmCall& c);   // S16: bf16 block summaries (bf16 tensors + MHLA_FLAG_BF16_SUMMARIES)
template <typename ET, bool S16> int bm_bwd_typed(const BmCall& c);

}  // namespace capi
}  // namespace mhla
