// C ABI of libmhla_hip.so (see include/mhla_hip.h): library-wide entry points and the block-mixing operator.  Validates
// arguments, carves the caller's workspace, picks the path and enqueues kernels on the caller's stream.  The bf16 fast paths
// (fused.hpp, fused_tile16.hpp, smalln.hpp) are launched from here; the generic / split-operand launches live in the per-dtype
// units (capi_bm_typed.hpp), the causal operator in capi_causal.hip, prologues / epilogues / LePE in capi_misc.hip.
#include "capi_common.hpp"
#include "fused.hpp"
#include "fused_tile16.hpp"
#include "smalln.hpp"
#include "smalln_f32.hpp"

using namespace mhla;
using namespace mhla::capi;

namespace mhla {
namespace capi {
extern template int bm_fwd_typed<float, false>(const BmCall&);
extern template int bm_fwd_typed<bf16_t, true>(const BmCall&);
extern template int bm_fwd_typed<bf16_t, false>(const BmCall&);
extern template int bm_fwd_typed<f16_t, false>(const BmCall&);
extern template int bm_bwd_typed<float, false>(const BmCall&);
extern template int bm_bwd_typed<bf16_t, true>(const BmCall&);
extern template int bm_bwd_typed<bf16_t, false>(const BmCall&);
extern template int bm_bwd_typed<f16_t, false>(const BmCall&);
}  // namespace capi
}  // namespace mhla

namespace {

// ---- fast path (bf16, D = 64, M <= 64, q_den aliasing q_num): see fused.hpp ----
// summaries of single-chunk blocks (S <= 64): the straight-line kernel, instantiated on (gather map, normaliser)
template <int MODE>
static int launch_state1c(const fast::FsStateArgs& sa, int njg, int BH, hipStream_t st, const char* name) {
    const dim3 g(njg, BH), t(fast::FT8);
    const bool idx = sa.idx != nullptr, norm = sa.normalize != 0;
    if (idx && norm) return launch(fast::k_fs_state1c<MODE, true, true>, g, t, fast::FS_STATE1C_SMEM, st, name, sa);
    if (idx) return launch(fast::k_fs_state1c<MODE, true, false>, g, t, fast::FS_STATE1C_SMEM, st, name, sa);
    if (norm) return launch(fast::k_fs_state1c<MODE, false, true>, g, t, fast::FS_STATE1C_SMEM, st, name, sa);
    return launch(fast::k_fs_state1c<MODE, false, false>, g, t, fast::FS_STATE1C_SMEM, st, name, sa);
}

// small-sequence kernels (smalln.hpp): instantiated on (head-dim tiles, gather map, exactly 16 blocks, hi + lo score tiles)
template <int DT, bool HL>
static auto sn_fwd_kernel(bool gather, int M) {
    return gather ? fast::k_sn_fwd<DT, true, false, HL> : (M == 16 ? fast::k_sn_fwd<DT, false, true, HL> : fast::k_sn_fwd<DT, false, false, HL>);
}
#ifndef SN_BWD_NB
#define SN_BWD_NB 1   // blocks per wave of the default-arithmetic small-sequence backward (smalln.hpp k_sn_bwd): sixteen waves with one block each
                      // beat eight with two by 3.5 % at C3 (107.0 -> 103.0 us, twice each; workgroup life 91 400 -> 80 000 cycles in tools/trace_smalln.py)
#endif
template <int DT, bool HL>
static auto sn_bwd_kernel(bool gather, int M) {
    // (HL: the run-time-guarded block loops also for exactly 16 blocks -- fully unrolled, pass A becomes one basic block whose
    // schedule needs 100-135 registers more than the 256 there are; the guarded form allocates 187 / 230 without a spill)
    if constexpr (HL) return gather ? fast::k_sn_bwd<DT, true, false, true, SN_BWD_NB> : fast::k_sn_bwd<DT, false, false, true, SN_BWD_NB>;
    else return gather ? fast::k_sn_bwd<DT, true, false, false> : (M == 16 ? fast::k_sn_bwd<DT, false, true, false> : fast::k_sn_bwd<DT, false, false, false>);
}

struct FastWs {
    fast::u16 *state, *dstate;
    float *z, *ksum, *ninv, *dn, *dz, *dwp, *dksum;
    int* done;   // per 16-block tile: dQ done (k_tile_bwd)
    int* err;    // error word of the token-gradient launch (a hand-over flag that did not arrive)
    size_t total_fwd, total_bwd;
    int njg, ntt;
    int cs;      // workgroups per tile and role for blocks of several 64-token chunks (S > 64), 1 otherwise
};
FastWs fast_carve(void* ws, int B, int H, int M, int S) {
    const size_t bh = (size_t)B * H;
    FastWs w;
    w.njg = (M + fast::IT - 1) / fast::IT;
    const size_t st = bh * w.njg * fast::FE * fast::IT * 2;   // bytes, multiple of 16
    char* p = (char*)ws;
    w.state = (fast::u16*)p; p += st;
    w.z = (float*)p; p += al4(bh * M * S) * 4;
    w.ksum = (float*)p; p += al4(bh * M * 64) * 4;
    w.ninv = (float*)p; p += al4(bh * M * S) * 4;
    w.total_fwd = (size_t)(p - (char*)ws);
    w.dstate = (fast::u16*)p; p += st;
    w.dn = (float*)p; p += al4(bh * M * S) * 4;
    w.dz = (float*)p; p += al4(bh * M * S) * 4;
    w.cs = S > 64 ? std::min((S + 63) / 64, 4) : 1;
    w.dksum = (float*)p; p += al4(bh * M * 64) * 4 * w.cs;   // one share per chunk part
    w.dwp = (float*)p; p += bh * fast::DW_SPLIT * 4096 * 4;
    w.ntt = fast::tiles_per_bh(w.njg, 16);
    w.done = (int*)p; p += al4(bh * w.ntt * w.cs + 1) * 4;   // per-tile (and part) flags
    w.err = nullptr;                                  // (the error word lives at the tail of the workspace: bwd_err_word)
    w.total_bwd = (size_t)(p - (char*)ws);
    return w;
}
// ---- process-wide options of the fused token-gradient launch (read ONCE, at library load, from the environment; changed afterwards
// only through mhla_set_option) ----
std::atomic<int> g_two_launches{[] { const char* e = getenv("MHLA_BWD_TWO_LAUNCHES"); return (e && e[0] == '1') ? 1 : 0; }()};
std::atomic<int> g_drop_signal{getenv("MHLA_DEBUG_DROP_SIGNAL") != nullptr ? 1 : 0};

// Self-healing of the in-launch hand-over (fused.hpp, tile_wait): every fused launch is followed by an asynchronous copy of its
// error word into a pinned host slot (+ an event on the same stream); the NEXT backward of this process looks at the slots whose
// event has completed -- no synchronisation anywhere -- and the first raised word latches the process to the two-launch form
// (the kernel boundary then orders the hand-over, whatever the dispatch order is) and says so once on stderr.
struct HandoverWatch {
    static constexpr int SLOTS = 64, MAXDEV = 16;
    std::mutex mu;
    int* host = nullptr;              // pinned (portable: visible to every device's streams), MAXDEV x SLOTS words
    hipEvent_t ev[MAXDEV][SLOTS] = {};   // an event belongs to the device it was created on: one set per device
    bool pending[MAXDEV][SLOTS] = {};
    int next[MAXDEV] = {};
    bool warned = false, unarmed_said = false;
    void unarmed(const char* why) {   // (mu held) say once that the watch cannot arm; the fused launch still runs, only the self-healing is off
        if (!unarmed_said) {
            unarmed_said = true;
            fprintf(stderr, "[mhla] the hand-over watch of the fused token-gradient launch could not be armed (%s): an expired hand-over will only "
                            "show through mhla_blockmix_bwd_status\n", why);
        }
        (void)hipGetLastError();
    }
    void poll(int dev) {   // (mu held) event queries are allowed while another thread captures a stream in global mode only in relaxed mode
        hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
        (void)hipThreadExchangeStreamCaptureMode(&mode);
        for (int i = 0; i < SLOTS; ++i) {
            if (!pending[dev][i] || hipEventQuery(ev[dev][i]) != hipSuccess) continue;
            pending[dev][i] = false;
            if (host[dev * SLOTS + i] != 0) {
                g_two_launches.store(1);
                if (!warned) {
                    warned = true;
                    fprintf(stderr, "[mhla] a dK/dV tile of the fused token-gradient launch gave up waiting for its dQ tile's hand-over (that "
                                    "backward's dk is NaN); this process runs the two roles as two launches from now on\n");
                }
            }
        }
        (void)hipThreadExchangeStreamCaptureMode(&mode);
        (void)hipGetLastError();   // (hipEventQuery's hipErrorNotReady is not an error of the caller)
    }
    static int device_of() { int d = 0; (void)hipGetDevice(&d); return d; }   // (the caller's current device: the one its stream and workspace live on)
    void watch(const int* err_word, hipStream_t st) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return; }   // a graph cannot adapt anyway
        const int dev = device_of();
        std::lock_guard<std::mutex> lk(mu);
        if (dev < 0 || dev >= MAXDEV) { unarmed("device index beyond the watch's table"); return; }
        if (!host && hipHostMalloc((void**)&host, MAXDEV * SLOTS * sizeof(int), hipHostMallocPortable) != hipSuccess) { host = nullptr; unarmed("no pinned host memory"); return; }
        poll(dev);
        int i = next[dev];
        for (int t = 0; t < SLOTS && pending[dev][i]; ++t) i = (i + 1) % SLOTS;
        if (pending[dev][i]) return;       // every slot still in flight: skip this one
        next[dev] = (i + 1) % SLOTS;
        if (!ev[dev][i] && hipEventCreateWithFlags(&ev[dev][i], hipEventDisableTiming) != hipSuccess) { ev[dev][i] = nullptr; unarmed("hipEventCreate failed"); return; }
        host[dev * SLOTS + i] = 0;
        if (hipMemcpyAsync(&host[dev * SLOTS + i], err_word, sizeof(int), hipMemcpyDeviceToHost, st) == hipSuccess && hipEventRecord(ev[dev][i], st) == hipSuccess)
            pending[dev][i] = true;
        else
            unarmed("copy / event record on the launch stream failed");
    }
    void check(hipStream_t st) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;   // (no event queries while the caller's stream is being captured)
        if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return; }
        const int dev = device_of();
        std::lock_guard<std::mutex> lk(mu);
        if (host && dev >= 0 && dev < MAXDEV) poll(dev);
    }
};
HandoverWatch g_watch;

// Error word of the fused token-gradient launch: the LAST 16 bytes of the backward workspace (mhla_blockmix_bwd_ws_bytes), behind
// the carve of every path a problem may take.  Every backward of a shape that can take the fast path leaves a defined word there:
// the fast path clears it in k_fs_dw and raises it in k_tile_bwd; when such a shape falls back to another path (misaligned views,
// rotary prologue) the dispatcher clears it with a 4-byte memset -- so mhla_blockmix_bwd_status never reads an unrelated word
// (round-3 ADVICE: it used to infer the path from the shape alone).
size_t bwd_ws_body_bytes(int B, int H, int M, int S, int D, int dtype, int split, unsigned flags) {
    const size_t gen = bm_carve_for(nullptr, B, H, M, S, D, dtype, flags, false).total_bwd;
    return (std::max(gen, bm_fast_layout(M, S, D, dtype, split != 0, flags) ? fast_carve(nullptr, B, H, M, S).total_bwd : (size_t)0) + 15) & ~(size_t)15;
}
int* bwd_err_word(void* ws, int B, int H, int M, int S, int D, int dtype, int split, unsigned flags) {
    return (int*)((char*)ws + bwd_ws_body_bytes(B, H, M, S, D, dtype, split, flags));
}

}  // namespace

extern "C" {


int mhla_abi_version(void) { return MHLA_ABI_VERSION; }

// the device-code options this library was compiled with (mhla_amd/build.py passes them as -DMHLA_BUILD_FLAGS): the loader
// refuses a library whose flags differ from the ones the package expects (no packed-fp32 VALU code)
#ifndef MHLA_BUILD_FLAGS
#define MHLA_BUILD_FLAGS "unknown"
#endif
const char* mhla_build_flags(void) { return MHLA_BUILD_FLAGS; }

void mhla_prof_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = on != 0;
}

// Waits for the recorded events, writes "name count total_ms" lines (one per kernel name) and clears.
int mhla_prof_report(char* buf, size_t cap) {
    std::vector<ProfRec> recs;
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        recs.swap(g_prof);
    }
    std::map<std::string, std::pair<long, double>> agg;
    for (auto& r : recs) {
        float ms = 0.f;
        (void)hipEventSynchronize(r.e1);
        (void)hipEventElapsedTime(&ms, r.e0, r.e1);
        auto& a = agg[r.name];
        a.first += 1;
        a.second += ms;
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    std::string out;
    char line[256];
    for (auto& kv : agg) {
        snprintf(line, sizeof(line), "%s %ld %.6f\n", kv.first.c_str(), kv.second.first, kv.second.second);
        out += line;
    }
    if (!buf || cap == 0) return (int)out.size();
    const size_t n = out.size() < cap - 1 ? out.size() : cap - 1;
    memcpy(buf, out.data(), n);
    buf[n] = 0;
    return (int)n;
}
const char* mhla_last_error(void) { return g_err; }

// Process-wide options (the two environment variables of the same meaning are read once, when the library is loaded):
//   "bwd_two_launches"   1: the backward's dQ and dK/dV tile roles as two launches (also latched by the library itself after a
//                        hand-over expired), 0: one fused launch
//   "debug_drop_signal"  testing aid: the dQ role does not raise its hand-over flags
//   "fp32_summaries"     1: 16-bit tensors at the default arithmetic keep their block summaries as fp32 in the workspace instead of
//                        24-bit floats (split.hpp p24) -- a measurement aid; set it BETWEEN calls, not between a forward and the
//                        backward that reuses its state
// Returns the previous value, or MHLA_EINVAL for an unknown name.
int mhla_set_option(const char* name, int value) {
    if (name && !strcmp(name, "bwd_two_launches")) return g_two_launches.exchange(value != 0);
    if (name && !strcmp(name, "debug_drop_signal")) return g_drop_signal.exchange(value != 0);
    if (name && !strcmp(name, "fp32_summaries")) return g_no_p24.exchange(value != 0);
    if (name && !strcmp(name, "recut_kernels")) return g_recut.exchange(value != 0);
    return fail(MHLA_EINVAL, "mhla_set_option: unknown option '%s'", name ? name : "(null)");
}

void mhla_debug_set_trace(void* buf) { g_trace = (unsigned long long*)buf; }

// 1 when mhla_blockmix_fwd leaves reusable block summaries in its workspace for this problem (pass it as fwd_ws to the
// backward), 0 when the forward is stateless (generic recompute / small-sequence path).
int mhla_blockmix_fwd_keeps_state(int B, int H, int M, int S, int D, int dtype, int split, unsigned flags) {
    (void)B; (void)H;
    switch (bm_route(M, S, D, dtype, split != 0, flags)) {
        case BM_SNF: case BM_SN: return 0;
        case BM_FAST: return 1;
        default: return sp_shape_ok(D, flags) ? 1 : 0;   // split-operand path: KV, G, z, ksum, 1/n (fp32)
    }
}

// Upper bound over the paths the library may take for this problem (the fast path needs less).
// (the fast path needs less than the split-operand path, but which one runs also depends on the alignment of the views, which
// these queries do not see: the bound covers both)
size_t mhla_blockmix_fwd_ws_bytes(int B, int H, int M, int S, int D, int dtype, int split, unsigned flags) {
    const size_t gen = bm_carve_for(nullptr, B, H, M, S, D, dtype, flags, true).total_fwd;
    return bm_fast_layout(M, S, D, dtype, split != 0, flags) ? std::max(gen, fast_carve(nullptr, B, H, M, S).total_fwd) : gen;
}
size_t mhla_blockmix_bwd_ws_bytes(int B, int H, int M, int S, int D, int dtype, int split, unsigned flags) {
    return bwd_ws_body_bytes(B, H, M, S, D, dtype, split, flags) + 16;   // + the error word of the fused token-gradient launch
}

// what every block-mix entry point hands on: the call as validated so far (c.w: carved by the family that runs)
static BmCall bm_call(mhla_view q_num, mhla_view k_num, mhla_view v, mhla_view q_den, mhla_view k_den, const float* W, int ldw, const int32_t* block_index,
                      int B, int H, int M, int S, int D, int dtype, float eps, unsigned flags, void* stream, const float* rcos, const float* rsin, long ldr) {
    BmCall c{};
    c.normalize = q_den.ptr != nullptr;
    c.split = c.normalize && (q_den.ptr != q_num.ptr || k_den.ptr != k_num.ptr);
    c.q_num = q_num; c.k_num = k_num; c.v = v; c.q_den = c.normalize ? q_den : q_num; c.k_den = c.normalize ? k_den : k_num;
    c.W = W; c.ldw = ldw; c.block_index = block_index; c.B = B; c.H = H; c.M = M; c.S = S; c.D = D; c.dtype = dtype; c.eps = eps; c.flags = flags;
    c.st = (hipStream_t)stream; c.rcos = rcos; c.rsin = rsin; c.ldr = ldr;
    return c;
}
static int bm_typed(const BmCall& c, const bool FWD) {
    switch (c.dtype) {
        case MHLA_F32: return FWD ? bm_fwd_typed<float, false>(c) : bm_bwd_typed<float, false>(c);
        case MHLA_BF16:
            if (bm_sum16(c.D, c.dtype, c.flags)) return FWD ? bm_fwd_typed<bf16_t, true>(c) : bm_bwd_typed<bf16_t, true>(c);
            return FWD ? bm_fwd_typed<bf16_t, false>(c) : bm_bwd_typed<bf16_t, false>(c);
        case MHLA_F16: return FWD ? bm_fwd_typed<f16_t, false>(c) : bm_bwd_typed<f16_t, false>(c);
        default: return fail(MHLA_EINVAL, "unknown dtype %d", c.dtype);
    }
}

// ---- small-sequence families (smalln.hpp, smalln_f32.hpp): one launch per direction, dW partials [bh][M][M] in `dwp` (backward) ----
static fast::SnArgs sn_args(const BmCall& c, void* dwp) {
    fast::SnArgs sa{};
    sa.q = cv(c.q_num); sa.k = cv(c.k_num); sa.v = cv(c.v); sa.idx = c.block_index; sa.W = c.W; sa.ldw = c.ldw;
    sa.H = c.H; sa.M = c.M; sa.D = c.D; sa.eps = c.eps; sa.relu = c.relu(); sa.normalize = c.normalize;
    if (!dwp) { sa.out = cmv(c.out); return sa; }
    sa.o = c.normalize ? cv(c.outv) : cv(c.q_num); sa.dout = cv(c.dout); sa.dq = cmv(c.dq_num); sa.dk = cmv(c.dk_num); sa.dv = cmv(c.dv); sa.dwp = (float*)dwp;
    return sa;
}
static int sn_fwd(const BmCall& c, BmRoute r) {
    const fast::SnArgs sa = sn_args(c, nullptr);
    const int M = c.M;
    const bool hl = !(c.flags & MHLA_FLAG_BF16_SUMMARIES), g = sa.idx != nullptr, d4 = c.D <= 64;
    const char* name = bm_sn_name(r, false, c.D, hl);
    const dim3 grid(c.B * c.H);
    if (r == BM_SN) {
        if (d4) return launch(hl ? sn_fwd_kernel<4, true>(g, M) : sn_fwd_kernel<4, false>(g, M), grid, dim3(fast::SN_T), fast::sn_fwd_smem<4>(), c.st, name, sa);
        return launch(hl ? sn_fwd_kernel<5, true>(g, M) : sn_fwd_kernel<5, false>(g, M), grid, dim3(fast::SN_T), fast::sn_fwd_smem<5>(), c.st, name, sa);
    }
    // fp32 tensors in the DiT / ViT regime: the attention-form kernels with hi + lo bf16 operands (smalln_f32.hpp)
    if (d4) return launch(g ? fast::k_snf_fwd<4, true> : (M == 16 ? fast::k_snf_fwd<4, false, true> : fast::k_snf_fwd<4, false>), grid, dim3(fast::SNF_T), fast::snf_smem<4>(), c.st, name, sa);
    return launch(g ? fast::k_snf_fwd<5, true> : (M == 16 ? fast::k_snf_fwd<5, false, true> : fast::k_snf_fwd<5, false>), grid, dim3(fast::SNF_T), fast::snf_smem<5>(), c.st, name, sa);
}
static int sn_bwd(const BmCall& c, BmRoute r, void* ws, size_t ws_bytes) {
    const int M = c.M, BH = c.B * c.H;
    const size_t need = (size_t)BH * M * M * 4;
    if (ws_bytes < need) return ws_too_small(ws_bytes, need);
    fast::SnArgs sa = sn_args(c, ws);
    const bool hl = !(c.flags & MHLA_FLAG_BF16_SUMMARIES), g = sa.idx != nullptr, d4 = c.D <= 64;
    const char* name = bm_sn_name(r, true, c.D, hl);
    if (r == BM_SN) {
        sa.trace = g_trace.load();
        const int nth = hl ? fast::SN_TB * (3 - SN_BWD_NB) : fast::SN_TB;
        if (d4) RC(launch(hl ? sn_bwd_kernel<4, true>(g, M) : sn_bwd_kernel<4, false>(g, M), dim3(BH), dim3(nth), hl ? fast::sn_bwd_smem<4, SN_BWD_NB>() : fast::sn_bwd_smem<4>(), c.st, name, sa));
        else    RC(launch(hl ? sn_bwd_kernel<5, true>(g, M) : sn_bwd_kernel<5, false>(g, M), dim3(BH), dim3(nth), hl ? fast::sn_bwd_smem<5, SN_BWD_NB>() : fast::sn_bwd_smem<5>(), c.st, name, sa));
    } else if (d4) RC(launch(g ? fast::k_snf_bwd<4, true> : (M == 16 ? fast::k_snf_bwd<4, false, true> : fast::k_snf_bwd<4, false>), dim3(BH), dim3(fast::SNF_T), fast::snf_smem<4>(), c.st, name, sa));
    else           RC(launch(g ? fast::k_snf_bwd<5, true> : (M == 16 ? fast::k_snf_bwd<5, false, true> : fast::k_snf_bwd<5, false>), dim3(BH), dim3(fast::SNF_T), fast::snf_smem<5>(), c.st, name, sa));
    return launch(fast::k_sn_dw_reduce, dim3(M * M), dim3(256), 0, c.st, N_SN_DW_REDUCE, (const float*)ws, c.dW, M * M, BH);
}

// ---- bf16 fast path (fused.hpp, fused_tile16.hpp) ----
// its summaries KV^T, ksum, z and 1 / n: the forward, and the recompute leg of a backward that was handed no forward workspace
static int fast_summaries(const BmCall& c, const FastWs& f) {
    const int BH = c.B * c.H, S = c.S;
    fast::FsStateArgs sa{};
    sa.x = cv(c.k_num); sa.y = cv(c.v); sa.t = cv(c.q_num); sa.idx = c.block_index; sa.state = f.state; sa.ksum = f.ksum;
    sa.z_out = f.z; sa.H = c.H; sa.M = c.M; sa.S = S; sa.eps = c.eps; sa.relu = c.relu(); sa.normalize = c.normalize;
    if (S <= 64) RC(launch_state1c<0>(sa, f.njg, BH, c.st, N_FS_STATE[0]));
    else RC(launch(fast::k_fs_state_fwd<0>, dim3(f.njg, BH), dim3(fast::FT8), fast::FS_STATE_FWD_SMEM, c.st, N_FS_STATE[0], sa));
    if (c.normalize)
        RC(launch(fast::k_fs_wz<0>, dim3((S + fast::WZ_C - 1) / fast::WZ_C, BH), dim3(fast::FT), 0, c.st, N_FS_WZ, c.W, c.ldw, (const float*)f.z, f.ninv, c.M, S, c.eps));
    return MHLA_OK;
}
static int fast_fwd(const BmCall& c, void* ws, size_t ws_bytes) {
    const int B = c.B, H = c.H, M = c.M, S = c.S;
    const FastWs f = fast_carve(ws, B, H, M, S);
    if (ws_bytes < f.total_fwd) return ws_too_small(ws_bytes, f.total_fwd);
    RC(fast_summaries(c, f));
    fast::FsOutArgs oa{};
    oa.q = cv(c.q_num); oa.o = cmv(c.out); oa.idx = c.block_index; oa.W = c.W; oa.ldw = c.ldw; oa.state = f.state; oa.ninv = f.ninv;
    oa.H = H; oa.M = M; oa.S = S; oa.njg = f.njg; oa.eps = c.eps; oa.relu = c.relu(); oa.normalize = c.normalize;
    oa.trace = g_trace.load();
    oa.cs = f.cs;
    if (f.cs > 1) return launch(fast::k_tile_out<16, true>, dim3(fast::tiles_per_bh(f.njg, 16) * B * H * f.cs), dim3(fast::FT8), fast::tile_smem<16>(), c.st, N_T16_OUT, oa);
    return launch(fast::k_tile_out<16>, dim3(fast::tiles_per_bh(f.njg, 16) * B * H), dim3(fast::FT8), fast::tile_smem<16>(), c.st, N_T16_OUT, oa);
}
static int fast_bwd(const BmCall& c, void* ws, size_t ws_bytes, const void* fwd_ws, int* err_word) {
    const int B = c.B, H = c.H, M = c.M, S = c.S;
    const bool normalize = c.normalize;
    hipStream_t st = c.st;
    FastWs f = fast_carve(ws, B, H, M, S);
    const size_t need = mhla_blockmix_bwd_ws_bytes(B, H, M, S, c.D, c.dtype, c.split, c.flags);
    if (ws_bytes < need) return ws_too_small(ws_bytes, need);
    f.err = err_word;
    const fast::u16* state = f.state;
    const float *z = f.z, *ksum = f.ksum, *ninv = f.ninv;
    if (fwd_ws) {   // forward workspace retained by the caller: reuse KV^T, z, ksum, 1/n
        const FastWs ff = fast_carve(const_cast<void*>(fwd_ws), B, H, M, S);
        state = ff.state; z = ff.z; ksum = ff.ksum; ninv = ff.ninv;
    } else {
        RC(fast_summaries(c, f));
    }
    fast::FsStateArgs ga{};
    ga.x = cv(c.q_num); ga.y = cv(c.dout); ga.t = cv(c.outv); ga.idx = c.block_index; ga.W = c.W; ga.ldw = c.ldw; ga.ninv = ninv;
    ga.state = f.dstate; ga.dn = f.dn; ga.H = H; ga.M = M; ga.S = S; ga.eps = c.eps; ga.relu = c.relu(); ga.normalize = normalize;
    if (S <= 64) RC(launch_state1c<1>(ga, f.njg, B * H, st, N_FS_STATE[1]));
    else RC(launch(fast::k_fs_state<1>, dim3(f.njg, B * H), dim3(fast::FT8), fast::FS_STATE_SMEM, st, N_FS_STATE[1], ga));
    // dW needs only dG^T, KV^T, dn and z, all complete here; dz = W^T dn (needed by the token-gradient kernels) rides in
    // the same launch as extra workgroups
    fast::FsDwArgs da{f.dstate, state, normalize ? f.dn : nullptr, z, f.dwp, M, S, f.njg, c.W, c.ldw, f.dz, f.done, f.err, f.ntt * f.cs};
    const int nwz = normalize ? (S + fast::WZ_C - 1) / fast::WZ_C : 0;
    RC(launch(fast::k_fs_dw<>, dim3(fast::DW_SPLIT + nwz, B * H), dim3(fast::FT8), fast::FS_DW_SMEM, st, N_FS_DW, da));
    fast::FsTokArgs ta{};
    ta.q = cv(c.q_num); ta.k = cv(c.k_num); ta.v = cv(c.v); ta.dout = cv(c.dout); ta.dq = cmv(c.dq_num); ta.dk = cmv(c.dk_num);
    ta.dv = cmv(c.dv); ta.idx = c.block_index; ta.W = c.W; ta.ldw = c.ldw; ta.state = state; ta.dstate = f.dstate; ta.ninv = ninv;
    ta.dz = f.dz; ta.ksum = ksum; ta.H = H; ta.M = M; ta.S = S; ta.njg = f.njg; ta.eps = c.eps; ta.relu = c.relu();
    ta.normalize = normalize;
    ta.dksum = f.dksum;
    const long ntile_wgs = (long)f.ntt * B * H * f.cs;
    ta.cs = f.cs; ta.dks_part = (long)al4((size_t)B * H * M * 64);
    unsigned long long* tr = g_trace.load();   // regions: [0] k_t16_out, [1] dQ role, [2] dK/dV role (record = ntiles + blockIdx.x)
    ta.trace = tr ? tr + ntile_wgs * fast::TRACE_SLOTS : nullptr;
    ta.dwp = f.dwp; ta.dW = c.dW; ta.nparts = B * H * fast::DW_SPLIT; ta.ntiles = (int)ntile_wgs; ta.done = f.done;
    ta.err = f.err;
    ta.drop_signal = g_drop_signal.load();   // testing aid for the bounded wait (mhla_set_option)
    g_watch.check(st);                        // did an earlier fused launch of this process report an expired hand-over?
    const auto tile_bwd = f.cs > 1 ? fast::k_tile_bwd<16, true> : fast::k_tile_bwd<16, false>;   // (multi-chunk blocks: cs workgroups per tile)
    if (g_two_launches.load()) {   // (the kernel boundary orders dksum and the flags: the wait returns at its first poll)
        RC(launch(tile_bwd, dim3((unsigned)ntile_wgs), dim3(fast::FT8), fast::tile_smem<16>(), st, "k_t16_bwd_dq", ta));
        ta.x0 = (int)ntile_wgs;
        return launch(tile_bwd, dim3((unsigned)ntile_wgs + fast::DWR_WGS), dim3(fast::FT8), fast::tile_smem<16>(), st, "k_t16_bwd_dkv", ta);
    }
    RC(launch(tile_bwd, dim3((unsigned)(2 * ntile_wgs) + fast::DWR_WGS), dim3(fast::FT8), fast::tile_smem<16>(), st, N_T16_BWD, ta));
    if (normalize) g_watch.watch(f.err, st);
    return MHLA_OK;
}

static int bm_fwd_impl(mhla_view q_num, mhla_view k_num, mhla_view v, mhla_view q_den, mhla_view k_den, const float* W,
                       int ldw, mhla_mview out, const int32_t* block_index, void* ws, size_t ws_bytes, int B, int H,
                       int M, int S, int D, int dtype, float eps, unsigned flags, void* stream, const float* rcos,
                       const float* rsin, long ldr, bool epi = false, const float* nw = nullptr, float neps = 0.f,
                       mhla_view gate = mhla_view{nullptr, 0, 0, 0}, int out_dtype = 0) {
    BmCall c = bm_call(q_num, k_num, v, q_den, k_den, W, ldw, block_index, B, H, M, S, D, dtype, eps, flags, stream, rcos, rsin, ldr);
    RC(bm_check(B, H, M, S, D, dtype, flags, c.split));
    CHECK_VIEW(q_num); CHECK_VIEW(k_num); CHECK_VIEW(v); CHECK_VIEW(out);
    if (c.normalize) { CHECK_VIEW(q_den); CHECK_VIEW(k_den); }
    if (!W || ldw < M) return fail(MHLA_EINVAL, "W null or ldw=%d < M=%d", ldw, M);
    if (!ws || ((uintptr_t)ws) % 16) return fail(MHLA_EINVAL, "workspace null or not 16-byte aligned");
    if (epi && (!sp_shape_ok(D, flags) || dtype != MHLA_F32))
        return fail(MHLA_ENOTSUP, "fused norm/gate epilogue needs fp32 q, k, v, D %% 8 == 0 and the split-operand kernels (D=%d, dtype=%d)", D, dtype);
    if (rcos && !sp_shape_ok(D, flags)) return fail(MHLA_ENOTSUP, "fused rotary prologue needs D %% 8 == 0 and the split-operand kernels (D=%d, flags=%u)", D, flags);
    if (rcos && dtype != MHLA_F32 && sf_packed(bm_sumfmt(M, S, D, dtype, flags)))   // (no rotary summary kernel is built for 16-bit tensors on h16 / p24)
        return fail(MHLA_ENOTSUP, "rotary forward on 16-bit tensors with h16 / p24 summaries is not built (M=%d S=%d D=%d dtype=%d): use fp32 tensors, or rotate "
                                  "on the host and call mhla_blockmix(q_rope, k_rope, v, W, q_den=q, k_den=k)", M, S, D, dtype);
    c.out = out; c.epi = epi; c.gate = gate; c.nw = nw; c.neps = neps; c.out_dtype = out_dtype;
    switch (const BmRoute r = bm_call_route(c, false)) {
        case BM_SN: case BM_SNF: return sn_fwd(c, r);
        case BM_FAST: return fast_fwd(c, ws, ws_bytes);
        default: break;
    }
    c.w = bm_carve_for(ws, B, H, M, S, D, dtype, flags, true);
    if (ws_bytes < c.w.total_fwd) return ws_too_small(ws_bytes, c.w.total_fwd);
    return bm_typed(c, true);
}

int mhla_blockmix_fwd(mhla_view q_num, mhla_view k_num, mhla_view v, mhla_view q_den, mhla_view k_den, const float* W,
                      int ldw, mhla_mview out, const int32_t* block_index, void* ws, size_t ws_bytes, int B, int H,
                      int M, int S, int D, int dtype, float eps, unsigned flags, void* stream) {
    return bm_fwd_impl(q_num, k_num, v, q_den, k_den, W, ldw, out, block_index, ws, ws_bytes, B, H, M, S, D, dtype, eps, flags,
                       stream, nullptr, nullptr, 0);
}

int mhla_blockmix_rope_fwd(mhla_view q, mhla_view k, mhla_view v, int normalize, const float* W, int ldw,
                           const float* rope_cos, const float* rope_sin, int64_t ld_rope, mhla_mview out,
                           const int32_t* block_index, void* ws, size_t ws_bytes, int B, int H, int M, int S, int D,
                           int dtype, float eps, unsigned flags, void* stream) {
    RC(check_rope(rope_cos, rope_sin, ld_rope, D, true));
    if (flags & MHLA_FLAG_RELU_EPS) return fail(MHLA_ENOTSUP, "relu prologue and rotary prologue are not combined (Wan applies relu before the norm output is roped: use mhla_qk_prologue)");
    const mhla_view none{nullptr, 0, 0, 0};
    return bm_fwd_impl(q, k, v, normalize ? q : none, normalize ? k : none, W, ldw, out, block_index, ws, ws_bytes, B, H, M, S, D,
                       dtype, eps, flags, stream, rope_cos, rope_sin, (long)ld_rope);
}

int mhla_blockmix_wan_fwd(mhla_view q, mhla_view k, mhla_view v, int normalize, const float* W, int ldw,
                          const float* rope_cos, const float* rope_sin, int64_t ld_rope, const float* norm_w, float norm_eps,
                          mhla_view gate, mhla_mview out, int out_dtype, const int32_t* block_index, void* ws,
                          size_t ws_bytes, int B, int H, int M, int S, int D, int dtype, float eps, unsigned flags,
                          void* stream) {
    RC(check_rope(rope_cos, rope_sin, ld_rope, D, false));
    if (out_dtype < 0 || out_dtype > 2) return fail(MHLA_EINVAL, "unknown out_dtype %d", out_dtype);
    if (flags & MHLA_FLAG_RELU_EPS) return fail(MHLA_ENOTSUP, "relu prologue is not combined with the Wan prologue / epilogue (use mhla_qk_prologue)");
    RC(check_gate(gate));
    if (norm_w && ((uintptr_t)norm_w) % 16) return fail(MHLA_EINVAL, "norm_w must be 16-byte aligned");
    const mhla_view none{nullptr, 0, 0, 0};
    return bm_fwd_impl(q, k, v, normalize ? q : none, normalize ? k : none, W, ldw, out, block_index, ws, ws_bytes, B, H, M, S, D,
                       dtype, eps, flags, stream, rope_cos, rope_sin, (long)ld_rope, true, norm_w, norm_eps, gate, out_dtype);
}

static int bm_bwd_impl(mhla_view q_num, mhla_view k_num, mhla_view v, mhla_view q_den, mhla_view k_den, const float* W,
                       int ldw, mhla_view out, mhla_view dout, mhla_mview dq_num, mhla_mview dk_num, mhla_mview dv,
                       mhla_mview dq_den, mhla_mview dk_den, float* dW, const int32_t* block_index, void* ws,
                       size_t ws_bytes, const void* fwd_ws, int B, int H, int M, int S, int D, int dtype, float eps,
                       unsigned flags, void* stream, const float* rcos = nullptr, const float* rsin = nullptr, long ldr = 0) {
    BmCall c = bm_call(q_num, k_num, v, q_den, k_den, W, ldw, block_index, B, H, M, S, D, dtype, eps, flags, stream, rcos, rsin, ldr);
    RC(bm_check(B, H, M, S, D, dtype, flags, c.split));
    CHECK_VIEW(q_num); CHECK_VIEW(k_num); CHECK_VIEW(v); CHECK_VIEW(dout);
    CHECK_VIEW(dq_num); CHECK_VIEW(dk_num); CHECK_VIEW(dv);
    if (c.normalize) { CHECK_VIEW(q_den); CHECK_VIEW(k_den); CHECK_VIEW(out); }
    if (c.split) { CHECK_VIEW(dq_den); CHECK_VIEW(dk_den); }
    if (!W || ldw < M || !dW) return fail(MHLA_EINVAL, "W/dW null or ldw=%d < M=%d", ldw, M);
    if (!ws || ((uintptr_t)ws) % 16) return fail(MHLA_EINVAL, "workspace null or not 16-byte aligned");
    if (fwd_ws && ((uintptr_t)fwd_ws) % 16) return fail(MHLA_EINVAL, "fwd_ws not 16-byte aligned");
    c.outv = out; c.dout = dout; c.dq_num = dq_num; c.dk_num = dk_num; c.dv = dv; c.dq_den = dq_den; c.dk_den = dk_den; c.dW = dW;
    const bool fast_layout = bm_fast_layout(M, S, D, dtype, c.split, flags);
    switch (const BmRoute r = bm_call_route(c, true)) {
        case BM_SN: case BM_SNF: return sn_bwd(c, r, ws, ws_bytes);
        case BM_FAST: return fast_bwd(c, ws, ws_bytes, fwd_ws, bwd_err_word(ws, B, H, M, S, D, dtype, c.split, flags));
        default: break;
    }
    c.w = bm_carve_for(ws, B, H, M, S, D, dtype, flags, false);
    if (ws_bytes < c.w.total_bwd) return ws_too_small(ws_bytes, c.w.total_bwd);
    if (fast_layout) {
        // a fast-path shape on another path (misaligned views, rotary prologue): leave a defined error word for the status call
        const size_t need = mhla_blockmix_bwd_ws_bytes(B, H, M, S, D, dtype, c.split, flags);
        if (ws_bytes < need) return ws_too_small(ws_bytes, need);
        if (hipMemsetAsync(bwd_err_word(ws, B, H, M, S, D, dtype, c.split, flags), 0, 4, c.st) != hipSuccess)
            return fail(MHLA_ELAUNCH, "hipMemsetAsync of the error word failed");
    }
    // the forward's KV, G, z, ksum, 1/n are still in its workspace (only when the shape cannot have taken the bf16 fast path,
    // whose workspace has another layout)
    c.reuse = fwd_ws && sp_shape_ok(D, flags) && (rcos || !fast_layout);
    c.olo_own = c.w.olo;
    if (c.reuse) {
        const BmWs f = bm_carve_for(const_cast<void*>(fwd_ws), B, H, M, S, D, dtype, flags, true);
        c.w.kv = f.kv; c.w.g = f.g; c.w.z = f.z; c.w.ksum = f.ksum; c.w.ninv = f.ninv;
        if (f.olo) c.w.olo = f.olo;   // (a forward given MHLA_FLAG_NO_BWD_STATE has no residual region: the backward recomputes it into its own)
    }
    return bm_typed(c, false);
}

int mhla_blockmix_bwd(mhla_view q_num, mhla_view k_num, mhla_view v, mhla_view q_den, mhla_view k_den, const float* W,
                      int ldw, mhla_view out, mhla_view dout, mhla_mview dq_num, mhla_mview dk_num, mhla_mview dv,
                      mhla_mview dq_den, mhla_mview dk_den, float* dW, const int32_t* block_index, void* ws,
                      size_t ws_bytes, const void* fwd_ws, int B, int H, int M, int S, int D, int dtype, float eps,
                      unsigned flags, void* stream) {
    return bm_bwd_impl(q_num, k_num, v, q_den, k_den, W, ldw, out, dout, dq_num, dk_num, dv, dq_den, dk_den, dW, block_index, ws,
                       ws_bytes, fwd_ws, B, H, M, S, D, dtype, eps, flags, stream);
}

// Backward of mhla_blockmix_rope_fwd: q, k are the UN-rotated tensors the forward was given; the kernels rotate them on load
// where the rotated ones are needed (dG = Q_rot^T dP, dV = K_rot dKV) and turn the gradients of the rotated tensors back before
// the normaliser's part is added, so dq / dk are the gradients w.r.t. q / k themselves -- no rotated copies, no second
// gradient pair.  fp32 tensors, D % 8 == 0 (the split-operand kernels).
int mhla_blockmix_rope_bwd(mhla_view q, mhla_view k, mhla_view v, int normalize, const float* W, int ldw,
                           const float* rope_cos, const float* rope_sin, int64_t ld_rope, mhla_view out, mhla_view dout,
                           mhla_mview dq, mhla_mview dk, mhla_mview dv, float* dW, const int32_t* block_index, void* ws,
                           size_t ws_bytes, const void* fwd_ws, int B, int H, int M, int S, int D, int dtype, float eps,
                           unsigned flags, void* stream) {
    RC(check_rope(rope_cos, rope_sin, ld_rope, D, true));
    if (dtype != MHLA_F32 || !sp_shape_ok(D, flags))
        return fail(MHLA_ENOTSUP, "rotary backward needs fp32 tensors and D %% 8 == 0 (D=%d, dtype=%d, flags=%u)", D, dtype, flags);
    if (flags & MHLA_FLAG_RELU_EPS) return fail(MHLA_ENOTSUP, "relu prologue and rotary prologue are not combined");
    const mhla_view none{nullptr, 0, 0, 0};
    const mhla_mview mnone{nullptr, 0, 0, 0};
    return bm_bwd_impl(q, k, v, normalize ? q : none, normalize ? k : none, W, ldw, out, dout, dq, dk, dv, mnone, mnone, dW, block_index,
                       ws, ws_bytes, fwd_ws, B, H, M, S, D, dtype, eps, flags, stream, rope_cos, rope_sin, (long)ld_rope);
}

// Which kernel family, summary format and launch sequence serve a block-mix problem (16-byte aligned views assumed; a misaligned view
// of a small-sequence / fast-path shape falls through to the split-operand family): the dispatcher's own predicates, as text --
// "family=...; summaries=...; fwd=k1,k2,...; bwd=k1,k2,..." -- so that tests and tools can assert the path a BASELINE configuration
// takes instead of inferring it from timings (DESIGN.md section 0a is the same table).  Returns the length written (without the NUL).
int mhla_describe_dispatch(int B, int H, int M, int S, int D, int dtype, int split, unsigned flags, char* buf, size_t cap) {
    RC(bm_check(B, H, M, S, D, dtype, flags, split != 0));
    std::string fam, sum, fwd, bwd;
    const BmRoute r = bm_route(M, S, D, dtype, split != 0, flags);
    const bool hl = !(flags & MHLA_FLAG_BF16_SUMMARIES);
    if (r == BM_SNF || r == BM_SN) {
        fam = r == BM_SNF ? "small-sequence fp32 (attention form, one launch per direction)" : "small-sequence bf16 (attention form, one launch per direction)";
        sum = hl || r == BM_SNF ? "none (score tiles in LDS as bf16 hi + lo pairs)" : "none (score tiles as single bf16: reduced precision)";
        fwd = bm_sn_name(r, false, D, hl); bwd = std::string(bm_sn_name(r, true, D, hl)) + " " + N_SN_DW_REDUCE;
    } else if (r == BM_FAST) {
        fam = "bf16 fast path (fused mixing + token tiles)";
        sum = "bf16 (single bf16 values, 8-block interleaved: reduced precision, opt-in)";
        fwd = std::string(N_FS_STATE[0]) + " " + N_FS_WZ + " " + N_T16_OUT; bwd = std::string(N_FS_STATE[1]) + " " + N_FS_DW + " " + N_T16_BWD;
    } else {   // the plan of a call with the normaliser, aligned views, no rotary tables or epilogue, the forward's workspace kept
        const BmPlan p = bm_plan((long)B * H, M, S, D, dtype, flags, true, split != 0, false, false, true);
        fam = p.sp ? "split-operand (bf16 hi + lo MFMA operands)" : "generic (exact fp32 MFMA)";
        sum = !p.sp ? "fp32 words (dense rows)" : p.fmt == SF_H16 ? "h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes)"
              : p.fmt == SF_P24 ? "p24 (24-bit floats: 16 significand bits, 3 bytes)" : p.fmt == SF_BF16 ? "bf16 (single bf16 values: reduced precision, opt-in)" : "fp32 words";
        const std::string wz0 = p.wz_kernel ? std::string(" ") + N_WZ[0] : "", wz1 = p.wz_kernel ? std::string(" ") + N_WZ[1] : "";
        const std::string summaries = std::string(p.n_state[0]) + " " + p.n_mix[0] + wz0;
        fwd = summaries + " " + p.n_out;
        // (the split-operand rows name k_wz<1> behind the mixing, wherever the plan launches it; the generic backward recomputes the forward's summaries)
        bwd = (p.sp ? "" : summaries + " ") + p.n_state[1] + (p.sp ? std::string(" ") + p.n_mix[1] + wz1 : wz1 + " " + p.n_mix[1]) + (p.n_dw ? std::string(" ") + p.n_dw : "") +
              (p.dnz ? std::string(" ") + N_DNZ : "") + " " + N_DW_REDUCE + " " + p.n_tok[0] + (p.n_tok[1] ? std::string(" ") + p.n_tok[1] : "");
    }
    const std::string txt = "family=" + fam + "; summaries=" + sum + "; fwd=" + fwd + "; bwd=" + bwd;
    if (buf && cap) {
        const size_t n = txt.size() < cap - 1 ? txt.size() : cap - 1;
        memcpy(buf, txt.data(), n);
        buf[n] = 0;
    }
    return (int)txt.size();
}

// Did the last mhla_blockmix_bwd on this workspace run into a hand-over flag that never arrived (fused.hpp, tile_wait)?
// Synchronises `stream`, reads the launch's error word.  MHLA_OK also for problems that do not take the in-launch hand-over.
int mhla_blockmix_bwd_status(const void* ws, size_t ws_bytes, int B, int H, int M, int S, int D, int dtype, int split, unsigned flags,
                             void* stream) {
    if (!ws) return fail(MHLA_EINVAL, "workspace null");
    if (bm_route(M, S, D, dtype, split != 0, flags) != BM_FAST) return MHLA_OK;
    const size_t need = mhla_blockmix_bwd_ws_bytes(B, H, M, S, D, dtype, split, flags);
    if (ws_bytes < need) return ws_too_small(ws_bytes, need);
    int word = 0;
    hipError_t e = hipMemcpyAsync(&word, bwd_err_word(const_cast<void*>(ws), B, H, M, S, D, dtype, split, flags), sizeof(int),
                                  hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return fail(MHLA_ELAUNCH, "mhla_blockmix_bwd_status: %s", hipGetErrorString(e));
    if (word != 0)
        return fail(MHLA_ELAUNCH, "k_t16_bwd: a dK/dV tile gave up waiting for its dQ tile's dksum rows (hand-over flag never raised); "
                                  "dk is invalid -- the library switches this process to two launches on its own at its next backward (mhla_set_option(\"bwd_two_launches\", 1) forces it)");
    return MHLA_OK;
}

}  // extern "C"
