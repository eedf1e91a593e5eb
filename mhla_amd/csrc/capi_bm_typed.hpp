// Generic (exact fp32 MFMA) and split-operand block-mix launches for one element type: bm_fwd_typed / bm_bwd_typed execute the call's
// BmPlan (capi_common.hpp) -- the branching here is plan field -> template instantiation.  Included by capi_bm_f32.hip, capi_bm_bf16.hip,
// capi_bm_f16.hip, each of which instantiates the two functions for its type -- the three are compiled side by side.
#pragma once
#include "capi_common.hpp"
#include "blockmix.hpp"
#include "split.hpp"
#include "split16.hpp"
#include "mixh2.hpp"

namespace mhla {
namespace capi {

static_assert(sp::mixr_te<4, SF_BF16>() == mixr_slice(true) && sp::mixr_te<4, SF_F32>() == mixr_slice(false) && sp::mixr_te<4, SF_P24>() == mixr_slice(false), "bm_plan's resident-mixing rule");
template <int DT> constexpr int sp_state_threads() {   // eight waves at D = 128 (split.hpp)
#ifdef MHLA_SP_STATE_4WAVES
    return NTHREADS;
#else
    return DT == 8 ? 512 : NTHREADS;
#endif
}
#ifndef SP_MIXH2_IH
#define SP_MIXH2_IH 2   // 193 .. 256 blocks: the output rows of k_sp_mixh2 in this many workgroups (each reads the whole slice)
#endif
#ifndef SP_MIXH2_RT
#define SP_MIXH2_RT 1   // 16-row output tiles per wave of k_sp_mixh2 (1: twelve / sixteen waves, 2: six / eight)
#endif

// The summary formats (common.hpp SF_*) a unit builds its split-operand kernels for; capi_common.hpp bm_sumfmt decides per call.  S16 (the
// unit of bf16 tensors with MHLA_FLAG_BF16_SUMMARIES) builds bf16 summaries and nothing else; the other units build fp32 words and
//   p24 (split.hpp: 24-bit floats, 3 / 4 of the bytes of every summary transfer) on the resident-mixing pipeline: 16-bit tensors with head
//       dims up to 96 and up to 128 blocks (the fused dW), and fp32 tensors at head dims 113 .. 128 with 33 .. 192 blocks (the Wan shape,
//       rotary tables and fused epilogue included: the operands are bf16 hi + lo pairs there too, 16 significand bits either way);
//   h16 (2-byte summaries, the default on 16-bit tensors): the same pipeline, for 16-bit element types.
template <typename ET, int DT, bool S16, int FMT>
constexpr bool bm_fmt_built() {
    if (S16 || FMT == SF_BF16) return S16 && FMT == SF_BF16;
    if (FMT == SF_P24) return (sizeof(ET) == 2 && DT <= 6) || (std::is_same<ET, float>::value && DT == 8);
    if (FMT == SF_H16) return sizeof(ET) == 2 && DT <= 6;
    return true;
}
template <bool S16> constexpr int sf_plain() { return S16 ? SF_BF16 : SF_F32; }   // the unit's format of one stored value per element
// the plan names a kernel this unit has no instantiation of: nothing is launched
template <typename ET, int DT>
int not_built(const char* kernel, int fmt) {
    static const char* const fmts[] = {"fp32-word", "p24", "h16", "bf16"};
    return fail(MHLA_ENOTSUP, "%s is not built for %s tensors with %s summaries at head dims up to %d", kernel,
                std::is_same<ET, float>::value ? "fp32" : std::is_same<ET, bf16_t>::value ? "bf16" : "fp16", fmts[fmt & 3], 16 * DT);
}
// run launch_fmt.operator()<FMT>() with FMT = the call's summary format, where <ET, DT, S16> build it  (the cases' order is the order in
// which a unit instantiates, and lays out, the kernels of one launch site)
template <typename ET, int DT, bool S16, typename F>
int with_fmt(int fmt, const char* kernel, F&& launch_fmt) {
    switch (fmt) {
        case SF_H16: if constexpr (bm_fmt_built<ET, DT, S16, SF_H16>()) return launch_fmt.template operator()<SF_H16>(); break;
        case SF_P24: if constexpr (bm_fmt_built<ET, DT, S16, SF_P24>()) return launch_fmt.template operator()<SF_P24>(); break;
        case SF_F32: if constexpr (bm_fmt_built<ET, DT, S16, SF_F32>()) return launch_fmt.template operator()<SF_F32>(); break;
        case SF_BF16: if constexpr (bm_fmt_built<ET, DT, S16, SF_BF16>()) return launch_fmt.template operator()<SF_BF16>(); break;
    }
    return not_built<ET, DT>(kernel, fmt);
}

// ---- mixing: Out_i = sum_j Wm(i, j) In_j over the block summaries ----
struct MixOp {
    const float* W; int ldw; const float* in; float* out; int M; long E, es; int BH; hipStream_t st;
    const float* zin; float* zout; int S; float eps;    // the normaliser's rows, mixed with the same weights where they ride along (`wz`)
    const float* in2; float* dwp; const float* zin2;    // dW riding along: the other summary set, the per-workgroup partials, z
};
inline MixOp mix_op(const BmPlan& p, const BmCall& c, int dir) {
    const BmWs& w = c.w;
    MixOp o{c.W, c.ldw, dir ? w.dg : w.kv, dir ? w.dkv : w.g, c.M, (long)c.D * c.D, w.es, c.B * c.H, c.st, dir ? w.dn : w.z, dir ? w.dz : w.ninv, c.S, dir ? 0.f : c.eps, nullptr, nullptr, nullptr};
    if (dir && p.dw_fused) { o.in2 = w.kv; o.dwp = w.dwp; o.zin2 = w.z; }
    return o;
}
// Slice plan of the persistent mixing kernels: every (b, h)'s summaries in slices of `te` elements (the last one of a row may be short), dealt
// to at most `max_wgs` workgroups; the normaliser's rows as `zt` extra slices of `tez` values, dealt round-robin over the workgroups
struct MixSlices { long total, zt; int spw, gw; };
inline MixSlices mix_slices(const MixOp& o, int te, int tez, bool wz, int max_wgs) {
    MixSlices s;
    s.total = (long)o.BH * ((o.E + te - 1) / te);
    s.zt = wz ? (long)o.BH * ((o.S + tez - 1) / tez) : 0;
    const int wgs = (int)std::min<long>(s.total, max_wgs);
    s.spw = (int)((s.total + wgs - 1) / wgs);
    s.gw = (int)((s.total + s.spw - 1) / s.spw);
    return s;
}
inline sp::MixrArgs mixr_args(const MixOp& o, const MixSlices& s, bool wz, bool trace) {
    const sp::MixrArgs a{o.W, o.ldw, o.in, o.out, o.M, o.E, o.es, s.total, s.spw, wz ? o.zin : nullptr, wz ? o.zout : nullptr, wz ? o.S : 0, o.eps,
                          trace ? g_trace.load() : nullptr, o.in2, o.dwp, s.zt, wz ? o.zin2 : nullptr};
    return a;
}
// sp::k_sp_mixr (split.hpp).  DW: the backward's dKV = W^T dG with the dW products riding along (fp32 / 24-bit summaries, up to 128 blocks): one
// [M][M] partial per workgroup (`*parts`); with `wz`, dz = W^T dn and the <dn_i, z_j> term of dW ride along too
template <int NW, int TRANS, int FMT, bool DW>
int sp_mixr_nw(const MixOp& o, bool wz, const char* name, int* parts) {
    // persistent workgroups: as many as fit a CU beside each other (35 KB of LDS at four waves, 70 KB at eight)
    // DW: 54 KB of LDS at four waves: two per CU; 27 KB at two waves
    const MixSlices s = mix_slices(o, sp::mixr_te<NW, FMT>(), sp::mixr_te<NW, FMT>(), wz, DW ? 256 * (NW <= 2 ? 4 : NW <= 4 ? 2 : 1) : 256 * (NW <= 2 ? 8 : NW <= 4 ? 4 : NW <= 8 ? 2 : 1));
    if (parts) *parts = s.gw;
    return launch(sp::k_sp_mixr<NW, TRANS, FMT, DW>, dim3(s.gw), dim3(64 * NW), sp::sp_mixr_smem<NW, FMT, DW>(), o.st, name, mixr_args(o, s, wz, !DW));
}
template <int TRANS, int FMT, bool DW>
int sp_mixr(const MixOp& o, int nw, bool wz, const char* name, int* parts = nullptr) {
    switch (nw) {
        case 2: if constexpr (FMT != SF_BF16) return sp_mixr_nw<2, TRANS, FMT, DW>(o, wz, name, parts); break;
        case 4: return sp_mixr_nw<4, TRANS, FMT, DW>(o, wz, name, parts);
        case 8: return sp_mixr_nw<8, TRANS, FMT, DW>(o, wz, name, parts);
        case 12: if constexpr (!DW) return sp_mixr_nw<12, TRANS, FMT, DW>(o, wz, name, parts); break;   // (twelve waves have no registers for the dW tiles)
        case 16: if constexpr (!DW && FMT == SF_F32) return sp_mixr_nw<16, TRANS, FMT, DW>(o, wz, name, parts); break;   // (p24: bm_sumfmt admits up to 192 blocks; bf16: k_sp_mixr_dma)
    }
    return fail(MHLA_EINVAL, "sp_mixr: M=%d out of range", o.M);
}
// bf16 summaries of 193 .. 256 blocks: eight waves x 32 output blocks, LDS-DMA staging with three slices in flight; the normaliser's product
// (k_wz) rides along: same weights, at most 16 values per block
template <int TRANS>
int sp_mixr_dma(const MixOp& o, bool wz, const char* name) {
    const MixSlices s = mix_slices(o, 64, 64, false, 256);
    sp::MixrArgs a = mixr_args(o, s, wz, true);
    a.S = o.S;
    return launch(sp::k_sp_mixr_dma<TRANS>, dim3(s.gw), dim3(sp::MIXR_DMA_T), sp::sp_mixr_dma_smem(), o.st, name, a);
}
// h16 summaries: the mixing on the fp16 payload (mixh.hpp k_sp_mixh).  Slices of 128 elements (the last one of a row may be half), the
// normaliser's rows as extra slices of 64 values when the block length is even; persistent workgroups, as many as fit a CU.  DW as above.
template <int NW, int TRANS, bool DW>
int sp_mixh_nw(const MixOp& o, bool wz, const char* name, int* parts) {
    // (DW: bm_carve: at most 1024 / 512 / 256 partials at two / four / eight waves)
    const MixSlices s = mix_slices(o, sp::mixh_te<NW>(), sp::mixh_tez<NW>(), wz, DW ? 256 * (NW <= 2 ? 4 : NW <= 4 ? 2 : 1) : 256 * (NW <= 2 ? 8 : NW <= 4 ? 4 : 1));
    if (parts) *parts = s.gw;
    return launch(sp::k_sp_mixh<NW, TRANS, DW>, dim3(s.gw), dim3(64 * NW), sp::sp_mixh_smem<NW, DW>(), o.st, name, mixr_args(o, s, wz, !DW));
}
// 129 .. 256 blocks: 64-element slices, one workgroup per CU; dW by k_sp_dwr<.., h16>.  With eight or more slices per workgroup (sp_mixh2_applies)
// the re-cut kernel (mixh2.hpp: half the waves, two output tiles each, the rescaled weights kept per (b, h))
template <int NW, int RT, int TRANS, int IH>
int sp_mixh2_nw(const MixOp& o, bool wz, const char* name) {
    const MixSlices s = mix_slices(o, SP_MIXH2_TE, SP_MIXH2_TE / 2, wz, 256);
    return launch(sp::k_sp_mixh2<NW, RT, TRANS, SP_MIXH2_TE, IH>, dim3(s.gw, IH), dim3(64 * NW), sp::sp_mixh2_smem<NW, RT, SP_MIXH2_TE, IH>(), o.st, name, mixr_args(o, s, wz, false));
}
template <int TRANS>
int sp_mixh(const MixOp& o, BmKern kind, int nw, bool dw, bool wz, const char* name, int* parts) {
    if (kind == K_SP_MIXH2) {
        if (nw == 12) return sp_mixh2_nw<12 / SP_MIXH2_RT, SP_MIXH2_RT, TRANS, 1>(o, wz, name);
        if (nw == 16) return sp_mixh2_nw<16 / SP_MIXH2_RT / SP_MIXH2_IH, SP_MIXH2_RT, TRANS, SP_MIXH2_IH>(o, wz, name);
    } else if (dw) {
        if constexpr (TRANS == 1) switch (nw) {
            case 2: return sp_mixh_nw<2, 1, true>(o, wz, name, parts);
            case 4: return sp_mixh_nw<4, 1, true>(o, wz, name, parts);
            case 8: return sp_mixh_nw<8, 1, true>(o, wz, name, parts);
        }
    } else switch (nw) {
        case 2: return sp_mixh_nw<2, TRANS, false>(o, wz, name, parts);
        case 4: return sp_mixh_nw<4, TRANS, false>(o, wz, name, parts);
        case 8: return sp_mixh_nw<8, TRANS, false>(o, wz, name, parts);
        case 12: return sp_mixh_nw<12, TRANS, false>(o, wz, name, parts);
        case 16: return sp_mixh_nw<16, TRANS, false>(o, wz, name, parts);
    }
    return fail(MHLA_EINVAL, "sp_mixh: M=%d out of range", o.M);
}
// the plan's mixing kernel of direction TRANS; `*parts`: the [M][M] dW partials it left, where dW rode along
template <typename ET, int DT, int TRANS, bool S16>
int bm_mix(const BmPlan& p, const BmCall& c, int* parts = nullptr) {
    constexpr int PLAIN = sf_plain<S16>();
    constexpr bool PACKED = bm_fmt_built<ET, DT, S16, SF_P24>();   // the unit has the p24 mixing kernels and, with them, the h16 ones (mixh.hpp)
    const MixOp o = mix_op(p, c, TRANS);
    const bool wz = c.normalize && p.wz_fused;
    const char* name = p.n_mix[TRANS];
    const MixArgs tiled{o.W, o.ldw, o.in, o.out, o.M, o.E, o.es}, dense{o.W, o.ldw, o.in, o.out, o.M, o.E, TRANS ? 0 : o.es};   // (dense rows: the row stride is not read)
    switch (p.mix[TRANS]) {
        case K_MIX:
            return launch(k_mix<TRANS, 0>, dim3((unsigned)((o.E + MIX_TE - 1) / MIX_TE), (o.M + MIX_TI - 1) / MIX_TI, o.BH), dim3(NTHREADS), MIX_SMEM_FLOATS * 4, o.st, name, dense);
        case K_SP_MIX:
            if (p.fmt == PLAIN) return launch(sp::k_sp_mix<TRANS, PLAIN>, dim3((unsigned)((o.E + sp::SPM_TE - 1) / sp::SPM_TE), (o.M + 63) / 64, o.BH), dim3(NTHREADS), sp::sp_mix_smem<PLAIN>(), o.st, name, tiled);
            break;
        case K_SP_MIXR_DMA:
            if constexpr (S16) return sp_mixr_dma<TRANS>(o, wz, name);
            break;
        case K_SP_MIXR:
            if (TRANS == 1 && p.dw_fused) {   // (the plan lets dW ride on fp32 words and p24 only)
                if constexpr (TRANS == 1) {
                    if (p.fmt == SF_P24) { if constexpr (PACKED) return sp_mixr<1, SF_P24, true>(o, p.nw, wz, name, parts); }
                    else if (p.fmt == SF_F32) return sp_mixr<1, SF_F32, true>(o, p.nw, wz, name, parts);
                }
            } else if (p.fmt == SF_P24) { if constexpr (PACKED) return sp_mixr<TRANS, SF_P24, false>(o, p.nw, wz, name); }
            else if (p.fmt == PLAIN) return sp_mixr<TRANS, PLAIN, false>(o, p.nw, wz, name);
            break;
        case K_SP_MIXH: case K_SP_MIXH2:
            if constexpr (PACKED) return sp_mixh<TRANS>(o, p.mix[TRANS], p.nw, TRANS && p.dw_fused, wz, name, parts);
            break;
        default: break;
    }
    return not_built<ET, DT>(name, p.fmt);
}
// the normaliser's product as a launch of its own: 1 / n = 1 / (eps + W z) (TRANS 0), dz = W^T dn (TRANS 1)
template <int TRANS>
int launch_wz(const float* W, int ldw, const float* x, float* out, int BH, int M, int S, float eps, hipStream_t st) {
    return launch(k_wz<TRANS>, dim3((S + 63) / 64, (M + 63) / 64, BH), dim3(NTHREADS), 0, st, N_WZ[TRANS], W, ldw, x, out, M, S, eps);
}

// ---- summaries: KV_j = K_j^T V_j (+ ksum, z) for the forward, dG_i = Q_i^T (dO_i / n_i) (+ dn) for the backward ----
template <typename ET, int DT, int TRANS, bool S16>
int bm_state(const BmPlan& p, const BmCall& c, const StateArgs& a) {
    constexpr bool F32 = std::is_same<ET, float>::value;
    constexpr int SNT = sp_state_threads<DT>();
    const dim3 g(c.M, c.B * c.H);
    const char* name = p.n_state[TRANS];
    if (p.state == K_BM_STATE) return launch(k_bm_state<ET, DT, TRANS>, g, dim3(NTHREADS), state_smem_floats<DT>() * 4, c.st, name, a);
    if (p.state == K_S16_STATE) return launch(s16::k_s16_state<TRANS>, dim3((c.M + s16::WPB - 1) / s16::WPB, c.B * c.H), dim3(64 * s16::WPB), s16::state_smem(), c.st, name, a);
    if (p.rope) {   // (the rotary backward serves fp32 tensors; 24-bit summaries with rotary tables likewise)
        constexpr sp::StateVar ROPE{.rope = true};
        if (p.fmt == SF_P24) {
            if constexpr (F32 && bm_fmt_built<ET, DT, S16, SF_P24>()) return launch(sp::k_sp_state<ET, DT, TRANS, SNT, SF_P24, ROPE>, g, dim3(SNT), sp::sp_state_smem<DT>(), c.st, name, a);
        } else if (p.fmt == sf_plain<S16>()) {
            if constexpr (F32 || TRANS == 0) return launch(sp::k_sp_state<ET, DT, TRANS, SNT, sf_plain<S16>(), ROPE>, g, dim3(SNT), sp::sp_state_smem<DT>(), c.st, name, a);
        }
        return not_built<ET, DT>(name, p.fmt);
    }
    // (bf16 tensors under the relu prologue: relu(x) + eps is an fp32 value -- the instantiation that keeps its lo part; its row dots from G_i
    // take the hi + lo form fp16 tensors have)
    if constexpr (!S16 && std::is_same<ET, bf16_t>::value) {
        if (a.relu) return with_fmt<ET, DT, S16>(p.fmt, name, [&]<int FMT>() {
            constexpr int smem = (sf_packed(FMT) && TRANS && DT <= 4) ? sp::sp_state_rd_smem<DT, false>() : sp::sp_state_smem<DT>();
            return launch(sp::k_sp_state<ET, DT, TRANS, SNT, FMT, sp::StateVar{.lo = true}>, g, dim3(SNT), smem, c.st, name, a);
        });
    }
    // (forward on h16 summaries without a split normaliser pair: the instantiation that has no third row stream)
    if constexpr (TRANS == 0 && bm_fmt_built<ET, DT, S16, SF_H16>()) {
        if (p.fmt == SF_H16 && !(c.normalize && c.split) && g_recut.load())
            return launch(sp::k_sp_state<ET, DT, 0, SNT, SF_H16, sp::StateVar{.ts = false}>, g, dim3(SNT), sp::sp_state_smem<DT>(), c.st, name, a);
    }
    // (backward on h16 / p24, 16-bit tensors, D <= 64: the row dots come from G_i; two more LDS tiles)
    return with_fmt<ET, DT, S16>(p.fmt, name, [&]<int FMT>() {
        constexpr int smem = (sf_packed(FMT) && TRANS && sizeof(ET) == 2 && DT <= 4) ? sp::sp_state_rd_smem<DT, sp::sp_payrd<ET, DT, FMT>()>() : sp::sp_state_smem<DT>();
        return launch(sp::k_sp_state<ET, DT, TRANS, SNT, FMT>, g, dim3(SNT), smem, c.st, name, a);
    });
}
// KV / ksum / z, G and 1 / n: the forward, and the recompute leg of a backward that was handed no forward workspace
template <typename ET, int DT, bool S16>
int bm_state_and_mix(const BmPlan& p, const BmCall& c) {
    const BmWs& w = c.w;
    StateArgs a{};
    a.rcos = c.rcos; a.rsin = c.rsin; a.ldr = c.ldr;
    a.x = cv(c.k_num); a.y = cv(c.v); a.kd = cv(c.k_den); a.qd = cv(c.q_den); a.idx = c.block_index;
    a.out = w.kv; a.ksum = w.ksum; a.zo = w.z; a.es = w.es;
    a.H = c.H; a.M = c.M; a.S = c.S; a.D = c.D; a.eps = c.eps; a.relu = c.relu(); a.normalize = c.normalize; a.split = c.split;
    RC((bm_state<ET, DT, 0, S16>(p, c, a)));
    RC((bm_mix<ET, DT, 0, S16>(p, c)));
    if (p.wz_kernel) RC(launch_wz<0>(c.W, c.ldw, w.z, w.ninv, c.B * c.H, c.M, c.S, c.eps, c.st));
    return MHLA_OK;
}

// ---- output O_i = Q_i G_i / n_i: the forward's, and the backward's recompute of what the forward's 16-bit store of O rounded away ----
template <typename ET, int DT, bool S16, typename TO = ET, bool EPI = false>
int sp_out(const BmPlan& p, const BmCall& c, const OutArgs& o, const char* name) {
    const dim3 g(c.M, c.B * c.H), blk(sp::SP_OUT_T);
    // (bf16 tensors with rotary tables, served on fp32-word summaries only: the instantiation that keeps the lo part of the rotated q)
    if constexpr (!EPI && !S16 && std::is_same<ET, bf16_t>::value) {
        if (c.rcos) {
            if (p.fmt != SF_F32) return not_built<ET, DT>(name, p.fmt);
            return launch(sp::k_sp_out<ET, DT, TO, SF_F32, sp::OutVar{.rope = true}>, g, blk, sp::sp_out_smem<DT, SF_F32>(), c.st, name, o);
        }
    }
    // (bf16 tensors under the relu prologue: the instantiation that keeps the lo part of relu(q) + eps)
    if constexpr (!EPI && !S16 && std::is_same<ET, bf16_t>::value) {
        if (o.relu) return with_fmt<ET, DT, S16>(p.fmt, name, [&]<int FMT>() {
            return launch(sp::k_sp_out<ET, DT, TO, FMT, sp::OutVar{.lo = true}>, g, blk, sp::sp_out_smem<DT, FMT>(), c.st, name, o);
        });
    }
    // (16-bit tensors on h16 summaries, D <= 64, blocks of at most 64 tokens: the instantiation of one tile per wave)
    if constexpr (!EPI && bm_fmt_built<ET, DT, S16, SF_H16>() && DT <= 4) {
        if (p.fmt == SF_H16 && bm_one_tile(c.S))
            return launch(sp::k_sp_out<ET, DT, TO, SF_H16, sp::OutVar{.one = true}>, g, blk, sp::sp_out_smem<DT, SF_H16>(), c.st, name, o);
    }
    return with_fmt<ET, DT, S16>(p.fmt, name, [&]<int FMT>() {
        return launch(sp::k_sp_out<ET, DT, TO, FMT, sp::OutVar{.epi = EPI}>, g, blk, sp::sp_out_smem<DT, FMT>(), c.st, name, o);
    });
}
inline OutArgs out_args(const BmCall& c) {
    OutArgs o{};
    o.rcos = c.rcos; o.rsin = c.rsin; o.ldr = c.ldr;
    o.q = cv(c.q_num); o.idx = c.block_index; o.W = c.W; o.ldw = c.ldw; o.g = c.w.g; o.ninv = c.w.ninv;
    o.H = c.H; o.M = c.M; o.S = c.S; o.D = c.D; o.eps = c.eps; o.es = c.w.es; o.relu = c.relu(); o.normalize = c.normalize;
    return o;
}
template <typename ET, int DT, bool S16>
int bm_out(const BmPlan& p, const BmCall& c, OutArgs& o, const char* name) {
    if (p.out == K_BM_OUT) return launch(k_bm_out<ET, DT>, dim3(c.M, c.B * c.H), dim3(NTHREADS), out_smem_floats<DT>() * 4, c.st, name, o);
    if (p.out == K_S16_OUT) return launch(s16::k_s16_out<0>, dim3((c.M + s16::WPB - 1) / s16::WPB, c.B * c.H), dim3(64 * s16::WPB), s16::out_smem(), c.st, name, o);
    if (!c.epi) return sp_out<ET, DT, S16>(p, c, o, name);
    if constexpr (std::is_same<ET, float>::value) {   // fused norm x gate epilogue (Wan): fp32 tensors, the output in the caller's dtype
        o.nw = c.nw; o.neps = c.neps; o.gate = cv(c.gate);
        if (c.out_dtype == MHLA_BF16) return sp_out<float, DT, S16, bf16_t, true>(p, c, o, name);
        if (c.out_dtype == MHLA_F16) return sp_out<float, DT, S16, f16_t, true>(p, c, o, name);
        return sp_out<float, DT, S16, float, true>(p, c, o, name);
    }
    return not_built<ET, DT>(name, p.fmt);
}

// ---- dW = sum_bh (<dG_i, KV_j> + <dn_i, z_j>): partials in w.dwp, `*parts` of them, then k_dw_reduce ----
// dW partials with the whole M x M matrix in one workgroup (s16::k_sp_dwr): 64 < M <= 256, 16-bit summaries
inline int sp_dwr_splits(int BH, long E) {
    int ns = (256 + BH - 1) / BH;
    if (ns > DW_MAX_SPLIT) ns = DW_MAX_SPLIT;
    while (ns > 1 && E / ns < 256) --ns;
    return ns < 1 ? 1 : ns;
}
// (`es`: row stride in 16-bit elements.  h16: the rows are fp16 payload with their multiplier behind the E elements -- products on the fp16 MFMA)
inline int sp_dwr(const s16::DwrArgs& d, int tiles, bool h16, int BH, hipStream_t st, const char* name) {
    const dim3 g(d.nsplit, BH);
    if (h16) {
        if (tiles == 2) return launch(s16::k_sp_dwr<2, true>, g, dim3(256), s16::dwr_smem<2>(), st, name, d);
        if (tiles == 3) return launch(s16::k_sp_dwr<3, true>, g, dim3(576), s16::dwr_smem<3>(), st, name, d);
        return launch(s16::k_sp_dwr<4, true>, g, dim3(1024), s16::dwr_smem<4>(), st, name, d);
    }
    if (tiles == 2) return launch(s16::k_sp_dwr<2>, g, dim3(256), s16::dwr_smem<2>(), st, name, d);
    if (tiles == 3) return launch(s16::k_sp_dwr<3>, g, dim3(576), s16::dwr_smem<3>(), st, name, d);
    return launch(s16::k_sp_dwr<4>, g, dim3(1024), s16::dwr_smem<4>(), st, name, d);
}
template <typename ET, int DT, bool S16>
int bm_dw(const BmPlan& p, const BmCall& c, int tiles, int* parts) {
    const BmWs& w = c.w;
    const int BH = c.B * c.H, M = c.M;
    const long E = (long)c.D * c.D;
    if (p.dw == K_NONE) return MHLA_OK;   // (the partials of the mixing kernel are in w.dwp)
    const float *dn = c.normalize ? w.dn : nullptr, *z = c.normalize ? w.z : nullptr;
    if (p.dw == K_SP_DWR) {   // whole-matrix workgroups: the <dn_i, z_j> term is one of their stages
        const int nsplit = sp_dwr_splits(BH, E);
        *parts = BH * nsplit;
        const s16::DwrArgs d{(const sp::u16*)w.dg, (const sp::u16*)w.kv, E, p.fmt == SF_H16 ? 2 * w.es : w.es, dn, z, c.S, w.dwp, M, nsplit};   // (named: tools/record_launches.py hashes the padding too)
        return sp_dwr(d, p.dw_v, p.fmt == SF_H16, BH, c.st, p.n_dw);
    }
    int nsplit = dw_splits(tiles * tiles * BH, E);
    if (p.dw == K_DW) {
        *parts = BH * nsplit;
        const DwArgs d{w.dg, w.kv, E, dn, z, (long)c.S, w.dwp, M, tiles, nsplit};
        return launch(k_dw<0>, dim3(tiles * tiles, BH, nsplit), dim3(NTHREADS), DW_SMEM_FLOATS * 4, c.st, p.n_dw, d);
    }
    if (nsplit > DW_MAX_SPLIT - 1) nsplit = DW_MAX_SPLIT - 1;   // one more part per (b, h) holds the <dn_i, z_j> term
    *parts = BH * nsplit;
    const DwArgs d{w.dg, w.kv, E, nullptr, nullptr, 0, w.dwp, M, tiles, nsplit, w.es};
    const dim3 g(p.dw_v ? 1 : tiles * tiles, BH, nsplit);
    if (p.dw == K_SP_DWT) {   // 24-bit summaries of 129 .. 192 blocks: k_sp_dwt reads dG and KV again
        if constexpr (bm_fmt_built<ET, DT, S16, SF_P24>()) { if (p.fmt == SF_P24) return launch(sp::k_sp_dwt<SF_P24>, g, dim3(NTHREADS), sp::SP_DWT_SMEM, c.st, p.n_dw, d); }
        return not_built<ET, DT>(p.n_dw, p.fmt);
    }
    constexpr int PLAIN = sf_plain<S16>();
    if (p.fmt != PLAIN) return not_built<ET, DT>(p.n_dw, p.fmt);
    if (p.dw_v == 16) return launch(sp::k_sp_dw<PLAIN, 1>, g, dim3(NTHREADS), sp::SP_DW_SMEM, c.st, p.n_dw, d);
    if (p.dw_v == 32) return launch(sp::k_sp_dw<PLAIN, 2>, g, dim3(NTHREADS), sp::SP_DW_SMEM, c.st, p.n_dw, d);
    return launch(sp::k_sp_dw<PLAIN>, g, dim3(NTHREADS), sp::SP_DW_SMEM, c.st, p.n_dw, d);
}
// the <dn_i, z_j> term as one more part per (b, h), behind the `parts` there are
template <int MASK = 0>   // (templates: instantiated only in the units that launch them)
int launch_dnz(const BmCall& c, int tiles, int parts) {
    const DwArgs dzz{c.w.dn, c.w.z, (long)c.S, nullptr, nullptr, 0, c.w.dwp + (size_t)parts * c.M * c.M, c.M, tiles, 1};
    return launch(k_dw<MASK>, dim3(tiles * tiles, c.B * c.H, 1), dim3(NTHREADS), DW_SMEM_FLOATS * 4, c.st, N_DNZ, dzz);
}
// (16 elements x 16 part-lanes per workgroup when the matrix is small or the parts are many: a thread's chain of dependent
// load batches is what the kernel takes -- 512 parts of 64 x 64 at 64 x 4: 10 us)
template <int MASK = 0>
int launch_dw_reduce(const float* dwp, float* dW, int M, int parts, int BH, bool el16, hipStream_t st) {
    if (el16 || M * M <= 1024 || parts >= 128) return launch(k_dw_reduce<MASK, 16>, dim3((M * M + 15) / 16), dim3(256), 0, st, N_DW_REDUCE, dwp, (const float*)nullptr, dW, M, M, parts, BH);
    return launch(k_dw_reduce<MASK>, dim3((M * M + 63) / 64), dim3(256), 0, st, N_DW_REDUCE, dwp, (const float*)nullptr, dW, M, M, parts, BH);
}

// ---- token gradients dQ, dK, dV ----
template <typename ET, int DT, int FMT, sp::DqVar V = sp::DqVar{}>
int sp_dq(const BmPlan& p, const BmCall& c, const TokArgs& t) {
    return launch(sp::k_sp_bwd_dq<ET, DT, FMT, V>, dim3(c.M, c.B * c.H), dim3(NTHREADS), sp::sp_dq_smem<DT, FMT, sp::sp_payop<ET, DT, FMT, V.rope>()>(), c.st, p.n_tok[0], t);
}
template <typename ET, int DT, int FMT, sp::DkvVar V = sp::DkvVar{}>
int sp_dkv(const BmPlan& p, const BmCall& c, const TokArgs& t) {
    return launch(sp::k_sp_bwd_dkv<ET, DT, FMT, V>, dim3(c.M, c.B * c.H), dim3(NTHREADS), sp::sp_tok_smem<DT, FMT>(), c.st, p.n_tok[1], t);
}
template <typename ET, int DT, bool S16>
int bm_tok(const BmPlan& p, const BmCall& c, const TokArgs& t) {
    const dim3 g(c.M, c.B * c.H), blk(NTHREADS);
    if (p.tok == K_BM_TOK) return launch(k_bm_bwd_tok<ET, DT>, g, blk, tok_smem_floats<DT>() * 4, c.st, p.n_tok[0], t);
    if (p.tok == K_S16_TOK) {   // (the dK kernel forms dksum itself: no order between the two)
        const dim3 g16((c.M + s16::WPB - 1) / s16::WPB, c.B * c.H), b16(64 * s16::WPB);
        RC(launch(s16::k_s16_bwd_dq<0>, g16, b16, 0, c.st, p.n_tok[0], t));
        return launch(s16::k_s16_bwd_dkv<0>, g16, b16, s16::dkv_smem(), c.st, p.n_tok[1], t);
    }
    if (p.rope) {
        if constexpr (std::is_same<ET, float>::value) return with_fmt<ET, DT, S16>(p.fmt, p.n_tok[0], [&]<int FMT>() {
            RC((sp_dq<ET, DT, FMT, sp::DqVar{.rope = true}>(p, c, t)));
            return sp_dkv<ET, DT, FMT, sp::DkvVar{.rope = true}>(p, c, t);
        });
        return not_built<ET, DT>(p.n_tok[0], p.fmt);
    }
    // (16-bit tensors: q_den in 16-byte pieces when it only feeds dksum; not at D = 72 / 80, where the wider rows cost a wave of occupancy)
    const bool wq = c.normalize && !c.relu() && sizeof(ET) == 2 && DT != 5;
    // (h16 summaries, D <= 64, blocks of at most 64 tokens: a wave has one tile at the most -- the loop-free instantiation)
    constexpr bool ONE_BUILT = bm_fmt_built<ET, DT, S16, SF_H16>() && DT <= 4;
    if (wq && ONE_BUILT && p.fmt == SF_H16 && bm_one_tile(c.S)) {
        if constexpr (ONE_BUILT) RC((sp_dq<ET, DT, SF_H16, sp::DqVar{.wq = true, .one = true}>(p, c, t)));
    } else if (wq) RC((with_fmt<ET, DT, S16>(p.fmt, p.n_tok[0], [&]<int FMT>() { return sp_dq<ET, DT, FMT, sp::DqVar{.wq = true}>(p, c, t); })));
    else RC((with_fmt<ET, DT, S16>(p.fmt, p.n_tok[0], [&]<int FMT>() { return sp_dq<ET, DT, FMT>(p, c, t); })));
    if constexpr (!S16 && std::is_same<ET, bf16_t>::value) {   // (the relu prologue on bf16 tensors: relu(k) + eps keeps its lo part)
        if (c.relu()) return with_fmt<ET, DT, S16>(p.fmt, p.n_tok[1], [&]<int FMT>() { return sp_dkv<ET, DT, FMT, sp::DkvVar{.lo = true}>(p, c, t); });
    }
    return with_fmt<ET, DT, S16>(p.fmt, p.n_tok[1], [&]<int FMT>() { return sp_dkv<ET, DT, FMT>(p, c, t); });
}

// S16: the unit of bf16 block summaries (bf16 tensors with MHLA_FLAG_BF16_SUMMARIES); false: fp32-grade summaries, hi + lo operands (bm_fmt_built)
template <typename ET, bool S16>
int bm_fwd_typed(const BmCall& c) {
    const BmPlan p = bm_plan(c, false);
    DISPATCH_DT(dt_for(c.D), {
        RC((bm_state_and_mix<ET, DT, S16>(p, c)));
        OutArgs o = out_args(c);
        o.o = cmv(c.out);
        o.olo = (c.normalize && !c.epi && !(c.flags & MHLA_FLAG_NO_BWD_STATE)) ? c.w.olo : nullptr;   // (16-bit tensors, default arithmetic: BmWs::olo)
        RC((bm_out<ET, DT, S16>(p, c, o, p.n_out)));
    });
    return MHLA_OK;
}

template <typename ET, bool S16>
int bm_bwd_typed(const BmCall& c) {
    const BmPlan p = bm_plan(c, true);
    const BmWs& w = c.w;
    const int BH = c.B * c.H, M = c.M, S = c.S, tiles = (M + 63) / 64;
    DISPATCH_DT(dt_for(c.D), {
        if (!c.reuse) RC((bm_state_and_mix<ET, DT, S16>(p, c)));
        const bool want_olo = c.normalize && w.olo != nullptr, own_olo = !c.reuse || (c.flags & MHLA_FLAG_NO_BWD_STATE);
        if (want_olo && own_olo) {
            // what the forward's 16-bit store of O rounded away (BmWs::olo), recomputed: the output kernel without its output
            OutArgs o = out_args(c);
            o.o = MView{nullptr, 0, 0, 0}; o.olo = c.olo_own; o.skip_out = 1;
            RC((bm_out<ET, DT, S16>(p, c, o, p.n_olo)));
        }
        // dG_i = Q_i^T (dO_i / n_i), dn_i
        StateArgs a{};
        a.x = cv(c.q_num); a.y = cv(c.dout); a.o = cv(c.outv); a.idx = c.block_index; a.W = c.W; a.ldw = c.ldw; a.ninv = w.ninv;
        a.out = w.dg; a.dn = w.dn; a.es = w.es; a.H = c.H; a.M = M; a.S = S; a.D = c.D; a.eps = c.eps;
        a.relu = c.relu(); a.normalize = c.normalize; a.split = c.split;
        a.olo = !want_olo ? nullptr : (own_olo ? c.olo_own : w.olo);
        a.rcos = c.rcos; a.rsin = c.rsin; a.ldr = c.ldr;
        if (p.fmt == SF_P24 || p.fmt == SF_H16) a.g = w.g;   // (16-bit tensors, D <= 64: the row dots come from G_i)
        RC((bm_state<ET, DT, 1, S16>(p, c, a)));
        if (p.wz_kernel && p.wz1_first) RC(launch_wz<1>(c.W, c.ldw, w.dn, w.dz, BH, M, S, 0.f, c.st));
        // dKV = W^T dG, dz = W^T dn, dW
        int parts = 0;
        RC((bm_mix<ET, DT, 1, S16>(p, c, &parts)));
        RC((bm_dw<ET, DT, S16>(p, c, tiles, &parts)));
        if (p.wz_kernel && !p.wz1_first) RC(launch_wz<1>(c.W, c.ldw, w.dn, w.dz, BH, M, S, 0.f, c.st));
        if (p.dnz) {
            RC(launch_dnz(c, tiles, parts));
            parts += BH;
        }
        RC(launch_dw_reduce(w.dwp, c.dW, M, parts, BH, p.reduce16, c.st));
        // dQ, dK, dV
        TokArgs t{};
        t.q = cv(c.q_num); t.k = cv(c.k_num); t.v = cv(c.v); t.qd = cv(c.q_den); t.kd = cv(c.k_den); t.dout = cv(c.dout);
        t.dq = cmv(c.dq_num); t.dk = cmv(c.dk_num); t.dv = cmv(c.dv); t.dqd = cmv(c.dq_den); t.dkd = cmv(c.dk_den);
        t.idx = c.block_index; t.W = c.W; t.ldw = c.ldw; t.g = w.g; t.dkv = w.dkv; t.ninv = w.ninv; t.dz = w.dz; t.ksum = w.ksum;
        t.dks = w.dks; t.es = w.es;
        t.H = c.H; t.M = M; t.S = S; t.D = c.D; t.eps = c.eps; t.relu = c.relu(); t.normalize = c.normalize; t.split = c.split;
        t.rcos = c.rcos; t.rsin = c.rsin; t.ldr = c.ldr;
        RC((bm_tok<ET, DT, S16>(p, c, t)));
    });
    return MHLA_OK;
}

}  // namespace capi
}  // namespace mhla
