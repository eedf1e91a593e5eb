// Block-mix split kernels (split.hpp): k_sp_bwd_dq and k_sp_bwd_dkv, the token gradients.
#pragma once
#include "split_operands.hpp"

namespace mhla {
namespace sp {

// -------------------------------------------------------------------------------------------------
// Token gradients.  Both kernels keep one D x D matrix of the block in LDS as bf16 hi / lo and compute transposed
// products, so that the token tensors are MFMA B operands read straight from HBM (8 consecutive features per lane) and a
// lane ends up with 4 consecutive features of one token.
//   k_sp_bwd_dq : dQ_i = (dO_i / n_i) G_i^T (+ dz_i ksum_i^T) ; dksum_i = Qden_i^T dz_i ; dQden_i = dz_i ksum_i^T (split)
//   k_sp_bwd_dkv: dK_j = V_j dKV_j^T (+ dksum_j) ; dV_j = K_j dKV_j ; dKden_j = 1 dksum_j^T (split)
// -------------------------------------------------------------------------------------------------
// k_sp_bwd_dq: the staged G_i (ONEP: one payload plane, sp_payop), the waves' dksum partials [4][DW] and ksum [DW] -- not the store
// strips of k_sp_bwd_dkv below, which cost it a third of its workgroups per CU while it was launched with sp_tok_smem
template <int DT, int FMT, bool ONEP = false>
__host__ __device__ constexpr int sp_dq_smem() {
    return ((sf_has_lo(FMT) && !ONEP) ? 2 : 1) * Geo<DT>::KST * 32 * mat_ld<DT>() * 2 + Geo<DT>::DW * 4 * 4 + Geo<DT>::DW * 4;
}
static_assert(6 * sp_dq_smem<4, SF_F32>() <= 160 * 1024 && 6 * sp_dq_smem<4, SF_H16, true>() <= 160 * 1024, "six k_sp_bwd_dq workgroups per CU at D = 64");
template <int DT, int FMT>
__host__ __device__ constexpr int sp_tok_smem() {
    // (+ k_sp_bwd_dkv's row staging for 16-bit tensors with rows of up to 128 bytes: [4 waves][dK, dV][16 tokens][DW + 8] 16-bit values)
    return sp_dq_smem<DT, FMT>() + (DT <= 4 ? 4 * 2 * 16 * (Geo<DT>::DW + 8) * 2 : 0);
}

// ROPE: the numerator pair was rotated inside the forward (q_den aliases the un-rotated q): dQ_rot is turned back by the
// transposed rotation before dz ksum^T is added, so the one stored tensor is the gradient of the un-rotated q
// WQ: q_den enters only dksum (normaliser on, no relu prologue) and is fetched in 16-byte pieces in the operand layout; otherwise in
// the output layout, where the relu gradient mask needs it (a template flag: both register sets at once cost the occupancy)
// ONE: the launch has S <= 64, so a wave has at most its one tile `wave`: no loop, no second row set and no look-ahead -- the loop's
// unconditional prefetch asked for the wave's own rows a second time there (every dO and q_den piece, 1 / n, dz and a map entry)
struct DqVar { bool rope = false, wq = false, one = false; };
template <typename T, int DT, int FMT, DqVar V = DqVar{}>
__global__ __launch_bounds__(NTHREADS, (DT <= 4 && V.wq) ? 4 : 2) void k_sp_bwd_dq(const TokArgs a) {
    constexpr bool ROPE = V.rope, WQ = V.wq, ONE = V.one;
    constexpr int LD = mat_ld<DT>(), DW = Geo<DT>::DW, KST = Geo<DT>::KST, TILE = KST * 32 * LD;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr bool PAYOP = sp_payop<T, DT, FMT, ROPE>();   // G_i as ONE plane of its h16 payload, dO rows as scaled fp16 operands
    u16* Gh = reinterpret_cast<u16*>(smem_raw);
    u16* Gl = Gh + TILE;                                  // not allocated for bf16 summaries (or PAYOP)
    float* dksw = reinterpret_cast<float*>(Gh + ((sf_has_lo(FMT) && !PAYOP) ? 2 : 1) * TILE);   // [4 waves][DW]
    float* ksum = dksw + 4 * DW;                          // [DW]
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nl = lane & 15, kg = lane >> 4;
    const int blk = blockIdx.x, bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H, S = a.S, D = a.D, M = a.M;
    const long p0 = (long)blk * S;
    auto base = [&](const View& w) { return (const T*)w.ptr + b * w.sb + h * w.sh; };
    auto mbase = [&](const MView& w) { return (T*)w.ptr + b * w.sb + h * w.sh; };
    const T *gb = base(a.dout), *qdb = base(a.qd);
    T *dqb = mbase(a.dq), *dqdb = a.split ? mbase(a.dqd) : nullptr;
    const float* ninvb = a.ninv + ((long)bh * M + blk) * S;
    const float* dzb = a.dz + ((long)bh * M + blk) * S;
    constexpr bool wide_q = WQ;   // (the launch picks WQ = normalize && !relu)
    const bool wide_dq = view16(a.dq), wide_dqd = a.split && view16(a.dqd);   // (uniform) 16-byte store layout

    // one 16-token tile of this wave: the lane's token row, its dO features as the MFMA B operand (8 per reduction step) and
    // its q_den features in output layout (4 per feature tile); fetched one tile ahead of the tile being computed
    // (the rows AS LOADED, every load unconditional from a clamped address, nothing touched before the tile that consumes it, the gather
    // map looked up one fetch ahead: see k_sp_bwd_dkv)
    struct Rows {
        typename Raw4<T>::type g[KST][2];
        typename Raw4<T>::type qd[WQ ? 1 : DT];         // q_den in output layout (relu prologue: the gradient mask needs it there)
        typename Raw4<T>::type qw[WQ ? KST : 1][2];     // ... or in the operand layout of g (8 features per reduction step: 16-byte loads), for dksum only
        float ninv, dz;
        long row;
        bool live;
    } cur, nxt;
    const float* standin = a.g;
    auto look = [&](int tt) { return gld<int>(a.idx ? a.idx + p0 + min(tt * 16 + nl, S - 1) : reinterpret_cast<const int*>(a.g)); };
    auto fetch = [&](int tt, Rows& R, int looked) __attribute__((always_inline)) {
        const int s = tt * 16 + nl, sv = min(s, S - 1);
        R.live = s < S;
        R.row = a.idx ? (long)looked : p0 + sv;
        R.ninv = gld<float>(a.normalize ? ninvb + sv : standin);   // (1 / 0 are selected where the values are used)
        R.dz = gld<float>(a.normalize ? dzb + sv : standin);
        const T* grow = gb + R.row * a.dout.sn;
        const T* qrow = qdb + R.row * a.qd.sn;
#pragma unroll
        for (int ks = 0; ks < KST; ++ks) {
            const int c = ks * 32 + kg * 8 < D ? ks * 32 + kg * 8 : 0;
            R.g[ks][0] = gld<typename Raw4<T>::type>(grow + c);
            R.g[ks][1] = gld<typename Raw4<T>::type>(grow + c + 4);
        }
        if constexpr (!WQ) {
#pragma unroll
            for (int ct = 0; ct < DT; ++ct) R.qd[ct] = gld<typename Raw4<T>::type>(qrow + (ct * 16 + kg * 4 < D ? ct * 16 + kg * 4 : 0));
        }
        // no relu prologue: q_den is needed for dksum = sum_s dz[s] q[s][:] alone -- 8 features per load, as the dO rows (the 4-feature
        // pieces of the output layout are 8-byte loads for 16-bit tensors: 0.54-0.70 of the 16-byte rate)
        if constexpr (WQ) {
#pragma unroll
            for (int ks = 0; ks < KST; ++ks) {
                const int c = ks * 32 + kg * 8 < D ? ks * 32 + kg * 8 : 0;
                R.qw[ks][0] = gld<typename Raw4<T>::type>(qrow + c);
                R.qw[ks][1] = gld<typename Raw4<T>::type>(qrow + c + 4);
            }
        }
    };
    int lk = 0;
    if (a.idx) lk = gld<int>(a.idx + p0 + min(wave * 16 + nl, S - 1));   // (uniform branch; nothing is in flight yet)
    fetch(wave, cur, lk);   // in flight while G_i is staged
    if constexpr (!ONE) lk = look(wave + 4);
    const float ksum_v = gld<float>(a.normalize ? a.ksum + ((long)bh * M + blk) * D + min(tid, D - 1) : standin);
    float gm = 1.f;   // PAYOP: the multiplier of G_i's payload
    if constexpr (PAYOP) gm = stage_mat_payload<DT>(Gh, a.g, ((long)bh * M + blk) * a.es, D, tid);
    else stage_mat_split<DT, FMT>(Gh, Gl, a.g, ((long)bh * M + blk) * a.es, D, tid);
    if (tid < DW) ksum[tid] = (a.normalize && tid < D) ? ksum_v : 0.f;
    __syncthreads();
    f32x4 dksp[WQ ? 1 : DT], dksw8[WQ ? KST : 1][2];   // per-lane dksum partials: output layout / operand layout (WQ)
#pragma unroll
    for (int ct = 0; ct < (WQ ? 1 : DT); ++ct) dksp[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < (WQ ? KST : 1); ++ks) dksw8[ks][0] = dksw8[ks][1] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto tile = [&]() __attribute__((always_inline)) {
        const float cninv = a.normalize ? cur.ninv : 1.f, cdz = (a.normalize && cur.live) ? cur.dz : 0.f;
        bf16x8 gh[KST], gl[KST];   // dO / n : B[k = d2][n = s]
        f16x8 g16[KST];            // PAYOP: dO 2^e, and m 2^-e / n for the accumulators (1 / n in fp32: dO / n is not rounded to 16 bits)
        float cscale = 1.f;
        if constexpr (PAYOP) {
            f32x4 x[KST][2];
#pragma unroll
            for (int ks = 0; ks < KST; ++ks) {
                const bool in = ks * 32 + kg * 8 < D;
                const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
                x[ks][0] = in ? raw4_to_f32(T{}, cur.g[ks][0]) : z4;
                x[ks][1] = in ? raw4_to_f32(T{}, cur.g[ks][1]) : z4;
            }
            cscale = (gm * cninv) * h16_inv(tok16_operands<KST>(x, g16));
        } else {
#pragma unroll
            for (int ks = 0; ks < KST; ++ks) {
                uint4 hi, lo;
                const bool in = ks * 32 + kg * 8 < D;
                const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
                split8((in ? raw4_to_f32(T{}, cur.g[ks][0]) : z4) * cninv, (in ? raw4_to_f32(T{}, cur.g[ks][1]) : z4) * cninv, hi, lo);
                gh[ks] = as_bf16x8(hi);
                gl[ks] = as_bf16x8(lo);
            }
        }
        // gradient of one feature tile in output layout (4 features of the lane's token) and its q_den companion
        auto epilogue = [&](int ct, f32x4& c, f32x4& cd, const f32x2& rc, const f32x2& rs) {
            const int d0 = ct * 16 + kg * 4;
            if constexpr (ROPE) unrope4(c, rc, rs);
            f32x4 qd = {0.f, 0.f, 0.f, 0.f};
            if constexpr (!WQ) {
                if ((a.normalize || a.relu) && d0 < D) qd = raw4_to_f32(T{}, cur.qd[ct]);   // (uniform / lane select; no memory operation)
            }
            if (a.relu)
#pragma unroll
                for (int i = 0; i < 4; ++i) qd[i] = fmaxf(qd[i], 0.f) + a.eps;
            const f32x4 ks4 = *reinterpret_cast<const f32x4*>(ksum + d0);
            cd = cdz * ks4;
            if (a.normalize) {
                if constexpr (!WQ) dksp[ct] += cdz * qd;
                if (!a.split) c += cd;
            }
            if (a.relu)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (!(qd[i] > a.eps)) c[i] = 0.f;
        };
#pragma unroll
        for (int ct = 0; ct < DT; ct += 2) {   // two feature tiles at a time: independent MFMA chains, adjacent stores
            constexpr int LAST = DT - 1;
            const int c1t = ct + 1 <= LAST ? ct + 1 : LAST;
            f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0;
            f32x2 rc0 = {1.f, 1.f}, rs0 = {0.f, 0.f}, rc1 = rc0, rs1 = rs0;   // the angles of the two tiles' features: in flight during the products
            if constexpr (ROPE) {
                const long ro = cur.row * a.ldr + kg * 2;
                if (ct * 16 + kg * 4 < D) { rc0 = *reinterpret_cast<const f32x2*>(a.rcos + ro + ct * 8); rs0 = *reinterpret_cast<const f32x2*>(a.rsin + ro + ct * 8); }
                if (c1t * 16 + kg * 4 < D) { rc1 = *reinterpret_cast<const f32x2*>(a.rcos + ro + c1t * 8); rs1 = *reinterpret_cast<const f32x2*>(a.rsin + ro + c1t * 8); }
            }
#pragma unroll
            for (int ks = 0; ks < KST; ++ks) {
                const bf16x8 a0h = mat_row_read8<mat_new<DT>()>(Gh, LD, ct * 16, ks * 32, lane), a1h = mat_row_read8<mat_new<DT>()>(Gh, LD, c1t * 16, ks * 32, lane);
                if constexpr (PAYOP) {
                    c0 = fast::mfma_f16(fast::as_f16x8(a0h), g16[ks], c0);
                    c1 = fast::mfma_f16(fast::as_f16x8(a1h), g16[ks], c1);
                } else {
                    c0 = mfma_bf16(a0h, gh[ks], c0);
                    c1 = mfma_bf16(a1h, gh[ks], c1);
                    if (sf_has_lo(FMT)) {
                        const bf16x8 a0l = mat_row_read8<mat_new<DT>()>(Gl, LD, ct * 16, ks * 32, lane), a1l = mat_row_read8<mat_new<DT>()>(Gl, LD, c1t * 16, ks * 32, lane);
                        c0 = mfma_bf16(a0l, gh[ks], c0);
                        c1 = mfma_bf16(a1l, gh[ks], c1);
                    }
                    c0 = mfma_bf16(a0h, gl[ks], c0);
                    c1 = mfma_bf16(a1h, gl[ks], c1);
                }
            }
            if constexpr (PAYOP) {
                c0 *= cscale;
                c1 *= cscale;
            }
            f32x4 e0, e1 = {0.f, 0.f, 0.f, 0.f};
            epilogue(ct, c0, e0, rc0, rs0);
            if (ct + 1 < DT) epilogue(ct + 1, c1, e1, rc1, rs1);
            // the two 64-byte halves of a 128-byte line go out in consecutive store instructions (write combining):
            // half-line stores separated in time cost a fill read and a second write per line
            store_tile_pair<T>(dqb + cur.row * a.dq.sn, ct, DT, D, kg, c0, c1, cur.live, wide_dq);
            if (a.normalize && a.split) store_tile_pair<T>(dqdb + cur.row * a.dqd.sn, ct, DT, D, kg, e0, e1, cur.live, wide_dqd);
            __builtin_amdgcn_sched_barrier(0);   // keep the LDS operand reads of later tiles from being hoisted (register pressure)
        }
        if constexpr (WQ) {
#pragma unroll
            for (int ks = 0; ks < KST; ++ks) {
                const bool in = ks * 32 + kg * 8 < D;
                const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
                dksw8[ks][0] += cdz * (in ? raw4_to_f32(T{}, cur.qw[ks][0]) : z4);
                dksw8[ks][1] += cdz * (in ? raw4_to_f32(T{}, cur.qw[ks][1]) : z4);
            }
        }
    };
    if constexpr (ONE) {
        if (wave * 16 < S) tile();   // (uniform)
    } else {
        for (int tt = wave; tt * 16 < S; tt += 4) {
            fetch((tt + 4) * 16 < S ? tt + 4 : tt, nxt, lk);   // (unconditional; the wave's last tile: itself again -- lines it has just read)
            lk = look(tt + 8);
            tile();
            cur = nxt;
        }
    }
    if (a.normalize) {   // dksum[d] = sum_s dz[s] qden[s][d]: over the 16 token lanes, then over the waves
        if constexpr (WQ) {   // the lane's features 32 ks + 8 kg + 0..7
#pragma unroll
            for (int ks = 0; ks < KST; ++ks)
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float v = row16_sum(dksw8[ks][i >> 2][i & 3]);
                    if (nl == 0 && ks * 32 + kg * 8 + i < DW) dksw[wave * DW + ks * 32 + kg * 8 + i] = v;
                }
        } else {
#pragma unroll
            for (int ct = 0; ct < (WQ ? 1 : DT); ++ct)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = row16_sum(dksp[ct][i]);
                    if (nl == 0) dksw[wave * DW + ct * 16 + kg * 4 + i] = v;
                }
        }
        __syncthreads();
        if (tid < D) a.dks[((long)bh * M + blk) * D + tid] = dksw[tid] + dksw[DW + tid] + dksw[2 * DW + tid] + dksw[3 * DW + tid];
    }
}

// ROPE: k is the un-rotated tensor: it is rotated on its way into the dV product (KV was formed from the rotated keys), and
// dK_rot is turned back before dksum is added
struct DkvVar { bool rope = false, lo = false; };   // lo: bf16 tensors under the relu prologue (relu(k) + eps keeps its lo part)
template <typename T, int DT, int FMT, DkvVar V = DkvVar{}>
__global__ __launch_bounds__(NTHREADS, 2) void k_sp_bwd_dkv(const TokArgs a) {   // (a bound of 4 -- 128 VGPRs, four workgroups per CU at D <= 64 -- measured: C2 +-0, blocks of 256 tokens 85 -> 94 us)
    constexpr bool ROPE = V.rope;
    constexpr int LD = mat_ld<DT>(), DW = Geo<DT>::DW, KST = Geo<DT>::KST, TILE = KST * 32 * LD;
    constexpr bool LO = !std::is_same<T, bf16_t>::value || V.lo;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u16* Gh = reinterpret_cast<u16*>(smem_raw);   // dKV_j [d1][d2]
    u16* Gl = Gh + TILE;                          // not allocated for bf16 summaries
    float* dks = reinterpret_cast<float*>(Gh + (sf_has_lo(FMT) ? 2 : 1) * TILE);   // [DW]
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nl = lane & 15, kg = lane >> 4;
    const int blk = blockIdx.x, bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H, S = a.S, D = a.D, M = a.M;
    const long p0 = (long)blk * S;
    auto base = [&](const View& w) { return (const T*)w.ptr + b * w.sb + h * w.sh; };
    auto mbase = [&](const MView& w) { return (T*)w.ptr + b * w.sb + h * w.sh; };
    const T *kb = base(a.k), *vb = base(a.v);
    T *dkb = mbase(a.dk), *dvb = mbase(a.dv), *dkdb = a.split ? mbase(a.dkd) : nullptr;

    // A tile's rows AS LOADED (converted, masked and relu'd where they are used): every load of a fetch is unconditional, from clamped
    // addresses, and nothing touches a loaded value before the tile that consumes it.  The fetch used to convert on arrival, sit behind
    // `if (column < D)` / `if (a.relu)` and look its gather-map entry up itself: in the listing every piece was `load, s_waitcnt vmcnt(0)`
    // -- ten serial round trips in front of the first tile and seven per prefetch (tools/isa_waits.py).
    struct Rows {
        typename Raw4<T>::type v[KST][2], k[KST][2];   // B operands: 8 features per reduction step
        typename Raw4<T>::type km[ROPE ? 1 : DT];      // k in output layout (gradient mask of the relu prologue; never combined with the rotary one)
        f32x4 rc[ROPE ? KST : 1], rs[ROPE ? KST : 1];   // angles of the B-operand features (4 pairs per reduction step)
        long row;
        bool live;
    } cur, nxt;
    // the gather map's entry of the lane's row, looked up one fetch ahead (without a map: the summaries' first word, dropped)
    // (a wave whose tile is the block's last prefetches ITS OWN tile again -- lines it has just read; re-reading the block's last tile cost
    // the L2 a second pass over K and V, and a stand-in address selected by `has a next tile` became a branch around the loads.  A loop-free
    // second copy of the tile body for blocks of one tile per wave cost 30 registers and the fourth workgroup per CU; as an instantiation of
    // its own -- the form k_sp_bwd_dq and k_sp_out run at S <= 64 -- it took 78 registers for 126 and measured 61.9 -> 61.4, 61.9 -> 61.4 and
    // 62.2 -> 62.4 us at C2: this kernel's branch already keeps the second request away, so there was nothing to remove)
    auto look = [&](int tt) { return gld<int>(a.idx ? a.idx + p0 + min(tt * 16 + nl, S - 1) : reinterpret_cast<const int*>(a.dkv)); };
    auto fetch = [&](int tt, Rows& R, int looked) __attribute__((always_inline)) {
        const int s = tt * 16 + nl, sv = min(s, S - 1);
        R.live = s < S;
        R.row = a.idx ? (long)looked : p0 + sv;
        const T* vrow = vb + R.row * a.v.sn;
        const T* krow = kb + R.row * a.k.sn;
#pragma unroll
        for (int ks = 0; ks < KST; ++ks) {
            const int c = ks * 32 + kg * 8 < D ? ks * 32 + kg * 8 : 0;
            R.v[ks][0] = gld<typename Raw4<T>::type>(vrow + c);
            R.v[ks][1] = gld<typename Raw4<T>::type>(vrow + c + 4);
            R.k[ks][0] = gld<typename Raw4<T>::type>(krow + c);
            R.k[ks][1] = gld<typename Raw4<T>::type>(krow + c + 4);
            if constexpr (ROPE) {   // unconditional, clamped: features past D are zeros whatever their angle (a branch or a select
                const int co = min(ks * 16 + kg * 4, D / 2 - 4);   // of whole vectors here puts the arrays on the stack)
                R.rc[ks] = *reinterpret_cast<const f32x4*>(a.rcos + R.row * a.ldr + co);
                R.rs[ks] = *reinterpret_cast<const f32x4*>(a.rsin + R.row * a.ldr + co);
            }
        }
        if constexpr (!ROPE) {   // (pieces of lines the operand loads fetch anyway; used under the relu prologue only)
            if (DT <= 4 || a.relu) {   // (head dims above 64: 32 registers of fp32 pieces -- only when they are used)
#pragma unroll
                for (int ct = 0; ct < DT; ++ct) R.km[ct] = gld<typename Raw4<T>::type>(krow + (ct * 16 + kg * 4 < D ? ct * 16 + kg * 4 : 0));
            }
        }
    };
    const bool wide_dk = view16(a.dk), wide_dv = view16(a.dv);   // (uniform) 16-byte store layout
    int lk = 0;
    if (a.idx) lk = gld<int>(a.idx + p0 + min(wave * 16 + nl, S - 1));   // (uniform branch; nothing is in flight yet)
    fetch(wave, cur, lk);
    lk = look(wave + 4);
    const float dks_v = gld<float>(a.normalize ? a.dks + ((long)bh * M + blk) * D + min(tid, D - 1) : reinterpret_cast<const float*>(a.dkv));
    stage_mat_split<DT, FMT>(Gh, Gl, a.dkv, ((long)bh * M + blk) * a.es, D, tid);
    if (tid < DW) dks[tid] = (a.normalize && tid < D) ? dks_v : 0.f;
    __syncthreads();

    auto tile = [&]() __attribute__((always_inline)) {
        bf16x8 vh[KST], vl[KST], kh[KST], kl[KST];
        f32x4 dkst[2], dvst[2];
        // ROWST (16-bit tensors, rows of up to 128 bytes): the wave's dK and dV tiles go through a wave-private LDS strip and leave as WHOLE
        // rows -- 8 lanes x 16 bytes per token, eight rows per store instruction.  In the product layout a store covered 16 half rows (64
        // bytes each) of two alternating output streams, and the L2 wrote a quarter of the lines twice (WRITE_SIZE 165 MB for 134 MB of
        // results at C2, with the fill reads on top).  (Keeping the tiles in registers and storing a row's pieces back to back behind the
        // loop -- no LDS -- was measured first: 79.6 -> 85.3 us, the stores start later.)
        constexpr bool ROWST = sizeof(T) == 2 && DT <= 4;
        constexpr int SLD = DW + 8;
        u16* stk = reinterpret_cast<u16*>(dks + DW) + wave * 2 * 16 * SLD;   // [dK, dV][16][SLD]
#pragma unroll
        for (int ks = 0; ks < KST; ++ks) {
            uint4 hi, lo;
            const bool in = ks * 32 + kg * 8 < D;
            const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
            split8(in ? raw4_to_f32(T{}, cur.v[ks][0]) : z4, in ? raw4_to_f32(T{}, cur.v[ks][1]) : z4, hi, lo);
            vh[ks] = as_bf16x8(hi);
            vl[ks] = as_bf16x8(lo);
            f32x4 y0 = in ? raw4_to_f32(T{}, cur.k[ks][0]) : z4, y1 = in ? raw4_to_f32(T{}, cur.k[ks][1]) : z4;
            if constexpr (ROPE) rope8(y0, y1, cur.rc[ks], cur.rs[ks]);
            else if (a.relu && in) relu8(y0, y1, a.eps);
            split8(y0, y1, hi, lo);
            kh[ks] = as_bf16x8(hi);
            kl[ks] = as_bf16x8(lo);
        }
#pragma unroll
        for (int ct = 0; ct < DT; ++ct) {
            f32x4 ck = {0.f, 0.f, 0.f, 0.f}, cv = ck;
            f32x2 urc = {1.f, 1.f}, urs = {0.f, 0.f};
            if constexpr (ROPE) {
                if (ct * 16 + kg * 4 < D) {
                    urc = *reinterpret_cast<const f32x2*>(a.rcos + cur.row * a.ldr + ct * 8 + kg * 2);
                    urs = *reinterpret_cast<const f32x2*>(a.rsin + cur.row * a.ldr + ct * 8 + kg * 2);
                }
            }
#pragma unroll
            for (int ks = 0; ks < KST; ++ks) {
                // dK^T[d1][s] = sum_d2 dKV[d1][d2] V[s][d2]
                const bf16x8 ah = mat_row_read8<mat_new<DT>()>(Gh, LD, ct * 16, ks * 32, lane);
                // dV^T[d2][s] = sum_d1 dKV[d1][d2] K[s][d1]
                const bf16x8 th = mat_tr_read8<mat_new<DT>()>(Gh, LD, ks * 32, ct * 16, lane);
                ck = mfma_bf16(ah, vh[ks], ck);
                cv = mfma_bf16(th, kh[ks], cv);
                if (sf_has_lo(FMT)) {
                    const bf16x8 al = mat_row_read8<mat_new<DT>()>(Gl, LD, ct * 16, ks * 32, lane), tl = mat_tr_read8<mat_new<DT>()>(Gl, LD, ks * 32, ct * 16, lane);
                    ck = mfma_bf16(al, vh[ks], ck);
                    cv = mfma_bf16(tl, kh[ks], cv);
                }
                if (LO) {
                    ck = mfma_bf16(ah, vl[ks], ck);
                    cv = mfma_bf16(th, kl[ks], cv);
                }
            }
            const int d0 = ct * 16 + kg * 4;
            if constexpr (ROPE) unrope4(ck, urc, urs);
            if (a.normalize && !a.split) ck += *reinterpret_cast<const f32x4*>(dks + d0);
            if constexpr (!ROPE) {
                if (a.relu && ct * 16 + kg * 4 < D) {
                    const f32x4 kmf = raw4_to_f32(T{}, cur.km[ct]);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (!(fmaxf(kmf[i], 0.f) + a.eps > a.eps)) ck[i] = 0.f;
                }
            }
            if constexpr (ROWST) {
                const uint2 pk = std::is_same<T, bf16_t>::value ? make_uint2(pack_bf16x2(ck[0], ck[1]), pack_bf16x2(ck[2], ck[3])) : make_uint2(h16_pack2(ck[0], ck[1]), h16_pack2(ck[2], ck[3]));
                const uint2 pv = std::is_same<T, bf16_t>::value ? make_uint2(pack_bf16x2(cv[0], cv[1]), pack_bf16x2(cv[2], cv[3])) : make_uint2(h16_pack2(cv[0], cv[1]), h16_pack2(cv[2], cv[3]));
                *reinterpret_cast<uint2*>(stk + nl * SLD + ct * 16 + kg * 4) = pk;
                *reinterpret_cast<uint2*>(stk + 16 * SLD + nl * SLD + ct * 16 + kg * 4) = pv;
            } else {
            dkst[ct & 1] = ck;
            dvst[ct & 1] = cv;
            if ((ct & 1) || ct == DT - 1) {   // store pairs of feature tiles: whole 128-byte lines (fp32) / 16-byte pieces (16-bit tensors)
                const int cta = ct & ~1, nt2 = (ct & 1) ? DT : cta + 1;   // (a lone last tile: no partner)
                store_tile_pair<T>(dkb + cur.row * a.dk.sn, cta, nt2, D, kg, dkst[0], dkst[1], cur.live, wide_dk);
                store_tile_pair<T>(dvb + cur.row * a.dv.sn, cta, nt2, D, kg, dvst[0], dvst[1], cur.live, wide_dv);
                if (a.normalize && a.split && cur.live) {
                    const int da = cta * 16 + kg * 4, db = da + 16;
                    const bool sa = da < D, sb = (ct & 1) && db < D;
                    if (sa) Io<T>::st4(dkdb + cur.row * a.dkd.sn + da, *reinterpret_cast<const f32x4*>(dks + da));
                    if (sb) Io<T>::st4(dkdb + cur.row * a.dkd.sn + db, *reinterpret_cast<const f32x4*>(dks + db));
                }
            }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (ROWST) {
            __builtin_amdgcn_wave_barrier();
            const bool wide = wide_dk && wide_dv;   // (uniform) 16-byte aligned rows: whole-row stores; otherwise 8-byte pieces from the strip
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
                const int r = (lane >> 3) + 8 * ps, c = (lane & 7) * 8;   // token r of the tile, features c .. c + 7
                const long grow = __shfl(cur.row, r, 64);                 // (lanes 0 .. 15 hold the rows of tokens 0 .. 15)
                const bool glive = __shfl((int)cur.live, r, 64) != 0;
                if (wide) {
                    if (glive && c < D) {
                        gst<uint4>(dkb + grow * a.dk.sn + c, *reinterpret_cast<const uint4*>(stk + r * SLD + c));
                        gst<uint4>(dvb + grow * a.dv.sn + c, *reinterpret_cast<const uint4*>(stk + 16 * SLD + r * SLD + c));
                    }
                } else if (glive) {
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf)
                        if (c + 4 * hf < D) {
                            *reinterpret_cast<uint2*>(dkb + grow * a.dk.sn + c + 4 * hf) = *reinterpret_cast<const uint2*>(stk + r * SLD + c + 4 * hf);
                            *reinterpret_cast<uint2*>(dvb + grow * a.dv.sn + c + 4 * hf) = *reinterpret_cast<const uint2*>(stk + 16 * SLD + r * SLD + c + 4 * hf);
                        }
                }
            }
            if (a.normalize && a.split && cur.live) {
#pragma unroll
                for (int ct = 0; ct < DT; ++ct) {
                    const int da = ct * 16 + kg * 4;
                    if (da < D) Io<T>::st4(dkdb + cur.row * a.dkd.sn + da, *reinterpret_cast<const f32x4*>(dks + da));
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    };
    for (int tt = wave; tt * 16 < S; tt += 4) {
#ifdef DKV_UNCOND_PREFETCH
        fetch((tt + 4) * 16 < S ? tt + 4 : tt, nxt, lk);   // (unconditional; the wave's last tile: itself again -- lines it has just read)
        lk = look(tt + 8);
#else
        // (a branch around the prefetch: where it joins hipcc waits for the prefetch itself, so blocks of more than 64 tokens do not overlap it
        // with the products -- but the unconditional form, which re-reads the wave's own tile when there is no next one, measured slower here
        // at every block length but 16: twelve row pieces and the mask pieces per lane are a lot of requests to issue twice)
        if ((tt + 4) * 16 < S) {
            fetch(tt + 4, nxt, lk);
            lk = look(tt + 8);
        }
#endif
        tile();
        cur = nxt;
    }
}

}  // namespace sp
}  // namespace mhla
