// Block-mix split kernels (split.hpp): k_sp_state, the block summaries (forward) and their gradients (backward).
#pragma once
#include "split_operands.hpp"

namespace mhla {
namespace sp {

template <int DT>
__host__ __device__ constexpr int sp_state_smem() {
    // the column-sum partials [RPP][DW] of the epilogue reuse the tiles
    static_assert(Geo<DT>::RPP * Geo<DT>::DW * 4 <= 4 * 32 * Geo<DT>::LD * 2, "column-sum partials must fit in the tiles");
    return 4 * 32 * Geo<DT>::LD * 2 + Geo<DT>::DW * 4;
}

// MODE 1 on 16-bit tensors with 24-bit summaries and D <= 64 (RD): the row dots dO . O come from G_i -- two more tiles (G_i as hi / lo,
// [64][72] bf16 each) and the partial dots of a 32-token chunk
// ONEP (sp_payrd: h16 summaries, bf16 tensors): G_i is one plane of its payload and dO travels as fp16 rows in the Kl tile, which bf16
// tensors leave unused -- the 10 KB pay for the conflict-free token layout (Geo::LD) and a fifth workgroup per CU
template <int DT, bool ONEP = false> __host__ __device__ constexpr int sp_state_rd_smem() {   // (!ONEP: its token tiles keep the rows of DW + 8: four workgroups per CU)
    return 4 * 32 * (ONEP ? Geo<DT>::LD : Geo<DT>::LDR) * 2 + Geo<DT>::DW * 4 + (ONEP ? 1 : 2) * Geo<DT>::KST * 32 * mat_ld<DT>() * 2 + 2 * 32 * 4;
}
// fp16 tensors keep the hi + lo form: their Kl tile holds q's lo part, and a fifth tile would cost the form its gain
template <typename T, int DT, int FMT>
__host__ __device__ constexpr bool sp_payrd() { return sp_payop<T, DT, FMT>() && std::is_same<T, bf16_t>::value; }
static_assert(!SP_PAYLOAD_OPERANDS || 5 * sp_state_rd_smem<4, true>() <= 160 * 1024, "five k_sp_state<1> (row dots from G) workgroups per CU at D = 64");

// MODE 0 (forward):  out = KV_j = K_j^T V_j; ksum_j; z_j                      x = k_num, y = v, kd = k_den, qd = q_den
// MODE 1 (backward): out = dG_i = Q_i^T (dO_i / n_i); dn_i[s] = -(dO_i[s] . O_i[s]) / n_i[s]     x = q_num, y = dout, o = out
// ROPE: x (the keys of the KV product in MODE 0, the queries of dG = Q^T dP in MODE 1) is rotated on load (a.rcos / a.rsin); a
// template flag so that the plain variants do not carry the angle registers (3 waves per SIMD need <= 168 VGPRs)
// NT: threads.  512 (D = 128 only): a 32-row chunk is one staging pass and every wave owns ONE 16-row tile of the summary -- half
// the staging and accumulator registers per thread (<= 128 VGPRs: two workgroups = 16 waves per CU) and half the time per block,
// which matters at the Wan shape for a second reason: 1 800 blocks on 768 four-wave slots are 2.3 rounds that cost 3, on 512
// eight-wave slots of half the duration 3.5 rounds that cost 4 (of half the length).
// FMT: the format `out` is stored in (and G_i read in, where the row dots come from it).  SF_BF16 is the opt-in MHLA_FLAG_BF16_SUMMARIES
// arithmetic on bf16 tensors; otherwise the one operand that is an INTERMEDIATE (dP = dO / n, MODE 1) is split into hi + lo parts
// whatever the tensor type
// PRO (MODE 0, Wan inference): x and qd are 16-bit projection outputs; relu(x * rstd[token] * w[channel]) + eps is applied on load
// (StateArgs::pro_*), the values then carry a lo part like fp32 tensors
// TS: the call may have a third token tensor (MODE 0: the split pair's k_den, MODE 1: the forward output).  false (MODE 0, picked by the
// launch when the call has no split normaliser pair): no third row stream -- it was pointed at the key rows again and its values zeroed,
// half as many requests again in the chunk loop -- and no registers for it
// LO (bf16 tensors under the relu prologue, MHLA_FLAG_RELU_EPS): relu(x) + eps is an fp32 value, not a bf16 one -- x keeps its lo part like
// an fp16 tensor's (and the Kl tile holds it: the row dots take the hi + lo form of fp16 tensors, not the fp16 dO rows kept there)
struct StateVar { bool rope = false, pro = false, ts = true, lo = false; };
template <typename T, int DT, int MODE, int NT, int FMT, StateVar V = StateVar{}>
__global__ __launch_bounds__(NT, NT == 512 ? 4 : (V.rope ? 2 : 3)) void k_sp_state(const StateArgs a) {
    constexpr bool ROPE = V.rope, PRO = V.pro, TS = V.ts;
    static_assert(TS || MODE == 0, "the backward's third tensor is a property of its arithmetic (RD), not of the call");
    static_assert(!PRO || (MODE == 0 && FMT != SF_BF16), "the prologue on load serves the forward's summary kernel on fp32-grade summaries");
    // RD: the row dots dO . O = dO' . (Q G_i) are formed from the mixed summary G_i (staged as hi / lo tiles beside the operand tiles): the
    // stored output and its residual are not read, and the forward does not write the residual (capi_common.hpp bm_rowdots_from_g)
    constexpr bool RD = MODE == 1 && sf_packed(FMT) && sizeof(T) == 2 && DT <= 4 && !ROPE;
    constexpr bool THIRD = TS && !RD;   // a third row stream exists
    static_assert(!V.lo || (std::is_same<T, bf16_t>::value && FMT != SF_BF16 && !PRO && !ROPE), "the lo flag marks the bf16 variant of the relu prologue");
    constexpr bool PAYRD = RD && sp_payrd<T, DT, FMT>() && !V.lo;   // the row dots on G_i's payload and fp16 dO rows (kept in the Kl tile)
    constexpr bool TN = !RD || PAYRD;   // the token tiles in the conflict-free layout (Geo::LD, mat_row)
    constexpr int DW = Geo<DT>::DW, LD = TN ? Geo<DT>::LD : Geo<DT>::LDR, CGS = Geo<DT>::CGS, RPP = NT / CGS, IT = 32 / RPP, NWV = NT / 64,
                  RT = (DT + NWV - 1) / NWV, TILE = 32 * LD;
    static_assert(IT >= 1 && RPP * IT == 32, "a 32-row chunk must be whole staging passes");
    static_assert(RPP * DW * 4 <= 4 * 32 * LD * 2, "column-sum partials must fit in the tiles");
    constexpr bool LO = !std::is_same<T, bf16_t>::value || PRO || V.lo || (ROPE && sf_has_lo(FMT));   // the token operands carry a lo part (a rotated bf16 value is an fp32 one)
    constexpr bool LOY = !std::is_same<T, bf16_t>::value || (MODE == 1 && sf_has_lo(FMT));   // ... and so does y = dO / n, unless the reduced-precision form was asked for
    constexpr int GLD = mat_ld<DT>(), GT = Geo<DT>::KST * 32 * GLD;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u16* Kh = reinterpret_cast<u16*>(smem_raw);
    u16* Kl = Kh + TILE;
    u16* Vh = Kl + TILE;
    u16* Vl = Vh + TILE;
    float* cs = reinterpret_cast<float*>(smem_raw);    // [RPP][DW] column-sum partials: over the tiles, after the last product
    float* vecd = reinterpret_cast<float*>(Vl + TILE); // [DW] ksum
    u16* Gh = reinterpret_cast<u16*>(vecd + DW);       // RD: G_i [d1][d2] hi, lo ([KST * 32][GLD] each), then the chunk's partial row dots [2][32]
    u16* Gl = Gh + GT;                                 // (PAYRD: one plane)
    float* rdp = reinterpret_cast<float*>(Gh + (PAYRD ? 1 : 2) * GT);
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nl = lane & 15, kg = lane >> 4;
    const int blk = blockIdx.x, bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H, S = a.S, D = a.D;
    const long p0 = (long)blk * S;
    const T* kb = (const T*)a.x.ptr + b * a.x.sb + h * a.x.sh;
    const T* vb = (const T*)a.y.ptr + b * a.y.sb + h * a.y.sh;
    const View& third = MODE == 0 ? a.kd : a.o;   // MODE 0: the normaliser's keys; MODE 1: the forward output
    const T* kdb = (const T*)third.ptr + b * third.sb + h * third.sh;
    const bool den = THIRD && a.normalize && ((MODE == 1 && !RD) || (MODE == 0 && a.split));   // a third tensor is read
    const int r0 = tid / CGS, cg = (tid % CGS) * 8;
    const float* ninvb = a.ninv + ((long)bh * a.M + blk) * S;   // MODE 1

    // the chunk's rows AS LOADED (kr, vr, dr): converted in `settle`, at the commit -- `ld8` converted them as they arrived, i.e. the wait for
    // the next chunk sat right behind its request, in front of this chunk's products (tools/isa_waits.py: `L L L L W3 W2` at the loop top)
    typename Raw4<T>::type kr[IT][2], vr[IT][2], dr[THIRD ? IT : 1][2];
    f32x4 kx[IT][2], vx[IT][2], dx[THIRD ? IT : 1][2], rc[ROPE ? IT : 1], rs[ROPE ? IT : 1];
    float nv[IT];
    float prr[PRO ? IT : 1];   // PRO: the rows' rstd
    f32x4 pw[PRO ? 2 : 1];     // ... and the norm weights of the thread's 8 channels
    constexpr bool rope = ROPE;
    int crow = 0;   // first token of the chunk held in registers
    // Gather map: the rows of a chunk are looked up ONE FETCH EARLIER than they are used (clamped, unconditional), so that a fetch
    // is one memory round trip, not two (map entry, then the row it names) -- with the map the chunk-ahead prefetch was a chain
    // of two latencies against one 32-row chunk of products.
    int nraw[IT], npos[IT];   // the map entry as loaded, and the position it was loaded for (used when there is no map)
    auto lookup = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const long p = p0 + min(c0 + r0 + RPP * it, S - 1);
            // (no branch around the load -- hipcc waits for everything in flight where a branch with a load in it joins: without
            // a map the load reads the first word of x and its result is dropped -- and no use of the loaded value before the next
            // fetch: a select right here would wait for it, and for the data loads issued before it)
            nraw[it] = gld<int>(a.idx ? (const void*)(a.idx + p) : a.x.ptr);
            npos[it] = (int)p;
        }
    };
    lookup(0);
    // Every load of a fetch is unconditional (rows past the block's end and column groups past D are clamped onto valid ones and
    // zeroed in `commit`; a tensor the call does not have is replaced by x and its values dropped): a load behind a branch makes
    // hipcc wait for everything in flight where the branch joins, i.e. before the products the prefetch is meant to overlap.
    const int cgc = min(cg, D - 8);
    if constexpr (PRO) {
        pw[0] = pw[1] = f32x4{1.f, 1.f, 1.f, 1.f};
        if (a.pro_wk) {
            pw[0] = *reinterpret_cast<const f32x4*>(a.pro_wk + h * D + cgc);
            pw[1] = *reinterpret_cast<const f32x4*>(a.pro_wk + h * D + cgc + 4);
        }
    }
    const T* kdq = den ? kdb : kb;                  // (uniform selects)
    const long kdsn = den ? third.sn : a.x.sn;
    const float* nvp = (MODE == 1 && a.normalize) ? ninvb : reinterpret_cast<const float*>(a.x.ptr);
    // MODE 1, 16-bit tensors at the default arithmetic: the residual of the forward's store of O (StateArgs::olo), fetched with
    // the rows (unconditionally: without it, the first bytes of x, dropped in `settle`)
    constexpr bool OLO = MODE == 1 && sf_has_lo(FMT) && sizeof(T) == 2 && !RD;
    const bool olo_on = OLO && a.normalize && a.olo != nullptr;
    const u16* olop = olo_on ? a.olo + ((long)bh * a.M * S + p0) * D + cgc : reinterpret_cast<const u16*>(a.x.ptr);
    uint4 ox[OLO ? IT : 1];
    auto fetch = [&](int c0) __attribute__((always_inline)) {
        crow = c0;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int rcl = min(c0 + r0 + RPP * it, S - 1);
            const long row = a.idx ? nraw[it] : npos[it];
            kr[it][0] = gld<typename Raw4<T>::type>(kb + row * a.x.sn + cgc);
            kr[it][1] = gld<typename Raw4<T>::type>(kb + row * a.x.sn + cgc + 4);
            vr[it][0] = gld<typename Raw4<T>::type>(vb + row * a.y.sn + cgc);
            vr[it][1] = gld<typename Raw4<T>::type>(vb + row * a.y.sn + cgc + 4);
            if constexpr (THIRD) {
                dr[it][0] = gld<typename Raw4<T>::type>(kdq + row * kdsn + cgc);
                dr[it][1] = gld<typename Raw4<T>::type>(kdq + row * kdsn + cgc + 4);
            }
            nv[it] = gld<float>(nvp + ((MODE == 1 && a.normalize) ? rcl : 0));
            if constexpr (PRO) prr[it] = gld<float>(a.pro_rk ? a.pro_rk + b * a.pro_n + row : reinterpret_cast<const float*>(a.x.ptr));
            if constexpr (OLO) ox[it] = gld<uint4>(olop + (olo_on ? (long)rcl * D : 0));
            if constexpr (rope) {
                rc[it] = *reinterpret_cast<const f32x4*>(a.rcos + row * a.ldr + cgc / 2);
                rs[it] = *reinterpret_cast<const f32x4*>(a.rsin + row * a.ldr + cgc / 2);
            }
        }
        lookup(c0 + 32);   // (the rows of the next fetch)
    };
    // what `fetch` used to do behind its branch: zeros for padded rows / columns, relu + eps on the keys, 1 for an absent 1 / n
    auto settle = [&]() __attribute__((always_inline)) {   // (two call sites since the loop's last chunk was peeled: left to the inliner's size
                                                            //  heuristics, the register arrays these lambdas share went to scratch)
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const bool valid = crow + r0 + RPP * it < S && cg < D;
            const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                kx[it][hf] = raw4_to_f32(T{}, kr[it][hf]);
                vx[it][hf] = raw4_to_f32(T{}, vr[it][hf]);
                if constexpr (THIRD) dx[it][hf] = raw4_to_f32(T{}, dr[it][hf]);
            }
            if constexpr (PRO) {
                const float r = a.pro_rk ? prr[it] : 1.f;   // ((x rstd) w: the order of k_qk_prologue, so that the two paths agree bit for bit)
                kx[it][0] = (kx[it][0] * r) * pw[0];
                kx[it][1] = (kx[it][1] * r) * pw[1];
            }
            if (a.relu) relu8(kx[it][0], kx[it][1], a.eps);
            kx[it][0] = valid ? kx[it][0] : z4; kx[it][1] = valid ? kx[it][1] : z4;
            vx[it][0] = valid ? vx[it][0] : z4; vx[it][1] = valid ? vx[it][1] : z4;
            if constexpr (THIRD) { dx[it][0] = (valid && den) ? dx[it][0] : z4; dx[it][1] = (valid && den) ? dx[it][1] : z4; }
            if constexpr (OLO) {   // O = stored value + what the store rounded away
                const unsigned w[4] = {ox[it].x, ox[it].y, ox[it].z, ox[it].w};
                const bool on = valid && olo_on;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    dx[it][0][2 * i] += on ? __uint_as_float(w[i] << 16) : 0.f;
                    dx[it][0][2 * i + 1] += on ? __uint_as_float(w[i] & 0xffff0000u) : 0.f;
                    dx[it][1][2 * i] += on ? __uint_as_float(w[2 + i] << 16) : 0.f;
                    dx[it][1][2 * i + 1] += on ? __uint_as_float(w[2 + i] & 0xffff0000u) : 0.f;
                }
            }
            nv[it] = (valid && MODE == 1 && a.normalize) ? nv[it] : 1.f;
            if constexpr (rope) {   // padded rows: 0 * (uninitialised angle) could be NaN
                rc[it] = valid ? rc[it] : z4;
                rs[it] = valid ? rs[it] : z4;
            }
        }
    };
    float ksp[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float nvc[IT];   // RD: 1 / n (PAYRD: m 2^-e / n^2, the row's whole factor) and the first row of the chunk whose row dots are in flight
    int crowc = 0;
    float gm = 1.f;  // PAYRD: the multiplier of G_i's payload
    auto commit = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);   // (the fetched values are not touched before this point: hipcc would hoist `settle` above the products and wait there)
        settle();
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int off = mat_row<TN>(r0 + RPP * it) * LD + cg;
            uint4 hi, lo;
            if (MODE == 1 && a.normalize) {   // dn[s] and the 1/n scaling of dO
                if constexpr (THIRD) {
                    float d = 0.f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) d += vx[it][0][i] * dx[it][0][i] + vx[it][1][i] * dx[it][1][i];
#pragma unroll
                    for (int o = CGS / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
                    const int r = crow + r0 + RPP * it;
                    if (r < S && (tid % CGS) == 0) a.dn[((long)bh * a.M + blk) * S + r] = -d * nv[it];
                } else {
                    nvc[it] = nv[it];   // (the next fetch overwrites nv and crow before this chunk's dots are complete)
                    crowc = crow;
                    if constexpr (PAYRD) {   // the dO row itself, scaled into fp16, for the row dots: the CGS threads of a row share its maximum
                        float mx = 0.f;
#pragma unroll
                        for (int i = 0; i < 4; ++i) mx = fmaxf(mx, fmaxf(fabsf(vx[it][0][i]), fabsf(vx[it][1][i])));
                        const float u = tok16_scale<1, CGS>(mx);
                        *reinterpret_cast<uint4*>(Kl + off) = h16_pack8(vx[it][0], vx[it][1], u);
                        nvc[it] = ((gm * nv[it]) * h16_inv(u)) * nv[it];   // dO . O = (dO . q G) / n, and dn = -(dO . O) / n
                    }
                }
                vx[it][0] *= nv[it];
                vx[it][1] *= nv[it];
            }
            if constexpr (rope) {   // KV takes the rotated keys, ksum the plain ones
                f32x4 r0 = kx[it][0], r1 = kx[it][1];
                rope8(r0, r1, rc[it], rs[it]);
                split8(r0, r1, hi, lo);
            } else {
                split8(kx[it][0], kx[it][1], hi, lo);
            }
            *reinterpret_cast<uint4*>(Kh + off) = hi;
            if (LO) *reinterpret_cast<uint4*>(Kl + off) = lo;
            split8(vx[it][0], vx[it][1], hi, lo);
            *reinterpret_cast<uint4*>(Vh + off) = hi;
            if (LOY) *reinterpret_cast<uint4*>(Vl + off) = lo;
            if (MODE == 0) {
                const f32x4* s = kx[it];
                if constexpr (THIRD) s = den ? dx[it] : kx[it];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ksp[i] += s[0][i];
                    ksp[4 + i] += s[1][i];
                }
            }
        }
    };

    f32x4 acc[RT][DT];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < DT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    fetch(0);
    if constexpr (RD) {   // (its loads travel with the first chunk's; the loop's first barrier covers the tiles)
        if (a.normalize) {
            if constexpr (PAYRD) gm = stage_mat_payload<DT, NT>(Gh, a.g, ((long)bh * a.M + blk) * a.es, D, tid);
            else stage_mat_split<DT, FMT, NT>(Gh, Gl, a.g, ((long)bh * a.M + blk) * a.es, D, tid);
        }
    }
    // one 32-token chunk: commit, request the next one (PF: there is one -- a compile-time fact of the call site, so that no branch sits
    // around the request: where such a branch joins hipcc waits for the loads in it), products
    auto chunk = [&]<bool PF>(std::bool_constant<PF>, int c0) __attribute__((always_inline)) {
        commit();
        __syncthreads();
        if constexpr (PF) fetch(c0 + 32);
        if constexpr (RD) {
            // dots[s] = sum_d1 q[s][d1] T[d1][s],  T = G_i dO'^T (transposed product: a lane gets T[16 ct + 4 kg + r][s = nl]); wave w takes
            // token tile w & 1 of the chunk and the feature tiles of half w >> 1, the two halves meet in LDS after the loop's barrier
            if (a.normalize) {
                constexpr int KSTG = Geo<DT>::KST, CTH = (DT + 1) / 2;
                const int tt = wave & 1, hf = wave >> 1;
                bf16x8 bh_[KSTG], bl_[KSTG];   // dO / n as hi + lo; PAYRD: bh_ = the fp16 dO rows
#pragma unroll
                for (int ks = 0; ks < KSTG; ++ks) {
                    bh_[ks] = mat_row_read8<TN>(PAYRD ? Kl : Vh, LD, tt * 16, ks * 32, lane);
                    if constexpr (!PAYRD) bl_[ks] = mat_row_read8<TN>(Vl, LD, tt * 16, ks * 32, lane);
                }
                float dot = 0.f;
#pragma unroll
                for (int c = 0; c < CTH; ++c) {
                    const int ct = hf * CTH + c;
                    if (ct < DT) {   // (uniform)
                        f32x4 t4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int ks = 0; ks < KSTG; ++ks) {
                            const bf16x8 gh = mat_row_read8<mat_new<DT>()>(Gh, GLD, ct * 16, ks * 32, lane);
                            if constexpr (PAYRD) {
                                t4 = fast::mfma_f16(fast::as_f16x8(gh), fast::as_f16x8(bh_[ks]), t4);
                            } else {
                                const bf16x8 gl = mat_row_read8<mat_new<DT>()>(Gl, GLD, ct * 16, ks * 32, lane);
                                t4 = mfma_bf16(gh, bh_[ks], t4);
                                t4 = mfma_bf16(gl, bh_[ks], t4);
                                t4 = mfma_bf16(gh, bl_[ks], t4);
                            }
                        }
                        const uint2 qr = *reinterpret_cast<const uint2*>(Kh + (tt * 16 + mat_row<TN>(nl)) * LD + ct * 16 + kg * 4);   // q[s][16 ct + 4 kg ..]: hi part
                        f32x4 q4 = {__uint_as_float(qr.x << 16), __uint_as_float(qr.x & 0xffff0000u), __uint_as_float(qr.y << 16), __uint_as_float(qr.y & 0xffff0000u)};
                        if (LO) {   // (fp16 tensors, and bf16 ones under the relu prologue: + lo part; stored bf16 values are their hi part)
                            const uint2 ql = *reinterpret_cast<const uint2*>(Kl + (tt * 16 + mat_row<TN>(nl)) * LD + ct * 16 + kg * 4);
                            q4 += f32x4{__uint_as_float(ql.x << 16), __uint_as_float(ql.x & 0xffff0000u), __uint_as_float(ql.y << 16), __uint_as_float(ql.y & 0xffff0000u)};
                        }
                        dot += t4[0] * q4[0] + t4[1] * q4[1] + t4[2] * q4[2] + t4[3] * q4[3];
                    }
                }
                dot += __shfl_xor(dot, 16, 64);
                dot += __shfl_xor(dot, 32, 64);
                if (kg == 0) rdp[hf * 32 + tt * 16 + nl] = dot;
            }
        }
        bf16x8 ah[RT], al[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {   // row tiles past DT read zero / unused columns of the tile: harmless, not stored
            const int c0 = min(wave * RT + rt, DW / 16 - 1) * 16;
            ah[rt] = mat_tr_read8<TN>(Kh, LD, 0, c0, lane);
            if (LO) al[rt] = mat_tr_read8<TN>(Kl, LD, 0, c0, lane);
        }
#pragma unroll
        for (int ct = 0; ct < DT; ++ct) {
            const bf16x8 bh_ = mat_tr_read8<TN>(Vh, LD, 0, ct * 16, lane);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt][ct] = mfma_bf16(ah[rt], bh_, acc[rt][ct]);
            if (LOY) {
                const bf16x8 bl_ = mat_tr_read8<TN>(Vl, LD, 0, ct * 16, lane);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) acc[rt][ct] = mfma_bf16(ah[rt], bl_, acc[rt][ct]);
            }
            if (LO) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) acc[rt][ct] = mfma_bf16(al[rt], bh_, acc[rt][ct]);
            }
        }
        __syncthreads();
        if constexpr (RD) {   // dn[s] = -(dO . O)[s] / n[s] from the two halves of the chunk's row dots
            if (a.normalize && (tid % CGS) == 0) {
#pragma unroll
                for (int it = 0; it < IT; ++it) {
                    const int lr = r0 + RPP * it, r = crowc + lr;
                    if (r < S) a.dn[((long)bh * a.M + blk) * S + r] = -(rdp[lr] + rdp[32 + lr]) * nvc[it];
                }
            }
        }
    };
    int c0 = 0;
    for (; c0 + 32 < S; c0 += 32) chunk(std::true_type{}, c0);
    chunk(std::false_type{}, c0);   // (the block's last chunk)

    // KV_j -> ws  (C layout: row d1 = 16 tile + 4 kg + r, column d2 = 16 ct + nl)
    float* ob = a.out + ((long)bh * a.M + blk) * a.es;
    // fp32 summaries: through a wave-private LDS tile [16][CW + 4] (the operand tiles are free after the last product), so that a lane
    // stores 16-byte pieces and 16 lanes cover a whole row of the summary -- in the C layout a store instruction wrote four 64-byte
    // segments (k_sp_state ran at 3.9 TB/s of its bytes at C2)
    constexpr int CW = (DW > 64 && NWV == 8) ? 64 : DW, LDO = CW + 4, PPRO = CW / 4;
    static_assert(NWV * 16 * LDO * 4 <= 4 * 32 * LD * 2, "the staging tiles of all waves must fit in the operand tiles");
    const bool staged = sf_has_lo(FMT) && (sf_packed(FMT) || ((D & 3) == 0 && (a.es & 3) == 0));   // (uniform; p24: D % 8 == 0 by the path's shape test)
    float hinv = 0.f;   // h16: 1 / the row's multiplier
    if constexpr (FMT == SF_H16) {
        // the row's multiplier from the summary's largest magnitude: lane -> wave (shuffles) -> workgroup (NWV floats in `vecd`, free until
        // the column sums); padded rows / columns are zero products and do not matter
        float mx = 0.f;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < DT; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, fabsf(acc[rt][ct][r]));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        if (lane == 0) vecd[wave] = mx;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NWV; ++w) mx = fmaxf(mx, vecd[w]);
        const float hm = h16_mult_from_max(mx);
        hinv = h16_inv(hm);
        if (tid == 0) gst<float>(reinterpret_cast<char*>(ob) + 2 * D * D, hm);
    }
    if (staged) {
        float* Os = reinterpret_cast<float*>(smem_raw) + wave * 16 * LDO;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int tile = wave * RT + rt;
            if (tile * 16 < D) {   // (uniform)
#pragma unroll
                for (int c0 = 0; c0 < DW; c0 += CW) {
#pragma unroll
                    for (int ct = c0 / 16; ct < (c0 + CW) / 16; ++ct)
                        if (ct < DT)
#pragma unroll
                            for (int r = 0; r < 4; ++r) Os[(kg * 4 + r) * LDO + ct * 16 - c0 + nl] = acc[rt][ct][r];
                    __builtin_amdgcn_wave_barrier();
                    if constexpr (sf_packed(FMT)) {   // units of 8 elements: a 16-byte piece of the hi plane and an 8-byte piece of the lo plane
#pragma unroll
                        for (int p = 0; p < CW / 32; ++p) {
                            const int v = lane + 64 * p, row = v / (CW / 8), c8 = v % (CW / 8);
                            const int grow = tile * 16 + row, gcol = c0 + c8 * 8;
                            if (grow < D && gcol < D) {
                                const float* src = Os + row * LDO + c8 * 8;
                                const int e = grow * D + gcol;
                                if constexpr (FMT == SF_H16) {
                                    gst<uint4>(reinterpret_cast<char*>(ob) + 2 * e, h16_pack8(*reinterpret_cast<const f32x4*>(src), *reinterpret_cast<const f32x4*>(src + 4), hinv));
                                } else {
                                uint4 hi;
                                uint2 lo;
                                p24_pack8(*reinterpret_cast<const f32x4*>(src), *reinterpret_cast<const f32x4*>(src + 4), hi, lo);
                                gst<uint4>(reinterpret_cast<char*>(ob) + 2 * e, hi);
                                gst<uint2>(reinterpret_cast<char*>(ob) + 2 * D * D + e, lo);
                                }
                            }
                        }
                    } else {
#pragma unroll
                    for (int p = 0; p < CW / 16; ++p) {
                        const int v = lane + 64 * p, row = v / PPRO, c4 = v % PPRO;
                        const int grow = tile * 16 + row, gcol = c0 + c4 * 4;
                        if (grow < D && gcol < D) gst<f32x4>(ob + (long)grow * D + gcol, *reinterpret_cast<const f32x4*>(Os + row * LDO + c4 * 4));
                    }
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
        if (MODE == 0 && a.normalize) __syncthreads();   // (the column sums below reuse the tiles)
    } else {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < DT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = (wave * RT + rt) * 16 + kg * 4 + r, col = ct * 16 + nl;
                if (row < D && col < D) {
                    if (FMT == SF_BF16) reinterpret_cast<u16*>(a.out)[((long)bh * a.M + blk) * a.es + (long)row * D + col] = cvt_bf16(acc[rt][ct][r]);
                    else                 ob[(long)row * D + col] = acc[rt][ct][r];
                }
            }
    }

    if (MODE == 0 && a.normalize) {
#pragma unroll
        for (int i = 0; i < 8; ++i) cs[r0 * DW + cg + i] = ksp[i];
        __syncthreads();
        if (tid < DW) {
            float s = 0.f;
#pragma unroll 4
            for (int r = 0; r < RPP; ++r) s += cs[r * DW + tid];
            vecd[tid] = s;
            if (tid < D) a.ksum[((long)bh * a.M + blk) * D + tid] = s;
        }
        __syncthreads();
        // z_j[s] = Qden_j[s] . ksum_j : CGS lanes per token row
        const T* qb = (const T*)a.qd.ptr + b * a.qd.sb + h * a.qd.sh;
        float kv8[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) kv8[i] = vecd[cg + i];
        f32x4 qw[PRO ? 2 : 1];   // PRO: the q norm weights of the thread's channels
        if constexpr (PRO) {
            qw[0] = qw[1] = f32x4{1.f, 1.f, 1.f, 1.f};
            if (a.pro_wq && cg < D) {
                qw[0] = *reinterpret_cast<const f32x4*>(a.pro_wq + h * D + cg);
                qw[1] = *reinterpret_cast<const f32x4*>(a.pro_wq + h * D + cg + 4);
            }
        }
        constexpr int ZB = 4;   // token rows in flight per thread: the loads of a batch are issued before any is used
        for (int rb = 0; rb < S; rb += RPP * ZB) {
            f32x4 x0[ZB], x1[ZB];
            int rw[ZB];   // the batch's rows first (the map lookups travel together), then the batch's data loads
            if (a.idx) {
#pragma unroll
                for (int u = 0; u < ZB; ++u) rw[u] = gld<int>(a.idx + p0 + min(rb + u * RPP + r0, S - 1));
            } else {
#pragma unroll
                for (int u = 0; u < ZB; ++u) rw[u] = (int)p0 + min(rb + u * RPP + r0, S - 1);
            }
#pragma unroll
            for (int u = 0; u < ZB; ++u) {
                const int r = rb + u * RPP + r0;
                x0[u] = x1[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (r < S && cg < D) ld8(qb + (long)rw[u] * a.qd.sn + cg, x0[u], x1[u]);
            }
#pragma unroll
            for (int u = 0; u < ZB; ++u) {
                const int r = rb + u * RPP + r0;
                float d = 0.f;
                if (r < S && cg < D) {
                    if constexpr (PRO) {
                        const float rq = a.pro_rq ? a.pro_rq[b * a.pro_n + rw[u]] : 1.f;
                        x0[u] = (x0[u] * rq) * qw[0];
                        x1[u] = (x1[u] * rq) * qw[1];
                    }
                    if (a.relu) relu8(x0[u], x1[u], a.eps);
#pragma unroll
                    for (int i = 0; i < 4; ++i) d += x0[u][i] * kv8[i] + x1[u][i] * kv8[4 + i];
                }
#pragma unroll
                for (int o = CGS / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
                if (r < S && (tid % CGS) == 0) a.zo[((long)bh * a.M + blk) * S + r] = d;
            }
        }
    }
}

}  // namespace sp
}  // namespace mhla
