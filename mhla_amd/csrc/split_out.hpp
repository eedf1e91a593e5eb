// Block-mix split kernels (split.hpp): k_sp_out, the output tokens from the mixed summaries.
#pragma once
#include "split_operands.hpp"

namespace mhla {
namespace sp {

constexpr int SP_OUT_T = 512;   // 8 waves share the staged G_i: twice the loads in flight per LDS byte
// FLAT (24-bit summaries, 16-bit tensors): the launch is one persistent workgroup per CU and the token tiles of ALL blocks are one flat list
// cut into gridDim.x equal ranges; a workgroup walks its range in rounds of eight consecutive tiles (one per wave) with the summaries of
// the (at most two) blocks a round touches in two LDS buffers, the next block's pieces requested a round ahead.  A block per workgroup
// quantises twice at the Wan shape -- 14 tiles on 8 waves are two rounds (87.5 %), 1 800 workgroups on 256 CUs are eight waves of
// workgroups for 7.03 (88 %) -- 77 % together; the flat list leaves the last round of a range (98.4 tiles in 13 rounds: 94.6 %).
// OutArgs::nbh = B H; needs at least 8 tiles per block (a round then spans at most two blocks, the next round at most one more).
// ONE: the launch has S <= 64 -- a wave has its one tile `wave` at the most: no loop, no second row set, no fetch of a next tile (it was
// clamped onto the block's last row and dropped) and no map look-ahead
// ROPE (bf16 tensors): the launch has rotary tables -- the rotated q is an fp32 value and keeps its lo part, like fp32 / fp16 tensors and the
// prologue's values do (without it the variant of calls without tables, where a bf16 q is its own hi part, is unchanged)
struct OutVar { bool epi = false, pro = false, flat = false, one = false, rope = false, lo = false; };   // pro: the q prologue on load (OutArgs::pro_*)
template <typename T, int DT, typename TO, int FMT, OutVar V = OutVar{}>
#ifndef SP_OUT_EPI_WAVES
#define SP_OUT_EPI_WAVES 2   // the fused-epilogue variant takes 142 VGPRs: one workgroup per CU without spills (157 us at C4) beats two with 28 spilled registers (163 us)
#endif
__global__ __launch_bounds__(SP_OUT_T, V.epi ? SP_OUT_EPI_WAVES : 2) void k_sp_out(const OutArgs a) {
    constexpr bool EPI = V.epi, PRO = V.pro, FLAT = V.flat, ONE = V.one;
    constexpr int LD = mat_ld<DT>(), KST = Geo<DT>::KST, KP = KST * 32, TILE = KP * LD;
    constexpr bool LO = !std::is_same<T, bf16_t>::value || PRO || V.rope || V.lo;   // (lo: bf16 tensors under the relu prologue -- relu(q) + eps is no bf16 value)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    static_assert(!V.rope || (std::is_same<T, bf16_t>::value && sf_has_lo(FMT) && !PRO && !FLAT && !ONE), "the rotary flag marks the bf16 variant that keeps the lo part of the rotated q");
    static_assert(!FLAT || (FMT == SF_P24 && sizeof(T) == 2), "the flat tile list serves 16-bit tensors with 24-bit summaries");
    static_assert(!ONE || (!FLAT && SP_OUT_T / 64 >= 4), "one tile per wave: blocks of at most 64 tokens, one block per workgroup");
    u16* Gh = reinterpret_cast<u16*>(smem_raw);   // [d1][d2], rows >= D and columns >= D zero   (FLAT: two (hi, lo) pairs, block parity)
    u16* Gl = Gh + TILE;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nl = lane & 15, kg = lane >> 4;
    const int S = a.S, D = a.D;
    // the block in hand (FLAT: of the wave's tile of this round)
    int blk = blockIdx.x, bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
    long p0 = (long)blk * S;
    const T* qb = (const T*)a.q.ptr + b * a.q.sb + h * a.q.sh;
    TO* ob = (TO*)a.o.ptr + b * a.o.sb + h * a.o.sh;
    // The lane's token row of a 16-token tile as loaded: 8 q features per reduction step, 1 / n, (PRO) the token's rstd.  The first tile's
    // rows are requested BEFORE G_i is staged (one memory round trip per workgroup instead of two: a workgroup of the C2 step has one
    // tile per wave); 16-bit tensors also keep the wave's next tile in flight under the products (8 registers per reduction step).
    // Every load is unconditional, from clamped addresses (rows past the block: its last row; columns past D: the row's first piece).
    constexpr bool DBL = sizeof(T) == 2;
    // (Fetching the token's rope angles with its rows too -- 64 more registers in the fused-epilogue variants, which have them -- was
    // measured and lost: k_sp_out<norm,pro> 189 -> 218 us per Wan layer, the fp32 variant 176 -> 184.)
    struct QRows {
        typename Raw4<T>::type x[KST][2];
        float ninv, rq;
        long row;
    };
    QRows cur, nxt;
    // FLAT: tile g of the flat list = tile g % TPI of block g / TPI (blocks in the order of the summaries: (b, h) major)
    const int TPI = (S + 15) / 16;
    // the gather map's entry for the lane's row of a tile: looked up ONE FETCH AHEAD of the rows it names (unconditional: without a map the
    // load reads the summaries' first word and is dropped) -- looked up inside the fetch it was a dependent round trip in front of every
    // tile's loads, and behind `idx ? idx[p] : p` a branch with a load in it
    auto look = [&](int tt) __attribute__((always_inline)) {
        int fblk = blk;
        if constexpr (FLAT) {
            const int item = tt / TPI;
            tt -= item * TPI;
            fblk = item % a.M;
        }
        const long p = (long)fblk * S + min(tt * 16 + nl, S - 1);
        return gld<int>(a.idx ? a.idx + p : reinterpret_cast<const int*>(a.g));
    };
    auto fetch = [&](int tt, QRows& R, int looked) __attribute__((always_inline)) {   // (FLAT: tt is the tile's place in the flat list)
        int fb = b, fh = h, fbh = bh, fblk = blk;
        if constexpr (FLAT) {
            const int item = tt / TPI;
            tt -= item * TPI;
            fbh = item / a.M; fblk = item - fbh * a.M; fb = fbh / a.H; fh = fbh - fb * a.H;
        }
        const int sv = min(tt * 16 + nl, S - 1);
        R.row = a.idx ? (long)looked : (long)fblk * S + sv;
        const T* qrow = (const T*)a.q.ptr + fb * a.q.sb + fh * a.q.sh + R.row * a.q.sn;
#pragma unroll
        for (int ks = 0; ks < KST; ++ks) {
            const int c = ks * 32 + kg * 8 < D ? ks * 32 + kg * 8 : 0;
            R.x[ks][0] = *reinterpret_cast<const typename Raw4<T>::type*>(qrow + c);
            R.x[ks][1] = *reinterpret_cast<const typename Raw4<T>::type*>(qrow + c + 4);
        }
        R.ninv = gld<float>(a.normalize ? a.ninv + ((long)fbh * a.M + fblk) * S + sv : a.W);
        R.rq = 1.f;
        if constexpr (PRO) R.rq = gld<float>(a.pro_rq ? a.pro_rq + fb * a.pro_n + R.row : a.W);
    };
    // EARLY (the fused-epilogue variants: Wan): the prologue's channel weights and the rope angles of ALL reduction steps are requested
        // first, unconditionally (a table the call does not have is replaced by the summaries, its values dropped).  Fetched where they are
        // used -- behind `if (column < D)`, `if (a.pro_wq)`, `if (a.rcos)` -- every step's pieces were a round trip of their own (hipcc waits
        // for everything in flight where a branch with a load in it joins): ~17 serial L2 round trips per 16-token tile with the norm
        // weights of the epilogue, 12 us of a 13 us tile (tools/isa_waits.py: `L L W1 W0` x 8).
    // (`early` is called for the tile in hand BEFORE the next tile's rows and the next block's summary are requested: the wait for its values
    // then leaves those in flight -- the counter retires in order)
    constexpr bool EARLY = EPI;
    f32x4 pw[(EARLY && PRO) ? KST : 1][2], rcv[EARLY ? KST : 1], rsv[EARLY ? KST : 1];
    auto early = [&]() __attribute__((always_inline)) {
        if constexpr (EARLY) {
            const long row = cur.row;
            const float* standin = a.g;   // (always there, readable well past any offset used below)
            const float* pwb = (PRO && a.pro_wq) ? a.pro_wq + h * D : standin;
            const float* rcb = a.rcos ? a.rcos + row * a.ldr : standin;
            const float* rsb = a.rcos ? a.rsin + row * a.ldr : standin;
#pragma unroll
            for (int ks = 0; ks < KST; ++ks) {
                const int c = ks * 32 + kg * 8 < D ? ks * 32 + kg * 8 : 0;
                if constexpr (PRO) {
                    pw[ks][0] = gld<f32x4>(pwb + c);
                    pw[ks][1] = gld<f32x4>(pwb + c + 4);
                }
                rcv[ks] = gld<f32x4>(rcb + c / 2);
                rsv[ks] = gld<f32x4>(rsb + c / 2);
            }
        }
    };
    // the products, epilogue and stores of one tile of the block in hand, from `cur`; `live`: the tile exists (every lane runs this: shuffles)
    auto tile = [&](int tt, bool live) __attribute__((always_inline)) {
        const int s = live ? tt * 16 + nl : S, sv = min(s, S - 1);
        const long row = cur.row;
        bf16x8 qh[KST], ql[KST];
#pragma unroll
        for (int ks = 0; ks < KST; ++ks) {
            f32x4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = x0;
            if constexpr (EARLY) {   // (no branch: selects)
                const bool in = ks * 32 + kg * 8 < D;
                x0 = raw4_to_f32(T{}, cur.x[ks][0]);
                x1 = raw4_to_f32(T{}, cur.x[ks][1]);
                if constexpr (PRO) {   // relu(q rstd[token] w[channel]) + eps: the values k_qk_prologue used to materialise
                    const float rq = a.pro_rq ? cur.rq : 1.f;
                    x0 *= rq;
                    x1 *= rq;
                    const f32x4 one = {1.f, 1.f, 1.f, 1.f};
                    x0 *= a.pro_wq ? pw[ks][0] : one;
                    x1 *= a.pro_wq ? pw[ks][1] : one;
                }
                if (a.relu) relu8(x0, x1, a.eps);
                if (a.rcos) rope8(x0, x1, rcv[ks], rsv[ks]);   // (uniform; no memory operation inside)
                const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
                x0 = in ? x0 : z4;
                x1 = in ? x1 : z4;
            } else if (ks * 32 + kg * 8 < D) {
                x0 = raw4_to_f32(T{}, cur.x[ks][0]);
                x1 = raw4_to_f32(T{}, cur.x[ks][1]);
                if constexpr (PRO) {   // relu(q rstd[token] w[channel]) + eps: the values k_qk_prologue used to materialise
                    const float rq = a.pro_rq ? cur.rq : 1.f;
                    x0 *= rq;
                    x1 *= rq;
                    if (a.pro_wq) {
                        x0 *= *reinterpret_cast<const f32x4*>(a.pro_wq + h * D + ks * 32 + kg * 8);
                        x1 *= *reinterpret_cast<const f32x4*>(a.pro_wq + h * D + ks * 32 + kg * 8 + 4);
                    }
                }
                if (a.relu) relu8(x0, x1, a.eps);
                if (a.rcos) {
                    const long ro = row * a.ldr + ks * 16 + kg * 4;
                    rope8(x0, x1, *reinterpret_cast<const f32x4*>(a.rcos + ro), *reinterpret_cast<const f32x4*>(a.rsin + ro));
                }
            }
            uint4 hi, lo;
            split8(x0, x1, hi, lo);
            qh[ks] = as_bf16x8(hi);
            ql[ks] = as_bf16x8(lo);
        }
        (void)sv;
        const float ninv = a.normalize ? cur.ninv : 1.f;
        TO* orow = ob + row * a.o.sn + kg * 4;
        f32x4 res[EPI ? DT + 1 : 1];
        // gate values of this lane's features, fetched (packed) before the products: latency off the epilogue.
        // 16-bit activations with 16-byte aligned rows (WIDE): the epilogue runs in a STORE layout -- lane pairs (kg, kg ^ 1)
        // swap halves of two neighbouring feature tiles, so that a lane owns 8 consecutive features (one 16-byte piece) of the
        // token and the four lanes of a token cover 64 contiguous bytes per instruction; gate pieces are read the same way.
        // (In the product layout a lane owns 4 features: 8-byte pieces, 32 bytes per token and instruction -- the gate read of
        // 97 MB cost 70 us and every output line was written by four instructions.)
        constexpr bool WIDE_T = EPI && sizeof(TO) == 2;
        constexpr int NPAIR = DT / 2;
        bool wide = false;
        if constexpr (WIDE_T)
            wide = (((reinterpret_cast<uintptr_t>(a.o.ptr) | reinterpret_cast<uintptr_t>(a.gate.ptr)) & 15) == 0) &&
                   (((a.o.sb | a.o.sn | a.o.sh | (a.gate.ptr ? (a.gate.sb | a.gate.sn | a.gate.sh) : 0)) & 7) == 0);
        const int podd = kg & 1, phalf = (kg >> 1) * 8;   // store layout: tile 2 j + podd, features phalf .. phalf + 7 of it
        bool wide2 = false;   // the plain (no-epilogue) store of 16-bit results in the same layout
        if constexpr (!EPI && sizeof(TO) == 2)
            wide2 = a.skip_out || ((reinterpret_cast<uintptr_t>(a.o.ptr) & 15) == 0 && ((a.o.sb | a.o.sn | a.o.sh) & 7) == 0);
        typename Raw4<TO>::type gv[EPI ? DT : 1];
        uint4 gv8[WIDE_T ? (NPAIR ? NPAIR : 1) : 1];
        f32x4 nwv[WIDE_T ? (NPAIR ? NPAIR : 1) : 1][2];   // the norm weights of the lane's pieces (wide layout), requested with the gate
        if constexpr (WIDE_T) {
            if (wide) {   // (uniform; every load inside is unconditional)
                const TO* gtok = a.gate.ptr ? (const TO*)a.gate.ptr + b * a.gate.sb + row * a.gate.sn + h * a.gate.sh : reinterpret_cast<const TO*>(a.g);
                const float* nwb = a.nw ? a.nw : a.g;
#pragma unroll
                for (int j = 0; j < NPAIR; ++j) {
                    const int f0 = (2 * j + podd) * 16 + phalf, fc = f0 < D ? f0 : 0;
                    gv8[j] = gld<uint4>(gtok + fc);
                    nwv[j][0] = gld<f32x4>(nwb + fc);
                    nwv[j][1] = gld<f32x4>(nwb + fc + 4);
                }
            }
        }
        if constexpr (EPI) {
            if (a.gate.ptr) {
                const TO* gtok = (const TO*)a.gate.ptr + b * a.gate.sb + row * a.gate.sn + h * a.gate.sh;
                if (WIDE_T && wide) {
                    if (DT & 1) {
                        if ((DT - 1) * 16 + kg * 4 < D) gv[DT - 1] = *reinterpret_cast<const typename Raw4<TO>::type*>(gtok + kg * 4 + (DT - 1) * 16);
                    }
                } else {
#pragma unroll
                    for (int ct = 0; ct < DT; ++ct)
                        if (ct * 16 + kg * 4 < D) gv[ct] = *reinterpret_cast<const typename Raw4<TO>::type*>(gtok + kg * 4 + ct * 16);
                }
            }
        }
#pragma unroll
        for (int ct = 0; ct < DT; ct += 2) {
            f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0;
#pragma unroll
            for (int ks = 0; ks < KST; ++ks) {
                const bf16x8 a0h = mat_tr_read8<mat_new<DT>()>(Gh, LD, ks * 32, ct * 16, lane), a1h = mat_tr_read8<mat_new<DT>()>(Gh, LD, ks * 32, ct * 16 + 16, lane);
                c0 = mfma_bf16(a0h, qh[ks], c0);
                c1 = mfma_bf16(a1h, qh[ks], c1);
                if (sf_has_lo(FMT)) {
                    const bf16x8 a0l = mat_tr_read8<mat_new<DT>()>(Gl, LD, ks * 32, ct * 16, lane), a1l = mat_tr_read8<mat_new<DT>()>(Gl, LD, ks * 32, ct * 16 + 16, lane);
                    c0 = mfma_bf16(a0l, qh[ks], c0);
                    c1 = mfma_bf16(a1l, qh[ks], c1);
                }
                if (LO) {
                    c0 = mfma_bf16(a0h, ql[ks], c0);
                    c1 = mfma_bf16(a1h, ql[ks], c1);
                }
            }
            if constexpr (EPI) {
                res[ct] = c0 * ninv;
                res[ct + 1] = c1 * ninv;
            } else {
                const f32x4 o0 = c0 * ninv, o1 = c1 * ninv;
                bool stored = false;
                if constexpr (sizeof(TO) == 2) {
                    if (wide2 && ct + 1 < DT) {   // (uniform) the store layout of the fused epilogue: 16-byte pieces, 64 contiguous bytes per token and instruction
                        const f32x4 send = podd ? o0 : o1, keep = podd ? o1 : o0;
                        f32x4 recv;
#pragma unroll
                        for (int i = 0; i < 4; ++i) recv[i] = __shfl_xor(send[i], 16, 64);   // (every lane takes part)
                        const f32x4 lo4 = podd ? recv : keep, hi4 = podd ? keep : recv;
                        const int f0 = (ct + podd) * 16 + phalf;
                        if (s < S && f0 < D) {
                            if (!a.skip_out) gst<uint4>(ob + row * a.o.sn + f0, pack8_16(TO{}, lo4, hi4));
                            if (a.olo) {   // what the 16-bit store loses, for the backward's row dots (OutArgs::olo)
                                const uint2 r0 = store_residual4<TO>(lo4), r1 = store_residual4<TO>(hi4);
                                gst<uint4>(a.olo + ((long)bh * a.M * S + p0 + s) * D + f0, make_uint4(r0.x, r0.y, r1.x, r1.y));
                            }
                        }
                        stored = true;
                    }
                }
                if (!stored && s < S) {
                    if (!a.skip_out) {
                        if (ct * 16 + kg * 4 < D) Io<TO>::st4(orow + ct * 16, o0);
                        if (ct * 16 + 16 + kg * 4 < D) Io<TO>::st4(orow + ct * 16 + 16, o1);
                    }
                    if constexpr (sizeof(TO) == 2) {
                        if (a.olo) {
                            u16* lo = a.olo + ((long)bh * a.M * S + p0 + s) * D + kg * 4;
                            if (ct * 16 + kg * 4 < D) *reinterpret_cast<uint2*>(lo + ct * 16) = store_residual4<TO>(o0);
                            if (ct * 16 + 16 + kg * 4 < D) *reinterpret_cast<uint2*>(lo + ct * 16 + 16) = store_residual4<TO>(o1);
                        }
                    }
                }
            }
        }
        if constexpr (EPI) {
            float ss = 0.f;
#pragma unroll
            for (int ct = 0; ct < DT; ++ct) {
                if (!std::is_same<TO, float>::value)   // out.to(dtype) before the norm
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        res[ct][i] = std::is_same<TO, bf16_t>::value ? bf16_to_f32(cvt_bf16(res[ct][i])) : (float)(_Float16)res[ct][i];
                if (ct * 16 + kg * 4 < D) ss += res[ct][0] * res[ct][0] + res[ct][1] * res[ct][1] + res[ct][2] * res[ct][2] + res[ct][3] * res[ct][3];
            }
            ss += __shfl_xor(ss, 16, 64);   // the token's features live in the 4 lanes kg = 0..3
            ss += __shfl_xor(ss, 32, 64);
            const float rstd = 1.f / sqrtf(ss / (float)D + a.neps);
            int ct_first = 0;   // tiles below it were stored in the wide layout
            if constexpr (WIDE_T) {
                if (wide) {
                    TO* otok = ob + row * a.o.sn;
#pragma unroll
                    for (int j = 0; j < NPAIR; ++j) {
                        const f32x4 send = podd ? res[2 * j] : res[2 * j + 1], keep = podd ? res[2 * j + 1] : res[2 * j];
                        f32x4 recv;
#pragma unroll
                        for (int i = 0; i < 4; ++i) recv[i] = __shfl_xor(send[i], 16, 64);   // (every lane takes part)
                        const f32x4 lo4 = podd ? recv : keep, hi4 = podd ? keep : recv;
                        const int f0 = (2 * j + podd) * 16 + phalf;
                        if (s < S && f0 < D) {
                            f32x4 y0 = lo4 * rstd, y1 = hi4 * rstd;
                            if (a.nw) {   // (uniform; the values were requested before the products)
                                y0 *= nwv[j][0];
                                y1 *= nwv[j][1];
                            }
                            if (a.gate.ptr) {
                                const f32x4 g0 = raw4_to_f32(TO{}, make_uint2(gv8[j].x, gv8[j].y)), g1 = raw4_to_f32(TO{}, make_uint2(gv8[j].z, gv8[j].w));
#pragma unroll
                                for (int i = 0; i < 4; ++i) {
                                    y0[i] *= g0[i] / (1.f + __expf(-g0[i]));
                                    y1[i] *= g1[i] / (1.f + __expf(-g1[i]));
                                }
                            }
                            gst<uint4>(otok + f0, pack8_16(TO{}, y0, y1));
                        }
                    }
                    ct_first = 2 * NPAIR;
                }
            }
            if (s < S) {
#pragma unroll
                for (int ct = 0; ct < DT; ++ct) {
                    if (ct < ct_first) continue;
                    const int d0 = ct * 16 + kg * 4;
                    if (d0 < D) {
                        f32x4 y = res[ct] * rstd;
                        if (a.nw) y *= *reinterpret_cast<const f32x4*>(a.nw + d0);
                        if (a.gate.ptr) {
                            const f32x4 gf = raw4_to_f32(TO{}, gv[ct]);
#pragma unroll
                            for (int i = 0; i < 4; ++i) y[i] *= gf[i] / (1.f + __expf(-gf[i]));
                        }
                        Io<TO>::st4(orow + ct * 16, y);
                    }
                }
            }
        }
    };
    if constexpr (!FLAT) {
        constexpr int NWV = SP_OUT_T / 64;
        int lk = 0;
        if (a.idx) lk = gld<int>(a.idx + p0 + min(wave * 16 + nl, S - 1));   // (uniform branch; nothing is in flight yet)
        fetch(wave, cur, lk);
        if constexpr (!ONE) lk = look(wave + NWV);   // (for the next fetch)
        // (SF_BF16: no lo tile)
        stage_mat_split<DT, FMT, SP_OUT_T>(Gh, Gl, a.g, ((long)bh * a.M + blk) * a.es, D, tid);
        __syncthreads();
        if constexpr (ONE) {
            if (wave * 16 < S) {   // (uniform)
                early();
                tile(wave, true);
            }
            return;
        }
        for (int tt = wave; tt * 16 < S; tt += NWV) {
            if constexpr (DBL) {
                early();
                fetch(tt + NWV, nxt, lk);
                lk = look(tt + 2 * NWV);
            } else {
                if (tt != wave) {   // (uniform)
                    fetch(tt, cur, lk);
                    lk = look(tt + NWV);
                }
                early();
            }
            tile(tt, true);
            if constexpr (DBL) cur = nxt;
        }
    } else {
        constexpr int NWV = SP_OUT_T / 64;
        u16* const G0 = Gh;
        const long total = (long)a.nbh * a.M * TPI;
        const int g0 = (int)(total * blockIdx.x / gridDim.x), g1 = (int)(total * (blockIdx.x + 1) / gridDim.x);
        if (g1 <= g0) return;
        const int nrounds = (g1 - g0 + NWV - 1) / NWV;
        MatStage<DT, SP_OUT_T> stg;
        int staged = g0 / TPI;   // the last block whose summary is in LDS (or on its way)
        int lk = 0;
        if (a.idx) lk = look(min(g0 + wave, g1 - 1));   // (uniform branch; nothing is in flight yet)
        fetch(min(g0 + wave, g1 - 1), cur, lk);
        lk = look(min(g0 + wave + NWV, g1 - 1));   // (for the next fetch)
        {   // the first round's blocks: one, or -- when it already ends in the next block -- two, requested together (one round trip)
            const bool two = min(g0 + NWV - 1, g1 - 1) / TPI > staged;   // (uniform)
            MatStage<DT, SP_OUT_T> stg2;
            stage_mat_issue<DT, SP_OUT_T>(stg, a.g, (long)staged * a.es, D, tid);
            stage_mat_issue<DT, SP_OUT_T>(stg2, a.g, (long)(staged + (two ? 1 : 0)) * a.es, D, tid);
            stage_mat_commit<DT, SP_OUT_T>(G0 + (staged & 1) * 2 * TILE, G0 + (staged & 1) * 2 * TILE + TILE, stg, D, tid);
            if (two) {
                ++staged;
                stage_mat_commit<DT, SP_OUT_T>(G0 + (staged & 1) * 2 * TILE, G0 + (staged & 1) * 2 * TILE + TILE, stg2, D, tid);
            }
        }
        __syncthreads();
        for (int r = 0; r < nrounds; ++r) {
            const int g = g0 + r * NWV + wave, gc = min(g, g1 - 1), item = gc / TPI;
            // the block a later round needs first: requested now, committed behind this round's products (uniform)
            const bool ahead = r + 1 < nrounds && min(g0 + (r + 1) * NWV + NWV - 1, g1 - 1) / TPI > staged;
            bh = item / a.M; blk = item - bh * a.M; b = bh / a.H; h = bh - b * a.H;
            p0 = (long)blk * S;
            qb = (const T*)a.q.ptr + b * a.q.sb + h * a.q.sh;
            ob = (TO*)a.o.ptr + b * a.o.sb + h * a.o.sh;
            Gh = G0 + (item & 1) * 2 * TILE;
            Gl = Gh + TILE;
            early();   // this tile's channel weights and rope angles first, then what is needed later
            fetch(min(g + NWV, g1 - 1), nxt, lk);
            lk = look(min(g + 2 * NWV, g1 - 1));
            stage_mat_issue<DT, SP_OUT_T>(stg, a.g, (long)(staged + (ahead ? 1 : 0)) * a.es, D, tid, ahead);   // (no branch around the loads)
            tile(gc - item * TPI, g < g1);
            cur = nxt;
            if (ahead) {   // (the buffer it goes to held the block before the previous one: this round may still have read it)
                __syncthreads();
                ++staged;
                stage_mat_commit<DT, SP_OUT_T>(G0 + (staged & 1) * 2 * TILE, G0 + (staged & 1) * 2 * TILE + TILE, stg, D, tid);
                __syncthreads();
            }
        }
    }
}

}  // namespace sp
}  // namespace mhla
