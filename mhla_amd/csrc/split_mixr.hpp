// Block-mix split kernels (split.hpp): k_sp_mixr and k_sp_mixr_dma, the resident-sequence mixing, and the weight staging every
// resident mixing kernel uses (mixh.hpp and mixh2.hpp too).
#pragma once
#include "split_operands.hpp"

namespace mhla {
namespace sp {

// -------------------------------------------------------------------------------------------------
// k_sp_mixr<NW, TRANS, FMT>: the same mixing with EVERY block of the (b,h) resident in the workgroup (M <= 16 NW <= 256), the
// causal path's k_csf_mixf for a full matrix.  A workgroup owns slices of 256-byte row pieces (TE = 64 fp32 or 128 bf16 elements):
// the slice's rows of all blocks sit in LDS (fp32 summaries as bf16 hi + lo tiles), so every summary byte is read from HBM once
// (k_sp_mix re-reads a slice per 64-row output tile: 1.5x at M = 150, 4x at M = 256) and the mixing weights of a wave's 16 output
// blocks live in its registers as bf16 hi + lo for the whole launch (k_sp_mix rebuilt them per step and was bound by its LDS
// operand reads: 3.1 TB/s at the Wan shape, 2.3 TB/s at M = 256).  One wave per 16 output blocks; the summaries enter the MFMA
// through the transpose read as the A operand, so a lane ends up with four consecutive elements of one output block (16-byte /
// 8-byte staging writes, full 256-byte rows out); a workgroup walks `spw` consecutive slices with the next slice's rows in
// flight in registers.  grid: wgs <= 256 persistent workgroups of 64 NW threads.
//   TRANS 0: out[i][e] = sum_j W[i][j] in[j][e]      TRANS 1: out[j][e] = sum_i W[i][j] in[i][e]
// -------------------------------------------------------------------------------------------------
// Mixing weights of a wave's NB tiles of 16 output blocks as MFMA B operands, bf16 hi + lo:
//   B[k = r][n = o] = Wm(o, r), o = obase + 16 n + (lane & 15), r = 32 ks + 8 (lane >> 4) + t   (Wm = W, or W^T with TRANS)
// Every workgroup needs the whole matrix: it is fetched in chunks of 64 input blocks with coalesced 16-byte loads into LDS (`Tf`,
// any region of ROWS x 68 / 64 x (ROWS + 4) floats that is free before the first slice) and picked from there.  Per-lane dword
// loads straight from global memory touched 16 lines per instruction for 16 bytes of each and re-fetched them for every t: 35 us
// of a 190 us launch at M = 256.  Blocks past M get zero weights.  Ends with a barrier (Tf may be reused).
template <int TRANS, int NTH, int ROWS, int NK, int NB>
__device__ __forceinline__ void mixr_weights(bf16x8 (&wh)[NK][NB], bf16x8 (&wl)[NK][NB], float* __restrict__ Tf, const float* __restrict__ W,
                                             int ldw, int M, int obase, int tid) {
    constexpr int TR = TRANS ? 64 : ROWS, TC = TRANS ? ROWS : 64, LDT = TC + 4, PPRW = TC / 4, NCH = (NK + 1) / 2;
    const int lane = tid & 63, nl = lane & 15, kg = lane >> 4;
    const bool vec = ((reinterpret_cast<uintptr_t>(W) & 15) == 0) && (ldw & 3) == 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        __syncthreads();
        for (int v = tid; v < TR * PPRW; v += NTH) {
            const int row = v / PPRW, c4 = (v - row * PPRW) * 4;
            const int gr = TRANS ? c * 64 + row : row, gc = TRANS ? c4 : c * 64 + c4;   // row / first column in W
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (gr < M) {
                const float* src = W + (long)gr * ldw + gc;
                if (vec && gc + 4 <= M) {
                    x = gld<f32x4>(src);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (gc + i < M) x[i] = gld<float>(src + i);
                }
            }
            *reinterpret_cast<f32x4*>(Tf + row * LDT + c4) = x;
        }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            const int o = obase + n * 16 + nl;
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) {
                if (2 * c + k2 < NK) {
                    float w[8];
                    if (TRANS) {
#pragma unroll
                        for (int t = 0; t < 8; ++t) w[t] = Tf[(k2 * 32 + kg * 8 + t) * LDT + o];
                    } else {
                        const f32x4 lo4 = *reinterpret_cast<const f32x4*>(Tf + o * LDT + k2 * 32 + kg * 8);
                        const f32x4 hi4 = *reinterpret_cast<const f32x4*>(Tf + o * LDT + k2 * 32 + kg * 8 + 4);
#pragma unroll
                        for (int t = 0; t < 4; ++t) { w[t] = lo4[t]; w[4 + t] = hi4[t]; }
                    }
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        const __bf16 h = (__bf16)w[t];
                        wh[2 * c + k2][n][t] = h;
                        wl[2 * c + k2][n][t] = (__bf16)(w[t] - (float)h);
                    }
                }
            }
        }
    }
    __syncthreads();
}
// The same staging for the h16 mixing kernels (k_sp_mixh, mixh.hpp; k_sp_mixh2, mixh2.hpp), one reduction step at a time: f(ks, w) is
// called with the lane's eight fp32 weights of step ks -- w[t] = weight of input block r = 32 ks + 8 kg + t in output block
// o0 + obase + nl (TRANS: W[r][o], else W[o][r]); blocks past M: 0 -- while the chunk that holds them is staged: a caller that consumes
// them at once has 8 temporaries, not 8 NK.  ROWS output blocks from o0 are staged (o0 = 0 and ROWS >= M: the whole matrix), NK steps
// of input blocks.  Ends with a barrier.
// k_sp_mixr and k_sp_mixr_dma stay on mixr_weights above: through this function (with a loop over NB tiles, and the bf16 hi + lo
// conversion as f) their TRANS = 1 forms of eight and more waves come out of hipcc 7.2 with other code -- one v_mad_u32_u24 and one
// s_movk_i32 fewer and the address registers around the staging loop renumbered, in k_sp_mixr<8, 1, p24> down into the slice loop --
// whether f is a capturing or captureless lambda, always_inline or not, taken by value or by reference (profiles/split_headers.md).
template <int TRANS, int NTH, int ROWS, int NK, typename F>
__device__ __forceinline__ void mix_weights_each(float* __restrict__ Tf, const float* __restrict__ W, int ldw, int M, int o0, int obase, int tid, F f) {
    constexpr int TR = TRANS ? 64 : ROWS, TC = TRANS ? ROWS : 64, LDT = TC + 4, PPRW = TC / 4, NCH = (NK + 1) / 2;
    const int lane = tid & 63, nl = lane & 15, kg = lane >> 4;
    const bool vec = ((reinterpret_cast<uintptr_t>(W) & 15) == 0) && (ldw & 3) == 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        __syncthreads();
        for (int v = tid; v < TR * PPRW; v += NTH) {
            const int row = v / PPRW, c4 = (v - row * PPRW) * 4;
            const int gr = TRANS ? c * 64 + row : o0 + row, gc = TRANS ? o0 + c4 : c * 64 + c4;   // (output blocks o0 .. o0 + ROWS - 1 of the matrix)
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (gr < M) {
                const float* src = W + (long)gr * ldw + gc;
                if (vec && gc + 4 <= M) {
                    x = gld<f32x4>(src);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (gc + i < M) x[i] = gld<float>(src + i);
                }
            }
            *reinterpret_cast<f32x4*>(Tf + row * LDT + c4) = x;
        }
        __syncthreads();
        const int o = obase + nl;
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
            if (2 * c + k2 < NK) {
                float w[8];
                if (TRANS) {
#pragma unroll
                    for (int t = 0; t < 8; ++t) w[t] = Tf[(k2 * 32 + kg * 8 + t) * LDT + o];
                } else {
                    const f32x4 lo4 = *reinterpret_cast<const f32x4*>(Tf + o * LDT + k2 * 32 + kg * 8);
                    const f32x4 hi4 = *reinterpret_cast<const f32x4*>(Tf + o * LDT + k2 * 32 + kg * 8 + 4);
#pragma unroll
                    for (int t = 0; t < 4; ++t) { w[t] = lo4[t]; w[4 + t] = hi4[t]; }
                }
                f(2 * c + k2, w);
            }
        }
    }
    __syncthreads();
}

struct MixrArgs {
    const float* W;
    int ldw;
    const void* in;
    void* out;
    int M;
    long E;        // elements per block summary (multiple of the slice width)
    long es;       // row stride of `in` / `out` in elements (E + padding)
    long total;    // slices = bh * E / TE
    int spw;       // slices per workgroup
    // k_sp_mixr_dma only: the normaliser's product with the same weights, out = f(sum_r Wm(o, r) zin[bh][r][s]) for S <= 16 fp32
    // values per block (k_wz<0>: f = 1 / (eps + .), Wm = W with TRANS 0; k_wz<1>: f = identity, Wm = W^T with TRANS 1); null: none
    const float* zin;
    float* zout;
    int S;
    float eps;
    unsigned long long* trace;   // debugging aid (mhla_debug_set_trace): s_memtime stamps of the first workgroups' slice loop, or null
    // k_sp_mixr<.., DW> (backward, fp32 summaries): the OTHER summary set of the dW product (KV, laid out like `in` = dG) and the
    // per-workgroup partials dwp[workgroup][M][M] of dW[i][j] = sum_bh sum_e dG[i][e] KV[j][e] -- formed from the slice rows this
    // kernel stages anyway, so that dG is read from HBM once for dKV and dW together
    const void* in2;
    float* dwp;
    // k_sp_mixr, fp32 summaries: the normaliser's product rides along as EXTRA SLICES after the summaries' -- block r's S values zin[bh][r][:]
    // are one more row set mixed with the same weights (slices of TE values, ztotal = bh * ceil(S / TE) of them, dealt round-robin over the workgroups; S even), stored
    // through f into zout.  DW: zin = dn, zin2 = z, and the <dn_i, z_j> term of dW falls out of the same products (k_dw is not launched).
    long ztotal;
    const float* zin2;
};
// slice width: 256-byte row pieces; 128-byte ones for 16 waves (1024 threads on 128 VGPRs: half the accumulators and staging registers)
template <int NW, int FMT> __host__ __device__ constexpr int mixr_te() { return (FMT == SF_BF16 ? 128 : 64) / (NW > 12 ? 2 : 1); }
template <int NW, int FMT, bool DW = false>
__host__ __device__ constexpr int sp_mixr_smem() {
    constexpr int TE = mixr_te<NW, FMT>(), ROWS = 16 * NW;
    return (FMT == SF_BF16 ? 1 : (DW ? 4 : 2)) * ROWS * (TE + 8) * 2 + (FMT == SF_BF16 ? ROWS * (TE + 8) * 2 : ROWS * (TE + 4) * 4);
}

// DW (TRANS 1, fp32 summaries, M <= 128): the kernel also stages the KV rows of every slice (hi + lo, two more tiles) and accumulates
// dW[i][j] += sum_{e in slice} dG[i][e] KV[j][e] over ALL its slices -- every (b,h) it meets: dW is their sum anyway -- in
// registers (wave w owns rows i = 16 w .. 16 w + 15, all columns: NW tiles); one [M][M] partial per workgroup at the end, summed in a
// fixed order by k_dw_reduce.  Replaces k_sp_dw, which read dG and KV a second time (C2 at the default arithmetic: 81 us).
// p24: the summaries (in, in2, out) are stored as 24-bit floats in two planes per row (p24_pack8).  A thread's unit is then 8 elements
// of a row -- one 16-byte piece of the hi plane and one 8-byte piece of the lo plane -- instead of a 16-byte piece of 4 floats.
// (h16 summaries are mixed by k_sp_mixh, mixh.hpp: on the payload, with the fp16 MFMA.  A decode-at-the-commit variant of THIS kernel was
// built first in round 6 and was no faster than p24: 2-byte rows in 64-element slices put fewer bytes in flight per workgroup.)
template <int NW, int TRANS, int FMT, bool DW = false>   // FMT: fp32 words, p24 or bf16
__global__ __launch_bounds__(64 * NW, (NW == 8 && !DW && FMT == SF_P24) ? 4 : (NW + 3) / 4) void k_sp_mixr(const MixrArgs a) {   // (eight waves on 24-bit summaries without dW: 128 VGPRs, two workgroups per CU instead of one at 136)
    static_assert(!DW || (TRANS == 1 && sf_has_lo(FMT) && NW <= 8), "dW rides in the backward's fp32 mixing kernel, M <= 128 (twelve waves: 77 spilled registers)");
    static_assert(FMT != SF_H16 && (FMT != SF_P24 || NW <= 12), "h16 is mixed by k_sp_mixh; p24: up to twelve waves");
    constexpr int TE = mixr_te<NW, FMT>(), ROWS = 16 * NW, LD = TE + 8, LDO = TE + 4, NK = (NW + 1) / 2, NT = TE / 16;
    constexpr int PPR = TE * (FMT == SF_BF16 ? 2 : 4) / 16;          // 16-byte pieces per row of the slice (16, or 8 with 16 waves)
    constexpr int NTH = 64 * NW, NP = FMT == SF_P24 ? ROWS * 8 / NTH : ROWS * PPR / NTH;   // pieces (p24: units of 8 elements) per thread and slice
    constexpr int UPR = FMT == SF_P24 ? 8 : PPR;                    // ... per row
    static_assert(NP * NTH == ROWS * UPR, "pieces must tile the slice");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u16* Th = reinterpret_cast<u16*>(smem_raw);
    u16* Tl = Th + ROWS * LD;                                        // (fp32 summaries only)
    u16* Kh = Tl + ROWS * LD;                                        // (DW only: the KV rows of the slice)
    u16* Kl = Kh + ROWS * LD;
    unsigned char* Os = smem_raw + (FMT == SF_BF16 ? 1 : (DW ? 4 : 2)) * ROWS * LD * 2;     // bf16 [ROWS][LD] or fp32 [ROWS][LDO]
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nl = lane & 15, kg = lane >> 4;
    const int M = a.M;
    const long nsl = a.E / TE;
    const long s0 = (long)blockIdx.x * a.spw;
    const int cnt_s = (int)max(0L, min((long)a.spw, a.total - s0));   // this workgroup's summary slices: a consecutive range
    const int nzs = (a.S + TE - 1) / TE;                              // normaliser slices per (b, h): dealt round-robin, see the loops
    if (cnt_s <= 0 && (FMT == SF_BF16 || (long)blockIdx.x >= a.ztotal)) return;
    // B operand: B[k = r][n = o] = weight of input block r in output block o = 16 wave + nl, r = 32 ks + 8 kg + t
    bf16x8 wh[NK][1], wl[NK][1];
    static_assert((TRANS ? 64 * (ROWS + 4) : ROWS * 68) * 4 <= sp_mixr_smem<NW, FMT, DW>(), "weight chunk must fit in the tiles");
    mixr_weights<TRANS, 64 * NW, ROWS, NK, 1>(wh, wl, reinterpret_cast<float*>(smem_raw), a.W, a.ldw, M, wave * 16, tid);
    constexpr int ESZ = FMT == SF_BF16 ? 2 : 4;
    constexpr int SLB = FMT == SF_P24 ? 128 : TE * ESZ;             // bytes of a slice in a summary row (p24: of its hi plane)
    // p24: the lo piece of a unit relative to its hi piece (goff + 16 c of slice es): lo plane at 2 E, slice at 64 es, piece at 8 c
    auto lo_rel = [&](int es, int c) { return (long)2 * a.E - 64 * es - 8 * c; };
    // byte offset of slice (bh, es); a workgroup's slices are consecutive, so the pair is advanced rather than divided out per
    // slice (the 64-bit division was 150 instructions with branches between the barrier and the next slice's loads)
    auto slice_off = [&](int bh, int es) { return (long)bh * M * a.es * ESZ + (long)es * SLB; };
    auto zslice_off = [&](int bh, int es) { return ((long)bh * M * a.S + (long)es * TE) * 4; };   // (normaliser rows: S plain floats)
    auto advance = [&](int& bh, int& es) { if (++es == (int)nsl) { es = 0; ++bh; } };
    // the thread's pieces: piece v = tid + p NTH -> row v / PPR, 16 bytes at column piece v % PPR (rows past M: the last row, zeroed)
    unsigned goff[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int v = tid + p * NTH, row = v / UPR, c = v % UPR;
        goff[p] = (unsigned)((long)(row < M ? row : M - 1) * a.es * ESZ + c * 16);   // (p24: the unit's hi piece; its lo piece: lo_rel)
    }
    // staging registers.  p24: pre = hi piece, prl = lo piece; a normaliser slice (plain floats) takes the unit's 8 floats in pre + prz
    struct Stage {
        uint4 pre[NP], pre2[DW ? NP : 1], prz[FMT == SF_P24 ? NP : 1], prz2[(FMT == SF_P24 && DW) ? NP : 1];
        u32x2_t prl[FMT == SF_P24 ? NP : 1], prl2[(FMT == SF_P24 && DW) ? NP : 1];   // (native vectors: an array of uint2 in here stays in scratch)
    };
    // (A second slice in flight per workgroup -- two Stage objects, the loop unrolled by two -- gained nothing: hipcc's wait in front of
    // the commit is vmcnt(0), i.e. for both.  Nor did starting the workgroups of a CU a fraction of an iteration apart, or fetching and
    // storing the lo pieces of an even / odd slice pair together, whole 128-byte lines at a time.)
    Stage sga;
    // a normaliser slice: rows of S floats, pieces past the row's end are not touched (zeros)
    constexpr int ZPB = FMT == SF_P24 ? 32 : 16, ZPF = ZPB / 4;   // bytes / floats of a thread's piece of a normaliser row
    auto zoff = [&](int p) { const int v = tid + p * NTH, row = v / UPR, c = v % UPR; return (unsigned)((row < M ? row : M - 1) * a.S * 4 + c * ZPB); };
    auto zlive = [&](int p, int es, int half = 0) { return ((tid + p * NTH) % UPR) * ZPF + half * 4 + es * TE < a.S; };
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
    // four floats of a normaliser row (piece `half` of unit p): one 16-byte load when rows are multiples of 4 floats, two 8-byte loads
    // when they are only even (S = 210: rows start on 8-byte boundaries), each half on its own side of the row's end
    // Unconditional, from clamped addresses -- a load behind a lane-dependent branch makes hipcc wait for everything in flight where the
    // branch joins (eight serial round trips per normaliser slice, and those workgroups were the kernel's tail); floats past the row's end
    // are zeroed at the commit (zmask).
    const bool zwide = (a.S & 3) == 0;   // (uniform)
    auto zf0 = [&](int p, int es, int half) { return ((tid + p * NTH) % UPR) * ZPF + half * 4 + es * TE; };
    auto zld = [&](const char* base, int p, int es, int half) __attribute__((always_inline)) {
        const int f0 = zf0(p, es, half);
        const char* src = base + zoff(p) + half * 16;
        if (zwide) return gld_stream16(f0 < a.S ? src : base);
        const uint2 lo = gld<uint2>(f0 < a.S ? src : base), hi = gld<uint2>(f0 + 2 < a.S ? src + 8 : base);
        return make_uint4(lo.x, lo.y, hi.x, hi.y);
    };
    auto zmask = [&](const uint4& x, bool ok, int p, int es, int half) {
        const int f0 = zf0(p, es, half);
        return make_uint4((ok && f0 < a.S) ? x.x : 0u, (ok && f0 + 1 < a.S) ? x.y : 0u, (ok && f0 + 2 < a.S) ? x.z : 0u, (ok && f0 + 3 < a.S) ? x.w : 0u);
    };
    // ZS: a normaliser slice.  A compile-time flag, and the summary slices and the normaliser slices of a workgroup are two loops:
    // with both kinds of loads behind one runtime branch, writing the same staging registers, hipcc waited for ALL loads right after
    // issuing them (`L L L L W0 M M`: k_sp_mixr<1,dw> 78 -> 121 us at C2).
    auto issue = [&]<bool ZS>(std::bool_constant<ZS>, Stage& g, int bh, int es) __attribute__((always_inline)) {
        const long boff = ZS ? zslice_off(bh, es) : slice_off(bh, es);
        if constexpr (ZS) {
            const char* base = reinterpret_cast<const char*>(a.zin) + boff;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                g.pre[p] = zld(base, p, es, 0);
                if constexpr (FMT == SF_P24) g.prz[p] = zld(base, p, es, 1);
            }
            if constexpr (DW) {
                const char* base2 = reinterpret_cast<const char*>(a.zin2) + boff;
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    g.pre2[p] = zld(base2, p, es, 0);
                    if constexpr (FMT == SF_P24) g.prz2[p] = zld(base2, p, es, 1);
                }
            }
            return;
        }
        const char* base = reinterpret_cast<const char*>(a.in) + boff;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            g.pre[p] = gld_stream16(base + goff[p]);
            if constexpr (FMT == SF_P24) g.prl[p] = *(const MHLA_GLOBAL_AS u32x2_t*)(base + goff[p] + lo_rel(es, (tid + p * NTH) % UPR));
        }
        if constexpr (DW) {
            const char* base2 = reinterpret_cast<const char*>(a.in2) + boff;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                g.pre2[p] = gld_stream16(base2 + goff[p]);
                if constexpr (FMT == SF_P24) g.prl2[p] = *(const MHLA_GLOBAL_AS u32x2_t*)(base2 + goff[p] + lo_rel(es, (tid + p * NTH) % UPR));
            }
        }
    };
    f32x4 dwacc[DW ? NW : 1];
#pragma unroll
    for (int t = 0; t < (DW ? NW : 1); ++t) dwacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // four floats -> four bf16 hi + four bf16 lo at tile position (row, 4 c)
    auto commit_hl = [&](u16* th, u16* tl, const uint4& x, int row, int c) {
        const float f[4] = {__uint_as_float(x.x), __uint_as_float(x.y), __uint_as_float(x.z), __uint_as_float(x.w)};
        float l[4];
        unsigned short hs[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            hs[i] = cvt_bf16(f[i]);
            l[i] = f[i] - __uint_as_float((unsigned)hs[i] << 16);
        }
        *reinterpret_cast<uint2*>(th + row * LD + c * 4) = make_uint2(hs[0] | ((unsigned)hs[1] << 16), hs[2] | ((unsigned)hs[3] << 16));
        *reinterpret_cast<uint2*>(tl + row * LD + c * 4) = make_uint2(pack_bf16x2(l[0], l[1]), pack_bf16x2(l[2], l[3]));
    };
    // The stores of a slice are issued at the top of the NEXT iteration, after that slice's loads have been committed to LDS: hipcc
    // waits with vmcnt(0) in front of the commit -- with the stores at the end of the iteration that wait included their
    // acknowledgement (loads and stores retire in order), a round trip per slice on top of the load's.  The staging tile keeps the
    // results across the iteration boundary: it is not written again before the barrier that follows the stores.
    long poff = 0;
    bool pz = false;
    int pzes = 0;
    auto store_slice = [&](long off, bool zslice, int zes) __attribute__((always_inline)) {
        if constexpr (sf_has_lo(FMT)) {
            if (zslice) {   // the normaliser's rows: 1 / (eps + .) in the forward, as they are in the backward
                char* zb = reinterpret_cast<char*>(a.zout) + off;
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const int v = tid + p * NTH, row = v / UPR, c = v % UPR;
#pragma unroll
                    for (int hf = 0; hf < ZPF / 4; ++hf) {
                        if (row < M && zlive(p, zes, hf)) {
                            f32x4 x = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(Os) + row * LDO + c * ZPF + hf * 4);
                            if (TRANS == 0)
#pragma unroll
                                for (int i = 0; i < 4; ++i) x[i] = 1.f / (a.eps + x[i]);
                            if (zwide) {
                                *reinterpret_cast<f32x4*>(zb + zoff(p) + hf * 16) = x;
                            } else {   // (even rows: 8-byte pieces, the second one only inside the row)
                                *reinterpret_cast<f32x2*>(zb + zoff(p) + hf * 16) = f32x2{x[0], x[1]};
                                if (((tid + p * NTH) % UPR) * ZPF + hf * 4 + zes * TE + 2 < a.S) *reinterpret_cast<f32x2*>(zb + zoff(p) + hf * 16 + 8) = f32x2{x[2], x[3]};
                            }
                        }
                    }
                }
                return;
            }
        }
        char* ob = reinterpret_cast<char*>(a.out) + off;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int v = tid + p * NTH, row = v / UPR, c = v % UPR;
            if constexpr (FMT == SF_P24) {
                if (row < M) {
                    const float* src = reinterpret_cast<const float*>(Os) + row * LDO + c * 8;
                    uint4 hi;
                    uint2 lo;
                    p24_pack8(*reinterpret_cast<const f32x4*>(src), *reinterpret_cast<const f32x4*>(src + 4), hi, lo);
                    gst<uint4>(ob + goff[p], hi);
                    gst<uint2>(ob + goff[p] + lo_rel(zes, c), lo);
                }
                continue;
            }
            if (row < M) {
                const uint4 x = FMT == SF_BF16 ? *reinterpret_cast<const uint4*>(reinterpret_cast<const u16*>(Os) + row * LD + c * 8)
                                    : *reinterpret_cast<const uint4*>(reinterpret_cast<const float*>(Os) + row * LDO + c * 4);
                gst<uint4>(ob + goff[p], x);
            }
        }
    };
    // it: the slice's position in this phase; first: nothing to store yet; more: another slice of the SAME kind follows (prefetch it)
    auto body = [&]<bool ZS>(std::bool_constant<ZS> zs, Stage& g, bool first, bool more, int bh, int es, int nbh, int nes) __attribute__((always_inline)) {
        const long off = ZS ? zslice_off(bh, es) : slice_off(bh, es);
        constexpr bool zslice = ZS;
        const int zes = es;
#ifdef MIXR_X_NOCOMMIT
        if (first)
#endif
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int v = tid + p * NTH, row = v / UPR, c = v % UPR;
            const bool ok = row < M;   // rows past the last block: zeros (their weights are zero too, but 0 x NaN is not)
            const uint4 x = make_uint4(ok ? g.pre[p].x : 0u, ok ? g.pre[p].y : 0u, ok ? g.pre[p].z : 0u, ok ? g.pre[p].w : 0u);
            if constexpr (FMT == SF_P24) {
                if (zslice) {   // 8 plain floats
                    commit_hl(Th, Tl, zmask(g.pre[p], ok, p, zes, 0), row, 2 * c);
                    commit_hl(Th, Tl, zmask(g.prz[p], ok, p, zes, 1), row, 2 * c + 1);
                    if constexpr (DW) {
                        commit_hl(Kh, Kl, zmask(g.pre2[p], ok, p, zes, 0), row, 2 * c);
                        commit_hl(Kh, Kl, zmask(g.prz2[p], ok, p, zes, 1), row, 2 * c + 1);
                    }
                } else {   // the hi piece is the operand; the lo operand is rebuilt from the third bytes
                    const uint2 l = make_uint2(ok ? g.prl[p][0] : 0u, ok ? g.prl[p][1] : 0u);
                    *reinterpret_cast<uint4*>(Th + row * LD + c * 8) = x;
                    *reinterpret_cast<uint4*>(Tl + row * LD + c * 8) = p24_lo8(x, l);
                    if constexpr (DW) {
                        const uint4 y = make_uint4(ok ? g.pre2[p].x : 0u, ok ? g.pre2[p].y : 0u, ok ? g.pre2[p].z : 0u, ok ? g.pre2[p].w : 0u);
                        const uint2 yl = make_uint2(ok ? g.prl2[p][0] : 0u, ok ? g.prl2[p][1] : 0u);
                        *reinterpret_cast<uint4*>(Kh + row * LD + c * 8) = y;
                        *reinterpret_cast<uint4*>(Kl + row * LD + c * 8) = p24_lo8(y, yl);
                    }
                }
            } else if constexpr (FMT == SF_BF16) {
                *reinterpret_cast<uint4*>(Th + row * LD + c * 8) = x;
            } else if (zslice) {   // (fp32 summaries: the unit is the 16-byte piece)
                commit_hl(Th, Tl, zmask(g.pre[p], ok, p, zes, 0), row, c);
                if constexpr (DW) commit_hl(Kh, Kl, zmask(g.pre2[p], ok, p, zes, 0), row, c);
            } else {   // four floats -> four bf16 hi + four bf16 lo
                commit_hl(Th, Tl, x, row, c);
                if constexpr (DW) {
                    const uint4 y = make_uint4(ok ? g.pre2[p].x : 0u, ok ? g.pre2[p].y : 0u, ok ? g.pre2[p].z : 0u, ok ? g.pre2[p].w : 0u);
                    commit_hl(Kh, Kl, y, row, c);
                }
            }
        }
#ifndef MIXR_X_NOSTORE   // (experiment builds only, tools/build_variant.sh: MIXR_X_* drop one phase of the slice loop -- results are wrong)
        if (!first) store_slice(poff, pz, pzes);
#endif
        __syncthreads();
        if (more) {
#ifndef MIXR_X_NOLOAD
            issue(zs, g, nbh, nes);
#endif
        }
        f32x4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int kend = (M + 31) / 32;   // (uniform) reduction steps that hold a block
#ifndef MIXR_X_NOMFMA
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) {
            if (ks < kend) {
                constexpr int TB = NT < 4 ? NT : 4;   // operand tiles per batch
#pragma unroll
                for (int t4 = 0; t4 < NT; t4 += TB) {
                    bf16x8 sv[TB], sl[FMT == SF_BF16 ? 1 : TB];
#pragma unroll
                    for (int t = 0; t < TB; ++t) {
                        sv[t] = tr_read8(Th, LD, ks * 32, (t4 + t) * 16, lane);
                        if constexpr (sf_has_lo(FMT)) sl[t] = tr_read8(Tl, LD, ks * 32, (t4 + t) * 16, lane);
                    }
#pragma unroll
                    for (int t = 0; t < TB; ++t) acc[t4 + t] = mfma_bf16(sv[t], wh[ks][0], acc[t4 + t]);
                    if constexpr (sf_has_lo(FMT)) {
#pragma unroll
                        for (int t = 0; t < TB; ++t) acc[t4 + t] = mfma_bf16(sl[t], wh[ks][0], acc[t4 + t]);
                    }
#pragma unroll
                    for (int t = 0; t < TB; ++t) acc[t4 + t] = mfma_bf16(sv[t], wl[ks][0], acc[t4 + t]);
                }
            }
        }
#endif
        if constexpr (DW) {   // dW[i][j] += sum_e dG[i][e] KV[j][e]: rows i of this wave, every column tile that holds a block
            if (wave * 16 < M) {   // (uniform)
#pragma unroll
                for (int k2 = 0; k2 < TE / 32; ++k2) {
                    const bf16x8 ah = row_read8(Th, LD, wave * 16, k2 * 32, lane), al = row_read8(Tl, LD, wave * 16, k2 * 32, lane);   // A[m = i][k = e]
#pragma unroll
                    for (int jt = 0; jt < NW; ++jt) {
                        if (jt * 16 < M) {   // (uniform)
                            const bf16x8 bh_ = row_read8(Kh, LD, jt * 16, k2 * 32, lane), bl_ = row_read8(Kl, LD, jt * 16, k2 * 32, lane);   // B[k = e][n = j]
                            dwacc[jt] = mfma_bf16(ah, bh_, dwacc[jt]);
                            dwacc[jt] = mfma_bf16(ah, bl_, dwacc[jt]);
                            dwacc[jt] = mfma_bf16(al, bh_, dwacc[jt]);
                        }
                    }
                }
            }
        }
        // lane: elements 16 t + 4 kg .. + 3 of output block 16 wave + nl -> staging tile [block][element]
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if constexpr (FMT == SF_BF16)
                *reinterpret_cast<uint2*>(reinterpret_cast<u16*>(Os) + (wave * 16 + nl) * LD + t * 16 + kg * 4) =
                    make_uint2(pack_bf16x2(acc[t][0], acc[t][1]), pack_bf16x2(acc[t][2], acc[t][3]));
            else
                *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(Os) + (wave * 16 + nl) * LDO + t * 16 + kg * 4) = acc[t];
        }
        __syncthreads();
        poff = off;
        pz = zslice;
        pzes = zes;
    };
    // The workgroup's summary slices (a consecutive range), then its share of the normaliser slices: slice zi goes to workgroup
    // zi % gridDim.x -- at C2 one of them for a quarter of the workgroups -- so that no workgroup is left with a tail of them (as a
    // range behind the summaries they were 17 latency-bound iterations for the last eight workgroups).
    if (cnt_s > 0) {
        int bh = (int)(s0 / nsl), es = (int)(s0 - (long)bh * nsl);
        issue(std::false_type{}, sga, bh, es);
        for (int it = 0; it < cnt_s; ++it) {
            int nb = bh, ne = es;
            advance(nb, ne);
            body(std::false_type{}, sga, it == 0, it + 1 < cnt_s, bh, es, nb, ne);
            bh = nb;
            es = ne;
        }
    }
    if constexpr (sf_has_lo(FMT)) {
        bool firstz = cnt_s <= 0;
        for (long zi = blockIdx.x; zi < a.ztotal; zi += gridDim.x) {   // (the first one is not prefetched under the last summary slice)
            const long nzi = zi + gridDim.x;
            if (zi == (long)blockIdx.x) issue(std::true_type{}, sga, (int)(zi / nzs), (int)(zi % nzs));
            body(std::true_type{}, sga, firstz, nzi < a.ztotal, (int)(zi / nzs), (int)(zi % nzs), (int)(nzi / nzs), (int)(nzi % nzs));
            firstz = false;
        }
    }
    store_slice(poff, pz, pzes);
    if constexpr (DW) {   // C layout: rows i = 16 wave + 4 kg + r, column j = 16 jt + nl
        float* dp = a.dwp + (long)blockIdx.x * M * M;
#pragma unroll
        for (int jt = 0; jt < NW; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = wave * 16 + kg * 4 + r, j = jt * 16 + nl;
                if (i < M && j < M) dp[(long)i * M + j] = dwacc[jt][r];
            }
    }
}

// -------------------------------------------------------------------------------------------------
// k_sp_mixr_dma<TRANS>: resident-sequence mixing for 16-bit summaries and 192 < M <= 256 blocks.
// k_sp_mixr<16> (sixteen waves, sixteen output blocks each, 64-element slices, register staging) ran at 3 TB/s.  This kernel
//   * runs EIGHT waves with 32 output blocks each (256-register budget): every operand read feeds four MFMAs (two block tiles x
//     weight hi / lo), the next reduction step's operands are requested before the current step's products, half the LDS reads;
//   * stages by LDS-DMA (global_load_lds_dwordx4) into THREE images: two slices (64 KB) in flight while one is multiplied, no
//     staging registers, no ds_write pass.  The DMA writes lane-linear images (8 rows x 8 pieces per wave instruction); the tile
//     kernels' bank swizzle (fast::gt_off) is applied to the SOURCE piece index and again by the transposed operand reads;
//   * stages its results in TWO tiles, so that the stores of slice k - 1 are issued at the top of iteration k, beside the request
//     for slice k + 2, and both travel under the products of slice k: one barrier per slice;
//   * fetches the weights once per workgroup through LDS (mixr_weights) and computes the normaliser's small product (k_wz) with them.
// What it gained is the weight prologue (35 -> 8 us) and the two k_wz launches; the slice loop itself takes the same 170 us in
// every arrangement tried -- DESIGN.md 3d' has the measurements (tools/trace_mixr.py): the launch runs at the chip's power limit.
// vmcnt counts loads and stores in order: slice k's copy is complete when at most the instructions issued after it are
// outstanding (counted per iteration, see the loop).
// Rows past M repeat the last row (their weights are zero), so every reduction step runs unguarded.
// -------------------------------------------------------------------------------------------------
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
constexpr int MIXR_DMA_NBUF = 3;   // input images; two staging tiles follow them
constexpr int MIXR_DMA_T = 512;
__host__ __device__ constexpr int sp_mixr_dma_smem() { return (MIXR_DMA_NBUF + 2) * 256 * 64 * 2; }

template <int TRANS>
__global__ __launch_bounds__(MIXR_DMA_T) void k_sp_mixr_dma(const MixrArgs a) {
    constexpr int NW = 8, NB = 2, TE = 64, ROWS = 256, NK = 8, NT = 4, NBUF = MIXR_DMA_NBUF, IMG = ROWS * TE, NTH = MIXR_DMA_T, NP = 4;
    static_assert(NW * NB * 16 == ROWS && NTH == 64 * NW, "eight waves of 32 output blocks");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u16* lds = reinterpret_cast<u16*>(smem_raw);   // [NBUF] input images, then two output staging tiles
    u16* Os = lds + NBUF * IMG;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nl = lane & 15, kg = lane >> 4;
    const int M = a.M;
    const long nsl = a.E / TE;
    const long s0 = (long)blockIdx.x * a.spw;
    const int cnt = (int)min((long)a.spw, a.total - s0);
    if (cnt <= 0) return;
    // B operands of the wave's 32 output blocks (hi + lo), through LDS (mixr_weights; the not yet used images)
    bf16x8 wh[NK][NB], wl[NK][NB];
    static_assert((TRANS ? 64 * (ROWS + 4) : ROWS * 68) * 4 <= NBUF * IMG * 2, "weight chunk must fit in the images");
    mixr_weights<TRANS, NTH, ROWS, NK, NB>(wh, wl, reinterpret_cast<float*>(smem_raw), a.W, a.ldw, M, wave * 32, tid);
    // the weights are in, and converted before the first copy is issued (the compiler's own waits for them would otherwise sit
    // behind the prologue's copies and drain them): from here on the outstanding-instruction count is ours
#pragma unroll
    for (int ks = 0; ks < NK; ++ks)
#pragma unroll
        for (int n = 0; n < NB; ++n) asm volatile("" : "+v"(wh[ks][n]), "+v"(wl[ks][n]));
    wait_vmcnt<0>();
    auto slice_off = [&](int bh, int es) { return ((long)bh * M * a.es + (long)es * TE) * 2; };   // bytes
    auto advance = [&](int& bh, int& es) { if (++es == (int)nsl) { es = 0; ++bh; } };
    int cbh = (int)(s0 / nsl), ces = (int)(s0 - (long)cbh * nsl), nbh = cbh, nes = ces;
    // The normaliser's small product for every (b, h) whose first slice is this workgroup's: z as bf16 hi + lo in a swizzled tile
    // [256 r][hi s 0..15 | lo s 16..31], the weights already in registers, three products (hi hi + hi lo + lo hi) per step.
    // (Two launches of k_wz -- 30 + 37 us at the 256 x 16 shape for 2 MB of z -- become 3 us here.)
    if (a.zin) {
        u16* Zt = lds;
        const int S = a.S;
        int zbh = cbh + (ces ? 1 : 0);
        for (long first = (long)zbh * nsl; first < s0 + cnt; first += nsl, ++zbh) {
            __syncthreads();
            {
                const int row = tid >> 1, h8 = (tid & 1) * 8;
                float v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = (row < M && h8 + i < S) ? gld<float>(a.zin + ((long)zbh * M + row) * S + h8 + i) : 0.f;
                uint4 hi, lo;
                split8(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]}, hi, lo);
                *reinterpret_cast<uint4*>(Zt + fast::gt_off(row, h8)) = hi;
                *reinterpret_cast<uint4*>(Zt + fast::gt_off(row, 16 + h8)) = lo;
            }
            __syncthreads();
            f32x4 za[NB];
#pragma unroll
            for (int n = 0; n < NB; ++n) za[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < NK; ++ks) {
                const bf16x8 zh = fast::tr_read8_gt(Zt, ks * 32, 0, lane), zl = fast::tr_read8_gt(Zt, ks * 32, 16, lane);
#pragma unroll
                for (int n = 0; n < NB; ++n) {
                    za[n] = mfma_bf16(zh, wh[ks][n], za[n]);
                    za[n] = mfma_bf16(zh, wl[ks][n], za[n]);
                    za[n] = mfma_bf16(zl, wh[ks][n], za[n]);
                }
            }
            // lane: s = 4 kg .. + 3 of output block o = 32 wave + 16 n + nl
#pragma unroll
            for (int n = 0; n < NB; ++n) {
                const int o = wave * 32 + n * 16 + nl;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int sc = kg * 4 + i;
                    if (o < M && sc < S) a.zout[((long)zbh * M + o) * S + sc] = TRANS ? za[n][i] : 1.f / (a.eps + za[n][i]);
                }
            }
        }
        __syncthreads();
        wait_vmcnt<0>();
    }
    // DMA units of a slice: 32 x (8 rows x 128 bytes); wave w copies rows 8 w + 64 p ..; lane -> row + lane / 8,
    // LDS position lane % 8 <- source piece (lane % 8) ^ swizzle(row)
    unsigned soff[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int row = p * 64 + wave * 8 + (lane >> 3), piece = (lane & 7) ^ ((row ^ (row >> 1)) & 7);
        soff[p] = (unsigned)((long)min(row, M - 1) * a.es * 2 + piece * 16);
    }
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr(lds));
    auto issue = [&](int k, long boff) {
        const char* base = reinterpret_cast<const char*>(a.in) + boff;
        const unsigned buf = lds0 + (unsigned)((k % NBUF) * IMG * 2) + (unsigned)(wave * 8 * TE * 2);
#pragma unroll
        for (int p = 0; p < NP; ++p) glds16(base + soff[p], buf + (unsigned)(p * 64 * TE * 2));
    };
    // this thread's four 16-byte store pieces: piece v = tid + p NTH -> row v / 8, column piece v % 8
    unsigned goff[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int v = tid + p * NTH, row = v >> 3, c = v & 7;
        goff[p] = (unsigned)((long)min(row, M - 1) * a.es * 2 + c * 16);
    }
    // transposed operand reads: the piece permutation depends on the row's low four bits only, so the addresses of reduction step 0
    // serve every step with a constant offset, and element tile t is tile 0 with bit t of the piece index flipped (offset ^ 16 t)
    const int g = lane >> 4, li = lane & 15;
    const int tr0 = fast::gt_off(g * 8 + (li >> 2), (li & 3) * 4), tr1 = fast::gt_off(g * 8 + (li >> 2) + 4, (li & 3) * 4);
    auto operands = [&](const u16* Th, int ks, bf16x8 (&sv)[NT]) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const s16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_S16X4(Th + ks * 32 * TE + (tr0 ^ (t << 4))));
            const s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_S16X4(Th + ks * 32 * TE + (tr1 ^ (t << 4))));
            fast::s16x8 r8;
            r8[0] = lo4[0]; r8[1] = lo4[1]; r8[2] = lo4[2]; r8[3] = lo4[3];
            r8[4] = hi4[0]; r8[5] = hi4[1]; r8[6] = hi4[2]; r8[7] = hi4[3];
            sv[t] = __builtin_bit_cast(bf16x8, r8);
        }
    };

    // One barrier per slice.  Iteration k: wait for slice k's copy, barrier, THEN store slice k - 1 from its staging tile and request
    // slice k + 2 -- both travel while slice k is multiplied -- and stage slice k's result in the other staging tile.
    //   staging tile (k & 1): written at the end of iteration k, read at the top of iteration k + 1, rewritten in k + 2 (barrier k + 2 between)
    //   image k % 3: refilled by the copy of slice k + 3, issued after barrier k + 1, i.e. after everyone's products of slice k
    // vmcnt (in order): younger than slice k's copy are the stores of slice k - 2 (k >= 2) and the copy of slice k + 1.
    for (int k = 0; k < NBUF - 1 && k < cnt; ++k) {
        issue(k, slice_off(nbh, nes));
        advance(nbh, nes);
    }
    auto store_slice = [&](const u16* St, long off) {
        char* ob = reinterpret_cast<char*>(a.out) + off;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int v = tid + p * NTH, row = v >> 3, c = v & 7;
            const uint4 x = *reinterpret_cast<const uint4*>(St + fast::gt_off(row, c * 8));
            if (row < M) gst<uint4>(ob + goff[p], x);
        }
    };
    long off_prev = 0;
    for (int k = 0; k < cnt; ++k) {
        const long off = slice_off(cbh, ces);
        advance(cbh, ces);
        const int younger = (k + 1 < cnt ? 1 : 0) + (k >= 2 ? 1 : 0);   // in units of NP instructions
        auto stamp = [&](int i) { if (a.trace && tid == 0 && blockIdx.x < 8 && k < 32) a.trace[(blockIdx.x * 32 + k) * 8 + i] = __builtin_amdgcn_s_memtime(); };
        stamp(0);
        if (younger == 2)      wait_vmcnt<2 * NP>();
        else if (younger == 1) wait_vmcnt<NP>();
        else                   wait_vmcnt<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (this wave's staging writes of iteration k - 1)
        stamp(4);
        __builtin_amdgcn_s_barrier();
        stamp(1);
        if (k >= 1) store_slice(Os + ((k - 1) & 1) * IMG, off_prev);
        if (k + NBUF - 1 < cnt) {
            issue(k + NBUF - 1, slice_off(nbh, nes));
            advance(nbh, nes);
        }
        stamp(2);
        off_prev = off;
        const u16* Th = lds + (k % NBUF) * IMG;
        u16* St = Os + (k & 1) * IMG;
        f32x4 acc[NB][NT];
#pragma unroll
        for (int n = 0; n < NB; ++n)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[n][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        bf16x8 svA[NT], svB[NT];
        operands(Th, 0, svA);
#pragma unroll
        for (int ks = 0; ks < NK; ks += 2) {
            operands(Th, ks + 1, svB);
#pragma unroll
            for (int n = 0; n < NB; ++n) {
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[n][t] = mfma_bf16(svA[t], wh[ks][n], acc[n][t]);
#ifndef MIXR_NOLO   // (experiment builds only, tools/build_variant.sh -DMIXR_NOLO=1: without the weights' lo products -- results are wrong)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[n][t] = mfma_bf16(svA[t], wl[ks][n], acc[n][t]);
#endif
            }
            if (ks + 2 < NK) operands(Th, ks + 2, svA);
#pragma unroll
            for (int n = 0; n < NB; ++n) {
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[n][t] = mfma_bf16(svB[t], wh[ks + 1][n], acc[n][t]);
#ifndef MIXR_NOLO
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[n][t] = mfma_bf16(svB[t], wl[ks + 1][n], acc[n][t]);
#endif
            }
        }
        // lane: elements 16 t + 4 kg .. + 3 of output block 32 wave + 16 n + nl; neighbouring element tiles paired into 16-byte pieces
#pragma unroll
        for (int n = 0; n < NB; ++n)
#pragma unroll
            for (int t = 0; t < NT; t += 2) {
                const uint4 pc = fast::pair_pieces(make_uint2(pack_bf16x2(acc[n][t][0], acc[n][t][1]), pack_bf16x2(acc[n][t][2], acc[n][t][3])),
                                                   make_uint2(pack_bf16x2(acc[n][t + 1][0], acc[n][t + 1][1]), pack_bf16x2(acc[n][t + 1][2], acc[n][t + 1][3])));
                *reinterpret_cast<uint4*>(St + fast::gt_off(wave * 32 + n * 16 + nl, (t + (kg & 1)) * 16 + 8 * (kg >> 1))) = pc;
            }
        stamp(3);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    store_slice(Os + ((cnt - 1) & 1) * IMG, off_prev);
}

}  // namespace sp
}  // namespace mhla
