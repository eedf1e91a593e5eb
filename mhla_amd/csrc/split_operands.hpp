// Block-mix split kernels (split.hpp): the element and format helpers, tile geometry and staged-matrix layout they share.
#pragma once
#include <type_traits>

#include "blockmix.hpp"
#include "fused.hpp"

namespace mhla {
namespace sp {

using fast::bf16x8;
using fast::mfma_bf16;
using fast::tr_read8;
using fast::s16x4;
using fast::s16x8;
using fast::u16;

// A operand with the reduction index along the rows' columns: A[m][k] = T[c0 + m][k0 + 8 kg .. + 7]
__device__ __forceinline__ bf16x8 row_read8(const u16* tile, int ld, int c0, int k0, int lane) {
    return *reinterpret_cast<const bf16x8*>(tile + (c0 + (lane & 15)) * ld + k0 + (lane >> 4) * 8);
}

template <typename T>
__device__ __forceinline__ void ld8(const T* p, f32x4& a, f32x4& b) {
    a = Io<T>::ld4(p);
    b = Io<T>::ld4(p + 4);
}
// 4 elements of TO as loaded (packed for 16-bit types) and their conversion to fp32
template <typename TO> struct Raw4 { typedef uint2 type; };
template <> struct Raw4<float> { typedef f32x4 type; };
__device__ __forceinline__ f32x4 raw4_to_f32(bf16_t, uint2 r) {
    return f32x4{__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16), __uint_as_float(r.y & 0xffff0000u)};
}
__device__ __forceinline__ f32x4 raw4_to_f32(f16_t, uint2 r) {
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    const h4 h = __builtin_bit_cast(h4, r);
    return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}
__device__ __forceinline__ f32x4 raw4_to_f32(float, f32x4 r) { return r; }
__device__ __forceinline__ void relu8(f32x4& a, f32x4& b, float eps) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a[i] = fmaxf(a[i], 0.f) + eps;
        b[i] = fmaxf(b[i], 0.f) + eps;
    }
}
// 8 fp32 -> 8 bf16 hi + 8 bf16 lo (packed, element 0 in the low half of word 0)
__device__ __forceinline__ void split8(const f32x4& a, const f32x4& b, uint4& hi, uint4& lo) {
    const float x[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    unsigned h[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        h[i] = pack_bf16x2(x[2 * i], x[2 * i + 1]);
        l[i] = pack_bf16x2(x[2 * i] - __uint_as_float(h[i] << 16), x[2 * i + 1] - __uint_as_float(h[i] & 0xffff0000u));
    }
    hi = make_uint4(h[0], h[1], h[2], h[3]);
    lo = make_uint4(l[0], l[1], l[2], l[3]);
}
__device__ __forceinline__ bf16x8 as_bf16x8(const uint4& v) { return __builtin_bit_cast(bf16x8, v); }
// rotate the 4 consecutive channel pairs (x[2i], x[2i+1]) held in (a, b) by the angles (c[i], s[i])
// (rope_apply, wan/mhla_utils.py:127-156: complex multiply of consecutive pairs)
__device__ __forceinline__ void rope8(f32x4& a, f32x4& b, const f32x4& c, const f32x4& s) {
    const f32x4 a0 = a, b0 = b;
    a[0] = a0[0] * c[0] - a0[1] * s[0]; a[1] = a0[0] * s[0] + a0[1] * c[0];
    a[2] = a0[2] * c[1] - a0[3] * s[1]; a[3] = a0[2] * s[1] + a0[3] * c[1];
    b[0] = b0[0] * c[2] - b0[1] * s[2]; b[1] = b0[0] * s[2] + b0[1] * c[2];
    b[2] = b0[2] * c[3] - b0[3] * s[3]; b[3] = b0[2] * s[3] + b0[3] * c[3];
}

// transposed rotation of a gradient in output layout: the lane's 4 consecutive features are 2 pairs with angles (c[0], s[0]), (c[1], s[1])
__device__ __forceinline__ void unrope4(f32x4& g, const f32x2& c, const f32x2& s) {
    const f32x4 g0 = g;
    g[0] = g0[0] * c[0] + g0[1] * s[0]; g[1] = g0[1] * c[0] - g0[0] * s[0];
    g[2] = g0[2] * c[1] + g0[3] * s[1]; g[3] = g0[3] * c[1] - g0[2] * s[1];
}

// -------------------------------------------------------------------------------------------------
// p24: block summaries as 24-bit floats -- sign, 8 exponent bits, 15 stored mantissa bits: the top three bytes of the fp32, i.e. 16
// significand bits, which is what the hi + lo bf16 operand pair of the products carries anyway -- in 3 / 4 of the bytes.  A summary row
// of E elements is two planes: [E x u16: the top two bytes = the bf16 hi operand as it is][E x u8: the third byte].  Whole-block readers
// and writers see two contiguous runs; a 64-element slice of the resident mixing is one 128-byte line of the hi plane and half a line
// of the lo plane (its neighbour slice, taken next by the same workgroup, owns the other half).  (192-byte
// groups of 64 elements -- hi and lo side by side -- put every second hi piece across two lines, and the streaming loads dropped the
// shared line between slices: the mixing kernels ran 10-25 % slower than on fp32 summaries.)
// The lo operand, value - hi, has at most 8 significant bits: exact in bf16.  Used by the resident-mixing pipeline on 16-bit tensors
// (capi_bm_typed.hpp bm_p24); rows keep their stride in float units (BmWs::es), 3 E / 4 + padding.
// -------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned p24_round(float x) { return (__float_as_uint(x) + 0x80u) & 0xffffff00u; }
// 8 values -> their hi piece (16 bytes) and lo piece (8 bytes)
__device__ __forceinline__ void p24_pack8(const f32x4& a, const f32x4& b, uint4& hi, uint2& lo) {
    unsigned r[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) { r[i] = p24_round(a[i]); r[4 + i] = p24_round(b[i]); }
    hi = make_uint4(__builtin_amdgcn_perm(r[1], r[0], 0x07060302u), __builtin_amdgcn_perm(r[3], r[2], 0x07060302u),
                    __builtin_amdgcn_perm(r[5], r[4], 0x07060302u), __builtin_amdgcn_perm(r[7], r[6], 0x07060302u));
    // byte 1 of each value: (r1.b1, r0.b1) -> low half, (r3.b1, r2.b1) -> high half
    lo = make_uint2(__builtin_amdgcn_perm(__builtin_amdgcn_perm(r[3], r[2], 0x0c0c0501u), __builtin_amdgcn_perm(r[1], r[0], 0x0c0c0501u), 0x05040100u),
                    __builtin_amdgcn_perm(__builtin_amdgcn_perm(r[7], r[6], 0x0c0c0501u), __builtin_amdgcn_perm(r[5], r[4], 0x0c0c0501u), 0x05040100u));
}
// the bf16 lo operands of 8 stored values: (hi | third byte) - hi, exact
__device__ __forceinline__ uint4 p24_lo8(const uint4& hi, const uint2& lo) {
    const unsigned hw[4] = {hi.x, hi.y, hi.z, hi.w};
    const unsigned lw[2] = {lo.x, lo.y};
    unsigned o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {   // elements 2 j (low half of the word) and 2 j + 1
        const unsigned l = lw[j >> 1];
        // v_perm_b32 (S0, S1): selector bytes 0-3 pick from S1, 4-7 from S0, 0x0c is a zero byte
        const unsigned h0 = hw[j] << 16, h1 = hw[j] & 0xffff0000u;
        const unsigned f0 = __builtin_amdgcn_perm(hw[j], l, (j & 1) ? 0x05040200u | 0x0cu : 0x05040000u | 0x0cu);
        const unsigned f1 = __builtin_amdgcn_perm(hw[j], l, (j & 1) ? 0x07060300u | 0x0cu : 0x07060100u | 0x0cu);
        const float d0 = __uint_as_float(f0) - __uint_as_float(h0), d1 = __uint_as_float(f1) - __uint_as_float(h1);
        o[j] = __builtin_amdgcn_perm(__float_as_uint(d1), __float_as_uint(d0), 0x07060302u);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}
// the 8 stored values as floats
__device__ __forceinline__ void p24_unpack8(const uint4& hi, const uint2& lo, f32x4& a, f32x4& b) {
    const unsigned hw[4] = {hi.x, hi.y, hi.z, hi.w};
    const unsigned lw[2] = {lo.x, lo.y};
    float f[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned l = lw[j >> 1];
        f[2 * j] = __uint_as_float(__builtin_amdgcn_perm(hw[j], l, (j & 1) ? 0x05040200u | 0x0cu : 0x05040000u | 0x0cu));
        f[2 * j + 1] = __uint_as_float(__builtin_amdgcn_perm(hw[j], l, (j & 1) ? 0x07060300u | 0x0cu : 0x07060100u | 0x0cu));
    }
    a = f32x4{f[0], f[1], f[2], f[3]};
    b = f32x4{f[4], f[5], f[6], f[7]};
}

// -------------------------------------------------------------------------------------------------
// h16 (summary format 2, round 6): block summaries as an fp16 payload x ONE power-of-two multiplier per block row -- 11 significand
// bits, the precision the reference's own products run at (TF32: mhla_dit/train.py:12-13 turns allow_tf32 on for the matmul / 1x1-conv
// of mhla_dit/mhla/mhla.py:262-263) -- in 2 bytes per element where p24 takes 3.  A summary row of E elements is [E x fp16][fp32
// multiplier m at byte 2 E]: value = payload * m.  The kernels that own a whole row (k_sp_state) take m from the row's measured
// maximum (payload maximum in [2^14, 2^15)); the mixing kernels, whose output rows are spread over workgroups, take it from the bound
// |out_o[e]| <= sum_r |W(o, r)| 2^15 m_r, which every workgroup computes alike from the input rows' multipliers -- a loose bound costs
// nothing: fp16 keeps 11 bits over 29 binades.  Consumers decode to the same bf16 hi + lo operand pair as every other fp32-grade format
// (hi = top 16 bits of payload * m, lo = the remaining 3 significand bits: exact).  16-bit tensors with blocks of >= 16 tokens
// (capi_common.hpp bm_sumfmt); tools/sim_h16.py is the CPU model of its error (<= 4e-4 of a result's maximum on every BASELINE shape).
// -------------------------------------------------------------------------------------------------
// (the format's helpers -- h16_mult_from_max / _from_bound, h16_inv, h16_pack2 / _pack8, h16_split8 -- are in common.hpp: the causal pipeline uses them too)

template <int DT> struct Geo {
    static constexpr int CGS = DT > 4 ? 16 : 8;        // column groups of 8 per tile row
    static constexpr int DW = CGS * 8;                 // tile width (columns), >= 16 DT
    static constexpr int LD = DW + 16;                 // LDS row stride (bf16) of k_sp_state's token tiles (row r at mat_row(r), below) ...
    static constexpr int LDR = DW + 8;                 // ... except in its row-dots-from-G variant, whose fourth workgroup per CU needs the 2 KB
    static constexpr int RPP = NTHREADS / CGS;         // tile rows covered per pass of the 256 threads
    static constexpr int RT = (DT + 3) / 4;            // 16-row output tiles per wave
    static constexpr int KST = (DT + 1) / 2;           // reduction steps of 32 over a head dim
};

// (used by k_sp_state's row-dots-from-G variant as well as by the output and token-gradient kernels further down)
// LDS row stride (bf16) of a staged D x D summary matrix [KST * 32 rows][KST * 32 columns + 8]: the reads cover KST * 32
// columns, not the DW of the token tiles (D = 72: 104 instead of 136 -> a third workgroup per CU for the fp32 kernels)
// Bank layout (round 6).  gfx950's LDS has 64 banks and serves the 16-byte row reads in groups of 16 lanes, the transpose reads in groups
// of 32 (MI355X_MICROARCH.md, LDS): with the round-1 padding of 8 elements (derived for 32 banks) every operand read of these kernels is
// 2-way conflicted (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE 0.28 - 0.44 at C2; `tools/lds_conflicts.py split` reproduces it).  In the
// new layout rows are padded by 16 elements (consecutive rows 8 banks apart) and matrix row r is kept at LDS row mat_row(r) = r with bits
// 2 and 3 swapped: the 32 lanes of a transpose read (rows 8 g + j, g = 0, 1) then touch 8 consecutive LDS rows = all 64 banks once, and a
// 16-byte row read's lane groups keep their sets of rows.  Counters after: 0.00 (k_sp_out, k_sp_bwd_dq), 0.16 (k_sp_bwd_dkv: its strip
// stores).  What it buys is small, because these kernels wait for HBM, not for the LDS: C2 step 0.382 -> 0.373 ms (k_sp_bwd_dkv 81.8 ->
// 76.6 us; at 256 blocks of 16 tokens 214 -> 191 us), nothing at D = 72 .. 96, and at D = 128 the Wan inference output kernel LOSES 11 %
// (5.69 -> 6.3 ms per forward, twice) -- so the staged matrices take it for D <= 64 only (MAT_NEW_MAX_DT; `tools/ab_configs.sh` is the
// A/B), k_sp_state's token tiles always except in the row-dots-from-G variant (whose fourth workgroup per CU needs the 2 KB).
// Everything that touches a staged matrix goes through mat_row / mat_tr_read8 / mat_row_read8.
#ifndef MAT_NEW_MAX_DT
#define MAT_NEW_MAX_DT 4
#endif
template <int DT> __host__ __device__ constexpr bool mat_new() { return DT <= MAT_NEW_MAX_DT; }
template <int DT>
__host__ __device__ constexpr int mat_ld() { return Geo<DT>::KST * 32 + (mat_new<DT>() ? 16 : 8); }
template <bool NEW = true>
__host__ __device__ constexpr int mat_row(int r) { return NEW ? ((r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1)) : r; }
// tr_read8 of a staged matrix: lane (c = lane & 15, g = lane >> 4) receives T[k0 + 8 g + 0..7][c0 + c]   (k0 a multiple of 32)
template <bool NEW = true>
__device__ __forceinline__ bf16x8 mat_tr_read8(const u16* tile, int ld, int k0, int c0, int lane) {
    if constexpr (!NEW) return tr_read8(tile, ld, k0, c0, lane);
    const int g = lane >> 4, li = lane & 15;
    const u16* p = tile + (k0 + (g >> 1) * 16 + (g & 1) * 4 + (li >> 2)) * ld + c0 + (li & 3) * 4;   // = mat_row(k0 + 8 g + (li >> 2))
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_S16X4(p));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_S16X4(p + 8 * ld));                  // = mat_row(.. + 4)
    s16x8 r;
    r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
    r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
    return __builtin_bit_cast(bf16x8, r);
}
// row_read8 of a staged matrix: A[m][k] = T[c0 + m][k0 + 8 kg .. + 7]   (c0 a multiple of 16)
template <bool NEW = true>
__device__ __forceinline__ bf16x8 mat_row_read8(const u16* tile, int ld, int c0, int k0, int lane) {
    return *reinterpret_cast<const bf16x8*>(tile + (c0 + mat_row<NEW>(lane & 15)) * ld + k0 + (lane >> 4) * 8);
}
template <int DT, int FMT>
__host__ __device__ constexpr int sp_out_smem() { return (sf_has_lo(FMT) ? 2 : 1) * Geo<DT>::KST * 32 * mat_ld<DT>() * 2; }

// EPI: the per-head RMSNorm (x SiLU gate) that follows the operator in the Wan host (wan/mhla_utils.py:356-362) is applied
// to the token's D outputs before they are stored, in the dtype TO of the host's activations: O is rounded to TO (the
// `.to(dtype)` at :356), normalised over the head dim in fp32, scaled by the norm weight and the gate, stored once.
// D x D summary matrix in the format FMT -> LDS [KP][LD] hi (/ lo) tiles; rows and columns >= D zero.  NT threads.
template <int DT, int FMT, int NT = NTHREADS>
__device__ __forceinline__ void stage_mat_split(u16* __restrict__ Gh, u16* __restrict__ Gl, const float* __restrict__ base, long elem_off, int D, int tid) {
    constexpr int LD = mat_ld<DT>(), CGS = Geo<DT>::CGS, RPP = NT / CGS, KP = Geo<DT>::KST * 32;
    const int r0 = tid / CGS, cg = (tid % CGS) * 8;
    constexpr int PASSES = (KP + RPP - 1) / RPP, UB = PASSES < 4 ? PASSES : (PASSES % 4 == 0 ? 4 : (PASSES % 3 == 0 ? 3 : 2));
    static_assert(PASSES % UB == 0, "staging batches must tile the passes");
    const float* g = base + elem_off;
    const u16* g16 = reinterpret_cast<const u16*>(base) + elem_off;
    float hm = 0.f;   // h16: the row's multiplier
    if constexpr (FMT == SF_H16) hm = gld<float>(reinterpret_cast<const char*>(base + elem_off) + 2 * D * D);
    for (int pb = 0; pb < PASSES; pb += UB) {
        f32x4 x[UB][2];
        uint4 x16[UB];
        uint2 xl[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            // (every load unconditional, from a clamped position: rows / columns past D are zeroed below.  Behind `if (r < D && cg < D)` the
            // pieces of a batch were round trips of their own -- hipcc waits for everything in flight where a branch with a load in it joins)
            const int r = min(r0 + RPP * (pb + u), D - 1), c = min(cg, D - 8);
            x[u][0] = x[u][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            x16[u] = make_uint4(0, 0, 0, 0);
            xl[u] = make_uint2(0, 0);
            if (sf_packed(FMT)) {   // 8 elements: a piece of the hi plane and one of the lo plane (elem_off counts floats: the row's start)
                const int e = r * D + c;
                const char* rowp = reinterpret_cast<const char*>(base + elem_off);
                x16[u] = gld<uint4>(rowp + 2 * e);
                if constexpr (FMT == SF_P24) xl[u] = gld<uint2>(rowp + 2 * D * D + e);
            } else if (FMT == SF_BF16) {
                x16[u] = gld<uint4>(g16 + (long)r * D + c);
            } else {
                const float* src = g + (long)r * D + c;
                x[u][0] = gld<f32x4>(src);
                x[u][1] = gld<f32x4>(src + 4);
            }
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int r = r0 + RPP * (pb + u), off = mat_row<mat_new<DT>()>(r) * LD + cg;
            if (!(r < D && cg < D)) {   // (no memory operation in here)
                x[u][0] = x[u][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                x16[u] = make_uint4(0, 0, 0, 0);
                xl[u] = make_uint2(0, 0);
            }
            if (r < KP && cg < KP) {
                if (FMT == SF_H16) {
                    uint4 hi, lo;
                    h16_split8(x16[u], hm, hi, lo);
                    *reinterpret_cast<uint4*>(Gh + off) = hi;
                    *reinterpret_cast<uint4*>(Gl + off) = lo;
                } else if (FMT == SF_P24) {
                    *reinterpret_cast<uint4*>(Gh + off) = x16[u];
                    *reinterpret_cast<uint4*>(Gl + off) = p24_lo8(x16[u], xl[u]);
                } else if (FMT == SF_BF16) {
                    *reinterpret_cast<uint4*>(Gh + off) = x16[u];
                } else {
                    uint4 hi, lo;
                    split8(x[u][0], x[u][1], hi, lo);
                    *reinterpret_cast<uint4*>(Gh + off) = hi;
                    *reinterpret_cast<uint4*>(Gl + off) = lo;
                }
            }
        }
    }
}

// Payload operands (common.hpp tok16_operands): where the summary is h16, the tensors are 16-bit, D <= 64 and the token operand of a
// product is an exact tensor element, the staged matrix is ONE plane of the payload as stored and the token row a scaled fp16 operand --
// one fp16 MFMA per step for the two or three bf16 ones, half the LDS, no decode.  -DSP_PAYLOAD_OPERANDS=0 (MHLA_BUILD_DEFINES) builds
// the hi + lo form for A/B timing.  Used by k_sp_bwd_dq (its dO rows) and by the row dots of k_sp_state<1> (sp_payrd).  Not by k_sp_bwd_dkv:
// built and measured (profiles/payload_operands.md) -- 126 -> 113 VGPRs still leave it four workgroups per CU, 61.7 -> 62.8 us at C2.  Not
// by k_sp_out: its q rows may be relu'd or rotated by a run-time flag of the call, and it holds the most workgroups a CU takes already.
#ifndef SP_PAYLOAD_OPERANDS
#define SP_PAYLOAD_OPERANDS 1
#endif
template <typename T, int DT, int FMT, bool ROPE = false>
__host__ __device__ constexpr bool sp_payop() { return SP_PAYLOAD_OPERANDS && FMT == SF_H16 && sizeof(T) == 2 && DT <= 4 && !ROPE; }
// h16 row of a D x D summary -> ONE LDS plane [KP][mat_ld] of its payload, undecoded, in the mat_row layout (mat_row_read8 /
// mat_tr_read8 then deliver fp16 operands: as_f16x8); rows and columns >= D zero.  Returns the row's multiplier m.  Through registers,
// not global_load_lds_dwordx4: the LDS-DMA writes a wave's 64 pieces back to back, which allows neither the padded row stride nor
// the zero rows and columns of a D < KP matrix, and the matrix is one round trip per workgroup that the token rows' loads already cover.
template <int DT, int NT = NTHREADS>
__device__ __forceinline__ float stage_mat_payload(u16* __restrict__ G, const float* __restrict__ base, long elem_off, int D, int tid) {
    constexpr int LD = mat_ld<DT>(), CGS = Geo<DT>::CGS, RPP = NT / CGS, KP = Geo<DT>::KST * 32;
    const int r0 = tid / CGS, cg = (tid % CGS) * 8;
    constexpr int PASSES = (KP + RPP - 1) / RPP;
    const char* rowp = reinterpret_cast<const char*>(base + elem_off);   // (elem_off counts floats: the row's start)
    const float hm = gld<float>(rowp + 2 * D * D);
    uint4 x16[PASSES];
#pragma unroll
    for (int u = 0; u < PASSES; ++u) {   // (every load unconditional, from a clamped position: see stage_mat_split)
        const int r = min(r0 + RPP * u, D - 1), c = min(cg, D - 8);
        x16[u] = gld<uint4>(rowp + 2 * (r * D + c));
    }
#pragma unroll
    for (int u = 0; u < PASSES; ++u) {
        const int r = r0 + RPP * u;
        if (r < KP && cg < KP) *reinterpret_cast<uint4*>(G + mat_row<mat_new<DT>()>(r) * LD + cg) = (r < D && cg < D) ? x16[u] : make_uint4(0, 0, 0, 0);
    }
    return hm;
}

// stage_mat_split in two halves for 24-bit summaries staged in ONE batch (D = 128 by 512 threads: four passes): the loads are requested,
// the workgroup multiplies a round of token tiles, then the pieces are committed (k_sp_out<.., FLAT>)
template <int DT, int NT>
struct MatStage {
    static constexpr int PASSES = (Geo<DT>::KST * 32 + NT / Geo<DT>::CGS - 1) / (NT / Geo<DT>::CGS);
    uint4 x16[PASSES];
    uint2 xl[PASSES];
};
// (real = false: the loads are issued all the same -- no branch around them -- but every lane reads the matrix's first piece)
template <int DT, int NT>
__device__ __forceinline__ void stage_mat_issue(MatStage<DT, NT>& g, const float* __restrict__ base, long elem_off, int D, int tid, bool real = true) {
    constexpr int CGS = Geo<DT>::CGS, RPP = NT / CGS;
    const int r0 = tid / CGS, cg = (tid % CGS) * 8;
    const char* rowp = reinterpret_cast<const char*>(base + elem_off);
#pragma unroll
    for (int u = 0; u < MatStage<DT, NT>::PASSES; ++u) {   // (unconditional, from clamped addresses: rows / columns past D are zeroed at the commit)
        const int r = min(r0 + RPP * u, D - 1), c = min(cg, D - 8), e = real ? r * D + c : 0;
        g.x16[u] = gld<uint4>(rowp + 2 * e);
        g.xl[u] = gld<uint2>(rowp + 2 * D * D + e);
    }
}
template <int DT, int NT>
__device__ __forceinline__ void stage_mat_commit(u16* __restrict__ Gh, u16* __restrict__ Gl, const MatStage<DT, NT>& g, int D, int tid) {
    constexpr int LD = mat_ld<DT>(), CGS = Geo<DT>::CGS, RPP = NT / CGS, KP = Geo<DT>::KST * 32;
    const int r0 = tid / CGS, cg = (tid % CGS) * 8;
#pragma unroll
    for (int u = 0; u < MatStage<DT, NT>::PASSES; ++u) {
        const int r = r0 + RPP * u, off = mat_row<mat_new<DT>()>(r) * LD + cg;
        const bool in = r < D && cg < D;
        const uint4 hi = in ? g.x16[u] : make_uint4(0, 0, 0, 0);
        const uint2 lo = in ? g.xl[u] : make_uint2(0, 0);
        if (r < KP && cg < KP) {
            *reinterpret_cast<uint4*>(Gh + off) = hi;
            *reinterpret_cast<uint4*>(Gl + off) = p24_lo8(hi, lo);
        }
    }
}

// -------------------------------------------------------------------------------------------------
// 8 fp32 values -> one 16-byte piece of a 16-bit type
__device__ __forceinline__ uint4 pack8_16(bf16_t, f32x4 a, f32x4 b) {
    return make_uint4(pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3]), pack_bf16x2(b[0], b[1]), pack_bf16x2(b[2], b[3]));
}
__device__ __forceinline__ uint4 pack8_16(f16_t, f32x4 a, f32x4 b) {
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    const h8 h = {(_Float16)a[0], (_Float16)a[1], (_Float16)a[2], (_Float16)a[3], (_Float16)b[0], (_Float16)b[1], (_Float16)b[2], (_Float16)b[3]};
    return __builtin_bit_cast(uint4, h);
}
__device__ __forceinline__ uint4 pack8_16(float, f32x4, f32x4) { return make_uint4(0, 0, 0, 0); }   // (never called: fp32 stores 16-byte pieces already)

// Two neighbouring feature tiles of a token in the products' output layout (a lane owns features 16 ct + 4 kg .. + 3 of each) -> the
// token's row.  16-bit tensors on 16-byte aligned rows (`wide`): lane pairs (kg, kg ^ 1) swap halves, a lane then owns 8 consecutive
// features -- one 16-byte piece -- and the four lanes of a token cover 64 contiguous bytes per instruction (the 8-byte pieces of
// the plain layout cost k_sp_out 1.47x its bytes in HBM writes at C2).  EVERY lane must call this (shuffles); `live`: the lane's
// token exists.
template <typename T>
__device__ __forceinline__ void store_tile_pair(T* tok, int ct, int ntiles, int D, int kg, const f32x4& v0, const f32x4& v1, bool live, bool wide) {
    if constexpr (sizeof(T) == 2) {
        if (wide && ct + 1 < ntiles) {   // (uniform)
            const int podd = kg & 1;
            const f32x4 send = podd ? v0 : v1, keep = podd ? v1 : v0;
            f32x4 recv;
#pragma unroll
            for (int i = 0; i < 4; ++i) recv[i] = __shfl_xor(send[i], 16, 64);
            const int f0 = (ct + podd) * 16 + (kg >> 1) * 8;
            if (live && f0 < D) gst<uint4>(tok + f0, pack8_16(T{}, podd ? recv : keep, podd ? keep : recv));
            return;
        }
    }
    if (live) {
        const int d0 = ct * 16 + kg * 4;
        if (d0 < D) Io<T>::st4(tok + d0, v0);
        if (ct + 1 < ntiles && d0 + 16 < D) Io<T>::st4(tok + d0 + 16, v1);
    }
}
template <typename V>
__device__ __forceinline__ bool view16(const V& w) { return (reinterpret_cast<uintptr_t>(w.ptr) & 15) == 0 && ((w.sb | w.sn | w.sh) & 7) == 0; }

}  // namespace sp
}  // namespace mhla
