// Block-mix split kernels (split.hpp): k_sp_dw and k_sp_dwt, the gradient of the mixing matrix.
#pragma once
#include "split_operands.hpp"

namespace mhla {
namespace sp {

// -------------------------------------------------------------------------------------------------
// k_sp_dw: dwp[bh][split][i][j] = sum_{e in slice} dG_i[e] KV_j[e]  (fp32 operands straight from HBM, split in
// registers; the reduction index is contiguous for both, lane kg takes e = 8 kg .. 8 kg + 7 of every 32).
// grid (tile pairs, bh, E-slices) and output layout as k_dw; each wave reduces a quarter of the slice for the whole
// 64 x 64 tile and the four partial tiles are summed through LDS in wave order.
// -------------------------------------------------------------------------------------------------
constexpr int SP_DW_LD = 68;
constexpr int SP_DW_SMEM = 64 * SP_DW_LD * 4;

// NT: 16-row tiles per side of the output tile (4: 64 x 64; 1 / 2 when M <= 16 / 32, where the full tile would spend 15/16 or 3/4 of
// its loads and MFMAs on clamped rows); UE = 4 / NT reduction steps per loop iteration keep the same number of loads in flight.
// FMT: fp32 words, or SF_BF16 (24-bit summaries: dW rides in k_sp_mixr, or k_sp_dwt below)
template <int FMT, int NT = 4>
__global__ __launch_bounds__(NTHREADS) void k_sp_dw(const DwArgs a) {
    constexpr int UE = 4 / NT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* Rs = reinterpret_cast<float*>(smem_raw);
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nl = lane & 15, kg = lane >> 4;
    // the tile pairs of one (b, h, slice) share their operand rows: consecutive logical indices, which xcd_swizzle keeps on one
    // XCD (one L2) and next to each other in dispatch order
    const int np = gridDim.x, nbh = gridDim.y;
    const int L = fast::xcd_swizzle(blockIdx.x + np * (blockIdx.y + nbh * blockIdx.z), np * nbh * gridDim.z);
    const int unit = L / np, pair = L - unit * np, split = unit / nbh, bh = unit - split * nbh, M = a.M;
    const int it = pair / a.tiles, jt = pair - it * a.tiles;
    const int i0 = it * 64, j0 = jt * 64;
    const long E = a.E;
    const long per = ((E + a.nsplit - 1) / a.nsplit + 127) & ~127L;   // slice: multiple of 4 waves x 32 elements
    const long ebeg = (long)split * per, eend = min(E, ebeg + per);
    const long span = eend > ebeg ? eend - ebeg : 0;
    const long wper = ((span + 3) / 4 + 31) & ~31L;                    // E is a multiple of 32
    const long wbeg = ebeg + wave * wper, wend = min(eend, wbeg + wper);
    const float* xp[NT];
    const float* yp[NT];
    const u16* xp16[NT];
    const u16* yp16[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int ri = min(i0 + t * 16 + nl, M - 1), rj = min(j0 + t * 16 + nl, M - 1);
        xp[t] = a.x + ((long)bh * M + ri) * a.es + kg * 8;
        yp[t] = a.y + ((long)bh * M + rj) * a.es + kg * 8;
        xp16[t] = reinterpret_cast<const u16*>(a.x) + ((long)bh * M + ri) * a.es + kg * 8;
        yp16[t] = reinterpret_cast<const u16*>(a.y) + ((long)bh * M + rj) * a.es + kg * 8;
    }
    f32x4 acc[NT][NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long e0 = wbeg; e0 < wend; e0 += 32 * UE) {
        if constexpr (FMT == SF_BF16) {   // operands as stored
            bf16x8 xa[UE][NT], ya[UE][NT];
#pragma unroll
            for (int u = 0; u < UE; ++u) {
                const long e = e0 + 32 * u;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    xa[u][t] = ya[u][t] = __builtin_bit_cast(bf16x8, make_uint4(0, 0, 0, 0));
                    if (e < wend) {
                        xa[u][t] = *reinterpret_cast<const bf16x8*>(xp16[t] + e);
                        ya[u][t] = *reinterpret_cast<const bf16x8*>(yp16[t] + e);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < UE; ++u)
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[i][j] = mfma_bf16(xa[u][i], ya[u][j], acc[i][j]);
            continue;
        }
        uint4 xh[UE][NT], xl[UE][NT], yh[UE][NT], yl[UE][NT];
        f32x4 raw[UE][2 * NT][2];
#pragma unroll
        for (int u = 0; u < UE; ++u) {
            const long e = e0 + 32 * u;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                raw[u][t][0] = raw[u][t][1] = raw[u][NT + t][0] = raw[u][NT + t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (e < wend) {
                    raw[u][t][0] = *reinterpret_cast<const f32x4*>(xp[t] + e);
                    raw[u][t][1] = *reinterpret_cast<const f32x4*>(xp[t] + e + 4);
                    raw[u][NT + t][0] = *reinterpret_cast<const f32x4*>(yp[t] + e);
                    raw[u][NT + t][1] = *reinterpret_cast<const f32x4*>(yp[t] + e + 4);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < UE; ++u)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                split8(raw[u][t][0], raw[u][t][1], xh[u][t], xl[u][t]);
                split8(raw[u][NT + t][0], raw[u][NT + t][1], yh[u][t], yl[u][t]);
            }
#pragma unroll
        for (int u = 0; u < UE; ++u) {
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = mfma_bf16(as_bf16x8(xh[u][i]), as_bf16x8(yh[u][j]), acc[i][j]);
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = mfma_bf16(as_bf16x8(xh[u][i]), as_bf16x8(yl[u][j]), acc[i][j]);
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = mfma_bf16(as_bf16x8(xl[u][i]), as_bf16x8(yh[u][j]), acc[i][j]);
        }
    }
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float* d = Rs + (i * 16 + kg * 4 + r) * SP_DW_LD + j * 16 + nl;
                        *d = (w == 0 ? 0.f : *d) + acc[i][j][r];
                    }
        }
        __syncthreads();
    }
    float* out = a.out + ((long)bh * a.nsplit + split) * M * M;
    for (int v = tid; v < 64 * 64; v += NTHREADS) {
        const int r = v >> 6, c = v & 63;
        if (i0 + r < M && j0 + c < M) out[(long)(i0 + r) * M + j0 + c] = Rs[r * SP_DW_LD + c];
    }
}

// -------------------------------------------------------------------------------------------------
// k_sp_dwt: the same partials as k_sp_dw for 24-bit summaries (two planes per row: the hi plane is the hi operand, the lo operand is
// rebuilt, p24_lo8) and more than 128 blocks, with the
// operand rows STAGED THROUGH LDS: k_sp_dw's lanes fetch their MFMA operands straight from memory -- 16 rows x 64 bytes (32 for the lo
// plane) per load instruction -- and ran at 2.1-2.6 TB/s of its bytes (C4: 127 us, the 256 x 16 variant: 490 us).  Here a workgroup walks
// its E-slice in chunks of 64 elements: 64 rows of dG and 64 rows of KV as 256-byte (128 + 64) row pieces, 16 or 8 lanes per row, the
// next chunk in flight in registers while the current one is multiplied from hi / lo tiles ([64][72] bf16 x 4: 37 KB); wave w owns the
// 32 x 32 quadrant (w >> 1, w & 1) of the 64 x 64 output tile, so there is no reduction across waves.  Grid and output as k_sp_dw.
// Used on the 24-bit summaries of the Wan shape (E = 16 384, 9 tile pairs: 124 -> 92 us); on fp32 summaries with E = 4 096 and 16 tile
// pairs (the 256 x 16 variant) its 64 chunks of two barriers and 24 products per wave each ran 773 us against k_sp_dw's 490 -- that
// shape keeps k_sp_dw, whose waves multiply whole 64 x 64 tiles from registers.
// -------------------------------------------------------------------------------------------------
constexpr int SP_DWT_LD = 72, SP_DWT_SMEM = 4 * 64 * SP_DWT_LD * 2;
template <int FMT>   // (a template so that only the units that launch it carry it: a plain kernel in this header is emitted by every unit)
__global__ __launch_bounds__(NTHREADS, 2) void k_sp_dwt(const DwArgs a) {
    static_assert(FMT == SF_P24, "fp32 words keep k_sp_dw (above)");
    constexpr int LD = SP_DWT_LD, CE = 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u16* Xh = reinterpret_cast<u16*>(smem_raw);
    u16* Xl = Xh + 64 * LD;
    u16* Yh = Xl + 64 * LD;
    u16* Yl = Yh + 64 * LD;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nl = lane & 15, kg = lane >> 4;
    const int np = gridDim.x, nbh = gridDim.y;
    const int L = fast::xcd_swizzle(blockIdx.x + np * (blockIdx.y + nbh * blockIdx.z), np * nbh * gridDim.z);
    const int unit = L / np, pair = L - unit * np, split = unit / nbh, bh = unit - split * nbh, M = a.M;
    const int it = pair / a.tiles, jt = pair - it * a.tiles;
    const int i0 = it * 64, j0 = jt * 64;
    const long E = a.E;
    const long per = ((E + a.nsplit - 1) / a.nsplit + CE - 1) / CE * CE;   // slice: whole chunks (E is a multiple of 64)
    const long ebeg = (long)split * per, eend = min(E, ebeg + per);
    // the thread's two units per operand: unit v = tid + 256 p -> row v / 8, elements 8 (v % 8) .. + 7 of the chunk
    const char* xr[2];
    const char* yr[2];
    int urow[2], ucol[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int v = tid + p * NTHREADS;
        urow[p] = v >> 3;
        ucol[p] = (v & 7) * 8;
        xr[p] = reinterpret_cast<const char*>(a.x + ((long)bh * M + min(i0 + urow[p], M - 1)) * a.es);
        yr[p] = reinterpret_cast<const char*>(a.y + ((long)bh * M + min(j0 + urow[p], M - 1)) * a.es);
    }
    uint4 xa[2], xb[2], ya[2], yb[2];   // xa = hi piece, xb.xy = lo piece
    auto issue = [&](long e0) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const long e = e0 + ucol[p];
            xa[p] = gld_stream16(xr[p] + 2 * e);
            ya[p] = gld_stream16(yr[p] + 2 * e);
            const uint2 lx = gld<uint2>(xr[p] + 2 * E + e), ly = gld<uint2>(yr[p] + 2 * E + e);
            xb[p] = make_uint4(lx.x, lx.y, 0u, 0u);
            yb[p] = make_uint4(ly.x, ly.y, 0u, 0u);
        }
    };
    auto commit = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const bool okx = i0 + urow[p] < M, oky = j0 + urow[p] < M;   // rows past the last block: zeros
            const int off = urow[p] * LD + ucol[p];
            const uint4 hx = xa[p], lx = p24_lo8(xa[p], make_uint2(xb[p].x, xb[p].y));
            const uint4 hy = ya[p], ly = p24_lo8(ya[p], make_uint2(yb[p].x, yb[p].y));
            // (component-wise: a select of whole uint4 structs goes through the stack)
            auto sel = [](bool ok, const uint4& v) { return make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u); };
            *reinterpret_cast<uint4*>(Xh + off) = sel(okx, hx);
            *reinterpret_cast<uint4*>(Xl + off) = sel(okx, lx);
            *reinterpret_cast<uint4*>(Yh + off) = sel(oky, hy);
            *reinterpret_cast<uint4*>(Yl + off) = sel(oky, ly);
        }
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wi = wave >> 1, wj = wave & 1;
    if (ebeg < eend) issue(ebeg);
    for (long e0 = ebeg; e0 < eend; e0 += CE) {
        commit();
        __syncthreads();
        if (e0 + CE < eend) issue(e0 + CE);
#pragma unroll
        for (int ks = 0; ks < CE / 32; ++ks) {
            bf16x8 ah[2], al[2], bh_[2], bl_[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                ah[t] = row_read8(Xh, LD, (2 * wi + t) * 16, ks * 32, lane);
                al[t] = row_read8(Xl, LD, (2 * wi + t) * 16, ks * 32, lane);
                bh_[t] = row_read8(Yh, LD, (2 * wj + t) * 16, ks * 32, lane);
                bl_[t] = row_read8(Yl, LD, (2 * wj + t) * 16, ks * 32, lane);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = mfma_bf16(ah[i], bh_[j], acc[i][j]);
                    acc[i][j] = mfma_bf16(ah[i], bl_[j], acc[i][j]);
                    acc[i][j] = mfma_bf16(al[i], bh_[j], acc[i][j]);
                }
        }
        __syncthreads();
    }
    // C layout: rows i = 32 wi + 16 ti + 4 kg + r, column j = 32 wj + 16 tj + nl
    float* out = a.out + ((long)bh * a.nsplit + split) * M * M;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + 32 * wi + 16 * ti + 4 * kg + r, j = j0 + 32 * wj + 16 * tj + nl;
                if (i < M && j < M) out[(long)i * M + j] = acc[ti][tj][r];
            }
}

}  // namespace sp
}  // namespace mhla
