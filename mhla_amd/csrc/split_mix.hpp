// Block-mix split kernels (split.hpp): k_sp_mix, the tiled mixing of block summaries.
#pragma once
#include "split_operands.hpp"

namespace mhla {
namespace sp {

// -------------------------------------------------------------------------------------------------
constexpr int SPM_TE = 128, SPM_LD = SPM_TE + 8, SPM_TILE = 32 * SPM_LD;
constexpr int SP_MIX_SMEM = 4 * SPM_TILE * 2;   // two buffers of (hi, lo) [32][SPM_LD] bf16; reused as [64][SPM_TE + 4] fp32 staging
static_assert(64 * (SPM_TE + 4) * 4 <= SP_MIX_SMEM, "output staging must fit in the input tiles");
// bf16 summaries: no lo tiles and a bf16 output staging [64][SPM_LD]: half the LDS, twice the resident workgroups
constexpr int SP_MIX_SMEM16 = 2 * SPM_TILE * 2;
static_assert(64 * SPM_LD * 2 <= SP_MIX_SMEM16, "bf16 output staging must fit in the input tiles");
template <int FMT> constexpr int sp_mix_smem() { return FMT == SF_BF16 ? SP_MIX_SMEM16 : SP_MIX_SMEM; }

template <int TRANS, int FMT>   // FMT: fp32 words, or SF_BF16 (no lo part)
__global__ __launch_bounds__(NTHREADS, 2) void k_sp_mix(const MixArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u16* Xs = reinterpret_cast<u16*>(smem_raw);
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nl = lane & 15, kg = lane >> 4;
    const long e0 = (long)blockIdx.x * SPM_TE;
    const int i0 = blockIdx.y * 64, bh = blockIdx.z, M = a.M;
    const float* inb = a.in + (long)bh * M * a.es + e0;
    float* outb = a.out + (long)bh * M * a.es + e0;
    const u16* inb16 = reinterpret_cast<const u16*>(a.in) + (long)bh * M * a.es + e0;
    u16* outb16 = reinterpret_cast<u16*>(a.out) + (long)bh * M * a.es + e0;
    const int steps = (M + 31) / 32;
    const int sr = tid >> 3, sc = (tid & 7) * 8;   // staging: row sr, 8 floats at columns sc and sc + 64

    f32x4 pre[2][2];
    uint4 pre16[2];
    auto fetch = [&](int step) {
        const int row = step * 32 + sr;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            pre[u][0] = pre[u][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            pre16[u] = make_uint4(0, 0, 0, 0);
        }
        if (row < M) {
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (e0 + sc + 64 * u < a.E) {   // E is a multiple of 8
                    if (FMT == SF_BF16) {
                        pre16[u] = *reinterpret_cast<const uint4*>(inb16 + (long)row * a.es + sc + 64 * u);
                    } else {
                        const float* src = inb + (long)row * a.es + sc;
                        pre[u][0] = *reinterpret_cast<const f32x4*>(src + 64 * u);
                        pre[u][1] = *reinterpret_cast<const f32x4*>(src + 64 * u + 4);
                    }
                }
        }
    };
    auto commit = [&](int buf) {
        u16* th = Xs + buf * (sf_has_lo(FMT) ? 2 : 1) * SPM_TILE + sr * SPM_LD + sc;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (FMT == SF_BF16) {
                *reinterpret_cast<uint4*>(th + 64 * u) = pre16[u];
            } else {
                uint4 hi, lo;
                split8(pre[u][0], pre[u][1], hi, lo);
                *reinterpret_cast<uint4*>(th + 64 * u) = hi;
                *reinterpret_cast<uint4*>(th + SPM_TILE + 64 * u) = lo;
            }
        }
    };

    f32x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int orow = i0 + wave * 16 + nl;

    // this lane's 8 mixing weights of a step (row orow, columns step * 32 + kg * 8 ..): fetched one step ahead like the tiles,
    // so their L2 latency is not on the MFMA chain
    float wc[8], wn[8];
    const bool wvec = !TRANS && (reinterpret_cast<uintptr_t>(a.W) & 15) == 0 && (a.ldw & 3) == 0;
    const bool wvec2 = !TRANS && (reinterpret_cast<uintptr_t>(a.W) & 7) == 0 && (a.ldw & 1) == 0;
    auto fetch_w = [&](int step, float (&w)[8]) {
        const int k0 = step * 32 + kg * 8;
        if (wvec && orow < M && k0 + 8 <= M) {   // 8 consecutive weights of one row: two 16-byte loads
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(a.W + (long)orow * a.ldw + k0);
            const f32x4 w1 = *reinterpret_cast<const f32x4*>(a.W + (long)orow * a.ldw + k0 + 4);
#pragma unroll
            for (int t = 0; t < 4; ++t) { w[t] = w0[t]; w[4 + t] = w1[t]; }
            return;
        }
        if (wvec2 && orow < M && k0 + 8 <= M) {  // even row stride (M = 150): four 8-byte loads
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float2 wp = *reinterpret_cast<const float2*>(a.W + (long)orow * a.ldw + k0 + 2 * t);
                w[2 * t] = wp.x; w[2 * t + 1] = wp.y;
            }
            return;
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int kk = k0 + t;
            w[t] = (orow < M && kk < M) ? (TRANS ? a.W[(long)kk * a.ldw + orow] : a.W[(long)orow * a.ldw + kk]) : 0.f;
        }
    };
    fetch(0);
    fetch_w(0, wc);
    commit(0);
    for (int step = 0; step < steps; ++step) {
        const int buf = step & 1;
        __syncthreads();
        if (step + 1 < steps) {
            fetch(step + 1);
            fetch_w(step + 1, wn);
        }
        bf16x8 ah, al;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const __bf16 hi = (__bf16)wc[t];
            ah[t] = hi;
            al[t] = (__bf16)(wc[t] - (float)hi);
        }
        const u16* th = Xs + buf * (sf_has_lo(FMT) ? 2 : 1) * SPM_TILE;
#pragma unroll
        for (int t4 = 0; t4 < 8; t4 += 4) {
            bf16x8 bh_[4], bl_[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                bh_[t] = tr_read8(th, SPM_LD, 0, (t4 + t) * 16, lane);
                if (sf_has_lo(FMT)) bl_[t] = tr_read8(th + SPM_TILE, SPM_LD, 0, (t4 + t) * 16, lane);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t4 + t] = mfma_bf16(ah, bh_[t], acc[t4 + t]);
            if (sf_has_lo(FMT))
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t4 + t] = mfma_bf16(ah, bl_[t], acc[t4 + t]);
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t4 + t] = mfma_bf16(al, bh_[t], acc[t4 + t]);
        }
        if (step + 1 < steps) {
            commit(buf ^ 1);
#pragma unroll
            for (int t = 0; t < 8; ++t) wc[t] = wn[t];
        }
    }
    __syncthreads();
    if constexpr (FMT == SF_BF16) {
        u16* Os = Xs;   // [64][SPM_LD] bf16
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) Os[(wave * 16 + kg * 4 + r) * SPM_LD + t * 16 + nl] = cvt_bf16(acc[t][r]);
        __syncthreads();
#pragma unroll
        for (int v0 = 0; v0 < 4; ++v0) {
            const int v = tid + v0 * NTHREADS, r = v >> 4, c = (v & 15) * 8;
            if (i0 + r < M && e0 + c < a.E)   // E is a multiple of 8
                *reinterpret_cast<uint4*>(outb16 + (long)(i0 + r) * a.es + c) = *reinterpret_cast<const uint4*>(Os + r * SPM_LD + c);
        }
    } else {
        float* Os = reinterpret_cast<float*>(smem_raw);   // [64][SPM_TE + 4]
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) Os[(wave * 16 + kg * 4 + r) * (SPM_TE + 4) + t * 16 + nl] = acc[t][r];
        __syncthreads();
#pragma unroll
        for (int v0 = 0; v0 < 8; ++v0) {
            const int v = tid + v0 * NTHREADS, r = v >> 5, c = (v & 31) * 4;
            if (i0 + r < M && e0 + c < a.E)
                *reinterpret_cast<f32x4*>(outb + (long)(i0 + r) * a.es + c) = *reinterpret_cast<const f32x4*>(Os + r * (SPM_TE + 4) + c);
        }
    }
}

}  // namespace sp
}  // namespace mhla
