// Causal chunk-mixing MHLA, decoding: T >= 1 new tokens on an existing decode state in a number of launches that does not
// depend on T (mhla_causal_extend; the state and the single-token step: causal_step.hpp).
//
// With `pos` tokens seen, i = pos / 64, r = pos % 64, the new tokens fall into segments that never cross a chunk boundary: the
// first has a = min(T, 64 - r) rows of the open chunk i, then whole chunks, then a tail.  For a segment in chunk c (<= 64 rows):
//   O   = scale (Q (P_c + m_cc Cur_before) + m_cc tril(Q K^T) V)          tril over the segment's own rows
//   Cur = Cur_before + K^T V ;  chunk full: S[c] = Cur, Cur = 0, P_{c+1} = sum_{j<=c} mix[c+1][j] S[j]
// Cur_before is the state's Cur for the first segment and zero afterwards; P_c of a later chunk depends on finished chunks only,
// so every K^T V of the extension is formed before any prefix mix:
//   k_cx_out     : O of the first segment from the state's P and Cur (P + m_ii Cur formed on the load)
//   k_cx_xty_acc : Cur (or S[i], when the chunk closes) = Cur + K^T V of the first segment
//   k_bm_state<2>: K^T V of the later whole chunks -> S[i+1 ...], of the tail -> Cur            (blockmix.hpp, as the prefill state)
//   k_cx_mix     : P_c of every later chunk the extension touches -> workspace, the open one's -> the state's P
//   k_cx_out     : O of all later segments, the segment as a grid dimension
//   k_cs_step_finish over the token rows (fp32 rows staged by k_cx_out): scale, norm x gate, ONE rounding
// Every product is an exact fp32 MFMA tile product with fp32 accumulation (k_cs_out's machinery), never the 11-bit stored
// summaries: the rows are of the same grade as the step's.  No atomics, every sum in a fixed order.
#pragma once
#include "causal.hpp"
#include "causal_step.hpp"

namespace mhla {

struct CxOutArgs {
    View q, k, v;          // [B][T][H][K / V]: the extension's tokens
    MView o;               // [B][T][H][V] rows, rounded once; ptr null: fp32 rows to `stage` instead
    float* stage;          // [bh][T][V] fp32, NOT scaled (k_cs_step_finish scales, normalises and rounds)
    const float* P;        // prefix mix of this launch's segment 0
    long p_bh, p_seg;      // floats from one (b, h) / one segment to the next
    const float* Cur;      // [bh][K][V] the open chunk's K^T V before the segment (first segment), or null: zero
    const float* mdiag;    // &mix[c][c] of segment 0's chunk
    long mstep;            // ldmix + 1
    long tok0, tend;       // segment s: tokens tok0 + 64 s .. min(tok0 + 64 s + 64, tend)
    int H, K, V;
    long T;
    float scale;
};

// [64 kk][64 cols] slice of P + mii Cur (Cur null: P alone) -> LDS, zero padded; V % 4 == 0
__device__ __forceinline__ void cx_load_pc(float* __restrict__ dst, int ld, const float* __restrict__ P, const float* __restrict__ Cur,
                                           float mii, long src_ld, int rows_valid, int cols_valid, int tid) {
    constexpr int CV = 16, U = 4;
    for (int v0 = tid; v0 < 64 * CV; v0 += NTHREADS * U) {
        f32x4 x[U], c[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int v = v0 + u * NTHREADS, r = v / CV, cc = (v - r * CV) * 4;
            x[u] = c[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (r < rows_valid && cc < cols_valid) {
                x[u] = gld<f32x4>(P + (long)r * src_ld + cc);
                if (Cur) c[u] = gld<f32x4>(Cur + (long)r * src_ld + cc);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int v = v0 + u * NTHREADS, r = v / CV, cc = (v - r * CV) * 4;
            if (Cur) {
#pragma unroll
                for (int t = 0; t < 4; ++t) x[u][t] = fmaf(mii, c[u][t], x[u][t]);
            }
            *reinterpret_cast<f32x4*>(dst + r * ld + cc) = x[u];
        }
    }
}

// grid (segments, B H, ceil(V / 64)): k_cs_out on a run of <= 64 token rows of one chunk
template <typename T>
__global__ __launch_bounds__(NTHREADS) void k_cx_out(const CxOutArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Qs = smem;                  // [64 c][66]
    float* Ks = Qs + CS * CS_LDX;      // [64 c'][66]
    float* As = Ks + CS * CS_LDX;      // [64 c][66]
    float* Ps = As + CS * CS_LDX;      // [64 kk][80]  P slice, later V slice [64 c][80]
    float* Os = Ps + CS * CS_LDK;      // [64][68]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
    const int seg = blockIdx.x, bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
    const int v0 = blockIdx.z * 64, vv = min(64, a.V - v0);
    const long p0 = a.tok0 + (long)seg * CS;
    const int rv = (int)min((long)CS, a.tend - p0);
    const T* qb = (const T*)a.q.ptr + b * a.q.sb + h * a.q.sh;
    const T* kb = (const T*)a.k.ptr + b * a.k.sb + h * a.k.sh;
    const T* vb = (const T*)a.v.ptr + b * a.v.sb + h * a.v.sh;
    const float* Pi = a.P + (long)bh * a.p_bh + (long)seg * a.p_seg;
    const float* Ci = a.Cur ? a.Cur + (long)bh * a.K * a.V : nullptr;
    const float mii = a.mdiag[(long)seg * a.mstep];

    f32x4 accO[4], accA[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) accO[i] = accA[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ks = 0; ks < a.K; ks += 64) {
        const int kv = min(64, a.K - ks);
        load_tile<T, 64, false>(Qs, CS_LDX, qb + ks, a.q.sn, nullptr, p0, rv, CS, kv, 0.f, tid, NTHREADS);
        load_tile<T, 64, false>(Ks, CS_LDX, kb + ks, a.k.sn, nullptr, p0, rv, CS, kv, 0.f, tid, NTHREADS);
        cx_load_pc(Ps, CS_LDK, Pi + (long)ks * a.V + v0, Ci ? Ci + (long)ks * a.V + v0 : nullptr, mii, a.V, kv, vv, tid);
        __syncthreads();
        ab_accum<4, 4, true>(accA, Qs, CS_LDX, Ks, CS_LDX, 16, 64, wave, lane);
        ab_accum<4, 4, false>(accO, Qs, CS_LDX, Ps, CS_LDK, 16, 64, wave, lane);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = wave + 4 * i, tm = t >> 2, tn = t & 3, col = tn * 16 + r16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = tm * 16 + kq * 4 + r;
            As[row * CS_LDX + col] = col <= row ? mii * accA[i][r] : 0.f;
        }
    }
    load_tile<T, 64, false>(Ps, CS_LDK, vb + v0, a.v.sn, nullptr, p0, rv, CS, vv, 0.f, tid, NTHREADS);
    __syncthreads();
    ab_accum<4, 4, false>(accO, As, CS_LDX, Ps, CS_LDK, 16, 64, wave, lane);
    const float sc = a.o.ptr ? a.scale : 1.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = wave + 4 * i, tm = t >> 2, tn = t & 3, col = tn * 16 + r16;
#pragma unroll
        for (int r = 0; r < 4; ++r) Os[(tm * 16 + kq * 4 + r) * CS_LDO + col] = sc * accO[i][r];
    }
    __syncthreads();
    if (a.o.ptr) {
        T* ob = (T*)a.o.ptr + b * a.o.sb + h * a.o.sh;
        store_tile<T, 64>(ob + v0, a.o.sn, nullptr, p0, Os, CS_LDO, rv, vv, tid, NTHREADS);
    } else {
        float* sb = a.stage + ((long)bh * a.T + p0) * a.V + v0;
        for (int v = tid; v < rv * 16; v += NTHREADS) {
            const int r = v >> 4, c = (v & 15) * 4;
            if (c < vv) gst<f32x4>(sb + (long)r * a.V + c, *reinterpret_cast<const f32x4*>(Os + r * CS_LDO + c));
        }
    }
}

struct CxAccArgs {
    View x, y;             // k, v: [B][T][H][K / V]; rows 0 .. rows - 1 are the segment
    const float* src;      // [bh][K][V] Cur before the segment
    float* dst;            // Cur, or S[i] when the segment closes the chunk
    long dst_bh;           // floats from one (b, h) to the next in dst
    int H, rows, DX, DY;
};

// grid (1, B H, strips of 64 x 64): dst = src + X^T Y over the segment's rows -- the accumulating form of k_bm_state<MODE 2>
template <typename T>
__global__ __launch_bounds__(NTHREADS) void k_cx_xty_acc(const CxAccArgs a) {
    constexpr int LD = ld_kmajor(64);
    __shared__ __attribute__((aligned(16))) float Xs[CS * LD];
    __shared__ __attribute__((aligned(16))) float Ys[CS * LD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
    const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
    const int nsy = (a.DY + 63) / 64;
    const int x0 = (blockIdx.z / nsy) * 64, y0 = (blockIdx.z % nsy) * 64;
    const T* xb = (const T*)a.x.ptr + b * a.x.sb + h * a.x.sh;
    const T* yb = (const T*)a.y.ptr + b * a.y.sb + h * a.y.sh;
    const int kend = (a.rows + 3) & ~3;
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    load_tile<T, 64, false>(Xs, LD, xb + x0, a.x.sn, nullptr, 0, a.rows, kend, a.DX - x0, 0.f, tid, NTHREADS);
    load_tile<T, 64, false>(Ys, LD, yb + y0, a.y.sn, nullptr, 0, a.rows, kend, a.DY - y0, 0.f, tid, NTHREADS);
    __syncthreads();
    xty_accum<4, 4>(acc, Xs, Ys, LD, kend, wave, lane);
    const float* sb = a.src + (long)bh * a.DX * a.DY;
    float* db = a.dst + (long)bh * a.dst_bh;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = wave + 4 * i, tm = t >> 2, tn = t & 3;
        const int col = y0 + tn * 16 + r16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = x0 + tm * 16 + kq * 4 + r;
            if (row < a.DX && col < a.DY) db[(long)row * a.DY + col] = sb[(long)row * a.DY + col] + acc[i][r];
        }
    }
}

constexpr int CX_MIX_NC = 8;   // chunks per workgroup of k_cx_mix: S[j] is read once for all of them

struct CxMixArgs {
    const float* S;        // [bh][cap][K][V]; chunks below the largest c formed are finished
    float* ws;             // [bh][nws][K][V]: P_c of chunk c0 + u, u < nws
    float* P;              // [bh][K][V] the state's
    const float* mix;
    long E;                // K V
    int ldmix, cap, c0, nws, nc;
    int cP;                // chunk whose prefix mix is the state's P (c0 <= cP < c0 + nc), or -1: the state is full, P = 0
};

// grid (ceil(E / 4 / 64), B H, ceil(nc / 8)), one wave per workgroup: P_c = sum_{j < c} mix[c][j] S[j], ascending j (k_cs_roll's sum)
__global__ __launch_bounds__(64) void k_cx_mix(const CxMixArgs a) {
    const long e = ((long)blockIdx.x * 64 + threadIdx.x) * 4;
    if (e >= a.E) return;   // (E % 4 == 0)
    const long bh = blockIdx.y;
    const float* Sb = a.S + bh * a.cap * a.E + e;
    const int u0 = blockIdx.z * CX_MIX_NC, nu = min(CX_MIX_NC, a.nc - u0);
    f32x4 acc[CX_MIX_NC];
#pragma unroll
    for (int u = 0; u < CX_MIX_NC; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int cbase = a.c0 + u0, jend = nu > 0 ? cbase + nu - 1 : 0;   // the last chunk of the group sums j < jend
    // j < cbase: a term of every chunk of the group (eight tiles in flight, no per-chunk test); cbase <= j < jend: of the chunks behind j
    constexpr int U = 8;
    const int jall = nu > 0 ? cbase : 0;
    int j0 = 0;
    for (; j0 + U <= jall; j0 += U) {
        f32x4 s[U];
#pragma unroll
        for (int w = 0; w < U; ++w) s[w] = gld<f32x4>(Sb + (long)(j0 + w) * a.E);
#pragma unroll
        for (int u = 0; u < CX_MIX_NC; ++u) {
            if (u < nu) {
                const float* mr = a.mix + (long)(cbase + u) * a.ldmix + j0;
#pragma unroll
                for (int w = 0; w < U; ++w) {
                    const float m = mr[w];
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[u][t] = fmaf(m, s[w][t], acc[u][t]);
                }
            }
        }
    }
    for (int j = j0; j < jend; ++j) {
        const f32x4 s = gld<f32x4>(Sb + (long)j * a.E);
#pragma unroll
        for (int u = 0; u < CX_MIX_NC; ++u) {
            if (u < nu && j < cbase + u) {
                const float m = a.mix[(long)(cbase + u) * a.ldmix + j];
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[u][t] = fmaf(m, s[t], acc[u][t]);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < CX_MIX_NC; ++u) {
        if (u < nu) {
            if (u0 + u < a.nws) gst<f32x4>(a.ws + (bh * a.nws + u0 + u) * a.E + e, acc[u]);
            if (cbase + u == a.cP) gst<f32x4>(a.P + bh * a.E + e, acc[u]);
        }
    }
    if (a.cP < 0 && blockIdx.z == 0) gst<f32x4>(a.P + bh * a.E + e, f32x4{0.f, 0.f, 0.f, 0.f});
}

}  // namespace mhla
