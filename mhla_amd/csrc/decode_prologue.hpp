// q / k prologue of a decode call's NEW tokens at positions read from the decode state (mhla_featmap_rotary_decode): feature map, then
// the NeoX rotary at table row p = pos[sb] + r of every token row -- r the row's index inside its sequence's window, sb the state row
// of its sequence (b, or slot[b] of a slotted call: cst_slot, causal_step.hpp).  q and k of the call in ONE launch; no host value that
// depends on a position, so a captured graph replays it; pos is read, never written (the call goes ahead of the chain that advances it).
// Token layouts as in the extend chain (CxRag / cx_seq, causal_extend.hpp): padded [B][T] with the window [0, w) or, left-padded,
// [T - w, T), w = ntok[b] (null: T); or PACKED, one run of T rows with sequence b's the rows [off[b], off[b + 1]) -- the binary search
// of k_cs_step_finish<.., PACKED>.  The arithmetic is k_fmap_rotary's (fmrot_*, common.hpp; rounded by the same Io<T> stores): the bits
// of that kernel on table rows gathered at the same positions.  Every other row -- outside every window, of an inactive slot entry, of
// a sequence whose offsets decrease or leave [0, T) or whose count leaves 0 .. T, or with p outside the tables -- is written as zeros.
// Nothing read from the device arrays forms an address: b < B indexes ntok / off / slot, a slot passes cst_slot's range test before it
// indexes pos, and p passes 0 <= p < tab_rows before it indexes the tables.
// grid (token rows), 256 threads: the row's sequence, slot and position once per workgroup (uniform loads), then the threads walk the
// (H + Hkv) K / (2 W) pieces of the row, W + W elements each (x[i .. i + W) and its partners x[i + K/2 ..)).  W = 4 is k_fmap_rotary's
// piece; W = 8 (16-bit tensors whose rows allow 16-byte pieces: the host decides) halves the requests -- 8-byte requests run at
// 0.54-0.70x the rate of 16-byte ones on this memory system -- and computes every element as W = 4 does: the same bits.
// yq may be q and yk may be k: a thread reads its 2 W elements before it writes them, and no other thread touches them.
#pragma once
#include "common.hpp"

namespace mhla {

struct FrDecArgs {
    View q, k;             // [B][T][H][K], [B][T][Hkv][K]; PACKED: one run of T rows, sb unused
    MView yq, yk;
    const void* cos;       // [tab_rows][ldt], tensor dtype, K / 2 columns read
    const void* sin;
    long ldt;
    long tab_rows;
    const int* pos;        // [B], or the pool's [n_slots] with a slot map
    const int* slot;       // [B] or null
    int n_slots;
    const int* ntok;       // [B] or null: all T rows (padded only)
    const int* off;        // PACKED: [B + 1]
    int T, left;
    int B, H, Hkv, K, fmap;
};

// W elements of a row of T: 4 through Io<T> (8 bytes of a 16-bit type, 16 of fp32), 8 (16-bit types) as ONE 16-byte piece whose halves
// go through the same Io<T> conversions
template <typename T, int W> struct FrIo;
template <typename T> struct FrIo<T, 4> {
    static __device__ __forceinline__ void ld(const T* p, f32x4 (&x)[1]) { x[0] = Io<T>::ld4(p); }
    static __device__ __forceinline__ void st(T* p, const f32x4 (&x)[1]) { Io<T>::st4(p, x[0]); }
    static __device__ __forceinline__ void zero(T* p) { Io<T>::st4(p, f32x4{0.f, 0.f, 0.f, 0.f}); }
};
template <typename T> struct FrIo<T, 8> {
    static_assert(sizeof(T) == 2, "8-element pieces are for 16-bit tensors");
    static __device__ __forceinline__ void ld(const T* p, f32x4 (&x)[2]) {
        union { uint4 raw; T e[8]; } u;
        u.raw = *reinterpret_cast<const uint4*>(p);
        x[0] = Io<T>::ld4(u.e);
        x[1] = Io<T>::ld4(u.e + 4);
    }
    static __device__ __forceinline__ void st(T* p, const f32x4 (&x)[2]) {
        union { uint4 raw; T e[8]; } u;
        Io<T>::st4(u.e, x[0]);
        Io<T>::st4(u.e + 4, x[1]);
        *reinterpret_cast<uint4*>(p) = u.raw;
    }
    static __device__ __forceinline__ void zero(T* p) { *reinterpret_cast<uint4*>(p) = make_uint4(0u, 0u, 0u, 0u); }
};

template <typename T, int W, bool PACKED>
__global__ __launch_bounds__(256) void k_fr_decode(const FrDecArgs a) {
    constexpr int NV = W / 4;
    const long row = blockIdx.x;
    // ---- the row's sequence b, its index r inside the window, whether it is inside one (workgroup-uniform)
    int b, r;
    long tok;              // the row inside its batch row of the views
    bool live;
    if constexpr (PACKED) {
        const auto off_at = [&](int i) { return *(const __attribute__((address_space(4))) int*)(a.off + i); };
        int lo = 0, hi = a.B;   // the last b with off[b] <= row: empty sequences before it share its offset
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (off_at(mid) <= (int)row) lo = mid;
            else hi = mid;
        }
        b = lo;
        const int first = off_at(b), end = off_at(b + 1);
        live = first >= 0 && end <= a.T && (int)row >= first && (int)row < end;   // (offsets that decrease: end <= first, no row)
        r = (int)row - first;
        tok = row;
    } else {
        b = (int)(row / a.T);
        tok = row - (long)b * a.T;
        const int w = a.ntok ? a.ntok[b] : a.T;
        const int t0 = a.left ? a.T - w : 0;
        live = w >= 0 && w <= a.T && tok >= t0 && tok < (long)t0 + w;
        r = (int)tok - t0;
    }
    long p = -1;
    if (live) {
        // cst_slot's test (causal_step.hpp, whose non-template kernels live in another translation unit): an entry outside the pool is inactive
        const int sb = a.slot ? a.slot[b] : b;
        if (!a.slot || (unsigned)sb < (unsigned)a.n_slots) p = (long)a.pos[sb] + r;
    }
    live = p >= 0 && p < a.tab_rows;
    const long vb = PACKED ? 0 : b;
    const int half = a.K / 2, G = half / W, nq = a.H * G, total = nq + a.Hkv * G;
    const T* cosr = (const T*)a.cos + (live ? p : 0) * a.ldt;
    const T* sinr = (const T*)a.sin + (live ? p : 0) * a.ldt;
    for (int e = threadIdx.x; e < total; e += 256) {
        const bool isq = e < nq;
        const int eh = isq ? e : e - nq, h = eh / G, i = (eh - h * G) * W;
        const View& x = isq ? a.q : a.k;
        const MView& y = isq ? a.yq : a.yk;
        T* yp = (T*)y.ptr + vb * y.sb + tok * y.sn + h * y.sh + i;
        if (!live) {
            FrIo<T, W>::zero(yp);
            FrIo<T, W>::zero(yp + half);
            continue;
        }
        const T* xp = (const T*)x.ptr + vb * x.sb + tok * x.sn + h * x.sh + i;
        f32x4 x0[NV], x1[NV], c[NV], s[NV], y0[NV], y1[NV];
        FrIo<T, W>::ld(xp, x0);
        FrIo<T, W>::ld(xp + half, x1);
        FrIo<T, W>::ld(cosr + i, c);
        FrIo<T, W>::ld(sinr + i, s);
#pragma unroll
        for (int n = 0; n < NV; ++n)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float f0 = fmrot_map(x0[n][u], a.fmap), f1 = fmrot_map(x1[n][u], a.fmap);
                y0[n][u] = fmrot_lo(f0, f1, c[n][u], s[n][u]);
                y1[n][u] = fmrot_hi(f0, f1, c[n][u], s[n][u]);
            }
        FrIo<T, W>::st(yp, y0);
        FrIo<T, W>::st(yp + half, y1);
    }
}

}  // namespace mhla
