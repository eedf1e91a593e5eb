// Causal decode, paged pools: lift the state of chosen slots out of a pool into one contiguous buffer (the BLOB) and put it back,
// into other slots, other pages or another pool (mhla_causal_swap_out_paged / mhla_causal_swap_in_paged, mhla_hip.h).  Plain data
// movement: no arithmetic touches an element, an h16 page travels as payload and multipliers and is never decoded.
//
// The blob is a run of ITEMS, each on a 16-byte boundary, every item of a kind the same size (cs_swap_layout):
//   n_seqs sequence items   P [H][K][V] fp32 | Cur [H][K][V] fp32 | pos, full (int32) and 8 bytes of zeros
//   n_pages page items      fp32 pages: [H][K][V] fp32;  h16 pages: _Float16 [H][K][V] | float [H][K V / 64] | zeros up to 16 bytes
// `items` (device int32 [n_seqs + n_pages]) names the pool slot of every sequence item and the pool page of every page item.
// k_cs_swap<OUT, FMT>: grid (pieces, items), 256 threads, capped and grid-strided in both dimensions; a lane moves 16-byte pieces (an
// h16 payload as f16x8), four in flight; the multipliers of an h16 page, 1/32 of its payload's bytes, are the only 4-byte traffic.  A
// launch serves the items [i0, i1) and `blob` points at item i0, so that a caller may stage a blob in slices of whole items.  The
// entry of an item is workgroup-uniform and read through the constant address space, as cst_page reads the table; one outside
// 0 .. n_slots - 1 (n_pages - 1) forms no address: the item is skipped (defence only, the host layer produces none).  OUT writes
// every byte of its items, padding included; IN writes pos and full of a slot with ordinary vector stores by one lane, the first
// of the item's first workgroup -- no other workgroup of the launch touches them.
#pragma once
#include "causal_step.hpp"

namespace mhla {

struct CsSwapArgs {
    char* blob;             // where item i0 begins
    const int* items;       // [n_seqs + n_pages moved]: slot of a sequence item, pool page of a page item
    int i0, i1, n_seqs;
    char* pages;            // the pool's pages: fp32 [n_pages][H][K][V], or the h16 payload _Float16 [n_pages][H][K][V]
    float* mult;            // h16 pages: [n_pages][H][K V / 64]
    int n_pages;
    float *P, *Cur;         // [n_slots][H][K][V]
    int *pos, *full;        // [n_slots]; full may be null (OUT: reads as 0; IN: not written)
    int n_slots;
    long state_pieces;      // 16-byte pieces of one slot's P (= of its Cur): H K V / 4
    long pay_pieces;        // 16-byte pieces of one page's payload: H K V / 4 (fp32), H K V / 8 (h16)
    long n_mult, n_mult_pad;   // h16: multipliers of one page, H K V / 64, and that rounded up to a multiple of 4
    long seq_bytes, page_bytes;   // item sizes
};

// item sizes of the blob (host and device): the one statement of the layout
struct CsSwapLayout { long seq_bytes, page_bytes, state_pieces, pay_pieces, n_mult, n_mult_pad; };
__host__ __device__ inline CsSwapLayout cs_swap_layout(long H, long K, long V, int fmt) {
    CsSwapLayout l;
    const long E = H * K * V;
    l.state_pieces = E / 4;
    l.seq_bytes = 2 * E * 4 + 16;
    l.pay_pieces = fmt == PF_H16 ? E / CSH_EPL : E / 4;
    l.n_mult = fmt == PF_H16 ? E / CSH_GROUP : 0;
    l.n_mult_pad = (l.n_mult + 3) & ~3L;
    l.page_bytes = l.pay_pieces * 16 + l.n_mult_pad * 4;
    return l;
}

// pieces c, c + stride, ... below n of a run of 16-byte pieces, from src to dst: four requests in flight per lane
template <typename T>
__device__ __forceinline__ void cs_swap_run(char* dst, const char* src, long n, long c, long stride) {
    constexpr int U = 4;
    for (; c + (U - 1) * stride < n; c += U * stride) {
        T x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = gld<T>(src + (c + u * stride) * 16);
#pragma unroll
        for (int u = 0; u < U; ++u) gst<T>(dst + (c + u * stride) * 16, x[u]);
    }
    for (; c < n; c += stride) gst<T>(dst + c * 16, gld<T>(src + c * 16));
}

template <bool OUT, int FMT>
__global__ __launch_bounds__(256) void k_cs_swap(const CsSwapArgs a) {
    using PT = std::conditional_t<FMT == PF_H16, f16x8, f32x4>;   // a 16-byte piece of a page's payload
    const long c0 = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    const long first = a.i0 < a.n_seqs ? (long)a.i0 * a.seq_bytes : (long)a.n_seqs * a.seq_bytes + (long)(a.i0 - a.n_seqs) * a.page_bytes;
    for (int i = a.i0 + (int)blockIdx.y; i < a.i1; i += (int)gridDim.y) {
        const int e = *(const __attribute__((address_space(4))) int*)(a.items + i);
        if (i < a.n_seqs) {
            if ((unsigned)e >= (unsigned)a.n_slots) continue;
            char* item = a.blob + ((long)i * a.seq_bytes - first);
            char* p = (char*)a.P + (long)e * a.state_pieces * 16;
            char* cur = (char*)a.Cur + (long)e * a.state_pieces * 16;
            char* tail = item + 2 * a.state_pieces * 16;
            if constexpr (OUT) {
                cs_swap_run<f32x4>(item, p, a.state_pieces, c0, stride);
                cs_swap_run<f32x4>(item + a.state_pieces * 16, cur, a.state_pieces, c0, stride);
                if (c0 == 0) {
                    typedef int i32x4 __attribute__((ext_vector_type(4)));
                    gst<i32x4>(tail, i32x4{gld<int>(a.pos + e), a.full ? gld<int>(a.full + e) : 0, 0, 0});
                }
            } else {
                cs_swap_run<f32x4>(p, item, a.state_pieces, c0, stride);
                cs_swap_run<f32x4>(cur, item + a.state_pieces * 16, a.state_pieces, c0, stride);
                if (c0 == 0) {
                    gst<int>(a.pos + e, gld<int>(tail));
                    if (a.full) gst<int>(a.full + e, gld<int>(tail + 4));
                }
            }
        } else {
            if ((unsigned)e >= (unsigned)a.n_pages) continue;
            char* item = a.blob + ((long)a.n_seqs * a.seq_bytes + (long)(i - a.n_seqs) * a.page_bytes - first);
            char* pay = a.pages + (long)e * a.pay_pieces * 16;
            if constexpr (OUT) cs_swap_run<PT>(item, pay, a.pay_pieces, c0, stride);
            else cs_swap_run<PT>(pay, item, a.pay_pieces, c0, stride);
            if constexpr (FMT == PF_H16) {
                float* m = a.mult + (long)e * a.n_mult;
                char* bm = item + a.pay_pieces * 16;
                if constexpr (OUT) {
                    for (long c = c0; c < a.n_mult_pad; c += stride) gst<float>(bm + c * 4, c < a.n_mult ? gld<float>(m + c) : 0.f);
                } else {
                    for (long c = c0; c < a.n_mult; c += stride) gst<float>(m + c, gld<float>(bm + c * 4));
                }
            }
        }
    }
}

}  // namespace mhla
