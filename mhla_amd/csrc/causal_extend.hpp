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
// Ragged extend (RAGGED; mhla_causal_extend_ragged): ONE chain for a batch whose sequence b takes ntok[b] tokens (0 .. T) at its
// own position pos[b], the tokens padded to [B][T][...] (rows [0, n), or [T - n, T) left-padded).  Every (b, h) workgroup reads
// pos[b] and ntok[b] (device int32 [B]) and derives the plan the host derives above (cx_seq): i, r, the first segment's rows a, the
// chunks touched after the first, whether the first segment closes chunk i, whether the state is full afterwards.  The later
// segments are a grid dimension sized by the batch maximum the host vouches for; a workgroup whose sequence has no such segment
// (or no token at all) returns after those two loads, before any LDS or other global traffic.  Six launches, whatever B, ntok, pos:
//   k_cx_out<.ragged>    first segment (also: nval[b] = the tokens the chain accepts for b, which the finish reads instead of pos)
//   k_cx_xty_acc<.ragged> first segment: Cur, or S[i_b] where that sequence's chunk closes
//   k_cx_xty_acc<.ragged> later segments (src null): whole chunks -> S[i_b + 1 + s], the tail -> Cur, no tail -> Cur = 0.  A launch
//                        of its own: the one before READS Cur, this one WRITES it
//   k_cx_mix_ragged      c0 = i_b + 1, nc and cP per sequence; workspace stride = the batch maximum of later chunks
//   k_cx_out<.ragged>    later segments, P from the workspace
//   k_cs_step_finish<.win> every row of [B][T]: rows of the window from the staged fp32 rows, rows outside it written as ZEROS;
//                        pos[b] += nval[b] -- the last launch, the only one that does not address by pos
// (the middle three only when the host says some sequence closes a chunk).  Tiling and the order of every sum are the uniform
// chain's, so a sequence gets the bits mhla_causal_extend gives it alone in a batch of one; a sequence with ONE token gets the
// step's arithmetic (k_cs_step's row walk and K split of a batch of one, fmaf for fmaf), as T = 1 of the uniform call is the step.
// Defence only: a sequence whose pos / ntok fall outside what the host vouched for is skipped (state untouched, rows zeros).
// Verify (CxRag::dry; mhla_causal_verify_ragged): the same six launches, tiles and sums, minus every write to the committed state --
// Cur, P and pos.  S[i_b] and S[i_b + 1 ...] are still written: those rows are unfinished at pos[b], nothing reads them before a later
// call finishes them, and the later segments' prefix mixes are formed from them.  The rows are the ragged extend's, bit for bit.
// Commit (CxRag::acc; mhla_causal_commit_ragged): the state half of the chain alone, on the first min(acc[b], ntok[b]) tokens of each
// window (the window still placed by ntok[b]), no q and no output -- at most four launches:
//   k_cx_xty_acc<.ragged> first segment (also nval[b]), k_cx_xty_acc<.ragged> later segments, k_cx_mix_ragged with no workspace (only
//   the P of the chunk open afterwards is formed), k_cx_advance: pos[b] += nval[b] -- the last, the only one not addressing by pos
// (the middle two only when some sequence closes a chunk).  The same tiles and sums again: the state is the one the ragged extend
// leaves after acc[b] tokens, bit for bit; one accepted token takes the step's fmaf.
// Packed new tokens (CxRag::off; mhla_causal_{extend,verify,commit}_packed): the tokens of all sequences are ONE run of T rows and
// sequence b's are [off[b], off[b + 1]) -- the three chains above with the token views' batch stride 0, w = off[b + 1] - off[b] where
// cx_seq reads ntok[b] and shift = off[b]; the fp32 rows are staged [h][T][V] and the finish is k_cs_step_finish<.win, .packed> over
// (H, T), which finds each row's sequence by a binary search over off.  The tiles, the K split and the order of every sum are the
// padded chain's: the same bits per sequence.  Defence only: offsets that decrease or leave [0, T) skip the sequence.  PACKED is a
// template parameter of cx_seq and (CxVar::packed) of the three k_cx_* kernels that call it, so that the padded instantiations are the code they were.
#pragma once
#include "causal.hpp"
#include "causal_step.hpp"

namespace mhla {

// the variants of k_cx_out, k_cx_xty_acc and k_cx_mix_ragged, named at the launch site: CxVar{.ragged = true, .packed = true}
struct CxVar {
    bool ragged = false, packed = false;
    constexpr bool operator==(const CxVar&) const = default;
    constexpr bool valid() const { return !packed || ragged; }   // a pack runs the ragged chain
};

// RAGGED: what every kernel of the ragged chain derives its sequence's plan from
struct CxRag {
    const int* pos;        // [B] tokens seen per sequence
    const int* ntok;       // [B] new tokens per sequence, 0 .. T
    int T, cap;            // padded width; chunks the state holds
    int max_end;           // host-vouched: the largest pos[b] + ntok[b] over sequences with tokens (<= 64 cap)
    int max_later;         // host-vouched: the largest number of chunks touched after the first
    int any_close;         // host-vouched: some sequence closes a chunk (the later-segment launches exist)
    int left;              // left-padded: sequence b's tokens are rows [T - n, T)
    int dry;               // verify: Cur, P and pos are not written (S rows at and beyond pos[b] / 64 still are)
    const int* acc;        // [B] or null; commit: sequence b takes the first min(acc[b], ntok[b]) tokens of its ntok[b]-token window
    // slotted calls (cst_slot, causal_step.hpp): pos is the pool's [n_slots] and call row b reads pos[slot[b]]; ntok and acc stay the call's
    const int* slot;       // [B] or null
    int n_slots;
    // paged pools (cst_page, causal_step.hpp): S is a pool of pages and chunk j of state row sb lives in page table[sb cap + j]
    const int* table;      // [n_slots][cap] or null: S is dense
    int n_pages;
    // packed new tokens (the mhla_causal_*_packed entry points): the tokens of all sequences are ONE run of T rows, sequence b's the rows
    // [off[b], off[b + 1]) -- the token views come with sb = 0, ntok is unused and left is 0
    const int* off;        // [B + 1] (the kernels' PACKED instantiations read it), or null: padded, [B][T]
};
struct CxSeq {
    int n, i, r, a;        // tokens; chunk and fill of the open chunk; rows of the first segment
    int later;             // chunks touched after the first
    int iend;              // chunk open after the extension
    int shift;             // first token row inside [0, T): of the sequence's padded rows, or -- packed -- of the pack
    int sb;                // the state's batch row: b, or slot[b] of a slotted call
    bool closes, full;     // the first segment closes chunk i; the state is full afterwards
};
// false: no token, an inactive row of a slotted call, or (defence only) entries outside what the host vouched for -- the caller
// returns at once.  PACKED (g.off set) is a template parameter of this and of the chain's kernels, not a run-time test of the pointer:
// with the test compiled in, the padded k_cx_xty_acc became other code (60 SGPRs for 70; profiles/causal_extend_packed.md); as a
// parameter the padded instantiations are the code they were
template <bool PACKED = false>
__device__ __forceinline__ bool cx_seq(const CxRag& g, int b, CxSeq& s) {
    s.sb = cst_slot(g.slot, g.n_slots, b);
    if (s.sb < 0) return false;
    const int p = g.pos[s.sb];
    int w;
    [[maybe_unused]] int first = 0;
    if constexpr (PACKED) {   // workgroup-uniform entries read as cst_page reads the page table; a window that leaves [0, T) or offsets that decrease (w < 0, so n < 1): skipped
        first = *(const __attribute__((address_space(4))) int*)(g.off + b);
        const int end = *(const __attribute__((address_space(4))) int*)(g.off + b + 1);
        if (first < 0 || end > g.T) return false;
        w = end - first;
    } else {
        w = g.ntok[b];
    }
    const int n = g.acc ? min(g.acc[b], w) : w;
    if (p < 0 || n < 1 || w > g.T || (long)p + n > (long)g.max_end) return false;
    s.n = n; s.i = p / CS; s.r = p - s.i * CS;
    s.a = min(n, CS - s.r);
    s.later = (p + n - 1) / CS - s.i;
    s.iend = (p + n) / CS;
    s.closes = s.iend > s.i;
    s.full = s.iend >= g.cap;
    if constexpr (PACKED) s.shift = first;
    else s.shift = g.left ? g.T - w : 0;
    return s.later <= g.max_later && (!s.closes || g.any_close);
}

// where chunk j of state row sb, head h (of H) lives: S[sb][h][j] of a dense state, or its page; null: the table names no page
// for it (the host assigns every page a call can touch: defence only) and the caller drops the write
__device__ __forceinline__ float* cx_chunk(float* S, const CxRag& g, int sb, int H, int h, int j, long E) {
    if (!g.table) return S + (((long)sb * H + h) * g.cap + j) * E;
    const long pg = cst_page(g.table, g.n_pages, (long)sb * g.cap + j);
    return pg < 0 ? nullptr : S + (pg * H + h) * E;
}

struct CxOutArgs {
    View q, k, v;          // [B][T][H][K / V]: the extension's tokens
    MView o;               // [B][T][H][V] rows, rounded once; ptr null: fp32 rows to `stage` instead
    float* stage;          // [bh][T][V] fp32, NOT scaled (k_cs_step_finish scales, normalises and rounds); packed (rag.off): [h][T][V]
    const float* P;        // prefix mix of this launch's segment 0
    long p_bh, p_seg;      // floats from one (b, h) / one segment to the next
    const float* Cur;      // [bh][K][V] the open chunk's K^T V before the segment (first segment), or null: zero
    const float* mdiag;    // &mix[c][c] of segment 0's chunk
    long mstep;            // ldmix + 1
    long tok0, tend;       // segment s: tokens tok0 + 64 s .. min(tok0 + 64 s + 64, tend)
    int H, K, V;
    long T;
    float scale;
    // RAGGED only: P is the state's (later = 0) or the workspace (later = 1), Cur the state's, mdiag = &mix[0][0]
    CxRag rag;
    int later;             // 0: the first segment of every sequence; 1: segment blockIdx.x of the later ones
    int* nval;             // [B] (later = 0 writes it) tokens the chain accepts for sequence b: what the finish reads
    int kr, nsplit;        // the K split of k_cs_step for a batch of one: the sums of a one-token sequence
    // grouped-query heads: q, o and stage have H heads, k, v, P, Cur and the workspace tiles H / G -- query head h reads k/v head h / G
    int G;                 // >= 1
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

// One token of sequence (b, h) with the arithmetic of k_cs_step + k_cs_step_finish for a batch of one (RAGGED, n = 1): per K split
// thread (rg, c4) walks rows rg, rg + 16, ... with c = fmaf(k, v, Cur), acc = fmaf(q, fmaf(mii, c, P), acc); the 16 row groups are
// summed in order, then the splits in order.  Cur is NOT written here (k_cx_xty_acc forms the same fmaf).  red: [16][64] floats
template <typename T>
__device__ __forceinline__ void cx_one_token(const CxOutArgs& a, float* red, const T* qr, const T* kr, const T* vr, const float* Pi,
                                             const float* Ci, float mii, int v0, float* srow, int tid) {
    const int c4 = (tid & 15) * 4, rg = tid >> 4, col = v0 + c4;
    const bool live = col < a.V;
    f32x4 vv = {0.f, 0.f, 0.f, 0.f};
    if (live) vv = Io<T>::ld4(vr + col);
    float tot = 0.f;
    for (int sp = 0; sp < a.nsplit; ++sp) {
        const int k0 = sp * a.kr, k1 = min(a.K, k0 + a.kr);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            for (int r = k0 + rg; r < k1; r += CST_RG) {
                const f32x4 p = gld<f32x4>(Pi + (long)r * a.V + col);
                f32x4 c = gld<f32x4>(Ci + (long)r * a.V + col);
                const float qv = cst_ld1(qr + r), kv = cst_ld1(kr + r);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    c[t] = fmaf(kv, vv[t], c[t]);
                    acc[t] = fmaf(qv, fmaf(mii, c[t], p[t]), acc[t]);
                }
            }
        }
        *reinterpret_cast<f32x4*>(red + rg * CST_VT + c4) = acc;
        __syncthreads();
        if (tid < CST_VT) {
            float s = 0.f;
#pragma unroll
            for (int g = 0; g < CST_RG; ++g) s += red[g * CST_VT + tid];
            tot += s;
        }
        __syncthreads();
    }
    if (tid < CST_VT && v0 + tid < a.V) srow[tid] = tot;
}

// grid (segments, B H, ceil(V / 64)): k_cs_out on a run of <= 64 token rows of one chunk.  It only reads the state: with a.G > 1 the G
// query heads of a group read the one state of their k/v head (causal_step.hpp), each with the tiles and sums of the ungrouped call
template <typename T, CxVar VAR = CxVar{}>
__global__ __launch_bounds__(NTHREADS) void k_cx_out(const CxOutArgs a) {
    static_assert(VAR.valid(), "no such extend: see CxVar::valid");
    constexpr bool RAGGED = VAR.ragged, PACKED = VAR.packed;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Qs = smem;                  // [64 c][66]
    float* Ks = Qs + CS * CS_LDX;      // [64 c'][66]
    float* As = Ks + CS * CS_LDX;      // [64 c][66]
    float* Ps = As + CS * CS_LDX;      // [64 kk][80]  P slice, later V slice [64 c][80]
    float* Os = Ps + CS * CS_LDK;      // [64][68]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
    const int seg = blockIdx.x, bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
    const int hk = h / a.G;
    const long bhk = (long)b * (a.H / a.G) + hk;   // the call's (b, k/v head); G = 1: bh
    const int v0 = blockIdx.z * 64, vv = min(64, a.V - v0);
    long p0;
    int rv;
    const float* Pi;
    const float* Ci;
    float mii;
    [[maybe_unused]] bool one = false;
    if constexpr (RAGGED) {
        CxSeq s;
        const bool ok = cx_seq<PACKED>(a.rag, b, s);
        if (!a.later && h == 0 && blockIdx.z == 0 && tid == 0) a.nval[b] = ok ? s.n : 0;
        if (!ok || (a.later && seg >= s.later)) return;   // ahead of any LDS or further global traffic
        const long E = (long)a.K * a.V;
        const long sbhk = (long)s.sb * (a.H / a.G) + hk;   // the state's (row, k/v head)
        if (a.later) {
            const int tok = s.a + seg * CS;
            p0 = s.shift + tok;
            rv = min(CS, s.n - tok);
            Pi = a.P + (bhk * a.rag.max_later + seg) * E;
            Ci = nullptr;
            mii = a.mdiag[(long)(s.i + 1 + seg) * a.mstep];
        } else {
            p0 = s.shift;
            rv = s.a;
            Pi = a.P + sbhk * E;
            Ci = a.Cur + sbhk * E;
            mii = a.mdiag[(long)s.i * a.mstep];
            one = s.n == 1;
        }
    } else {
        p0 = a.tok0 + (long)seg * CS;
        rv = (int)min((long)CS, a.tend - p0);
        Pi = a.P + bhk * a.p_bh + (long)seg * a.p_seg;
        Ci = a.Cur ? a.Cur + bhk * a.K * a.V : nullptr;
        mii = a.mdiag[(long)seg * a.mstep];
    }
    const T* qb = (const T*)a.q.ptr + b * a.q.sb + h * a.q.sh;
    const T* kb = (const T*)a.k.ptr + b * a.k.sb + hk * a.k.sh;
    const T* vb = (const T*)a.v.ptr + b * a.v.sb + hk * a.v.sh;
    // the stage's rows of this (b, h): bh T ..; packed: the rows of head h are the pack's, h T .., and p0 counts from the pack's start
    const long sbh = PACKED ? h : bh;
    if constexpr (RAGGED) {
        if (one) {
            cx_one_token<T>(a, smem, qb + p0 * a.q.sn, kb + p0 * a.k.sn, vb + p0 * a.v.sn, Pi, Ci, mii, v0,
                            a.stage + (sbh * a.T + p0) * a.V + v0, tid);
            return;
        }
    }

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
        float* sb = a.stage + (sbh * a.T + p0) * a.V + v0;
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
    // RAGGED only: rows, src and dst are derived per sequence
    CxRag rag;
    int later;             // 0: the first segment (src = Cur); 1: segment blockIdx.x of the later ones (src null)
    float* S;              // [bh][cap][K][V]
    float* Cur;            // [bh][K][V]
    int* nval;             // [B] or null (later = 0 writes it): the tokens the chain accepts for sequence b, as k_cx_out's
};

// grid (1, B H, strips of 64 x 64): dst = src + X^T Y over the segment's rows -- the accumulating form of k_bm_state<MODE 2>
// RAGGED, grid (segments, B H, strips): each (b, h) for itself.  later = 0: the first segment, dst = S[i_b] where that sequence's chunk
// closes, else Cur; one token: fmaf(k, v, Cur), the step's rank-1 update.  later = 1: K^T V alone (k_bm_state<2>'s tiles, loads and
// kend: the same sums) of later segment blockIdx.x -- 64 rows -> S[i_b + 1 + s], fewer (the tail) -> Cur -- and segment 0's workgroups
// write Cur = 0 for a sequence that closed its chunk and has no tail.  The two are separate launches: the first reads Cur.
template <typename T, CxVar VAR = CxVar{}>
__global__ __launch_bounds__(NTHREADS) void k_cx_xty_acc(const CxAccArgs a) {
    static_assert(VAR.valid(), "no such extend: see CxVar::valid");
    constexpr bool RAGGED = VAR.ragged, PACKED = VAR.packed;
    constexpr int LD = ld_kmajor(64);
    __shared__ __attribute__((aligned(16))) float Xs[CS * LD];
    __shared__ __attribute__((aligned(16))) float Ys[CS * LD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
    const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
    const int nsy = (a.DY + 63) / 64;
    const int x0 = (blockIdx.z / nsy) * 64, y0 = (blockIdx.z % nsy) * 64;
    int rows = a.rows;
    long tok0 = 0;
    const float* sb = nullptr;
    float* db = nullptr;
    [[maybe_unused]] bool one = false, zero_cur = false;
    [[maybe_unused]] long sbh = bh;   // the state's (row, head)
    if constexpr (RAGGED) {
        CxSeq s;
        const bool ok = cx_seq<PACKED>(a.rag, b, s);
        if (a.nval && !a.later && h == 0 && blockIdx.z == 0 && tid == 0) a.nval[b] = ok ? s.n : 0;
        if (!ok) return;   // ahead of any LDS or further global traffic
        const long E = (long)a.DX * a.DY;
        sbh = (long)s.sb * a.H + h;
        if (a.later) {
            const int seg = blockIdx.x, rest = s.n - s.a;
            if (!s.closes) return;
            zero_cur = seg == 0 && rest % CS == 0 && !a.rag.dry;
            rows = seg < s.later ? min(CS, rest - seg * CS) : 0;
            if (a.rag.dry && rows < CS) return;   // (the tail would go to Cur)
            if (!rows && !zero_cur) return;
            tok0 = s.shift + s.a + (long)seg * CS;
            db = rows == CS ? cx_chunk(a.S, a.rag, s.sb, a.H, h, s.i + 1 + seg, E) : a.Cur + sbh * E;
            if (!db) {   // (no page)
                if (!zero_cur) return;
                rows = 0;
            }
        } else {
            if (a.rag.dry && !s.closes) return;   // (the sum would go to Cur)
            rows = s.a;
            tok0 = s.shift;
            sb = a.Cur + sbh * E;
            db = s.closes ? cx_chunk(a.S, a.rag, s.sb, a.H, h, s.i, E) : a.Cur + sbh * E;
            if (!db) return;   // (no page)
            one = s.n == 1;
        }
    } else {
        sb = a.src + (long)bh * a.DX * a.DY;
        db = a.dst + (long)bh * a.dst_bh;
    }
    const T* xb = (const T*)a.x.ptr + b * a.x.sb + h * a.x.sh;
    const T* yb = (const T*)a.y.ptr + b * a.y.sb + h * a.y.sh;
    const int kend = (rows + 3) & ~3;
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!RAGGED || rows) {
        load_tile<T, 64, false>(Xs, LD, xb + x0, a.x.sn, nullptr, tok0, rows, kend, a.DX - x0, 0.f, tid, NTHREADS);
        load_tile<T, 64, false>(Ys, LD, yb + y0, a.y.sn, nullptr, tok0, rows, kend, a.DY - y0, 0.f, tid, NTHREADS);
        __syncthreads();
        xty_accum<4, 4>(acc, Xs, Ys, LD, kend, wave, lane);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = wave + 4 * i, tm = t >> 2, tn = t & 3;
        const int col = y0 + tn * 16 + r16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = x0 + tm * 16 + kq * 4 + r;
            if (row < a.DX && col < a.DY) {
                if constexpr (RAGGED) {
                    const long at = (long)row * a.DY + col;
                    if (rows) {
                        float val = acc[i][r];
                        if (one) val = fmaf(Xs[row - x0], Ys[col - y0], sb[at]);
                        else if (sb) val = sb[at] + val;
                        db[at] = val;
                    }
                    if (zero_cur) a.Cur[sbh * a.DX * a.DY + at] = 0.f;
                } else {
                    db[(long)row * a.DY + col] = sb[(long)row * a.DY + col] + acc[i][r];
                }
            }
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

// P_c of the chunks c0 + u0 .. of one (b, h), elements e .. e + 3: ascending j with fmaf (k_cs_roll's sum).  `nws` of them go to the
// workspace, whose stride per (b, h) is `ws_bh` tiles.  bh: the call's (b, h), which owns the workspace; sbh: the state's (row, head),
// another only in a slotted call.  PAGED: S[j] through `trow`, the state row's entries of the page table (n_pages pages of pg_floats floats,
// this head's element e at `he` floats from a page's start): a group's eight entries are fetched ahead of its eight tile loads, a chunk without
// a page contributes no term, and every other term keeps its place
template <bool PAGED = false>
__device__ __forceinline__ void cx_mix_sums(const CxMixArgs& a, long bh, long sbh, long e, int c0, int nws, int ws_bh, int nc, int cP,
                                            [[maybe_unused]] const int* trow = nullptr, [[maybe_unused]] int n_pages = 0,
                                            [[maybe_unused]] long pg_floats = 0, [[maybe_unused]] long he = 0) {
    [[maybe_unused]] const float* Sb = PAGED ? nullptr : a.S + sbh * a.cap * a.E + e;
    const int u0 = blockIdx.z * CX_MIX_NC, nu = min(CX_MIX_NC, nc - u0);
    f32x4 acc[CX_MIX_NC];
#pragma unroll
    for (int u = 0; u < CX_MIX_NC; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int cbase = c0 + u0, jend = nu > 0 ? cbase + nu - 1 : 0;   // the last chunk of the group sums j < jend
    // j < cbase: a term of every chunk of the group (eight tiles in flight, no per-chunk test); cbase <= j < jend: of the chunks behind j
    constexpr int U = 8;
    const int jall = nu > 0 ? cbase : 0;
    int j0 = 0;
    for (; j0 + U <= jall; j0 += U) {
        f32x4 s[U];
        [[maybe_unused]] long pg[U];
        if constexpr (PAGED) {
#pragma unroll
            for (int w = 0; w < U; ++w) pg[w] = cst_page(trow, n_pages, j0 + w);
#pragma unroll
            for (int w = 0; w < U; ++w) {
                s[w] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (pg[w] >= 0) s[w] = gld<f32x4>(a.S + pg[w] * pg_floats + he);
            }
        } else {
#pragma unroll
            for (int w = 0; w < U; ++w) s[w] = gld<f32x4>(Sb + (long)(j0 + w) * a.E);
        }
#pragma unroll
        for (int u = 0; u < CX_MIX_NC; ++u) {
            if (u < nu) {
                const float* mr = a.mix + (long)(cbase + u) * a.ldmix + j0;
#pragma unroll
                for (int w = 0; w < U; ++w) {
                    if (PAGED && pg[w] < 0) continue;
                    const float m = mr[w];
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[u][t] = fmaf(m, s[w][t], acc[u][t]);
                }
            }
        }
    }
    for (int j = j0; j < jend; ++j) {
        const float* src;
        if constexpr (PAGED) {
            const long pg = cst_page(trow, n_pages, j);
            if (pg < 0) continue;
            src = a.S + pg * pg_floats + he;
        } else {
            src = Sb + (long)j * a.E;
        }
        const f32x4 s = gld<f32x4>(src);
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
            if (u0 + u < nws) gst<f32x4>(a.ws + (bh * ws_bh + u0 + u) * a.E + e, acc[u]);
            if (cbase + u == cP) gst<f32x4>(a.P + sbh * a.E + e, acc[u]);
        }
    }
    if (cP < 0 && blockIdx.z == 0) gst<f32x4>(a.P + sbh * a.E + e, f32x4{0.f, 0.f, 0.f, 0.f});
}

// grid (ceil(E / 4 / 64), B H, ceil(nc / 8)), one wave per workgroup: P_c = sum_{j < c} mix[c][j] S[j], ascending j (k_cs_roll's sum)
__global__ __launch_bounds__(64) void k_cx_mix(const CxMixArgs a) {
    const long e = ((long)blockIdx.x * 64 + threadIdx.x) * 4;
    if (e >= a.E) return;   // (E % 4 == 0)
    cx_mix_sums(a, blockIdx.y, blockIdx.y, e, a.c0, a.nws, a.nws, a.nc, a.cP);
}

struct CxMixRagArgs {
    CxMixArgs m;           // c0, nws, nc and cP unused: per sequence; ws null (commit): only the state's P is formed
    CxRag rag;
    int H;
};

// grid (ceil(E / 4 / 64), B H, groups of the largest nc): each (b, h) for itself -- a sequence that closes no chunk returns; else
// c0 = i_b + 1, its own later chunks to the workspace (stride rag.max_later), P of the chunk open afterwards to the state's P, or P = 0
// where that sequence's state is then full
template <CxVar VAR = CxVar{.ragged = true}>
__global__ __launch_bounds__(64) void k_cx_mix_ragged(const CxMixRagArgs a) {
    static_assert(VAR.valid() && VAR.ragged, "the ragged mix: see CxVar::valid");
    constexpr bool PACKED = VAR.packed;
    const long e = ((long)blockIdx.x * 64 + threadIdx.x) * 4;
    if (e >= a.m.E) return;   // (E % 4 == 0)
    const long bh = blockIdx.y;
    const int b = (int)(bh / a.H);
    CxSeq s;
    if (!cx_seq<PACKED>(a.rag, b, s) || !s.closes) return;
    const long sbh = bh + (long)(s.sb - b) * a.H;
    int c0 = s.i + 1, nws = s.later, ws_bh = a.rag.max_later, nc, cP;
    if (a.rag.dry) {   // the workspace tiles alone: no cP matches and none is negative
        if (!s.later) return;
        nc = s.later; cP = 0x7fffffff;
    } else if (!a.m.ws) {     // chunk iend alone (every accumulator sums ascending j by itself: the group does not change its bits), or P = 0
        c0 = s.iend; nws = 0; ws_bh = 0; nc = s.full ? 0 : 1; cP = s.full ? -1 : s.iend;
    } else {
        nc = (s.full ? s.i + s.later : s.iend) - s.i;
        cP = s.full ? -1 : s.iend;
    }
    if (a.rag.table)   // a paged pool: the same sums with every S[j] looked up in the row's table
        cx_mix_sums<true>(a.m, bh, sbh, e, c0, nws, ws_bh, nc, cP, a.rag.table + (long)s.sb * a.rag.cap, a.rag.n_pages, (long)a.H * a.m.E,
                          (bh - (long)b * a.H) * a.m.E + e);
    else
        cx_mix_sums(a.m, bh, sbh, e, c0, nws, ws_bh, nc, cP);
}

// grid (ceil(B / 64)): the last launch of the commit chain, pos[b] += nval[b] (nval: what the first launch of the chain accepted);
// a slotted call: the pool's pos[slot[b]], an inactive row none
__global__ __launch_bounds__(64) void k_cx_advance(int* pos, const int* nval, int B, const int* slot, int n_slots) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int sb = cst_slot(slot, n_slots, b);
    if (sb >= 0) pos[sb] += nval[b];
}

}  // namespace mhla
