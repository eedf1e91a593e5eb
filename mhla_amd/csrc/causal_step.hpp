// Causal chunk-mixing MHLA, token-by-token decoding (generation): the decode state of a sequence and the kernels of one step.
//
// Row t of the chunk operator (causal.hpp: naive_chunk_simple_mhla_fixed) depends on the tokens <= t only, so a step that
// reproduces row t needs, per (batch, head), in fp32:
//   S[j]  [K][V]  K_j^T V_j of every FINISHED chunk j  (mix[i][j] differs for every row i: no S[j] can be folded away)
//   P     [K][V]  the prefix mix of the open chunk i:  sum_{j<i} mix[i][j] S[j]
//   Cur   [K][V]  the open chunk's running K^T V
// With pos tokens seen, i = pos / 64, r = pos % 64, the step on the new token's (q, k, v) is
//   Cur += k (x) v ;  o = scale q^T (P + mix[i][i] Cur) ;  r == 63: S[i] = Cur, Cur = 0, P = sum_{j<=i} mix[i+1][j] S[j].
//   k_cs_step        : the rank-1 update and the mat-vec, tiled over V (64 columns) and split over K (16 rows x `kr / 16` per
//                      workgroup) so that B H = 4 still fills the machine; per-split partial sums of o -> fp32 workspace
//   k_cs_step_finish : partials summed in split order, scale, one rounding; optional RMSNorm x swish gate over the head's V channels
//   k_cs_roll        : the chunk boundary (and the prefix mix of a prefilled state; PACK: of every sequence of a prefilled pack)
//   k_cs_page_encode : h16 pages only -- the staged fp32 chunks of a pack prefill into their 2-byte pages
// Ragged batches (every sequence at a position of its own): the same kernels, instantiated with RAGGED, read pos[b] from a device
// int32 [B] array and derive i, r per (b, h) workgroup -- the step its mix[i][i], the roll whether this sequence is on a boundary
// at all.  Tiling, K split, row walk and the order of every sum are the uniform ones, so equal positions give the uniform bits.
// pos[b] advances in k_cs_step_finish, the last launch of the ragged chain (step, roll, finish) and the only one that does not
// address by it: no workgroup writes pos[b] in a launch in which another reads it.
// The finish is also the last launch of the ragged extend (WIN; causal_extend.hpp): over all B T padded rows it writes the rows outside a
// sequence's window as zeros and adds that sequence's token count to pos[b].
// Device-positioned steps (DEV; mhla_causal_step_dev): a launch chain whose shape and arguments do not depend on the positions
// at all, so that a captured graph can replay it token after token.  Always step, roll, finish; the bound on pos[b] is the
// state's capacity instead of a number the host vouches for per call.  A sequence with 0 <= pos[b] < 64 cap is LIVE and takes
// the ragged step (the same tiling, K split, row walk and order of every sum: the same bits).  Any other pos[b] makes it FROZEN,
// a defined branch: its workgroups touch neither P, Cur nor S, write zeros as their partial sums (so the finish really writes
// the row: o = 0, and y = 0 through the epilogue), pos[b] stays, and the finish sets full[b] = 1.  The roll is the ragged one
// with max_pos = 64 cap - 1: it returns after reading pos[b] unless that sequence is live and on a boundary.  The finish reads
// and writes pos[b] in ONE thread per sequence and nowhere else, so the rule above holds.  With PRO the step applies the fla
// layer's q / k prologue itself (feature map, then the NeoX rotary at row pos[b] of the cos / sin tables) where it loads q[r]
// and k[r]: fmrot_* (common.hpp), the arithmetic k_fmap_rotary runs, rounded to the tensor dtype where that kernel stores.
// Grouped-query heads (GMAX > 1; the *_gqa entry points): S, P and Cur depend on k and v alone, so the G = H / Hkv query heads of a
// group share ONE state, [B][Hkv][...].  A workgroup of the grouped step belongs to a k/v head: it loads its P / Cur rows, forms
// c = fmaf(k, v, Cur) and stores Cur once, and keeps one accumulator per query head of the group, acc[g] = fmaf(q_g, fmaf(mii, c, p),
// acc[g]) -- the sums of the ungrouped step on repeated heads, term for term and in order (the K split is chosen from the QUERY
// head count for that reason), at 1 / G of its state traffic.  The finish runs unchanged over the B H query heads.
// Memory-bound (P and Cur read, Cur written: 12 K V bytes per (b, h) and token); plain fp32 FMA, no MFMA, no atomics: every
// sum has a fixed order, so results repeat bit for bit.  The state is fp32 whatever the tensor dtype: Cur takes up to 64
// rank-1 updates and P sums up to L chunks -- a 16-bit state would round at every token.  (A FINISHED chunk is written once: the
// h16 pages of a paged pool, below, round it once; P and Cur stay fp32.)
#pragma once
#include "common.hpp"
#include "causal.hpp"   // CS, the chunk length

namespace mhla {

constexpr int CST_THREADS = 256;
constexpr int CST_VT = 64;        // V columns per workgroup: 16 lanes x 4
constexpr int CST_RG = 16;        // row groups per workgroup: thread (rg, c4) walks rows rg, rg + 16, ...

struct CsStepArgs {
    View q, k, v;          // [B][1][H][K / V]
    const float* mix;      // &mix[i][i]; RAGGED: &mix[0][0]
    float* P;              // [bh][K][V]
    float* Cur;            // [bh][K][V]
    float* part;           // [bh][nsplit][V]
    int H, K, V, kr, nsplit;
    // RAGGED only
    const int* pos;        // [B] tokens seen per sequence
    int ldmix, max_pos;    // row stride of mix; the largest position the host vouches for (a pos[b] outside 0 .. max_pos is clamped)
    // DEV only (max_pos = 64 cap - 1: a pos[b] outside 0 .. max_pos is a frozen sequence)
    const void* cos;       // PRO: [tab_rows][ldt] rotary tables in the tensor dtype, K / 2 columns read
    const void* sin;
    long ldt;
    int tab_rows, fmap;    // tab_rows >= 64 cap (the host checked); feature map: 0 identity, 1 relu, 2 elu + 1
    // GMAX > 1 only: H counts the k/v heads (k, v, P, Cur and the grid), q and part have G H heads, head hk G + g in group hk
    int G;                 // 1 .. GMAX
    // RAGGED only, slotted calls (cst_slot below): P, Cur and pos belong to a pool of n_slots rows, call row b uses row slot[b]
    const int* slot;       // [B] or null: row b itself
    int n_slots;
    // PAGED only (DEV on a paged pool, cst_page below): the page table, its row length (the capacity in chunks) and the page count
    const int* table;      // [n_slots][tcap]
    int tcap, n_pages;
};

// Slotted calls (the mhla_causal_*_slots entry points): the state -- S, P, Cur, pos, full -- is a pool of n_slots batch rows, and
// call row b works on row slot[b] of it; everything that belongs to the call (tokens, rows, workspace, ntok, accept, nval) stays
// addressed by b.  The state row of call row b: b itself without a map (today's addressing, the same bits), slot[b] with one, or -1
// where slot[b] is outside 0 .. n_slots - 1 -- such a row is INACTIVE: nothing of the pool is read or written for it and its rows
// come out as zeros, the frozen / skipped branches that exist.  Workgroup-uniform: every workgroup serves one call row.
__device__ __forceinline__ int cst_slot(const int* slot, int n_slots, int b) {
    if (!slot) return b;
    const int s = slot[b];
    return (unsigned)s < (unsigned)n_slots ? s : -1;
}
// the step's kernels take "slotted" as a template parameter, so that the un-slotted instantiations are the code they were (measured:
// profiles/causal_state_slots.md); the extend chain's kernels test the pointer at run time
template <bool SLOT>
__device__ __forceinline__ int cst_row(const int* slot, int n_slots, int b) {
    if constexpr (SLOT) return cst_slot(slot, n_slots, b);
    else return b;
}

// Paged pools (the mhla_causal_*_paged entry points): the finished chunks S[j] are not a dense [n_slots][H][cap] array but PAGES of
// a pool [n_pages][H][K][V] -- one page holds one chunk of one sequence, all k/v heads -- and table[sb cap + j] names the page of
// chunk j of state row sb.  A finished S[j] is never written again, so slots may share pages; P, Cur, pos and full stay dense per
// slot.  An entry outside 0 .. n_pages - 1 is NO PAGE (-1 here): no address is ever formed from it, a write there is dropped and a
// read contributes nothing.  The entry is workgroup-uniform and read through the constant address space, a scalar load, as
// ld_tab1 (blockmix.hpp) reads the pack tables.  Tiling and the order of every sum do not depend on where a chunk lives: the
// bits are those of the dense state that `compact()` gathers.
__device__ __forceinline__ long cst_page(const int* table, int n_pages, long at) {
    const int pg = *(const __attribute__((address_space(4))) int*)(table + at);
    return (unsigned)pg < (unsigned)n_pages ? (long)pg : -1L;
}

// pos[b] as the ragged step addresses by it.  Defence only: the caller keeps the array equal to its host mirror, and then the clamp
// changes nothing.  An array that disagrees with the mirror is a caller's error that gives wrong rows (another mix[i][i]); what the
// clamp -- and the roll's skip of such a sequence -- guarantee is that it cannot address outside what the host checked.
__device__ __forceinline__ int cst_pos(const int* pos, int b, int max_pos) { return min(max(pos[b], 0), max_pos); }

template <typename T> __device__ __forceinline__ float cst_ld1(const T* p);
template <> __device__ __forceinline__ float cst_ld1<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float cst_ld1<bf16_t>(const bf16_t* p) { return bf16_to_f32(p->v); }
template <> __device__ __forceinline__ float cst_ld1<f16_t>(const f16_t* p) { return (float)p->v; }
template <typename T> __device__ __forceinline__ void cst_st1(T* p, float x);
template <> __device__ __forceinline__ void cst_st1<float>(float* p, float x) { *p = x; }
template <> __device__ __forceinline__ void cst_st1<bf16_t>(bf16_t* p, float x) { p->v = cvt_bf16(x); }
template <> __device__ __forceinline__ void cst_st1<f16_t>(f16_t* p, float x) { p->v = (_Float16)x; }

// element r of a token's q or k row x [K] after the layer's prologue, as the tensor would hold it: f(x[r]) rotated with its
// partner f(x[r +- K / 2]) by the angle in row `cosr` / `sinr` of the tables (null: no rotation), rounded to T
template <typename T>
__device__ __forceinline__ float cst_pro1(const T* x, int r, int half, const T* cosr, const T* sinr, int fmap) {
    if (!cosr) return stored_value<T>(fmrot_map(cst_ld1(x + r), fmap));   // (a feature map without rotary)
    const bool lo = r < half;
    const int j = lo ? r : r - half;
    const float x0 = fmrot_map(cst_ld1(x + j), fmap), x1 = fmrot_map(cst_ld1(x + j + half), fmap);
    const float c = cst_ld1(cosr + j), s = cst_ld1(sinr + j);
    return stored_value<T>(lo ? fmrot_lo(x0, x1, c, s) : fmrot_hi(x0, x1, c, s));
}

constexpr int CST_GMAX = 8;       // query heads per k/v head the grouped step serves

// grid (ceil(V / 64), nsplit, B H); GMAX > 1 (grouped-query heads, a.H = Hkv): one accumulator per query head g < a.G of the group,
// the loop over g fully unrolled and predicated by a.G alone (uniform over the launch)
// PAGED (DEV on a paged pool): a sequence is live iff its position is inside the capacity AND the table names a page for chunk
// pos / 64 -- the page its boundary roll will write; the step itself touches no page
// the step's variants, named at the launch site: StepVar{.ragged = true, .dev = true, .gmax = CST_GMAX}
struct StepVar {
    bool ragged = false, dev = false, pro = false;
    int gmax = 1;
    bool slot = false, paged = false;
    constexpr bool operator==(const StepVar&) const = default;
    constexpr bool valid() const {
        return (!slot || ragged)              // a slot map goes with positions on the device
               && (!paged || (slot && dev))   // the step reads the page table only to tell a live sequence from a frozen one
               && (!dev || ragged)            // dev is the ragged step, bounded by the capacity
               && (!pro || dev)               // the fused prologue goes with the device-positioned step
               && (gmax == 1 || ragged);      // grouped heads: the ragged and device-positioned steps only
    }
};
template <typename T, StepVar VAR = StepVar{}>
__global__ __launch_bounds__(CST_THREADS) void k_cs_step(const CsStepArgs a) {
    static_assert(VAR.valid(), "no such step: see StepVar::valid");
    constexpr bool RAGGED = VAR.ragged, DEV = VAR.dev, PRO = VAR.pro, SLOT = VAR.slot, PAGED = VAR.paged;
    constexpr int GMAX = VAR.gmax;
    __shared__ __attribute__((aligned(16))) float red[GMAX][CST_RG][CST_VT];
    const int tid = threadIdx.x, c4 = (tid & 15) * 4, rg = tid >> 4;
    const int bh = blockIdx.z, b = bh / a.H, h = bh - b * a.H;
    const int G = GMAX > 1 ? a.G : 1;
    const int col = blockIdx.x * CST_VT + c4;
    const int k0 = blockIdx.y * a.kr, k1 = min(a.K, k0 + a.kr);
    bool live = col < a.V;   // (V % 4 == 0: a thread's four columns are inside or outside together)
    const T* qb = (const T*)a.q.ptr + b * a.q.sb + (long)h * G * a.q.sh;   // (query head h G of the group)
    const T* kb = (const T*)a.k.ptr + b * a.k.sb + h * a.k.sh;
    const T* vb = (const T*)a.v.ptr + b * a.v.sb + h * a.v.sh;
    float mii;
    [[maybe_unused]] const T* cosr = nullptr;
    [[maybe_unused]] const T* sinr = nullptr;
    long sbh = bh;   // the state's (row, head): the call's own without a slot map
    [[maybe_unused]] int sb = b;
    if constexpr (SLOT) {
        sb = cst_slot(a.slot, a.n_slots, b);
        sbh = (long)max(sb, 0) * a.H + h;
    }
    if constexpr (DEV) {
        int p = SLOT && sb < 0 ? -1 : a.pos[sb];
        if constexpr (PAGED) {   // (no page for the open chunk: frozen, as a full state is)
            if (p >= 0 && p <= a.max_pos && cst_page(a.table, a.n_pages, (long)sb * a.tcap + p / CS) < 0) p = -1;
        }
        if (p < 0 || p > a.max_pos) {   // frozen (an inactive row of a slotted call included): zeros as partial sums, the state untouched
            live = false;
            p = 0;
        }
        const long i = p / CS;          // (< cap <= ldmix and the rows of mix: the host checked)
        mii = a.mix[i * a.ldmix + i];
        if constexpr (PRO) {
            if (a.cos) {
                const long row = min(p, a.tab_rows - 1);
                cosr = (const T*)a.cos + row * a.ldt;
                sinr = (const T*)a.sin + row * a.ldt;
            }
        }
    } else if constexpr (RAGGED) {
        if (SLOT && sb < 0) live = false;   // an inactive row of a slotted call: zeros as partial sums, the state untouched
        const long i = SLOT && sb < 0 ? 0 : cst_pos(a.pos, sb, a.max_pos) / CS;
        mii = a.mix[i * a.ldmix + i];
    } else {
        mii = *a.mix;
    }
    f32x4 acc[GMAX];
#pragma unroll
    for (int g = 0; g < GMAX; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (live) {
        const f32x4 vv = Io<T>::ld4(vb + col);
        const long base = sbh * a.K * a.V + col;
        constexpr int U = 4;   // rows in flight per thread: 2 U 16-byte loads
        for (int r0 = k0 + rg; r0 < k1; r0 += CST_RG * U) {
            f32x4 p[U], c[U];
            float qv[GMAX][U], kv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int r = r0 + u * CST_RG;
                if (r < k1) {
                    p[u] = gld<f32x4>(a.P + base + (long)r * a.V);
                    c[u] = gld<f32x4>(a.Cur + base + (long)r * a.V);
                    if constexpr (PRO) kv[u] = cst_pro1(kb, r, a.K / 2, cosr, sinr, a.fmap);
                    else               kv[u] = cst_ld1(kb + r);
#pragma unroll
                    for (int g = 0; g < GMAX; ++g) {
                        if (g < G) {
                            if constexpr (PRO) qv[g][u] = cst_pro1(qb + g * a.q.sh, r, a.K / 2, cosr, sinr, a.fmap);
                            else               qv[g][u] = cst_ld1(qb + g * a.q.sh + r);
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int r = r0 + u * CST_RG;
                if (r < k1) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) c[u][t] = fmaf(kv[u], vv[t], c[u][t]);
#pragma unroll
                    for (int g = 0; g < GMAX; ++g) {
                        if (g < G) {
#pragma unroll
                            for (int t = 0; t < 4; ++t) acc[g][t] = fmaf(qv[g][u], fmaf(mii, c[u][t], p[u][t]), acc[g][t]);
                        }
                    }
                    gst<f32x4>(a.Cur + base + (long)r * a.V, c[u]);
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < GMAX; ++g)
        if (g < G) *reinterpret_cast<f32x4*>(&red[g][rg][c4]) = acc[g];
    __syncthreads();
    if (tid < CST_VT) {
        const int cc = blockIdx.x * CST_VT + tid;
        if (cc < a.V) {
#pragma unroll
            for (int g = 0; g < GMAX; ++g) {
                if (g < G) {
                    float s = 0.f;
#pragma unroll
                    for (int j = 0; j < CST_RG; ++j) s += red[g][j][tid];
                    a.part[(((long)bh * G + g) * a.nsplit + blockIdx.y) * a.V + cc] = s;
                }
            }
        }
    }
}

struct CsFinishArgs {
    const float* part;     // [bh][T][nsplit][V]
    MView out, y;          // [B][T][H][V], T = gridDim.y (the step: 1); either ptr may be null
    View gate;             // ptr null: no gate
    const float* nw;       // [V] or null
    float neps, scale;
    int H, V, nsplit;
    int* advance;          // [B] or null: positions of a ragged state, each advanced once (by the workgroup of head 0, token 0)
    // DEV only: a position outside 0 .. max_pos (64 cap - 1) stays, and full[b] = 1 instead
    int max_pos;
    int* full;             // [B], never cleared here
    // WIN only (the ragged extend, causal_extend.hpp): sequence b's rows are nval[b] <= T of the T padded ones
    const int* nval;       // [B] tokens the chain accepted per sequence
    int left;              // the window is rows [T - nval[b], T) instead of [0, nval[b])
    // slotted calls (cst_slot): advance and full are the pool's [n_slots], call row b moves entry slot[b]; an inactive row moves none
    const int* slot;       // [B] or null
    int n_slots;
    // PAGED only (DEV on a paged pool): a position whose chunk has no page in the table stays as well, and full[b] = 1
    const int* table;      // [n_slots][tcap]
    int tcap, n_pages;
    // PACKED only (WIN; the packed extend, causal_extend.hpp): the rows are ONE run of gridDim.y tokens, sequence b's [off[b], off[b + 1])
    const int* off;        // [nseq + 1]
    int nseq;
};

// grid (B H, T tokens): o = scale * (partials in split order); y = o rsqrt(mean(o^2 over V) + neps) nw g sigmoid(g), from the fp32 o
// DEV: the one thread that advances pos[b] is the only one of the launch to read it; a frozen sequence's partial sums are the zeros
// its step wrote, so its row needs no branch here
// WIN: a row outside its sequence's window is written as zeros (out and y) and reads nothing else; advance[b] += nval[b].  pos is
// not read by any other thread of this launch: the window comes from nval, which an earlier launch of the chain wrote
// PACKED (with WIN), grid (H, tokens of the pack): part is [h][tokens][V] and out, y, gate come with sb = 0.  The workgroup finds the
// sequence its row belongs to by a binary search over off (workgroup-uniform, read as cst_page reads the table; at most 17 halvings
// for the 65535 sequences a grid holds); a row of a sequence the chain did not accept (nval[b] = 0), or -- defence only -- of no
// sequence, is written as zeros; the workgroup of head 0 on the first row of sequence b advances its position
struct FinishVar {
    bool dev = false, win = false, slot = false, paged = false, packed = false;
    constexpr bool operator==(const FinishVar&) const = default;
    constexpr bool valid() const {
        return !(dev && win)                  // the device-positioned step has one row per sequence
               && (!paged || (slot && dev))   // the finish reads the page table only to tell a live sequence from a frozen one
               && (!packed || win);           // a pack is a set of windows
    }
};
template <typename T, FinishVar VAR = FinishVar{}>
__global__ __launch_bounds__(CST_THREADS) void k_cs_step_finish(const CsFinishArgs a) {
    static_assert(VAR.valid(), "no such finish: see FinishVar::valid");
    constexpr bool DEV = VAR.dev, WIN = VAR.win, SLOT = VAR.slot, PAGED = VAR.paged, PACKED = VAR.packed;
    __shared__ float red[CST_THREADS / 64];
    const int tid = threadIdx.x;
    int bh = blockIdx.x, b = bh / a.H, h = bh - b * a.H;
    const long tok = blockIdx.y;
    if constexpr (PACKED) {
        const auto off_at = [&](int i) { return *(const __attribute__((address_space(4))) int*)(a.off + i); };
        h = bh;   // (bh stays the head: part's rows of a head are the pack's)
        int lo = 0, hi = a.nseq;   // the last b with off[b] <= tok: empty sequences before it share its offset
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (off_at(mid) <= (int)tok) lo = mid;
            else hi = mid;
        }
        b = lo;
        const int first = off_at(b), n = a.nval[b];
        if (a.advance && h == 0 && tok == first && tid == 0 && n > 0) {   // (nothing in this launch reads it; null: a verify)
            const int sb = cst_row<SLOT>(a.slot, a.n_slots, b);
            if (!SLOT || sb >= 0) a.advance[sb] += n;
        }
        if (tok < first || tok - first >= n) {
            T* ob = a.out.ptr ? (T*)a.out.ptr + tok * a.out.sn + h * a.out.sh : nullptr;
            T* yb = a.y.ptr ? (T*)a.y.ptr + tok * a.y.sn + h * a.y.sh : nullptr;
            for (int c = tid; c < a.V; c += CST_THREADS) {
                if (ob) cst_st1(ob + c, 0.f);
                if (yb) cst_st1(yb + c, 0.f);
            }
            return;
        }
        b = 0;   // (the views of a pack have one batch row)
    } else if constexpr (WIN) {
        const int n = a.nval[b], t0 = a.left ? (int)gridDim.y - n : 0;
        if (a.advance && h == 0 && tok == 0 && tid == 0) {   // (nothing in this launch reads it; null: a verify)
            const int sb = cst_row<SLOT>(a.slot, a.n_slots, b);
            if (!SLOT || sb >= 0) a.advance[sb] += n;
        }
        if (tok < t0 || tok >= t0 + n) {
            T* ob = a.out.ptr ? (T*)a.out.ptr + b * a.out.sb + tok * a.out.sn + h * a.out.sh : nullptr;
            T* yb = a.y.ptr ? (T*)a.y.ptr + b * a.y.sb + tok * a.y.sn + h * a.y.sh : nullptr;
            for (int c = tid; c < a.V; c += CST_THREADS) {
                if (ob) cst_st1(ob + c, 0.f);
                if (yb) cst_st1(yb + c, 0.f);
            }
            return;
        }
    } else if constexpr (DEV) {
        if (h == 0 && tok == 0 && tid == 0) {
            const int sb = cst_row<SLOT>(a.slot, a.n_slots, b);
            if (!SLOT || sb >= 0) {
                const int p = a.advance[sb];
                bool frozen = p < 0 || p > a.max_pos;
                if constexpr (PAGED) frozen = frozen || cst_page(a.table, a.n_pages, (long)sb * a.tcap + p / CS) < 0;
                if (frozen) a.full[sb] = 1;
                else a.advance[sb] = p + 1;
            }
        }
    } else {
        if (a.advance && h == 0 && tok == 0 && tid == 0) {   // (nothing in this launch reads it)
            const int sb = cst_row<SLOT>(a.slot, a.n_slots, b);
            if (!SLOT || sb >= 0) a.advance[sb] += 1;
        }
    }
    const float* pb = a.part + ((long)bh * gridDim.y + tok) * a.nsplit * a.V;
    T* ob = a.out.ptr ? (T*)a.out.ptr + b * a.out.sb + tok * a.out.sn + h * a.out.sh : nullptr;
    auto o_at = [&](int c) {   // one accumulator, split order; the loads of a batch of eight issued together
        float s = 0.f;
        int j = 0;
        for (; j + 8 <= a.nsplit; j += 8) {
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = pb[(long)(j + u) * a.V + c];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += t[u];
        }
        for (; j < a.nsplit; ++j) s += pb[(long)j * a.V + c];
        return a.scale * s;
    };
    constexpr int NC = 4;   // columns a thread keeps in registers between the two passes (V <= 1024); beyond: summed again
    float oreg[NC];
    float ss = 0.f;
#pragma unroll
    for (int u = 0; u < NC; ++u) {
        const int c = tid + u * CST_THREADS;
        oreg[u] = c < a.V ? o_at(c) : 0.f;
        ss = fmaf(oreg[u], oreg[u], ss);
        if (ob && c < a.V) cst_st1(ob + c, oreg[u]);
    }
    for (int c = tid + NC * CST_THREADS; c < a.V; c += CST_THREADS) {
        const float o = o_at(c);
        ss = fmaf(o, o, ss);
        if (ob) cst_st1(ob + c, o);
    }
    if (!a.y.ptr) return;
    ss = wave_sum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    const float rstd = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)a.V + a.neps);
    T* yb = (T*)a.y.ptr + b * a.y.sb + tok * a.y.sn + h * a.y.sh;
    const T* gb = a.gate.ptr ? (const T*)a.gate.ptr + b * a.gate.sb + tok * a.gate.sn + h * a.gate.sh : nullptr;
    auto put = [&](int c, float o) {
        float yv = o * rstd;
        if (a.nw) yv *= a.nw[c];
        if (gb) {
            const float g = cst_ld1(gb + c);
            yv *= g / (1.f + __expf(-g));
        }
        cst_st1(yb + c, yv);
    };
#pragma unroll
    for (int u = 0; u < NC; ++u) {
        const int c = tid + u * CST_THREADS;
        if (c < a.V) put(c, oreg[u]);
    }
    for (int c = tid + NC * CST_THREADS; c < a.V; c += CST_THREADS) put(c, o_at(c));   // (the same sum in the same order as above)
}

struct CsRollArgs {
    float* S;              // [bh][cap][K][V]
    float* P;              // [bh][K][V]
    float* Cur;            // [bh][K][V]
    const float* mixrow;   // row of mix the new P is formed with (nj entries read), or null: P = 0
    long E;                // K V
    int cap, nj, commit;   // commit: S[nj - 1] = Cur, Cur = 0 first (the boundary); else S[0 .. nj) as they are (prefill)
    // RAGGED only: nj, commit and mixrow are derived per sequence from pos[b], the position of the token the step just took
    // PACK only (the prefill of a pack, mhla_causal_varlen_state_init): from pos[b], the tokens of sequence b; max_pos: the longest
    const int* pos;        // [B]
    const float* mix;      // &mix[0][0]
    int ldmix, max_pos, H;
    // slotted calls (cst_slot): S, P and Cur are the pool's, (b, h) works on row slot[b]; RAGGED reads the pool's pos[slot[b]], PACK
    // the call's own pos[b] (the tokens of sequence b of the pack)
    const int* slot;       // [B] or null
    int n_slots;
    // PAGED only (cst_page): S is a pool of pages [n_pages][H][K][V] and chunk j of state row sb lives in page table[sb cap + j]
    const int* table;      // [n_slots][cap]
    int n_pages;
    // FMT == PF_H16 only (h16 pages, below): the pool's payload [n_pages][H][K][V] and multipliers [n_pages][H][K V / 64]; S is unused
    _Float16* pay;
    float* mult;
};

// ---- h16 pages: a paged pool whose finished chunks take 2 bytes an element (the mhla_causal_*_paged_h16 entry points)
// A page is a payload _Float16 [H][K][V] and, apart from it, multipliers float [H][K V / 64]: group g of a head is elements
// [64 g, 64 g + 64) of the head's flattened [K][V] chunk (K V % 64 == 0: the host checked), stored as the h16 format of common.hpp --
// m = h16_mult_from_max(largest magnitude of the group), payload = (_Float16)(x h16_inv(m)) rounded to nearest even, decoded as
// (float)payload m, exact in fp32.  A finished chunk is written once, so it is rounded once; P and Cur stay fp32.
// A lane holds CSH_EPL = 8 adjacent elements, one 16-byte piece of the payload (8-byte requests move at 0.54 - 0.70 of the 16-byte
// rate, which would give back what the halved bytes gain: profiles/causal_state_h16.md), so a group is 8 adjacent lanes and a wave
// covers 512 elements.  Encode and decode below are the only ones: every writer and every reader of a page goes through them.
constexpr int PF_F32 = 0, PF_H16 = 1;   // page formats
constexpr int CSH_GROUP = 64;           // elements per multiplier
constexpr int CSH_EPL = 8;              // elements per lane
typedef float f32x8 __attribute__((ext_vector_type(8)));

// x: this lane's 8 elements of a group whose other 56 the 7 neighbouring lanes hold (all 8 lanes of the group must call: the group's
// largest magnitude is taken across them).  Magnitudes compare as bit patterns, so a NaN or an infinity orders above every finite
// value -- the multiplier reads the exponent field alone.  Returns the payload piece; m: the group's multiplier, the same in all 8 lanes
__device__ __forceinline__ f16x8 csh_encode(const f32x8 x, float& m) {
    unsigned mx = 0u;
#pragma unroll
    for (int t = 0; t < CSH_EPL; ++t) mx = max(mx, __float_as_uint(x[t]) & 0x7fffffffu);
#pragma unroll
    for (int o = 1; o < CSH_GROUP / CSH_EPL; o <<= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o, 64));
    m = h16_mult_from_max(__uint_as_float(mx));
    const float inv = h16_inv(m);
    f16x8 p;
#pragma unroll
    for (int t = 0; t < CSH_EPL; ++t) p[t] = (_Float16)(x[t] * inv);   // (round to nearest even)
    return p;
}
__device__ __forceinline__ f32x8 csh_decode(const f16x8 p, float m) {
    f32x8 x;
#pragma unroll
    for (int t = 0; t < CSH_EPL; ++t) x[t] = (float)p[t] * m;
    return x;
}
__device__ __forceinline__ f32x8 csh_ld8(const float* p) {
    const f32x4 a = gld<f32x4>(p), b = gld<f32x4>(p + 4);
    return f32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
__device__ __forceinline__ void csh_st8(float* p, const f32x8 x) {
    gst<f32x4>(p, f32x4{x[0], x[1], x[2], x[3]});
    gst<f32x4>(p + 4, f32x4{x[4], x[5], x[6], x[7]});
}

// the h16 roll: k_cs_roll<RollVar{.ragged or .pack, .slot, .paged, .fmt = PF_H16}>, grid (ceil(E / 8 / 64), B H), one wave per workgroup.  What RAGGED
// and PACK derive per sequence is what the fp32 kernel derives.  The commit encodes Cur into the page (the multiplier from one lane
// of the group, the payload from all) and zeroes Cur; the new P is the ascending fmaf sum over DECODED pages, the chunk just
// committed included -- mixrow[n] * decode(encode(last)), not the fp32 `last` -- so that P is a function of the pages alone and a
// slot that was prefilled and one that was stepped to the same tokens hold the same bits.  E % 64 == 0: whole groups leave together at
// the `e >= E` test, every other return is uniform over the wave, so all 8 lanes of a group that stays reach the reduction.
template <bool RAGGED, bool PACK>
__device__ __forceinline__ void cs_roll_h16(const CsRollArgs& a) {
    const long e = ((long)blockIdx.x * 64 + threadIdx.x) * CSH_EPL;
    if (e >= a.E) return;
    const int b = (int)(blockIdx.y / a.H), h = (int)(blockIdx.y - b * a.H);
    const int sb = cst_slot(a.slot, a.n_slots, b);
    if (sb < 0) return;   // an inactive row of a slotted call
    const long pe = ((long)sb * a.H + h) * a.E + e;
    int nj, commit;
    if constexpr (PACK) {
        const int p = a.pos[b];
        if (p < 0 || p > a.max_pos) return;
        nj = p / CS;
        commit = 0;
        if (p % CS == 0) csh_st8(a.Cur + pe, f32x8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f});
    } else {
        static_assert(RAGGED, "the h16 roll is the ragged or the pack one");
        const int p = a.pos[sb];
        if (p < 0 || p > a.max_pos || p % CS != CS - 1) return;
        nj = p / CS + 1;
        commit = 1;
    }
    const float* mixrow = nj < a.cap ? a.mix + (long)nj * a.ldmix : nullptr;
    const int* trow = a.table + (long)sb * a.cap;
    const long G = a.E / CSH_GROUP;                        // multipliers per head
    const long he = (long)h * a.E + e, hg = h * G + e / CSH_GROUP;   // from a page's start: this lane's payload piece, its group's multiplier
    const long PE = (long)a.H * a.E, PG = a.H * G;         // elements, multipliers per page
    int n = nj;
    f32x8 last = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (commit) {
        const long pg = cst_page(trow, a.n_pages, nj - 1);
        if (pg < 0) return;   // ahead of any write
        float m;
        const f16x8 pay = csh_encode(csh_ld8(a.Cur + pe), m);
        gst<f16x8>(a.pay + pg * PE + he, pay);
        if ((threadIdx.x & (CSH_GROUP / CSH_EPL - 1)) == 0) a.mult[pg * PG + hg] = m;
        csh_st8(a.Cur + pe, f32x8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f});
        last = csh_decode(pay, m);
        n = nj - 1;
    }
    f32x8 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (mixrow) {
        constexpr int U = 8;
        int j = 0;
        for (; j + U <= n; j += U) {
            f16x8 s[U];
            float m[U];
            long pg[U];
#pragma unroll
            for (int u = 0; u < U; ++u) pg[u] = cst_page(trow, a.n_pages, j + u);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (pg[u] >= 0) {
                    s[u] = gld<f16x8>(a.pay + pg[u] * PE + he);
                    m[u] = a.mult[pg[u] * PG + hg];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (pg[u] < 0) continue;
                const float w = mixrow[j + u];
                const f32x8 d = csh_decode(s[u], m[u]);
#pragma unroll
                for (int t = 0; t < CSH_EPL; ++t) acc[t] = fmaf(w, d[t], acc[t]);
            }
        }
        for (; j < n; ++j) {
            const long pg = cst_page(trow, a.n_pages, j);
            if (pg < 0) continue;
            const f32x8 d = csh_decode(gld<f16x8>(a.pay + pg * PE + he), a.mult[pg * PG + hg]);
            const float w = mixrow[j];
#pragma unroll
            for (int t = 0; t < CSH_EPL; ++t) acc[t] = fmaf(w, d[t], acc[t]);
        }
        if (commit) {
            const float w = mixrow[n];
#pragma unroll
            for (int t = 0; t < CSH_EPL; ++t) acc[t] = fmaf(w, last[t], acc[t]);
        }
    }
    csh_st8(a.P + pe, acc);
}

// grid (ceil(E / 4 / 64), B H), one wave per workgroup: P = sum_{j < nj} mixrow[j] S[j], ascending j
// RAGGED: each (b, h) for itself -- not on a boundary (pos[b] % 64 != 63): nothing; else the commit with nj = i + 1 and the new P
// from row i + 1 of mix, or P = 0 when i + 1 == cap (this sequence's state is full)
// PACK: each (b, h) for itself, the prefix mix of a state whose finished chunks S[0 .. nj) were just written, nj = pos[b] / 64 --
// no commit; P from row nj of mix, or P = 0 when nj == cap; Cur = 0 where the sequence has no open chunk (pos[b] % 64 == 0, an
// empty sequence included: P = Cur = 0).  A pos[b] outside 0 .. max_pos leaves the sequence untouched (defence only, as RAGGED)
// PAGED: every S[j] through the table, the group's eight entries fetched ahead of its eight tile loads; the same terms in the same
// order.  A boundary whose chunk has no page leaves the sequence untouched: for the device-positioned step that sequence is frozen
// (step and finish derive the same from pos and the table), for a host-positioned call it is defence only
// FMT == PF_H16 (h16 pages): cs_roll_h16 above, grid (ceil(E / 8 / 64), B H); the fp32 instantiations are the code they were
struct RollVar {
    bool ragged = false, pack = false, slot = false, paged = false;
    int fmt = PF_F32;
    constexpr bool operator==(const RollVar&) const = default;
    constexpr bool valid() const {
        return !(ragged && pack)                          // one addressing mode
               && (!paged || (slot && (ragged || pack)))  // a paged pool is addressed through a slot map
               && (fmt == PF_F32 || paged);               // a page format goes with a paged pool
    }
};
template <RollVar VAR = RollVar{}>
__global__ __launch_bounds__(64) void k_cs_roll(const CsRollArgs a) {
    static_assert(VAR.valid(), "no such roll: see RollVar::valid");
    constexpr bool RAGGED = VAR.ragged, PACK = VAR.pack, SLOT = VAR.slot, PAGED = VAR.paged;
    constexpr int FMT = VAR.fmt;
    if constexpr (FMT == PF_H16) {
        cs_roll_h16<RAGGED, PACK>(a);
        return;
    }
    const long e = ((long)blockIdx.x * 64 + threadIdx.x) * 4;
    if (e >= a.E) return;   // (E % 4 == 0)
    long bh = blockIdx.y;   // below: the state's (row, head)
    int nj = a.nj, commit = a.commit;
    const float* mixrow = a.mixrow;
    [[maybe_unused]] int sb = 0;
    if constexpr (RAGGED || PACK) {
        const int b = (int)(bh / a.H);
        sb = cst_row<SLOT>(a.slot, a.n_slots, b);
        if (SLOT && sb < 0) return;   // an inactive row of a slotted call
        if constexpr (SLOT) bh += (long)(sb - b) * a.H;
    }
    if constexpr (PACK) {
        const int p = a.pos[blockIdx.y / a.H];
        if (p < 0 || p > a.max_pos) return;
        nj = p / CS;   // (<= cap: the host checked ceil(max_pos / 64) <= cap)
        commit = 0;
        mixrow = nj < a.cap ? a.mix + (long)nj * a.ldmix : nullptr;
        if (p % CS == 0) gst<f32x4>(a.Cur + bh * a.E + e, f32x4{0.f, 0.f, 0.f, 0.f});
    }
    if constexpr (RAGGED) {
        const int p = a.pos[sb];
        if (p < 0 || p > a.max_pos || p % CS != CS - 1) return;   // (outside 0 .. max_pos: defence only, see cst_pos)
        nj = p / CS + 1;   // (<= cap: the host checked max_pos / 64 < cap)
        commit = 1;
        mixrow = nj < a.cap ? a.mix + (long)nj * a.ldmix : nullptr;
    }
    [[maybe_unused]] float* Sb = nullptr;          // dense: S[0] of this (row, head)
    [[maybe_unused]] const int* trow = nullptr;    // PAGED: this row's entries of the table
    [[maybe_unused]] long he = 0;                  // PAGED: floats from a page's start to this head's element e
    if constexpr (PAGED) {
        trow = a.table + (long)sb * a.cap;
        he = (long)(blockIdx.y % a.H) * a.E + e;
    } else {
        Sb = a.S + bh * a.cap * a.E + e;
    }
    const long pe = bh * a.E + e;
    int n = nj;
    f32x4 last = {0.f, 0.f, 0.f, 0.f};
    if (commit) {
        float* dst;
        if constexpr (PAGED) {
            const long pg = cst_page(trow, a.n_pages, nj - 1);
            if (pg < 0) return;   // ahead of any write
            dst = a.S + pg * a.H * a.E + he;
        } else {
            dst = Sb + (long)(nj - 1) * a.E;
        }
        last = gld<f32x4>(a.Cur + pe);
        gst<f32x4>(dst, last);
        gst<f32x4>(a.Cur + pe, f32x4{0.f, 0.f, 0.f, 0.f});
        n = nj - 1;
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (mixrow) {
        constexpr int U = 8;
        int j = 0;
        for (; j + U <= n; j += U) {
            f32x4 s[U];
            [[maybe_unused]] long pg[U];
            if constexpr (PAGED) {
#pragma unroll
                for (int u = 0; u < U; ++u) pg[u] = cst_page(trow, a.n_pages, j + u);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    s[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (pg[u] >= 0) s[u] = gld<f32x4>(a.S + pg[u] * a.H * a.E + he);
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) s[u] = gld<f32x4>(Sb + (long)(j + u) * a.E);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (PAGED && pg[u] < 0) continue;
                const float w = mixrow[j + u];
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = fmaf(w, s[u][t], acc[t]);
            }
        }
        for (; j < n; ++j) {
            const float* src;
            if constexpr (PAGED) {
                const long pg = cst_page(trow, a.n_pages, j);
                if (pg < 0) continue;
                src = a.S + pg * a.H * a.E + he;
            } else {
                src = Sb + (long)j * a.E;
            }
            const f32x4 s = gld<f32x4>(src);
            const float w = mixrow[j];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = fmaf(w, s[t], acc[t]);
        }
        if (commit) {
            const float w = mixrow[n];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = fmaf(w, last[t], acc[t]);
        }
    }
    gst<f32x4>(a.P + pe, acc);
}

struct CsEncodeArgs {
    const float* stage;    // [H][n][K V] fp32: K^T V of chunk c of this slice of the pack's chunk list, head h, at (h n + c) K V
    const int* tab;        // [n][2] {first row, rows} of the slice's chunks (a chunk of 64 rows is a finished one)
    const int* dst;        // [n][2] {sequence, index of the chunk within its sequence}
    _Float16* pay;         // the pool: [n_pages][H][K][V]
    float* mult;           //           [n_pages][H][K V / 64]
    float* Cur;            //           [n_slots][H][K][V]
    const int* slot;       // [nseq]
    const int* table;      // [n_slots][cap]
    long E;                // K V
    int n, H, nseq, cap, n_slots, n_pages;
};

// The pack prefill into h16 slots: k_bm_state<2> leaves the fp32 K^T V of a slice of the pack's chunks in the call's workspace; this
// moves each to its place.  grid (n, H, ceil(E / 8 / 64)), one wave per workgroup and 512 elements, as the h16 roll.  A finished chunk
// is encoded into the page its sequence's table row names (none: dropped), an open one is copied to Cur of its sequence's slot -- the
// destinations, and the entries that write nothing, of k_bm_state<2, StateArgsDst> (blockmix.hpp).
__global__ __launch_bounds__(64) void k_cs_page_encode(const CsEncodeArgs a) {
    const long e = ((long)blockIdx.z * 64 + threadIdx.x) * CSH_EPL;
    if (e >= a.E) return;   // (E % 64 == 0: whole groups)
    const int h = blockIdx.y, c = blockIdx.x;
    const bool whole = ld_tab1(a.tab, 2 * c + 1) == CS;
    const int seq = ld_tab1(a.dst, 2 * c), loc = ld_tab1(a.dst, 2 * c + 1);
    if ((unsigned)seq >= (unsigned)a.nseq || (whole && (unsigned)loc >= (unsigned)a.cap)) return;   // (uniform over the wave, as all below)
    const int row = ld_tab1(a.slot, seq);
    if ((unsigned)row >= (unsigned)a.n_slots) return;
    const f32x8 x = csh_ld8(a.stage + ((long)h * a.n + c) * a.E + e);
    if (!whole) {
        csh_st8(a.Cur + ((long)row * a.H + h) * a.E + e, x);
        return;
    }
    const long pg = cst_page(a.table + (long)row * a.cap, a.n_pages, loc);
    if (pg < 0) return;
    float m;
    const f16x8 pay = csh_encode(x, m);
    const long G = a.E / CSH_GROUP;
    gst<f16x8>(a.pay + (pg * a.H + h) * a.E + e, pay);
    if ((threadIdx.x & (CSH_GROUP / CSH_EPL - 1)) == 0) a.mult[(pg * a.H + h) * G + e / CSH_GROUP] = m;
}

}  // namespace mhla
