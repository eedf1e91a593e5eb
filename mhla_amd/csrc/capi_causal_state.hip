// C ABI, causal operator: the decode state of a sequence, the single-token step and the extension by T tokens
// (mhla_causal_state_init, mhla_causal_varlen_state_init, mhla_causal_step, mhla_causal_step_ragged, mhla_causal_step_dev, mhla_causal_extend, mhla_causal_extend_ragged, mhla_causal_verify_ragged, mhla_causal_commit_ragged, the grouped-query forms mhla_causal_*_gqa of the ragged entry points, their forms on chosen rows of a state pool, mhla_causal_*_slots, those on a pool whose finished chunks are pages, mhla_causal_*_paged, the extend, verify and commit on packed new tokens, mhla_causal_*_packed, the step, the device-positioned step and the pack prefill on a pool of 2-byte pages, mhla_causal_*_paged_h16, and the swap of a paged pool's slots out into one buffer and back in, mhla_causal_swap_{out,in}_paged; kernels: causal_step.hpp, causal_extend.hpp, causal_swap.hpp).  The prefill state reuses the generic path's exact-fp32 chunk products (blockmix.hpp
// k_bm_state<MODE 2>) written straight into the state's layout; the 16-bit pipeline's 11-bit summaries are never decoded.
#include "capi_common.hpp"
#include "blockmix.hpp"
#include "causal.hpp"
#include "causal_step.hpp"
#include "causal_extend.hpp"
#include "causal_swap.hpp"

using namespace mhla;
using namespace mhla::capi;

namespace {

int cst_check(int B, int H, int K, int V, int chunk, int dtype) {
    if (B <= 0 || H <= 0 || K <= 0 || V <= 0) return fail(MHLA_EINVAL, "non-positive dimension B=%d H=%d K=%d V=%d", B, H, K, V);
    if (chunk != 64) return fail(MHLA_ENOTSUP, "chunk=%d: only 64 is supported", chunk);
    if ((K | V) & 3) return fail(MHLA_EINVAL, "K=%d and V=%d must be multiples of 4", K, V);
    if (dtype < 0 || dtype > 2) return fail(MHLA_EINVAL, "unknown dtype %d", dtype);
    if ((size_t)B * H > 65535) return fail(MHLA_ENOTSUP, "B*H=%zu exceeds grid limit 65535", (size_t)B * H);
    return MHLA_OK;
}
// grouped-query heads: the state, k and v have Hkv heads, each shared by G = H / Hkv query heads (Hkv = H: the ungrouped call)
int cst_check_group(int H, int Hkv) {
    if (Hkv < 1 || H % Hkv) return fail(MHLA_EINVAL, "Hkv=%d must be positive and divide H=%d", Hkv, H);
    if (H / Hkv > CST_GMAX) return fail(MHLA_ENOTSUP, "H=%d query heads on Hkv=%d k/v heads: at most %d per k/v head are supported", H, Hkv, CST_GMAX);
    return MHLA_OK;
}
int cst_check_state(const float* S, int cap, const float* P, const float* Cur) {
    if (cap <= 0) return fail(MHLA_EINVAL, "cap_chunks=%d must be positive", cap);
    if (!S || !P || !Cur) return fail(MHLA_EINVAL, "state: S, P or Cur null");
    if (((uintptr_t)S | (uintptr_t)P | (uintptr_t)Cur) % 16) return fail(MHLA_EINVAL, "state: S, P and Cur must be 16-byte aligned");
    return MHLA_OK;
}
// what every step and extend entry point checks of its tokens, outputs and state, in this order (the parameter names are the messages')
int cst_check_io(const mhla_view& q, const mhla_view& k, const mhla_view& v, const mhla_mview& out, const mhla_mview& y, const mhla_view& gate,
                 const float* norm_w, int dtype, const float* S, int cap, const float* P, const float* Cur) {
    CHECK_VIEW(q); CHECK_VIEW(k); CHECK_VIEW(v);
    if (!out.ptr && !y.ptr) return fail(MHLA_EINVAL, "out and y both null");
    if (out.ptr) CHECK_VIEW(out);
    if (y.ptr) CHECK_VIEW(y);
    if (gate.ptr) CHECK_VIEW(gate);
    if ((gate.ptr || norm_w) && !y.ptr) return fail(MHLA_EINVAL, "gate / norm_w given without y");
    return cst_check_state(S, cap, P, Cur);
}
int cst_check_ws(const void* ws, size_t ws_bytes, size_t need) {
    if (!ws || ws_bytes < need) return ws_too_small(ws_bytes, need);
    if (((uintptr_t)ws) % 16) return fail(MHLA_EINVAL, "workspace not 16-byte aligned");
    return MHLA_OK;
}
int cst_check_dev(const char* name, const void* p) {   // an int32 array on the device
    if (!p || ((uintptr_t)p) % 4) return fail(MHLA_EINVAL, "%s null or not 4-byte aligned", name);
    return MHLA_OK;
}
// the slot map of a slotted call (the *_slots entry points): call row b works on row map[b] of a state pool of n rows; map null:
// the un-slotted namesake, row b itself
// a paged pool (the *_paged entry points) on top: the chains' `S` is then the pool of pages [n_pages][Hkv][K][V], and
// table[map[b] cap_chunks + j] names the page of chunk j of call row b; table null: S is the dense array it was
// h16 pages (the *_paged_h16 entry points) on top of that: the chains' `S` is the pool's payload, _Float16 [n_pages][Hkv][K][V], and
// mult its multipliers, float [n_pages][Hkv][K V / 64]; mult null: the pages are fp32
struct Slots {
    const int32_t* map = nullptr;
    int n = 0;
    const int32_t* table = nullptr;
    int n_pages = 0;
    float* mult = nullptr;
};
int cst_check_slots(const int32_t* slot_dev, int n_slots) {
    RC(cst_check_dev("slot_dev", slot_dev));
    if (n_slots <= 0) return fail(MHLA_EINVAL, "n_slots=%d must be positive", n_slots);
    return MHLA_OK;
}
int cst_check_pages(const float* pages, int n_pages, const int32_t* table_dev) {
    if (!pages || ((uintptr_t)pages) % 16) return fail(MHLA_EINVAL, "pages null or not 16-byte aligned");
    RC(cst_check_dev("table_dev", table_dev));
    if (n_pages <= 0) return fail(MHLA_EINVAL, "n_pages=%d must be positive", n_pages);
    return MHLA_OK;
}
// what a packed entry point checks of its nullable state arguments, and the Slots they make: off_dev is what makes the call packed,
// so it is refused here, ahead of the chain (which takes a null off_dev for a padded call)
int cst_packed_state(const float* S, int n_pages, const int32_t* table_dev, const int32_t* slot_dev, int n_slots, const int32_t* off_dev,
                     Slots& sl) {
    RC(cst_check_dev("off_dev", off_dev));
    if (table_dev) RC(cst_check_pages(S, n_pages, table_dev));
    if (slot_dev) RC(cst_check_slots(slot_dev, n_slots));
    sl = Slots{slot_dev, slot_dev ? n_slots : 0, table_dev, table_dev ? n_pages : 0};
    return MHLA_OK;
}
int cst_check_pages_h16(const void* pages_h16, const float* page_mult, int K, int V) {
    if (!pages_h16 || !page_mult) return fail(MHLA_EINVAL, "pages_h16 or page_mult null");
    if (((uintptr_t)pages_h16) % 16 || ((uintptr_t)page_mult) % 4)
        return fail(MHLA_EINVAL, "pages_h16 must be 16-byte aligned and page_mult 4-byte aligned");
    if (((long)K * V) % CSH_GROUP) return fail(MHLA_EINVAL, "K=%d V=%d: h16 pages need K*V %% %d == 0 (one multiplier per %d elements)", K, V, CSH_GROUP, CSH_GROUP);
    return MHLA_OK;
}
int cst_check_mix(const float* mix, int ldmix, int64_t lastrow) {   // lastrow: the last row of mix the call reads, up to its diagonal
    if (!mix || ldmix < lastrow + 1)
        return fail(MHLA_EINVAL, "mix null or ldmix=%d < %lld (row %lld of mix is read)", ldmix, (long long)(lastrow + 1), (long long)lastrow);
    return MHLA_OK;
}
// K rows per workgroup of k_cs_step (a multiple of 16): the whole of K where (b, h) x V tiles already give every CU four
// workgroups, otherwise halved down to 16 rows -- B H = 4 at K = 128, V = 256 runs 128 workgroups instead of 16
int cst_rows(size_t bh, int K, int V) {
    const long vt = (V + CST_VT - 1) / CST_VT, groups = (K + CST_RG - 1) / CST_RG;
    long g = groups;
    while (g > 1 && (long)bh * vt * ((groups + g - 1) / g) < 1024) g = (g + 1) / 2;
    return (int)g * CST_RG;
}
size_t cst_ws_bytes(int B, int H, int K, int V) {   // the most splits any plan uses: 16 rows each
    return al4((size_t)B * H * ((K + CST_RG - 1) / CST_RG) * V) * 4;
}

int cst_roll(float* S, int cap, float* P, float* Cur, const float* mixrow, int nj, int commit, int BH, long E, hipStream_t st) {
    const CsRollArgs r{S, P, Cur, mixrow, E, cap, nj, commit};
    return launch(k_cs_roll<false>, dim3((unsigned)((E / 4 + 63) / 64), BH), dim3(64), 0, st, "k_cs_roll", r);
}
// the roll of a ragged state: each sequence for itself, by pos_dev (the position of the token its step just took)
int cst_roll_ragged(float* S, int cap, float* P, float* Cur, const int32_t* pos_dev, Slots sl, const float* mix, int ldmix, int max_pos, int H,
                    int BH, long E, hipStream_t st) {
    const CsRollArgs r{S, P, Cur, nullptr, E, cap, 0, 0, pos_dev, mix, ldmix, max_pos, H, sl.map, sl.n, sl.table, sl.n_pages, (_Float16*)S, sl.mult};
    if (sl.mult)   // (h16 pages: 8 elements a lane)
        return launch(k_cs_roll<true, false, true, true, PF_H16>, dim3((unsigned)((E / CSH_EPL + 63) / 64), BH), dim3(64), 0, st, "k_cs_roll_ragged<h16>", r);
    return launch(sl.table ? k_cs_roll<true, false, true, true> : sl.map ? k_cs_roll<true, false, true> : k_cs_roll<true>, dim3((unsigned)((E / 4 + 63) / 64), BH), dim3(64), 0, st,
                  "k_cs_roll_ragged", r);
}
int cst_zero_cur(float* Cur, int BH, long E, hipStream_t st) {
    hipError_t e = hipMemsetAsync(Cur, 0, (size_t)BH * E * 4, st);
    if (e != hipSuccess) return fail(MHLA_ELAUNCH, "hipMemsetAsync(Cur): %s", hipGetErrorString(e));
    return MHLA_OK;
}
// one launch of a k_cs_step variant: fills in the K split (s.kr rows per workgroup, s.nsplit partial sums per output, which the finish adds)
// BH counts the query heads, G of which share a workgroup (s.H: the k/v heads): the split is the one of the ungrouped call on
// repeated heads, so that every sum has its terms and its order
template <typename KERN>
int cst_step(KERN kernel, const char* name, CsStepArgs& s, int BH, hipStream_t st, int G = 1) {
    s.G = G;
    s.kr = cst_rows((size_t)BH, s.K, s.V);
    s.nsplit = (s.K + s.kr - 1) / s.kr;
    return launch(kernel, dim3((s.V + CST_VT - 1) / CST_VT, s.nsplit, BH / G), dim3(CST_THREADS), 0, st, name, s);
}

template <typename T>
int cst_xty(const mhla_view& k, const mhla_view& v, long tok0, long ntok, float* out, int stride_chunks, int B, int H, int K, int V,
            hipStream_t st) {
    StateArgs a{};
    a.x = cv(k); a.y = cv(v);
    a.x.ptr = (const T*)k.ptr + tok0 * k.sn;
    a.y.ptr = (const T*)v.ptr + tok0 * v.sn;
    a.out = out; a.H = H; a.M = stride_chunks; a.S = CS; a.D = 64; a.DX = K; a.DY = V; a.T = ntok; a.alpha = 1.f;
    const int strips = ((K + 63) / 64) * ((V + 63) / 64);
    return launch(k_bm_state<T, 4, 2>, dim3((unsigned)((ntok + CS - 1) / CS), B * H, strips), dim3(NTHREADS), state_smem_floats<4>() * 4, st,
                  "k_bm_state<2>", a);
}

// the chunks of a pack (B = 1), each tile into its sequence's state: a whole chunk to S[seq][h][loc], a ragged one to Cur[seq][h]
template <typename T>
int cst_xty_pack(const mhla_view& k, const mhla_view& v, float* S, int cap, float* Cur, int n_seqs, int n_chunks, const int* tab, const int* dst,
                 Slots sl, int T_, int H, int K, int V, hipStream_t st) {
    StateArgsDst a{};
    a.x = cv(k); a.y = cv(v);
    a.H = H; a.M = 0; a.S = CS; a.D = 64; a.DX = K; a.DY = V; a.T = T_; a.alpha = 1.f;
    a.tab = (const tab2_t*)tab; a.dst = dst; a.Sq = S; a.Cur = Cur; a.nseq = n_seqs; a.cap = cap;
    a.slot = sl.map; a.n_slots = sl.n; a.table = sl.table; a.n_pages = sl.n_pages;
    const int strips = ((K + 63) / 64) * ((V + 63) / 64);
    return launch(k_bm_state<T, 4, 2, StateArgsDst>, dim3((unsigned)n_chunks, H, strips), dim3(NTHREADS), state_smem_floats<4>() * 4, st,
                  "k_bm_state<2,dst>", a);
}

// h16 pages: the chunks [c0, c0 + n) of a pack's chunk list (B = 1), fp32, into the staging area [H][n][K][V] -- the tiles of
// cst_xty_pack, each at its place in the list instead of its place in a state
template <typename T>
int cst_xty_stage(const mhla_view& k, const mhla_view& v, float* stage, int n, const int* tab, int T_, int H, int K, int V, hipStream_t st) {
    StateArgsVar a{};
    a.x = cv(k); a.y = cv(v);
    a.out = stage; a.H = H; a.M = n; a.S = CS; a.D = 64; a.DX = K; a.DY = V; a.T = T_; a.alpha = 1.f;
    a.tab = (const tab2_t*)tab;
    const int strips = ((K + 63) / 64) * ((V + 63) / 64);
    return launch(k_bm_state<T, 4, 2, StateArgsVar>, dim3((unsigned)n, H, strips), dim3(NTHREADS), state_smem_floats<4>() * 4, st,
                  "k_bm_state<2,stage>", a);
}

// the extension's workspace, in floats: P_c of every chunk touched after the first, then the fp32 rows the epilogue reads
struct CxPlan {
    int64_t i, ilast, iend;   // chunk of the first / last new token, chunk open after the extension
    int r, a, nws;            // tokens in the open chunk, rows of the first segment, chunks touched after the first
    size_t tiles, stage, total;
};
CxPlan cx_plan(int B, int T, int H, int K, int V, int64_t pos) {
    CxPlan p{};
    p.i = pos / CS; p.r = (int)(pos - p.i * CS);
    p.a = T < CS - p.r ? T : CS - p.r;
    p.ilast = (pos + T - 1) / CS; p.iend = (pos + T) / CS;
    p.nws = (int)(p.ilast - p.i);
    p.tiles = al4((size_t)B * H * p.nws * K * V);
    p.stage = al4((size_t)B * H * T * V);
    p.total = p.tiles + p.stage;
    return p;
}

// the ragged extension's workspace, in floats: P_c tiles with the batch maximum of later chunks as the stride per (b, h), the fp32
// rows of every padded token, and nval[B] (int32)
struct CxRagPlan {
    size_t tiles, stage, nval, total;
};
// packed: T counts the tokens of the whole pack and the rows are [H][T][V], not [B H][T][V]
CxRagPlan cx_rag_plan(int B, int T, int H, int Hkv, int K, int V, int max_later, bool packed = false) {   // (tiles per k/v head, rows per query head)
    CxRagPlan p{};
    p.tiles = al4((size_t)B * Hkv * max_later * K * V);
    p.stage = al4((size_t)(packed ? 1 : B) * H * T * V);
    p.nval = al4((size_t)B);
    p.total = p.tiles + p.stage + p.nval;
    return p;
}

// what the ragged entry points check of the host values that vouch for the device arrays, and of the rows of mix they let be read
// (a packed call: off_dev where the padded one has ntok_dev, T the tokens of the pack)
int cx_rag_check(int T, int cap_chunks, const int32_t* pos_dev, const int32_t* ntok_dev, const int32_t* off_dev, int64_t max_end, int max_later,
                 int any_close, const float* mix, int ldmix) {
    if (cap_chunks > INT32_MAX / 64) return fail(MHLA_ENOTSUP, "cap_chunks=%d: positions beyond int32", cap_chunks);
    RC(cst_check_dev("pos_dev", pos_dev));
    if (off_dev) RC(cst_check_dev("off_dev", off_dev));
    else RC(cst_check_dev("ntok_dev", ntok_dev));
    if (max_end < 0) return fail(MHLA_EINVAL, "max_end=%lld is negative", (long long)max_end);
    if (max_end > (int64_t)64 * cap_chunks)
        return fail(MHLA_EINVAL, "max_end=%lld tokens need %lld chunks, the state holds %d", (long long)max_end, (long long)((max_end + 63) / 64), cap_chunks);
    if (max_later < 0 || max_later > (T + 62) / 64)
        return fail(MHLA_EINVAL, "max_later=%d: T=%d tokens touch at most %d chunks after the first", max_later, T, (T + 62) / 64);
    if (max_later && !any_close) return fail(MHLA_EINVAL, "max_later=%d without any_close", max_later);
    // rows of mix read: every sequence's diagonal up to chunk (its end - 1) / 64 and, where it closes a chunk and is not full then, row
    // (its end) / 64.  Which sequence closes is known on the device only: with any_close row max_end / 64 must be covered (or
    // the state's last), as if the furthest sequence were the one -- the restriction of mhla_causal_step_ragged
    const int64_t lastrow = any_close ? std::min<int64_t>(max_end / 64, cap_chunks - 1) : (max_end > 0 ? (max_end - 1) / 64 : 0);
    return cst_check_mix(mix, ldmix, lastrow);
}

// the ragged extend chain; dry (the verify): the same launches, nothing of the committed state -- Cur, P, pos_dev -- written
// Hkv < H (grouped-query heads): the launches that form or move state run over the B Hkv k/v heads, the two that compute rows
// (k_cx_out, the finish) over the B H query heads
// off_dev (the packed entry points; ntok_dev null, left_padded 0): the tokens are ONE run of T rows, sequence b's [off_dev[b], off_dev[b + 1]),
// the views come with sb = 0, the rows are staged [H][T][V] and the finish runs over (H, T)
int cx_ragged_chain(bool dry, mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                    float* Cur, int32_t* pos_dev, Slots sl, const int32_t* ntok_dev, const int32_t* off_dev, int T, int64_t max_end,
                    int max_later, int any_close, int left_padded, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                    mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk, float scale, int dtype,
                    void* stream) {
    RC(cst_check(B, H, K, V, chunk, dtype));
    RC(cst_check_group(H, Hkv));
    if (T <= 0) return fail(MHLA_EINVAL, "%s=%d must be positive", off_dev ? "n_tokens" : "T", T);
    if (T > 65535) return fail(MHLA_EINVAL, "%s=%d exceeds 65535 tokens per call", off_dev ? "n_tokens" : "T", T);   // (mhla_causal_extend answers MHLA_ENOTSUP here: kept, a caller may test the code)
    RC(cst_check_io(q, k, v, out, y, gate, norm_w, dtype, S, cap_chunks, P, Cur));
    RC(cx_rag_check(T, cap_chunks, pos_dev, ntok_dev, off_dev, max_end, max_later, any_close, mix, ldmix));
    const CxRagPlan p = cx_rag_plan(B, T, H, Hkv, K, V, max_later, off_dev != nullptr);
    RC(cst_check_ws(ws, ws_bytes, p.total * 4));
    hipStream_t st = (hipStream_t)stream;
    const int BH = B * H, BHk = B * Hkv, nvt = (V + 63) / 64, strips = ((K + 63) / 64) * nvt;
    const long E = (long)K * V;
    float* tiles = (float*)ws;
    float* stage = tiles + p.tiles;
    int* nval = (int*)(stage + p.stage);
    const CxRag g{pos_dev, ntok_dev, T, cap_chunks, (int)max_end, max_later, any_close ? 1 : 0, left_padded ? 1 : 0, dry ? 1 : 0, nullptr,
                  sl.map, sl.n, sl.table, sl.n_pages, off_dev};
    const int kr = cst_rows((size_t)H, K, V);   // a one-token sequence: the step's K split for a batch of one
    const bool pk = off_dev != nullptr;   // (the kernels' PACKED instantiations; the padded ones are the code they were)
    // every launch but the last addresses by pos_dev; the last, which does not, advances it (dry: does not)
    DISPATCH_T(dtype, {
        CxOutArgs o{};
        o.q = cv(q); o.k = cv(k); o.v = cv(v);
        o.stage = stage; o.H = H; o.K = K; o.V = V; o.T = T; o.scale = scale; o.mstep = (long)ldmix + 1;
        o.P = P; o.Cur = Cur; o.mdiag = mix; o.rag = g; o.later = 0; o.nval = nval; o.kr = kr; o.nsplit = (K + kr - 1) / kr;
        o.G = H / Hkv;
        RC(launch(pk ? k_cx_out<ET, true, true> : k_cx_out<ET, true>, dim3(1, BH, nvt), dim3(NTHREADS), CS_OUT_SMEM_FLOATS * 4, st, "k_cx_out_ragged", o));
        CxAccArgs c{};
        c.x = cv(k); c.y = cv(v); c.H = Hkv; c.DX = K; c.DY = V; c.rag = g; c.later = 0; c.S = S; c.Cur = Cur;
        RC(launch(pk ? k_cx_xty_acc<ET, true, true> : k_cx_xty_acc<ET, true>, dim3(1, BHk, strips), dim3(NTHREADS), 0, st, "k_cx_xty_acc_ragged", c));
        if (any_close) {
            c.later = 1;
            RC(launch(pk ? k_cx_xty_acc<ET, true, true> : k_cx_xty_acc<ET, true>, dim3(std::max(1, max_later), BHk, strips), dim3(NTHREADS), 0, st,
                      "k_cx_xty_acc_ragged", c));
            CxMixRagArgs m{};
            m.m.S = S; m.m.ws = tiles; m.m.P = P; m.m.mix = mix; m.m.E = E; m.m.ldmix = ldmix; m.m.cap = cap_chunks;
            m.rag = g; m.H = Hkv;
            const int groups = (max_later + 1 + CX_MIX_NC - 1) / CX_MIX_NC;   // (the largest nc is max_later + 1)
            RC(launch(pk ? k_cx_mix_ragged<true> : k_cx_mix_ragged<>, dim3((unsigned)((E / 4 + 63) / 64), BHk, groups), dim3(64), 0, st, "k_cx_mix_ragged", m));
            if (max_later) {
                o.P = tiles; o.Cur = nullptr; o.later = 1;
                RC(launch(pk ? k_cx_out<ET, true, true> : k_cx_out<ET, true>, dim3(max_later, BH, nvt), dim3(NTHREADS), CS_OUT_SMEM_FLOATS * 4, st,
                          "k_cx_out_ragged", o));
            }
        }
        CsFinishArgs f{stage, cmv(out), cmv(y), cv(gate), norm_w, norm_eps, scale, H, V, 1, dry ? nullptr : pos_dev};
        f.nval = nval; f.left = left_padded ? 1 : 0; f.slot = sl.map; f.n_slots = sl.n;
        if (pk) {
            f.off = off_dev; f.nseq = B;
            RC(launch(sl.map ? k_cs_step_finish<ET, false, true, true, false, true> : k_cs_step_finish<ET, false, true, false, false, true>,
                      dim3(H, T), dim3(CST_THREADS), 0, st, "k_cs_step_finish_packed", f));
        } else {
            RC(launch(sl.map ? k_cs_step_finish<ET, false, true, true> : k_cs_step_finish<ET, false, true>, dim3(BH, T), dim3(CST_THREADS), 0, st,
                      "k_cs_step_finish_ragged", f));
        }
    });
    return MHLA_OK;
}

// the ragged step chain (step, roll, finish); Hkv < H (grouped-query heads): step and roll run over the B Hkv k/v heads, the step
// writing the partial sums of all B H query heads, which the finish reads as ever
int cs_step_ragged_chain(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                         float* Cur, int32_t* pos_dev, Slots sl, int64_t max_pos, int any_boundary, mhla_mview out, mhla_view gate,
                         const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V,
                         int chunk, float scale, int dtype, void* stream) {
    RC(cst_check(B, H, K, V, chunk, dtype));
    RC(cst_check_group(H, Hkv));
    RC(cst_check_io(q, k, v, out, y, gate, norm_w, dtype, S, cap_chunks, P, Cur));
    RC(cst_check_dev("pos_dev", pos_dev));
    if (max_pos < 0 || max_pos >= INT32_MAX) return fail(MHLA_EINVAL, "max_pos=%lld is negative or beyond int32", (long long)max_pos);
    const int64_t i = max_pos / chunk;
    if (i >= cap_chunks) return fail(MHLA_EINVAL, "max_pos=%lld is in chunk %lld, the state holds %d", (long long)max_pos, (long long)i, cap_chunks);
    // which sequence is on a boundary is known on the device only: with any_boundary the row after the furthest sequence's chunk
    // must be covered (unless that chunk is the state's last), as if that sequence were the one -- a restriction (mhla_hip.h):
    // the matrix passed with a boundary step reaches one row past the furthest sequence, or the state's capacity
    const bool next = any_boundary && i + 1 < cap_chunks;
    RC(cst_check_mix(mix, ldmix, i + (next ? 1 : 0)));
    RC(cst_check_ws(ws, ws_bytes, cst_ws_bytes(B, H, K, V)));
    hipStream_t st = (hipStream_t)stream;
    const int BH = B * H, G = H / Hkv;
    // step and roll address by pos_dev; the finish, which does not, advances it: last in the chain
    DISPATCH_T(dtype, {
        CsStepArgs s{cv(q), cv(k), cv(v), mix, P, Cur, (float*)ws, Hkv, K, V, 0, 0, pos_dev, ldmix, (int)max_pos};
        s.slot = sl.map; s.n_slots = sl.n;
        // (a slotted call: the kernels' SLOT instantiations; the un-slotted ones are the code they were)
        if (G == 1) RC(cst_step(sl.map ? k_cs_step<ET, true, false, false, 1, true> : k_cs_step<ET, true>, "k_cs_step_ragged", s, BH, st));
        else        RC(cst_step(sl.map ? k_cs_step<ET, true, false, false, CST_GMAX, true> : k_cs_step<ET, true, false, false, CST_GMAX>,
                                "k_cs_step_ragged<gqa>", s, BH, st, G));
        if (any_boundary) RC(cst_roll_ragged(S, cap_chunks, P, Cur, pos_dev, sl, mix, ldmix, (int)max_pos, Hkv, B * Hkv, (long)K * V, st));
        CsFinishArgs f{(const float*)ws, cmv(out), cmv(y), cv(gate), norm_w, norm_eps, scale, H, V, s.nsplit, pos_dev};
        f.slot = sl.map; f.n_slots = sl.n;
        RC(launch(sl.map ? k_cs_step_finish<ET, false, false, true> : k_cs_step_finish<ET>, dim3(BH), dim3(CST_THREADS), 0, st, "k_cs_step_finish", f));
    });
    return MHLA_OK;
}

// the device-positioned step's kernel: un-slotted, slotted, or slotted on a paged pool (each instantiation the code it was)
template <typename ET, bool PRO, int GM>
auto cs_dev_step_kernel(const Slots& sl) {
    return sl.table ? k_cs_step<ET, true, true, PRO, GM, true, true> : sl.map ? k_cs_step<ET, true, true, PRO, GM, true> : k_cs_step<ET, true, true, PRO, GM>;
}

// the device-positioned step chain; Hkv < H as in cs_step_ragged_chain (the fused prologue: k once per k/v head, q per query head)
int cs_step_dev_chain(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                      float* Cur, int32_t* pos_dev, Slots sl, int32_t* full_dev, const void* rope_cos, const void* rope_sin, int64_t ld_tab,
                      int64_t tab_rows, int feature_map, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                      mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk, float scale, int dtype,
                      void* stream) {
    RC(cst_check(B, H, K, V, chunk, dtype));
    RC(cst_check_group(H, Hkv));
    RC(cst_check_io(q, k, v, out, y, gate, norm_w, dtype, S, cap_chunks, P, Cur));
    if (cap_chunks > INT32_MAX / 64) return fail(MHLA_ENOTSUP, "cap_chunks=%d: positions beyond int32", cap_chunks);
    RC(cst_check_dev("pos_dev", pos_dev));
    RC(cst_check_dev("full_dev", full_dev));
    // every bound is the capacity: whichever chunk a sequence is in, rows and columns 0 .. cap_chunks - 1 of mix may be read
    if (!mix || ldmix < cap_chunks)
        return fail(MHLA_EINVAL, "mix null or ldmix=%d < cap_chunks=%d (the matrix is read up to row %d)", ldmix, cap_chunks, cap_chunks - 1);
    if (feature_map < 0 || feature_map > 2) return fail(MHLA_EINVAL, "feature_map %d: 0 identity, 1 relu, 2 elu+1", feature_map);
    if (!rope_cos != !rope_sin) return fail(MHLA_EINVAL, "rope_cos and rope_sin must be given together");
    const bool pro = rope_cos || feature_map;
    if (pro && (K & 7)) return fail(MHLA_EINVAL, "K=%d: the fused prologue needs K %% 8 == 0", K);
    if (rope_cos) {
        if (ld_tab < K / 2 || (ld_tab & 3)) return fail(MHLA_EINVAL, "cos/sin tables: ld_tab=%lld < K/2 or not a multiple of 4", (long long)ld_tab);
        const size_t al = dtype == MHLA_F32 ? 16 : 8;
        if (((uintptr_t)rope_cos | (uintptr_t)rope_sin) % al) return fail(MHLA_EINVAL, "cos/sin tables must be %zu-byte aligned", al);
        if (tab_rows < (int64_t)64 * cap_chunks || tab_rows > INT32_MAX)
            return fail(MHLA_EINVAL, "tab_rows=%lld: the tables need a row per position, %lld (64 cap_chunks)", (long long)tab_rows, (long long)64 * cap_chunks);
    }
    RC(cst_check_ws(ws, ws_bytes, cst_ws_bytes(B, H, K, V)));
    hipStream_t st = (hipStream_t)stream;
    const int BH = B * H, G = H / Hkv, max_pos = 64 * cap_chunks - 1;
    // always the same three launches, none of whose arguments depends on a position: step and roll address by pos_dev, the
    // finish -- one thread per sequence reads it, none else -- advances it or sets full_dev
    DISPATCH_T(dtype, {
        CsStepArgs s{cv(q), cv(k), cv(v), mix, P, Cur, (float*)ws, Hkv, K, V, 0, 0, pos_dev, ldmix, max_pos,
                     rope_cos, rope_sin, (long)ld_tab, (int)tab_rows, feature_map};
        s.slot = sl.map; s.n_slots = sl.n; s.table = sl.table; s.tcap = cap_chunks; s.n_pages = sl.n_pages;
        if (G == 1) {
            if (pro) RC(cst_step(cs_dev_step_kernel<ET, true, 1>(sl), "k_cs_step_dev<pro>", s, BH, st));
            else     RC(cst_step(cs_dev_step_kernel<ET, false, 1>(sl), "k_cs_step_dev", s, BH, st));
        } else {
            if (pro) RC(cst_step(cs_dev_step_kernel<ET, true, CST_GMAX>(sl), "k_cs_step_dev<pro,gqa>", s, BH, st, G));
            else     RC(cst_step(cs_dev_step_kernel<ET, false, CST_GMAX>(sl), "k_cs_step_dev<gqa>", s, BH, st, G));
        }
        RC(cst_roll_ragged(S, cap_chunks, P, Cur, pos_dev, sl, mix, ldmix, max_pos, Hkv, B * Hkv, (long)K * V, st));
        CsFinishArgs f{(const float*)ws, cmv(out), cmv(y), cv(gate), norm_w, norm_eps, scale, H, V, s.nsplit, pos_dev, max_pos, full_dev};
        f.slot = sl.map; f.n_slots = sl.n; f.table = sl.table; f.tcap = cap_chunks; f.n_pages = sl.n_pages;
        RC(launch(sl.table ? k_cs_step_finish<ET, true, false, true, true>
                  : sl.map ? k_cs_step_finish<ET, true, false, true> : k_cs_step_finish<ET, true>, dim3(BH), dim3(CST_THREADS), 0, st,
                  "k_cs_step_finish_dev", f));
    });
    return MHLA_OK;
}

// the pack prefill chain (the chunks' K^T V into their sequences' states, then every sequence's prefix mix); slotted: sequence s of the
// pack into row sl.map[s] of the pool -- S, P and Cur of those rows only, seq_len_dev stays indexed by s
int cs_pack_chain(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur, int n_seqs,
                  const int32_t* seq_len_dev, Slots sl, int max_len, int T, int H, int K, int V, int chunk, int n_chunks,
                  const int32_t* chunk_tab_dev, const int32_t* chunk_dst_dev, void* ws, size_t ws_bytes, int dtype, void* stream) {
    RC(cst_check(1, H, K, V, chunk, dtype));
    if (n_seqs <= 0) return fail(MHLA_EINVAL, "n_seqs=%d must be positive", n_seqs);
    if ((size_t)n_seqs * H > 65535) return fail(MHLA_ENOTSUP, "n_seqs*H=%zu exceeds grid limit 65535", (size_t)n_seqs * H);
    if (T <= 0 || n_chunks <= 0) return fail(MHLA_EINVAL, "T=%d n_chunks=%d must be positive (an all-empty pack is an all-zero state)", T, n_chunks);
    CHECK_VIEW(k); CHECK_VIEW(v);
    RC(cst_check_state(S, cap_chunks, P, Cur));
    if (n_chunks < (T + chunk - 1) / chunk || n_chunks > T)
        return fail(MHLA_EINVAL, "n_chunks=%d outside ceil(T / %d)=%d .. T=%d", n_chunks, chunk, (T + chunk - 1) / chunk, T);
    if (max_len < 0 || max_len > T) return fail(MHLA_EINVAL, "max_len=%d outside 0 .. T=%d", max_len, T);
    if ((max_len + chunk - 1) / chunk > cap_chunks)
        return fail(MHLA_EINVAL, "max_len=%d tokens need %d chunks, the state holds %d", max_len, (max_len + chunk - 1) / chunk, cap_chunks);
    // sequence s reads row len[s] / 64 of mix up to its diagonal unless its state is then full: the longest one's row covers all
    RC(cst_check_mix(mix, ldmix, std::min(max_len / chunk, cap_chunks - 1)));
    RC(cst_check_dev("seq_len_dev", seq_len_dev));
    RC(cst_check_dev("chunk_dst_dev", chunk_dst_dev));
    if (!chunk_tab_dev || ((uintptr_t)chunk_tab_dev) % 8) return fail(MHLA_EINVAL, "chunk_tab_dev null or not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long E = (long)K * V;
    const CsRollArgs r{S, P, Cur, nullptr, E, cap_chunks, 0, 0, seq_len_dev, mix, ldmix, max_len, H, sl.map, sl.n, sl.table, sl.n_pages, (_Float16*)S, sl.mult};
    if (sl.mult) {
        // h16 pages: the chunks' fp32 K^T V staged in the workspace, then encoded into their pages (open chunks copied to Cur), over
        // slices of the chunk list of as many chunks as the workspace holds; the roll once at the end
        const size_t per = (size_t)H * E * 4;
        RC(cst_check_ws(ws, ws_bytes, per));
        const int fit = (int)std::min<size_t>((size_t)n_chunks, ws_bytes / per);
        for (int c0 = 0; c0 < n_chunks; c0 += fit) {
            const int n = std::min(fit, n_chunks - c0);
            DISPATCH_T(dtype, { RC(cst_xty_stage<ET>(k, v, (float*)ws, n, chunk_tab_dev + 2 * c0, T, H, K, V, st)); });
            const CsEncodeArgs en{(const float*)ws, chunk_tab_dev + 2 * c0, chunk_dst_dev + 2 * c0, (_Float16*)S, sl.mult, Cur, sl.map, sl.table, E,
                                  n, H, n_seqs, cap_chunks, sl.n, sl.n_pages};
            RC(launch(k_cs_page_encode, dim3((unsigned)n, H, (unsigned)((E / CSH_EPL + 63) / 64)), dim3(64), 0, st, "k_cs_page_encode", en));
        }
        return launch(k_cs_roll<false, true, true, true, PF_H16>, dim3((unsigned)((E / CSH_EPL + 63) / 64), n_seqs * H), dim3(64), 0, st,
                      "k_cs_roll_pack<h16>", r);
    }
    DISPATCH_T(dtype, { RC(cst_xty_pack<ET>(k, v, S, cap_chunks, Cur, n_seqs, n_chunks, chunk_tab_dev, chunk_dst_dev, sl, T, H, K, V, st)); });
    return launch(sl.table ? k_cs_roll<false, true, true, true> : sl.map ? k_cs_roll<false, true, true> : k_cs_roll<false, true>, dim3((unsigned)((E / 4 + 63) / 64), n_seqs * H), dim3(64), 0, st,
                  "k_cs_roll_pack", r);
}

// the commit chain: the state half of the ragged extend on the accepted tokens, no q and no rows (H: the k/v heads); off_dev: as
// cx_ragged_chain's
int cx_commit_chain(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur, int32_t* pos_dev,
                    Slots sl, const int32_t* ntok_dev, const int32_t* off_dev, const int32_t* accept_dev, int T, int64_t max_end, int max_later,
                    int any_close, int left_padded, void* ws, size_t ws_bytes, int B, int H, int K, int V, int chunk, int dtype, void* stream) {
    RC(cst_check(B, H, K, V, chunk, dtype));
    if (T <= 0) return fail(MHLA_EINVAL, "%s=%d must be positive", off_dev ? "n_tokens" : "T", T);
    if (T > 65535) return fail(MHLA_EINVAL, "%s=%d exceeds 65535 tokens per call", off_dev ? "n_tokens" : "T", T);
    CHECK_VIEW(k); CHECK_VIEW(v);
    RC(cst_check_state(S, cap_chunks, P, Cur));
    RC(cst_check_dev("accept_dev", accept_dev));
    RC(cx_rag_check(T, cap_chunks, pos_dev, ntok_dev, off_dev, max_end, max_later, any_close, mix, ldmix));
    RC(cst_check_ws(ws, ws_bytes, al4((size_t)B) * 4));
    hipStream_t st = (hipStream_t)stream;
    const int BH = B * H, strips = ((K + 63) / 64) * ((V + 63) / 64);
    const long E = (long)K * V;
    int* nval = (int*)ws;
    const bool pk = off_dev != nullptr;
    const CxRag g{pos_dev, ntok_dev, T, cap_chunks, (int)max_end, max_later, any_close ? 1 : 0, left_padded ? 1 : 0, 0, accept_dev, sl.map, sl.n, sl.table,
                  sl.n_pages, off_dev};
    // every launch but the last addresses by pos_dev; the last, which does not, advances it
    DISPATCH_T(dtype, {
        CxAccArgs c{};
        c.x = cv(k); c.y = cv(v); c.H = H; c.DX = K; c.DY = V; c.rag = g; c.later = 0; c.S = S; c.Cur = Cur; c.nval = nval;
        RC(launch(pk ? k_cx_xty_acc<ET, true, true> : k_cx_xty_acc<ET, true>, dim3(1, BH, strips), dim3(NTHREADS), 0, st, "k_cx_xty_acc_ragged", c));
        if (any_close) {
            c.later = 1;
            RC(launch(pk ? k_cx_xty_acc<ET, true, true> : k_cx_xty_acc<ET, true>, dim3(std::max(1, max_later), BH, strips), dim3(NTHREADS), 0, st,
                      "k_cx_xty_acc_ragged", c));
            CxMixRagArgs m{};
            m.m.S = S; m.m.ws = nullptr; m.m.P = P; m.m.mix = mix; m.m.E = E; m.m.ldmix = ldmix; m.m.cap = cap_chunks;
            m.rag = g; m.H = H;
            RC(launch(pk ? k_cx_mix_ragged<true> : k_cx_mix_ragged<>, dim3((unsigned)((E / 4 + 63) / 64), BH, 1), dim3(64), 0, st, "k_cx_mix_ragged", m));
        }
    });
    return launch(k_cx_advance, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, "k_cx_advance", pos_dev, (const int*)nval, B, sl.map, sl.n);
}

// the two directions of a swap (OUT: pool -> blob): the checks, then one launch of k_cs_swap over the items [i0, i1), whose first
// begins at `blob`.  mult null: fp32 pages
template <bool OUT>
int cs_swap(void* pages, float* mult, int n_pages, float* P, float* Cur, int32_t* pos_dev, int32_t* full_dev, int n_slots, const int32_t* items_dev,
            int n_seqs, int n_moved, int i0, int i1, void* blob, int Hkv, int K, int V, void* stream) {
    if (Hkv <= 0 || K <= 0 || V <= 0 || n_pages <= 0 || n_slots <= 0)
        return fail(MHLA_EINVAL, "non-positive size Hkv=%d K=%d V=%d n_pages=%d n_slots=%d", Hkv, K, V, n_pages, n_slots);
    if (((long)K * V) % 4) return fail(MHLA_EINVAL, "K=%d V=%d: K*V must be a multiple of 4 (16-byte pieces)", K, V);
    if (mult && ((long)K * V) % CSH_GROUP) return fail(MHLA_EINVAL, "K=%d V=%d: h16 pages need K*V %% %d == 0 (one multiplier per %d elements)", K, V, CSH_GROUP, CSH_GROUP);
    if (!pages || !P || !Cur || !blob) return fail(MHLA_EINVAL, "pages, P, Cur or the blob null");
    if (((uintptr_t)pages | (uintptr_t)P | (uintptr_t)Cur | (uintptr_t)blob) % 16) return fail(MHLA_EINVAL, "pages, P, Cur and the blob must be 16-byte aligned");
    if (mult) RC(cst_check_dev("page_mult", mult));
    RC(cst_check_dev("pos_dev", pos_dev));
    if (full_dev) RC(cst_check_dev("full_dev", full_dev));
    RC(cst_check_dev("items_dev", items_dev));
    if (n_seqs < 0 || n_moved < 0 || (long)n_seqs + n_moved > 0x7fffffffL) return fail(MHLA_EINVAL, "n_seqs=%d and n_pages_moved=%d must not be negative", n_seqs, n_moved);
    if (i0 < 0 || i1 < i0 || i1 > n_seqs + n_moved)
        return fail(MHLA_EINVAL, "items [%d, %d) are outside the list of %d sequences and %d pages", i0, i1, n_seqs, n_moved);
    if (i0 == i1) return MHLA_OK;
    const int fmt = mult ? PF_H16 : PF_F32;
    const CsSwapLayout l = cs_swap_layout(Hkv, K, V, fmt);
    const CsSwapArgs a{(char*)blob, items_dev, i0, i1, n_seqs, (char*)pages, mult, n_pages, P, Cur, pos_dev, full_dev, n_slots,
                       l.state_pieces, l.pay_pieces, l.n_mult, l.n_mult_pad, l.seq_bytes, l.page_bytes};
    // memory-bound: about 2048 workgroups at the most, the rest grid-strided -- x over the 16-byte pieces of an item, four to a lane of the
    // smaller kind of item in the range (the four requests cs_swap_run keeps in flight; the larger kind takes more rounds), y over items
    const long pieces = std::min(i0 < n_seqs ? l.state_pieces : l.pay_pieces, i1 > n_seqs ? l.pay_pieces : l.state_pieces);
    const unsigned gx = (unsigned)std::min<long>((pieces + 1023) / 1024, 2048);
    const unsigned gy = (unsigned)std::min<long>(i1 - i0, std::max<long>(1, 2048 / gx));
    const hipStream_t st = (hipStream_t)stream;
    if (mult) return launch(k_cs_swap<OUT, PF_H16>, dim3(gx, gy), dim3(256), 0, st, OUT ? "k_cs_swap<out,h16>" : "k_cs_swap<in,h16>", a);
    return launch(k_cs_swap<OUT, PF_F32>, dim3(gx, gy), dim3(256), 0, st, OUT ? "k_cs_swap<out>" : "k_cs_swap<in>", a);
}

}  // namespace

extern "C" {

size_t mhla_causal_step_ws_bytes(int B, int H, int K, int V, int dtype) {
    (void)dtype;
    if (B <= 0 || H <= 0 || K <= 0 || V <= 0) return 0;
    return cst_ws_bytes(B, H, K, V);
}

int mhla_causal_state_init(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                           int B, int T, int H, int K, int V, int chunk, int dtype, void* stream) {
    RC(cst_check(B, H, K, V, chunk, dtype));
    if (T <= 0) return fail(MHLA_EINVAL, "T=%d must be positive (an empty state is all zeros)", T);
    CHECK_VIEW(k); CHECK_VIEW(v);
    RC(cst_check_state(S, cap_chunks, P, Cur));
    const int nfull = T / chunk, tail = T - nfull * chunk;
    if (nfull + (tail ? 1 : 0) > cap_chunks) return fail(MHLA_EINVAL, "T=%d tokens need %d chunks, the state holds %d", T, nfull + (tail ? 1 : 0), cap_chunks);
    // the open chunk i = nfull reads mix[i][0 .. i]; a state that is full (nfull == cap_chunks) has no open chunk
    const bool open = nfull < cap_chunks;
    if (open) RC(cst_check_mix(mix, ldmix, nfull));
    hipStream_t st = (hipStream_t)stream;
    const long E = (long)K * V;
    DISPATCH_T(dtype, {
        if (nfull) RC(cst_xty<ET>(k, v, 0, (long)nfull * chunk, S, cap_chunks, B, H, K, V, st));
        if (tail)  RC(cst_xty<ET>(k, v, (long)nfull * chunk, tail, Cur, 1, B, H, K, V, st));
    });
    if (!tail) RC(cst_zero_cur(Cur, B * H, E, st));
    return cst_roll(S, cap_chunks, P, Cur, open ? mix + (long)nfull * ldmix : nullptr, nfull, 0, B * H, E, st);
}

int mhla_causal_varlen_state_init(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                                  int n_seqs, const int32_t* seq_len_dev, int max_len, int T, int H, int K, int V, int chunk, int n_chunks,
                                  const int32_t* chunk_tab_dev, const int32_t* chunk_dst_dev, int dtype, void* stream) {
    return cs_pack_chain(k, v, mix, ldmix, S, cap_chunks, P, Cur, n_seqs, seq_len_dev, Slots{}, max_len, T, H, K, V, chunk, n_chunks, chunk_tab_dev,
                         chunk_dst_dev, nullptr, 0, dtype, stream);
}

int mhla_causal_varlen_state_init_slots(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                                        int n_seqs, const int32_t* seq_len_dev, const int32_t* slot_dev, int n_slots, int max_len, int T, int H,
                                        int K, int V, int chunk, int n_chunks, const int32_t* chunk_tab_dev, const int32_t* chunk_dst_dev,
                                        int dtype, void* stream) {
    RC(cst_check_slots(slot_dev, n_slots));
    return cs_pack_chain(k, v, mix, ldmix, S, cap_chunks, P, Cur, n_seqs, seq_len_dev, Slots{slot_dev, n_slots}, max_len, T, H, K, V, chunk, n_chunks,
                         chunk_tab_dev, chunk_dst_dev, nullptr, 0, dtype, stream);
}

int mhla_causal_step(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                     int64_t pos, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws,
                     size_t ws_bytes, int B, int H, int K, int V, int chunk, float scale, int dtype, void* stream) {
    RC(cst_check(B, H, K, V, chunk, dtype));
    RC(cst_check_io(q, k, v, out, y, gate, norm_w, dtype, S, cap_chunks, P, Cur));
    if (pos < 0) return fail(MHLA_EINVAL, "pos=%lld is negative", (long long)pos);
    const int64_t i = pos / chunk;
    const int r = (int)(pos - i * chunk);
    if (i >= cap_chunks) return fail(MHLA_EINVAL, "pos=%lld is in chunk %lld, the state holds %d", (long long)pos, (long long)i, cap_chunks);
    const bool roll = r == chunk - 1, next = roll && i + 1 < cap_chunks;
    RC(cst_check_mix(mix, ldmix, i + (next ? 1 : 0)));
    RC(cst_check_ws(ws, ws_bytes, cst_ws_bytes(B, H, K, V)));
    hipStream_t st = (hipStream_t)stream;
    const int BH = B * H;
    DISPATCH_T(dtype, {
        CsStepArgs s{cv(q), cv(k), cv(v), mix + i * ldmix + i, P, Cur, (float*)ws, H, K, V};
        RC(cst_step(k_cs_step<ET>, "k_cs_step", s, BH, st));
        const CsFinishArgs f{(const float*)ws, cmv(out), cmv(y), cv(gate), norm_w, norm_eps, scale, H, V, s.nsplit};
        RC(launch(k_cs_step_finish<ET>, dim3(BH), dim3(CST_THREADS), 0, st, "k_cs_step_finish", f));
    });
    if (roll) RC(cst_roll(S, cap_chunks, P, Cur, next ? mix + (i + 1) * ldmix : nullptr, (int)i + 1, 1, BH, (long)K * V, st));
    return MHLA_OK;
}

int mhla_causal_step_ragged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                            float* Cur, int32_t* pos_dev, int64_t max_pos, int any_boundary, mhla_mview out, mhla_view gate,
                            const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int K, int V,
                            int chunk, float scale, int dtype, void* stream) {
    return cs_step_ragged_chain(q, k, v, mix, ldmix, S, cap_chunks, P, Cur, pos_dev, Slots{}, max_pos, any_boundary, out, gate, norm_w, norm_eps, y, ws,
                                ws_bytes, B, H, H, K, V, chunk, scale, dtype, stream);
}

int mhla_causal_step_ragged_gqa(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                                float* Cur, int32_t* pos_dev, int64_t max_pos, int any_boundary, mhla_mview out, mhla_view gate,
                                const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K,
                                int V, int chunk, float scale, int dtype, void* stream) {
    return cs_step_ragged_chain(q, k, v, mix, ldmix, S, cap_chunks, P, Cur, pos_dev, Slots{}, max_pos, any_boundary, out, gate, norm_w, norm_eps, y, ws,
                                ws_bytes, B, H, Hkv, K, V, chunk, scale, dtype, stream);
}

int mhla_causal_step_dev(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                         float* Cur, int32_t* pos_dev, int32_t* full_dev, const void* rope_cos, const void* rope_sin, int64_t ld_tab,
                         int64_t tab_rows, int feature_map, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                         mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int K, int V, int chunk, float scale, int dtype,
                         void* stream) {
    return cs_step_dev_chain(q, k, v, mix, ldmix, S, cap_chunks, P, Cur, pos_dev, Slots{}, full_dev, rope_cos, rope_sin, ld_tab, tab_rows, feature_map,
                             out, gate, norm_w, norm_eps, y, ws, ws_bytes, B, H, H, K, V, chunk, scale, dtype, stream);
}

int mhla_causal_step_dev_gqa(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                             float* Cur, int32_t* pos_dev, int32_t* full_dev, const void* rope_cos, const void* rope_sin, int64_t ld_tab,
                             int64_t tab_rows, int feature_map, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                             mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk, float scale,
                             int dtype, void* stream) {
    return cs_step_dev_chain(q, k, v, mix, ldmix, S, cap_chunks, P, Cur, pos_dev, Slots{}, full_dev, rope_cos, rope_sin, ld_tab, tab_rows, feature_map,
                             out, gate, norm_w, norm_eps, y, ws, ws_bytes, B, H, Hkv, K, V, chunk, scale, dtype, stream);
}

size_t mhla_causal_extend_ws_bytes(int B, int T, int H, int K, int V, int64_t pos, int dtype) {
    (void)dtype;
    if (B <= 0 || T <= 0 || H <= 0 || K <= 0 || V <= 0 || pos < 0) return 0;
    return cx_plan(B, T, H, K, V, pos).total * 4;
}

int mhla_causal_extend(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                       int64_t pos, int T, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws,
                       size_t ws_bytes, int B, int H, int K, int V, int chunk, float scale, int dtype, void* stream) {
    RC(cst_check(B, H, K, V, chunk, dtype));
    if (T <= 0) return fail(MHLA_EINVAL, "T=%d must be positive", T);
    if (T > 65535) return fail(MHLA_ENOTSUP, "T=%d exceeds 65535 tokens per call", T);
    RC(cst_check_io(q, k, v, out, y, gate, norm_w, dtype, S, cap_chunks, P, Cur));
    if (pos < 0) return fail(MHLA_EINVAL, "pos=%lld is negative", (long long)pos);
    const CxPlan p = cx_plan(B, T, H, K, V, pos);
    if (p.ilast >= cap_chunks)
        return fail(MHLA_EINVAL, "pos=%lld + T=%d tokens need %lld chunks, the state holds %d", (long long)pos, T, (long long)(p.ilast + 1), cap_chunks);
    // rows of mix read: the diagonal of chunks i .. ilast, and row iend (the chunk open afterwards) when a chunk closed and the state is not full
    const bool closing = p.iend > p.i, full = p.iend >= cap_chunks;
    const int64_t lastrow = closing && !full ? p.iend : p.ilast;
    RC(cst_check_mix(mix, ldmix, lastrow));
    RC(cst_check_ws(ws, ws_bytes, p.total * 4));
    hipStream_t st = (hipStream_t)stream;
    const int BH = B * H, nvt = (V + 63) / 64;
    const long E = (long)K * V;
    float* tiles = (float*)ws;
    float* stage = tiles + p.tiles;
    const int rest = T - p.a, nwhole = rest / CS, tail = rest - nwhole * CS;
    DISPATCH_T(dtype, {
        CxOutArgs o{};
        o.q = cv(q); o.k = cv(k); o.v = cv(v);
        if (!y.ptr) o.o = cmv(out);
        o.stage = stage; o.H = H; o.K = K; o.V = V; o.T = T; o.scale = scale; o.mstep = (long)ldmix + 1; o.G = 1;
        // the first segment reads the state's P and Cur before its own product is added to Cur
        o.P = P; o.p_bh = E; o.p_seg = 0; o.Cur = Cur; o.mdiag = mix + p.i * o.mstep; o.tok0 = 0; o.tend = p.a;
        RC(launch(k_cx_out<ET>, dim3(1, BH, nvt), dim3(NTHREADS), CS_OUT_SMEM_FLOATS * 4, st, "k_cx_out", o));
        const bool closes = p.r + p.a == CS;
        const CxAccArgs c{cv(k), cv(v), Cur, closes ? S + p.i * E : Cur, closes ? (long)cap_chunks * E : E, H, p.a, K, V};
        RC(launch(k_cx_xty_acc<ET>, dim3(1, BH, ((K + 63) / 64) * nvt), dim3(NTHREADS), 0, st, "k_cx_xty_acc", c));
        if (closes) {
            if (nwhole) RC(cst_xty<ET>(k, v, p.a, (long)nwhole * CS, S + (p.i + 1) * E, cap_chunks, B, H, K, V, st));
            if (tail) RC(cst_xty<ET>(k, v, p.a + (long)nwhole * CS, tail, Cur, 1, B, H, K, V, st));
            else      RC(cst_zero_cur(Cur, BH, E, st));
            CxMixArgs m{S, tiles, P, mix, E, ldmix, cap_chunks, (int)p.i + 1, p.nws, 0, full ? -1 : (int)p.iend};
            m.nc = (int)((full ? p.ilast : p.iend) - p.i);
            const int groups = std::max(1, (m.nc + CX_MIX_NC - 1) / CX_MIX_NC);   // (a full state forms no P: one group writes the zeros)
            RC(launch(k_cx_mix, dim3((unsigned)((E / 4 + 63) / 64), BH, groups), dim3(64), 0, st, "k_cx_mix", m));
            if (rest) {
                o.P = tiles; o.p_bh = (long)p.nws * E; o.p_seg = E; o.Cur = nullptr; o.mdiag = mix + (p.i + 1) * o.mstep;
                o.tok0 = p.a; o.tend = T;
                RC(launch(k_cx_out<ET>, dim3(p.nws, BH, nvt), dim3(NTHREADS), CS_OUT_SMEM_FLOATS * 4, st, "k_cx_out", o));
            }
        }
        if (y.ptr) {
            const CsFinishArgs f{stage, cmv(out), cmv(y), cv(gate), norm_w, norm_eps, scale, H, V, 1};
            RC(launch(k_cs_step_finish<ET>, dim3(BH, T), dim3(CST_THREADS), 0, st, "k_cs_step_finish", f));
        }
    });
    return MHLA_OK;
}

size_t mhla_causal_extend_ragged_ws_bytes(int B, int T, int H, int K, int V, int max_later, int dtype) {
    (void)dtype;
    if (B <= 0 || T <= 0 || H <= 0 || K <= 0 || V <= 0 || max_later < 0) return 0;
    return cx_rag_plan(B, T, H, H, K, V, max_later).total * 4;
}

size_t mhla_causal_extend_ragged_gqa_ws_bytes(int B, int T, int H, int Hkv, int K, int V, int max_later, int dtype) {
    (void)dtype;
    if (B <= 0 || T <= 0 || H <= 0 || Hkv <= 0 || H % Hkv || K <= 0 || V <= 0 || max_later < 0) return 0;
    return cx_rag_plan(B, T, H, Hkv, K, V, max_later).total * 4;
}

int mhla_causal_extend_ragged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                              float* Cur, int32_t* pos_dev, const int32_t* ntok_dev, int T, int64_t max_end, int max_later,
                              int any_close, int left_padded, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                              mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int K, int V, int chunk, float scale, int dtype,
                              void* stream) {
    return cx_ragged_chain(false, q, k, v, mix, ldmix, S, cap_chunks, P, Cur, pos_dev, Slots{}, ntok_dev, nullptr, T, max_end, max_later, any_close, left_padded,
                           out, gate, norm_w, norm_eps, y, ws, ws_bytes, B, H, H, K, V, chunk, scale, dtype, stream);
}

int mhla_causal_extend_ragged_gqa(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                                  float* Cur, int32_t* pos_dev, const int32_t* ntok_dev, int T, int64_t max_end, int max_later,
                                  int any_close, int left_padded, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                                  mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk, float scale,
                                  int dtype, void* stream) {
    return cx_ragged_chain(false, q, k, v, mix, ldmix, S, cap_chunks, P, Cur, pos_dev, Slots{}, ntok_dev, nullptr, T, max_end, max_later, any_close, left_padded,
                           out, gate, norm_w, norm_eps, y, ws, ws_bytes, B, H, Hkv, K, V, chunk, scale, dtype, stream);
}

int mhla_causal_verify_ragged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                              float* Cur, const int32_t* pos_dev, const int32_t* ntok_dev, int T, int64_t max_end, int max_later,
                              int any_close, int left_padded, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                              mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int K, int V, int chunk, float scale, int dtype,
                              void* stream) {
    return cx_ragged_chain(true, q, k, v, mix, ldmix, S, cap_chunks, P, Cur, const_cast<int32_t*>(pos_dev), Slots{}, ntok_dev, nullptr, T, max_end, max_later, any_close, left_padded, out, gate, norm_w,
                           norm_eps, y, ws, ws_bytes, B, H, H, K, V, chunk, scale, dtype, stream);
}

int mhla_causal_verify_ragged_gqa(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                                  float* Cur, const int32_t* pos_dev, const int32_t* ntok_dev, int T, int64_t max_end, int max_later,
                                  int any_close, int left_padded, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                                  mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk, float scale,
                                  int dtype, void* stream) {
    return cx_ragged_chain(true, q, k, v, mix, ldmix, S, cap_chunks, P, Cur, const_cast<int32_t*>(pos_dev), Slots{}, ntok_dev, nullptr, T, max_end, max_later,
                           any_close, left_padded, out, gate, norm_w, norm_eps, y, ws, ws_bytes, B, H, Hkv, K, V, chunk, scale, dtype, stream);
}

size_t mhla_causal_commit_ragged_ws_bytes(int B, int dtype) {
    (void)dtype;
    return B > 0 ? al4((size_t)B) * 4 : 0;
}

int mhla_causal_commit_ragged(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                              int32_t* pos_dev, const int32_t* ntok_dev, const int32_t* accept_dev, int T, int64_t max_end,
                              int max_later, int any_close, int left_padded, void* ws, size_t ws_bytes, int B, int H, int K, int V,
                              int chunk, int dtype, void* stream) {
    return cx_commit_chain(k, v, mix, ldmix, S, cap_chunks, P, Cur, pos_dev, Slots{}, ntok_dev, nullptr, accept_dev, T, max_end, max_later, any_close,
                           left_padded, ws, ws_bytes, B, H, K, V, chunk, dtype, stream);
}

// ---- slotted calls: the namesakes on chosen rows of a state pool (mhla_hip.h), each through its namesake's chain
int mhla_causal_step_slots(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                           int32_t* pos_dev, const int32_t* slot_dev, int n_slots, int64_t max_pos, int any_boundary, mhla_mview out,
                           mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv,
                           int K, int V, int chunk, float scale, int dtype, void* stream) {
    RC(cst_check_slots(slot_dev, n_slots));
    return cs_step_ragged_chain(q, k, v, mix, ldmix, S, cap_chunks, P, Cur, pos_dev, Slots{slot_dev, n_slots}, max_pos, any_boundary, out, gate,
                                norm_w, norm_eps, y, ws, ws_bytes, B, H, Hkv, K, V, chunk, scale, dtype, stream);
}

int mhla_causal_step_dev_slots(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                               float* Cur, int32_t* pos_dev, const int32_t* slot_dev, int n_slots, int32_t* full_dev, const void* rope_cos,
                               const void* rope_sin, int64_t ld_tab, int64_t tab_rows, int feature_map, mhla_mview out, mhla_view gate,
                               const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K,
                               int V, int chunk, float scale, int dtype, void* stream) {
    RC(cst_check_slots(slot_dev, n_slots));
    return cs_step_dev_chain(q, k, v, mix, ldmix, S, cap_chunks, P, Cur, pos_dev, Slots{slot_dev, n_slots}, full_dev, rope_cos, rope_sin, ld_tab,
                             tab_rows, feature_map, out, gate, norm_w, norm_eps, y, ws, ws_bytes, B, H, Hkv, K, V, chunk, scale, dtype, stream);
}

int mhla_causal_extend_slots(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                             float* Cur, int32_t* pos_dev, const int32_t* slot_dev, int n_slots, const int32_t* ntok_dev, int T,
                             int64_t max_end, int max_later, int any_close, int left_padded, mhla_mview out, mhla_view gate,
                             const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V,
                             int chunk, float scale, int dtype, void* stream) {
    RC(cst_check_slots(slot_dev, n_slots));
    return cx_ragged_chain(false, q, k, v, mix, ldmix, S, cap_chunks, P, Cur, pos_dev, Slots{slot_dev, n_slots}, ntok_dev, nullptr, T, max_end, max_later,
                           any_close, left_padded, out, gate, norm_w, norm_eps, y, ws, ws_bytes, B, H, Hkv, K, V, chunk, scale, dtype, stream);
}

int mhla_causal_verify_slots(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                             float* Cur, const int32_t* pos_dev, const int32_t* slot_dev, int n_slots, const int32_t* ntok_dev, int T,
                             int64_t max_end, int max_later, int any_close, int left_padded, mhla_mview out, mhla_view gate,
                             const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V,
                             int chunk, float scale, int dtype, void* stream) {
    RC(cst_check_slots(slot_dev, n_slots));
    return cx_ragged_chain(true, q, k, v, mix, ldmix, S, cap_chunks, P, Cur, const_cast<int32_t*>(pos_dev), Slots{slot_dev, n_slots}, ntok_dev, nullptr, T,
                           max_end, max_later, any_close, left_padded, out, gate, norm_w, norm_eps, y, ws, ws_bytes, B, H, Hkv, K, V, chunk, scale,
                           dtype, stream);
}

int mhla_causal_commit_slots(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                             int32_t* pos_dev, const int32_t* slot_dev, int n_slots, const int32_t* ntok_dev, const int32_t* accept_dev, int T,
                             int64_t max_end, int max_later, int any_close, int left_padded, void* ws, size_t ws_bytes, int B, int H, int K,
                             int V, int chunk, int dtype, void* stream) {
    RC(cst_check_slots(slot_dev, n_slots));
    return cx_commit_chain(k, v, mix, ldmix, S, cap_chunks, P, Cur, pos_dev, Slots{slot_dev, n_slots}, ntok_dev, nullptr, accept_dev, T, max_end, max_later,
                           any_close, left_padded, ws, ws_bytes, B, H, K, V, chunk, dtype, stream);
}

// ---- paged calls: the slotted calls on a pool whose finished chunks are pages named by a per-slot table (mhla_hip.h)
int mhla_causal_step_paged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages,
                           const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev, int n_slots,
                           int64_t max_pos, int any_boundary, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y,
                           void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk, float scale, int dtype, void* stream) {
    RC(cst_check_pages(pages, n_pages, table_dev));
    RC(cst_check_slots(slot_dev, n_slots));
    return cs_step_ragged_chain(q, k, v, mix, ldmix, pages, cap_chunks, P, Cur, pos_dev, Slots{slot_dev, n_slots, table_dev, n_pages}, max_pos,
                                any_boundary, out, gate, norm_w, norm_eps, y, ws, ws_bytes, B, H, Hkv, K, V, chunk, scale, dtype, stream);
}

int mhla_causal_step_dev_paged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages,
                               const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev,
                               int n_slots, int32_t* full_dev, const void* rope_cos, const void* rope_sin, int64_t ld_tab, int64_t tab_rows,
                               int feature_map, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws,
                               size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk, float scale, int dtype, void* stream) {
    RC(cst_check_pages(pages, n_pages, table_dev));
    RC(cst_check_slots(slot_dev, n_slots));
    return cs_step_dev_chain(q, k, v, mix, ldmix, pages, cap_chunks, P, Cur, pos_dev, Slots{slot_dev, n_slots, table_dev, n_pages}, full_dev,
                             rope_cos, rope_sin, ld_tab, tab_rows, feature_map, out, gate, norm_w, norm_eps, y, ws, ws_bytes, B, H, Hkv, K, V, chunk,
                             scale, dtype, stream);
}

int mhla_causal_extend_paged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages,
                             const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev,
                             int n_slots, const int32_t* ntok_dev, int T, int64_t max_end, int max_later, int any_close, int left_padded,
                             mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B,
                             int H, int Hkv, int K, int V, int chunk, float scale, int dtype, void* stream) {
    RC(cst_check_pages(pages, n_pages, table_dev));
    RC(cst_check_slots(slot_dev, n_slots));
    return cx_ragged_chain(false, q, k, v, mix, ldmix, pages, cap_chunks, P, Cur, pos_dev, Slots{slot_dev, n_slots, table_dev, n_pages}, ntok_dev,
                           nullptr, T, max_end, max_later, any_close, left_padded, out, gate, norm_w, norm_eps, y, ws, ws_bytes, B, H, Hkv, K, V, chunk,
                           scale, dtype, stream);
}

int mhla_causal_verify_paged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages,
                             const int32_t* table_dev, int cap_chunks, float* P, float* Cur, const int32_t* pos_dev, const int32_t* slot_dev,
                             int n_slots, const int32_t* ntok_dev, int T, int64_t max_end, int max_later, int any_close, int left_padded,
                             mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B,
                             int H, int Hkv, int K, int V, int chunk, float scale, int dtype, void* stream) {
    RC(cst_check_pages(pages, n_pages, table_dev));
    RC(cst_check_slots(slot_dev, n_slots));
    return cx_ragged_chain(true, q, k, v, mix, ldmix, pages, cap_chunks, P, Cur, const_cast<int32_t*>(pos_dev),
                           Slots{slot_dev, n_slots, table_dev, n_pages}, ntok_dev, nullptr, T, max_end, max_later, any_close, left_padded, out, gate, norm_w,
                           norm_eps, y, ws, ws_bytes, B, H, Hkv, K, V, chunk, scale, dtype, stream);
}

int mhla_causal_commit_paged(mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages, const int32_t* table_dev,
                             int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev, int n_slots,
                             const int32_t* ntok_dev, const int32_t* accept_dev, int T, int64_t max_end, int max_later, int any_close,
                             int left_padded, void* ws, size_t ws_bytes, int B, int H, int K, int V, int chunk, int dtype, void* stream) {
    RC(cst_check_pages(pages, n_pages, table_dev));
    RC(cst_check_slots(slot_dev, n_slots));
    return cx_commit_chain(k, v, mix, ldmix, pages, cap_chunks, P, Cur, pos_dev, Slots{slot_dev, n_slots, table_dev, n_pages}, ntok_dev, nullptr, accept_dev,
                           T, max_end, max_later, any_close, left_padded, ws, ws_bytes, B, H, K, V, chunk, dtype, stream);
}

int mhla_causal_varlen_state_init_paged(mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages,
                                        const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int n_seqs, const int32_t* seq_len_dev,
                                        const int32_t* slot_dev, int n_slots, int max_len, int T, int H, int K, int V, int chunk, int n_chunks,
                                        const int32_t* chunk_tab_dev, const int32_t* chunk_dst_dev, int dtype, void* stream) {
    RC(cst_check_pages(pages, n_pages, table_dev));
    RC(cst_check_slots(slot_dev, n_slots));
    return cs_pack_chain(k, v, mix, ldmix, pages, cap_chunks, P, Cur, n_seqs, seq_len_dev, Slots{slot_dev, n_slots, table_dev, n_pages}, max_len, T,
                         H, K, V, chunk, n_chunks, chunk_tab_dev, chunk_dst_dev, nullptr, 0, dtype, stream);
}

// ---- packed new tokens: the ragged extend, verify and commit on ONE run of tokens cut by off_dev (mhla_hip.h), each through its ragged
// namesake's chain; one entry point serves every kind of state: slot_dev null -- row b itself, table_dev null -- `S` is the dense array
size_t mhla_causal_extend_packed_ws_bytes(int B, int n_tokens, int H, int Hkv, int K, int V, int max_later, int dtype) {
    (void)dtype;
    if (B <= 0 || n_tokens <= 0 || H <= 0 || Hkv <= 0 || H % Hkv || K <= 0 || V <= 0 || max_later < 0) return 0;
    return cx_rag_plan(B, n_tokens, H, Hkv, K, V, max_later, true).total * 4;
}

int mhla_causal_extend_packed(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int n_pages,
                              const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev,
                              int n_slots, const int32_t* off_dev, int n_tokens, int64_t max_end, int max_later, int any_close, mhla_mview out,
                              mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H,
                              int Hkv, int K, int V, int chunk, float scale, int dtype, void* stream) {
    Slots sl{};
    RC(cst_packed_state(S, n_pages, table_dev, slot_dev, n_slots, off_dev, sl));
    return cx_ragged_chain(false, q, k, v, mix, ldmix, S, cap_chunks, P, Cur, pos_dev, sl, nullptr, off_dev, n_tokens, max_end, max_later, any_close,
                           0, out, gate, norm_w, norm_eps, y, ws, ws_bytes, B, H, Hkv, K, V, chunk, scale, dtype, stream);
}

int mhla_causal_verify_packed(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int n_pages,
                              const int32_t* table_dev, int cap_chunks, float* P, float* Cur, const int32_t* pos_dev, const int32_t* slot_dev,
                              int n_slots, const int32_t* off_dev, int n_tokens, int64_t max_end, int max_later, int any_close, mhla_mview out,
                              mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H,
                              int Hkv, int K, int V, int chunk, float scale, int dtype, void* stream) {
    Slots sl{};
    RC(cst_packed_state(S, n_pages, table_dev, slot_dev, n_slots, off_dev, sl));
    return cx_ragged_chain(true, q, k, v, mix, ldmix, S, cap_chunks, P, Cur, const_cast<int32_t*>(pos_dev), sl, nullptr, off_dev, n_tokens, max_end,
                           max_later, any_close, 0, out, gate, norm_w, norm_eps, y, ws, ws_bytes, B, H, Hkv, K, V, chunk, scale, dtype, stream);
}

int mhla_causal_commit_packed(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int n_pages, const int32_t* table_dev,
                              int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev, int n_slots,
                              const int32_t* off_dev, const int32_t* accept_dev, int n_tokens, int64_t max_end, int max_later, int any_close,
                              void* ws, size_t ws_bytes, int B, int Hkv, int K, int V, int chunk, int dtype, void* stream) {
    Slots sl{};
    RC(cst_packed_state(S, n_pages, table_dev, slot_dev, n_slots, off_dev, sl));
    return cx_commit_chain(k, v, mix, ldmix, S, cap_chunks, P, Cur, pos_dev, sl, nullptr, off_dev, accept_dev, n_tokens, max_end, max_later, any_close,
                           0, ws, ws_bytes, B, Hkv, K, V, chunk, dtype, stream);
}

// ---- h16 pages: the paged step, device-positioned step and pack prefill on a pool of 2-byte pages (mhla_hip.h), each through its
// namesake's chain
int mhla_causal_step_paged_h16(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, void* pages_h16, float* page_mult, int n_pages,
                               const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev,
                               int n_slots, int64_t max_pos, int any_boundary, mhla_mview out, mhla_view gate, const float* norm_w,
                               float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk,
                               float scale, int dtype, void* stream) {
    RC(cst_check_pages_h16(pages_h16, page_mult, K, V));
    RC(cst_check_pages((const float*)pages_h16, n_pages, table_dev));
    RC(cst_check_slots(slot_dev, n_slots));
    return cs_step_ragged_chain(q, k, v, mix, ldmix, (float*)pages_h16, cap_chunks, P, Cur, pos_dev, Slots{slot_dev, n_slots, table_dev, n_pages, page_mult},
                                max_pos, any_boundary, out, gate, norm_w, norm_eps, y, ws, ws_bytes, B, H, Hkv, K, V, chunk, scale, dtype, stream);
}

int mhla_causal_step_dev_paged_h16(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, void* pages_h16, float* page_mult,
                                   int n_pages, const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int32_t* pos_dev,
                                   const int32_t* slot_dev, int n_slots, int32_t* full_dev, const void* rope_cos, const void* rope_sin,
                                   int64_t ld_tab, int64_t tab_rows, int feature_map, mhla_mview out, mhla_view gate, const float* norm_w,
                                   float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk,
                                   float scale, int dtype, void* stream) {
    RC(cst_check_pages_h16(pages_h16, page_mult, K, V));
    RC(cst_check_pages((const float*)pages_h16, n_pages, table_dev));
    RC(cst_check_slots(slot_dev, n_slots));
    return cs_step_dev_chain(q, k, v, mix, ldmix, (float*)pages_h16, cap_chunks, P, Cur, pos_dev, Slots{slot_dev, n_slots, table_dev, n_pages, page_mult},
                             full_dev, rope_cos, rope_sin, ld_tab, tab_rows, feature_map, out, gate, norm_w, norm_eps, y, ws, ws_bytes, B, H, Hkv, K,
                             V, chunk, scale, dtype, stream);
}

size_t mhla_causal_varlen_state_init_paged_h16_ws_bytes(int n_chunks, int H, int K, int V, int dtype) {
    (void)dtype;
    if (n_chunks <= 0 || H <= 0 || K <= 0 || V <= 0) return 0;
    return (size_t)n_chunks * H * K * V * 4;
}

int mhla_causal_varlen_state_init_paged_h16(mhla_view k, mhla_view v, const float* mix, int ldmix, void* pages_h16, float* page_mult, int n_pages,
                                            const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int n_seqs,
                                            const int32_t* seq_len_dev, const int32_t* slot_dev, int n_slots, int max_len, int T, int H, int K,
                                            int V, int chunk, int n_chunks, const int32_t* chunk_tab_dev, const int32_t* chunk_dst_dev, void* ws,
                                            size_t ws_bytes, int dtype, void* stream) {
    RC(cst_check_pages_h16(pages_h16, page_mult, K, V));
    RC(cst_check_pages((const float*)pages_h16, n_pages, table_dev));
    RC(cst_check_slots(slot_dev, n_slots));
    return cs_pack_chain(k, v, mix, ldmix, (float*)pages_h16, cap_chunks, P, Cur, n_seqs, seq_len_dev, Slots{slot_dev, n_slots, table_dev, n_pages, page_mult},
                         max_len, T, H, K, V, chunk, n_chunks, chunk_tab_dev, chunk_dst_dev, ws, ws_bytes, dtype, stream);
}

// ---- swap: the state of chosen slots of a paged pool out into one contiguous blob and back in (mhla_hip.h; kernels: causal_swap.hpp)
size_t mhla_causal_swap_ws_bytes(int n_seqs, int n_pages, int Hkv, int K, int V, int page_format) {
    if (n_seqs < 0 || n_pages < 0 || Hkv <= 0 || K <= 0 || V <= 0 || ((long)K * V) % 4) return 0;
    if (page_format != PF_F32 && (page_format != PF_H16 || ((long)K * V) % CSH_GROUP)) return 0;
    const CsSwapLayout l = cs_swap_layout(Hkv, K, V, page_format);
    return (size_t)n_seqs * l.seq_bytes + (size_t)n_pages * l.page_bytes;
}

int mhla_causal_swap_out_paged(const void* pages, const float* page_mult, int n_pages, const float* P, const float* Cur, const int32_t* pos_dev,
                               const int32_t* full_dev, int n_slots, const int32_t* items_dev, int n_seqs, int n_pages_moved, int i0, int i1,
                               void* blob_at, int Hkv, int K, int V, void* stream) {
    return cs_swap<true>((void*)pages, (float*)page_mult, n_pages, (float*)P, (float*)Cur, (int32_t*)pos_dev, (int32_t*)full_dev, n_slots, items_dev, n_seqs,
                         n_pages_moved, i0, i1, blob_at, Hkv, K, V, stream);
}

int mhla_causal_swap_in_paged(void* pages, float* page_mult, int n_pages, float* P, float* Cur, int32_t* pos_dev, int32_t* full_dev, int n_slots,
                              const int32_t* items_dev, int n_seqs, int n_pages_moved, int i0, int i1, const void* blob_at, int Hkv, int K, int V,
                              void* stream) {
    return cs_swap<false>(pages, page_mult, n_pages, P, Cur, pos_dev, full_dev, n_slots, items_dev, n_seqs, n_pages_moved, i0, i1, (void*)blob_at, Hkv, K,
                          V, stream);
}

}  // extern "C"
