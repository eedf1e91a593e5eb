// C ABI, causal operator: the decode state of a sequence, the single-token step and the extension by T tokens (mhla_hip.h; kernels:
// causal_step.hpp, causal_extend.hpp, causal_swap.hpp).
//
// A call is described by four structs -- DecState (whose state), DecTokens (which tokens), DecRows (which rows come out), DecProblem (sizes,
// dtype, stream, workspace) -- that a wrapper fills by name and a chain takes by reference.  Entry point -> chain:
//
//   mhla_causal_state_init, mhla_causal_step, mhla_causal_extend            their own bodies: one position for the batch, on the host
//   mhla_causal_step_ragged   [_gqa, _slots, _paged, _paged_h16]            cs_step_ragged_chain   step, roll on a boundary, finish
//   mhla_causal_step_dev      [_gqa, _slots, _paged, _paged_h16]            cs_step_dev_chain      step, roll, finish: nothing depends on a position
//   mhla_causal_extend_ragged [_gqa], mhla_causal_extend_{slots,paged,packed}   cx_ragged_chain(dry = false)
//   mhla_causal_verify_ragged [_gqa], mhla_causal_verify_{slots,paged,packed}   cx_ragged_chain(dry = true): nothing of the committed state written
//   mhla_causal_commit_ragged, mhla_causal_commit_{slots,paged,packed}      cx_commit_chain        the state half of the extend, no q and no rows
//   mhla_causal_varlen_state_init [_slots, _paged, _paged_h16]              cs_pack_chain          the pack prefill
//   mhla_causal_swap_{out,in}_paged                                         cs_swap<OUT>
//   mhla_causal_*_ws_bytes                                                  the plans below (cst_ws_bytes, cx_plan, cx_rag_plan, cs_swap_layout)
//
// The forms differ in the state alone, and each has one checked constructor: cs_dense (row b of a dense state), cs_slots (row
// slot_dev[b] of a pool), cs_paged (finished chunks in fp32 pages named by a table), cs_paged_h16 (2-byte pages), cs_packed (the
// nullable arguments of the *_packed calls, which serve every kind of fp32 state).  _gqa is Hkv < H in DecProblem and nothing else.
// Which instantiation of a kernel a call runs is decided once per kernel, by with_step_var, with_finish_var, with_roll_var and
// with_cx_var: from the variant as the call's facts give it to the constant, over the list of the instantiations that exist.
// The prefill state reuses the generic path's exact-fp32 chunk products (blockmix.hpp k_bm_state<MODE 2>) written straight into the
// state's layout; the 16-bit pipeline's 11-bit summaries are never decoded.
#include "capi_common.hpp"
#include "blockmix.hpp"
#include "causal.hpp"
#include "causal_step.hpp"
#include "causal_extend.hpp"
#include "causal_swap.hpp"

using namespace mhla;
using namespace mhla::capi;

namespace {

// ---- the call, as the chains take it
// the finished chunks S[j] of a state: fp32 -- a dense array [rows][Hkv][cap][K][V], or with DecState::table pages [n_pages][Hkv][K][V] --
// or h16 pages, payload _Float16 [n_pages][Hkv][K][V] and multipliers float [n_pages][Hkv][K V / 64] (causal_step.hpp).  One of f32 / h16 is set
struct DecChunks {
    float* f32 = nullptr;
    _Float16* h16 = nullptr;
    float* mult = nullptr;
    const void* base() const { return h16 ? (const void*)h16 : (const void*)f32; }
};
// the slot map of a slotted call (the *_slots entry points): call row b works on row map[b] of a state pool of n_slots rows; map null:
// the un-slotted namesake, row b itself
// a paged pool (the *_paged entry points) on top: S is the pool of pages, and table[map[b] cap + j] names the page of chunk j of call
// row b; table null: S is the dense array
// h16 pages (the *_paged_h16 entry points) on top of that: S.h16 and S.mult; the pages are fp32 otherwise
struct DecState {
    const float* mix = nullptr;
    int ldmix = 0;
    DecChunks S;
    int cap = 0;
    float* P = nullptr;
    float* Cur = nullptr;
    int32_t* pos_dev = nullptr;
    int32_t* full_dev = nullptr;   // the device-positioned step only
    const int32_t* map = nullptr;
    int n_slots = 0;
    const int32_t* table = nullptr;
    int n_pages = 0;
    bool slotted() const { return map != nullptr; }
    bool paged() const { return table != nullptr; }
    bool h16() const { return S.h16 != nullptr; }
};
// the new tokens: one per sequence (the steps: q, k, v alone), a padded window of T (ntok_dev) or one run of T cut by off_dev (packed)
struct DecTokens {
    mhla_view q{}, k{}, v{};
    const int32_t* ntok_dev = nullptr;
    const int32_t* off_dev = nullptr;
    int T = 0;
    int64_t max_end = 0;
    int max_later = 0, any_close = 0, left_padded = 0;
    const int32_t* accept_dev = nullptr;   // the commit only
    bool packed() const { return off_dev != nullptr; }
};
struct DecRows {
    mhla_mview out{};
    mhla_view gate{};
    const float* norm_w = nullptr;
    float norm_eps = 0.f;
    mhla_mview y{};
};
struct DecProblem {   // H: the query heads, Hkv: the heads of k, v and the state (Hkv = H: the ungrouped call)
    int B = 0, H = 0, Hkv = 0, K = 0, V = 0, chunk = 0, dtype = 0;
    void* stream = nullptr;
    float scale = 0.f;
    void* ws = nullptr;
    size_t ws_bytes = 0;
};
// the fla layer's q / k prologue inside the device-positioned step
struct DecPrologue {
    const void* rope_cos = nullptr;
    const void* rope_sin = nullptr;
    int64_t ld_tab = 0, tab_rows = 0;
    int feature_map = 0;
};
// a pack of prompts (B = 1): n_seqs sequences of seq_len_dev[s] tokens, T in all, cut into n_chunks chunks listed by the two tables
struct DecPack {
    int n_seqs = 0;
    const int32_t* seq_len_dev = nullptr;
    int max_len = 0, T = 0, n_chunks = 0;
    const int32_t* chunk_tab_dev = nullptr;
    const int32_t* chunk_dst_dev = nullptr;
};

// the slot and page fields of a device argument struct, from the state (tcap: CsStepArgs and CsFinishArgs; pages = false: a launch
// that reads no page table -- the host-positioned step and the finishes of the host-positioned chains -- names the slot map alone)
template <typename A>
void cst_pool_fields(A& a, const DecState& s, bool pages = true) {
    a.slot = s.map; a.n_slots = s.n_slots;
    if (!pages) return;
    a.table = s.table; a.n_pages = s.n_pages;
    if constexpr (requires { a.tcap; }) a.tcap = s.cap;
}

// ---- from a variant as a call's facts give it to the kernel's constant: VS are the instantiations that exist, nothing else is launched
template <auto... VS, typename VAR, typename F>
int with_var(const VAR& v, const char* kernel, F&& f) {
    int rc = MHLA_OK;
    if (((v == VS ? (rc = f.template operator()<VS>(), true) : false) || ...)) return rc;
    return fail(MHLA_ENOTSUP, "%s: this call's variant is not built", kernel);
}
// k_cs_step<T>: the host-positioned step plain, slotted, grouped; the device-positioned one also with the prologue and on a paged pool
template <typename F>
int with_step_var(const StepVar& v, F&& f) {
    constexpr int GM = CST_GMAX;
    return with_var<StepVar{.ragged = true}, StepVar{.ragged = true, .slot = true}, StepVar{.ragged = true, .gmax = GM}, StepVar{.ragged = true, .gmax = GM, .slot = true},
                    StepVar{.ragged = true, .dev = true}, StepVar{.ragged = true, .dev = true, .slot = true}, StepVar{.ragged = true, .dev = true, .slot = true, .paged = true},
                    StepVar{.ragged = true, .dev = true, .pro = true}, StepVar{.ragged = true, .dev = true, .pro = true, .slot = true},
                    StepVar{.ragged = true, .dev = true, .pro = true, .slot = true, .paged = true},
                    StepVar{.ragged = true, .dev = true, .gmax = GM}, StepVar{.ragged = true, .dev = true, .gmax = GM, .slot = true},
                    StepVar{.ragged = true, .dev = true, .gmax = GM, .slot = true, .paged = true},
                    StepVar{.ragged = true, .dev = true, .pro = true, .gmax = GM}, StepVar{.ragged = true, .dev = true, .pro = true, .gmax = GM, .slot = true},
                    StepVar{.ragged = true, .dev = true, .pro = true, .gmax = GM, .slot = true, .paged = true}>(v, "k_cs_step", f);
}
template <typename F>
int with_finish_var(const FinishVar& v, F&& f) {
    return with_var<FinishVar{}, FinishVar{.slot = true}, FinishVar{.dev = true}, FinishVar{.dev = true, .slot = true}, FinishVar{.dev = true, .slot = true, .paged = true},
                    FinishVar{.win = true}, FinishVar{.win = true, .slot = true}, FinishVar{.win = true, .packed = true},
                    FinishVar{.win = true, .slot = true, .packed = true}>(v, "k_cs_step_finish", f);
}
// k_cs_roll of a ragged state or of a pack: un-slotted, slotted, on fp32 pages, on h16 pages
template <typename F>
int with_roll_var(const RollVar& v, F&& f) {
    return with_var<RollVar{.ragged = true}, RollVar{.ragged = true, .slot = true}, RollVar{.ragged = true, .slot = true, .paged = true},
                    RollVar{.ragged = true, .slot = true, .paged = true, .fmt = PF_H16},
                    RollVar{.pack = true}, RollVar{.pack = true, .slot = true}, RollVar{.pack = true, .slot = true, .paged = true},
                    RollVar{.pack = true, .slot = true, .paged = true, .fmt = PF_H16}>(v, "k_cs_roll", f);
}
// the three k_cx_* kernels of the ragged chains: padded or packed tokens
template <typename F>
int with_cx_var(bool packed, const char* kernel, F&& f) {
    return with_var<CxVar{.ragged = true}, CxVar{.ragged = true, .packed = true}>(CxVar{.ragged = true, .packed = packed}, kernel, f);
}

// ---- checks
int cst_check(int B, int H, int K, int V, int chunk, int dtype) {
    if (B <= 0 || H <= 0 || K <= 0 || V <= 0) return fail(MHLA_EINVAL, "non-positive dimension B=%d H=%d K=%d V=%d", B, H, K, V);
    if (chunk != 64) return fail(MHLA_ENOTSUP, "chunk=%d: only 64 is supported", chunk);
    if ((K | V) & 3) return fail(MHLA_EINVAL, "K=%d and V=%d must be multiples of 4", K, V);
    if (dtype < 0 || dtype > 2) return fail(MHLA_EINVAL, "unknown dtype %d", dtype);
    if ((size_t)B * H > 65535) return fail(MHLA_ENOTSUP, "B*H=%zu exceeds grid limit 65535", (size_t)B * H);
    return MHLA_OK;
}
int cst_check(const DecProblem& p) { return cst_check(p.B, p.H, p.K, p.V, p.chunk, p.dtype); }
// grouped-query heads: the state, k and v have Hkv heads, each shared by G = H / Hkv query heads (Hkv = H: the ungrouped call)
int cst_check_group(int H, int Hkv) {
    if (Hkv < 1 || H % Hkv) return fail(MHLA_EINVAL, "Hkv=%d must be positive and divide H=%d", Hkv, H);
    if (H / Hkv > CST_GMAX) return fail(MHLA_ENOTSUP, "H=%d query heads on Hkv=%d k/v heads: at most %d per k/v head are supported", H, Hkv, CST_GMAX);
    return MHLA_OK;
}
int cst_check_state(const void* S, int cap, const float* P, const float* Cur) {
    if (cap <= 0) return fail(MHLA_EINVAL, "cap_chunks=%d must be positive", cap);
    if (!S || !P || !Cur) return fail(MHLA_EINVAL, "state: S, P or Cur null");
    if (((uintptr_t)S | (uintptr_t)P | (uintptr_t)Cur) % 16) return fail(MHLA_EINVAL, "state: S, P and Cur must be 16-byte aligned");
    return MHLA_OK;
}
int cst_check_state(const DecState& s) { return cst_check_state(s.S.base(), s.cap, s.P, s.Cur); }
// what every step and extend entry point checks of its tokens, outputs and state, in this order (the parameter names are the messages')
int cst_check_io(const mhla_view& q, const mhla_view& k, const mhla_view& v, const DecRows& r, int dtype, const void* S, int cap, const float* P,
                 const float* Cur) {
    const mhla_mview &out = r.out, &y = r.y;
    const mhla_view& gate = r.gate;
    CHECK_VIEW(q); CHECK_VIEW(k); CHECK_VIEW(v);
    if (!out.ptr && !y.ptr) return fail(MHLA_EINVAL, "out and y both null");
    if (out.ptr) CHECK_VIEW(out);
    if (y.ptr) CHECK_VIEW(y);
    if (gate.ptr) CHECK_VIEW(gate);
    if ((gate.ptr || r.norm_w) && !y.ptr) return fail(MHLA_EINVAL, "gate / norm_w given without y");
    return cst_check_state(S, cap, P, Cur);
}
int cst_check_io(const DecTokens& n, const DecRows& r, int dtype, const DecState& s) {
    return cst_check_io(n.q, n.k, n.v, r, dtype, s.S.base(), s.cap, s.P, s.Cur);
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
int cst_check_slots(const int32_t* slot_dev, int n_slots) {
    RC(cst_check_dev("slot_dev", slot_dev));
    if (n_slots <= 0) return fail(MHLA_EINVAL, "n_slots=%d must be positive", n_slots);
    return MHLA_OK;
}
int cst_check_pages(const void* pages, int n_pages, const int32_t* table_dev) {
    if (!pages || ((uintptr_t)pages) % 16) return fail(MHLA_EINVAL, "pages null or not 16-byte aligned");
    RC(cst_check_dev("table_dev", table_dev));
    if (n_pages <= 0) return fail(MHLA_EINVAL, "n_pages=%d must be positive", n_pages);
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

// ---- the state of a call, one checked constructor per kind.  What they check of the pool comes ahead of everything the chain checks
// the part every kind shares: nothing of it is checked here (the chains do, each in its own order)
DecState cs_state(const float* mix, int ldmix, int cap_chunks, float* P, float* Cur, int32_t* pos_dev, int32_t* full_dev = nullptr) {
    DecState s;
    s.mix = mix; s.ldmix = ldmix; s.cap = cap_chunks; s.P = P; s.Cur = Cur; s.pos_dev = pos_dev; s.full_dev = full_dev;
    return s;
}
int cs_dense(DecState& s, float* S) {
    s.S.f32 = S;
    return MHLA_OK;
}
int cs_slots(DecState& s, float* S, const int32_t* slot_dev, int n_slots) {
    RC(cst_check_slots(slot_dev, n_slots));
    s.S.f32 = S; s.map = slot_dev; s.n_slots = n_slots;
    return MHLA_OK;
}
int cs_paged(DecState& s, float* pages, int n_pages, const int32_t* table_dev, const int32_t* slot_dev, int n_slots) {
    RC(cst_check_pages(pages, n_pages, table_dev));
    RC(cs_slots(s, pages, slot_dev, n_slots));
    s.table = table_dev; s.n_pages = n_pages;
    return MHLA_OK;
}
int cs_paged_h16(DecState& s, void* pages_h16, float* page_mult, int n_pages, const int32_t* table_dev, const int32_t* slot_dev, int n_slots, int K,
                 int V) {
    RC(cst_check_pages_h16(pages_h16, page_mult, K, V));
    RC(cst_check_pages(pages_h16, n_pages, table_dev));
    RC(cst_check_slots(slot_dev, n_slots));
    s.S.h16 = (_Float16*)pages_h16; s.S.mult = page_mult;
    s.map = slot_dev; s.n_slots = n_slots; s.table = table_dev; s.n_pages = n_pages;
    return MHLA_OK;
}
// what a packed entry point checks of its nullable state arguments: off_dev is what makes the call packed, so it is refused here,
// ahead of the chain (which takes a null off_dev for a padded call)
int cs_packed(DecState& s, float* S, int n_pages, const int32_t* table_dev, const int32_t* slot_dev, int n_slots, const int32_t* off_dev) {
    RC(cst_check_dev("off_dev", off_dev));
    if (table_dev) RC(cst_check_pages(S, n_pages, table_dev));
    if (slot_dev) RC(cst_check_slots(slot_dev, n_slots));
    s.S.f32 = S;
    s.map = slot_dev; s.n_slots = slot_dev ? n_slots : 0; s.table = table_dev; s.n_pages = table_dev ? n_pages : 0;
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
    return launch(k_cs_roll<>, dim3((unsigned)((E / 4 + 63) / 64), BH), dim3(64), 0, st, "k_cs_roll", r);
}
// what the roll of a ragged state (pos: the pool's positions) or of a pack (pos: the sequences' lengths) is told.  The argument names
// the finished chunks twice, as fp32 (S) and as h16 payload (pay); an instantiation reads the one of its format, and both fields have
// always carried the one address the call has
CsRollArgs cst_roll_args(const DecState& s, const int32_t* pos, int max_pos, int H, long E) {
    float* const S = s.h16() ? reinterpret_cast<float*>(s.S.h16) : s.S.f32;
    _Float16* const pay = s.h16() ? s.S.h16 : reinterpret_cast<_Float16*>(s.S.f32);
    CsRollArgs r{S, s.P, s.Cur, nullptr, E, s.cap, 0, 0, pos, s.mix, s.ldmix, max_pos, H};
    cst_pool_fields(r, s);
    r.pay = pay; r.mult = s.S.mult;
    return r;
}
// (h16 pages: 8 elements a lane)
unsigned cst_roll_grid_x(const DecState& s, long E) { return (unsigned)((E / (s.h16() ? CSH_EPL : 4) + 63) / 64); }
// the roll of a ragged state: each sequence for itself, by pos_dev (the position of the token its step just took)
int cst_roll_ragged(const DecState& s, int max_pos, int H, int BH, long E, hipStream_t st) {
    const CsRollArgs r = cst_roll_args(s, s.pos_dev, max_pos, H, E);
    return with_roll_var(RollVar{.ragged = true, .slot = s.slotted(), .paged = s.paged(), .fmt = s.h16() ? PF_H16 : PF_F32}, [&]<RollVar VAR>() {
        return launch(k_cs_roll<VAR>, dim3(cst_roll_grid_x(s, E), BH), dim3(64), 0, st, VAR.fmt == PF_H16 ? "k_cs_roll_ragged<h16>" : "k_cs_roll_ragged", r);
    });
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

// K^T V of ntok tokens from tok0 on, chunk by chunk, to out[(b, h)][chunk]: p gives B, H, K, V
template <typename T>
int cst_xty(const mhla_view& k, const mhla_view& v, long tok0, long ntok, float* out, int stride_chunks, const DecProblem& p, hipStream_t st) {
    StateArgs a{};
    a.x = cv(k); a.y = cv(v);
    a.x.ptr = (const T*)k.ptr + tok0 * k.sn;
    a.y.ptr = (const T*)v.ptr + tok0 * v.sn;
    a.out = out; a.H = p.H; a.M = stride_chunks; a.S = CS; a.D = 64; a.DX = p.K; a.DY = p.V; a.T = ntok; a.alpha = 1.f;
    const int strips = ((p.K + 63) / 64) * ((p.V + 63) / 64);
    return launch(k_bm_state<T, 4, 2>, dim3((unsigned)((ntok + CS - 1) / CS), p.B * p.H, strips), dim3(NTHREADS), state_smem_floats<4>() * 4, st,
                  "k_bm_state<2>", a);
}

// the chunks of a pack (B = 1), each tile into its sequence's state: a whole chunk to S[seq][h][loc], a ragged one to Cur[seq][h]
template <typename T>
int cst_xty_pack(const mhla_view& k, const mhla_view& v, const DecState& s, const DecPack& pk, const DecProblem& p, hipStream_t st) {
    StateArgsDst a{};
    a.x = cv(k); a.y = cv(v);
    a.H = p.H; a.M = 0; a.S = CS; a.D = 64; a.DX = p.K; a.DY = p.V; a.T = pk.T; a.alpha = 1.f;
    a.tab = (const tab2_t*)pk.chunk_tab_dev; a.dst = pk.chunk_dst_dev; a.Sq = s.S.f32; a.Cur = s.Cur; a.nseq = pk.n_seqs; a.cap = s.cap;
    cst_pool_fields(a, s);
    const int strips = ((p.K + 63) / 64) * ((p.V + 63) / 64);
    return launch(k_bm_state<T, 4, 2, StateArgsDst>, dim3((unsigned)pk.n_chunks, p.H, strips), dim3(NTHREADS), state_smem_floats<4>() * 4, st,
                  "k_bm_state<2,dst>", a);
}

// h16 pages: the chunks [c0, c0 + n) of a pack's chunk list (B = 1), fp32, into the staging area [H][n][K][V] -- the tiles of
// cst_xty_pack, each at its place in the list instead of its place in a state
template <typename T>
int cst_xty_stage(const mhla_view& k, const mhla_view& v, float* stage, int n, const int* tab, int T_, const DecProblem& p, hipStream_t st) {
    StateArgsVar a{};
    a.x = cv(k); a.y = cv(v);
    a.out = stage; a.H = p.H; a.M = n; a.S = CS; a.D = 64; a.DX = p.K; a.DY = p.V; a.T = T_; a.alpha = 1.f;
    a.tab = (const tab2_t*)tab;
    const int strips = ((p.K + 63) / 64) * ((p.V + 63) / 64);
    return launch(k_bm_state<T, 4, 2, StateArgsVar>, dim3((unsigned)n, p.H, strips), dim3(NTHREADS), state_smem_floats<4>() * 4, st,
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
int cx_rag_check(const DecState& s, const DecTokens& n) {
    const int cap_chunks = s.cap, T = n.T;
    if (cap_chunks > INT32_MAX / 64) return fail(MHLA_ENOTSUP, "cap_chunks=%d: positions beyond int32", cap_chunks);
    RC(cst_check_dev("pos_dev", s.pos_dev));
    if (n.off_dev) RC(cst_check_dev("off_dev", n.off_dev));
    else RC(cst_check_dev("ntok_dev", n.ntok_dev));
    if (n.max_end < 0) return fail(MHLA_EINVAL, "max_end=%lld is negative", (long long)n.max_end);
    if (n.max_end > (int64_t)64 * cap_chunks)
        return fail(MHLA_EINVAL, "max_end=%lld tokens need %lld chunks, the state holds %d", (long long)n.max_end,
                    (long long)(n.max_end / 64 + (n.max_end % 64 != 0)), cap_chunks);   // (ceil without max_end + 63, which overflows near INT64_MAX)
    if (n.max_later < 0 || n.max_later > (T + 62) / 64)
        return fail(MHLA_EINVAL, "max_later=%d: T=%d tokens touch at most %d chunks after the first", n.max_later, T, (T + 62) / 64);
    if (n.max_later && !n.any_close) return fail(MHLA_EINVAL, "max_later=%d without any_close", n.max_later);
    // rows of mix read: every sequence's diagonal up to chunk (its end - 1) / 64 and, where it closes a chunk and is not full then, row
    // (its end) / 64.  Which sequence closes is known on the device only: with any_close row max_end / 64 must be covered (or
    // the state's last), as if the furthest sequence were the one -- the restriction of mhla_causal_step_ragged
    const int64_t lastrow = n.any_close ? std::min<int64_t>(n.max_end / 64, cap_chunks - 1) : (n.max_end > 0 ? (n.max_end - 1) / 64 : 0);
    return cst_check_mix(s.mix, s.ldmix, lastrow);
}
// what every kernel of the ragged chains derives its sequence's plan from
CxRag cx_rag(const DecState& s, const DecTokens& n, bool dry) {
    CxRag g{s.pos_dev, n.ntok_dev, n.T, s.cap, (int)n.max_end, n.max_later, n.any_close ? 1 : 0, n.left_padded ? 1 : 0, dry ? 1 : 0, n.accept_dev};
    cst_pool_fields(g, s);
    g.off = n.off_dev;
    return g;
}

// the ragged extend chain; dry (the verify): the same launches, nothing of the committed state -- Cur, P, pos_dev -- written
// Hkv < H (grouped-query heads): the launches that form or move state run over the B Hkv k/v heads, the two that compute rows
// (k_cx_out, the finish) over the B H query heads
// off_dev (the packed entry points; ntok_dev null, left_padded 0): the tokens are ONE run of T rows, sequence b's [off_dev[b], off_dev[b + 1]),
// the views come with sb = 0, the rows are staged [H][T][V] and the finish runs over (H, T)
int cx_ragged_chain(bool dry, const DecState& s, const DecTokens& n, const DecRows& rows, const DecProblem& pr) {
    const int B = pr.B, H = pr.H, Hkv = pr.Hkv, K = pr.K, V = pr.V, T = n.T, max_later = n.max_later;
    const bool pk = n.packed();   // (the kernels' packed instantiations; the padded ones are the code they were)
    RC(cst_check(pr));
    RC(cst_check_group(H, Hkv));
    if (T <= 0) return fail(MHLA_EINVAL, "%s=%d must be positive", pk ? "n_tokens" : "T", T);
    if (T > 65535) return fail(MHLA_EINVAL, "%s=%d exceeds 65535 tokens per call", pk ? "n_tokens" : "T", T);   // (mhla_causal_extend answers MHLA_ENOTSUP here: kept, a caller may test the code)
    RC(cst_check_io(n, rows, pr.dtype, s));
    RC(cx_rag_check(s, n));
    const CxRagPlan p = cx_rag_plan(B, T, H, Hkv, K, V, max_later, pk);
    RC(cst_check_ws(pr.ws, pr.ws_bytes, p.total * 4));
    hipStream_t st = (hipStream_t)pr.stream;
    const int BH = B * H, BHk = B * Hkv, nvt = (V + 63) / 64, strips = ((K + 63) / 64) * nvt;
    const long E = (long)K * V;
    float* tiles = (float*)pr.ws;
    float* stage = tiles + p.tiles;
    int* nval = (int*)(stage + p.stage);
    const CxRag g = cx_rag(s, n, dry);
    const int kr = cst_rows((size_t)H, K, V);   // a one-token sequence: the step's K split for a batch of one
    // every launch but the last addresses by pos_dev; the last, which does not, advances it (dry: does not)
    DISPATCH_T(pr.dtype, {
        CxOutArgs o{};
        o.q = cv(n.q); o.k = cv(n.k); o.v = cv(n.v);
        o.stage = stage; o.H = H; o.K = K; o.V = V; o.T = T; o.scale = pr.scale; o.mstep = (long)s.ldmix + 1;
        o.P = s.P; o.Cur = s.Cur; o.mdiag = s.mix; o.rag = g; o.later = 0; o.nval = nval; o.kr = kr; o.nsplit = (K + kr - 1) / kr;
        o.G = H / Hkv;
        const auto out_rows = [&](int segments) {
            return with_cx_var(pk, "k_cx_out", [&]<CxVar VAR>() {
                return launch(k_cx_out<ET, VAR>, dim3(segments, BH, nvt), dim3(NTHREADS), CS_OUT_SMEM_FLOATS * 4, st, "k_cx_out_ragged", o);
            });
        };
        RC(out_rows(1));
        CxAccArgs c{};
        c.x = cv(n.k); c.y = cv(n.v); c.H = Hkv; c.DX = K; c.DY = V; c.rag = g; c.later = 0; c.S = s.S.f32; c.Cur = s.Cur;
        const auto xty_acc = [&](int segments) {
            return with_cx_var(pk, "k_cx_xty_acc", [&]<CxVar VAR>() {
                return launch(k_cx_xty_acc<ET, VAR>, dim3(segments, BHk, strips), dim3(NTHREADS), 0, st, "k_cx_xty_acc_ragged", c);
            });
        };
        RC(xty_acc(1));
        if (n.any_close) {
            c.later = 1;
            RC(xty_acc(std::max(1, max_later)));
            CxMixRagArgs m{};
            m.m.S = s.S.f32; m.m.ws = tiles; m.m.P = s.P; m.m.mix = s.mix; m.m.E = E; m.m.ldmix = s.ldmix; m.m.cap = s.cap;
            m.rag = g; m.H = Hkv;
            const int groups = (max_later + 1 + CX_MIX_NC - 1) / CX_MIX_NC;   // (the largest nc is max_later + 1)
            RC(with_cx_var(pk, "k_cx_mix_ragged", [&]<CxVar VAR>() {
                return launch(k_cx_mix_ragged<VAR>, dim3((unsigned)((E / 4 + 63) / 64), BHk, groups), dim3(64), 0, st, "k_cx_mix_ragged", m);
            }));
            if (max_later) {
                o.P = tiles; o.Cur = nullptr; o.later = 1;
                RC(out_rows(max_later));
            }
        }
        CsFinishArgs f{stage, cmv(rows.out), cmv(rows.y), cv(rows.gate), rows.norm_w, rows.norm_eps, pr.scale, H, V, 1, dry ? nullptr : s.pos_dev};
        f.nval = nval; f.left = n.left_padded ? 1 : 0;
        cst_pool_fields(f, s, false);
        if (pk) { f.off = n.off_dev; f.nseq = B; }
        RC(with_finish_var(FinishVar{.win = true, .slot = s.slotted(), .packed = pk}, [&]<FinishVar VAR>() {
            return launch(k_cs_step_finish<ET, VAR>, pk ? dim3(H, T) : dim3(BH, T), dim3(CST_THREADS), 0, st,
                          pk ? "k_cs_step_finish_packed" : "k_cs_step_finish_ragged", f);
        }));
    });
    return MHLA_OK;
}

// the ragged step chain (step, roll, finish); Hkv < H (grouped-query heads): step and roll run over the B Hkv k/v heads, the step
// writing the partial sums of all B H query heads, which the finish reads as ever
int cs_step_ragged_chain(const DecState& s, const DecTokens& n, int64_t max_pos, int any_boundary, const DecRows& rows, const DecProblem& pr) {
    const int B = pr.B, H = pr.H, Hkv = pr.Hkv, K = pr.K, V = pr.V, cap_chunks = s.cap;
    RC(cst_check(pr));
    RC(cst_check_group(H, Hkv));
    RC(cst_check_io(n, rows, pr.dtype, s));
    RC(cst_check_dev("pos_dev", s.pos_dev));
    if (max_pos < 0 || max_pos >= INT32_MAX) return fail(MHLA_EINVAL, "max_pos=%lld is negative or beyond int32", (long long)max_pos);
    const int64_t i = max_pos / pr.chunk;
    if (i >= cap_chunks) return fail(MHLA_EINVAL, "max_pos=%lld is in chunk %lld, the state holds %d", (long long)max_pos, (long long)i, cap_chunks);
    // which sequence is on a boundary is known on the device only: with any_boundary the row after the furthest sequence's chunk
    // must be covered (unless that chunk is the state's last), as if that sequence were the one -- a restriction (mhla_hip.h):
    // the matrix passed with a boundary step reaches one row past the furthest sequence, or the state's capacity
    const bool next = any_boundary && i + 1 < cap_chunks;
    RC(cst_check_mix(s.mix, s.ldmix, i + (next ? 1 : 0)));
    RC(cst_check_ws(pr.ws, pr.ws_bytes, cst_ws_bytes(B, H, K, V)));
    hipStream_t st = (hipStream_t)pr.stream;
    const int BH = B * H, G = H / Hkv;
    // step and roll address by pos_dev; the finish, which does not, advances it: last in the chain
    DISPATCH_T(pr.dtype, {
        CsStepArgs a{cv(n.q), cv(n.k), cv(n.v), s.mix, s.P, s.Cur, (float*)pr.ws, Hkv, K, V, 0, 0, s.pos_dev, s.ldmix, (int)max_pos};
        cst_pool_fields(a, s, false);
        // (a slotted call: the kernels' slot instantiations; the un-slotted ones are the code they were)
        RC(with_step_var(StepVar{.ragged = true, .gmax = G == 1 ? 1 : CST_GMAX, .slot = s.slotted()}, [&]<StepVar VAR>() {
            return cst_step(k_cs_step<ET, VAR>, VAR.gmax == 1 ? "k_cs_step_ragged" : "k_cs_step_ragged<gqa>", a, BH, st, G);
        }));
        if (any_boundary) RC(cst_roll_ragged(s, (int)max_pos, Hkv, B * Hkv, (long)K * V, st));
        CsFinishArgs f{(const float*)pr.ws, cmv(rows.out), cmv(rows.y), cv(rows.gate), rows.norm_w, rows.norm_eps, pr.scale, H, V, a.nsplit, s.pos_dev};
        cst_pool_fields(f, s, false);
        RC(with_finish_var(FinishVar{.slot = s.slotted()}, [&]<FinishVar VAR>() {
            return launch(k_cs_step_finish<ET, VAR>, dim3(BH), dim3(CST_THREADS), 0, st, "k_cs_step_finish", f);
        }));
    });
    return MHLA_OK;
}

// the device-positioned step chain; Hkv < H as in cs_step_ragged_chain (the fused prologue: k once per k/v head, q per query head)
int cs_step_dev_chain(const DecState& s, const DecTokens& n, const DecPrologue& pl, const DecRows& rows, const DecProblem& pr) {
    const int B = pr.B, H = pr.H, Hkv = pr.Hkv, K = pr.K, V = pr.V, cap_chunks = s.cap, dtype = pr.dtype;
    RC(cst_check(pr));
    RC(cst_check_group(H, Hkv));
    RC(cst_check_io(n, rows, dtype, s));
    if (cap_chunks > INT32_MAX / 64) return fail(MHLA_ENOTSUP, "cap_chunks=%d: positions beyond int32", cap_chunks);
    RC(cst_check_dev("pos_dev", s.pos_dev));
    RC(cst_check_dev("full_dev", s.full_dev));
    // every bound is the capacity: whichever chunk a sequence is in, rows and columns 0 .. cap_chunks - 1 of mix may be read
    if (!s.mix || s.ldmix < cap_chunks)
        return fail(MHLA_EINVAL, "mix null or ldmix=%d < cap_chunks=%d (the matrix is read up to row %d)", s.ldmix, cap_chunks, cap_chunks - 1);
    if (pl.feature_map < 0 || pl.feature_map > 2) return fail(MHLA_EINVAL, "feature_map %d: 0 identity, 1 relu, 2 elu+1", pl.feature_map);
    if (!pl.rope_cos != !pl.rope_sin) return fail(MHLA_EINVAL, "rope_cos and rope_sin must be given together");
    const bool pro = pl.rope_cos || pl.feature_map;
    if (pro && (K & 7)) return fail(MHLA_EINVAL, "K=%d: the fused prologue needs K %% 8 == 0", K);
    if (pl.rope_cos) {
        if (pl.ld_tab < K / 2 || (pl.ld_tab & 3)) return fail(MHLA_EINVAL, "cos/sin tables: ld_tab=%lld < K/2 or not a multiple of 4", (long long)pl.ld_tab);
        const size_t al = dtype == MHLA_F32 ? 16 : 8;
        if (((uintptr_t)pl.rope_cos | (uintptr_t)pl.rope_sin) % al) return fail(MHLA_EINVAL, "cos/sin tables must be %zu-byte aligned", al);
        if (pl.tab_rows < (int64_t)64 * cap_chunks || pl.tab_rows > INT32_MAX)
            return fail(MHLA_EINVAL, "tab_rows=%lld: the tables need a row per position, %lld (64 cap_chunks)", (long long)pl.tab_rows, (long long)64 * cap_chunks);
    }
    RC(cst_check_ws(pr.ws, pr.ws_bytes, cst_ws_bytes(B, H, K, V)));
    hipStream_t st = (hipStream_t)pr.stream;
    const int BH = B * H, G = H / Hkv, max_pos = 64 * cap_chunks - 1;
    // always the same three launches, none of whose arguments depends on a position: step and roll address by pos_dev, the
    // finish -- one thread per sequence reads it, none else -- advances it or sets full_dev
    DISPATCH_T(dtype, {
        CsStepArgs a{cv(n.q), cv(n.k), cv(n.v), s.mix, s.P, s.Cur, (float*)pr.ws, Hkv, K, V, 0, 0, s.pos_dev, s.ldmix, max_pos,
                     pl.rope_cos, pl.rope_sin, (long)pl.ld_tab, (int)pl.tab_rows, pl.feature_map};
        cst_pool_fields(a, s);
        // un-slotted, slotted, or slotted on a paged pool (each instantiation the code it was)
        RC(with_step_var(StepVar{.ragged = true, .dev = true, .pro = pro, .gmax = G == 1 ? 1 : CST_GMAX, .slot = s.slotted(), .paged = s.paged()},
                         [&]<StepVar VAR>() {
            const char* name = VAR.gmax == 1 ? (VAR.pro ? "k_cs_step_dev<pro>" : "k_cs_step_dev") : (VAR.pro ? "k_cs_step_dev<pro,gqa>" : "k_cs_step_dev<gqa>");
            return cst_step(k_cs_step<ET, VAR>, name, a, BH, st, G);
        }));
        RC(cst_roll_ragged(s, max_pos, Hkv, B * Hkv, (long)K * V, st));
        CsFinishArgs f{(const float*)pr.ws, cmv(rows.out), cmv(rows.y), cv(rows.gate), rows.norm_w, rows.norm_eps, pr.scale, H, V, a.nsplit, s.pos_dev, max_pos,
                       s.full_dev};
        cst_pool_fields(f, s);
        RC(with_finish_var(FinishVar{.dev = true, .slot = s.slotted(), .paged = s.paged()}, [&]<FinishVar VAR>() {
            return launch(k_cs_step_finish<ET, VAR>, dim3(BH), dim3(CST_THREADS), 0, st, "k_cs_step_finish_dev", f);
        }));
    });
    return MHLA_OK;
}

// the pack prefill chain (the chunks' K^T V into their sequences' states, then every sequence's prefix mix); slotted: sequence q of the
// pack into row map[q] of the pool -- S, P and Cur of those rows only, seq_len_dev stays indexed by q.  pr.H: the k/v heads
int cs_pack_chain(const mhla_view& k, const mhla_view& v, const DecState& s, const DecPack& pk, const DecProblem& pr) {
    const int H = pr.H, K = pr.K, V = pr.V, chunk = pr.chunk, dtype = pr.dtype, cap_chunks = s.cap, T = pk.T, n_seqs = pk.n_seqs, n_chunks = pk.n_chunks,
              max_len = pk.max_len;
    RC(cst_check(1, H, K, V, chunk, dtype));
    if (n_seqs <= 0) return fail(MHLA_EINVAL, "n_seqs=%d must be positive", n_seqs);
    if ((size_t)n_seqs * H > 65535) return fail(MHLA_ENOTSUP, "n_seqs*H=%zu exceeds grid limit 65535", (size_t)n_seqs * H);
    if (T <= 0 || n_chunks <= 0) return fail(MHLA_EINVAL, "T=%d n_chunks=%d must be positive (an all-empty pack is an all-zero state)", T, n_chunks);
    CHECK_VIEW(k); CHECK_VIEW(v);
    RC(cst_check_state(s));
    if (n_chunks < (T + chunk - 1) / chunk || n_chunks > T)
        return fail(MHLA_EINVAL, "n_chunks=%d outside ceil(T / %d)=%d .. T=%d", n_chunks, chunk, (T + chunk - 1) / chunk, T);
    if (max_len < 0 || max_len > T) return fail(MHLA_EINVAL, "max_len=%d outside 0 .. T=%d", max_len, T);
    if ((max_len + chunk - 1) / chunk > cap_chunks)
        return fail(MHLA_EINVAL, "max_len=%d tokens need %d chunks, the state holds %d", max_len, (max_len + chunk - 1) / chunk, cap_chunks);
    // sequence q reads row len[q] / 64 of mix up to its diagonal unless its state is then full: the longest one's row covers all
    RC(cst_check_mix(s.mix, s.ldmix, std::min(max_len / chunk, cap_chunks - 1)));
    RC(cst_check_dev("seq_len_dev", pk.seq_len_dev));
    RC(cst_check_dev("chunk_dst_dev", pk.chunk_dst_dev));
    if (!pk.chunk_tab_dev || ((uintptr_t)pk.chunk_tab_dev) % 8) return fail(MHLA_EINVAL, "chunk_tab_dev null or not 8-byte aligned");
    hipStream_t st = (hipStream_t)pr.stream;
    const long E = (long)K * V;
    const CsRollArgs r = cst_roll_args(s, pk.seq_len_dev, max_len, H, E);
    if (s.h16()) {
        // h16 pages: the chunks' fp32 K^T V staged in the workspace, then encoded into their pages (open chunks copied to Cur), over
        // slices of the chunk list of as many chunks as the workspace holds; the roll once at the end
        const size_t per = (size_t)H * E * 4;
        RC(cst_check_ws(pr.ws, pr.ws_bytes, per));
        const int fit = (int)std::min<size_t>((size_t)n_chunks, pr.ws_bytes / per);
        for (int c0 = 0; c0 < n_chunks; c0 += fit) {
            const int n = std::min(fit, n_chunks - c0);
            DISPATCH_T(dtype, { RC(cst_xty_stage<ET>(k, v, (float*)pr.ws, n, pk.chunk_tab_dev + 2 * c0, T, pr, st)); });
            const CsEncodeArgs en{(const float*)pr.ws, pk.chunk_tab_dev + 2 * c0, pk.chunk_dst_dev + 2 * c0, s.S.h16, s.S.mult, s.Cur, s.map, s.table, E,
                                  n, H, n_seqs, cap_chunks, s.n_slots, s.n_pages};
            RC(launch(k_cs_page_encode, dim3((unsigned)n, H, (unsigned)((E / CSH_EPL + 63) / 64)), dim3(64), 0, st, "k_cs_page_encode", en));
        }
    } else {
        DISPATCH_T(dtype, { RC(cst_xty_pack<ET>(k, v, s, pk, pr, st)); });
    }
    return with_roll_var(RollVar{.pack = true, .slot = s.slotted(), .paged = s.paged(), .fmt = s.h16() ? PF_H16 : PF_F32}, [&]<RollVar VAR>() {
        return launch(k_cs_roll<VAR>, dim3(cst_roll_grid_x(s, E), n_seqs * H), dim3(64), 0, st, VAR.fmt == PF_H16 ? "k_cs_roll_pack<h16>" : "k_cs_roll_pack", r);
    });
}

// the commit chain: the state half of the ragged extend on the accepted tokens, no q and no rows (pr.H: the k/v heads); off_dev: as
// cx_ragged_chain's
int cx_commit_chain(const DecState& s, const DecTokens& n, const DecProblem& pr) {
    const int B = pr.B, H = pr.H, K = pr.K, V = pr.V, T = n.T, max_later = n.max_later, dtype = pr.dtype;
    const mhla_view &k = n.k, &v = n.v;
    const bool pk = n.packed();
    RC(cst_check(pr));
    if (T <= 0) return fail(MHLA_EINVAL, "%s=%d must be positive", pk ? "n_tokens" : "T", T);
    if (T > 65535) return fail(MHLA_EINVAL, "%s=%d exceeds 65535 tokens per call", pk ? "n_tokens" : "T", T);
    CHECK_VIEW(k); CHECK_VIEW(v);
    RC(cst_check_state(s));
    RC(cst_check_dev("accept_dev", n.accept_dev));
    RC(cx_rag_check(s, n));
    RC(cst_check_ws(pr.ws, pr.ws_bytes, al4((size_t)B) * 4));
    hipStream_t st = (hipStream_t)pr.stream;
    const int BH = B * H, strips = ((K + 63) / 64) * ((V + 63) / 64);
    const long E = (long)K * V;
    int* nval = (int*)pr.ws;
    const CxRag g = cx_rag(s, n, false);
    // every launch but the last addresses by pos_dev; the last, which does not, advances it
    DISPATCH_T(dtype, {
        CxAccArgs c{};
        c.x = cv(k); c.y = cv(v); c.H = H; c.DX = K; c.DY = V; c.rag = g; c.later = 0; c.S = s.S.f32; c.Cur = s.Cur; c.nval = nval;
        const auto xty_acc = [&](int segments) {
            return with_cx_var(pk, "k_cx_xty_acc", [&]<CxVar VAR>() {
                return launch(k_cx_xty_acc<ET, VAR>, dim3(segments, BH, strips), dim3(NTHREADS), 0, st, "k_cx_xty_acc_ragged", c);
            });
        };
        RC(xty_acc(1));
        if (n.any_close) {
            c.later = 1;
            RC(xty_acc(std::max(1, max_later)));
            CxMixRagArgs m{};
            m.m.S = s.S.f32; m.m.ws = nullptr; m.m.P = s.P; m.m.mix = s.mix; m.m.E = E; m.m.ldmix = s.ldmix; m.m.cap = s.cap;
            m.rag = g; m.H = H;
            RC(with_cx_var(pk, "k_cx_mix_ragged", [&]<CxVar VAR>() {
                return launch(k_cx_mix_ragged<VAR>, dim3((unsigned)((E / 4 + 63) / 64), BH, 1), dim3(64), 0, st, "k_cx_mix_ragged", m);
            }));
        }
    });
    return launch(k_cx_advance, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, "k_cx_advance", s.pos_dev, (const int*)nval, B, s.map, s.n_slots);
}

// the two directions of a swap (OUT: pool -> blob): the checks, then one launch of k_cs_swap over the items [i0, i1), whose first
// begins at `blob`.  mult null: fp32 pages
struct DecSwap {
    void* pages; float* mult; int n_pages;
    float* P; float* Cur; int32_t* pos_dev; int32_t* full_dev; int n_slots;
    const int32_t* items_dev; int n_seqs, n_moved, i0, i1;
    void* blob;
    int Hkv, K, V;
    void* stream;
};
template <bool OUT>
int cs_swap(const DecSwap& w) {
    const int Hkv = w.Hkv, K = w.K, V = w.V, n_seqs = w.n_seqs, n_moved = w.n_moved, i0 = w.i0, i1 = w.i1;
    if (Hkv <= 0 || K <= 0 || V <= 0 || w.n_pages <= 0 || w.n_slots <= 0)
        return fail(MHLA_EINVAL, "non-positive size Hkv=%d K=%d V=%d n_pages=%d n_slots=%d", Hkv, K, V, w.n_pages, w.n_slots);
    if (((long)K * V) % 4) return fail(MHLA_EINVAL, "K=%d V=%d: K*V must be a multiple of 4 (16-byte pieces)", K, V);
    if (w.mult && ((long)K * V) % CSH_GROUP) return fail(MHLA_EINVAL, "K=%d V=%d: h16 pages need K*V %% %d == 0 (one multiplier per %d elements)", K, V, CSH_GROUP, CSH_GROUP);
    if (!w.pages || !w.P || !w.Cur || !w.blob) return fail(MHLA_EINVAL, "pages, P, Cur or the blob null");
    if (((uintptr_t)w.pages | (uintptr_t)w.P | (uintptr_t)w.Cur | (uintptr_t)w.blob) % 16) return fail(MHLA_EINVAL, "pages, P, Cur and the blob must be 16-byte aligned");
    if (w.mult) RC(cst_check_dev("page_mult", w.mult));
    RC(cst_check_dev("pos_dev", w.pos_dev));
    if (w.full_dev) RC(cst_check_dev("full_dev", w.full_dev));
    RC(cst_check_dev("items_dev", w.items_dev));
    if (n_seqs < 0 || n_moved < 0 || (long)n_seqs + n_moved > 0x7fffffffL) return fail(MHLA_EINVAL, "n_seqs=%d and n_pages_moved=%d must not be negative", n_seqs, n_moved);
    if (i0 < 0 || i1 < i0 || i1 > n_seqs + n_moved)
        return fail(MHLA_EINVAL, "items [%d, %d) are outside the list of %d sequences and %d pages", i0, i1, n_seqs, n_moved);
    if (i0 == i1) return MHLA_OK;
    const int fmt = w.mult ? PF_H16 : PF_F32;
    const CsSwapLayout l = cs_swap_layout(Hkv, K, V, fmt);
    const CsSwapArgs a{(char*)w.blob, w.items_dev, i0, i1, n_seqs, (char*)w.pages, w.mult, w.n_pages, w.P, w.Cur, w.pos_dev, w.full_dev, w.n_slots,
                       l.state_pieces, l.pay_pieces, l.n_mult, l.n_mult_pad, l.seq_bytes, l.page_bytes};
    // memory-bound: about 2048 workgroups at the most, the rest grid-strided -- x over the 16-byte pieces of an item, four to a lane of the
    // smaller kind of item in the range (the four requests cs_swap_run keeps in flight; the larger kind takes more rounds), y over items
    const long pieces = std::min(i0 < n_seqs ? l.state_pieces : l.pay_pieces, i1 > n_seqs ? l.pay_pieces : l.state_pieces);
    const unsigned gx = (unsigned)std::min<long>((pieces + 1023) / 1024, 2048);
    const unsigned gy = (unsigned)std::min<long>(i1 - i0, std::max<long>(1, 2048 / gx));
    const hipStream_t st = (hipStream_t)w.stream;
    if (w.mult) return launch(k_cs_swap<OUT, PF_H16>, dim3(gx, gy), dim3(256), 0, st, OUT ? "k_cs_swap<out,h16>" : "k_cs_swap<in,h16>", a);
    return launch(k_cs_swap<OUT, PF_F32>, dim3(gx, gy), dim3(256), 0, st, OUT ? "k_cs_swap<out>" : "k_cs_swap<in>", a);
}

}  // namespace

// what the wrappers below say of a call, by name (the parameters are the entry point's own, so each mention is a parameter of that name)
#define CS_TOKENS .q = q, .k = k, .v = v
#define CS_WINDOW .ntok_dev = ntok_dev, .T = T, .max_end = max_end, .max_later = max_later, .any_close = any_close, .left_padded = left_padded
#define CS_PACKED .off_dev = off_dev, .T = n_tokens, .max_end = max_end, .max_later = max_later, .any_close = any_close
#define CS_ROWS DecRows{.out = out, .gate = gate, .norm_w = norm_w, .norm_eps = norm_eps, .y = y}
#define CS_PROLOGUE DecPrologue{.rope_cos = rope_cos, .rope_sin = rope_sin, .ld_tab = ld_tab, .tab_rows = tab_rows, .feature_map = feature_map}
#define CS_PACK DecPack{.n_seqs = n_seqs, .seq_len_dev = seq_len_dev, .max_len = max_len, .T = T, .n_chunks = n_chunks, .chunk_tab_dev = chunk_tab_dev, .chunk_dst_dev = chunk_dst_dev}
// (B_: 1 for a pack; HQ, HKV: the query heads and the k/v heads -- a commit and a pack prefill know the k/v heads alone)
#define CS_SIZES(B_, HQ, HKV) .B = B_, .H = HQ, .Hkv = HKV, .K = K, .V = V, .chunk = chunk, .dtype = dtype, .stream = stream
#define CS_WS .ws = ws, .ws_bytes = ws_bytes
#define CS_PROBLEM(HQ, HKV) DecProblem{CS_SIZES(B, HQ, HKV), .scale = scale, CS_WS}

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
    const DecProblem pr{.B = B, .H = H, .Hkv = H, .K = K, .V = V};
    DISPATCH_T(dtype, {
        if (nfull) RC(cst_xty<ET>(k, v, 0, (long)nfull * chunk, S, cap_chunks, pr, st));
        if (tail)  RC(cst_xty<ET>(k, v, (long)nfull * chunk, tail, Cur, 1, pr, st));
    });
    if (!tail) RC(cst_zero_cur(Cur, B * H, E, st));
    return cst_roll(S, cap_chunks, P, Cur, open ? mix + (long)nfull * ldmix : nullptr, nfull, 0, B * H, E, st);
}

int mhla_causal_varlen_state_init(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                                  int n_seqs, const int32_t* seq_len_dev, int max_len, int T, int H, int K, int V, int chunk, int n_chunks,
                                  const int32_t* chunk_tab_dev, const int32_t* chunk_dst_dev, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, nullptr);
    RC(cs_dense(s, S));
    return cs_pack_chain(k, v, s, CS_PACK, DecProblem{CS_SIZES(1, H, H)});
}

int mhla_causal_varlen_state_init_slots(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                                        int n_seqs, const int32_t* seq_len_dev, const int32_t* slot_dev, int n_slots, int max_len, int T, int H,
                                        int K, int V, int chunk, int n_chunks, const int32_t* chunk_tab_dev, const int32_t* chunk_dst_dev,
                                        int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, nullptr);
    RC(cs_slots(s, S, slot_dev, n_slots));
    return cs_pack_chain(k, v, s, CS_PACK, DecProblem{CS_SIZES(1, H, H)});
}

int mhla_causal_step(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                     int64_t pos, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws,
                     size_t ws_bytes, int B, int H, int K, int V, int chunk, float scale, int dtype, void* stream) {
    RC(cst_check(B, H, K, V, chunk, dtype));
    RC(cst_check_io(q, k, v, CS_ROWS, dtype, S, cap_chunks, P, Cur));
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
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev);
    RC(cs_dense(s, S));
    return cs_step_ragged_chain(s, DecTokens{CS_TOKENS}, max_pos, any_boundary, CS_ROWS, CS_PROBLEM(H, H));
}

int mhla_causal_step_ragged_gqa(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                                float* Cur, int32_t* pos_dev, int64_t max_pos, int any_boundary, mhla_mview out, mhla_view gate,
                                const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K,
                                int V, int chunk, float scale, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev);
    RC(cs_dense(s, S));
    return cs_step_ragged_chain(s, DecTokens{CS_TOKENS}, max_pos, any_boundary, CS_ROWS, CS_PROBLEM(H, Hkv));
}

int mhla_causal_step_dev(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                         float* Cur, int32_t* pos_dev, int32_t* full_dev, const void* rope_cos, const void* rope_sin, int64_t ld_tab,
                         int64_t tab_rows, int feature_map, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                         mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int K, int V, int chunk, float scale, int dtype,
                         void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev, full_dev);
    RC(cs_dense(s, S));
    return cs_step_dev_chain(s, DecTokens{CS_TOKENS}, CS_PROLOGUE, CS_ROWS, CS_PROBLEM(H, H));
}

int mhla_causal_step_dev_gqa(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                             float* Cur, int32_t* pos_dev, int32_t* full_dev, const void* rope_cos, const void* rope_sin, int64_t ld_tab,
                             int64_t tab_rows, int feature_map, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                             mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk, float scale,
                             int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev, full_dev);
    RC(cs_dense(s, S));
    return cs_step_dev_chain(s, DecTokens{CS_TOKENS}, CS_PROLOGUE, CS_ROWS, CS_PROBLEM(H, Hkv));
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
    RC(cst_check_io(q, k, v, CS_ROWS, dtype, S, cap_chunks, P, Cur));
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
    const DecProblem pr{.B = B, .H = H, .Hkv = H, .K = K, .V = V};
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
            if (nwhole) RC(cst_xty<ET>(k, v, p.a, (long)nwhole * CS, S + (p.i + 1) * E, cap_chunks, pr, st));
            if (tail) RC(cst_xty<ET>(k, v, p.a + (long)nwhole * CS, tail, Cur, 1, pr, st));
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
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev);
    RC(cs_dense(s, S));
    return cx_ragged_chain(false, s, DecTokens{CS_TOKENS, CS_WINDOW}, CS_ROWS, CS_PROBLEM(H, H));
}

int mhla_causal_extend_ragged_gqa(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                                  float* Cur, int32_t* pos_dev, const int32_t* ntok_dev, int T, int64_t max_end, int max_later,
                                  int any_close, int left_padded, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                                  mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk, float scale,
                                  int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev);
    RC(cs_dense(s, S));
    return cx_ragged_chain(false, s, DecTokens{CS_TOKENS, CS_WINDOW}, CS_ROWS, CS_PROBLEM(H, Hkv));
}

// (a verify writes no position: its pos_dev is const in the ABI and the chain, told `dry`, only reads it)
int mhla_causal_verify_ragged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                              float* Cur, const int32_t* pos_dev, const int32_t* ntok_dev, int T, int64_t max_end, int max_later,
                              int any_close, int left_padded, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                              mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int K, int V, int chunk, float scale, int dtype,
                              void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, const_cast<int32_t*>(pos_dev));
    RC(cs_dense(s, S));
    return cx_ragged_chain(true, s, DecTokens{CS_TOKENS, CS_WINDOW}, CS_ROWS, CS_PROBLEM(H, H));
}

int mhla_causal_verify_ragged_gqa(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                                  float* Cur, const int32_t* pos_dev, const int32_t* ntok_dev, int T, int64_t max_end, int max_later,
                                  int any_close, int left_padded, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                                  mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk, float scale,
                                  int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, const_cast<int32_t*>(pos_dev));
    RC(cs_dense(s, S));
    return cx_ragged_chain(true, s, DecTokens{CS_TOKENS, CS_WINDOW}, CS_ROWS, CS_PROBLEM(H, Hkv));
}

size_t mhla_causal_commit_ragged_ws_bytes(int B, int dtype) {
    (void)dtype;
    return B > 0 ? al4((size_t)B) * 4 : 0;
}

int mhla_causal_commit_ragged(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                              int32_t* pos_dev, const int32_t* ntok_dev, const int32_t* accept_dev, int T, int64_t max_end,
                              int max_later, int any_close, int left_padded, void* ws, size_t ws_bytes, int B, int H, int K, int V,
                              int chunk, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev);
    RC(cs_dense(s, S));
    return cx_commit_chain(s, DecTokens{.k = k, .v = v, CS_WINDOW, .accept_dev = accept_dev}, DecProblem{CS_SIZES(B, H, H), CS_WS});
}

// ---- slotted calls: the namesakes on chosen rows of a state pool (mhla_hip.h), each through its namesake's chain
int mhla_causal_step_slots(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                           int32_t* pos_dev, const int32_t* slot_dev, int n_slots, int64_t max_pos, int any_boundary, mhla_mview out,
                           mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv,
                           int K, int V, int chunk, float scale, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev);
    RC(cs_slots(s, S, slot_dev, n_slots));
    return cs_step_ragged_chain(s, DecTokens{CS_TOKENS}, max_pos, any_boundary, CS_ROWS, CS_PROBLEM(H, Hkv));
}

int mhla_causal_step_dev_slots(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                               float* Cur, int32_t* pos_dev, const int32_t* slot_dev, int n_slots, int32_t* full_dev, const void* rope_cos,
                               const void* rope_sin, int64_t ld_tab, int64_t tab_rows, int feature_map, mhla_mview out, mhla_view gate,
                               const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K,
                               int V, int chunk, float scale, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev, full_dev);
    RC(cs_slots(s, S, slot_dev, n_slots));
    return cs_step_dev_chain(s, DecTokens{CS_TOKENS}, CS_PROLOGUE, CS_ROWS, CS_PROBLEM(H, Hkv));
}

int mhla_causal_extend_slots(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                             float* Cur, int32_t* pos_dev, const int32_t* slot_dev, int n_slots, const int32_t* ntok_dev, int T,
                             int64_t max_end, int max_later, int any_close, int left_padded, mhla_mview out, mhla_view gate,
                             const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V,
                             int chunk, float scale, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev);
    RC(cs_slots(s, S, slot_dev, n_slots));
    return cx_ragged_chain(false, s, DecTokens{CS_TOKENS, CS_WINDOW}, CS_ROWS, CS_PROBLEM(H, Hkv));
}

int mhla_causal_verify_slots(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                             float* Cur, const int32_t* pos_dev, const int32_t* slot_dev, int n_slots, const int32_t* ntok_dev, int T,
                             int64_t max_end, int max_later, int any_close, int left_padded, mhla_mview out, mhla_view gate,
                             const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V,
                             int chunk, float scale, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, const_cast<int32_t*>(pos_dev));
    RC(cs_slots(s, S, slot_dev, n_slots));
    return cx_ragged_chain(true, s, DecTokens{CS_TOKENS, CS_WINDOW}, CS_ROWS, CS_PROBLEM(H, Hkv));
}

int mhla_causal_commit_slots(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                             int32_t* pos_dev, const int32_t* slot_dev, int n_slots, const int32_t* ntok_dev, const int32_t* accept_dev, int T,
                             int64_t max_end, int max_later, int any_close, int left_padded, void* ws, size_t ws_bytes, int B, int H, int K,
                             int V, int chunk, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev);
    RC(cs_slots(s, S, slot_dev, n_slots));
    return cx_commit_chain(s, DecTokens{.k = k, .v = v, CS_WINDOW, .accept_dev = accept_dev}, DecProblem{CS_SIZES(B, H, H), CS_WS});
}

// ---- paged calls: the slotted calls on a pool whose finished chunks are pages named by a per-slot table (mhla_hip.h)
int mhla_causal_step_paged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages,
                           const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev, int n_slots,
                           int64_t max_pos, int any_boundary, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y,
                           void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk, float scale, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev);
    RC(cs_paged(s, pages, n_pages, table_dev, slot_dev, n_slots));
    return cs_step_ragged_chain(s, DecTokens{CS_TOKENS}, max_pos, any_boundary, CS_ROWS, CS_PROBLEM(H, Hkv));
}

int mhla_causal_step_dev_paged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages,
                               const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev,
                               int n_slots, int32_t* full_dev, const void* rope_cos, const void* rope_sin, int64_t ld_tab, int64_t tab_rows,
                               int feature_map, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws,
                               size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk, float scale, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev, full_dev);
    RC(cs_paged(s, pages, n_pages, table_dev, slot_dev, n_slots));
    return cs_step_dev_chain(s, DecTokens{CS_TOKENS}, CS_PROLOGUE, CS_ROWS, CS_PROBLEM(H, Hkv));
}

int mhla_causal_extend_paged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages,
                             const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev,
                             int n_slots, const int32_t* ntok_dev, int T, int64_t max_end, int max_later, int any_close, int left_padded,
                             mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B,
                             int H, int Hkv, int K, int V, int chunk, float scale, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev);
    RC(cs_paged(s, pages, n_pages, table_dev, slot_dev, n_slots));
    return cx_ragged_chain(false, s, DecTokens{CS_TOKENS, CS_WINDOW}, CS_ROWS, CS_PROBLEM(H, Hkv));
}

int mhla_causal_verify_paged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages,
                             const int32_t* table_dev, int cap_chunks, float* P, float* Cur, const int32_t* pos_dev, const int32_t* slot_dev,
                             int n_slots, const int32_t* ntok_dev, int T, int64_t max_end, int max_later, int any_close, int left_padded,
                             mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B,
                             int H, int Hkv, int K, int V, int chunk, float scale, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, const_cast<int32_t*>(pos_dev));
    RC(cs_paged(s, pages, n_pages, table_dev, slot_dev, n_slots));
    return cx_ragged_chain(true, s, DecTokens{CS_TOKENS, CS_WINDOW}, CS_ROWS, CS_PROBLEM(H, Hkv));
}

int mhla_causal_commit_paged(mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages, const int32_t* table_dev,
                             int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev, int n_slots,
                             const int32_t* ntok_dev, const int32_t* accept_dev, int T, int64_t max_end, int max_later, int any_close,
                             int left_padded, void* ws, size_t ws_bytes, int B, int H, int K, int V, int chunk, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev);
    RC(cs_paged(s, pages, n_pages, table_dev, slot_dev, n_slots));
    return cx_commit_chain(s, DecTokens{.k = k, .v = v, CS_WINDOW, .accept_dev = accept_dev}, DecProblem{CS_SIZES(B, H, H), CS_WS});
}

int mhla_causal_varlen_state_init_paged(mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages,
                                        const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int n_seqs, const int32_t* seq_len_dev,
                                        const int32_t* slot_dev, int n_slots, int max_len, int T, int H, int K, int V, int chunk, int n_chunks,
                                        const int32_t* chunk_tab_dev, const int32_t* chunk_dst_dev, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, nullptr);
    RC(cs_paged(s, pages, n_pages, table_dev, slot_dev, n_slots));
    return cs_pack_chain(k, v, s, CS_PACK, DecProblem{CS_SIZES(1, H, H)});
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
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev);
    RC(cs_packed(s, S, n_pages, table_dev, slot_dev, n_slots, off_dev));
    return cx_ragged_chain(false, s, DecTokens{CS_TOKENS, CS_PACKED}, CS_ROWS, CS_PROBLEM(H, Hkv));
}

int mhla_causal_verify_packed(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int n_pages,
                              const int32_t* table_dev, int cap_chunks, float* P, float* Cur, const int32_t* pos_dev, const int32_t* slot_dev,
                              int n_slots, const int32_t* off_dev, int n_tokens, int64_t max_end, int max_later, int any_close, mhla_mview out,
                              mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H,
                              int Hkv, int K, int V, int chunk, float scale, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, const_cast<int32_t*>(pos_dev));
    RC(cs_packed(s, S, n_pages, table_dev, slot_dev, n_slots, off_dev));
    return cx_ragged_chain(true, s, DecTokens{CS_TOKENS, CS_PACKED}, CS_ROWS, CS_PROBLEM(H, Hkv));
}

int mhla_causal_commit_packed(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int n_pages, const int32_t* table_dev,
                              int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev, int n_slots,
                              const int32_t* off_dev, const int32_t* accept_dev, int n_tokens, int64_t max_end, int max_later, int any_close,
                              void* ws, size_t ws_bytes, int B, int Hkv, int K, int V, int chunk, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev);
    RC(cs_packed(s, S, n_pages, table_dev, slot_dev, n_slots, off_dev));
    return cx_commit_chain(s, DecTokens{.k = k, .v = v, CS_PACKED, .accept_dev = accept_dev}, DecProblem{CS_SIZES(B, Hkv, Hkv), CS_WS});
}

// ---- h16 pages: the paged step, device-positioned step and pack prefill on a pool of 2-byte pages (mhla_hip.h), each through its
// namesake's chain
int mhla_causal_step_paged_h16(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, void* pages_h16, float* page_mult, int n_pages,
                               const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev,
                               int n_slots, int64_t max_pos, int any_boundary, mhla_mview out, mhla_view gate, const float* norm_w,
                               float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk,
                               float scale, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev);
    RC(cs_paged_h16(s, pages_h16, page_mult, n_pages, table_dev, slot_dev, n_slots, K, V));
    return cs_step_ragged_chain(s, DecTokens{CS_TOKENS}, max_pos, any_boundary, CS_ROWS, CS_PROBLEM(H, Hkv));
}

int mhla_causal_step_dev_paged_h16(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, void* pages_h16, float* page_mult,
                                   int n_pages, const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int32_t* pos_dev,
                                   const int32_t* slot_dev, int n_slots, int32_t* full_dev, const void* rope_cos, const void* rope_sin,
                                   int64_t ld_tab, int64_t tab_rows, int feature_map, mhla_mview out, mhla_view gate, const float* norm_w,
                                   float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk,
                                   float scale, int dtype, void* stream) {
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, pos_dev, full_dev);
    RC(cs_paged_h16(s, pages_h16, page_mult, n_pages, table_dev, slot_dev, n_slots, K, V));
    return cs_step_dev_chain(s, DecTokens{CS_TOKENS}, CS_PROLOGUE, CS_ROWS, CS_PROBLEM(H, Hkv));
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
    DecState s = cs_state(mix, ldmix, cap_chunks, P, Cur, nullptr);
    RC(cs_paged_h16(s, pages_h16, page_mult, n_pages, table_dev, slot_dev, n_slots, K, V));
    return cs_pack_chain(k, v, s, CS_PACK, DecProblem{CS_SIZES(1, H, H), CS_WS});
}

// ---- swap: the state of chosen slots of a paged pool out into one contiguous blob and back in (mhla_hip.h; kernels: causal_swap.hpp)
size_t mhla_causal_swap_ws_bytes(int n_seqs, int n_pages, int Hkv, int K, int V, int page_format) {
    if (n_seqs < 0 || n_pages < 0 || Hkv <= 0 || K <= 0 || V <= 0 || ((long)K * V) % 4) return 0;
    if (page_format != PF_F32 && (page_format != PF_H16 || ((long)K * V) % CSH_GROUP)) return 0;
    const CsSwapLayout l = cs_swap_layout(Hkv, K, V, page_format);
    return (size_t)n_seqs * l.seq_bytes + (size_t)n_pages * l.page_bytes;
}

// (swapping out writes nothing of the pool: its pointers are const in the ABI, and k_cs_swap<OUT> only reads through them)
int mhla_causal_swap_out_paged(const void* pages, const float* page_mult, int n_pages, const float* P, const float* Cur, const int32_t* pos_dev,
                               const int32_t* full_dev, int n_slots, const int32_t* items_dev, int n_seqs, int n_pages_moved, int i0, int i1,
                               void* blob_at, int Hkv, int K, int V, void* stream) {
    return cs_swap<true>(DecSwap{.pages = (void*)pages, .mult = (float*)page_mult, .n_pages = n_pages, .P = (float*)P, .Cur = (float*)Cur,
                                    .pos_dev = (int32_t*)pos_dev, .full_dev = (int32_t*)full_dev, .n_slots = n_slots, .items_dev = items_dev, .n_seqs = n_seqs,
                                    .n_moved = n_pages_moved, .i0 = i0, .i1 = i1, .blob = blob_at, .Hkv = Hkv, .K = K, .V = V, .stream = stream});
}

int mhla_causal_swap_in_paged(void* pages, float* page_mult, int n_pages, float* P, float* Cur, int32_t* pos_dev, int32_t* full_dev, int n_slots,
                              const int32_t* items_dev, int n_seqs, int n_pages_moved, int i0, int i1, const void* blob_at, int Hkv, int K, int V,
                              void* stream) {
    return cs_swap<false>(DecSwap{.pages = pages, .mult = page_mult, .n_pages = n_pages, .P = P, .Cur = Cur, .pos_dev = pos_dev, .full_dev = full_dev,
                                     .n_slots = n_slots, .items_dev = items_dev, .n_seqs = n_seqs, .n_moved = n_pages_moved, .i0 = i0, .i1 = i1,
                                     .blob = (void*)blob_at, .Hkv = Hkv, .K = K, .V = V, .stream = stream});
}

}  // extern "C"

#undef CS_TOKENS
#undef CS_WINDOW
#undef CS_PACKED
#undef CS_ROWS
#undef CS_PROLOGUE
#undef CS_PACK
#undef CS_SIZES
#undef CS_WS
#undef CS_PROBLEM
