/*
 * mhla_hip.h -- C ABI of libmhla_hip.so: the MI355X (gfx950) MHLA operator.
 *
 * This is the drop-in boundary for the MHLA hot path.  The reference
 * (DAGroup-PKU/MHLA) has no FFI / plugin registry: its boundary is plain Python
 * class substitution, and the operator itself is a handful of eager
 * torch.matmul / 1x1-conv calls.  Each entry point below names the reference
 * lines it replaces (paths relative to the reference tree).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer; the library owns no memory, all
 *     buffers (inputs, outputs, workspaces) belong to the caller;
 *   - all work is enqueued on the caller's `stream` (a hipStream_t passed as
 *     void*), nothing synchronises, no global mutable state: re-entrant;
 *   - token tensors are token-major `[B, N, H, D]` with ELEMENT strides
 *     (sb, sn, sh) and unit stride along D, so heads can be read in place from
 *     a fused QKV projection output; D and every stride must be multiples of 4
 *     elements and base pointers 16-byte aligned;
 *   - tokens are in block-major order (token p = m*S + s is offset s of block
 *     m); `block_index` (int32[N], may be NULL) maps block-major position p to
 *     the token's row in memory, which realises the reference's
 *     `rearrange(... "(fb p1 hb p2 wb p3) -> (fb hb wb) (p1 p2 p3)")` gather
 *     without a copy;
 *   - returns 0 on success, a negative MHLA_E* code otherwise (outputs
 *     untouched); mhla_last_error() gives a thread-local message.
 */
#ifndef MHLA_HIP_H
#define MHLA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHLA_ABI_VERSION 9

enum { MHLA_F32 = 0, MHLA_BF16 = 1, MHLA_F16 = 2 };

enum {
    MHLA_OK = 0,
    MHLA_EINVAL = -22,   /* bad shape / stride / alignment / flag combination */
    MHLA_ENOTSUP = -95,  /* shape outside what the kernels cover */
    MHLA_ELAUNCH = -5    /* HIP launch error */
};

/* flags */
#define MHLA_FLAG_RELU_EPS 1u      /* apply relu(x)+eps to q,k while loading (mhla_dit/mhla/mhla.py:229-230) */
#define MHLA_FLAG_FORCE_GENERIC 2u /* testing aid: take the generic fp32-MFMA path even where the bf16 fast path applies */
#define MHLA_FLAG_NO_SMALLN 4u     /* testing aid: skip the single-launch small-sequence path (S = 16, N <= 256) */
#define MHLA_FLAG_BF16_SUMMARIES 8u /* REDUCED PRECISION, opt-in, 16-bit tensors only: every intermediate that feeds a second
                                    * contraction -- the block summaries KV, G, dG, dKV, dP = dO / n, the score tiles of the
                                    * small-sequence path -- is kept as ONE bf16 value (what the reference's own matmuls store
                                    * under bf16 autocast; half the summary traffic; 2-3e-3 of the gradients' maximum).
                                    * bf16 tensors only (fp16 tensors: MHLA_EINVAL).  Default: bf16 hi + lo operand pairs and fp32
                                    * accumulation everywhere, summaries stored with >= 11 significand bits (see
                                    * MHLA_FLAG_FP32_GRADE_SUMMARIES), one rounding of the results at the store. */

#define MHLA_FLAG_FP32_GRADE_SUMMARIES 32u /* 16-bit tensors, opt-in: keep >= 16 significand bits in the block summaries (24-bit floats /
                                    * fp32 words in the workspace: round 5's default).  DEFAULT since ABI 9 for bf16 / fp16 tensors
                                    * with blocks of >= 16 tokens, D <= 96, M <= 128: KV, G, dG, dKV are stored in 2 bytes as an fp16
                                    * payload x one power-of-two multiplier per block row -- 11 significand bits, what the
                                    * reference's own matmul / 1x1 conv (mhla_dit/mhla/mhla.py:262-263) run at under
                                    * torch.backends.cuda.matmul.allow_tf32 = True (mhla_dit/train.py:12-13); operands stay bf16
                                    * hi + lo pairs, accumulation fp32; <= 4e-4 of a result's maximum from the fp32 result
                                    * (tools/sim_h16.py, tests).  fp32 tensors are never affected. */
#define MHLA_FLAG_NO_BWD_STATE 16u  /* mhla_blockmix_fwd: no backward will use this forward's workspace (inference) -- skip what only
                                    * the backward reads (16-bit tensors, default arithmetic: the bf16 residual O - fl(O) that
                                    * gives the backward's row dots dO . O an fp32-grade O).  A backward given this flag
                                    * recomputes it. */

/* flags of the causal entry points (mhla_causal_*) */
#define MHLA_CAUSAL_FORCE_GENERIC 1u   /* testing aid: the generic kernels (exact fp32 MFMA, fp32 summaries) for every shape */
#define MHLA_CAUSAL_BF16_SUMMARIES 2u  /* REDUCED PRECISION, opt-in: chunk summaries S, P, dP, dS and the score tiles as single
                                        * bf16 values (half the summary traffic; 2-3e-3 of the result's maximum).  Default: bf16
                                        * hi + lo pairs, >= 16 significand bits wherever the reference holds fp32
                                        * (mhla_nlp/fla/ops/mhla/naive.py:39, :60-78). */

#define MHLA_CAUSAL_FP32_GRADE_SUMMARIES 4u /* opt-in: chunk summaries as bf16 hi + lo pairs (>= 16 significand bits, 4 bytes per element: round
                                        * 5's default).  DEFAULT since ABI 9 on the 16-bit pipeline: S, P, dP, dS are stored as an fp16
                                        * payload x one power-of-two multiplier per 16-row strip of a 64 x 64 chunk tile -- 11
                                        * significand bits (TF32 grade), 2 bytes; score tiles and operands stay bf16 hi + lo pairs with
                                        * fp32 accumulation; <= 4.4e-4 of a result's maximum from the fp32 result
                                        * (tools/sim_h16_causal.py, tests). */

/* A token-major view [B, N, H, D]: element strides, D contiguous. */
typedef struct {
    const void* ptr;
    int64_t sb, sn, sh;
} mhla_view;

typedef struct {
    void* ptr;
    int64_t sb, sn, sh;
} mhla_mview;

int mhla_abi_version(void);
/* Device-code options the library was compiled with, e.g. "gfx950 -O3 no-packed-fp32" (mhla_amd/build.py); the Python loader
 * refuses a library built with another set. */
const char* mhla_build_flags(void);
const char* mhla_last_error(void);

/* Process-wide options.  "bwd_two_launches" (0 / 1): run the two tile roles of the bf16-summary fast path's backward as two
 * launches instead of one fused launch with an in-launch hand-over; the library sets it itself, asynchronously and without any
 * synchronisation, after a fused launch reported an expired hand-over (see mhla_blockmix_bwd_status).  "debug_drop_signal" (0 / 1):
 * testing aid for that bounded wait.  "fp32_summaries" (0 / 1): the block-mixing operator's default arithmetic keeps its block
 * summaries as fp32 words in the workspace instead of 24-bit floats (a measurement aid: same 16-significand-bit operands either
 * way; set it between calls, not between a forward and the backward that reuses its workspace).  "recut_kernels" (1 / 0): 0 runs the
 * kernels that the re-cut ones replaced -- the twelve / sixteen-wave payload mixing at 129 .. 256 blocks, the block-per-workgroup Wan
 * inference output kernel, the tile-loop forms of k_sp_out / k_sp_bwd_dq at blocks of at most 64 tokens and k_sp_state with its
 * stand-in third row stream -- with bit-identical results (A/B timing, equality tests).  Initial values:
 * MHLA_BWD_TWO_LAUNCHES=1 / MHLA_DEBUG_DROP_SIGNAL=1 / MHLA_FP32_SUMMARIES=1 / MHLA_RECUT=0 in the environment when the library is loaded.
 * Returns the previous value, MHLA_EINVAL for an unknown name. */
int mhla_set_option(const char* name, int value);

/* Which kernel family, block-summary format and launch sequence serve a block-mix / causal problem, as text:
 * "family=...; summaries=...; fwd=k1 k2 ...; bwd=k1 k2 ..." (kernel names as mhla_prof_report prints them, separated by blanks; the
 * dispatcher's own predicates; 16-byte aligned views assumed).
 * Writes at most cap - 1 characters + NUL into buf (buf may be NULL), returns the full length or a negative error code.  The
 * table in DESIGN.md section 0a lists the same for every BASELINE.json configuration. */
int mhla_describe_dispatch(int B, int H, int M, int S, int D, int dtype, int split, unsigned flags, char* buf, size_t cap);
int mhla_causal_describe_dispatch(int T, int K, int V, int chunk, int dtype, unsigned flags, char* buf, size_t cap);

/* Profiling aid (used by bench.py): when enabled, every kernel launch is bracketed by hipEvents on
 * its own stream; mhla_prof_report waits for them, writes one "kernel_name count total_ms" line per
 * kernel into buf (NUL-terminated, truncated to cap) and clears the records.  Off by default. */
void mhla_prof_enable(int on);
int mhla_prof_report(char* buf, size_t cap);
/* Debugging aid (tools/trace_tiles.py): when buf is a device buffer of 3 * tile_workgroups * 16 uint64, the three tile
 * kernels of the bf16 fast path write per-workgroup phase timestamps (s_memtime ticks) into it; NULL switches it off. */
void mhla_debug_set_trace(void* buf);

/* ---- block-mixing (non-causal) MHLA: DiT / ViT / Wan ------------------- */

/* Bytes of workspace mhla_blockmix_fwd / _bwd need for this problem (dtype: MHLA_F32/BF16/F16;
 * split: 1 when q_den/k_den do not alias q_num/k_num; flags: the flags of the call). */
size_t mhla_blockmix_fwd_ws_bytes(int B, int H, int M, int S, int D, int dtype, int split, unsigned flags);
size_t mhla_blockmix_bwd_ws_bytes(int B, int H, int M, int S, int D, int dtype, int split, unsigned flags);
/* 1 when the forward leaves reusable block summaries in `ws` (pass that buffer as `fwd_ws` to the backward). */
int mhla_blockmix_fwd_keeps_state(int B, int H, int M, int S, int D, int dtype, int split, unsigned flags);

/*
 * Forward.  Replaces mhla_dit/mhla/mhla.py:262-268 (identical:
 * mhla_image_classification/models/modules/attention/mhla.py:275-282) and
 * mhla_videogen/diffusion/model/wan/mhla_utils.py:331-341:
 *   KV_j = K_j^T V_j ; G_i = sum_j W[i,j] KV_j ;
 *   z_j[s] = Qd_j[s] . sum_s' Kd_j[s'] ; n_i[s] = sum_j W[i,j] z_j[s] + eps ;
 *   O_i = (Q_i G_i) / n_i          (no division when q_den.ptr == NULL).
 * q_num/k_num feed KV and the numerator, q_den/k_den the normaliser (Wan passes
 * roped / un-roped pairs); q_den may alias q_num (same ptr) -- the DiT/ViT case.
 * W is [M, M] fp32 row-major (row = output block i, col = input block j), ldw
 * its row stride.
 */
int mhla_blockmix_fwd(mhla_view q_num, mhla_view k_num, mhla_view v,
                      mhla_view q_den, mhla_view k_den,
                      const float* W, int ldw, mhla_mview out,
                      const int32_t* block_index, void* ws, size_t ws_bytes,
                      int B, int H, int M, int S, int D,
                      int dtype, float eps, unsigned flags, void* stream);

/*
 * Forward with the rotary prologue of the Wan host fused in (inference): replaces
 * wan/mhla_utils.py:314 (rope_apply of q and k, :127-156) + :317-341.  q, k are the un-rotated
 * tensors; the kernels rotate consecutive channel pairs (2i, 2i+1) of token row n by
 * (rope_cos[n*ld_rope + i], rope_sin[n*ld_rope + i]) while loading them: rotated k feeds KV,
 * rotated q the numerator, the plain q, k the normaliser (normalize != 0).  The tables are
 * [rows of one batch item][D/2] fp32, indexed by the token's memory row (the same index
 * block_index maps to), shared by all heads and batch items.  No q_rope / k_rope tensors exist.
 * Workspace: mhla_blockmix_fwd_ws_bytes(..., split = 0, flags).  Needs D % 8 == 0.
 * fp32 tensors; 16-bit tensors only where their summaries are fp32 words or bf16 (head dims above 96, MHLA_FLAG_BF16_SUMMARIES, the
 * "fp32_summaries" option).  On h16 / p24 summaries a 16-bit call is refused with MHLA_ENOTSUP during argument validation -- no
 * rotary summary kernel is built for it: pass fp32 tensors, or rotate on the host and call mhla_blockmix_fwd(q_rope, k_rope, v,
 * q_den = q, k_den = k).
 */
int mhla_blockmix_rope_fwd(mhla_view q, mhla_view k, mhla_view v, int normalize,
                           const float* W, int ldw,
                           const float* rope_cos, const float* rope_sin, int64_t ld_rope,
                           mhla_mview out, const int32_t* block_index,
                           void* ws, size_t ws_bytes,
                           int B, int H, int M, int S, int D,
                           int dtype, float eps, unsigned flags, void* stream);

/*
 * The Wan layer's operator with prologue and epilogue fused (inference): as mhla_blockmix_rope_fwd (rope tables
 * optional: NULL = no rotation), and the per-head RMSNorm (x SiLU gate) that follows the operator in the host
 * (wan/mhla_utils.py:356-362: out.to(dtype); g_norm(out) [* silu(g)]) applied to each token's D outputs before
 * they are stored:  y = rmsnorm_D(round_out_dtype(O)) * norm_w [* gate * sigmoid(gate)].  q, k, v are fp32 (`dtype`
 * must be MHLA_F32, the host's .float() at :308); `out` and `gate` ([B, N, H, D] views) are in `out_dtype`.
 * norm_w: fp32 [D] or NULL; gate.ptr NULL = no gate.  The fp32 O tensor is never written.
 */
int mhla_blockmix_wan_fwd(mhla_view q, mhla_view k, mhla_view v, int normalize,
                          const float* W, int ldw,
                          const float* rope_cos, const float* rope_sin, int64_t ld_rope,
                          const float* norm_w, float norm_eps, mhla_view gate,
                          mhla_mview out, int out_dtype, const int32_t* block_index,
                          void* ws, size_t ws_bytes,
                          int B, int H, int M, int S, int D,
                          int dtype, float eps, unsigned flags, void* stream);

/*
 * mhla_blockmix_wan_fwd with the q / k prologue of the Wan layer (wan/mhla_utils.py:268-272 after the .float() at :308:
 * relu(rmsnorm_C(x) * w) + eps over the full channel dim C = H * D) folded into the operator's loads ("read directly
 * from the QKV GEMM output").  q, k, v: the 16-bit projection outputs [B, N, H, D] (`dtype` MHLA_BF16 / MHLA_F16, 16-byte aligned
 * views), read in place; rstd_q / rstd_k: fp32 [B * N], 1 / sqrt(mean_C(x^2) + norm_eps) per token from mhla_rms_rstd (NULL: no
 * norm); wq / wk: fp32 [H * D] RMSNorm weights (NULL: 1).  The kernels form relu(x * rstd * w) + eps in fp32 while loading -- the
 * values mhla_qk_prologue writes as fp32 tensors -- then rotate (rope tables optional), multiply with bf16 hi + lo operands, and
 * apply the per-head norm x gate epilogue; the fp32 q / k / v tensors never exist.  Workspace: mhla_blockmix_fwd_ws_bytes(..,
 * MHLA_F32, 0, 0).  mhla_blockmix_wan_pro_ok: 1 when this entry point serves the problem (16-bit tensors, 96 < D <= 128, D % 8 == 0,
 * at most 192 blocks); otherwise MHLA_ENOTSUP and the caller composes mhla_qk_prologue + mhla_blockmix_wan_fwd.
 */
int mhla_blockmix_wan_pro_ok(int M, int S, int D, int dtype, unsigned flags);
int mhla_blockmix_wan_pro_fwd(mhla_view q, mhla_view k, mhla_view v,
                              const float* rstd_q, const float* rstd_k, const float* wq, const float* wk, int normalize,
                              const float* W, int ldw,
                              const float* rope_cos, const float* rope_sin, int64_t ld_rope,
                              const float* norm_w, float norm_eps, mhla_view gate,
                              mhla_mview out, int out_dtype, const int32_t* block_index,
                              void* ws, size_t ws_bytes,
                              int B, int H, int M, int S, int D,
                              int dtype, float eps, unsigned flags, void* stream);
/* rstd[row] = 1 / sqrt(mean(x[row][0 .. C)^2) + norm_eps): x [rows][ldx] in `dtype`, C % 8 == 0, rstd fp32 [rows]. */
int mhla_rms_rstd(const void* x, int64_t ldx, float* rstd, int64_t rows, int C, float norm_eps, int dtype, void* stream);

/*
 * Backward (autograd of the forward above; hand-derived).
 * Needs only the forward's inputs, its output `out` and the upstream gradient
 * `dout`: the block summaries are recomputed -- unless the caller kept the
 * forward's workspace and passes it as `fwd_ws` (same call arguments, contents
 * untouched since mhla_blockmix_fwd returned; NULL = recompute).  dq_den/dk_den are
 * written only when q_den does not alias q_num; otherwise both parts are summed
 * into dq_num/dk_num.  dW is [M, M] fp32 (ld = M), overwritten (not
 * accumulated), reduced over (b, h) in a fixed order: deterministic.
 */
int mhla_blockmix_bwd(mhla_view q_num, mhla_view k_num, mhla_view v,
                      mhla_view q_den, mhla_view k_den,
                      const float* W, int ldw, mhla_view out, mhla_view dout,
                      mhla_mview dq_num, mhla_mview dk_num, mhla_mview dv,
                      mhla_mview dq_den, mhla_mview dk_den, float* dW,
                      const int32_t* block_index, void* ws, size_t ws_bytes,
                      const void* fwd_ws,
                      int B, int H, int M, int S, int D,
                      int dtype, float eps, unsigned flags, void* stream);

/* Backward of mhla_blockmix_rope_fwd (the rope of wan/mhla_utils.py:314 inside the operator's backward).
 * q, k: the UN-rotated tensors the forward was given (numerator pair = their rotation, normaliser pair = themselves when
 * normalize != 0); out / dout as in mhla_blockmix_bwd; dq, dk: gradients w.r.t. the un-rotated q, k (the transposed rotation
 * of the numerator gradients and the normaliser's part are summed inside the kernels) -- replaces autograd through
 * rope_apply (mhla_utils.py:127-156) and the 5-tensor concat / rearrange (:317-326) in the backward direction.
 * fp32 tensors, D % 8 == 0.  fwd_ws: workspace of mhla_blockmix_rope_fwd for the same arguments, or NULL. */
int mhla_blockmix_rope_bwd(mhla_view q, mhla_view k, mhla_view v, int normalize, const float* W, int ldw,
                           const float* rope_cos, const float* rope_sin, int64_t ld_rope, mhla_view out, mhla_view dout,
                           mhla_mview dq, mhla_mview dk, mhla_mview dv, float* dW, const int32_t* block_index, void* ws,
                           size_t ws_bytes, const void* fwd_ws, int B, int H, int M, int S, int D, int dtype, float eps,
                           unsigned flags, void* stream);

/* Status of the last mhla_blockmix_bwd that used `ws` (same problem arguments).  The bf16 fast path hands a tile's dksum rows
 * from its dQ workgroup to its dK/dV workgroup inside one launch through a flag; the wait for that flag is bounded, and a
 * waiter that gives up raises an error word in the workspace.  This call synchronises `stream`, reads the word and returns
 * MHLA_ELAUNCH if it is set (dk is then invalid), MHLA_OK otherwise -- also for problems that take another path.
 * Replaces nothing in the reference (mhla_dit/mhla/mhla.py:262-268 is a sequence of separate kernels); it is the fail-safe
 * of this library's own fusion.  Without this call the failure is still loud (dk = NaN) and self-healing: the library reads the
 * word asynchronously after every fused launch and runs the two roles as two launches from the next backward on (mhla_set_option). */
int mhla_blockmix_bwd_status(const void* ws, size_t ws_bytes, int B, int H, int M, int S, int D, int dtype, int split,
                             unsigned flags, void* stream);

/* ---- causal chunk-mixing MHLA: fla ------------------------------------- */

/* Workspace bytes.  bf16 tensors with K, V multiples of 64, K <= 256 and at most 256 chunks run the 16-bit-MFMA pipeline,
 * whose chunk summaries are bf16 hi + lo pairs (4 bytes per element; 2 with MHLA_CAUSAL_BF16_SUMMARIES); everything else the
 * generic kernels with fp32 summaries.  `flags` must be the flags of the calls the workspace is for. */
size_t mhla_causal_fwd_ws_bytes(int B, int T, int H, int K, int V, int chunk, int dtype, unsigned flags);
size_t mhla_causal_bwd_ws_bytes(int B, int T, int H, int K, int V, int chunk, int dtype, unsigned flags);

/*
 * Forward.  Replaces naive_chunk_simple_mhla_fixed
 * (mhla_nlp/fla/ops/mhla/naive.py:10-83): fp32 compute, q scaled by `scale`
 * (the reference always uses K^-0.5), T right-padded with zeros to a multiple
 * of `chunk`, S_j = K_j^T V_j,
 *   O_i = Q_i (sum_{j<i} mix[i,j] S_j) + mix[i,i] tril(Q_i K_i^T) V_i.
 * q,k: [B,T,H,K]  v,out: [B,T,H,V]  mix: fp32 [n.., n..] row stride ldmix,
 * n = ceil(T/chunk) rows/cols are read.  chunk must be 64.
 * Arithmetic: every product accumulates in fp32 and every intermediate that the reference keeps in fp32 (naive.py:39,
 * :60-78: S_j, the prefix mix, tril(Q K^T)) keeps >= 16 significand bits (exact fp32 MFMA on the generic path, bf16 hi + lo
 * pairs on the 16-bit pipeline); one rounding to the tensor dtype at the store (naive.py:82).
 */
int mhla_causal_fwd(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix,
                    mhla_mview out, void* ws, size_t ws_bytes,
                    int B, int T, int H, int K, int V, int chunk,
                    float scale, int dtype, unsigned flags, void* stream);

/* N1: the causal operator with the fla layer's epilogue fused into its store --
 *   y = o * rsqrt(mean(o^2 over V) + norm_eps) * norm_w * gate * sigmoid(gate)
 * i.e. FusedRMSNormGated over each head's V channels (mhla_nlp/fla/layers/mhla.py:351-355; kernel math
 * mhla_nlp/fla/modules/fused_norm_gate.py:77-99).  `out` (the operator's own output o) is optional: a NULL ptr skips its
 * store (inference); training passes it so that the norm's backward (mhla_rmsnorm_gate_bwd) has its input.  `gate` ptr NULL:
 * no gate; `norm_w` NULL: no affine weight.  Covers what mhla_causal_normgate_fusable() reports (bf16 tensors, K % 64 == 0,
 * K <= 256, V % 64 == 0 with V <= 256 or V = 384 / 512 -- one workgroup owns a head's channels, the wide heads in two halves --,
 * at most 256 chunks); otherwise MHLA_ENOTSUP and
 * the caller runs mhla_causal_fwd + mhla_rmsnorm_gate_fwd.  Workspace: as mhla_causal_fwd (usable as `fwd_ws` of
 * mhla_causal_bwd with the same flags). */
int mhla_causal_normgate_fusable(int T, int K, int V, int chunk, int dtype, unsigned flags);
int mhla_causal_normgate_fwd(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, mhla_mview out, mhla_view gate,
                             const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int T, int H,
                             int K, int V, int chunk, float scale, int dtype, unsigned flags, void* stream);

/* Backward (autograd of naive.py:39-82).  dmix is [n, n] fp32 with row stride lddmix;
 * every entry of the leading n x n is written (zeros above the diagonal).
 * fwd_ws: the workspace mhla_causal_fwd was given for the same arguments and flags, contents untouched
 * (its chunk summaries S_j and the prefix mixes are reused), or NULL to recompute them. */
int mhla_causal_bwd(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix,
                    mhla_view dout, mhla_mview dq, mhla_mview dk, mhla_mview dv,
                    float* dmix, int lddmix, void* ws, size_t ws_bytes, const void* fwd_ws,
                    int B, int T, int H, int K, int V, int chunk,
                    float scale, int dtype, unsigned flags, void* stream);

/* Packed sequences (cu_seqlens): one row of T tokens (B = 1 by convention; B > 1 applies the same table to every batch row) holds
 * several sequences, and each is computed exactly as if it were alone in a call of its own (added without a change of any
 * existing signature or behaviour: MHLA_ABI_VERSION stays 9).  The caller cuts every sequence into its own 64-token chunks
 * (ragged last chunk, none for an empty sequence), numbers them c = 0 .. n_chunks - 1 along the pack and passes
 *   chunk_tab_dev  device int32 [n_chunks][2]: {first token row, rows in 1 .. 64} of chunk c, 8-byte aligned
 *   mix            fp32 [n_chunks, n_chunks]: mix_eff[c][c'] = mix[loc(c)][loc(c')] where c, c' belong to the same sequence
 *                  and c' <= c (loc: the chunk's index within its sequence), 0 elsewhere.
 * The calls are then the uniform calls above over n_chunks chunks: the same kernels (the token-facing ones take a chunk's rows
 * from the table instead of from its index), grids, dispatch -- the 16-bit pipeline serves bf16 with K, V multiples of 64,
 * K <= 256 and n_chunks <= 256 -- and workspace layout, all by n_chunks; T stays the token count of the views.  dmix is the
 * gradient of mix_eff, [n_chunks, n_chunks].  The table lives on the device and is NOT read by the validation, which checks
 * n_chunks in ceil(T / 64) .. T and what the uniform calls check: its contents are the caller's contract -- rows
 * start .. start + count - 1 inside 0 .. T - 1 and disjoint between chunks (rows that no chunk covers are not written).
 * mhla_causal_varlen_normgate_fusable: mhla_causal_normgate_fusable by n_chunks. */
size_t mhla_causal_varlen_fwd_ws_bytes(int B, int T, int H, int K, int V, int chunk, int n_chunks, int dtype, unsigned flags);
size_t mhla_causal_varlen_bwd_ws_bytes(int B, int T, int H, int K, int V, int chunk, int n_chunks, int dtype, unsigned flags);
int mhla_causal_varlen_normgate_fusable(int T, int K, int V, int chunk, int n_chunks, int dtype, unsigned flags);
int mhla_causal_varlen_fwd(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, mhla_mview out, void* ws,
                           size_t ws_bytes, int B, int T, int H, int K, int V, int chunk, int n_chunks, const int* chunk_tab_dev,
                           float scale, int dtype, unsigned flags, void* stream);
int mhla_causal_varlen_normgate_fwd(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, mhla_mview out, mhla_view gate,
                                    const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int T, int H,
                                    int K, int V, int chunk, int n_chunks, const int* chunk_tab_dev, float scale, int dtype,
                                    unsigned flags, void* stream);
int mhla_causal_varlen_bwd(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, mhla_view dout, mhla_mview dq,
                           mhla_mview dk, mhla_mview dv, float* dmix, int lddmix, void* ws, size_t ws_bytes, const void* fwd_ws,
                           int B, int T, int H, int K, int V, int chunk, int n_chunks, const int* chunk_tab_dev, float scale, int dtype,
                           unsigned flags, void* stream);

/* Grouped-query heads in the forward (added without a change of any existing signature or behaviour: MHLA_ABI_VERSION stays 9).
 * Each call is its namesake with one more integer, Hkv, after H: q, out, gate, y have H heads, k [B,T,Hkv,K] and v [B,T,Hkv,V] have
 * Hkv, H = G Hkv, and query head h reads k/v head h / G (the layer's repeat order).  The result is, bit for bit, the namesake's on
 * k, v repeated G times per head: the chunk summaries and their prefix mixes are formed once per k/v head -- the same sums in the
 * same order -- and the output kernel's arithmetic per query head is the namesake's.  MHLA_EINVAL for Hkv < 1 or H % Hkv != 0,
 * MHLA_ENOTSUP for G > 8; B * H <= 65535 counts query heads; every other check as the namesake.  Hkv == H makes the namesake's own
 * launches.  Workspace: exactly mhla_causal_fwd_ws_bytes(B, T, Hkv, ...) / mhla_causal_varlen_fwd_ws_bytes(B, T, Hkv, ...) -- 1 / G
 * of the namesake's -- and mhla_causal_normgate_fusable / mhla_causal_varlen_normgate_fusable answer unchanged (they take no head
 * count).  There is no grouped backward: mhla_causal_bwd takes k, v on H heads, and a workspace these calls filled is not a
 * `fwd_ws` for it. */
int mhla_causal_fwd_gqa(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, mhla_mview out, void* ws, size_t ws_bytes,
                        int B, int T, int H, int Hkv, int K, int V, int chunk, float scale, int dtype, unsigned flags, void* stream);
int mhla_causal_normgate_fwd_gqa(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, mhla_mview out, mhla_view gate,
                                 const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int T, int H,
                                 int Hkv, int K, int V, int chunk, float scale, int dtype, unsigned flags, void* stream);
int mhla_causal_varlen_fwd_gqa(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, mhla_mview out, void* ws,
                               size_t ws_bytes, int B, int T, int H, int Hkv, int K, int V, int chunk, int n_chunks,
                               const int* chunk_tab_dev, float scale, int dtype, unsigned flags, void* stream);
int mhla_causal_varlen_normgate_fwd_gqa(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, mhla_mview out,
                                        mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes,
                                        int B, int T, int H, int Hkv, int K, int V, int chunk, int n_chunks, const int* chunk_tab_dev,
                                        float scale, int dtype, unsigned flags, void* stream);

/* Decoding (generation): the state of a sequence and the single-token step.  Row t of the forward above depends on the
 * tokens <= t only, so a step reproduces it from, per (b, h), in fp32 whatever the tensor dtype:
 *   S   [B][H][cap_chunks][K][V]  K_j^T V_j of every finished chunk j (mix[i][j] differs per row i: all are kept --
 *                                 4 K V bytes per chunk and head, 128 KB at K = 128, V = 256)
 *   P   [B][H][K][V]              the prefix mix sum_{j<i} mix[i][j] S[j] of the open chunk i
 *   Cur [B][H][K][V]              the open chunk's running K^T V
 * all dense and 16-byte aligned; an empty state (no token seen) is P = Cur = 0.
 * mhla_causal_state_init: the state after the T tokens of k, v ([B,T,H,K], [B,T,H,V]); needs ceil(T / chunk) <= cap_chunks and,
 * unless the state is then full, ldmix > T / chunk.  Rows of S beyond the finished chunks are neither read nor written.
 * mhla_causal_step: one token (q, k: [B,1,H,K]; v, out, y, gate: [B,1,H,V]) at position `pos` = tokens seen so far, with
 * i = pos / chunk:  Cur += k (x) v;  out = scale q^T (P + mix[i][i] Cur);  at pos % chunk == chunk - 1 the chunk closes:
 * S[i] = Cur, Cur = 0, P = sum_{j<=i} mix[i+1][j] S[j] (P = 0 when i + 1 == cap_chunks: the state is full).  The caller
 * advances pos.  `y` non-NULL: the epilogue of mhla_causal_normgate_fwd on this token (`gate` ptr NULL: no gate, `norm_w`
 * NULL: no weight), and `out` may then be a NULL ptr.  MHLA_EINVAL when pos / chunk >= cap_chunks, when ldmix does not cover
 * the row of mix the call reads, or when ws_bytes < mhla_causal_step_ws_bytes (pure host arithmetic).  K, V multiples of 4,
 * chunk 64, B*H <= 65535.  No atomics: results repeat bit for bit. */
size_t mhla_causal_step_ws_bytes(int B, int H, int K, int V, int dtype);
int mhla_causal_state_init(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                           int B, int T, int H, int K, int V, int chunk, int dtype, void* stream);
int mhla_causal_step(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                     float* Cur, int64_t pos, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y,
                     void* ws, size_t ws_bytes, int B, int H, int K, int V, int chunk, float scale, int dtype, void* stream);

/* mhla_causal_varlen_state_init: mhla_causal_state_init for a pack (cu_seqlens) -- the ragged decode state of every sequence of
 * one packed row k [1,T,H,K], v [1,T,H,V] in one launch chain (two launches, whatever n_seqs; added without a change of any existing
 * signature or behaviour: MHLA_ABI_VERSION stays 9).  S [n_seqs][H][cap_chunks][K][V], P and Cur [n_seqs][H][K][V] as above.
 *   chunk_tab_dev  the table of mhla_causal_varlen_fwd: device int32 [n_chunks][2] {first token row, rows in 1 .. 64}, 8-byte aligned
 *   chunk_dst_dev  device int32 [n_chunks][2]: {sequence, index of the chunk within its sequence} of chunk c
 *   seq_len_dev    device int32 [n_seqs]: the tokens of every sequence -- the ragged state's position array
 *   max_len        host value: the longest sequence
 * Per sequence s of n = seq_len_dev[s] tokens and per head, with nfull = n / 64: S[s][h][j] = K_j^T V_j of every finished chunk
 * j < nfull (a last chunk of exactly 64 rows is finished); Cur[s][h] the K^T V of the ragged last chunk, zeros when n % 64 == 0
 * (an empty sequence included); P[s][h] = sum_{j<nfull} mix[nfull][j] S[j] in ascending j, zeros when nfull == 0 or
 * nfull == cap_chunks (the state is full).  P and Cur of every sequence are written by the call itself; rows of S beyond the
 * finished chunks are neither read nor written.  Exact fp32 products, the kernels and the order of every sum of
 * mhla_causal_state_init: the result is bit for bit what that call leaves for the sequence alone.  No atomics.
 * The three arrays live on the device and are NOT read by the validation (host arithmetic only, before any launch): what
 * mhla_causal_state_init checks of dimensions, views and state; n_seqs > 0; n_seqs * H <= 65535 (MHLA_ENOTSUP); T > 0 and
 * n_chunks in ceil(T / 64) .. T (an all-empty pack is an all-zero state, the caller's to make); 0 <= max_len <= T;
 * ceil(max_len / 64) <= cap_chunks; ldmix covers row min(max_len / 64, cap_chunks - 1) of mix; the arrays non-null and 4-byte
 * aligned, the chunk table 8-byte.  Their contents are the caller's contract (the table as for mhla_causal_varlen_fwd; the
 * destinations distinct); as a defence only, a seq_len_dev[s] outside 0 .. max_len leaves P and Cur of that sequence untouched,
 * and a destination outside n_seqs / cap_chunks is not written. */
int mhla_causal_varlen_state_init(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                                  int n_seqs, const int32_t* seq_len_dev, int max_len, int T, int H, int K, int V, int chunk,
                                  int n_chunks, const int32_t* chunk_tab_dev, const int32_t* chunk_dst_dev, int dtype, void* stream);

/* mhla_causal_step_ragged: mhla_causal_step for a batch whose sequences are at positions of their own (added without a change of
 * any existing signature or behaviour: MHLA_ABI_VERSION stays 9).  `pos_dev`: device int32 [B], tokens seen by each sequence.
 * Sequence b behaves as in a batch of one: i = pos_dev[b] / chunk, its out row uses mix[i][i], and it closes its chunk -- S[i] = Cur,
 * Cur = 0, P from row i + 1 of mix, or P = 0 when i + 1 == cap_chunks -- only if pos_dev[b] % chunk == chunk - 1.  The call itself
 * adds one to every pos_dev[b], in its last launch and in stream order (no copy, no synchronisation; the earlier launches of
 * the chain address by pos_dev, the last does not), so the array is the caller's to keep in step with, not to advance.
 * The library cannot read device memory to validate, hence two host values: `max_pos`, the largest entry of pos_dev, which
 * takes the place of `pos` in the MHLA_EINVAL checks of mhla_causal_step (cap_chunks, ldmix, the rows of mix read); and
 * `any_boundary`, non-zero when at least one sequence is at pos % chunk == chunk - 1 (zero: the boundary kernel is not
 * launched, and no chunk closes).  Restriction: with any_boundary the row after chunk max_pos / chunk must be covered by ldmix
 * unless that chunk is the state's last, whichever sequence is the one on the boundary (MHLA_EINVAL otherwise, before any
 * launch).  pos_dev must hold what max_pos and any_boundary were computed from; an array that disagrees is the caller's
 * error and gives wrong rows.  As a defence only, an entry outside 0 .. max_pos is never used to address: the step clamps
 * it, the boundary kernel skips that sequence.  Tiling and the order of every sum are those of mhla_causal_step: equal
 * positions give the same bits.  Workspace: mhla_causal_step_ws_bytes. */
int mhla_causal_step_ragged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                            float* Cur, int32_t* pos_dev, int64_t max_pos, int any_boundary, mhla_mview out, mhla_view gate,
                            const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int K, int V,
                            int chunk, float scale, int dtype, void* stream);

/* mhla_causal_step_dev: the device-positioned step -- mhla_causal_step_ragged whose launch chain and arguments depend on no
 * position, so that one captured graph (hipGraph) replays it token after token (added without a change of any existing signature
 * or behaviour: MHLA_ABI_VERSION stays 9).  No `max_pos`, no `any_boundary`: every call enqueues the same three launches (step,
 * boundary, finish), and the bound on pos_dev[b] is the state's capacity.  Per sequence b, with p = pos_dev[b] read on the device:
 *   LIVE   (0 <= p < chunk * cap_chunks): exactly the ragged step (the same bits); the chunk closes only if p % chunk == chunk - 1
 *          (P from row p / chunk + 1 of mix, or P = 0 when that chunk was the state's last); pos_dev[b] = p + 1.
 *   FROZEN (any other p -- a sequence whose state is full, or a caller's mark such as -1): a defined branch, not an error: S, P,
 *          Cur and pos_dev[b] are untouched, the sequence's row of `out` / `y` is written as zeros (o = 0 through the epilogue: y
 *          is zero for finite gate and weight), and full_dev[b] = 1.  full_dev (device int32 [B]) is never cleared by the library.
 * No content of pos_dev can address outside S, the matrix or the tables: chunk index and matrix row are < cap_chunks, the table
 * row < tab_rows.  Hence the static checks, all MHLA_EINVAL before any launch: ldmix >= cap_chunks (the matrix has at least
 * cap_chunks rows, any of which may be read); workspace as mhla_causal_step_ws_bytes; the others as mhla_causal_step.
 * Fused q / k prologue of the fla layer (the call then takes the projections' q and k): `feature_map` (0 identity, 1 relu,
 * 2 elu + 1) and then, with `rope_cos` / `rope_sin` (given together or both NULL), the NeoX rotary at row p of the tables --
 * [tab_rows][K/2] in the tensor dtype with row stride ld_tab, as mhla_featmap_rotary takes them (ld_tab >= K / 2, a multiple of 4,
 * bases aligned to 4 elements) and tab_rows >= chunk * cap_chunks.  Needs K % 8 == 0.  The fp32 arithmetic is that of
 * mhla_featmap_rotary and the result is rounded to the tensor dtype where that call stores it, so a state advanced by fused
 * steps is the state mhla_featmap_rotary + mhla_causal_step(_ragged) leave, bit for bit. */
int mhla_causal_step_dev(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                         float* Cur, int32_t* pos_dev, int32_t* full_dev, const void* rope_cos, const void* rope_sin, int64_t ld_tab,
                         int64_t tab_rows, int feature_map, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                         mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int K, int V, int chunk, float scale, int dtype,
                         void* stream);

/* mhla_causal_extend: T >= 1 new tokens (q, k: [B,T,H,K]; v, out, y, gate: [B,T,H,V]) on a state with `pos` tokens seen, in a
 * number of launches that does not depend on T.  out = rows pos .. pos + T - 1 of the forward over the whole sequence, the
 * state afterwards is what T steps leave (the caller advances pos by T).  With i = pos / chunk, r = pos % chunk the tokens
 * fall into segments that never cross a chunk boundary -- min(T, chunk - r) rows of the open chunk i, whole chunks, a tail --
 * and for a segment in chunk c with rows Q, K, V:
 *   O   = scale (Q (P_c + mix[c][c] Cur_before) + mix[c][c] tril(Q K^T) V)        tril over the segment's own rows
 *   Cur = Cur_before + K^T V ;  chunk full: S[c] = Cur, Cur = 0, P_{c+1} = sum_{j<=c} mix[c+1][j] S[j]  (0 when c + 1 == cap_chunks)
 * Cur_before is the state's Cur for the first segment and zero afterwards, P_c the state's P for the first segment.  Exact
 * fp32 products with fp32 accumulation (never the stored 11-bit summaries), no atomics.  `y`, `gate`, `norm_w`, `out`: as
 * mhla_causal_step, the epilogue applied to the fp32 rows before their one rounding.  An empty state (pos = 0, P = Cur = 0)
 * makes it a prefill.  Rows of S beyond the finished chunks are neither read nor written.
 * Workspace (mhla_causal_extend_ws_bytes, pure host arithmetic, independent of dtype): one fp32 [K][V] tile per (b, h) and
 * chunk touched after the first -- (pos + T - 1) / chunk - pos / chunk of them -- plus the T fp32 rows [V] per (b, h) the
 * epilogue reads.  MHLA_EINVAL before any launch, the message naming the value: pos + T needs more chunks than cap_chunks;
 * ldmix does not cover the last row of mix read (row (pos + T) / chunk when a chunk closes and the state is not full then,
 * else row (pos + T - 1) / chunk); ws_bytes short.  T <= 65535 per call; K, V multiples of 4, chunk 64, B*H <= 65535. */
size_t mhla_causal_extend_ws_bytes(int B, int T, int H, int K, int V, int64_t pos, int dtype);
int mhla_causal_extend(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                       float* Cur, int64_t pos, int T, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                       mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int K, int V, int chunk, float scale, int dtype,
                       void* stream);

/* mhla_causal_extend_ragged: mhla_causal_extend for a batch whose sequence b is at a position of its own, pos_dev[b], and takes a
 * token count of its own, ntok_dev[b] in 0 .. T (added without a change of any existing signature or behaviour: MHLA_ABI_VERSION
 * stays 9).  pos_dev, ntok_dev: device int32 [B].  q, k, v, gate, out, y are padded to T rows per sequence: the tokens of sequence b
 * are rows [0, ntok_dev[b]), or [T - ntok_dev[b], T) with `left_padded`.  Sequence b behaves as in mhla_causal_extend alone in a
 * batch of one at pos = pos_dev[b], T = ntok_dev[b] (the same tiles and order of every sum: the same bits; one token: the bits of
 * mhla_causal_step for a batch of one); ntok_dev[b] = 0 leaves its state untouched.  Rows outside a sequence's window are never read
 * into anything (q, k, v, gate) and are WRITTEN as zeros (out, y): the caller clears nothing.  At most six launches whatever B,
 * the counts and the positions; the last adds ntok_dev[b] to pos_dev[b] in stream order (the earlier launches address by
 * pos_dev, the last does not), so the array is the caller's to keep in step with, not to advance.
 * The library cannot read device memory to validate, hence host values that vouch for the arrays:
 *   T           the padded width, 1 .. 65535
 *   max_end     the largest pos_dev[b] + ntok_dev[b] over the sequences with ntok_dev[b] > 0 (0: none has): takes the place of
 *               pos + T in the capacity and ldmix checks of mhla_causal_extend
 *   max_later   the largest number of chunks a sequence touches after its first, (pos + n - 1) / chunk - pos / chunk: sizes the grid
 *               of the later segments and the workspace stride per (b, h)
 *   any_close   non-zero when at least one sequence closes a chunk (pos % chunk + n >= chunk); zero: the three launches that form
 *               later chunks and prefix mixes are not made.  Restriction, as mhla_causal_step_ragged: with any_close row
 *               max_end / chunk of mix must be covered by ldmix unless max_end fills the state, whichever sequence closes
 *   left_padded non-zero: windows are right-aligned, [T - n, T)
 * pos_dev / ntok_dev must hold what these were computed from; arrays that disagree are the caller's error.  As a defence only, no
 * content of the arrays addresses outside S, the matrix, the workspace or the token tensors: a sequence with pos < 0, n > T,
 * pos + n > max_end, more later chunks than max_later, or a closing chunk without any_close is SKIPPED -- its state and position
 * stay untouched and its rows are zeros.
 * Workspace (mhla_causal_extend_ragged_ws_bytes, pure host arithmetic, independent of dtype), in 4-byte words, each term rounded
 * up to a multiple of 4:  B H max_later K V  +  B H T V  +  B.  MHLA_EINVAL before any launch, the message naming the value:
 * T outside 1 .. 65535; max_end beyond 64 cap_chunks; max_later beyond what T tokens can touch, or given without any_close; ldmix
 * short of the row above; ws_bytes short or ws misaligned; pos_dev / ntok_dev null or misaligned.  Others as mhla_causal_extend. */
size_t mhla_causal_extend_ragged_ws_bytes(int B, int T, int H, int K, int V, int max_later, int dtype);
int mhla_causal_extend_ragged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                              float* Cur, int32_t* pos_dev, const int32_t* ntok_dev, int T, int64_t max_end, int max_later,
                              int any_close, int left_padded, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                              mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int K, int V, int chunk, float scale, int dtype,
                              void* stream);

/* mhla_causal_verify_ragged: the rows of mhla_causal_extend_ragged WITHOUT committing a token -- a draft to verify (added without a
 * change of any existing signature or behaviour: MHLA_ABI_VERSION stays 9).  Arguments, workspace
 * (mhla_causal_extend_ragged_ws_bytes), checks, the six launches, the tiles and the order of every sum are those of
 * mhla_causal_extend_ragged, and out / y hold the same bits; pos_dev is const.  After the call P, Cur, pos_dev and the FINISHED rows of
 * S -- S[b][h][0 .. pos_dev[b] / chunk) -- hold their previous bits: the state still describes pos_dev[b] tokens, and any call that
 * takes such a state gives what it would have given without the verify.  Rows pos_dev[b] / chunk .. of S are UNSPECIFIED afterwards:
 * the chain scribbles the draft's K^T V sums on them (the prefix mixes of the draft's later chunks are formed from them).  That is
 * within the state's contract -- rows of S beyond the finished chunks are neither read nor relied on by any call before a later
 * call finishes them, which overwrites them -- so undoing a draft needs no copy of S. */
int mhla_causal_verify_ragged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                              float* Cur, const int32_t* pos_dev, const int32_t* ntok_dev, int T, int64_t max_end, int max_later,
                              int any_close, int left_padded, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                              mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int K, int V, int chunk, float scale, int dtype,
                              void* stream);

/* mhla_causal_commit_ragged: advance a ragged state by the first accept_dev[b] tokens of sequence b's draft window, no rows computed
 * (added without a change of any existing signature or behaviour: MHLA_ABI_VERSION stays 9).  k, v, ntok_dev, T and left_padded
 * are those of the verify: the window of sequence b is placed by ntok_dev[b] -- rows [0, ntok_dev[b]), or [T - ntok_dev[b], T) with
 * `left_padded` -- and its first min(accept_dev[b], ntok_dev[b]) rows are taken; accept_dev: device int32 [B].  The state afterwards,
 * pos_dev included, is bit for bit the one mhla_causal_extend_ragged leaves with those rows as the sequence's tokens (the same
 * tiles and order of every sum; one accepted token: the step's rank-1 fmaf); accept_dev[b] = 0 leaves the sequence untouched.
 * At most four launches whatever B, the counts and the positions, none of which touches q, out, y or gate: the first segment's
 * K^T V, then -- only with any_close -- the later segments' and the prefix mix of the chunk open afterwards, then pos_dev[b] +=
 * the accepted count in stream order (the earlier launches address by pos_dev, the last does not).
 * max_end, max_later and any_close vouch for the ACCEPTED counts -- the values of mhla_causal_extend_ragged computed from pos_dev and
 * min(accept_dev, ntok_dev) -- with the same restriction on ldmix and the same defence: a sequence outside what they vouch for is
 * skipped, state and position untouched.  Workspace (mhla_causal_commit_ragged_ws_bytes, pure host arithmetic): B 4-byte words
 * rounded up to a multiple of 4.  MHLA_EINVAL before any launch: what mhla_causal_extend_ragged checks of T, the views k and v, the
 * state, the three device arrays, the host values, ldmix and the workspace. */
size_t mhla_causal_commit_ragged_ws_bytes(int B, int dtype);
int mhla_causal_commit_ragged(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                              int32_t* pos_dev, const int32_t* ntok_dev, const int32_t* accept_dev, int T, int64_t max_end,
                              int max_later, int any_close, int left_padded, void* ws, size_t ws_bytes, int B, int H, int K, int V,
                              int chunk, int dtype, void* stream);

/* Grouped-query heads (added without a change of any existing signature or behaviour: MHLA_ABI_VERSION stays 9).  S, P and Cur are
 * functions of k and v alone, so with Hkv k/v heads serving H = G Hkv query heads (query head h uses k/v head h / G) the G heads of
 * a group share one state.  The four calls below are their namesakes with one more integer, `Hkv`, after `H`: q, gate, out, y have H
 * heads; k, v have Hkv heads; S is [B][Hkv][cap_chunks][K][V], P and Cur [B][Hkv][K][V].  Rows, state and pos_dev afterwards are bit for
 * bit those of the namesake on k, v repeated G times per head with a state of H heads (every head of a group then holding the same
 * state): each sum has the same terms in the same order -- the K split of the step is chosen from the query head count for that
 * reason -- while P and Cur are read, and Cur written, once per k/v head: 1 / G of the state, of the per-token traffic and of the
 * chunk-boundary re-mix.  Hkv = H is the namesake itself (the same launches).  mhla_causal_state_init, mhla_causal_varlen_state_init
 * and mhla_causal_commit_ragged touch no q: they serve a grouped state as they are, given the un-repeated k, v and H = Hkv.
 * Checks, before any launch: MHLA_EINVAL for Hkv < 1 or H % Hkv != 0, MHLA_ENOTSUP for H / Hkv > 8; everything else as the namesake
 * (B*H <= 65535 counts query heads).  Workspace of the steps: mhla_causal_step_ws_bytes(B, H, ...), the query head count; of the extend
 * and the verify (mhla_causal_extend_ragged_gqa_ws_bytes), in 4-byte words, each term rounded up to a multiple of 4:
 * B Hkv max_later K V  +  B H T V  +  B. */
int mhla_causal_step_ragged_gqa(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                                float* Cur, int32_t* pos_dev, int64_t max_pos, int any_boundary, mhla_mview out, mhla_view gate,
                                const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K,
                                int V, int chunk, float scale, int dtype, void* stream);
int mhla_causal_step_dev_gqa(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                             float* Cur, int32_t* pos_dev, int32_t* full_dev, const void* rope_cos, const void* rope_sin, int64_t ld_tab,
                             int64_t tab_rows, int feature_map, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                             mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk, float scale,
                             int dtype, void* stream);
size_t mhla_causal_extend_ragged_gqa_ws_bytes(int B, int T, int H, int Hkv, int K, int V, int max_later, int dtype);
int mhla_causal_extend_ragged_gqa(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                                  float* Cur, int32_t* pos_dev, const int32_t* ntok_dev, int T, int64_t max_end, int max_later,
                                  int any_close, int left_padded, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                                  mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk, float scale,
                                  int dtype, void* stream);
int mhla_causal_verify_ragged_gqa(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                                  float* Cur, const int32_t* pos_dev, const int32_t* ntok_dev, int T, int64_t max_end, int max_later,
                                  int any_close, int left_padded, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps,
                                  mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk, float scale,
                                  int dtype, void* stream);

/* Slotted calls: steps, extends and prefills on CHOSEN ROWS of a state pool (added without a change of any existing signature or
 * behaviour: MHLA_ABI_VERSION stays 9).  A pool is an ordinary ragged state with n_slots batch rows -- S [n_slots][Hkv][cap_chunks][K][V],
 * P and Cur [n_slots][Hkv][K][V], pos_dev (and full_dev) int32 [n_slots] -- that outlives the calls; a server keeps every request in its
 * row while the set of live requests changes from token to token, without concatenating or gathering states.  Each call below is its
 * namesake (mhla_causal_step_ragged, _step_dev, _extend_ragged, _verify_ragged, _commit_ragged, _varlen_state_init) with a map after
 * pos_dev: `slot_dev`, device int32 [B], and `n_slots`.  Call row b works on row slot_dev[b] of the pool: everything the call reads or
 * writes of the STATE -- S, P, Cur, pos_dev, full_dev -- is addressed by slot_dev[b]; everything that belongs to the CALL -- q, k, v,
 * gate, out, y, the workspace, ntok_dev, accept_dev -- stays addressed by b.  The calls that take q also take `Hkv` after `H`
 * (Hkv = H: the ungrouped call; otherwise as the *_gqa forms above), so there are no separate grouped twins; the commit and the
 * prefill touch no q and take the k/v head count as H, as their namesakes.
 * Row b gets, bit for bit, what the namesake gives that row on a compact state holding copies of the chosen rows in call order: the
 * same launches, tiles and order of every sum, the K split of the step chosen from the call's B H.  Rows of the pool the call does
 * not name keep every bit of S, P, Cur, pos_dev and full_dev.  The map is the caller's contract: entries are distinct -- DUPLICATES ARE
 * THE CALLER'S ERROR, rows that share a slot race on it.  An entry outside 0 .. n_slots - 1 (a caller's mark such as -1) never
 * addresses anything: that call row is INACTIVE, its rows of out / y are written as zeros (the frozen / skipped behaviour of the
 * namesake) and no state, position or flag is touched -- for mhla_causal_step_dev_slots a map rewritten in place between the
 * replays of a captured graph is how requests join and leave.  mhla_causal_varlen_state_init_slots writes sequence s of the pack into
 * row slot_dev[s]: the finished chunks of S, P and Cur of THOSE rows only (the namesake handed the pool would write P and Cur of every
 * row); seq_len_dev stays indexed by s, pos_dev of the pool is the caller's to set.
 * Checks, before any launch: slot_dev non-null and 4-byte aligned, n_slots > 0 (MHLA_EINVAL); then those of the namesake with B
 * (n_seqs) counting call rows -- B*H <= 65535 as before, n_slots is not bounded by the grid.  The host values that vouch for device
 * arrays (max_pos, any_boundary, max_end, max_later, any_close) are computed by the caller over the SELECTED rows.  Workspaces: the
 * namesakes' functions (mhla_causal_step_ws_bytes, mhla_causal_extend_ragged_gqa_ws_bytes, mhla_causal_commit_ragged_ws_bytes) with the
 * call's B -- they do not depend on the pool. */
int mhla_causal_step_slots(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                           int32_t* pos_dev, const int32_t* slot_dev, int n_slots, int64_t max_pos, int any_boundary, mhla_mview out,
                           mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv,
                           int K, int V, int chunk, float scale, int dtype, void* stream);
int mhla_causal_step_dev_slots(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                               float* Cur, int32_t* pos_dev, const int32_t* slot_dev, int n_slots, int32_t* full_dev, const void* rope_cos,
                               const void* rope_sin, int64_t ld_tab, int64_t tab_rows, int feature_map, mhla_mview out, mhla_view gate,
                               const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K,
                               int V, int chunk, float scale, int dtype, void* stream);
int mhla_causal_extend_slots(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                             float* Cur, int32_t* pos_dev, const int32_t* slot_dev, int n_slots, const int32_t* ntok_dev, int T,
                             int64_t max_end, int max_later, int any_close, int left_padded, mhla_mview out, mhla_view gate,
                             const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V,
                             int chunk, float scale, int dtype, void* stream);
int mhla_causal_verify_slots(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P,
                             float* Cur, const int32_t* pos_dev, const int32_t* slot_dev, int n_slots, const int32_t* ntok_dev, int T,
                             int64_t max_end, int max_later, int any_close, int left_padded, mhla_mview out, mhla_view gate,
                             const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V,
                             int chunk, float scale, int dtype, void* stream);
int mhla_causal_commit_slots(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                             int32_t* pos_dev, const int32_t* slot_dev, int n_slots, const int32_t* ntok_dev, const int32_t* accept_dev, int T,
                             int64_t max_end, int max_later, int any_close, int left_padded, void* ws, size_t ws_bytes, int B, int H, int K,
                             int V, int chunk, int dtype, void* stream);
int mhla_causal_varlen_state_init_slots(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int cap_chunks, float* P, float* Cur,
                                        int n_seqs, const int32_t* seq_len_dev, const int32_t* slot_dev, int n_slots, int max_len, int T, int H,
                                        int K, int V, int chunk, int n_chunks, const int32_t* chunk_tab_dev, const int32_t* chunk_dst_dev,
                                        int dtype, void* stream);

/* Paged calls: the slotted calls above on a pool whose FINISHED CHUNKS ARE PAGES (added without a change of any existing signature or
 * behaviour: MHLA_ABI_VERSION stays 9).  A dense pool reserves cap_chunks chunks of S per slot whatever the request's length; a paged
 * pool keeps S as `pages`, fp32 [n_pages][Hkv][K][V], 16-byte aligned -- one page holds one chunk of one sequence, all k/v heads --
 * and `table_dev`, device int32 [n_slots][cap_chunks], 4-byte aligned: chunk j of state row sb, head h lives at
 * pages + ((int64)table_dev[sb * cap_chunks + j] * Hkv + h) * K * V.  An entry outside 0 .. n_pages - 1 means NO PAGE.  A finished
 * chunk is never written again (the open chunk lives in Cur, its summary reaches S only when the chunk closes, and a verify writes
 * only chunks at and beyond pos / 64), so rows may name the same page for a shared prefix: pages are the caller's to count and free.
 * Each call is its *_slots namesake with `float* S` replaced by (pages, n_pages, table_dev); P, Cur, pos_dev, full_dev and the slot
 * map keep their meaning, cap_chunks is the table's row length and remains the bound on positions.  Row b gets, bit for bit, what
 * the namesake gives on the dense pool whose S[sb][h][j] holds the page's tile: the same launches, tiles, K split and order of
 * every sum -- only the address of a chunk differs.
 * Host-positioned calls (step, extend, verify, commit, varlen_state_init): the caller has given a page to every chunk that holds a
 * token of the row afterwards, chunks 0 .. ceil(n_after / 64) - 1.  Defence only: no address is ever formed from an entry that
 * is no page -- a write there is dropped (a step on a boundary then leaves that row's S, P and Cur as they are), a read there
 * contributes no term.
 * mhla_causal_step_dev_paged: row sb is LIVE iff 0 <= pos < 64 cap_chunks AND table_dev[sb][pos / 64] names a page; otherwise it
 * takes the frozen branch of mhla_causal_step_dev unchanged (nothing of the pool touched, the row zeros, full_dev[sb] = 1).  Step,
 * roll and finish each derive that from pos and the table alone; the boundary roll writes S[pos / 64] to the page that made the
 * row live.  Like the slot map, the table may be rewritten in place between the replays of a captured graph.
 * Checks, before any launch: pages non-null and 16-byte aligned, table_dev non-null and 4-byte aligned, n_pages > 0 (MHLA_EINVAL);
 * then those of the namesake.  Workspaces: the namesakes' functions. */
int mhla_causal_step_paged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages,
                           const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev, int n_slots,
                           int64_t max_pos, int any_boundary, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y,
                           void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk, float scale, int dtype, void* stream);
int mhla_causal_step_dev_paged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages,
                               const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev,
                               int n_slots, int32_t* full_dev, const void* rope_cos, const void* rope_sin, int64_t ld_tab, int64_t tab_rows,
                               int feature_map, mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws,
                               size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk, float scale, int dtype, void* stream);
int mhla_causal_extend_paged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages,
                             const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev,
                             int n_slots, const int32_t* ntok_dev, int T, int64_t max_end, int max_later, int any_close, int left_padded,
                             mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B,
                             int H, int Hkv, int K, int V, int chunk, float scale, int dtype, void* stream);
int mhla_causal_verify_paged(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages,
                             const int32_t* table_dev, int cap_chunks, float* P, float* Cur, const int32_t* pos_dev, const int32_t* slot_dev,
                             int n_slots, const int32_t* ntok_dev, int T, int64_t max_end, int max_later, int any_close, int left_padded,
                             mhla_mview out, mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B,
                             int H, int Hkv, int K, int V, int chunk, float scale, int dtype, void* stream);
int mhla_causal_commit_paged(mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages, const int32_t* table_dev,
                             int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev, int n_slots,
                             const int32_t* ntok_dev, const int32_t* accept_dev, int T, int64_t max_end, int max_later, int any_close,
                             int left_padded, void* ws, size_t ws_bytes, int B, int H, int K, int V, int chunk, int dtype, void* stream);
int mhla_causal_varlen_state_init_paged(mhla_view k, mhla_view v, const float* mix, int ldmix, float* pages, int n_pages,
                                        const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int n_seqs, const int32_t* seq_len_dev,
                                        const int32_t* slot_dev, int n_slots, int max_len, int T, int H, int K, int V, int chunk, int n_chunks,
                                        const int32_t* chunk_tab_dev, const int32_t* chunk_dst_dev, int dtype, void* stream);

/* Packed new tokens: mhla_causal_extend_ragged, mhla_causal_verify_ragged and mhla_causal_commit_ragged on tokens that are NOT padded
 * (added without a change of any existing signature or behaviour: MHLA_ABI_VERSION stays 9).  The new tokens of all B sequences are
 * ONE run of n_tokens rows -- q, k, v, gate, out, y are [1][n_tokens][heads][K / V]; their batch stride sb is not used: pass 0 -- and
 * sequence b's tokens are rows [off_dev[b], off_dev[b + 1]): off_dev is device int32 [B + 1], off_dev[0] = 0, non-decreasing,
 * off_dev[B] = n_tokens; a sequence with no token (equal neighbours) keeps every bit of its state.  The layout of a scheduler step
 * of continuous batching (and of mhla_causal_varlen_state_init): no padding row is allocated, staged or written.
 * One entry point serves every kind of state, where the padded calls have one per kind:
 *   Hkv          the k/v heads of k, v and the state; Hkv = H: ungrouped (the commit touches no q and takes Hkv alone)
 *   slot_dev     device int32 [B], or NULL (n_slots unused): call row b works on row b of the state.  Non-null: on row slot_dev[b] of a
 *                pool of n_slots rows, as the *_slots calls
 *   table_dev    device int32 [n_slots][cap_chunks], or NULL (n_pages unused): `S` is the dense array [rows][Hkv][cap_chunks][K][V].
 *                Non-null: `S` is the pool of fp32 pages [n_pages][Hkv][K][V], as `pages` of the *_paged calls
 * Each runs its ragged namesake's chain -- the same launches (at most six; the commit at most four), tiles, K split and order of
 * every sum, no atomics -- with w = off_dev[b + 1] - off_dev[b] where that reads ntok_dev[b] and off_dev[b] as the window's first
 * row: sequence b's rows, its finished chunks, P, Cur and pos_dev[b] are BIT FOR BIT those of the padded call with ntok_dev[b] = w
 * (one token: the bits of mhla_causal_step for a batch of one).  The fp32 rows are staged [H][n_tokens][V] and the last launch runs
 * over (H, n_tokens): each workgroup finds its row's sequence by a binary search over off_dev, and the one of head 0 on a
 * sequence's first row adds the sequence's tokens to pos_dev (the verify: does not).  accept_dev (commit): device int32 [B], the
 * first min(accept_dev[b], w) rows of sequence b's window are taken.
 * Host values that vouch for the arrays, as mhla_causal_extend_ragged's:
 *   n_tokens     the rows of the pack, 1 .. 65535 (the last launch puts them on a grid dimension); takes T's place in every check
 *   max_end, max_later, any_close   computed from pos_dev and the differences of off_dev (the commit: from the accepted counts)
 * As a defence only, no content of the arrays addresses outside S, the matrix, the workspace or the token tensors: a sequence
 * whose offsets decrease, whose window leaves [0, n_tokens), or which fails a test of mhla_causal_extend_ragged's defence is
 * SKIPPED -- state and position untouched, its rows zeros -- and a row that belongs to no sequence is written as zeros.
 * Workspace of extend and verify (mhla_causal_extend_packed_ws_bytes, pure host arithmetic, independent of dtype), in 4-byte words,
 * each term rounded up to a multiple of 4:  B Hkv max_later K V  +  H n_tokens V  +  B; of the commit:
 * mhla_causal_commit_ragged_ws_bytes(B).  MHLA_EINVAL before any launch, the message naming the value: off_dev null or misaligned;
 * table_dev given with S misaligned or n_pages <= 0; slot_dev misaligned or given with n_slots <= 0; n_tokens outside 1 .. 65535;
 * then what the ragged namesake checks (max_end, max_later, any_close, ldmix, the views, the state, the workspace, Hkv). */
size_t mhla_causal_extend_packed_ws_bytes(int B, int n_tokens, int H, int Hkv, int K, int V, int max_later, int dtype);
int mhla_causal_extend_packed(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int n_pages,
                              const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev,
                              int n_slots, const int32_t* off_dev, int n_tokens, int64_t max_end, int max_later, int any_close, mhla_mview out,
                              mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H,
                              int Hkv, int K, int V, int chunk, float scale, int dtype, void* stream);
int mhla_causal_verify_packed(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int n_pages,
                              const int32_t* table_dev, int cap_chunks, float* P, float* Cur, const int32_t* pos_dev, const int32_t* slot_dev,
                              int n_slots, const int32_t* off_dev, int n_tokens, int64_t max_end, int max_later, int any_close, mhla_mview out,
                              mhla_view gate, const float* norm_w, float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H,
                              int Hkv, int K, int V, int chunk, float scale, int dtype, void* stream);
int mhla_causal_commit_packed(mhla_view k, mhla_view v, const float* mix, int ldmix, float* S, int n_pages, const int32_t* table_dev,
                              int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev, int n_slots,
                              const int32_t* off_dev, const int32_t* accept_dev, int n_tokens, int64_t max_end, int max_later, int any_close,
                              void* ws, size_t ws_bytes, int B, int Hkv, int K, int V, int chunk, int dtype, void* stream);

/* h16 pages: the paged step, device-positioned step and pack prefill on a pool whose pages take 2 bytes an element (added without a
 * change of any existing signature or behaviour: MHLA_ABI_VERSION stays 9).  A page is a payload, `pages_h16` _Float16
 * [n_pages][Hkv][K][V], 16-byte aligned, and apart from it multipliers, `page_mult` float [n_pages][Hkv][K V / 64], 4-byte aligned:
 * group g of a head is elements [64 g, 64 g + 64) of the head's flattened [K][V] chunk, its multiplier m the power of two
 * 2^(floor(log2 max|x|) - 14) (exponent field clamped to 1 .. 240; the largest magnitude of the group by its bit pattern), its
 * payload (_Float16)(x / m) rounded to nearest even; an element decodes as (float)payload * m, exact in fp32: 11 significand bits
 * relative to the group's largest element, the precision of the forward's default chunk summaries.  Requires K V % 64 == 0.
 * P, Cur, pos_dev, full_dev, the slot map and the table are those of the fp32 paged calls.  The contract:
 *   pages    Cur of an open chunk depends on no page, so a chunk finishes with the fp32 values of the fp32 pool, bit for bit, and
 *            the page written is the encoding of exactly those values.  A finished chunk is written, and so rounded, once.
 *   readers  every prefix mix is the sum of the fp32 calls -- ascending j, fmaf -- over DECODED pages, the chunk a boundary just
 *            committed included: P is a function of the pages alone, and a slot filled by the pack prefill holds the bits (payload,
 *            multipliers, P, Cur) of one that reached the same tokens step by step.
 *   no page  an entry outside 0 .. n_pages - 1 forms no address, of the multipliers as of the payload; pages, multipliers and slots
 *            a call does not name keep every bit.
 * Each call is its *_paged namesake with `float* pages` replaced by (pages_h16, page_mult).  The pack prefill stages the chunks'
 * fp32 K^T V in a workspace before it encodes them: mhla_causal_varlen_state_init_paged_h16_ws_bytes gives the size that takes the
 * whole pack in one pass (4 n_chunks H K V); any 16-byte aligned workspace that holds one chunk (4 H K V bytes) will do, the call
 * then works through the chunk list in slices (MHLA_EINVAL below that).  Extend, verify and commit have no h16 form.
 * Checks, before any launch: pages_h16 and page_mult non-null, 16-byte and 4-byte aligned, K V % 64 == 0 (MHLA_EINVAL); then those
 * of the namesake. */
int mhla_causal_step_paged_h16(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, void* pages_h16, float* page_mult, int n_pages,
                               const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int32_t* pos_dev, const int32_t* slot_dev,
                               int n_slots, int64_t max_pos, int any_boundary, mhla_mview out, mhla_view gate, const float* norm_w,
                               float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk,
                               float scale, int dtype, void* stream);
int mhla_causal_step_dev_paged_h16(mhla_view q, mhla_view k, mhla_view v, const float* mix, int ldmix, void* pages_h16, float* page_mult,
                                   int n_pages, const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int32_t* pos_dev,
                                   const int32_t* slot_dev, int n_slots, int32_t* full_dev, const void* rope_cos, const void* rope_sin,
                                   int64_t ld_tab, int64_t tab_rows, int feature_map, mhla_mview out, mhla_view gate, const float* norm_w,
                                   float norm_eps, mhla_mview y, void* ws, size_t ws_bytes, int B, int H, int Hkv, int K, int V, int chunk,
                                   float scale, int dtype, void* stream);
size_t mhla_causal_varlen_state_init_paged_h16_ws_bytes(int n_chunks, int H, int K, int V, int dtype);
int mhla_causal_varlen_state_init_paged_h16(mhla_view k, mhla_view v, const float* mix, int ldmix, void* pages_h16, float* page_mult, int n_pages,
                                            const int32_t* table_dev, int cap_chunks, float* P, float* Cur, int n_seqs,
                                            const int32_t* seq_len_dev, const int32_t* slot_dev, int n_slots, int max_len, int T, int H, int K,
                                            int V, int chunk, int n_chunks, const int32_t* chunk_tab_dev, const int32_t* chunk_dst_dev, void* ws,
                                            size_t ws_bytes, int dtype, void* stream);

/* Swap: the state of chosen slots of a paged pool OUT into one contiguous buffer (the blob) and back IN -- into other slots, other
 * pages or another pool of the same Hkv, K, V and page format (added without a change of any existing signature or behaviour:
 * MHLA_ABI_VERSION stays 9).  A finished page is immutable, so the state of a sequence -- its finished pages, P, Cur, pos, full --
 * goes out and comes back with every bit intact: no arithmetic touches an element, an h16 page travels as payload and multipliers and
 * is never decoded.  One entry point per direction serves both page formats: page_mult NULL means fp32 pages.
 * The blob is a run of ITEMS, each starting on a 16-byte boundary, every item of a kind the same size:
 *   n_seqs sequence items   P [Hkv][K][V] fp32 | Cur [Hkv][K][V] fp32 | pos, full as two int32, zeros up to 16 bytes
 *   n_pages page items      fp32 pages: [Hkv][K][V] fp32;  h16 pages: _Float16 [Hkv][K][V] | float [Hkv][K V / 64] | zeros up to 16 bytes
 * so items [i0, i1) are one contiguous byte range, and mhla_causal_swap_ws_bytes (pure host arithmetic; page_format 0: fp32, 1: h16;
 * 0 for sizes it does not take) gives the size of a blob -- of one item with (1, 0) and (0, 1).
 *   items_dev      device int32 [n_seqs + n_pages_moved]: the pool slot of every sequence item, then the pool page of every page item;
 *                  slots distinct, pages distinct.  Which page of the blob holds which chunk of which sequence is the caller's record
 *                  (and its page table's on the way in): a page that several sequences share is one item
 *   i0, i1         the call moves the items [i0, i1) of that list, blob_at is the device address where item i0 begins (16-byte
 *                  aligned): a blob that lives on the host is staged through a smaller device buffer in slices of whole items
 *   full_dev       may be NULL: out, the flag reads as 0; in, the blob's flag is dropped
 * mhla_causal_swap_out_paged reads the pool and writes every byte of its items, padding included; mhla_causal_swap_in_paged writes
 * the pages, P, Cur, pos_dev and full_dev of the slots and pages the list names and nothing else.  As a defence only, an entry
 * outside 0 .. n_slots - 1 (a sequence item) or 0 .. n_pages - 1 (a page item) forms no address and its item is skipped.
 * One launch, stream-ordered, no synchronisation.  MHLA_EINVAL before any launch: non-positive Hkv, K, V, n_pages or n_slots;
 * K V % 4 != 0; page_mult given with K V % 64 != 0; pages, P, Cur or blob_at null or not 16-byte aligned; page_mult (when given),
 * pos_dev, full_dev (when given) or items_dev null or not 4-byte aligned; negative n_seqs or n_pages_moved; a range outside
 * 0 <= i0 <= i1 <= n_seqs + n_pages_moved.  An empty range returns 0 without a launch. */
size_t mhla_causal_swap_ws_bytes(int n_seqs, int n_pages, int Hkv, int K, int V, int page_format);
int mhla_causal_swap_out_paged(const void* pages, const float* page_mult, int n_pages, const float* P, const float* Cur, const int32_t* pos_dev,
                               const int32_t* full_dev, int n_slots, const int32_t* items_dev, int n_seqs, int n_pages_moved, int i0, int i1,
                               void* blob_at, int Hkv, int K, int V, void* stream);
int mhla_causal_swap_in_paged(void* pages, float* page_mult, int n_pages, float* P, float* Cur, int32_t* pos_dev, int32_t* full_dev, int n_slots,
                              const int32_t* items_dev, int n_seqs, int n_pages_moved, int i0, int i1, const void* blob_at, int Hkv, int K, int V,
                              void* stream);

/* ---- prologue: q / k of the Wan host -------------------------------------- */

/*
 * y = relu(rmsnorm_C(x) * w) + eps  per token row over the whole channel dim C = H*D.
 * Replaces wan/mhla_utils.py:268-272 (norm_q / norm_k = WanRMSNorm(dim), wan/model.py:181-196,
 * then relu + eps) after the .float() at :308: x is the projection output in `dtype`, y fp32.
 * norm == 0 (qk_norm=False): y = relu(x) + eps.  w: fp32 [C] or NULL.  C % 8 == 0, C <= 4096.
 */
int mhla_qk_prologue(const void* x, int64_t ldx, const float* w, float* y, int64_t ldy,
                     int64_t rows, int C, int norm, float norm_eps, float eps,
                     int dtype, void* stream);
/* The same with a second output y_rope = rope(y) (wan/mhla_utils.py:314, rope_apply :127-156): consecutive channel pairs
 * of every head (head dim D, C = H*D) rotated by (rope_cos, rope_sin)[row % ntok][pair], tables fp32 [ntok][D/2].  The
 * training path of the Wan host: y feeds the normaliser, y_rope KV and the numerator.  y_rope NULL = mhla_qk_prologue. */
int mhla_qk_prologue_rope(const void* x, int64_t ldx, const float* w, float* y, int64_t ldy,
                          float* y_rope, int64_t ldyr,
                          const float* rope_cos, const float* rope_sin, int64_t ld_tab, int ntok, int D,
                          int64_t rows, int C, int norm, float norm_eps, float eps,
                          int dtype, void* stream);
/* Backward of the two above: dx (dtype of x) from dy and / or dy_rope (fp32, either may be NULL), and per-workgroup
 * partial weight gradients dw_partial fp32 [mhla_qk_prologue_dw_rows(rows)][C] (sum the rows; NULL when w is NULL).
 * C <= 2048. */
int64_t mhla_qk_prologue_dw_rows(int64_t rows);
int mhla_qk_prologue_bwd(const void* x, int64_t ldx, const float* w,
                         const float* dy, int64_t lddy, const float* dy_rope, int64_t lddyr,
                         const float* rope_cos, const float* rope_sin, int64_t ld_tab, int ntok, int D,
                         void* dx, int64_t lddx, float* dw_partial,
                         int64_t rows, int C, int norm, float norm_eps, int dtype, void* stream);

/*
 * q / k prologue of the fla layer in one pass: feature map (0 identity, 1 relu, 2 elu+1;
 * mhla_nlp/fla/layers/mhla.py:297-299) then the NeoX-style rotary embedding (:311,
 * mhla_nlp/fla/modules/rotary.py:45-135): y[i] = f(x[i]) c - f(x[i+K/2]) s, y[i+K/2] = f(x[i+K/2]) c + f(x[i]) s with
 * (c, s) = (cos, sin)[t_offset + t][i], fp32 math, tables [rows][K/2] in the activation dtype (row stride ld_tab).
 * backward != 0: x is the upstream gradient, x_saved the forward's input; y receives dL/dx.  x, y: [B, T, H, K] views.
 */
int mhla_featmap_rotary(mhla_view x, mhla_view x_saved, const void* cos, const void* sin, int64_t ld_tab,
                        int64_t t_offset, mhla_mview y, int B, int T, int H, int K,
                        int feature_map, int backward, int dtype, void* stream);

/*
 * The same prologue for the NEW tokens of a decode call, q and k in ONE launch, at positions read from the decode state (added
 * without a change of any existing signature or behaviour: MHLA_ABI_VERSION stays 9).  No host value depends on a position, so a
 * captured graph can replay the call; `pos_dev` is read and never written -- enqueue the call ahead of the chain that advances it.
 * Token layouts, as in the extend chain:
 *   padded (off_dev NULL): q, yq [B][T][H][K], k, yk [B][T][Hkv][K] views.  Sequence b takes w = ntok_dev[b] rows (ntok_dev NULL: all
 *     T), the window [0, w), or [T - w, T) with left_padded.
 *   packed (off_dev: device int32 [B + 1]; ntok_dev NULL, left_padded 0): the tokens are one run of T rows, the views' batch stride is
 *     unused, and row n belongs to the last b with off[b] <= n < off[b + 1]; empty sequences are skipped.
 * Position: a row with index r inside its sequence's window sits at p = pos_dev[sb] + r, sb = b, or slot_dev[b] with a slot map
 * (device int32 [B] of rows of a pool of n_slots; pos_dev is then the pool's [n_slots]; an entry outside 0 .. n_slots - 1 is an
 * INACTIVE row, as in the slotted decode calls).
 * Result: a row inside a window with 0 <= p < tab_rows holds the feature map followed by the rotary at table row p -- the fp32
 * arithmetic of mhla_featmap_rotary, rounded where that call rounds: bit for bit its output on table rows gathered at the same
 * positions.  Every other row -- outside every window, of an inactive slot entry, of a sequence whose offsets decrease or leave
 * [0, T) (or whose count leaves 0 .. T), or with p outside the tables -- is written as zeros in both yq and yk.  Nothing read from the
 * device arrays forms an address outside q, k, the tables or the outputs.
 * yq may be q and yk may be k (in place); strided views work, q and k as slices of one fused projection included.  cos, sin:
 * [tab_rows][K/2] in the tensor dtype, row stride ld_tab.  16-bit tensors move 16-byte pieces where every row of the views and the
 * tables starts on 16 bytes and K % 16 == 0, 8-byte pieces otherwise: the same bits.
 * MHLA_EINVAL before the launch: a non-positive size, K % 8 != 0, H % Hkv != 0, T outside 1 .. 65535, feature_map or dtype out of
 * range, an invalid view, tables null or misaligned, ld_tab < K / 2 or not a multiple of 4, tab_rows <= 0, pos_dev null, any device
 * array not 4-byte aligned, n_slots <= 0 with a slot map, off_dev together with ntok_dev or left_padded.
 */
int mhla_featmap_rotary_decode(mhla_view q, mhla_view k, const void* cos, const void* sin, int64_t ld_tab, int64_t tab_rows,
                               const int32_t* pos_dev, const int32_t* slot_dev, int n_slots,
                               const int32_t* ntok_dev, const int32_t* off_dev, int T, int left_padded,
                               mhla_mview yq, mhla_mview yk, int B, int H, int Hkv, int K, int feature_map, int dtype, void* stream);

/* ---- LePE: depthwise K x K convolution over V on the token layout --------- */

/*
 * y[b, n, c] = (bias[c]) + sum_taps w_taps[tap][c] * x[b, nbr(n, tap), c] (+ add[b, n, c]).
 * Replaces the NCHW round trip around nn.Conv2d(dim, dim, K, 1, K/2, groups=dim) at
 * mhla_dit/mhla/mhla.py:246-247 (+ the add at :271-273) and
 * mhla_image_classification/models/modules/attention/mhla.py:169 (K = 5).  Tokens are block-major:
 * n = m*S + s, block m = (py, px) on a pieces_len^2 grid, s = (by, bx) on a block_len^2 grid, pixel
 * (py*block_len + by, px*block_len + bx); zero padding at the image border.  x, add, y: [B, N, C] with batch /
 * token strides in elements (x may be the V slice of the fused QKV buffer).  w_taps: fp32 [K*K][C]
 * (the conv weight [C,1,K,K] transposed), bias: fp32 [C] or NULL, add: NULL or a tensor to add.
 * flip = 1 correlates with the flipped kernel: the gradient w.r.t. x when `x` is dout.
 */
int mhla_lepe2d(const void* x, int64_t x_sb, int64_t x_sn, const float* w_taps, const float* bias,
                const void* add, int64_t add_sb, int64_t add_sn,
                void* y, int64_t y_sb, int64_t y_sn,
                int B, int pieces_len, int block_len, int C, int K, int flip,
                int dtype, void* stream);
/* Weight and bias gradient: dwb fp32 [(K*K + 1)][C], rows 0..K*K-1 = dw_taps, row K*K = dbias;
 * overwritten, deterministic (fixed-order two-stage sum). */
size_t mhla_lepe2d_wgrad_ws_bytes(int C, int K);
int mhla_lepe2d_wgrad(const void* x, int64_t x_sb, int64_t x_sn, const void* dout, int64_t g_sb, int64_t g_sn,
                      float* dwb, void* ws, size_t ws_bytes,
                      int B, int pieces_len, int block_len, int C, int K, int dtype, void* stream);

/*
 * 3-D LePE of the Wan host: y = conv3d(x as video, w [C,1,3,3,3], bias, padding 1, groups = C) (+ add), replacing the
 * 'b (f h w) c -> b c f h w' round trip around nn.Conv3d at wan/mhla_utils.py:199-201, 349-352.  Tokens are in raster
 * order n = (f*H + h)*W + w.  w_taps: fp32 [27][C], tap = (df*3 + dh)*3 + dw; other arguments as mhla_lepe2d.
 */
int mhla_lepe3d(const void* x, int64_t x_sb, int64_t x_sn, const float* w_taps, const float* bias,
                const void* add, int64_t add_sb, int64_t add_sn,
                void* y, int64_t y_sb, int64_t y_sn,
                int B, int F, int H, int W, int C, int flip, int dtype, void* stream);
/* dwb fp32 [28][C]: rows 0..26 = dw_taps, row 27 = dbias; overwritten, deterministic. */
size_t mhla_lepe3d_wgrad_ws_bytes(int C);
int mhla_lepe3d_wgrad(const void* x, int64_t x_sb, int64_t x_sn, const void* dout, int64_t g_sb, int64_t g_sn,
                      float* dwb, void* ws, size_t ws_bytes,
                      int B, int F, int H, int W, int C, int dtype, void* stream);

/* ---- epilogue: per-head RMSNorm (x optional swish gate) ----------------- */

/*
 * y = x * rsqrt(mean_d(x^2) + eps) * w[d]  [ * g * sigmoid(g) ]   per (token, head).
 * Replaces FusedRMSNormGated (mhla_nlp/fla/modules/fused_norm_gate.py:77-99,
 * used at mhla_nlp/fla/layers/mhla.py:351-355) and Wan's per-head g_norm
 * [x SiLU gate] (mhla_videogen/diffusion/model/wan/mhla_utils.py:357-362).
 * x, g, y: [rows, D] with row strides (elements); g.ptr NULL => no gate.
 * rstd (fp32 [rows], may be NULL) is saved for the backward.
 */
int mhla_rmsnorm_gate_fwd(const void* x, int64_t ldx, const void* g, int64_t ldg,
                          const float* w, void* y, int64_t ldy, float* rstd,
                          int64_t rows, int D, float eps, int dtype, void* stream);

/* dx, dg (when gated) and a per-row-block partial of dw: dw_partial is fp32
 * [mhla_rmsnorm_gate_dw_rows(rows), D]; the caller sums it over dim 0. */
int64_t mhla_rmsnorm_gate_dw_rows(int64_t rows);
int mhla_rmsnorm_gate_bwd(const void* x, int64_t ldx, const void* g, int64_t ldg,
                          const float* w, const void* dy, int64_t lddy,
                          void* dx, int64_t lddx, void* dg, int64_t lddg,
                          float* dw_partial, int64_t rows, int D, float eps,
                          int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MHLA_HIP_H */
