// Block-mixing kernels for any head dim D <= 128 with D % 8 == 0 in any dtype (the Wan2.1 shape: fp32, D = 128, M = 150
// blocks of 210 tokens, wan/mhla_utils.py:331-341; DiT-XL/2: D = 72), computing on the bf16 MFMA with split operands.
// DT = ceil(D / 16) output tiles per side; LDS tiles are 64 or 128 columns wide with the columns >= D zero.
//
// An fp32 value x is carried as two bf16 numbers, hi = bf16(x) and lo = bf16(x - hi), which keep 16 mantissa bits;
// a product a b is evaluated as a_hi b_hi + a_hi b_lo + a_lo b_hi with fp32 accumulation (the dropped lo*lo term is
// below 2^-17 |a b|).  Three v_mfma_f32_16x16x32_bf16 do the work of eight v_mfma_f32_16x16x4_f32 at a sixteenth of the
// issue cycles each, and a bf16 operand fetch from LDS moves 8 reduction steps per lane instead of 1 -- the generic
// fp32-MFMA kernels are bound by exactly those two.  bf16 tensors have lo = 0 and skip the extra products.
// Workspace formats are the generic path's (blockmix.hpp): KV, G fp32 [bh][M][D][D]; ksum [bh][M][D]; z, 1/n [bh][M][S].
//
// This file is the table of contents: one header per kernel, each of which compiles on its own.
//   split_operands.hpp  what the kernels share: element and format helpers (row_read8, ld8, Raw4, relu8, split8, rope8, unrope4,
//                       p24_*), Geo, the mat_* layout of a staged D x D matrix, stage_mat_*, MatStage, sp_payop, pack8_16,
//                       store_tile_pair, view16
//   split_state.hpp     k_sp_state    : KV_j = K_j^T V_j, ksum_j, z_j (backward: dG_i, dn_i)      grid (M, bh)
//   split_mix.hpp       k_sp_mix      : G = W . KV  (or W^T .)                                    grid (D^2 / 128, ceil(M / 64), bh)
//   split_mixr.hpp      k_sp_mixr     : the same mixing with every block of a (b, h) resident in the workgroup (M <= 256)
//                       k_sp_mixr_dma : ... for 16-bit summaries and 192 < M <= 256, staged by LDS-DMA
//                       mixr_weights, mix_weights_each: the mixing matrix through LDS, for these two and for k_sp_mixh / k_sp_mixh2
//   split_out.hpp       k_sp_out      : O_i = (Q_i G_i) / n_i, computed transposed so that a lane owns 4 consecutive output features
//   split_dw.hpp        k_sp_dw       : dW[i][j] = sum_e dG_i[e] KV_j[e] on fp32 or bf16 summaries
//                       k_sp_dwt      : ... on 24-bit summaries
//   split_tok.hpp       k_sp_bwd_dq   : dQ_i = (dO_i / n_i) G_i^T (+ dz_i ksum_i^T); dksum_i; dQden_i
//                       k_sp_bwd_dkv  : dK_j = V_j dKV_j^T (+ dksum_j); dV_j = K_j dKV_j; dKden_j
// (h16 summaries are mixed by k_sp_mixh, mixh.hpp, and k_sp_mixh2, mixh2.hpp; blocks of 16 tokens have split16.hpp.)
// The order below is the order of definition the kernels were developed in; keep it.
#pragma once
#include "split_operands.hpp"
#include "split_state.hpp"
#include "split_mix.hpp"
#include "split_mixr.hpp"
#include "split_out.hpp"
#include "split_dw.hpp"
#include "split_tok.hpp"
