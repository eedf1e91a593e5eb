"""The block-mix dispatch without a GPU: the description, workspace sizes and keeps_state of rows on each side of every dispatch boundary,
pinned to what the library answered BEFORE route, plan and description became one code path (capi_common.hpp bm_route / bm_plan), and the
argument checks the rope- and gate-taking entry points share.  tools/dispatch_table.py --sweep prints the whole grid these rows come from."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

# (option set to 0 / 1 for the row or None, B*H, M, S, D, dtype, split, flags, description | sizes): rows around 32|33, 64|65, 128|129, 192|193
# and 256|257 blocks for each summaries option and fp32; S = 8|16 and odd S; D = 96|104; D % 8 != 0; the small-sequence and fast-path
# routes with no_smalln / force_generic / a split pair; B*H = 2 against 128 (k_sp_mixh2); recut_kernels = 0 and fp32_summaries = 1
PINNED = [
    (None, 128, 32, 64, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes); fwd=k_sp_state k_sp_mixh<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixh<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=79691776 bwd_ws=167772176 keeps_state=1'),
    (None, 128, 32, 64, 64, 1, 0, 8,
     'family=bf16 fast path (fused mixing + token tiles); summaries=bf16 (single bf16 values, 8-block interleaved: reduced precision, opt-in); fwd=k_fs_state_fwd k_fs_wz<0> k_t16_out; bwd=k_fs_state<1> k_fs_dw k_t16_bwd | fwd_ws=79691776 bwd_ws=167772176 keeps_state=1'),
    (None, 128, 32, 64, 64, 1, 0, 32,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=p24 (24-bit floats: 16 significand bits, 3 bytes); fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=113246208 bwd_ws=234881040 keeps_state=1'),
    (None, 128, 32, 64, 64, 0, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=146800640 bwd_ws=301989904 keeps_state=1'),
    (None, 128, 33, 64, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes); fwd=k_sp_state k_sp_mixh<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixh<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=82182144 bwd_ws=173285392 keeps_state=1'),
    (None, 128, 33, 64, 64, 1, 0, 8,
     'family=bf16 fast path (fused mixing + token tiles); summaries=bf16 (single bf16 values, 8-block interleaved: reduced precision, opt-in); fwd=k_fs_state_fwd k_fs_wz<0> k_t16_out; bwd=k_fs_state<1> k_fs_dw k_t16_bwd | fwd_ws=82182144 bwd_ws=173285392 keeps_state=1'),
    (None, 128, 33, 64, 64, 1, 0, 32,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=p24 (24-bit floats: 16 significand bits, 3 bytes); fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=116785152 bwd_ws=242491408 keeps_state=1'),
    (None, 128, 33, 64, 64, 0, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=151388160 bwd_ws=311697424 keeps_state=1'),
    (None, 128, 64, 64, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes); fwd=k_sp_state k_sp_mixh<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixh<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=159383552 bwd_ws=352321552 keeps_state=1'),
    (None, 128, 64, 64, 64, 1, 0, 8,
     'family=bf16 fast path (fused mixing + token tiles); summaries=bf16 (single bf16 values, 8-block interleaved: reduced precision, opt-in); fwd=k_fs_state_fwd k_fs_wz<0> k_t16_out; bwd=k_fs_state<1> k_fs_dw k_t16_bwd | fwd_ws=159383552 bwd_ws=352321552 keeps_state=1'),
    (None, 128, 64, 64, 64, 1, 0, 32,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=p24 (24-bit floats: 16 significand bits, 3 bytes); fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=226492416 bwd_ws=486539280 keeps_state=1'),
    (None, 128, 64, 64, 64, 0, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=293601280 bwd_ws=620757008 keeps_state=1'),
    (None, 128, 65, 64, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes); fwd=k_sp_state k_sp_mixh<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixh<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=161873920 bwd_ws=358359056 keeps_state=1'),
    (None, 128, 65, 64, 64, 1, 0, 8,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=bf16 (single bf16 values: reduced precision, opt-in); fwd=k_sp_state k_sp_mixr<0> k_wz<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1> k_wz<1> k_sp_dwr<2> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=161873920 bwd_ws=358359056 keeps_state=1'),
    (None, 128, 65, 64, 64, 1, 0, 32,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=p24 (24-bit floats: 16 significand bits, 3 bytes); fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=230031360 bwd_ws=494673936 keeps_state=1'),
    (None, 128, 65, 64, 64, 0, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=298188800 bwd_ws=630988816 keeps_state=1'),
    (None, 128, 128, 64, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes); fwd=k_sp_state k_sp_mixh<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixh<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=318767104 bwd_ws=771751952 keeps_state=1'),
    (None, 128, 128, 64, 64, 1, 0, 8,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=bf16 (single bf16 values: reduced precision, opt-in); fwd=k_sp_state k_sp_mixr<0> k_wz<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1> k_wz<1> k_sp_dwr<2> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=318767104 bwd_ws=771751952 keeps_state=1'),
    (None, 128, 128, 64, 64, 1, 0, 32,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=p24 (24-bit floats: 16 significand bits, 3 bytes); fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=452984832 bwd_ws=1040187408 keeps_state=1'),
    (None, 128, 128, 64, 64, 0, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=587202560 bwd_ws=1308622864 keeps_state=1'),
    (None, 128, 129, 64, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes); fwd=k_sp_state k_sp_mixh2<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixh2<1> k_sp_dwr<3,h16> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=321257472 bwd_ws=778838032 keeps_state=1'),
    (None, 128, 129, 64, 64, 1, 0, 8,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=bf16 (single bf16 values: reduced precision, opt-in); fwd=k_sp_state k_sp_mixr<0> k_wz<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1> k_wz<1> k_sp_dwr<3> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=321257472 bwd_ws=778838032 keeps_state=1'),
    (None, 128, 129, 64, 64, 1, 0, 32,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1> k_sp_dw k_dw k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=727056384 bwd_ws=1455169552 keeps_state=1'),
    (None, 128, 129, 64, 64, 0, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1> k_sp_dw k_dw k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=591790080 bwd_ws=1319903248 keeps_state=1'),
    (None, 128, 192, 64, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes); fwd=k_sp_state k_sp_mixh2<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixh2<1> k_sp_dwr<3,h16> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=478150656 bwd_ws=1258291216 keeps_state=1'),
    (None, 128, 192, 64, 64, 1, 0, 8,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=bf16 (single bf16 values: reduced precision, opt-in); fwd=k_sp_state k_sp_mixr<0> k_wz<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1> k_wz<1> k_sp_dwr<3> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=478150656 bwd_ws=1258291216 keeps_state=1'),
    (None, 128, 192, 64, 64, 1, 0, 32,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1> k_sp_dw k_dw k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=1082130432 bwd_ws=2264924176 keeps_state=1'),
    (None, 128, 192, 64, 64, 0, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1> k_sp_dw k_dw k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=880803840 bwd_ws=2063597584 keeps_state=1'),
    (None, 128, 193, 64, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes); fwd=k_sp_state k_sp_mixh2<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixh2<1> k_sp_dwr<4,h16> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=480641024 bwd_ws=1266425872 keeps_state=1'),
    (None, 128, 193, 64, 64, 1, 0, 8,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=bf16 (single bf16 values: reduced precision, opt-in); fwd=k_sp_state k_sp_mixr_dma<0> k_wz<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr_dma<1> k_wz<1> k_sp_dwr<4> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=480641024 bwd_ws=1266425872 keeps_state=1'),
    (None, 128, 193, 64, 64, 1, 0, 32,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1> k_sp_dw k_dw k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=1087766528 bwd_ws=2278301712 keeps_state=1'),
    (None, 128, 193, 64, 64, 0, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1> k_sp_dw k_dw k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=885391360 bwd_ws=2075926544 keeps_state=1'),
    (None, 128, 256, 64, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes); fwd=k_sp_state k_sp_mixh2<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixh2<1> k_sp_dwr<4,h16> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=637534208 bwd_ws=1811939344 keeps_state=1'),
    (None, 128, 256, 64, 64, 1, 0, 8,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=bf16 (single bf16 values: reduced precision, opt-in); fwd=k_sp_state k_sp_mixr_dma<0> k_wz<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr_dma<1> k_wz<1> k_sp_dwr<4> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=637534208 bwd_ws=1811939344 keeps_state=1'),
    (None, 128, 256, 64, 64, 1, 0, 32,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1> k_sp_dw k_dw k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=1442840576 bwd_ws=3154116624 keeps_state=1'),
    (None, 128, 256, 64, 64, 0, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1> k_sp_dw k_dw k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=1174405120 bwd_ws=2885681168 keeps_state=1'),
    (None, 128, 257, 64, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mix<0> k_wz<0> k_sp_out; bwd=k_sp_state<1> k_sp_mix<1> k_wz<1> k_sp_dw k_dw k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=1448476672 bwd_ws=3168542736 keeps_state=1'),
    (None, 128, 257, 64, 64, 1, 0, 8,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=bf16 (single bf16 values: reduced precision, opt-in); fwd=k_sp_state k_sp_mix<0> k_wz<0> k_sp_out; bwd=k_sp_state<1> k_sp_mix<1> k_wz<1> k_sp_dw k_dw k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=640024576 bwd_ws=1821122576 keeps_state=1'),
    (None, 128, 257, 64, 64, 1, 0, 32,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mix<0> k_wz<0> k_sp_out; bwd=k_sp_state<1> k_sp_mix<1> k_wz<1> k_sp_dw k_dw k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=1448476672 bwd_ws=3168542736 keeps_state=1'),
    (None, 128, 257, 64, 64, 0, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mix<0> k_wz<0> k_sp_out; bwd=k_sp_state<1> k_sp_mix<1> k_wz<1> k_sp_dw k_dw k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=1178992640 bwd_ws=2899058704 keeps_state=1'),
    (None, 128, 64, 8, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=p24 (24-bit floats: 16 significand bits, 3 bytes); fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=222822400 bwd_ws=479199248 keeps_state=1'),
    (None, 128, 64, 16, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes); fwd=k_sp_state k_sp_mixh<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixh<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=156237824 bwd_ws=346030096 keeps_state=1'),
    (None, 128, 64, 21, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes); fwd=k_sp_state k_sp_mixh<0> k_wz<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixh<1,dw> k_wz<1> k_dw k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=156565504 bwd_ws=346685456 keeps_state=1'),
    (None, 128, 64, 21, 64, 0, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_wz<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_wz<1> k_dw k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=290783232 bwd_ws=615120912 keeps_state=1'),
    (None, 128, 256, 16, 64, 1, 0, 8,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=bf16 (single bf16 values: reduced precision, opt-in); fwd=k_s16_state<0> k_sp_mixr_dma<0> k_s16_out; bwd=k_s16_state<1> k_sp_mixr_dma<1> k_sp_dwr<4> k_dw_reduce k_s16_bwd_dq k_s16_bwd_dkv | fwd_ws=624951296 bwd_ws=1786773520 keeps_state=1'),
    (None, 128, 256, 21, 64, 1, 0, 8,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=bf16 (single bf16 values: reduced precision, opt-in); fwd=k_sp_state k_sp_mixr_dma<0> k_wz<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr_dma<1> k_wz<1> k_sp_dwr<4> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=626262016 bwd_ws=1789394960 keeps_state=1'),
    (None, 128, 16, 16, 64, 1, 0, 8,
     'family=small-sequence bf16 (attention form, one launch per direction); summaries=none (score tiles as single bf16: reduced precision); fwd=k_sn_fwd<4>; bwd=k_sn_bwd<4> k_sn_dw_reduce | fwd_ws=39059456 bwd_ws=80216080 keeps_state=0'),
    (None, 128, 64, 64, 96, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes); fwd=k_sp_state k_sp_mixh<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixh<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=428867584 bwd_ws=790626320 keeps_state=1'),
    (None, 128, 64, 64, 96, 2, 0, 32,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=p24 (24-bit floats: 16 significand bits, 3 bytes); fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=579862528 bwd_ws=1092616208 keeps_state=1'),
    (None, 128, 64, 64, 104, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=844365824 bwd_ws=1613234192 keeps_state=1'),
    (None, 128, 64, 64, 104, 2, 0, 32,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=844365824 bwd_ws=1613234192 keeps_state=1'),
    (None, 128, 64, 64, 128, 0, 1, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=p24 (24-bit floats: 16 significand bits, 3 bytes); fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=832569344 bwd_ws=1698693136 keeps_state=1'),
    (None, 128, 193, 64, 128, 0, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1> k_sp_dw k_dw k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=3320217600 bwd_ws=6945579024 keeps_state=1'),
    (None, 2, 16, 16, 36, 0, 0, 0,
     'family=generic (exact fp32 MFMA); summaries=fp32 words (dense rows); fwd=k_bm_state<0> k_mix<0,0> k_wz<0> k_bm_out; bwd=k_bm_state<0> k_mix<0,0> k_wz<0> k_bm_state<1> k_wz<1> k_mix<1,0> k_dw k_dw_reduce k_bm_bwd_tok | fwd_ws=340480 bwd_ws=1731600 keeps_state=0'),
    (None, 2, 64, 64, 36, 1, 0, 0,
     'family=generic (exact fp32 MFMA); summaries=fp32 words (dense rows); fwd=k_bm_state<0> k_mix<0,0> k_wz<0> k_bm_out; bwd=k_bm_state<0> k_mix<0,0> k_wz<0> k_bm_state<1> k_wz<1> k_mix<1,0> k_dw k_dw_reduce k_bm_bwd_tok | fwd_ws=2000896 bwd_ws=11833360 keeps_state=0'),
    (None, 2, 16, 16, 72, 1, 0, 8,
     'family=small-sequence bf16 (attention form, one launch per direction); summaries=none (score tiles as single bf16: reduced precision); fwd=k_sn_fwd<5>; bwd=k_sn_bwd<5> k_sn_dw_reduce | fwd_ws=750592 bwd_ws=2551824 keeps_state=0'),
    (None, 2, 256, 64, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes); fwd=k_sp_state k_sp_mixh<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixh<1> k_sp_dwr<4,h16> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=9961472 bwd_ws=28311568 keeps_state=1'),
    (None, 128, 2, 64, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=p24 (24-bit floats: 16 significand bits, 3 bytes); fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=7077888 bwd_ws=14188560 keeps_state=1'),
    (None, 128, 4, 64, 32, 2, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes); fwd=k_sp_state k_sp_mixh<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixh<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=3604480 bwd_ws=7340048 keeps_state=1'),
    (None, 2, 16, 16, 64, 1, 0, 0,
     'family=small-sequence bf16 (attention form, one launch per direction); summaries=none (score tiles in LDS as bf16 hi + lo pairs); fwd=k_sn_fwd<4,hl>; bwd=k_sn_bwd<4,hl> k_sn_dw_reduce | fwd_ws=610304 bwd_ws=2271248 keeps_state=0'),
    (None, 2, 16, 16, 64, 1, 0, 4,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes); fwd=k_sp_state k_sp_mixh<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixh<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=610304 bwd_ws=2271248 keeps_state=1'),
    (None, 2, 16, 16, 64, 1, 0, 2,
     'family=generic (exact fp32 MFMA); summaries=fp32 words (dense rows); fwd=k_bm_state<0> k_mix<0,0> k_wz<0> k_bm_out; bwd=k_bm_state<0> k_mix<0,0> k_wz<0> k_bm_state<1> k_wz<1> k_mix<1,0> k_dw k_dw_reduce k_bm_bwd_tok | fwd_ws=1126400 bwd_ws=3237904 keeps_state=0'),
    (None, 2, 16, 16, 72, 0, 0, 0,
     'family=small-sequence fp32 (attention form, one launch per direction); summaries=none (score tiles in LDS as bf16 hi + lo pairs); fwd=k_snf_fwd<5>; bwd=k_snf_bwd<5> k_sn_dw_reduce | fwd_ws=1414144 bwd_ws=3878928 keeps_state=0'),
    (None, 2, 16, 16, 72, 0, 1, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=1414144 bwd_ws=3878928 keeps_state=1'),
    (None, 2, 17, 16, 72, 0, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=1502592 bwd_ws=4191264 keeps_state=1'),
    (None, 2, 16, 16, 64, 1, 0, 12,
     'family=bf16 fast path (fused mixing + token tiles); summaries=bf16 (single bf16 values, 8-block interleaved: reduced precision, opt-in); fwd=k_fs_state_fwd k_fs_wz<0> k_t16_out; bwd=k_fs_state<1> k_fs_dw k_t16_bwd | fwd_ws=610304 bwd_ws=2271248 keeps_state=1'),
    (None, 2, 16, 16, 64, 2, 0, 8,
     'rc=-22 MHLA_FLAG_BF16_SUMMARIES (single-bf16 summaries) serves bf16 tensors only | fwd_ws=610304 bwd_ws=2271248 keeps_state=1'),
    ('recut_kernels', 128, 256, 64, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes); fwd=k_sp_state k_sp_mixh<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixh<1> k_sp_dwr<4,h16> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=637534208 bwd_ws=1811939344 keeps_state=1'),
    ('recut_kernels', 128, 192, 16, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=h16 (fp16 payload x row multiplier: 11 significand bits, 2 bytes); fwd=k_sp_state k_sp_mixh<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixh<1> k_sp_dwr<3,h16> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=468713472 bwd_ws=1239416848 keeps_state=1'),
    ('fp32_summaries', 128, 64, 64, 64, 1, 0, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1,dw> k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=360710144 bwd_ws=687865872 keeps_state=1'),
    ('fp32_summaries', 128, 192, 64, 128, 0, 1, 0,
     'family=split-operand (bf16 hi + lo MFMA operands); summaries=fp32 words; fwd=k_sp_state k_sp_mixr<0> k_sp_out; bwd=k_sp_state<1> k_sp_mixr<1> k_sp_dw k_dw k_dw_reduce k_sp_bwd_dq k_sp_bwd_dkv | fwd_ws=3303014400 bwd_ws=6908018704 keeps_state=1'),
]
OPTION_VALUE = {"recut_kernels": 0, "fp32_summaries": 1}


def test_dispatch_rows_are_pinned_on_each_side_of_every_boundary():
    from dispatch_table import sweep_line
    from mhla_amd import _lib
    lib = _lib.load()
    wrong = []
    for option, BH, M, S, D, dt, split, flags, want in PINNED:
        before = lib.mhla_set_option(option.encode(), OPTION_VALUE[option]) if option else None
        try:
            got = sweep_line(lib, 1, BH, M, S, D, dt, split, flags).split(" -> ", 1)[1]
        finally:
            if option:
                lib.mhla_set_option(option.encode(), before)
        if got != want:
            wrong.append((option, BH, M, S, D, dt, split, flags, got, want))
    assert not wrong, wrong


ROPE_MSG = b"rope tables: ld=%d must be >= D/2, a multiple of 4, and the tables 16-byte aligned"
GATE_MSG = b"gate: pointer must be 8-byte aligned, strides multiples of 4"
P = 1 << 20   # an aligned address that is never dereferenced: every check below fails before the first HIP call


def _entry_points(lib, _lib):
    """name -> (call(cos, sin, ld, gate), message for a missing table): D = 128, M = 4 blocks of 16 tokens, B = H = 1."""
    V = _lib.View
    ok = V(P, 128 * 16, 128, 128)
    dims = (1, 1, 4, 16, 128)
    return {
        "rope_fwd": (lambda c, s, ld, g: lib.mhla_blockmix_rope_fwd(ok, ok, ok, 1, P, 4, c, s, ld, ok, None, P, 1 << 30, *dims, _lib.F32, 1e-6, 0, None),
                     b"rope tables null"),
        "rope_bwd": (lambda c, s, ld, g: lib.mhla_blockmix_rope_bwd(ok, ok, ok, 1, P, 4, c, s, ld, ok, ok, ok, ok, ok, P, None, P, 1 << 30, None, *dims,
                                                                    _lib.F32, 1e-6, 0, None), b"rope tables null"),
        "wan_fwd": (lambda c, s, ld, g: lib.mhla_blockmix_wan_fwd(ok, ok, ok, 1, P, 4, c, s, ld, None, 1e-6, g, ok, _lib.F32, None, P, 1 << 30, *dims,
                                                                  _lib.F32, 1e-6, 0, None), b"rope_cos and rope_sin must be given together"),
        "wan_pro_fwd": (lambda c, s, ld, g: lib.mhla_blockmix_wan_pro_fwd(ok, ok, ok, None, None, None, None, 1, P, 4, c, s, ld, None, 1e-6, g, ok, _lib.F32,
                                                                          None, P, 1 << 30, *dims, _lib.BF16, 1e-6, 0, None),
                        b"rope_cos and rope_sin must be given together"),
    }


@pytest.mark.parametrize("entry", ["rope_fwd", "rope_bwd", "wan_fwd", "wan_pro_fwd"])
def test_rope_table_checks_are_shared_by_the_four_entry_points(entry):
    from mhla_amd import _lib
    lib = _lib.load()
    call, missing = _entry_points(lib, _lib)[entry]
    none = _lib.NULL_VIEW
    for cos, sin in ((None, P), (P, None)) + (((None, None),) if entry.startswith("rope") else ()):
        assert call(cos, sin, 64, none) == -22 and lib.mhla_last_error() == missing, (cos, sin, lib.mhla_last_error())
    for cos, sin, ld in ((P, P, 60), (P, P, 66), (P + 8, P, 64), (P, P + 4, 64)):   # ld < D / 2, ld % 4 != 0, a misaligned table
        assert call(cos, sin, ld, none) == -22 and lib.mhla_last_error() == ROPE_MSG % ld, (cos, sin, ld, lib.mhla_last_error())


def test_rope_fwd_refuses_16bit_tensors_on_h16_or_p24_summaries():
    """No rotary summary kernel is built for 16-bit tensors on h16 / p24 summaries: bf16 at D = 64 (h16) is refused while the arguments are
    checked; at D = 128 (fp32 words) the same call passes this check and fails the next one, the workspace size."""
    from mhla_amd import _lib
    lib = _lib.load()
    call = lambda D, ws_bytes: lib.mhla_blockmix_rope_fwd(*(_lib.View(P, D * 16, D, D),) * 3, 1, P, 16, P, P, D // 2, _lib.View(P, D * 16, D, D), None, P, ws_bytes,
                                                          1, 1, 16, 16, D, _lib.BF16, 1e-6, 0, None)
    assert call(64, 1 << 30) == -95, lib.mhla_last_error()   # MHLA_ENOTSUP
    assert lib.mhla_last_error() == (b"rotary forward on 16-bit tensors with h16 / p24 summaries is not built (M=16 S=16 D=64 dtype=1): use fp32 tensors, or "
                                     b"rotate on the host and call mhla_blockmix(q_rope, k_rope, v, W, q_den=q, k_den=k)")
    assert call(128, 16) == -22 and lib.mhla_last_error().startswith(b"workspace too small"), lib.mhla_last_error()


@pytest.mark.parametrize("entry", ["wan_fwd", "wan_pro_fwd"])
def test_gate_check_is_shared_by_the_two_entry_points(entry):
    from mhla_amd import _lib
    lib = _lib.load()
    call, _ = _entry_points(lib, _lib)[entry]
    V = _lib.View
    for gate in (V(P + 4, 128 * 16, 128, 128), V(P, 128 * 16, 130, 128)):   # a pointer off 8 bytes, a stride off 4 elements
        for cos, sin in ((None, None), (P, P)):
            assert call(cos, sin, 64, gate) == -22 and lib.mhla_last_error() == GATE_MSG, lib.mhla_last_error()
