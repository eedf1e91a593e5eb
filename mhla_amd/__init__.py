"""mhla_amd -- the MHLA attention operator for AMD MI355X (gfx950 / CDNA4).

Hand-written HIP kernels behind a C ABI (include/mhla_hip.h, libmhla_hip.so), the autograd
operators over it (mhla_amd.ops) and drop-in attention modules for the DiT, timm-ViT, Wan2.1 and
flash-linear-attention hosts (mhla_amd.modules).  No CPU / eager fallback.
"""
from . import _lib
from .ops import (featmap_rotary, featmap_rotary_decode, lepe2d, lepe3d, mhla_dit_core, mhla_blockmix, mhla_blockmix_rope, mhla_blockmix_wan, mhla_blockmix_wan_pro, mhla_causal, mhla_causal_normgate, mhla_causal_prefill, mhla_causal_state, mhla_causal_step, mhla_causal_step_dev, mhla_causal_extend, mhla_causal_verify, mhla_causal_commit, CausalDraft, CausalState, CausalStateView, PagedCausalState, PagedStateView, PoolExhausted, SwappedSlots, CausalVarlenPlan, causal_varlen_plan, naive_chunk_simple_mhla_fixed, naive_recurrent_mhla, qk_prologue,
                  rmsnorm_gate, set_option, describe_dispatch, describe_causal_dispatch)
from .weights import block_distance_weights, block_index_2d, block_index_3d, causal_mixing_init

__all__ = ["mhla_blockmix", "mhla_blockmix_rope", "mhla_blockmix_wan", "mhla_blockmix_wan_pro", "qk_prologue", "lepe2d", "lepe3d", "featmap_rotary", "featmap_rotary_decode", "mhla_dit_core", "mhla_causal", "mhla_causal_normgate", "mhla_causal_prefill", "mhla_causal_state", "mhla_causal_step", "mhla_causal_step_dev", "mhla_causal_extend", "mhla_causal_verify", "mhla_causal_commit", "CausalDraft", "CausalState", "CausalVarlenPlan", "causal_varlen_plan", "naive_chunk_simple_mhla_fixed", "naive_recurrent_mhla", "rmsnorm_gate", "set_option", "describe_dispatch", "describe_causal_dispatch",
           "block_distance_weights", "block_index_2d", "block_index_3d", "causal_mixing_init", "_lib"]
__version__ = "0.1.0"
