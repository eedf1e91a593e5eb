// Grouped-query heads in the causal forward: the output launches, which live in a translation unit of their own
// (capi_causal_gqa.hip) so that the grouped twins of k_csf_out4 / k_cs_out compile beside capi_causal.hip, not behind it.  The
// chain (summaries, mixing, checks, workspace) stays in capi_causal.hip and runs on the k/v heads.
#pragma once
#include "capi_common.hpp"
#include "causal.hpp"

namespace mhla {
namespace capi {

constexpr int CS_GQA_MAX = 8;   // query heads per k/v head (as the decode calls: CST_GMAX)

// `o`: the arguments of the plain output launch, H its query heads, P the summaries of B * H / G (b, k/v head) pairs; `tab`: the
// chunk table of a pack, or null.  16-bit pipeline (hl: the summaries' format, epi: the fused norm x gate epilogue) and generic path.
int cs_out16_gqa(int hl, const CsOutArgs& o, int G, int B, bool epi, hipStream_t st, const cs_tab_t* tab);
int cs_out_gqa(int dtype, const CsOutArgs& o, int G, int B, hipStream_t st, const cs_tab_t* tab);

}  // namespace capi
}  // namespace mhla
