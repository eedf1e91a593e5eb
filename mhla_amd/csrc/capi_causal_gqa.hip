// Causal operator, grouped-query heads in the forward: the output kernels' grouped instantiations (k_csf_out4, k_cs_out over
// CsOutArgsGqa / CsOutArgsVarGqa) and their launches.  Geometry, LDS and dispatch are those of the plain launches in
// capi_causal.hip (cs_fwd16, cs_fwd_impl): one workgroup per query head, which reads k, v and the P tiles of its k/v head.
#include "capi_causal_gqa.hpp"
#include "causal_bf16.hpp"

namespace mhla {
namespace capi {

namespace {

// the uniform launch or, for a pack, the table instantiation: the plain arguments followed by the table, then the group
template <typename KP, typename KT>
int launch_gqa(KP plain, KT table, dim3 grid, dim3 block, size_t smem, hipStream_t st, const char* name, const char* name_tab,
               const CsOutArgs& o, int G, const cs_tab_t* tab) {
    if (!tab) {
        const CsOutArgsGqa a{o, G, o.H / G};
        return launch(plain, grid, block, smem, st, name, a);
    }
    const CsOutArgsVarGqa av{CsOutArgsVar{o, tab}, G, o.H / G};
    return launch(table, grid, block, smem, st, name_tab, av);
}

template <int HL>
int out16(const CsOutArgs& o, int G, int B, bool epi, hipStream_t st, const cs_tab_t* tab) {
    const int n = o.n, H = o.H;
    const int nvs = o.V / 64, nv = nvs % 4 == 0 ? 4 : nvs % 3 == 0 ? 3 : nvs % 2 == 0 ? 2 : 1;   // (as cs_fwd16)
#define OUT4(NV, EPI) launch_gqa(fast::k_csf_out4<NV, EPI, HL, 1, CsOutArgsGqa>, fast::k_csf_out4<NV, EPI, HL, 1, CsOutArgsVarGqa>,          \
                                 dim3(EPI ? n : (n + fast::CSF_OUT4_CPW - 1) / fast::CSF_OUT4_CPW, B * H, nvs / NV), dim3(fast::NT4),           \
                                 fast::csf_out4_smem<NV, EPI, HL>(), st, EPI ? "k_csf_out4<norm,gqa>" : "k_csf_out4<gqa>",                      \
                                 EPI ? "k_csf_out4<norm,tab,gqa>" : "k_csf_out4<tab,gqa>", o, G, tab)
#define OUT4H2(NV) launch_gqa(fast::k_csf_out4<NV, true, HL, 2, CsOutArgsGqa>, fast::k_csf_out4<NV, true, HL, 2, CsOutArgsVarGqa>,           \
                              dim3(n, B * H, 1), dim3(fast::NT4), fast::csf_out4_smem<NV, true, HL, 2>(), st, "k_csf_out4<norm,2,gqa>",         \
                              "k_csf_out4<norm,2,tab,gqa>", o, G, tab)
    if (epi && nvs > 4) return nvs == 6 ? OUT4H2(3) : OUT4H2(4);
    if (epi) return nvs == 1 ? OUT4(1, true) : nvs == 2 ? OUT4(2, true) : nvs == 3 ? OUT4(3, true) : OUT4(4, true);
    return nv == 1 ? OUT4(1, false) : nv == 2 ? OUT4(2, false) : nv == 3 ? OUT4(3, false) : OUT4(4, false);
#undef OUT4
#undef OUT4H2
}

}  // namespace

int cs_out16_gqa(int hl, const CsOutArgs& o, int G, int B, bool epi, hipStream_t st, const cs_tab_t* tab) {
    return hl == 2 ? out16<2>(o, G, B, epi, st, tab) : hl == 1 ? out16<1>(o, G, B, epi, st, tab) : out16<0>(o, G, B, epi, st, tab);
}

int cs_out_gqa(int dtype, const CsOutArgs& o, int G, int B, hipStream_t st, const cs_tab_t* tab) {
    DISPATCH_T(dtype, {
        return launch_gqa(k_cs_out<ET, CsOutArgsGqa>, k_cs_out<ET, CsOutArgsVarGqa>, dim3(o.n, B * o.H, (o.V + 63) / 64), dim3(NTHREADS),
                          CS_OUT_SMEM_FLOATS * 4, st, "k_cs_out<gqa>", "k_cs_out<tab,gqa>", o, G, tab);
    });
    return MHLA_OK;
}

}  // namespace capi
}  // namespace mhla
