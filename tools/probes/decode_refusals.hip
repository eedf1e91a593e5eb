// Host-only check of the decode C layer's argument handling under AddressSanitizer and UBSan: the checked state constructors of
// capi_causal_state.hip and entry points that are refused before any launch, with null, misaligned and extreme values.  No kernel
// runs and no GPU is needed; the pointers are fake addresses that are never dereferenced.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++20 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Xclang -target-feature -Xclang -packed-fp32-ops '-DMHLA_BUILD_FLAGS="asan"' tools/probes/decode_refusals.hip -o tools/probes/decode_refusals
//   ASAN_OPTIONS=detect_leaks=0 tools/probes/decode_refusals        # (the HIP runtime's own start-up allocations are not this program's)
// Prints one line per case and exits 0 when every case was refused (or accepted) as expected and no sanitizer report was raised.
#include <climits>
#include <cstdio>
#include <cstring>
#include "../../mhla_amd/csrc/capi_causal_state.hip"

static int bad = 0;
static void expect(const char* what, int rc, bool refused) {
    const bool ok = refused ? (rc != MHLA_OK && mhla::capi::g_err[0]) : rc == MHLA_OK;
    printf("%-4s %-58s rc=%d %s\n", ok ? "ok" : "FAIL", what, rc, rc ? mhla::capi::g_err : "");
    bad += !ok;
}
template <typename T> static T* at(int i, long off = 0) { return (T*)(((uintptr_t)1 << 32) + ((uintptr_t)i << 28) + off); }

int main() {
    float *mix = at<float>(1), *S = at<float>(2), *P = at<float>(3), *Cur = at<float>(4), *mult = at<float>(5);
    int32_t *pos = at<int32_t>(6), *full = at<int32_t>(7), *slot = at<int32_t>(8), *table = at<int32_t>(9), *off = at<int32_t>(10), *items = at<int32_t>(11);
    void *ws = at<void>(12), *blob = at<void>(13), *stream = nullptr;
    const auto fresh = [&] { return cs_state(mix, 4, 3, P, Cur, pos, full); };
    DecState s = fresh();

    // ---- the constructors
    expect("cs_dense", cs_dense(s, S), false);
    expect("cs_slots", cs_slots(s = fresh(), S, slot, 5), false);
    expect("cs_slots: map null", cs_slots(s = fresh(), S, nullptr, 5), true);
    expect("cs_slots: map misaligned", cs_slots(s = fresh(), S, at<int32_t>(8, 2), 5), true);
    expect("cs_slots: n_slots 0", cs_slots(s = fresh(), S, slot, 0), true);
    expect("cs_slots: n_slots INT_MIN", cs_slots(s = fresh(), S, slot, INT_MIN), true);
    expect("cs_paged", cs_paged(s = fresh(), S, 7, table, slot, 5), false);
    if (!(s.paged() && s.slotted() && !s.h16() && s.S.f32 == S && s.n_pages == 7 && s.n_slots == 5)) { puts("FAIL cs_paged: fields"); ++bad; }
    expect("cs_paged: pages null", cs_paged(s = fresh(), nullptr, 7, table, slot, 5), true);
    expect("cs_paged: pages misaligned", cs_paged(s = fresh(), at<float>(2, 8), 7, table, slot, 5), true);
    expect("cs_paged: table null", cs_paged(s = fresh(), S, 7, nullptr, slot, 5), true);
    expect("cs_paged: n_pages 0", cs_paged(s = fresh(), S, 0, table, slot, 5), true);
    expect("cs_paged: map null", cs_paged(s = fresh(), S, 7, table, nullptr, 5), true);
    expect("cs_paged_h16", cs_paged_h16(s = fresh(), S, mult, 7, table, slot, 5, 64, 64), false);
    if (!(s.h16() && !s.S.f32 && s.S.base() == (const void*)S && s.S.mult == mult)) { puts("FAIL cs_paged_h16: fields"); ++bad; }
    expect("cs_paged_h16: payload null", cs_paged_h16(s = fresh(), nullptr, mult, 7, table, slot, 5, 64, 64), true);
    expect("cs_paged_h16: multipliers null", cs_paged_h16(s = fresh(), S, nullptr, 7, table, slot, 5, 64, 64), true);
    expect("cs_paged_h16: multipliers misaligned", cs_paged_h16(s = fresh(), S, at<float>(5, 2), 7, table, slot, 5, 64, 64), true);
    expect("cs_paged_h16: K V not in groups of 64", cs_paged_h16(s = fresh(), S, mult, 7, table, slot, 5, 4, 4), true);
    expect("cs_paged_h16: K = V = INT_MAX", cs_paged_h16(s = fresh(), S, mult, 7, table, slot, 5, INT_MAX, INT_MAX), true);
    expect("cs_packed: rows of a dense state", cs_packed(s = fresh(), S, 0, nullptr, nullptr, 0, off), false);
    if (s.paged() || s.slotted() || s.n_pages || s.n_slots) { puts("FAIL cs_packed: fields"); ++bad; }
    expect("cs_packed: pages, no slots", cs_packed(s = fresh(), S, 7, table, nullptr, 9, off), false);
    if (!(s.paged() && !s.slotted() && s.n_pages == 7 && s.n_slots == 0)) { puts("FAIL cs_packed: fields with pages"); ++bad; }
    expect("cs_packed: off_dev null", cs_packed(s = fresh(), S, 7, table, slot, 5, nullptr), true);
    expect("cs_packed: off_dev misaligned", cs_packed(s = fresh(), S, 7, table, slot, 5, at<int32_t>(10, 1)), true);
    expect("cs_packed: table, S null", cs_packed(s = fresh(), nullptr, 7, table, slot, 5, off), true);
    expect("cs_packed: slots, n_slots -1", cs_packed(s = fresh(), S, 7, table, slot, -1, off), true);

    // ---- entry points, refused before any launch
    const mhla_view q{at<void>(14), 1 << 20, 128, 64}, k{at<void>(15), 1 << 20, 128, 64}, v{at<void>(16), 1 << 20, 128, 64}, none{};
    const mhla_mview out{at<void>(17), 1 << 20, 128, 64}, nom{};
    expect("step_paged: B 0", mhla_causal_step_paged(q, k, v, mix, 4, S, 7, table, 3, P, Cur, pos, slot, 5, 0, 0, out, none, nullptr, 0.f, nom, ws, 1 << 20, 0, 2, 2, 64,
                                                     64, 64, 1.f, MHLA_F32, stream), true);
    expect("step_paged: B = H = INT_MAX", mhla_causal_step_paged(q, k, v, mix, 4, S, 7, table, 3, P, Cur, pos, slot, 5, 0, 0, out, none, nullptr, 0.f, nom, ws, 1 << 20, INT_MAX,
                                                                 INT_MAX, INT_MAX, 64, 64, 64, 1.f, MHLA_F32, stream), true);
    expect("step_paged: max_pos INT64_MAX", mhla_causal_step_paged(q, k, v, mix, 4, S, 7, table, 3, P, Cur, pos, slot, 5, INT64_MAX, 1, out, none, nullptr, 0.f, nom, ws, 1 << 20,
                                                                   2, 2, 2, 64, 64, 64, 1.f, MHLA_F32, stream), true);
    expect("step_paged: workspace of 0 bytes", mhla_causal_step_paged(q, k, v, mix, 4, S, 7, table, 3, P, Cur, pos, slot, 5, 63, 1, out, none, nullptr, 0.f, nom, ws, 0, 2, 2, 2,
                                                                      64, 64, 64, 1.f, MHLA_F32, stream), true);
    expect("step_dev_paged_h16: cap_chunks INT_MAX", mhla_causal_step_dev_paged_h16(q, k, v, mix, INT_MAX, S, mult, 7, table, INT_MAX, P, Cur, pos, slot, 5, full, nullptr, nullptr,
                                                                                     0, 0, 0, out, none, nullptr, 0.f, nom, ws, 1 << 20, 2, 2, 2, 64, 64, 64, 1.f,
                                                                                     MHLA_F32, stream), true);
    expect("step_dev_slots: tab_rows INT64_MAX", mhla_causal_step_dev_slots(q, k, v, mix, 4, S, 3, P, Cur, pos, slot, 5, full, at<void>(18), at<void>(19), 32, INT64_MAX, 1, out,
                                                                            none, nullptr, 0.f, nom, ws, 1 << 20, 2, 2, 2, 64, 64, 64, 1.f, MHLA_F32, stream), true);
    expect("extend_packed: n_tokens INT_MAX", mhla_causal_extend_packed(q, k, v, mix, 4, S, 7, table, 3, P, Cur, pos, slot, 5, off, INT_MAX, 0, 0, 0, out, none, nullptr, 0.f,
                                                                        nom, ws, 1 << 20, 2, 2, 2, 64, 64, 64, 1.f, MHLA_F32, stream), true);
    expect("extend_packed: max_end INT64_MIN", mhla_causal_extend_packed(q, k, v, mix, 4, S, 7, table, 3, P, Cur, pos, slot, 5, off, 65535, INT64_MIN, 0, 0, out, none, nullptr,
                                                                         0.f, nom, ws, 1 << 20, 2, 2, 2, 64, 64, 64, 1.f, MHLA_F32, stream), true);
    expect("extend_packed: max_end INT64_MAX", mhla_causal_extend_packed(q, k, v, mix, 4, S, 7, table, 3, P, Cur, pos, slot, 5, off, 65535, INT64_MAX, 0, 0, out, none, nullptr,
                                                                         0.f, nom, ws, 1 << 20, 2, 2, 2, 64, 64, 64, 1.f, MHLA_F32, stream), true);
    expect("verify_slots: max_later INT_MAX", mhla_causal_verify_slots(q, k, v, mix, 4, S, 3, P, Cur, pos, slot, 5, off, 130, 65, INT_MAX, 1, 0, out, none, nullptr, 0.f, nom, ws,
                                                                       1 << 20, 2, 2, 2, 64, 64, 64, 1.f, MHLA_F32, stream), true);
    expect("commit_paged: accept_dev null", mhla_causal_commit_paged(k, v, mix, 4, S, 7, table, 3, P, Cur, pos, slot, 5, off, nullptr, 130, 65, 0, 0, 0, ws, 1 << 20, 2, 2, 64, 64,
                                                                     64, MHLA_F32, stream), true);
    expect("commit_packed: workspace null", mhla_causal_commit_packed(k, v, mix, 4, S, 7, table, 3, P, Cur, pos, slot, 5, off, off, 130, 65, 0, 0, nullptr, 0, 2, 2, 64, 64, 64,
                                                                      MHLA_F32, stream), true);
    expect("varlen_state_init_paged: n_seqs INT_MAX", mhla_causal_varlen_state_init_paged(k, v, mix, 4, S, 7, table, 3, P, Cur, INT_MAX, off, slot, 5, 64, 130, 2, 64, 64, 64, 3,
                                                                                          at<int32_t>(20), at<int32_t>(21), MHLA_F32, stream), true);
    expect("varlen_state_init_paged_h16: chunk table null", mhla_causal_varlen_state_init_paged_h16(k, v, mix, 4, S, mult, 7, table, 3, P, Cur, 2, off, slot, 5, 64, 130, 2, 64,
                                                                                                    64, 64, 3, nullptr, at<int32_t>(21), ws, 1 << 20, MHLA_F32, stream), true);
    expect("swap_out: n_seqs = n_pages_moved = INT_MAX", mhla_causal_swap_out_paged(S, mult, 7, P, Cur, pos, full, 5, items, INT_MAX, INT_MAX, 0, 1, blob, 2, 64, 64, stream), true);
    expect("swap_in: items [INT_MIN, INT_MAX)", mhla_causal_swap_in_paged(S, nullptr, 7, P, Cur, pos, nullptr, 5, items, 2, 3, INT_MIN, INT_MAX, blob, 2, 64, 64, stream), true);
    expect("swap_in: an empty range is accepted, nothing launched", mhla_causal_swap_in_paged(S, nullptr, 7, P, Cur, pos, nullptr, 5, items, 2, 3, 4, 4, blob, 2, 64, 64, stream), false);
    expect("swap_in: blob misaligned", mhla_causal_swap_in_paged(S, nullptr, 7, P, Cur, pos, nullptr, 5, items, 2, 3, 0, 1, at<void>(13, 8), 2, 64, 64, stream), true);
    // the size queries answer 0 where a dimension is not positive, and wrap nowhere a caller could reach with tensors that exist
    printf("ws: step %zu extend_packed %zu commit %zu prefill_h16 %zu swap %zu\n", mhla_causal_step_ws_bytes(0, 2, 64, 64, 0),
           mhla_causal_extend_packed_ws_bytes(2, 130, 4, 3, 64, 64, 1, 0), mhla_causal_commit_ragged_ws_bytes(-1, 0),
           mhla_causal_varlen_state_init_paged_h16_ws_bytes(INT_MAX, 0, 64, 64, 0), mhla_causal_swap_ws_bytes(INT_MAX, INT_MAX, 2, 64, 60, 1));
    printf("%s: %d case(s) not as expected\n", bad ? "FAILED" : "passed", bad);
    return bad ? 1 : 0;
}
