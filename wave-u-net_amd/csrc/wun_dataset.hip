// gfx950 (MI355X / CDNA4): the training batch producer behind the C ABI (include/wun.h: wun_gather_snippets) -- one batch of
// the snippet pipeline (Datasets.py:29-34 cut, Utils.py:26-36 gain + re-summed mix, Utils.py:38-42 centre crop) and the
// source-level augmentations (independent remix, channel swap, polarity) read straight out of planes resident in HBM.
//
//   gather_snippets_kernel   a_s = gain_s * x_s[start_s ..][c'] (sign flipped on request); targets[s][b] = the centre crop of
//                            a_s; mix[b] = ((a_0 + a_1) + a_2) + ... or a copy of the mix plane's window
//
// Copy-bound.  A lane owns one 16-byte granule of a mix row (four consecutive floats of the row, frames x channels) and takes
// it through EVERY source: each source float is read once, the running sum stays in registers, every destination float has
// one writer (no atomics).  Under remix each source of a row starts at its own frame, so its floats sit at their own offset
// inside a 16-byte granule: ld4_window (wun_device.h) reads the aligned granules inside the window and its two ends float by
// float, nothing outside [start, start + Tin).  The offsets are uniform per workgroup (one row per blockIdx.y), so the
// selection is a scalar branch.  The mix row is stored with 16-byte stores; a target row lies pad * C floats into the lane's
// grid and at its own address, so its stores are 16 bytes where that address allows and single floats elsewhere.
//
// Arithmetic (the bits are part of the contract): one float32 product per sample, rounded on its own, skipped when gain == 1
// (bits pass through); ascending adds, each rounded; no fused multiply-add -- __fmul_rn / __fadd_rn are never contracted.
// The descriptor table travels by value in the kernel arguments: no host-to-device copy, no allocation, no synchronisation.
// All index arithmetic is 64-bit (a resident data set exceeds 2^31 floats).
//
// Built WITHOUT the packed fp32 VALU instructions like the other shared elementwise units (csrc/Makefile NO_PK_FP32,
// DESIGN.md 5.3).  The entry's argument checks run before any GPU work.
#include "wun_device.h"
#include "wun_plan_impl.h"

#include <algorithm>

#define WUN_SNIPPET_BLOCK 256                  // lanes per workgroup, one granule of the mix row each
#define WUN_SNIPPET_MAX_SOURCES 8
// rows x sources of one launch: 24 * 8 * 16 bytes = 3 KB of table + 128 bytes of pointers and sizes, under HIP's 4 KB of
// kernel arguments
#define WUN_SNIPPET_ENTRIES (WUN_SNIPPET_ROWS * WUN_SNIPPET_MAX_SOURCES)

namespace wun {

struct SnippetArgs {
    const float* plane[WUN_SNIPPET_MAX_SOURCES];
    const float* mix_plane;                    // mix_mode 0 only
    float* mix;                                // row 0 of this launch: [rows][n]
    float* tgt;                                // source 0, row 0 of this launch: [S][B][nt]
    long long n, nt, padc, tgt_plane;          // floats: Tin * C, Tout * C, pad * C, B * Tout * C
    int S, mix_mode;
    wun_snippet_source d[WUN_SNIPPET_ENTRIES]; // [rows][S], packed
};
static_assert(sizeof(SnippetArgs) <= 4096, "the argument block must fit HIP's kernel-argument limit");

// floats j0 .. j0 + 3 of the window p[lo .. lo + n) (0 outside), channels swapped on request (n is even then)
__device__ __forceinline__ f32x4 window_quad(const float* __restrict__ p, long long lo, long long j0, long long n, bool swap) {
    if (swap && (j0 & 1)) {                    // a quad that straddles frames (an output row at an odd float): float by float
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long j = (j0 + r) ^ 1;
            v[r] = (j >= 0 && j < n) ? p[lo + j] : 0.f;
        }
        return v;
    }
    f32x4 v;
    switch (granule_offset(p, lo + j0)) {      // uniform over the workgroup
        case 0: v = ld4_window<0>(p, lo + j0, lo, lo + n); break;
        case 1: v = ld4_window<1>(p, lo + j0, lo, lo + n); break;
        case 2: v = ld4_window<2>(p, lo + j0, lo, lo + n); break;
        default: v = ld4_window<3>(p, lo + j0, lo, lo + n); break;
    }
    return swap ? (f32x4){v[1], v[0], v[3], v[2]} : v;
}

// floats [j0, j0 + 4) of a row of `len` floats at dst (only those inside the row): 16 bytes when the address allows
__device__ __forceinline__ void store_quad(float* __restrict__ dst, long long j0, long long len, f32x4 v) {
    if (j0 >= 0 && j0 + 4 <= len && granule_offset(dst, j0) == 0) {
        *reinterpret_cast<f32x4*>(dst + j0) = v;
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (j0 + r >= 0 && j0 + r < len) dst[j0 + r] = v[r];
    }
}

// grid (granules of a mix row / 256, rows of the launch)
template <int C>
__global__ __launch_bounds__(WUN_SNIPPET_BLOCK) void gather_snippets_kernel(SnippetArgs a) {
    const long long row = blockIdx.y;
    float* mrow = a.mix + row * a.n;
    // the lane's granule of the mix row: 16-byte aligned by construction (the row may start inside a granule)
    const long long j0 = 4LL * ((long long)blockIdx.x * WUN_SNIPPET_BLOCK + threadIdx.x) - granule_offset(mrow, 0);
    if (j0 >= a.n) return;
    const bool in_crop = j0 + 4 > a.padc && j0 < a.padc + a.nt;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int ns = (a.mix_mode == 0 && !in_crop) ? 0 : a.S;   // the mix is copied: outside the crop nothing needs the sources
    for (int s = 0; s < ns; ++s) {
        const wun_snippet_source d = a.d[row * a.S + s];
        f32x4 v = window_quad(a.plane[s], (long long)d.start * C, j0, a.n, C == 2 && (d.flags & 1u));
        if (d.gain != 1.0f) {                                 // (gain 1: the bits pass through)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = __fmul_rn(d.gain, v[r]);
        }
        if (d.flags & 2u) v = -v;
        if (in_crop) store_quad(a.tgt + s * a.tgt_plane + row * a.nt, j0 - a.padc, a.nt, v);
        if (s == 0) acc = v;
        else {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = __fadd_rn(acc[r], v[r]);
        }
    }
    if (a.mix_mode == 0) acc = window_quad(a.mix_plane, (long long)a.d[row * a.S].start * C, j0, a.n, false);
    store_quad(mrow, j0, a.n, acc);
}

}  // namespace wun

extern "C" int32_t wun_snippet_abi_size(void) { return (int32_t)sizeof(wun_snippet_source); }

extern "C" int wun_gather_snippets(const float* const* planes, const float* mix_plane, int64_t plane_frames, int32_t C,
                                   int32_t S, int32_t B, int64_t Tin, int64_t Tout, const wun_snippet_source* desc,
                                   int32_t mix_mode, float* mix_out, float* targets_out, void* stream) {
    using namespace wun;
    const char* who = "wun_gather_snippets";
    if (!planes || !desc || !mix_out || !targets_out) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    if (mix_mode != 0 && mix_mode != 1) return fail(WUN_ERR_INVALID, std::string(who) + ": mix_mode must be 0 or 1");
    if (mix_mode == 0 && !mix_plane) return fail(WUN_ERR_INVALID, std::string(who) + ": mix_mode 0 needs the mix plane (null argument)");
    if (C != 1 && C != 2) return fail(WUN_ERR_INVALID, std::string(who) + ": C must be 1 or 2");
    if (S < 1 || S > WUN_SNIPPET_MAX_SOURCES) return fail(WUN_ERR_INVALID, std::string(who) + ": S must be in 1..8");
    if (B < 1) return fail(WUN_ERR_INVALID, std::string(who) + ": B < 1");
    if (Tout < 1 || Tout > Tin || ((Tin - Tout) & 1) != 0)
        return fail(WUN_ERR_INVALID, std::string(who) + ": need 1 <= Tout <= Tin and an even Tin - Tout (symmetric crop)");
    if (plane_frames < Tin || plane_frames > ((int64_t)1 << 46) || Tin > ((int64_t)1 << 40))
        return fail(WUN_ERR_INVALID, std::string(who) + ": bad plane_frames (a window lies outside [0, plane_frames])");
    for (int s = 0; s < S; ++s) {
        if (!planes[s]) return fail(WUN_ERR_INVALID, std::string(who) + ": null plane " + std::to_string(s));
        if ((reinterpret_cast<uintptr_t>(planes[s]) & 3) != 0)
            return fail(WUN_ERR_INVALID, std::string(who) + ": plane " + std::to_string(s) + " is not 4-byte aligned");
    }
    if (((reinterpret_cast<uintptr_t>(mix_out) | reinterpret_cast<uintptr_t>(targets_out) | reinterpret_cast<uintptr_t>(mix_plane)) & 3) != 0)
        return fail(WUN_ERR_INVALID, std::string(who) + ": the mix plane and the outputs must be 4-byte aligned");
    for (int64_t k = 0; k < (int64_t)B * S; ++k) {
        const wun_snippet_source& d = desc[k];
        if (d.start < 0 || d.start > plane_frames - Tin)
            return fail(WUN_ERR_INVALID, std::string(who) + ": window of row " + std::to_string(k / S) + ", source " +
                        std::to_string(k % S) + " lies outside [0, plane_frames]");
        if (d.flags & ~3u) return fail(WUN_ERR_INVALID, std::string(who) + ": unknown flag bits");
        if ((d.flags & 1u) && C != 2) return fail(WUN_ERR_INVALID, std::string(who) + ": the channel swap needs C == 2");
    }
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)Tin * C, nt = (long long)Tout * C;
    // granules a row can touch: its floats / 4, plus one for a row that starts inside a granule
    const long long granules = (n + 3) / 4 + 1;
    for (int r0 = 0; r0 < B; r0 += WUN_SNIPPET_ROWS) {
        const int rows = std::min(B - r0, WUN_SNIPPET_ROWS);
        SnippetArgs a;
        for (int s = 0; s < WUN_SNIPPET_MAX_SOURCES; ++s) a.plane[s] = s < S ? planes[s] : nullptr;
        a.mix_plane = mix_plane;
        a.mix = mix_out + (long long)r0 * n;
        a.tgt = targets_out + (long long)r0 * nt;
        a.n = n; a.nt = nt; a.padc = (long long)((Tin - Tout) / 2) * C; a.tgt_plane = (long long)B * nt;
        a.S = S; a.mix_mode = mix_mode;
        for (int k = 0; k < WUN_SNIPPET_ENTRIES; ++k)
            a.d[k] = k < rows * S ? desc[(int64_t)r0 * S + k] : wun_snippet_source{0, 1.0f, 0u};
        const dim3 grid((unsigned)((granules + WUN_SNIPPET_BLOCK - 1) / WUN_SNIPPET_BLOCK), (unsigned)rows);
        // bytes: every source read once + the targets, the mix written once (mode 0: the mix plane read, sources in the crop only)
        const double rd = mix_mode ? (double)S * n : (double)n + (double)S * nt;
        prof_scope_begin("gather_snippets_kernel", 0.0, st, "", 4.0 * rows * (rd + n + (double)S * nt));
        if (C == 1) hipLaunchKernelGGL(gather_snippets_kernel<1>, grid, dim3(WUN_SNIPPET_BLOCK), 0, st, a);
        else hipLaunchKernelGGL(gather_snippets_kernel<2>, grid, dim3(WUN_SNIPPET_BLOCK), 0, st, a);
        prof_scope_end(st);
        HIP_TRY(hipGetLastError());
    }
    return WUN_OK;
}
