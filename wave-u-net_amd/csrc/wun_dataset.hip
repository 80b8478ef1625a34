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
//   gather_snippets_speed_kernel   the same batch with speed perturbation (wun_gather_snippets_speed): a source
//                            whose rate index is not 0 is RESAMPLED while it is read.  The workgroup stages in LDS the input
//                            frames its 1024 output floats need (channel-swapped on request, zero outside the source's span)
//                            and the entry's phase-major table, then every lane walks the taps of its four floats, k
//                            ascending, one fmaf per tap and one accumulator per float: wun_resample's chain and bits.  Gain,
//                            sign, crop and the mix sum follow as above.  A source's rate is uniform over the workgroup (one
//                            row per blockIdx.y), so the choice of path is a scalar branch; no lane leaves before the last
//                            barrier (a granule behind the row's end is a store predicate here, not a return).
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

// ---- speed perturbation: the gather that resamples a rated source while it reads it ------------------------
// LDS of a workgroup: the input window of its 1024 output floats, then the entry's table at an odd row stride.
//   window: the outputs span at most 1024 / C frames (C == 2 and a row that starts at an odd float: 513), whose q = (t down +
//           half) / up span at most (frames - 1) down / up + 1 values, plus the K - 1 frames under the first:
//           C == 1: 1023 * 2 + 1 + 40 = 2087 floats;  C == 2: (512 * 2 + 1 + 40) * 2 = 2130 floats  (down / up <= 2, K <= 41)
//   table : up rows of K floats at stride K | 1: lanes of a wave read rows p at the same k, and an odd stride maps the 32
//           residues of p onto the 32 banks of a 4-byte LDS read (equal p: one address, a broadcast).  up * (K | 1) <= 64 * 21
//           for up >= down; (20 down + 1 + up - 1) + up <= 1407 for down > up.
//   A lane's four floats sit four floats behind its neighbour's, so at every tap the lanes of a wave read the window at a
//   stride of about 4 down / up floats -- 4-way on the 32 banks of a 4-byte read at stride 4.  The image therefore skips one
//   float after every 32 (WUN_SPEED_WIN_AT): 32 lanes at stride 4 then fall on 32 banks.
#define WUN_SPEED_WIN_FLOATS 2200
#define WUN_SPEED_WIN_AT(i) ((i) + ((i) >> 5))
#define WUN_SPEED_WIN_LDS (WUN_SPEED_WIN_FLOATS + WUN_SPEED_WIN_FLOATS / 32 + 1)
#define WUN_SPEED_TAB_FLOATS 1472
static_assert((WUN_SPEED_WIN_LDS + WUN_SPEED_TAB_FLOATS) * 4 <= 16384, "LDS of the speed gather");

struct SpeedArgs {
    SnippetArgs g;                                       // mix_mode is 1 here
    const float* table[WUN_SPEED_RATES];                 // device: wun_resample_design's phase-major tables
    long long nsrc[WUN_SPEED_RATES];                     // source frames of a window: ((Tin - 1) down) / up + 1
    int up[WUN_SPEED_RATES], down[WUN_SPEED_RATES], half[WUN_SPEED_RATES], K[WUN_SPEED_RATES];
    unsigned char rate[WUN_SNIPPET_ENTRIES];             // [rows][S], packed like g.d: 0 = unit, i = bank entry i - 1
};
static_assert(sizeof(SpeedArgs) <= 4096, "the argument block must fit HIP's kernel-argument limit");

// grid (granules of a mix row / 256, rows of the launch)
template <int C>
__global__ __launch_bounds__(WUN_SNIPPET_BLOCK) void gather_snippets_speed_kernel(SpeedArgs a) {
    __shared__ float win[WUN_SPEED_WIN_LDS];
    __shared__ float tab[WUN_SPEED_TAB_FLOATS];
    const int tid = threadIdx.x;
    const long long row = blockIdx.y;
    const long long n = a.g.n;
    float* mrow = a.g.mix + row * n;
    // first float of the workgroup's 1024 and the lane's granule, as in gather_snippets_kernel
    const long long jb = 4LL * (long long)blockIdx.x * WUN_SNIPPET_BLOCK - granule_offset(mrow, 0);
    if (jb >= n) return;                                 // the whole workgroup lies behind the row (uniform: nobody waits)
    const long long j0 = jb + 4 * tid;
    const bool live = j0 < n;                            // a lane behind the row's end stays for the barriers and stores nothing
    const bool in_crop = live && j0 + 4 > a.g.padc && j0 < a.g.padc + a.g.nt;
    // frames of the workgroup's outputs inside the row
    const long long jlo = jb < 0 ? 0 : jb, jhi = (jb + 4 * WUN_SNIPPET_BLOCK < n ? jb + 4 * WUN_SNIPPET_BLOCK : n) - 1;
    const long long t_first = jlo / C, t_last = jhi / C;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    bool staged = false;                                 // uniform: the LDS image of an earlier source may still be read
    for (int s = 0; s < a.g.S; ++s) {
        const wun_snippet_source d = a.g.d[row * a.g.S + s];
        const int ri = a.rate[row * a.g.S + s];          // uniform over the workgroup
        const bool swap = C == 2 && (d.flags & 1u);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ri == 0) {
            if (live) v = window_quad(a.g.plane[s], (long long)d.start * C, j0, n, swap);
        } else {
            const int e = ri - 1;
            const int up = a.up[e], down = a.down[e], K = a.K[e], Kp = K | 1;
            const long long nsrc = a.nsrc[e];
            const long long base = t_first * down + a.half[e];        // uniform 64-bit part of t down + half
            const long long qb = base / up;
            const unsigned rb = (unsigned)(base % up);
            const long long m_lo = qb - (K - 1);                      // first staged frame, relative to the window's start
            const int W = (int)((rb + (unsigned)(t_last - t_first) * (unsigned)down) / (unsigned)up) + K;   // staged frames
            if (staged) __syncthreads();                              // every lane has finished with the image of the last source
            const float* __restrict__ x = a.g.plane[s];
            const long long lo = ((long long)d.start + m_lo) * C;     // plane index of the image's first float
            for (int i = tid; i < W * C; i += WUN_SNIPPET_BLOCK) {
                const long long m = m_lo + i / C;
                win[WUN_SPEED_WIN_AT(i)] = (m >= 0 && m < nsrc) ? x[lo + (swap ? (i ^ 1) : i)] : 0.f;
            }
            const float* __restrict__ taps = a.table[e];
            for (int i = tid; i < up * K; i += WUN_SNIPPET_BLOCK) tab[(i / K) * Kp + i % K] = taps[i];
            __syncthreads();
            staged = true;
            // the lane's four floats: their frame, channel, tap row and the image index of v[q]
            int iq[4], ip[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                long long j = j0 + r;
                j = j < jlo ? jlo : (j > jhi ? jhi : j);              // outside the row: any staged float (never stored)
                const unsigned dt = (unsigned)(j / C - t_first);      // <= 1024 / C
                const unsigned tt = rb + dt * (unsigned)down;         // < 2^31: up, down <= WUN_SPEED_MAX_RATIO
                iq[r] = ((int)(tt / (unsigned)up) + K - 1) * C + (int)(j % C);
                ip[r] = (int)(tt % (unsigned)up) * Kp;
            }
            for (int k = 0; k < K; ++k) {                             // k ascending: the one accumulation order
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaf(tab[ip[r] + k], win[WUN_SPEED_WIN_AT(iq[r] - k * C)], v[r]);
            }
        }
        if (d.gain != 1.0f) {                                         // (gain 1: the bits pass through)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = __fmul_rn(d.gain, v[r]);
        }
        if (d.flags & 2u) v = -v;
        if (in_crop) store_quad(a.g.tgt + s * a.g.tgt_plane + row * a.g.nt, j0 - a.g.padc, a.g.nt, v);
        if (s == 0) acc = v;
        else {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = __fadd_rn(acc[r], v[r]);
        }
    }
    if (live) store_quad(mrow, j0, n, acc);
}

}  // namespace wun

extern "C" int32_t wun_snippet_abi_size(void) { return (int32_t)sizeof(wun_snippet_source); }

namespace wun {

// the argument checks of both entries, before any GPU work
static int check_gather(const char* who, const float* const* planes, const float* mix_plane, int64_t plane_frames, int32_t C,
                        int32_t S, int32_t B, int64_t Tin, int64_t Tout, const wun_snippet_source* desc, int32_t mix_mode,
                        float* mix_out, float* targets_out, const uint8_t* rate = nullptr) {
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
        // (a rated window has its own length: wun_gather_snippets_speed checks it against the bank)
        if (!(rate && rate[k]) && (d.start < 0 || d.start > plane_frames - Tin))
            return fail(WUN_ERR_INVALID, std::string(who) + ": window of row " + std::to_string(k / S) + ", source " +
                        std::to_string(k % S) + " lies outside [0, plane_frames]");
        if (d.flags & ~3u) return fail(WUN_ERR_INVALID, std::string(who) + ": unknown flag bits");
        if ((d.flags & 1u) && C != 2) return fail(WUN_ERR_INVALID, std::string(who) + ": the channel swap needs C == 2");
    }
    return WUN_OK;
}

// the argument block of the launch that carries rows [r0, r0 + rows) of the batch
static void fill_args(SnippetArgs& a, const float* const* planes, const float* mix_plane, int32_t C, int32_t S, int32_t B,
                      int64_t Tin, int64_t Tout, const wun_snippet_source* desc, int32_t mix_mode, float* mix_out,
                      float* targets_out, int r0, int rows) {
    const long long n = (long long)Tin * C, nt = (long long)Tout * C;
    for (int s = 0; s < WUN_SNIPPET_MAX_SOURCES; ++s) a.plane[s] = s < S ? planes[s] : nullptr;
    a.mix_plane = mix_plane;
    a.mix = mix_out + (long long)r0 * n;
    a.tgt = targets_out + (long long)r0 * nt;
    a.n = n; a.nt = nt; a.padc = (long long)((Tin - Tout) / 2) * C; a.tgt_plane = (long long)B * nt;
    a.S = S; a.mix_mode = mix_mode;
    for (int k = 0; k < WUN_SNIPPET_ENTRIES; ++k)
        a.d[k] = k < rows * S ? desc[(int64_t)r0 * S + k] : wun_snippet_source{0, 1.0f, 0u};
}

static void launch_plain(const SnippetArgs& a, dim3 grid, int32_t C, int rows, hipStream_t st) {
    // bytes: every source read once + the targets, the mix written once (mode 0: the mix plane read, sources in the crop only)
    const double rd = a.mix_mode ? (double)a.S * a.n : (double)a.n + (double)a.S * a.nt;
    prof_scope_begin("gather_snippets_kernel", 0.0, st, "", 4.0 * rows * (rd + a.n + (double)a.S * a.nt));
    if (C == 1) hipLaunchKernelGGL(gather_snippets_kernel<1>, grid, dim3(WUN_SNIPPET_BLOCK), 0, st, a);
    else hipLaunchKernelGGL(gather_snippets_kernel<2>, grid, dim3(WUN_SNIPPET_BLOCK), 0, st, a);
    prof_scope_end(st);
}

}  // namespace wun

extern "C" int wun_gather_snippets(const float* const* planes, const float* mix_plane, int64_t plane_frames, int32_t C,
                                   int32_t S, int32_t B, int64_t Tin, int64_t Tout, const wun_snippet_source* desc,
                                   int32_t mix_mode, float* mix_out, float* targets_out, void* stream) {
    using namespace wun;
    int rc;
    if ((rc = check_gather("wun_gather_snippets", planes, mix_plane, plane_frames, C, S, B, Tin, Tout, desc, mix_mode, mix_out,
                           targets_out)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    // granules a row can touch: its floats / 4, plus one for a row that starts inside a granule
    const long long granules = ((long long)Tin * C + 3) / 4 + 1;
    for (int r0 = 0; r0 < B; r0 += WUN_SNIPPET_ROWS) {
        const int rows = std::min(B - r0, WUN_SNIPPET_ROWS);
        SnippetArgs a;
        fill_args(a, planes, mix_plane, C, S, B, Tin, Tout, desc, mix_mode, mix_out, targets_out, r0, rows);
        launch_plain(a, dim3((unsigned)((granules + WUN_SNIPPET_BLOCK - 1) / WUN_SNIPPET_BLOCK), (unsigned)rows), C, rows, st);
        HIP_TRY(hipGetLastError());
    }
    return WUN_OK;
}

namespace {

int gcd_i(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

// a ratio of the rate bank: positive, coprime, not 1/1 (WUN_ERR_INVALID); within the ceiling and [1/2, 2] (WUN_ERR_UNSUPPORTED)
int check_speed_ratio(const std::string& who, int32_t up, int32_t down) {
    if (up <= 0 || down <= 0) return fail(WUN_ERR_INVALID, who + ": up and down must be positive");
    if (gcd_i(up, down) != 1) return fail(WUN_ERR_INVALID, who + ": up / down must be coprime (reduced by their gcd)");
    if (up == 1 && down == 1) return fail(WUN_ERR_INVALID, who + ": the ratio 1/1 is the unit rate (rate index 0), not a bank entry");
    if (up > WUN_SPEED_MAX_RATIO || down > WUN_SPEED_MAX_RATIO)
        return fail(WUN_ERR_UNSUPPORTED, who + ": max(up, down) above the ceiling of 64");
    if (down > 2 * up || up > 2 * down) return fail(WUN_ERR_UNSUPPORTED, who + ": the speed down / up lies outside [1/2, 2]");
    return WUN_OK;
}

int speed_taps(int up, int down) { return (20 * std::max(up, down) + 1 + up - 1) / up; }

}  // namespace

extern "C" int32_t wun_speed_abi_size(void) { return (int32_t)sizeof(wun_speed_bank); }

extern "C" int64_t wun_speed_source_frames(int64_t Tin, int32_t up, int32_t down) {
    const char* who = "wun_speed_source_frames";
    if (Tin < 1 || Tin > ((int64_t)1 << 40)) return fail(WUN_ERR_INVALID, std::string(who) + ": Tin must be in 1..2^40");
    int rc;
    if ((rc = check_speed_ratio(who, up, down))) return rc;
    return ((Tin - 1) * down) / up + 1;
}

extern "C" int wun_gather_snippets_speed(const float* const* planes, const float* mix_plane, int64_t plane_frames, int32_t C,
                                         int32_t S, int32_t B, int64_t Tin, int64_t Tout, const wun_snippet_source* desc,
                                         const uint8_t* rate, const wun_speed_bank* bank, int32_t mix_mode, float* mix_out,
                                         float* targets_out, void* stream) {
    using namespace wun;
    const std::string who = "wun_gather_snippets_speed";
    int rc;
    if ((rc = check_gather(who.c_str(), planes, mix_plane, plane_frames, C, S, B, Tin, Tout, desc, mix_mode, mix_out, targets_out, rate)))
        return rc;
    bool rated = false;
    if (rate)
        for (int64_t k = 0; k < (int64_t)B * S && !rated; ++k) rated = rate[k] != 0;
    if (rated && !bank) return fail(WUN_ERR_INVALID, who + ": a non-zero rate index needs a rate bank (null argument)");
    long long nsrc[WUN_SPEED_RATES] = {0};
    if (bank) {
        if (bank->n < 0 || bank->n > WUN_SPEED_RATES) return fail(WUN_ERR_INVALID, who + ": bank->n must be in 0..8");
        for (int e = 0; e < bank->n; ++e) {
            if ((rc = check_speed_ratio(who + ": bank entry " + std::to_string(e), bank->up[e], bank->down[e]))) return rc;
            if (!bank->table[e]) return fail(WUN_ERR_INVALID, who + ": null table of bank entry " + std::to_string(e));
            if ((reinterpret_cast<uintptr_t>(bank->table[e]) & 3) != 0)
                return fail(WUN_ERR_INVALID, who + ": the table of bank entry " + std::to_string(e) + " is not 4-byte aligned");
            const int up = bank->up[e], down = bank->down[e], K = speed_taps(up, down);
            // the LDS image of a workgroup (the bounds above make this hold; see WUN_SPEED_WIN_FLOATS)
            const long long span = C == 2 ? 512 : 1023;
            if (((up - 1 + span * down) / up + K) * C > WUN_SPEED_WIN_FLOATS || up * (K | 1) > WUN_SPEED_TAB_FLOATS)
                return fail(WUN_ERR_UNSUPPORTED, who + ": bank entry " + std::to_string(e) + " exceeds the LDS image of a workgroup");
            nsrc[e] = ((long long)(Tin - 1) * down) / up + 1;
        }
    }
    if (rated) {
        if (mix_mode != 1)
            return fail(WUN_ERR_INVALID, who + ": a rated source needs mix_mode 1 (the mix plane is not resampled)");
        for (int64_t k = 0; k < (int64_t)B * S; ++k) {
            if (rate[k] == 0) continue;
            if (rate[k] > bank->n)
                return fail(WUN_ERR_INVALID, who + ": rate index " + std::to_string((int)rate[k]) + " of row " + std::to_string(k / S) +
                            ", source " + std::to_string(k % S) + " is above bank->n");
            if (desc[k].start < 0 || desc[k].start > plane_frames - nsrc[rate[k] - 1])
                return fail(WUN_ERR_INVALID, who + ": rated window of row " + std::to_string(k / S) + ", source " +
                            std::to_string(k % S) + " lies outside [0, plane_frames]");
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)Tin * C, nt = (long long)Tout * C;
    const long long granules = (n + 3) / 4 + 1;
    for (int r0 = 0; r0 < B; r0 += WUN_SNIPPET_ROWS) {
        const int rows = std::min(B - r0, WUN_SNIPPET_ROWS);
        SpeedArgs a;
        fill_args(a.g, planes, mix_plane, C, S, B, Tin, Tout, desc, mix_mode, mix_out, targets_out, r0, rows);
        bool any = false;
        for (int k = 0; k < WUN_SNIPPET_ENTRIES; ++k) {
            a.rate[k] = (rated && k < rows * S) ? rate[(int64_t)r0 * S + k] : 0;
            any = any || a.rate[k] != 0;
        }
        const dim3 grid((unsigned)((granules + WUN_SNIPPET_BLOCK - 1) / WUN_SNIPPET_BLOCK), (unsigned)rows);
        if (!any) {                                  // rows at the unit rate: the plain kernel, either mix mode
            launch_plain(a.g, grid, C, rows, st);
        } else {
            double fma = 0.0;
            for (int e = 0; e < WUN_SPEED_RATES; ++e) {
                const bool used = e < bank->n;
                a.table[e] = used ? bank->table[e] : nullptr;
                a.up[e] = used ? bank->up[e] : 1; a.down[e] = used ? bank->down[e] : 1;
                a.half[e] = 10 * std::max(a.up[e], a.down[e]);
                a.K[e] = speed_taps(a.up[e], a.down[e]);
                a.nsrc[e] = nsrc[e];
            }
            for (int k = 0; k < rows * S; ++k)
                if (a.rate[k]) fma += (double)n * a.K[a.rate[k] - 1];
            prof_scope_begin("gather_snippets_speed_kernel", 2.0 * fma, st, "", 4.0 * rows * ((double)S * n + n + (double)S * nt));
            if (C == 1) hipLaunchKernelGGL(gather_snippets_speed_kernel<1>, grid, dim3(WUN_SNIPPET_BLOCK), 0, st, a);
            else hipLaunchKernelGGL(gather_snippets_speed_kernel<2>, grid, dim3(WUN_SNIPPET_BLOCK), 0, st, a);
            prof_scope_end(st);
        }
        HIP_TRY(hipGetLastError());
    }
    return WUN_OK;
}
