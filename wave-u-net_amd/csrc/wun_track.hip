// gfx950 (MI355X / CDNA4): whole-track separation behind the C ABI (include/wun.h: wun_forward_windows, wun_scatter_windows,
// wun_separate_track, wun_separate_positions) -- the loop of Evaluate.predict_track (Evaluate.py:113-143) without a host in it.
//
//   gather_windows_kernel   row b of the forward pass's NCW mix = track[pos[b] .. pos[b] + Tin): the first pass of wun_forward
//                           (btc_to_ncw*_kernel on a materialised [B, Tin, C] batch) reading the track itself
//   scatter_windows_kernel  preds[s][f] = outputs[s][row][f - pos[row]] for the runs of frames the host assigned to `row`
//
// Both only move floats: copy-bound, 16-byte accesses, consecutive lanes on consecutive quads.  A window starts at ANY frame
// of the track, so its source floats sit at any of the four offsets inside a 16-byte granule: a lane reads the aligned
// granules that hold its floats (vector loads) and picks its four; a granule that is not wholly inside the row (its first
// and last one) is read float by float, inside the row only -- nothing outside the window is ever touched.  The offset is
// uniform per workgroup (one row / one run per blockIdx.y) and a template parameter of the body, so the pick is register
// renaming, not indexing.  No atomics: every destination float has one writer.
//
// Built WITHOUT the packed fp32 VALU instructions like the other shared elementwise units (csrc/Makefile NO_PK_FP32,
// DESIGN.md 5.3).  The entry points' argument checks run before any GPU work.
#include "wun_device.h"
#include "wun_plan_impl.h"

#include <algorithm>
#include <new>
#include <vector>

#define WUN_TRACK_ROWS 64      // rows / runs per launch: the table travels by value in the kernel arguments
#define WUN_TRACK_BLOCK 256    // lanes per workgroup, one quad of destination floats each

namespace wun {      // the kernels carry the library's wun:: prefix in profiler output

// (ld4_window / granule_offset, the reads of a window that starts at any float: wun_device.h)
struct GatherArgs {
    const float* track; float* dst;          // dst: NCW row 0 of the launch's first batch row
    long long pos[WUN_TRACK_ROWS];           // first frame of the row's window; < 0: a row of zeros
    int T, pitch;
};

// grid (quads of a row / 256, rows): a lane owns time steps t0 .. t0 + 3 of every channel of one row
template <int C, int M>
__device__ __forceinline__ void gather_body(const GatherArgs& a, long long pos, int t0, float* __restrict__ drow) {
    const long long lo = pos * C, hi = (pos + a.T) * C, i = (pos + t0) * C;
    if (C == 1) {
        *reinterpret_cast<f32x4*>(drow + t0) = ld4_window<M>(a.track, i, lo, hi);
    } else {
        const f32x4 u = ld4_window<M>(a.track, i, lo, hi), v = ld4_window<M>(a.track, i + 4, lo, hi);
        *reinterpret_cast<f32x4*>(drow + t0) = (f32x4){u[0], u[2], v[0], v[2]};
        *reinterpret_cast<f32x4*>(drow + a.pitch + t0) = (f32x4){u[1], u[3], v[1], v[3]};
    }
}

template <int C>
__global__ __launch_bounds__(WUN_TRACK_BLOCK) void gather_windows_kernel(GatherArgs a) {
    const int t0 = ((int)blockIdx.x * WUN_TRACK_BLOCK + (int)threadIdx.x) * 4;
    if (t0 >= a.T) return;
    const long long pos = a.pos[blockIdx.y];
    float* drow = a.dst + (long long)blockIdx.y * C * a.pitch;
    if (pos < 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) *reinterpret_cast<f32x4*>(drow + (long long)c * a.pitch + t0) = (f32x4){0.f, 0.f, 0.f, 0.f};
        return;
    }
    switch (granule_offset(a.track, pos * C)) {       // uniform over the workgroup
        case 0: gather_body<C, 0>(a, pos, t0, drow); break;
        case 1: gather_body<C, 1>(a, pos, t0, drow); break;
        case 2: gather_body<C, 2>(a, pos, t0, drow); break;
        default: gather_body<C, 3>(a, pos, t0, drow); break;
    }
}

struct ScatterArgs {
    const float* outputs; float* preds;
    ScatterSeg seg[WUN_TRACK_ROWS];
    long long out_plane, row_floats, pred_plane;     // floats: B * Tout * C, Tout * C, pred_frames * C
    int C;
};

// d .. d + 3 of the destination plane (d 16-byte aligned; the run is [d0, d1)) from the source row at d + delta
template <int M>
__device__ __forceinline__ void scatter_body(const float* __restrict__ src, float* __restrict__ dst, long long d, long long d0,
                                             long long d1, long long delta) {
    const f32x4 v = ld4_window<M>(src, d + delta, d0 + delta, d1 + delta);
    if (d >= d0 && d + 4 <= d1) {
        *reinterpret_cast<f32x4*>(dst + d) = v;
    } else {                                          // the run's first and last granule belong to it in part only
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (d + r >= d0 && d + r < d1) dst[d + r] = v[r];
    }
}

// grid (granules of the longest run / 256, runs, sources): a lane owns one 16-byte granule of preds
__global__ __launch_bounds__(WUN_TRACK_BLOCK) void scatter_windows_kernel(ScatterArgs a) {
    const ScatterSeg sg = a.seg[blockIdx.y];
    float* dst = a.preds + (long long)blockIdx.z * a.pred_plane;
    const float* src = a.outputs + (long long)blockIdx.z * a.out_plane + (long long)sg.row * a.row_floats;
    const long long d0 = sg.dst * a.C, d1 = d0 + (long long)sg.len * a.C, delta = (long long)sg.src * a.C - d0;
    const long long d = d0 - granule_offset(dst, d0) + 4LL * ((long long)blockIdx.x * WUN_TRACK_BLOCK + threadIdx.x);
    if (d >= d1) return;
    switch (granule_offset(src, d + delta)) {         // uniform over the workgroup
        case 0: scatter_body<0>(src, dst, d, d0, d1, delta); break;
        case 1: scatter_body<1>(src, dst, d, d0, d1, delta); break;
        case 2: scatter_body<2>(src, dst, d, d0, d1, delta); break;
        default: scatter_body<3>(src, dst, d, d0, d1, delta); break;
    }
}

// (C is 1 or 2 for every plan: wun_plan_create refuses other num_channels, so launch_btc_to_ncw's general form has no
// counterpart here; pitch and the alignments are the plan's own and the entries' argument checks)
hipError_t launch_gather_windows(const MixWindows& w, float* dst, int B, int T, int C, int pitch, hipStream_t s) {
    if ((C != 1 && C != 2) || (pitch & 3) != 0 || pitch < T || (reinterpret_cast<uintptr_t>(dst) & 15) != 0 ||
        (reinterpret_cast<uintptr_t>(w.track) & 3) != 0)
        return hipErrorInvalidValue;
    for (int r0 = 0; r0 < B; r0 += WUN_TRACK_ROWS) {
        const int n = std::min(B - r0, WUN_TRACK_ROWS);
        GatherArgs a;
        a.track = w.track; a.dst = dst + (long long)r0 * C * pitch; a.T = T; a.pitch = pitch;
        for (int r = 0; r < WUN_TRACK_ROWS; ++r) a.pos[r] = (r < n && r0 + r < w.npos) ? (long long)w.pos[r0 + r] : -1;
        const dim3 grid((unsigned)((T + 4 * WUN_TRACK_BLOCK - 1) / (4 * WUN_TRACK_BLOCK)), (unsigned)n);
        prof_scope_begin("gather_windows_kernel", 0.0, s, "", 8.0 * (double)n * T * C);
        if (C == 1) hipLaunchKernelGGL(gather_windows_kernel<1>, grid, dim3(WUN_TRACK_BLOCK), 0, s, a);
        else hipLaunchKernelGGL(gather_windows_kernel<2>, grid, dim3(WUN_TRACK_BLOCK), 0, s, a);
        prof_scope_end(s);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_scatter_segments(const float* outputs, float* preds, const ScatterSeg* segs, int nsegs, int S, int B,
                                   int Tout, int C, long long pred_frames, hipStream_t s) {
    for (int k0 = 0; k0 < nsegs; k0 += WUN_TRACK_ROWS) {
        const int n = std::min(nsegs - k0, WUN_TRACK_ROWS);
        ScatterArgs a;
        a.outputs = outputs; a.preds = preds; a.C = C;
        a.out_plane = (long long)B * Tout * C; a.row_floats = (long long)Tout * C; a.pred_plane = pred_frames * C;
        int longest = 0;
        double frames = 0.0;
        for (int r = 0; r < WUN_TRACK_ROWS; ++r) {
            a.seg[r] = r < n ? segs[k0 + r] : ScatterSeg{0, 0, 0, 0};
            longest = std::max(longest, a.seg[r].len);
            frames += a.seg[r].len;
        }
        // granules a run of `longest` frames can touch: its floats / 4, plus one for a start inside a granule
        const long long granules = ((long long)longest * C + 3) / 4 + 1;
        const dim3 grid((unsigned)((granules + WUN_TRACK_BLOCK - 1) / WUN_TRACK_BLOCK), (unsigned)n, (unsigned)S);
        prof_scope_begin("scatter_windows_kernel", 0.0, s, "", 8.0 * frames * C * S);
        hipLaunchKernelGGL(scatter_windows_kernel, grid, dim3(WUN_TRACK_BLOCK), 0, s, a);
        prof_scope_end(s);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace wun

namespace {

// what the gather needs of its pointers (`who`: the entry the caller called, for the message)
int check_track_alignment(const char* who, const float* track, const float* ws) {
    if ((reinterpret_cast<uintptr_t>(track) & 3) != 0 || (reinterpret_cast<uintptr_t>(ws) & 15) != 0)
        return fail(WUN_ERR_INVALID, std::string(who) + ": the track must be 4-byte and the workspace 16-byte aligned");
    return WUN_OK;
}

int check_windows(const wun_plan* p, const float* track, int64_t track_frames, const int64_t* positions, int64_t npos,
                  const float* ws) {
    if (npos < 1 || npos > p->B) return fail(WUN_ERR_INVALID, "wun_forward_windows: npos must be in [1, batch]");
    if (track_frames < 0 || track_frames > ((int64_t)1 << 46)) return fail(WUN_ERR_INVALID, "wun_forward_windows: bad track_frames");
    for (int64_t b = 0; b < npos; ++b)
        if (positions[b] < 0 || positions[b] > track_frames - p->Tin)
            return fail(WUN_ERR_INVALID, "wun_forward_windows: window " + std::to_string(b) + " lies outside [0, track_frames]");
    return check_track_alignment("wun_forward_windows", track, ws);
}

// a host allocation that fails inside an entry is a status, not an exception through extern "C" (nothing aborts)
template <typename F> int no_throw(const char* who, F&& body) {
    try { return body(); }
    catch (const std::bad_alloc&) { g_err = std::string(who) + ": out of host memory"; return WUN_ERR_NOMEM; }
}

// The runs of preds frames each hop writes under "written last wins" (Evaluate.py:125-139): frame f belongs to the
// highest-indexed hop that covers it.  Hops are taken from the last to the first; each keeps what the later ones left.
// The covered set is re-sorted and re-merged after every hop: O(npos^2 log npos) on npos <= the plan's batch (16 by
// default) and at most 2 npos - 1 runs, a few microseconds of host time beside a forward pass.
std::vector<ScatterSeg> scatter_runs(const int64_t* positions, int64_t npos, int Tout) {
    std::vector<std::pair<long long, long long>> taken;      // disjoint, sorted [start, end)
    std::vector<ScatterSeg> segs;
    for (int64_t b = npos - 1; b >= 0; --b) {
        const long long lo = positions[b], hi = lo + Tout;
        long long cur = lo;
        for (const auto& t : taken) {
            if (t.second <= cur) continue;
            if (t.first >= hi) break;
            if (t.first > cur) segs.push_back(ScatterSeg{cur, (int)b, (int)(cur - lo), (int)(t.first - cur)});
            cur = std::max(cur, t.second);
            if (cur >= hi) break;
        }
        if (cur < hi) segs.push_back(ScatterSeg{cur, (int)b, (int)(cur - lo), (int)(hi - cur)});
        taken.emplace_back(lo, hi);
        std::sort(taken.begin(), taken.end());
        std::vector<std::pair<long long, long long>> merged;
        for (const auto& t : taken) {
            if (!merged.empty() && t.first <= merged.back().second) merged.back().second = std::max(merged.back().second, t.second);
            else merged.push_back(t);
        }
        taken.swap(merged);
    }
    return segs;
}

int check_scatter(const wun_plan* p, const int64_t* positions, int64_t npos, int64_t pred_frames) {
    if (npos < 1 || npos > p->B) return fail(WUN_ERR_INVALID, "wun_scatter_windows: npos must be in [1, batch]");
    if (pred_frames < 0 || pred_frames > ((int64_t)1 << 46)) return fail(WUN_ERR_INVALID, "wun_scatter_windows: bad pred_frames");
    for (int64_t b = 0; b < npos; ++b)
        if (positions[b] < 0 || positions[b] > pred_frames - p->Tout)
            return fail(WUN_ERR_INVALID, "wun_scatter_windows: window " + std::to_string(b) + " lies outside [0, pred_frames]");
    return WUN_OK;
}

int scatter_checked(const wun_plan* p, const float* outputs, const int64_t* positions, int64_t npos, float* preds,
                    int64_t pred_frames, hipStream_t s) {
    const std::vector<ScatterSeg> segs = scatter_runs(positions, npos, p->Tout);
    HIP_TRY(launch_scatter_segments(outputs, preds, segs.data(), (int)segs.size(), p->S, p->B, p->Tout, p->C, pred_frames, s));
    return WUN_OK;
}

}  // namespace

extern "C" int wun_forward_windows(const wun_plan* p, const float* params, const float* track_tc, int64_t track_frames,
                                   const int64_t* positions, int64_t npos, float* ws, float* outputs, int training,
                                   void* stream) {
    if (!p || !params || !track_tc || !positions || !ws || !outputs) return fail(WUN_ERR_INVALID, "null argument");
    int rc;
    if ((rc = check_windows(p, track_tc, track_frames, positions, npos, ws))) return rc;
    const MixWindows w = {track_tc, positions, (int)npos};
    return no_throw("wun_forward_windows", [&] { return forward_pass(p, params, nullptr, &w, ws, outputs, training, (hipStream_t)stream); });
}

extern "C" int wun_scatter_windows(const wun_plan* p, const float* outputs, const int64_t* positions, int64_t npos,
                                   float* preds, int64_t pred_frames, void* stream) {
    if (!p || !outputs || !positions || !preds) return fail(WUN_ERR_INVALID, "null argument");
    int rc;
    if ((rc = check_scatter(p, positions, npos, pred_frames))) return rc;
    if ((reinterpret_cast<uintptr_t>(outputs) & 3) != 0 || (reinterpret_cast<uintptr_t>(preds) & 3) != 0)
        return fail(WUN_ERR_INVALID, "wun_scatter_windows: outputs and preds must be 4-byte aligned");
    return no_throw("wun_scatter_windows", [&] { return scatter_checked(p, outputs, positions, npos, preds, pred_frames, (hipStream_t)stream); });
}

extern "C" int64_t wun_separate_positions(int64_t output_frames, int64_t n_frames, int64_t* positions, int64_t cap) {
    if (output_frames < 1 || n_frames < output_frames || n_frames > ((int64_t)1 << 46))
        return fail(WUN_ERR_INVALID, "wun_separate_positions: need 1 <= output_frames <= n_frames");
    const int64_t n = (n_frames + output_frames - 1) / output_frames;
    if (!positions) return n;
    if (cap < n) return fail(WUN_ERR_INVALID, "wun_separate_positions: cap below the number of hops");
    for (int64_t k = 0; k < n; ++k)                                  // Evaluate.py:125-128
        positions[k] = std::min(k * output_frames, n_frames - output_frames);
    return n;
}

extern "C" int wun_separate_track(const wun_plan* p, const float* params, const float* track_tc, int64_t n_frames,
                                  float* ws, float* outputs, float* preds, void* stream) {
    if (!p || !params || !track_tc || !ws || !outputs || !preds) return fail(WUN_ERR_INVALID, "null argument");
    if (n_frames < p->Tout || n_frames > ((int64_t)1 << 46))
        return fail(WUN_ERR_INVALID, "wun_separate_track: n_frames below output_frames (pad short tracks with zeros)");
    if ((p->Tin - p->Tout) % 2 != 0)
        return fail(WUN_ERR_INVALID, "wun_separate_track: input_frames - output_frames must be even (symmetric context padding)");
    int rc;
    if ((rc = check_track_alignment("wun_separate_track", track_tc, ws))) return rc;
    if ((reinterpret_cast<uintptr_t>(outputs) & 3) != 0 || (reinterpret_cast<uintptr_t>(preds) & 3) != 0)
        return fail(WUN_ERR_INVALID, "wun_separate_track: outputs and preds must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    // The hop table is built chunk by chunk (one plan's batch of positions, whatever the track's length).  Every window lies
    // inside the track by construction: the last one ends at n_frames - Tout + Tin = n_frames + 2 pad (Evaluate.py:121-122).
    // Chunk k + 1 overwrites `outputs`: its forward pass is queued on `s` behind the scatter of chunk k, which is all the
    // ordering the reuse needs (every forward pass ends with `s` waiting for the plan's side streams).
    return no_throw("wun_separate_track", [&] {
        std::vector<int64_t> pos((size_t)p->B);
        const int64_t hops = (n_frames + p->Tout - 1) / p->Tout;
        for (int64_t k = 0; k < hops; k += p->B) {
            const int n = (int)std::min<int64_t>(hops - k, p->B);
            for (int b = 0; b < n; ++b) pos[(size_t)b] = std::min((k + b) * (int64_t)p->Tout, n_frames - p->Tout);   // :125-128
            const MixWindows w = {track_tc, pos.data(), n};
            int r;
            if ((r = forward_pass(p, params, nullptr, &w, ws, outputs, 0, s))) return r;
            if ((r = scatter_checked(p, outputs, pos.data(), n, preds, n_frames, s))) return r;
        }
        return (int)WUN_OK;
    });
}
