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

struct BlendArgs {
    const float* outputs; float* preds; float* den;
    BlendRun run[WUN_TRACK_ROWS];
    long long out_plane, row_floats, pred_plane;     // floats: B * Tout * C, Tout * C, pred_frames * C
    int C, Tout, V;                                  // C is 1 or 2
};

// the trapezoid of include/wun.h at frame t of a window: one correctly rounded division of two exact integers
__device__ __forceinline__ float blend_weight(int t, int Tout, int V, unsigned flags) {
    int m = V + 1;
    if (!(flags & WUN_BLEND_NO_RISE)) m = min(m, t + 1);
    if (!(flags & WUN_BLEND_NO_FALL)) m = min(m, Tout - t);
    return __fdiv_rn((float)m, (float)(V + 1));
}

// grid (granules of the longest run / 256, runs, sources): a lane owns one 16-byte granule of preds (the accumulator) and
// walks the run's covering rows in table order; the lanes of source 0 that hold a frame's first channel own its den element
__global__ __launch_bounds__(WUN_TRACK_BLOCK) void blend_windows_kernel(BlendArgs a) {
    const BlendRun& rn = a.run[blockIdx.y];          // uniform: read from the kernel arguments where it is used
    float* dst = a.preds + (long long)blockIdx.z * a.pred_plane;
    const float* plane = a.outputs + (long long)blockIdx.z * a.out_plane;
    const long long d0 = rn.dst * a.C, d1 = d0 + (long long)rn.len * a.C;
    const long long d = d0 - granule_offset(dst, d0) + 4LL * ((long long)blockIdx.x * WUN_TRACK_BLOCK + threadIdx.x);
    if (d >= d1) return;
    const bool whole = d >= d0 && d + 4 <= d1;       // the run's first and last granule belong to it in part only
    float acc[4], dn[4];
    int tq[4];                                       // frame of float r, counted from the run's first
    bool in[4], own[4];
    if (whole) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(dst + d);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = v[r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long q = d + r - d0;
        in[r] = q >= 0 && d + r < d1;
        if (!whole) acc[r] = in[r] ? dst[d + r] : 0.f;
        tq[r] = (int)(a.C == 2 ? q >> 1 : q);
        own[r] = in[r] && blockIdx.z == 0 && (q & (a.C - 1)) == 0;
        dn[r] = own[r] ? a.den[rn.dst + tq[r]] : 0.f;
    }
    const int n = (int)(rn.meta & 7u);
#pragma unroll
    for (int j = 0; j < WUN_BLEND_COVER; ++j) {
        if (j >= n) break;
        const float* src = plane + (long long)rn.row[j] * a.row_floats;
        const long long delta = (long long)rn.t0[j] * a.C - d0;      // source float of destination float d: d + delta
        const unsigned flags = (rn.meta >> (4 + 2 * j)) & 3u;
        f32x4 x;
        switch (granule_offset(src, d + delta)) {     // uniform over the workgroup
            case 0: x = ld4_window<0>(src, d + delta, d0 + delta, d1 + delta); break;
            case 1: x = ld4_window<1>(src, d + delta, d0 + delta, d1 + delta); break;
            case 2: x = ld4_window<2>(src, d + delta, d0 + delta, d1 + delta); break;
            default: x = ld4_window<3>(src, d + delta, d0 + delta, d1 + delta); break;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float w = blend_weight(rn.t0[j] + tq[r], a.Tout, a.V, flags);
            acc[r] = __fmaf_rn(w, x[r], acc[r]);
            dn[r] = dn[r] + w;
        }
    }
    if (whole) {
        *reinterpret_cast<f32x4*>(dst + d) = (f32x4){acc[0], acc[1], acc[2], acc[3]};
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (in[r]) dst[d + r] = acc[r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (own[r]) a.den[rn.dst + tq[r]] = dn[r];
}

struct FinishArgs { float* preds; const float* den; long long plane; int C; };

__device__ __forceinline__ float blend_quotient(float acc, float den) { return den != 0.f ? __fdiv_rn(acc, den) : 0.f; }

// grid (granules of a source's plane / 256, sources): a lane owns one 16-byte granule of preds
__global__ __launch_bounds__(WUN_TRACK_BLOCK) void blend_finish_kernel(FinishArgs a) {
    float* dst = a.preds + (long long)blockIdx.y * a.plane;
    const long long d = 4LL * ((long long)blockIdx.x * WUN_TRACK_BLOCK + threadIdx.x) - granule_offset(dst, 0);
    if (d >= a.plane) return;
    if (d >= 0 && d + 4 <= a.plane) {
        f32x4 v = *reinterpret_cast<const f32x4*>(dst + d);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = blend_quotient(v[r], a.den[a.C == 2 ? (d + r) >> 1 : d + r]);
        *reinterpret_cast<f32x4*>(dst + d) = v;
    } else {                                          // a plane's first and last granule belong to it in part only
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (d + r >= 0 && d + r < a.plane) dst[d + r] = blend_quotient(dst[d + r], a.den[a.C == 2 ? (d + r) >> 1 : d + r]);
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

// (runs of one call are disjoint: one writer per preds float and per den element in every launch)
hipError_t launch_blend_runs(const float* outputs, float* preds, float* den, const BlendRun* runs, int nruns, int S, int B,
                             int Tout, int C, int overlap, long long pred_frames, hipStream_t s) {
    if (C != 1 && C != 2) return hipErrorInvalidValue;
    for (int k0 = 0; k0 < nruns; k0 += WUN_TRACK_ROWS) {
        const int n = std::min(nruns - k0, WUN_TRACK_ROWS);
        BlendArgs a;
        a.outputs = outputs; a.preds = preds; a.den = den; a.C = C; a.Tout = Tout; a.V = overlap;
        a.out_plane = (long long)B * Tout * C; a.row_floats = (long long)Tout * C; a.pred_plane = pred_frames * C;
        int longest = 0;
        double floats = 0.0;                          // moved per source: accumulator in and out, and every covering row
        for (int r = 0; r < WUN_TRACK_ROWS; ++r) {
            a.run[r] = r < n ? runs[k0 + r] : BlendRun{0, 0, 0u, {0, 0, 0, 0}, {0, 0, 0, 0}};
            longest = std::max(longest, a.run[r].len);
            floats += (double)a.run[r].len * C * (2.0 + (a.run[r].meta & 7u));
        }
        const long long granules = ((long long)longest * C + 3) / 4 + 1;
        const dim3 grid((unsigned)((granules + WUN_TRACK_BLOCK - 1) / WUN_TRACK_BLOCK), (unsigned)n, (unsigned)S);
        prof_scope_begin("blend_windows_kernel", 0.0, s, "", 4.0 * floats * S);
        hipLaunchKernelGGL(blend_windows_kernel, grid, dim3(WUN_TRACK_BLOCK), 0, s, a);
        prof_scope_end(s);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_blend_finish(float* preds, const float* den, int S, long long pred_frames, int C, hipStream_t s) {
    if (C != 1 && C != 2) return hipErrorInvalidValue;
    if (pred_frames < 1) return hipSuccess;
    const FinishArgs a = {preds, den, pred_frames * C, C};
    const long long granules = (a.plane + 3) / 4 + 1;
    const dim3 grid((unsigned)((granules + WUN_TRACK_BLOCK - 1) / WUN_TRACK_BLOCK), (unsigned)S);
    prof_scope_begin("blend_finish_kernel", 0.0, s, "", (8.0 * (double)a.plane + 4.0 * (double)pred_frames) * S);
    hipLaunchKernelGGL(blend_finish_kernel, grid, dim3(WUN_TRACK_BLOCK), 0, s, a);
    prof_scope_end(s);
    return hipGetLastError();
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

// The windows of a call, clipped to [0, pred_frames), cut at every window edge into runs of frames whose covering set is
// constant; each run carries its covering windows in table order (the caller's ascending g).  levels[k] holds covers
// WUN_BLEND_COVER k .. WUN_BLEND_COVER k + 3 of every run that has that many: level k + 1 is launched behind level k, and
// the chain of a frame passes through preds and den in memory, so where it is cut does not change its bits.  Frames no
// window covers make no run.  O(edges x windows) on the windows of one call (a plan's batch in wun_separate_track_blend).
std::vector<std::vector<BlendRun>> blend_runs(const wun_blend_window* w, int64_t nwin, int Tout, int64_t pred_frames) {
    std::vector<long long> cuts;
    for (int64_t g = 0; g < nwin; ++g) {
        const long long lo = std::max<long long>(w[g].pos, 0), hi = std::min<long long>(w[g].pos + Tout, pred_frames);
        if (lo < hi) { cuts.push_back(lo); cuts.push_back(hi); }
    }
    std::sort(cuts.begin(), cuts.end());
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    std::vector<std::vector<BlendRun>> levels;
    for (size_t c = 0; c + 1 < cuts.size(); ++c) {
        const long long f0 = cuts[c], f1 = cuts[c + 1];
        int covers = 0;
        for (int64_t g = 0; g < nwin; ++g) {
            if (w[g].pos > f0 || w[g].pos + Tout < f1) continue;       // an edge never lies inside [f0, f1): all or nothing
            const size_t level = (size_t)(covers / WUN_BLEND_COVER);
            const int j = covers % WUN_BLEND_COVER;
            if (levels.size() <= level) levels.emplace_back();
            if (j == 0) levels[level].push_back(BlendRun{f0, (int)(f1 - f0), 0u, {0, 0, 0, 0}, {0, 0, 0, 0}});
            BlendRun& r = levels[level].back();
            r.row[j] = w[g].row;
            r.t0[j] = (int)(f0 - w[g].pos);
            r.meta = (r.meta & ~7u) + (unsigned)(j + 1);
            r.meta |= ((unsigned)w[g].flags & 3u) << (4 + 2 * j);
            ++covers;
        }
    }
    return levels;
}

int check_blend(const char* who, int64_t S, int64_t B, int64_t Tout, int64_t C, const wun_blend_window* w, int64_t nwin,
                int64_t overlap, int64_t pred_frames) {
    const std::string me(who);
    if (S < 1 || S > 65535 || B < 1 || B > ((int64_t)1 << 30) || Tout < 1 || Tout > ((int64_t)1 << 30))
        return fail(WUN_ERR_INVALID, me + ": need 1 <= S <= 65535 and 1 <= B, Tout <= 2^30");
    if (C != 1 && C != 2) return fail(WUN_ERR_INVALID, me + ": C must be 1 or 2");
    if (overlap < 0 || overlap > Tout - 1) return fail(WUN_ERR_INVALID, me + ": overlap_frames must be in [0, Tout - 1]");
    if (pred_frames < 0 || pred_frames > ((int64_t)1 << 46)) return fail(WUN_ERR_INVALID, me + ": bad pred_frames");
    if (nwin < 1 || nwin > ((int64_t)1 << 24)) return fail(WUN_ERR_INVALID, me + ": nwin must be in [1, 2^24]");
    for (int64_t g = 0; g < nwin; ++g) {
        if (w[g].row < 0 || w[g].row >= B)
            return fail(WUN_ERR_INVALID, me + ": window " + std::to_string(g) + " names a row outside [0, B)");
        if (w[g].pos < -((int64_t)1 << 46) || w[g].pos > ((int64_t)1 << 46))
            return fail(WUN_ERR_INVALID, me + ": window " + std::to_string(g) + " has a position beyond 2^46");
        if ((w[g].flags & ~(WUN_BLEND_NO_RISE | WUN_BLEND_NO_FALL)) != 0)
            return fail(WUN_ERR_INVALID, me + ": window " + std::to_string(g) + " has unknown flag bits");
    }
    return WUN_OK;
}

int blend_checked(const float* outputs, int S, int B, int Tout, int C, const wun_blend_window* w, int64_t nwin, int overlap,
                  float* preds, float* den, int64_t pred_frames, hipStream_t s) {
    const std::vector<std::vector<BlendRun>> levels = blend_runs(w, nwin, Tout, pred_frames);
    for (const auto& runs : levels)
        HIP_TRY(launch_blend_runs(outputs, preds, den, runs.data(), (int)runs.size(), S, B, Tout, C, overlap, pred_frames, s));
    return WUN_OK;
}

// one pass of wun_blend_positions: K, or a negative status
int64_t blend_pass(const char* who, int64_t Tout, int64_t n_frames, int64_t overlap, int64_t shift) {
    const std::string me(who);
    if (Tout < 1 || Tout > ((int64_t)1 << 30) || n_frames < 1 || n_frames > ((int64_t)1 << 46))
        return fail(WUN_ERR_INVALID, me + ": need 1 <= output_frames <= 2^30 and 1 <= n_frames <= 2^46");
    if (overlap < 0 || overlap > Tout - 1) return fail(WUN_ERR_INVALID, me + ": overlap_frames must be in [0, output_frames - 1]");
    if (shift < 0 || shift > ((int64_t)1 << 46)) return fail(WUN_ERR_INVALID, me + ": a shift must be in [0, 2^46]");
    const int64_t H = Tout - overlap, over = std::max<int64_t>(0, n_frames + shift - Tout), K = 1 + (over + H - 1) / H;
    if (K > ((int64_t)1 << 30)) return fail(WUN_ERR_INVALID, me + ": more than 2^30 windows in a pass");
    return K;
}

}  // namespace

extern "C" int32_t wun_blend_abi_size(void) { return (int32_t)sizeof(wun_blend_window); }

extern "C" int64_t wun_blend_positions(int64_t output_frames, int64_t n_frames, int64_t overlap_frames, int64_t shift,
                                       wun_blend_window* windows, int64_t cap) {
    const int64_t K = blend_pass("wun_blend_positions", output_frames, n_frames, overlap_frames, shift);
    if (K < 0 || !windows) return K;
    if (cap < K) return fail(WUN_ERR_INVALID, "wun_blend_positions: cap below the number of windows");
    const int64_t H = output_frames - overlap_frames;
    for (int64_t k = 0; k < K; ++k)
        windows[k] = wun_blend_window{k * H - shift, (int32_t)k,
                                      (k == 0 ? WUN_BLEND_NO_RISE : 0) | (k == K - 1 ? WUN_BLEND_NO_FALL : 0)};
    return K;
}

extern "C" int wun_blend_windows(const float* outputs, int64_t S, int64_t B, int64_t Tout, int64_t C,
                                 const wun_blend_window* windows, int64_t nwin, int64_t overlap_frames, float* preds,
                                 float* den, int64_t pred_frames, void* stream) {
    if (!outputs || !windows || !preds || !den) return fail(WUN_ERR_INVALID, "null argument");
    int rc;
    if ((rc = check_blend("wun_blend_windows", S, B, Tout, C, windows, nwin, overlap_frames, pred_frames))) return rc;
    if (((reinterpret_cast<uintptr_t>(outputs) | reinterpret_cast<uintptr_t>(preds) | reinterpret_cast<uintptr_t>(den)) & 3) != 0)
        return fail(WUN_ERR_INVALID, "wun_blend_windows: outputs, preds and den must be 4-byte aligned");
    return no_throw("wun_blend_windows", [&] {
        return blend_checked(outputs, (int)S, (int)B, (int)Tout, (int)C, windows, nwin, (int)overlap_frames, preds, den,
                             pred_frames, (hipStream_t)stream);
    });
}

extern "C" int wun_blend_finish(float* preds, const float* den, int64_t S, int64_t pred_frames, int64_t C, void* stream) {
    if (!preds || !den) return fail(WUN_ERR_INVALID, "null argument");
    if (S < 1 || S > 65535 || (C != 1 && C != 2) || pred_frames < 0 || pred_frames > ((int64_t)1 << 46))
        return fail(WUN_ERR_INVALID, "wun_blend_finish: need 1 <= S <= 65535, C of 1 or 2 and 0 <= pred_frames <= 2^46");
    if (((reinterpret_cast<uintptr_t>(preds) | reinterpret_cast<uintptr_t>(den)) & 3) != 0)
        return fail(WUN_ERR_INVALID, "wun_blend_finish: preds and den must be 4-byte aligned");
    HIP_TRY(launch_blend_finish(preds, den, (int)S, pred_frames, (int)C, (hipStream_t)stream));
    return WUN_OK;
}

extern "C" int wun_separate_track_blend(const wun_plan* p, const float* params, const float* track_tc, int64_t track_frames,
                                        int64_t lead, int64_t n_frames, int64_t overlap_frames, const int64_t* shifts,
                                        int64_t nshifts, float* ws, float* outputs, float* preds, float* den, void* stream) {
    if (!p || !params || !track_tc || !shifts || !ws || !outputs || !preds || !den) return fail(WUN_ERR_INVALID, "null argument");
    const char* me = "wun_separate_track_blend";
    if (nshifts < 1 || nshifts > 4096) return fail(WUN_ERR_INVALID, std::string(me) + ": nshifts must be in [1, 4096]");
    if ((p->Tin - p->Tout) % 2 != 0)
        return fail(WUN_ERR_INVALID, std::string(me) + ": input_frames - output_frames must be even (symmetric context padding)");
    if (lead < 0 || track_frames < 0 || track_frames > ((int64_t)1 << 47))
        return fail(WUN_ERR_INVALID, std::string(me) + ": bad lead or track_frames");
    const int64_t H = p->Tout - overlap_frames;
    int64_t total = 0;
    for (int64_t i = 0; i < nshifts; ++i) {           // a pass's windows ascend: its first and its last bound the rest
        const int64_t K = blend_pass(me, p->Tout, n_frames, overlap_frames, shifts[i]);
        if (K < 0) return (int)K;
        const int64_t first = lead - shifts[i], last = lead + (K - 1) * H - shifts[i];
        if (first < 0 || last + p->Tin > track_frames)
            return fail(WUN_ERR_INVALID, std::string(me) + ": window " + std::to_string(first < 0 ? 0 : K - 1) + " of pass " +
                        std::to_string(i) + " lies outside [0, track_frames] (lead >= every shift, and zeros behind the track for "
                        "the overhanging last hop)");
        total += K;
    }
    if (total > ((int64_t)1 << 30)) return fail(WUN_ERR_INVALID, std::string(me) + ": more than 2^30 windows");
    int rc;
    if ((rc = check_track_alignment(me, track_tc, ws))) return rc;
    if (((reinterpret_cast<uintptr_t>(outputs) | reinterpret_cast<uintptr_t>(preds) | reinterpret_cast<uintptr_t>(den)) & 3) != 0)
        return fail(WUN_ERR_INVALID, std::string(me) + ": outputs, preds and den must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    // The window list is the passes one behind the other; chunks of the plan's batch run across pass boundaries.  Chunk
    // k + 1 overwrites `outputs` behind the blend of chunk k: stream order, as in wun_separate_track.
    return no_throw(me, [&] {
        std::vector<wun_blend_window> win((size_t)total);
        int64_t g = 0;
        for (int64_t i = 0; i < nshifts; ++i)
            g += wun_blend_positions(p->Tout, n_frames, overlap_frames, shifts[i], win.data() + g, total - g);
        HIP_TRY(hipMemsetAsync(preds, 0, sizeof(float) * (size_t)p->S * (size_t)n_frames * (size_t)p->C, s));
        HIP_TRY(hipMemsetAsync(den, 0, sizeof(float) * (size_t)n_frames, s));
        std::vector<int64_t> pos((size_t)p->B);
        std::vector<wun_blend_window> chunk((size_t)p->B);
        for (int64_t k = 0; k < total; k += p->B) {
            const int n = (int)std::min<int64_t>(total - k, p->B);
            for (int b = 0; b < n; ++b) {
                chunk[(size_t)b] = win[(size_t)(k + b)];
                chunk[(size_t)b].row = b;
                pos[(size_t)b] = lead + chunk[(size_t)b].pos;
            }
            const MixWindows w = {track_tc, pos.data(), n};
            int r;
            if ((r = forward_pass(p, params, nullptr, &w, ws, outputs, 0, s))) return r;
            if ((r = blend_checked(outputs, p->S, p->B, p->Tout, p->C, chunk.data(), n, (int)overlap_frames, preds, den,
                                   n_frames, s))) return r;
        }
        HIP_TRY(launch_blend_finish(preds, den, p->S, n_frames, p->C, s));
        return (int)WUN_OK;
    });
}

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
