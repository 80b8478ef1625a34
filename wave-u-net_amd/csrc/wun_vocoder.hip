// gfx950 (MI355X / CDNA4): the phase vocoder behind the C ABI (include/wun.h: wun_time_stretch) -- a table of jobs,
// each one span of interleaved audio stretched to its own tempo ratio num / den at constant pitch.  One launch set per
// WUN_STRETCH_JOBS jobs is four launches whatever the job count:
//
//   voc_analysis_kernel   (wun_fft.hip) per synthesis frame f the transforms of the span at a_f = (f hop num) / den and one hop
//                         before it, in one workgroup; |X_f| and the phase increment (turns, float32) go to scratch
//   voc_phase_kernel      a lane owns one (job, channel, bin): it walks f ascending with the float64 phase accumulator and
//                         overwrites |X_f| with Re Y_f and the increment with Im Y_f at its own element
//   istft_fft_kernel      (wun_fft.hip) the inverse transform of every frame row, windowed, into scratch
//   voc_ola_kernel        one lane per output float: the covering frames in ascending f over their float64 window squares
//
// The job table travels by value in the kernel arguments (VocArgs, wun_fft.h): no host-to-device copy, no allocation, no
// synchronisation, no atomics; every float of scratch that is read was written by the same launch set.  A job's frame rows,
// lanes and LDS regions are its own and every kernel runs one instruction sequence per element, so its floats do not depend on
// the other jobs, its place in the table, the launch set, the grid or alignment.  All index arithmetic is 64-bit.
//
// Built WITHOUT the packed fp32 VALU instructions like the other shared units (csrc/Makefile NO_PK_FP32).  The
// entry's argument checks run before any GPU work.
#include "wun_fft.h"
#include "../../include/wun.h"

#include <algorithm>
#include <cmath>
#include <string>

int fail(int code, const std::string& msg);      // wun_plan.hip

#define WUN_VOC_BLOCK 256

namespace wun {

// grid (bins / 256, job rows of the set: j C + c).  Phi_0 = Delta_0, Phi_f = Phi_{f-1} + (adv + Delta_f), adv = ((k hop) mod N) / N
// (dyadic: exact); Y_f = |X_f| (cos, sin)(2 pi Phi_f), the angle reduced exactly by sincospi.  Reads and writes are the lane's
// own elements, coalesced over k.
__global__ __launch_bounds__(WUN_VOC_BLOCK) void voc_phase_kernel(VocArgs p) {
    const int k = blockIdx.x * WUN_VOC_BLOCK + threadIdx.x;
    if (k >= p.K) return;
    const int j = blockIdx.y / p.C, c = blockIdx.y - j * p.C;
    const long long F = p.fp[j + 1] - p.fp[j];
    const long long e0 = (p.C * p.fp[j] + c * F) * p.K + k;
    const double adv = (double)((k * p.hop) & (p.n_fft - 1)) / (double)p.n_fft;
    const bool edge = k == 0 || k == p.K - 1;
    double phi = 0.0;
    for (long long f = 0; f < F; ++f) {                      // ascending f: the one accumulation order
        const long long e = e0 + f * p.K;
        const float m = p.mag[e];
        const double d = (double)p.dlt[e];
        phi = f == 0 ? d : phi + (adv + d);
        double sn, cs;
        sincospi(2.0 * phi, &sn, &cs);
        p.mag[e] = m * (float)cs;
        p.dlt[e] = edge ? 0.f : m * (float)sn;
    }
}

// grid (capped, jobs of the set), grid-stride over the job's n_out C floats: one writer per float.  istft_ola_kernel's rule:
// the frames that cover the sample in ascending f over the float64 window squares of the same frames (cospi: the argument is
// exact), 0 where those sum to less than 1e-8.
__global__ __launch_bounds__(WUN_VOC_BLOCK) void voc_ola_kernel(VocArgs p, const float* __restrict__ frames) {
    const int j = blockIdx.y;
    const wun_stretch_job jb = p.job[j];
    const long long F = p.fp[j + 1] - p.fp[j];
    const long long n = (long long)jb.n_out * p.C;
    const int N = p.n_fft, lead = p.n_fft - p.hop;
    for (long long e = (long long)blockIdx.x * WUN_VOC_BLOCK + threadIdx.x; e < n; e += (long long)gridDim.x * WUN_VOC_BLOCK) {
        const long long t = e / p.C, c = e - t * p.C, u = t + lead;      // u - f hop is the sample's place in frame f
        const long long f_lo = u >= N ? (u - N) / p.hop + 1 : 0;
        long long f_hi = u / p.hop;
        if (f_hi > F - 1) f_hi = F - 1;
        const float* __restrict__ fr = frames + (p.C * p.fp[j] + c * F) * N;
        float a = 0.f;
        double ws = 0.0;
        for (long long f = f_lo; f <= f_hi; ++f) {
            const long long m = u - f * p.hop;
            a += fr[f * N + m];
            const double w = 0.5 - 0.5 * cospi(2.0 * (double)m / (double)N);
            ws += w * w;
        }
        jb.y[e] = ws < 1e-8 ? 0.f : a / (float)ws;
    }
}

namespace {

int gcd_i(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

// a tempo ratio: positive and coprime (WUN_ERR_INVALID); within the ceiling and [1/2, 2] (WUN_ERR_UNSUPPORTED).  1/1 is legal.
int check_ratio(const std::string& who, int32_t num, int32_t den) {
    if (num <= 0 || den <= 0) return fail(WUN_ERR_INVALID, who + ": num and den must be positive");
    if (gcd_i(num, den) != 1) return fail(WUN_ERR_INVALID, who + ": num / den must be coprime (reduced by their gcd)");
    if (num > WUN_SPEED_MAX_RATIO || den > WUN_SPEED_MAX_RATIO)
        return fail(WUN_ERR_UNSUPPORTED, who + ": max(num, den) above the ceiling of 64");
    if (num > 2 * den || den > 2 * num) return fail(WUN_ERR_UNSUPPORTED, who + ": the tempo num / den lies outside [1/2, 2]");
    return WUN_OK;
}

// n_fft (UNSUPPORTED, as the FFT entries), then hop, C and J (INVALID)
int check_res(const std::string& who, const wun_stretch_job* jobs, int32_t J, int32_t C, int32_t n_fft, int32_t hop) {
    if (!jobs) return fail(WUN_ERR_INVALID, who + ": null argument");
    if (J < 1) return fail(WUN_ERR_INVALID, who + ": J < 1");
    if (C != 1 && C != 2) return fail(WUN_ERR_INVALID, who + ": C must be 1 or 2");
    if (n_fft < 64 || n_fft > 8192 || (n_fft & (n_fft - 1)))
        return fail(WUN_ERR_UNSUPPORTED, who + ": n_fft must be a power of two in 64..8192");
    if (hop < 1 || (hop & (hop - 1)) || hop > n_fft / 4)
        return fail(WUN_ERR_INVALID, who + ": hop must be a power of two, at most n_fft / 4");
    return WUN_OK;
}

long long centered_frames(long long T, int n_fft, int hop) { return (T + (n_fft - hop) + hop - 1) / hop; }

// frame rows of the launch set that starts at job j0 (n_out checked by the caller)
long long set_rows(const wun_stretch_job* jobs, int32_t J, int j0, int32_t C, int32_t n_fft, int32_t hop) {
    long long rows = 0;
    for (int j = j0; j < std::min<long long>(J, (long long)j0 + WUN_STRETCH_JOBS); ++j) rows += C * centered_frames(jobs[j].n_out, n_fft, hop);
    return rows;
}

}  // namespace
}  // namespace wun

extern "C" int32_t wun_stretch_abi_size(void) { return (int32_t)sizeof(wun_stretch_job); }

extern "C" int64_t wun_time_stretch_frames(int64_t n_in, int32_t num, int32_t den) {
    const std::string who = "wun_time_stretch_frames";
    if (n_in < 1 || n_in > ((int64_t)1 << 40)) return fail(WUN_ERR_INVALID, who + ": n_in must be in 1..2^40");
    int rc;
    if ((rc = wun::check_ratio(who, num, den))) return rc;
    return (n_in * den + num - 1) / num;
}

extern "C" int64_t wun_time_stretch_scratch_floats(const wun_stretch_job* jobs, int32_t J, int32_t C, int32_t n_fft, int32_t hop) {
    using namespace wun;
    const std::string who = "wun_time_stretch_scratch_floats";
    int rc;
    if ((rc = check_res(who, jobs, J, C, n_fft, hop))) return rc;
    for (int j = 0; j < J; ++j)
        if (jobs[j].n_out < 1) return fail(WUN_ERR_INVALID, who + ": job " + std::to_string(j) + ": n_out < 1");
    // the launch sets follow one another on the stream and share the scratch: |X| and the increment [rows][K], the frames [rows][n_fft]
    long long rows = 0;
    for (int j0 = 0; j0 < J; j0 += WUN_STRETCH_JOBS) rows = std::max(rows, set_rows(jobs, J, j0, C, n_fft, hop));
    return rows * (2 * (long long)(n_fft / 2 + 1) + n_fft);
}

extern "C" int wun_time_stretch(const wun_stretch_job* jobs, int32_t J, int32_t C, int32_t n_fft, int32_t hop,
                                const float* table_dev, float* scratch, void* stream) {
    using namespace wun;
    const std::string who = "wun_time_stretch";
    int rc;
    if ((rc = check_res(who, jobs, J, C, n_fft, hop))) return rc;
    if (!table_dev || !scratch) return fail(WUN_ERR_INVALID, who + ": null argument");
    if (((reinterpret_cast<uintptr_t>(table_dev) | reinterpret_cast<uintptr_t>(scratch)) & 3) != 0)
        return fail(WUN_ERR_INVALID, who + ": the table and the scratch must be 4-byte aligned");
    for (int j = 0; j < J; ++j) {
        const wun_stretch_job& b = jobs[j];
        const std::string wj = who + ": job " + std::to_string(j);
        if (!b.x || !b.y) return fail(WUN_ERR_INVALID, wj + ": null argument");
        if (((reinterpret_cast<uintptr_t>(b.x) | reinterpret_cast<uintptr_t>(b.y)) & 3) != 0)
            return fail(WUN_ERR_INVALID, wj + ": x and y must be 4-byte aligned");
        if (b.n_in < 1) return fail(WUN_ERR_INVALID, wj + ": n_in < 1");
        if ((rc = check_ratio(wj, b.num, b.den))) return rc;
        if (b.n_out < 1 || b.n_out > ((long long)b.n_in * b.den + b.num - 1) / b.num)
            return fail(WUN_ERR_INVALID, wj + ": n_out outside 1..wun_time_stretch_frames");
    }
    // no output may lie over an input: a later launch set would read what an earlier one wrote
    for (int j = 0; j < J; ++j) {
        const uintptr_t y0 = reinterpret_cast<uintptr_t>(jobs[j].y), y1 = y0 + 4ull * jobs[j].n_out * C;
        for (int i = 0; i < J; ++i) {
            const uintptr_t x0 = reinterpret_cast<uintptr_t>(jobs[i].x), x1 = x0 + 4ull * jobs[i].n_in * C;
            if (y0 < x1 && x0 < y1)
                return fail(WUN_ERR_INVALID, who + ": y of job " + std::to_string(j) + " overlaps x of job " + std::to_string(i));
        }
    }
    const int fpw = fft_frames_per_workgroup(n_fft), K = n_fft / 2 + 1;
    for (int j0 = 0; j0 < J; j0 += WUN_STRETCH_JOBS) {
        long long groups = 0;
        for (int j = j0; j < std::min<long long>(J, (long long)j0 + WUN_STRETCH_JOBS); ++j)
            groups += C * ((centered_frames(jobs[j].n_out, n_fft, hop) + fpw - 1) / fpw);
        if (groups > 0x7fffffffLL || set_rows(jobs, J, j0, C, n_fft, hop) > 0x7fffffffLL)
            return fail(WUN_ERR_UNSUPPORTED, who + ": more than 2^31 - 1 frame rows in one launch set");
    }
    hipStream_t st = (hipStream_t)stream;
    for (int j0 = 0; j0 < J; j0 += WUN_STRETCH_JOBS) {
        const int n = std::min(J - j0, WUN_STRETCH_JOBS);
        VocArgs v;
        long long max_out = 0;
        v.fp[0] = 0; v.gp[0] = 0;
        for (int j = 0; j < WUN_STRETCH_JOBS; ++j) {
            v.job[j] = j < n ? jobs[j0 + j] : wun_stretch_job{nullptr, nullptr, 0, 0, 1, 1};
            const long long F = j < n ? centered_frames(jobs[j0 + j].n_out, n_fft, hop) : 0;
            v.fp[j + 1] = v.fp[j] + F;
            v.gp[j + 1] = v.gp[j] + C * ((F + fpw - 1) / fpw);
            max_out = std::max(max_out, (long long)v.job[j].n_out * C);
        }
        const long long rows = C * v.fp[n];
        v.table = table_dev;
        v.mag = scratch; v.dlt = scratch + rows * K;
        float* frames = scratch + 2 * rows * K;
        v.J = n; v.C = C; v.n_fft = n_fft; v.hop = hop; v.K = K;
        const double logn = std::log2((double)n_fft);
        prof_scope_begin("voc_analysis_kernel", 2.0 * rows * (2.5 * n_fft * logn), st, "", 4.0 * rows * (2.0 * n_fft + 2.0 * K));
        if ((rc = fft_launch_voc_analysis(v, st))) return rc;
        prof_scope_end(st);
        prof_scope_begin("voc_phase_kernel", 0.0, st, "", 16.0 * rows * K);
        hipLaunchKernelGGL(voc_phase_kernel, dim3((unsigned)((K + WUN_VOC_BLOCK - 1) / WUN_VOC_BLOCK), (unsigned)(n * C)), dim3(WUN_VOC_BLOCK), 0, st, v);
        prof_scope_end(st);
        IstftGemmArgs g;
        g.re = v.mag; g.im = v.dlt; g.table = table_dev; g.frames = frames;
        g.M = rows; g.nb = rows; g.fstride = rows; g.foff = 0;
        g.n_fft = n_fft; g.K = K; g.c_edge = 1.0f / (float)n_fft; g.c_mid = 2.0f / (float)n_fft;
        prof_scope_begin("istft_fft_kernel", rows * (2.5 * n_fft * logn), st, "", 4.0 * rows * (2.0 * K + n_fft));
        if ((rc = fft_launch_inverse(g, st))) return rc;
        prof_scope_end(st);
        long long grid = (max_out + WUN_VOC_BLOCK - 1) / WUN_VOC_BLOCK;
        if (grid > (1 << 16)) grid = 1 << 16;
        prof_scope_begin("voc_ola_kernel", 0.0, st, "", 4.0 * rows * n_fft);
        hipLaunchKernelGGL(voc_ola_kernel, dim3((unsigned)grid, (unsigned)n), dim3(WUN_VOC_BLOCK), 0, st, v, (const float*)frames);
        prof_scope_end(st);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(WUN_ERR_HIP, who + " launch: " + hipGetErrorString(e));
    }
    return WUN_OK;
}
