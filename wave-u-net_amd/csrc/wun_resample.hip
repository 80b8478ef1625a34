// gfx950 (MI355X / CDNA4): rational polyphase resampler of the audio boundary (include/wun.h: wun_resample*) -- what the
// reference does with librosa on the way into and out of Evaluate.predict (Evaluate.py:59-67,104; Utils.py:94-95).
//
//   y[n] = sum_m v[m] * h[n*down - m*up + half],   v = the channel-mapped input, zero outside [0, n_in)
//
// h is scipy.signal.resample_poly's default filter: 2*half + 1 taps, half = 10*max(up, down), windowed sinc with cutoff
// 1/max(up, down) of Nyquist, Kaiser window beta = 5, unit DC gain, times up.  It is designed on the host in float64 and
// handed to the kernel as fp32 in PHASE-MAJOR order: output n uses row p = (n*down + half) % up,
//   taps[p][k] = h[p + k*up],  k < K = ceil((2*half + 1) / up)  (rows zero-padded to K),
//   y[n] = sum_k taps[p][k] * v[q - k],  q = (n*down + half) / up,
// accumulated with one fp32 FMA per tap, k ascending: bit-reproducible, independent of grid and alignment.
//
// Built WITHOUT the packed fp32 VALU instructions like wun_elementwise.hip (csrc/Makefile NO_PK_FP32): a
// track can be resampled while another stream runs bf16 MFMA waves on the same CUs.  The C ABI of the resampler lives in
// this unit too; its argument checks run before any GPU work.
#include "wun_device.h"
#include "../../include/wun.h"

#include <cmath>
#include <vector>

using namespace wun;
int fail(int code, const std::string& msg);      // wun_plan.hip: sets wun_last_error(), returns code

#define WUN_RESAMPLE_MAX_RATIO 16384     // ceiling on max(up, down): 44 100 -> 8 192 Hz needs 11 025
#define WUN_RESAMPLE_BLOCK 256           // output frames per workgroup, one per lane
#define WUN_RESAMPLE_LDS_FLOATS 16384    // 64 KB: input window (+ the table when it is small)
#define WUN_RESAMPLE_TAB_LDS 1024        // tables up to this many floats are staged in LDS (up = 1: the one shared row)
#define WUN_RESAMPLE_MAX_CH 8            // most input channels of a downmix

namespace wun {      // the kernels carry the library's wun:: prefix in profiler output

struct ResampleArgs {
    const float* x; float* y; const float* taps;
    long long n_in, n_out, y_offset;
    int c_in, c_out, up, down, half, K;
    int y_vec2;                             // c_out == 2 and y is 8-byte aligned: one 8-byte store per frame
};

// the three channel mappings: c_in == c_out (CL = c_in, per channel), c_out == 1 (CL = 1: the mean of the input
// channels -- sequential fp32 sum, one divide: np.mean(axis=1)), c_in == 1 && c_out == 2 (CL = 1, duplicated on store)
__device__ __forceinline__ float downmix_frame(const float* __restrict__ x, long long m, int c_in) {
    float s = x[m * c_in];
    for (int c = 1; c < c_in; ++c) s += x[m * c_in + c];
    return c_in > 1 ? s / (float)c_in : s;
}

template <int CL>
__device__ __forceinline__ void store_frame(const ResampleArgs& a, long long n, const float* acc) {
    float* dst = a.y + (a.y_offset + n) * a.c_out;
    if (CL == 2) {
        if (a.y_vec2) *reinterpret_cast<f32x2*>(dst) = (f32x2){acc[0], acc[1]};
        else { dst[0] = acc[0]; dst[1] = acc[1]; }
    } else if (a.c_out == 2) {
        if (a.y_vec2) *reinterpret_cast<f32x2*>(dst) = (f32x2){acc[0], acc[0]};
        else { dst[0] = acc[0]; dst[1] = acc[0]; }
    } else {
        dst[0] = acc[0];
    }
}

// One output frame per lane, all channels.  The workgroup's outputs n0 .. n0 + 255 read the input frames
// m_lo = q(n0) - (K - 1) .. q(n0 + 255): staged once in LDS (channel-mapped, zero outside the signal), then every lane
// walks its tap row.  TAB_LDS: the whole table sits in LDS behind the window.
template <int CL, bool TAB_LDS>
__global__ __launch_bounds__(WUN_RESAMPLE_BLOCK) void resample_kernel(ResampleArgs a) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const long long n0 = (long long)blockIdx.x * WUN_RESAMPLE_BLOCK;
    const long long base = n0 * a.down + a.half;             // wave-uniform 64-bit part of n*down + half
    const long long qb = base / a.up;
    const unsigned rb = (unsigned)(base % a.up);
    const int nb = (int)((a.n_out - n0) < WUN_RESAMPLE_BLOCK ? (a.n_out - n0) : WUN_RESAMPLE_BLOCK);
    const long long m_lo = qb - (a.K - 1);
    const int W = (int)((rb + (unsigned)(nb - 1) * (unsigned)a.down) / (unsigned)a.up) + a.K;    // frames of the window

    if (a.c_in == CL) {                                      // per channel: a linear, coalesced copy
        for (int i = tid; i < W * CL; i += WUN_RESAMPLE_BLOCK) {
            const long long m = m_lo + i / CL;
            lds[i] = (m >= 0 && m < a.n_in) ? a.x[m_lo * CL + i] : 0.f;
        }
    } else {                                                 // downmix to one channel
        for (int j = tid; j < W; j += WUN_RESAMPLE_BLOCK) {
            const long long m = m_lo + j;
            lds[j] = (m >= 0 && m < a.n_in) ? downmix_frame(a.x, m, a.c_in) : 0.f;
        }
    }
    float* tab = lds + W * CL;
    if (TAB_LDS)
        for (int i = tid; i < a.up * a.K; i += WUN_RESAMPLE_BLOCK) tab[i] = a.taps[i];
    __syncthreads();
    if (tid >= nb) return;

    const unsigned t = rb + (unsigned)tid * (unsigned)a.down;    // < 2^31: up, down <= WUN_RESAMPLE_MAX_RATIO
    const int j0 = (int)(t / (unsigned)a.up) + a.K - 1;          // window index of v[q]
    const int p = (int)(t % (unsigned)a.up);
    const float* row = (TAB_LDS ? tab : a.taps) + (long long)p * a.K;
    float acc[CL];
#pragma unroll
    for (int c = 0; c < CL; ++c) acc[c] = 0.f;
    for (int k = 0; k < a.K; ++k) {                              // k ascending: the one accumulation order
        const float h = row[k];
#pragma unroll
        for (int c = 0; c < CL; ++c) acc[c] = fmaf(h, lds[(j0 - k) * CL + c], acc[c]);
    }
    store_frame<CL>(a, n0 + tid, acc);
}

// up == down: the channel-mapped input itself
template <int CL>
__global__ __launch_bounds__(WUN_RESAMPLE_BLOCK) void resample_copy_kernel(ResampleArgs a) {
    const long long n = (long long)blockIdx.x * WUN_RESAMPLE_BLOCK + threadIdx.x;
    if (n >= a.n_out) return;
    float v[CL];
    if (a.c_in == CL) {
#pragma unroll
        for (int c = 0; c < CL; ++c) v[c] = a.x[n * CL + c];
    } else {
        v[0] = downmix_frame(a.x, n, a.c_in);
    }
    store_frame<CL>(a, n, v);
}

}  // namespace wun

namespace {

int gcd_i(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

// Bessel I0 by its power series, sum ((x/2)^2k / (k!)^2): the terms fall below 1e-17 of the sum within 40 for x <= 5
double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// the 2*half + 1 taps of scipy.signal.firwin(2*half + 1, 1/max(up, down), window=("kaiser", 5.0)) * up, float64
std::vector<double> design_filter(int up, int down) {
    const int mx = up > down ? up : down, half = 10 * mx, n = 2 * half + 1;
    std::vector<double> h((size_t)n);
    if (mx == 1) {                        // cutoff at Nyquist: sinc at the integers, a unit impulse
        h[(size_t)half] = 1.0;
        return h;
    }
    const double fc = 1.0 / (double)mx, beta = 5.0, i0b = bessel_i0(beta), pi = 3.14159265358979323846;
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        const double m = (double)(i - half), r = m / (double)half;
        const double arg = pi * fc * m;
        const double sinc = (i == half) ? 1.0 : sin(arg) / arg;
        const double win = bessel_i0(beta * sqrt(1.0 - r * r)) / i0b;
        h[(size_t)i] = fc * sinc * win;
        sum += h[(size_t)i];
    }
    for (int i = 0; i < n; ++i) h[(size_t)i] = h[(size_t)i] / sum * (double)up;
    return h;
}

int check_ratio(int32_t up, int32_t down) {
    if (up <= 0 || down <= 0) return fail(WUN_ERR_INVALID, "wun_resample: up and down must be positive");
    if (gcd_i(up, down) != 1) return fail(WUN_ERR_INVALID, "wun_resample: up / down must be reduced by their gcd (wun_resample_ratio)");
    if (up > WUN_RESAMPLE_MAX_RATIO || down > WUN_RESAMPLE_MAX_RATIO)
        return fail(WUN_ERR_UNSUPPORTED, "wun_resample: max(up, down) above 16384");
    return WUN_OK;
}

int taps_per_row(int up, int down) {
    const int mx = up > down ? up : down;
    return (20 * mx + 1 + up - 1) / up;
}

}  // namespace

extern "C" int wun_resample_ratio(int32_t sr_in, int32_t sr_out, int32_t* up, int32_t* down) {
    if (!up || !down) return fail(WUN_ERR_INVALID, "null argument");
    if (sr_in <= 0 || sr_out <= 0) return fail(WUN_ERR_INVALID, "wun_resample_ratio: sample rates must be positive");
    const int g = gcd_i(sr_in, sr_out);
    *up = sr_out / g;
    *down = sr_in / g;
    if (*up > WUN_RESAMPLE_MAX_RATIO || *down > WUN_RESAMPLE_MAX_RATIO)
        return fail(WUN_ERR_UNSUPPORTED, "wun_resample_ratio: max(up, down) above 16384 after reduction");
    return WUN_OK;
}

extern "C" int64_t wun_resample_frames(int64_t n_in, int32_t up, int32_t down) {
    if (n_in < 0) return fail(WUN_ERR_INVALID, "wun_resample_frames: negative length");
    if (n_in > ((int64_t)1 << 46)) return fail(WUN_ERR_INVALID, "wun_resample_frames: length above 2^46");
    int rc;
    if ((rc = check_ratio(up, down))) return rc;
    return (n_in * up + down - 1) / down;
}

extern "C" int64_t wun_resample_table_floats(int32_t up, int32_t down) {
    int rc;
    if ((rc = check_ratio(up, down))) return rc;
    return (int64_t)up * taps_per_row(up, down);
}

extern "C" int wun_resample_design(int32_t up, int32_t down, float* table_host, int64_t cap) {
    int rc;
    if ((rc = check_ratio(up, down))) return rc;
    if (!table_host) return fail(WUN_ERR_INVALID, "null argument");
    const int K = taps_per_row(up, down);
    if (cap < (int64_t)up * K) return fail(WUN_ERR_INVALID, "wun_resample_design: cap below wun_resample_table_floats");
    const std::vector<double> h = design_filter(up, down);
    for (int p = 0; p < up; ++p)
        for (int k = 0; k < K; ++k) {
            const long long i = (long long)p + (long long)k * up;
            table_host[(size_t)p * K + k] = i < (long long)h.size() ? (float)h[(size_t)i] : 0.f;
        }
    return WUN_OK;
}

extern "C" int wun_resample(const float* x, int64_t n_in, int32_t c_in, float* y, int64_t y_offset, int64_t n_out,
                            int32_t c_out, const float* table_dev, int32_t up, int32_t down, void* stream) {
    if (!x || !y) return fail(WUN_ERR_INVALID, "null argument");
    int rc;
    if ((rc = check_ratio(up, down))) return rc;
    if (up != down && !table_dev) return fail(WUN_ERR_INVALID, "wun_resample: null table");
    const bool same = c_in == c_out && (c_in == 1 || c_in == 2);
    const bool mix = c_out == 1 && c_in >= 1 && c_in <= WUN_RESAMPLE_MAX_CH;
    const bool dup = c_in == 1 && c_out == 2;
    if (!same && !mix && !dup)
        return fail(WUN_ERR_INVALID, "wun_resample: channels must be equal (1 or 2), c_out = 1 (downmix of up to 8), or 1 -> 2");
    if (n_in < 0 || n_in > ((int64_t)1 << 46) || n_out < 0 || y_offset < 0)
        return fail(WUN_ERR_INVALID, "wun_resample: negative or oversized length / offset");
    if (n_out > (n_in * up + down - 1) / down) return fail(WUN_ERR_INVALID, "wun_resample: n_out beyond ceil(n_in * up / down)");
    const long long blocks = (n_out + WUN_RESAMPLE_BLOCK - 1) / WUN_RESAMPLE_BLOCK;
    if (blocks > 0x7fffffffLL) return fail(WUN_ERR_UNSUPPORTED, "wun_resample: more than 2^31 workgroups");

    ResampleArgs a;
    a.x = x; a.y = y; a.taps = table_dev;
    a.n_in = n_in; a.n_out = n_out; a.y_offset = y_offset;
    a.c_in = c_in; a.c_out = c_out; a.up = up; a.down = down;
    a.half = 10 * (up > down ? up : down);
    a.K = taps_per_row(up, down);
    a.y_vec2 = (c_out == 2 && (reinterpret_cast<uintptr_t>(y) & 7) == 0) ? 1 : 0;
    const int CL = same ? c_in : 1;
    // the widest window of a workgroup, and whether the table fits behind it
    const long long win = (((long long)up - 1 + (long long)(WUN_RESAMPLE_BLOCK - 1) * down) / up + a.K) * CL;
    const long long tab = (long long)up * a.K;
    if (up != down && win > WUN_RESAMPLE_LDS_FLOATS)
        return fail(WUN_ERR_UNSUPPORTED, "wun_resample: down / up too large for the 64 KB input window of a workgroup");
    if (n_out == 0) return WUN_OK;

    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks), blk(WUN_RESAMPLE_BLOCK);
    if (up == down) {
        if (CL == 2) hipLaunchKernelGGL(resample_copy_kernel<2>, grid, blk, 0, s, a);
        else hipLaunchKernelGGL(resample_copy_kernel<1>, grid, blk, 0, s, a);
    } else {
        const bool tab_lds = tab <= WUN_RESAMPLE_TAB_LDS && win + tab <= WUN_RESAMPLE_LDS_FLOATS;
        const size_t lds = (size_t)(win + (tab_lds ? tab : 0)) * sizeof(float);
        if (CL == 2) {
            if (tab_lds) hipLaunchKernelGGL((resample_kernel<2, true>), grid, blk, lds, s, a);
            else hipLaunchKernelGGL((resample_kernel<2, false>), grid, blk, lds, s, a);
        } else {
            if (tab_lds) hipLaunchKernelGGL((resample_kernel<1, true>), grid, blk, lds, s, a);
            else hipLaunchKernelGGL((resample_kernel<1, false>), grid, blk, lds, s, a);
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(WUN_ERR_HIP, std::string("wun_resample launch: ") + hipGetErrorString(e));
    return WUN_OK;
}
