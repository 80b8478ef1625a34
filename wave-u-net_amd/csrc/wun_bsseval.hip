// gfx950 (MI355X / CDNA4): the two heavy steps of BSS Eval v4 scoring (include/wun.h: wun_bss_*) -- what the
// reference leaves to museval at the end of Evaluate.predict (Evaluate.py:146-158).
//
//   lagged correlations   out[a][b][l] = sum_t x_a[t] * y_b[t + l],  l in [0, L),  x = the A = S*C reference signals,
//                         y = the references again (R) and the estimates (D); signals are zero outside [0, n)
//   window energies       for one window and one source: the projections P_own / P_all of the window's reference slices on
//                         the track's filters, and the eight energies the four metrics are ratios of
//
// Everything is float64 from float32 audio (a product of two float32 values is exact in float64; only the sums round).  Both
// steps sum in ONE order that depends on the sizes alone: fixed time chunks / tiles, each accumulated in ascending time by one
// FMA per term (correlations) or reduced by one fixed tree (energies), then a finish kernel adds the chunks in ascending
// order.  No atomics: the bits do not depend on the grid, the stream or where the buffers lie.
//
// Built WITHOUT the packed fp32 VALU instructions like wun_resample.hip (csrc/Makefile NO_PK_FP32): a track can
// be scored while another stream runs bf16 MFMA waves on the same CUs.  The C ABI of the group lives in this unit; every
// argument check runs before any GPU work, nothing allocates or synchronises.
#include "wun_device.h"
#include "../../include/wun.h"

#include <string>

using namespace wun;
int fail(int code, const std::string& msg);      // wun_plan.hip: sets wun_last_error(), returns code

#define WUN_BSS_MAX_L 512            // filters_len ceiling (museval's default)
#define WUN_BSS_BLOCK 256            // threads per workgroup: one lag / one output frame per lane
#define WUN_BSS_SUB 256              // frames staged in LDS at a time by the correlation kernel
#define WUN_BSS_CHUNK 16384          // frames per correlation partial: THE summation-order constant (a multiple of SUB)
#define WUN_BSS_G 4                  // signals per side of a correlation workgroup: G x G accumulators per lane
#define WUN_BSS_MAX_A 8              // reference signals the energies kernel stages (A * (256 + L - 1) doubles of LDS)
#define WUN_BSS_WIN_BATCH 64         // windows per energies launch (their table travels in the kernel arguments)
#define WUN_BSS_NE 8                 // energies per (window, source)

namespace wun {      // the kernels carry the library's wun:: prefix in profiler output

struct BssCorrArgs {
    const float* refs; const float* ests;    // [S, n, C] each
    double* part;                            // [nchunks][A][2A][L]
    long long n;
    int S, C, A, L;
};

// signal q < 2A of the right-hand side (q < A: reference q, else estimate q - A), sample t, zero outside [0, n)
__device__ __forceinline__ double bss_sample(const float* __restrict__ base, int sig, long long t, long long n, int C) {
    if (t < 0 || t >= n) return 0.0;
    return (double)base[((long long)(sig / C) * n + t) * C + (sig % C)];
}

// grid: x = time chunk, y = block of 256 lags, z = (left group, right group).  A workgroup walks its chunk in sub-tiles of 256
// frames: the left samples x_a[t] (wave-uniform operand, LDS broadcast) and the right samples y_b[t .. t + 511] (sliding window,
// lane l reads y_b[t + l]: consecutive doubles, conflict-free) are staged as float64, then every lane runs G x G FMA chains in
// ascending t.  Slots beyond the signal count are staged as zeros and not stored.
template <int G>
__global__ __launch_bounds__(WUN_BSS_BLOCK) void bss_corr_kernel(BssCorrArgs p) {
    __shared__ double xs[G][WUN_BSS_SUB];
    __shared__ double ys[G][WUN_BSS_SUB + WUN_BSS_BLOCK];
    const int tid = threadIdx.x;
    const int lag0 = blockIdx.y * WUN_BSS_BLOCK;
    const int ngb = (2 * p.A + G - 1) / G;
    const int a0 = ((int)blockIdx.z / ngb) * G, b0 = ((int)blockIdx.z % ngb) * G;
    const long long c0 = (long long)blockIdx.x * WUN_BSS_CHUNK;

    double acc[G][G];
#pragma unroll
    for (int i = 0; i < G; ++i)
#pragma unroll
        for (int j = 0; j < G; ++j) acc[i][j] = 0.0;

    for (long long t0 = c0; t0 < c0 + WUN_BSS_CHUNK && t0 < p.n; t0 += WUN_BSS_SUB) {
        __syncthreads();                                     // the previous sub-tile is read
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int a = a0 + g, b = b0 + g;
            xs[g][tid] = a < p.A ? bss_sample(p.refs, a, t0 + tid, p.n, p.C) : 0.0;
            const float* src = b < p.A ? p.refs : p.ests;
            const int sig = b < p.A ? b : b - p.A;
            for (int i = tid; i < WUN_BSS_SUB + WUN_BSS_BLOCK; i += WUN_BSS_BLOCK)
                ys[g][i] = b < 2 * p.A ? bss_sample(src, sig, t0 + lag0 + i, p.n, p.C) : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < WUN_BSS_SUB; ++i) {              // ascending t: the one accumulation order
            double xv[G], yv[G];
#pragma unroll
            for (int g = 0; g < G; ++g) { xv[g] = xs[g][i]; yv[g] = ys[g][i + tid]; }
#pragma unroll
            for (int ga = 0; ga < G; ++ga)
#pragma unroll
                for (int gb = 0; gb < G; ++gb) acc[ga][gb] = fma(xv[ga], yv[gb], acc[ga][gb]);
        }
    }
    const int lag = lag0 + tid;
    if (lag >= p.L) return;
    double* dst = p.part + (long long)blockIdx.x * p.A * 2 * p.A * p.L;
#pragma unroll
    for (int ga = 0; ga < G; ++ga)
#pragma unroll
        for (int gb = 0; gb < G; ++gb)
            if (a0 + ga < p.A && b0 + gb < 2 * p.A)
                dst[((long long)(a0 + ga) * 2 * p.A + (b0 + gb)) * p.L + lag] = acc[ga][gb];
}

// one thread per (a, q, lag): the partials of the chunks added in ascending chunk order.  q < A goes to R, q >= A to D.
__global__ __launch_bounds__(WUN_BSS_BLOCK) void bss_corr_finish_kernel(const double* __restrict__ part, double* __restrict__ R,
                                                                        double* __restrict__ D, int A, int L, int nchunks) {
    const long long total = (long long)A * 2 * A * L;
    const long long e = (long long)blockIdx.x * WUN_BSS_BLOCK + threadIdx.x;
    if (e >= total) return;
    double s = 0.0;
    for (int k = 0; k < nchunks; ++k) s += part[(long long)k * total + e];
    const int lag = (int)(e % L);
    const int q = (int)((e / L) % (2 * A)), a = (int)(e / ((long long)L * 2 * A));
    if (q < A) R[((long long)a * A + q) * L + lag] = s;
    else D[((long long)a * A + (q - A)) * L + lag] = s;
}

struct BssEnergyArgs {
    const float* refs; const float* ests;    // [S, n, C]
    const double* c_all;                     // [S][A][L][C] or NULL
    const double* c_own;                     // [S][C][L][C] or NULL
    double* part;                            // [nw][S][tiles][8]
    double* out;                             // [nw][S][8] (this batch's slice)
    long long n;
    int S, C, A, L, nw, tiles;
    long long start[WUN_BSS_WIN_BATCH];
    int len[WUN_BSS_WIN_BATCH];
};

// the fixed tree over the 256 lanes of a tile, for eight values at once; lanes 0..7 then hold nothing: red[e][0] does
__device__ __forceinline__ void bss_tile_reduce(double (*red)[WUN_BSS_BLOCK], const double* e, int tid) {
#pragma unroll
    for (int k = 0; k < WUN_BSS_NE; ++k) red[k][tid] = e[k];
    __syncthreads();
    for (int s = WUN_BSS_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < WUN_BSS_NE; ++k) red[k][tid] += red[k][tid + s];
        }
        __syncthreads();
    }
}

// grid: x = tile of 256 output frames, y = source, z = window of the batch.  FILT: the window's slices of all A reference
// signals, frames u0 - (L - 1) .. u0 + 255 of the window (zero outside [0, w)), are staged once as float64; lane u walks
// a ascending, l ascending with the filter taps as wave-uniform operands.  !FILT: each lane reads its frame of s and s^ once.
template <int CH, bool FILT>
__global__ __launch_bounds__(WUN_BSS_BLOCK) void bss_energy_kernel(BssEnergyArgs p) {
    extern __shared__ double sl[];                           // FILT: [A][256 + L - 1]
    __shared__ double red[WUN_BSS_NE][WUN_BSS_BLOCK];
    const int tid = threadIdx.x, j = blockIdx.y, k = blockIdx.z;
    const long long start = p.start[k];
    const int w = p.len[k];
    const int nout = FILT ? w + p.L - 1 : w;
    const int u0 = (int)blockIdx.x * WUN_BSS_BLOCK;
    double e[WUN_BSS_NE];
#pragma unroll
    for (int i = 0; i < WUN_BSS_NE; ++i) e[i] = 0.0;

    if (u0 < nout) {                                         // block-uniform: a tile behind the window's end adds zeros
        const int span = WUN_BSS_BLOCK + p.L - 1;
        if (FILT) {
            for (int a = 0; a < p.A; ++a)
                for (int i = tid; i < span; i += WUN_BSS_BLOCK) {
                    const int f = u0 - (p.L - 1) + i;
                    sl[a * span + i] = (f >= 0 && f < w) ? bss_sample(p.refs, a, start + f, p.n, CH) : 0.0;
                }
            __syncthreads();
        }
        const int u = u0 + tid;
        if (u < nout) {
            double s[CH], sh[CH], pall[CH], pown[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const bool in = u < w;
                s[c] = in ? (double)p.refs[((long long)j * p.n + start + u) * CH + c] : 0.0;
                sh[c] = in ? (double)p.ests[((long long)j * p.n + start + u) * CH + c] : 0.0;
                pall[c] = 0.0; pown[c] = 0.0;
            }
            if (FILT) {
                for (int a = 0; a < p.A; ++a) {
                    const double* __restrict__ fa = p.c_all + ((long long)j * p.A + a) * p.L * CH;
                    const double* col = sl + a * span + tid + (p.L - 1);
                    const bool own = a / CH == j;
                    if (own) {
                        const double* __restrict__ fo = p.c_own + ((long long)j * CH + (a % CH)) * p.L * CH;
                        for (int l = 0; l < p.L; ++l) {
                            const double v = col[-l];
#pragma unroll
                            for (int c = 0; c < CH; ++c) {
                                pall[c] = fma(fa[l * CH + c], v, pall[c]);
                                pown[c] = fma(fo[l * CH + c], v, pown[c]);
                            }
                        }
                    } else {
                        for (int l = 0; l < p.L; ++l) {
                            const double v = col[-l];
#pragma unroll
                            for (int c = 0; c < CH; ++c) pall[c] = fma(fa[l * CH + c], v, pall[c]);
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) {                   // channels in ascending order
                const double d0 = sh[c] - s[c];
                e[0] = fma(s[c], s[c], e[0]);
                e[1] = fma(sh[c], sh[c], e[1]);
                e[2] = fma(d0, d0, e[2]);
                if (FILT) {
                    const double d1 = pown[c] - s[c], d2 = pall[c] - pown[c], d3 = sh[c] - pall[c];
                    e[3] = fma(d1, d1, e[3]);
                    e[4] = fma(pown[c], pown[c], e[4]);
                    e[5] = fma(d2, d2, e[5]);
                    e[6] = fma(pall[c], pall[c], e[6]);
                    e[7] = fma(d3, d3, e[7]);
                }
            }
        }
    }
    bss_tile_reduce(red, e, tid);
    if (tid < WUN_BSS_NE)
        p.part[(((long long)k * p.S + j) * p.tiles + blockIdx.x) * WUN_BSS_NE + tid] = red[tid][0];
}

// one thread per (window, source, energy): the tiles added in ascending order
__global__ __launch_bounds__(WUN_BSS_BLOCK) void bss_energy_finish_kernel(const double* __restrict__ part, double* __restrict__ out,
                                                                          int rows, int tiles) {
    const int i = blockIdx.x * WUN_BSS_BLOCK + threadIdx.x;
    if (i >= rows * WUN_BSS_NE) return;
    const int row = i / WUN_BSS_NE, e = i % WUN_BSS_NE;
    double s = 0.0;
    for (int t = 0; t < tiles; ++t) s += part[((long long)row * tiles + t) * WUN_BSS_NE + e];
    out[i] = s;
}

}  // namespace wun

namespace {

int check_shape(const char* who, int32_t S, int64_t n, int32_t C, int32_t L) {
    if (S < 1) return fail(WUN_ERR_INVALID, std::string(who) + ": S < 1");
    if (C != 1 && C != 2) return fail(WUN_ERR_INVALID, std::string(who) + ": C must be 1 or 2");
    if (L < 1 || L > WUN_BSS_MAX_L) return fail(WUN_ERR_INVALID, std::string(who) + ": filters_len outside 1..512");
    if (n < 1) return fail(WUN_ERR_INVALID, std::string(who) + ": n < 1");
    if (n > ((int64_t)1 << 40) || S > 4096) return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 2^40 frames or 4096 sources");
    return WUN_OK;
}

int64_t corr_chunks(int64_t n) { return (n + WUN_BSS_CHUNK - 1) / WUN_BSS_CHUNK; }
int64_t energy_tiles(int64_t max_len, int32_t L) { return (max_len + L - 1 + WUN_BSS_BLOCK - 1) / WUN_BSS_BLOCK; }

}  // namespace

extern "C" int64_t wun_bss_windows(int64_t n, int64_t window, int64_t hop, int64_t* starts, int64_t* lengths, int64_t cap) {
    if (n < 1) return fail(WUN_ERR_INVALID, "wun_bss_windows: n < 1");
    if (window < 0 || (window > 0 && hop < 1)) return fail(WUN_ERR_INVALID, "wun_bss_windows: window < 0 or hop < 1");
    if ((starts == nullptr) != (lengths == nullptr)) return fail(WUN_ERR_INVALID, "wun_bss_windows: starts and lengths go together");
    int64_t count = 1;
    if (window > 0 && n >= window) count = (n - window + hop) / hop;
    if (!starts) return count;
    if (cap < count) return fail(WUN_ERR_INVALID, "wun_bss_windows: cap below the count");
    if (window == 0 || n < window) { starts[0] = 0; lengths[0] = n; return 1; }
    for (int64_t k = 0; k < count; ++k) { starts[k] = k * hop; lengths[k] = window; }
    lengths[count - 1] = n - starts[count - 1];              // the last window runs to the end
    return count;
}

extern "C" int64_t wun_bss_scratch_doubles(int32_t S, int64_t n, int32_t C, int32_t L, int64_t nwin, int64_t max_len) {
    int rc;
    if ((rc = check_shape("wun_bss_scratch_doubles", S, n, C, L))) return rc;
    if (nwin < 0 || max_len < 0 || max_len > n) return fail(WUN_ERR_INVALID, "wun_bss_scratch_doubles: nwin < 0 or max_len outside 0..n");
    const int64_t A = (int64_t)S * C;
    const int64_t corr = corr_chunks(n) * A * 2 * A * L;
    const int64_t batch = nwin < WUN_BSS_WIN_BATCH ? nwin : WUN_BSS_WIN_BATCH;
    const int64_t en = batch * S * energy_tiles(max_len, L) * WUN_BSS_NE;
    return corr > en ? corr : en;
}

extern "C" int wun_bss_correlations(const float* refs, const float* ests, int32_t S, int64_t n, int32_t C, int32_t L,
                                    double* R, double* D, double* scratch, void* stream) {
    if (!refs || !ests || !R || !D || !scratch) return fail(WUN_ERR_INVALID, "null argument");
    int rc;
    if ((rc = check_shape("wun_bss_correlations", S, n, C, L))) return rc;
    const int A = S * C;
    const int64_t chunks = corr_chunks(n);
    const int G = A >= 3 ? WUN_BSS_G : A;
    const int nga = (A + G - 1) / G, ngb = (2 * A + G - 1) / G;
    if (chunks > 0x7fffffffLL || (int64_t)nga * ngb > 65535)
        return fail(WUN_ERR_UNSUPPORTED, "wun_bss_correlations: grid above the launch limits");

    BssCorrArgs a;
    a.refs = refs; a.ests = ests; a.part = scratch; a.n = n; a.S = S; a.C = C; a.A = A; a.L = L;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)chunks, (unsigned)((L + WUN_BSS_BLOCK - 1) / WUN_BSS_BLOCK), (unsigned)(nga * ngb)), blk(WUN_BSS_BLOCK);
    if (G == 1) hipLaunchKernelGGL(bss_corr_kernel<1>, grid, blk, 0, s, a);
    else if (G == 2) hipLaunchKernelGGL(bss_corr_kernel<2>, grid, blk, 0, s, a);
    else hipLaunchKernelGGL(bss_corr_kernel<WUN_BSS_G>, grid, blk, 0, s, a);
    const int64_t total = (int64_t)A * 2 * A * L;
    hipLaunchKernelGGL(bss_corr_finish_kernel, dim3((unsigned)((total + WUN_BSS_BLOCK - 1) / WUN_BSS_BLOCK)), blk, 0, s,
                       scratch, R, D, A, L, (int)chunks);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(WUN_ERR_HIP, std::string("wun_bss_correlations launch: ") + hipGetErrorString(e));
    return WUN_OK;
}

extern "C" int wun_bss_window_energies(const float* refs, const float* ests, int32_t S, int64_t n, int32_t C, int32_t L,
                                       const double* c_all, const double* c_own, const int64_t* starts,
                                       const int64_t* lengths, int64_t nwin, double* energies, double* scratch,
                                       void* stream) {
    if (!refs || !ests || !starts || !lengths || !energies || !scratch) return fail(WUN_ERR_INVALID, "null argument");
    if ((c_all == nullptr) != (c_own == nullptr))
        return fail(WUN_ERR_INVALID, "wun_bss_window_energies: c_all and c_own are both given or both NULL");
    int rc;
    if ((rc = check_shape("wun_bss_window_energies", S, n, C, L))) return rc;
    if (nwin < 1) return fail(WUN_ERR_INVALID, "wun_bss_window_energies: nwin < 1");
    int64_t max_len = 0;
    for (int64_t k = 0; k < nwin; ++k) {
        if (starts[k] < 0 || lengths[k] < 1 || lengths[k] > n - starts[k])
            return fail(WUN_ERR_INVALID, "wun_bss_window_energies: a window outside [0, n)");
        if (lengths[k] > max_len) max_len = lengths[k];
    }
    const bool filt = c_all != nullptr;
    const int A = S * C;
    if (filt && A > WUN_BSS_MAX_A)
        return fail(WUN_ERR_UNSUPPORTED, "wun_bss_window_energies: more than 8 reference signals (S * C) for the LDS staging of the projection");
    if (S > 65535) return fail(WUN_ERR_UNSUPPORTED, "wun_bss_window_energies: more than 65535 sources");
    const int Leff = filt ? L : 1;                           // output frames of a window: len + Leff - 1
    const int64_t tiles = energy_tiles(max_len, Leff);
    if (max_len + Leff - 1 > 0x7fffffffLL) return fail(WUN_ERR_UNSUPPORTED, "wun_bss_window_energies: a window above 2^31 frames");

    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(WUN_BSS_BLOCK);
    const size_t lds = filt ? (size_t)A * (WUN_BSS_BLOCK + L - 1) * sizeof(double) : 0;
    for (int64_t k0 = 0; k0 < nwin; k0 += WUN_BSS_WIN_BATCH) {
        BssEnergyArgs a;
        a.refs = refs; a.ests = ests; a.c_all = c_all; a.c_own = c_own; a.part = scratch;
        a.out = energies + k0 * S * WUN_BSS_NE;
        a.n = n; a.S = S; a.C = C; a.A = A; a.L = Leff;
        a.nw = (int)(nwin - k0 < WUN_BSS_WIN_BATCH ? nwin - k0 : WUN_BSS_WIN_BATCH);
        a.tiles = (int)tiles;
        for (int k = 0; k < WUN_BSS_WIN_BATCH; ++k) {
            a.start[k] = k < a.nw ? starts[k0 + k] : 0;
            a.len[k] = k < a.nw ? (int)lengths[k0 + k] : 0;
        }
        const dim3 grid((unsigned)tiles, (unsigned)S, (unsigned)a.nw);
        if (filt) {
            if (C == 2) hipLaunchKernelGGL((bss_energy_kernel<2, true>), grid, blk, lds, s, a);
            else hipLaunchKernelGGL((bss_energy_kernel<1, true>), grid, blk, lds, s, a);
        } else {
            if (C == 2) hipLaunchKernelGGL((bss_energy_kernel<2, false>), grid, blk, 0, s, a);
            else hipLaunchKernelGGL((bss_energy_kernel<1, false>), grid, blk, 0, s, a);
        }
        const int rows = a.nw * S;
        hipLaunchKernelGGL(bss_energy_finish_kernel, dim3((unsigned)((rows * WUN_BSS_NE + WUN_BSS_BLOCK - 1) / WUN_BSS_BLOCK)), blk,
                           0, s, scratch, a.out, rows, (int)tiles);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(WUN_ERR_HIP, std::string("wun_bss_window_energies launch: ") + hipGetErrorString(e));
    return WUN_OK;
}
