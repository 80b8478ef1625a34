// gfx950 (MI355X / CDNA4): the spectral training loss (include/wun.h: wun_stft_*, wun_spectral_*) -- the L1
// distance between STFT magnitudes the reference builds from tf.contrib.signal.stft (Training.py:55-60), its gradient with
// respect to the waveform, and the time-domain MSE beside it.
//
//   forward    Re / Im[m][k] = sum_n x_m[n] * Cb / Sb[n][k],  m = (row, frame): a GEMM of the frames against the windowed
//              cos / sin table -- the forward tile of wun_stft.h, which describes the tile, its staging and its lane layout
//   loss       |M_est - M_tgt| summed in float64 (fixed blocks of 1024 bins, one tree per block, blocks added in one order);
//              the same pass turns Re / Im of the estimates into the coefficients sgn * Re / M, sgn * Im / M
//   backward   dframe[m][n] = sum_k cre[m][k] * Cb[n][k] + cim[m][k] * Sb[n][k]: the transposed GEMM, the inverse tile there
//   gradient   one lane per output float: the MSE term, then per resolution the frames that cover the sample, ascending
//
// ONE forward kernel serves wun_stft_magnitude and wun_spectral_loss: the magnitudes the loss takes its signs from are the
// floats wun_stft_magnitude returns.  Every reduction index runs in ascending order inside one lane's accumulator, whatever the
// tile a frame falls in: the bits of a row do not depend on the batch around it, the grid, the scratch contents or pointer
// alignment.  No atomics.
//
// Built WITHOUT the packed fp32 VALU instructions (csrc/Makefile NO_PK_FP32): the loss runs between the forward
// and the backward pass of either compute mode.  Every argument check runs before any GPU work; nothing allocates or synchronises.
#include "wun_stft.h"

#include <cmath>
#include <vector>

using namespace wun;

#define WUN_STFT_ITEMS 4             // elements per lane of the loss / gradient kernels: 1024 per partial, THE summation constant
#define WUN_SPEC_MAX_RES 8

namespace wun {      // the kernels carry the library's wun:: prefix in profiler output

struct StftFwdArgs {
    const float* x[2];               // [S, B, T, C]; blockIdx.z picks one (estimates, targets)
    float* mag[2];                   // [M][K]
    float* re; float* im;            // [M][K] of x[0], or NULL
    const float* table;              // Cb [n_fft][K], then Sb [n_fft][K]
    long long T, M;                  // frames of audio per row; M = R * F frame rows
    int F, C, n_fft, hop, K;
};

// grid: x = tile of 64 frame rows, y = tile of 32 bins, z = signal.  stft_fwd_tile (wun_stft.h) without the bounds check --
// every frame lies inside its row, which keeps the kernel at 5 waves per SIMD -- and the magnitude as its epilogue.
__global__ __launch_bounds__(WUN_STFT_BLOCK) void stft_fwd_kernel(StftFwdArgs p) {
    float* __restrict__ mag = p.mag[blockIdx.z];
    const bool parts = blockIdx.z == 0 && p.re != nullptr;
    stft_fwd_tile<false>(
        p.x[blockIdx.z], p.table, p.M, p.T, p.C, p.n_fft, p.K,
        [&](long long m, long long& base, long long& t0) {
            const long long r = m / p.F, f = m - r * p.F;
            const long long sb = r / p.C, c = r - sb * p.C;
            base = sb * p.T * p.C + c;
            t0 = f * p.hop;
        },
        [&](long long m, int k, float re, float im) {
            mag[m * p.K + k] = sqrtf(fmaf(re, re, im * im));     // (spelled out: which product is fused decides the bits)
            if (parts) { p.re[m * p.K + k] = re; p.im[m * p.K + k] = im; }
        });
}

// the fixed tree over the 256 lanes of a block; red[0] holds the sum afterwards
__device__ __forceinline__ double stft_block_sum(double* red, double v, int tid) {
    red[tid] = v;
    __syncthreads();
    for (int s = WUN_STFT_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// 1024 bins per block: part[block] = sum |M_est - M_tgt|; with re / im the coefficients of the gradient replace them in place:
// sgn(M_est - M_tgt) * Re / M_est and the same of Im, 0 where M_est == 0 or the magnitudes tie (sgn(0) = 0)
__global__ __launch_bounds__(WUN_STFT_BLOCK) void spec_l1_kernel(const float* __restrict__ me, const float* __restrict__ mt,
                                                                 float* re, float* im, double* __restrict__ part, long long E) {
    __shared__ double red[WUN_STFT_BLOCK];
    const int tid = threadIdx.x;
    double acc = 0.0;
#pragma unroll
    for (int it = 0; it < WUN_STFT_ITEMS; ++it) {
        const long long e = ((long long)blockIdx.x * WUN_STFT_ITEMS + it) * WUN_STFT_BLOCK + tid;
        if (e >= E) continue;
        const float a = me[e];
        const float d = a - mt[e];
        acc += (double)fabsf(d);
        if (re != nullptr) {
            const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            const bool live = sg != 0.f && a > 0.f;
            re[e] = live ? sg * re[e] / a : 0.f;
            im[e] = live ? sg * im[e] / a : 0.f;
        }
    }
    const double s = stft_block_sum(red, acc, tid);
    if (tid == 0) part[blockIdx.x] = s;
}

struct StftBwdArgs {
    const float* cre; const float* cim;      // [M][K]
    const float* table;
    float* dframe;                           // [M][n_fft]
    long long M;
    int n_fft, K;
};

// grid: x = tile of 64 frame rows, y = tile of 32 samples of the frame.  stft_inv_tile (wun_stft.h), unscaled, on the dense
// coefficient rows.
__global__ __launch_bounds__(WUN_STFT_BLOCK) void stft_bwd_kernel(StftBwdArgs p) {
    stft_inv_tile<false>(p.cre, p.cim, p.table, p.dframe, p.M, p.n_fft, p.K, 1.f, 1.f, [&](long long m) { return m * p.K; });
}

struct SpecGradArgs {
    const float* out; const float* tgt;      // [S, B, T, C]
    float* dout;                             // the same shape (GRAD only)
    double* part;                            // [ceil(N / 1024)]: sums of (out - tgt)^2
    long long T, N;
    float cm;                                // mse_weight * 2 / N
    int C, nres;
    int n_fft[WUN_SPEC_MAX_RES], hop[WUN_SPEC_MAX_RES], F[WUN_SPEC_MAX_RES];
    float scale[WUN_SPEC_MAX_RES];           // weight_j / (R F_j K_j)
    const float* dframe[WUN_SPEC_MAX_RES];   // [R * F_j][n_fft_j]
};

// one lane per output float (four per lane, 1024 per block): the MSE term, then resolution after resolution the frames that
// cover the sample, summed in ascending f and scaled once.  The block's sum of squared differences goes to part[block].
template <bool GRAD>
__global__ __launch_bounds__(WUN_STFT_BLOCK) void spec_grad_kernel(SpecGradArgs p) {
    __shared__ double red[WUN_STFT_BLOCK];
    const int tid = threadIdx.x;
    double sq = 0.0;
#pragma unroll
    for (int it = 0; it < WUN_STFT_ITEMS; ++it) {
        const long long e = ((long long)blockIdx.x * WUN_STFT_ITEMS + it) * WUN_STFT_BLOCK + tid;
        if (e >= p.N) continue;
        const float d = p.out[e] - p.tgt[e];
        sq += (double)d * (double)d;
        if (GRAD) {
            float g = p.cm != 0.f ? p.cm * d : 0.f;
            const long long sbt = e / p.C, sb = sbt / p.T;
            const long long t = sbt - sb * p.T, r = sb * p.C + (e - sbt * p.C);
            for (int j = 0; j < p.nres; ++j) {
                const int nf = p.n_fft[j], hop = p.hop[j];
                const long long f_lo = t >= nf ? (t - nf) / hop + 1 : 0;
                long long f_hi = t / hop;
                if (f_hi > p.F[j] - 1) f_hi = p.F[j] - 1;
                if (f_lo > f_hi) continue;                   // behind the last frame
                const float* __restrict__ df = p.dframe[j] + r * p.F[j] * nf;
                float a = 0.f;
                for (long long f = f_lo; f <= f_hi; ++f) a += df[f * nf + (t - f * hop)];
                g = fmaf(p.scale[j], a, g);
            }
            p.dout[e] = g;
        }
    }
    const double s = stft_block_sum(red, sq, tid);
    if (tid == 0) p.part[blockIdx.x] = s;
}

struct SpecFinishArgs {
    const double* part[1 + WUN_SPEC_MAX_RES];    // slot 0: MSE, slot 1 + j: resolution j
    long long nparts[1 + WUN_SPEC_MAX_RES];
    double count[1 + WUN_SPEC_MAX_RES];          // elements the slot's mean is taken over
    float weight[1 + WUN_SPEC_MAX_RES];
    float* losses;                               // [2 + nres]
    int nres;
};

// one wave per slot: lane l adds the partials l, l + 64, ... in ascending order, the 64 lanes are added by one tree; thread 0
// then forms the total in slot order.  One block of (1 + WUN_SPEC_MAX_RES) waves.
__global__ __launch_bounds__(64 * (1 + WUN_SPEC_MAX_RES)) void spec_finish_kernel(SpecFinishArgs p) {
    __shared__ double red[1 + WUN_SPEC_MAX_RES][64];
    const int slot = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double s = 0.0;
    if (slot <= p.nres)
        for (long long i = lane; i < p.nparts[slot]; i += 64) s += p.part[slot][i];
    red[slot][lane] = s;
    __syncthreads();
    for (int h = 32; h > 0; h >>= 1) {
        if (lane < h) red[slot][lane] += red[slot][lane + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int k = 0; k <= p.nres; ++k) {
            const double mean = red[k][0] / p.count[k];
            p.losses[1 + k] = (float)mean;
            total += (double)p.weight[k] * mean;
        }
        p.losses[0] = (float)total;
    }
}

}  // namespace wun

namespace {

struct Res { int n_fft, hop, K; long long F, M; };

int make_res(const char* who, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop, Res* r) {
    int rc;
    if ((rc = check_res(who, WUN_TR_GEMM, n_fft, hop, T))) return rc;
    r->n_fft = n_fft; r->hop = hop; r->K = n_fft / 2 + 1;
    r->F = 1 + (T - n_fft) / hop;
    r->M = (long long)S * B * C * r->F;
    if (r->M > ((long long)1 << 30)) return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 2^30 frames in all");
    return WUN_OK;
}

long long parts_of(long long n) { return (n + WUN_STFT_BLOCK * WUN_STFT_ITEMS - 1) / (WUN_STFT_BLOCK * WUN_STFT_ITEMS); }
// floats of one resolution's slice of the scratch: magnitudes of both signals, Re and Im of the estimates, the frame gradients
long long res_floats(const Res& r) { return 4 * r.M * r.K + r.M * r.n_fft; }

void launch_fwd(const float* x0, const float* x1, float* mag0, float* mag1, float* re, float* im, const float* table, int64_t T,
                int32_t C, const Res& r, hipStream_t s) {
    StftFwdArgs a;
    a.x[0] = x0; a.x[1] = x1; a.mag[0] = mag0; a.mag[1] = mag1; a.re = re; a.im = im; a.table = table;
    a.T = T; a.M = r.M; a.F = (int)r.F; a.C = C; a.n_fft = r.n_fft; a.hop = r.hop; a.K = r.K;
    const dim3 grid((unsigned)((r.M + WUN_STFT_BM - 1) / WUN_STFT_BM), (unsigned)((r.K + WUN_STFT_BN - 1) / WUN_STFT_BN), x1 ? 2u : 1u);
    hipLaunchKernelGGL(stft_fwd_kernel, grid, dim3(WUN_STFT_BLOCK), 0, s, a);
}

}  // namespace

extern "C" int64_t wun_stft_frames(int64_t frames, int32_t n_fft, int32_t hop) {
    int rc;
    if ((rc = check_res("wun_stft_frames", WUN_TR_GEMM, n_fft, hop, frames))) return rc;
    return 1 + (frames - n_fft) / hop;
}

extern "C" int64_t wun_stft_table_floats(int32_t n_fft) {
    int rc;
    if ((rc = check_res("wun_stft_table_floats", WUN_TR_GEMM, n_fft, 1))) return rc;
    return 2 * (int64_t)n_fft * (n_fft / 2 + 1);
}

extern "C" int wun_stft_design(int32_t n_fft, float* table_host, int64_t cap) {
    const int64_t need = wun_stft_table_floats(n_fft);
    if (need < 0) return (int)need;
    if (!table_host) return fail(WUN_ERR_INVALID, "wun_stft_design: null table");
    if (cap < need) return fail(WUN_ERR_INVALID, "wun_stft_design: cap below wun_stft_table_floats");
    const int K = n_fft / 2 + 1;
    const double step = 2.0 * 3.14159265358979323846 / (double)n_fft;
    std::vector<double> c(n_fft), s(n_fft);                  // one period, so that every entry is one libm call's value
    for (int i = 0; i < n_fft; ++i) { c[i] = std::cos(step * i); s[i] = std::sin(step * i); }
    float* cb = table_host;
    float* sb = table_host + (int64_t)n_fft * K;
    for (int n = 0; n < n_fft; ++n) {
        const double w = 0.5 - 0.5 * c[n];                   // periodic Hann
        for (int k = 0; k < K; ++k) {
            const int i = (int)(((int64_t)n * k) & (n_fft - 1));     // the angle reduced in integers (n_fft is a power of two)
            cb[(int64_t)n * K + k] = (float)(w * c[i]);
            sb[(int64_t)n * K + k] = (float)(-w * s[i]);
        }
    }
    return WUN_OK;
}

extern "C" int wun_stft_magnitude(const float* x, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                                  const float* table_dev, float* mags, void* stream) {
    if (!x || !table_dev || !mags) return fail(WUN_ERR_INVALID, "wun_stft_magnitude: null argument");
    int rc;
    Res r;
    if ((rc = check_audio("wun_stft_magnitude", S, B, T, C))) return rc;
    if ((rc = make_res("wun_stft_magnitude", S, B, T, C, n_fft, hop, &r))) return rc;
    launch_fwd(x, nullptr, mags, nullptr, nullptr, nullptr, table_dev, T, C, r, (hipStream_t)stream);
    return launch_status("wun_stft_magnitude");
}

extern "C" int64_t wun_spectral_scratch_floats(int32_t S, int32_t B, int64_t Tout, int32_t C, int32_t nres, const int32_t* n_fft,
                                               const int32_t* hop) {
    int rc;
    if ((rc = check_audio("wun_spectral_scratch_floats", S, B, Tout, C))) return rc;
    if (nres < 0 || nres > WUN_SPEC_MAX_RES) return fail(WUN_ERR_INVALID, "wun_spectral_scratch_floats: nres outside 0..8");
    if (nres > 0 && (!n_fft || !hop)) return fail(WUN_ERR_INVALID, "wun_spectral_scratch_floats: null resolution table");
    long long floats = 0, parts = parts_of((long long)S * B * Tout * C);
    for (int j = 0; j < nres; ++j) {
        Res r;
        if ((rc = make_res("wun_spectral_scratch_floats", S, B, Tout, C, n_fft[j], hop[j], &r))) return rc;
        floats += res_floats(r);
        parts += parts_of(r.M * r.K);
    }
    return floats + 2 * parts + 2;                           // float64 partials, and room to align them to 8 bytes
}

extern "C" int wun_spectral_loss(const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
                                 float mse_weight, int32_t nres, const int32_t* n_fft, const int32_t* hop, const float* weights,
                                 const float* const* tables_dev, float* d_outputs, float* losses, float* scratch, void* stream) {
    if (!outputs || !targets || !losses || !scratch) return fail(WUN_ERR_INVALID, "wun_spectral_loss: null argument");
    int rc;
    if ((rc = check_audio("wun_spectral_loss", S, B, Tout, C))) return rc;
    if (nres < 0 || nres > WUN_SPEC_MAX_RES) return fail(WUN_ERR_INVALID, "wun_spectral_loss: nres outside 0..8");
    if (nres > 0 && (!n_fft || !hop || !weights || !tables_dev)) return fail(WUN_ERR_INVALID, "wun_spectral_loss: null resolution table");
    if (!(mse_weight >= 0.f) || !std::isfinite(mse_weight)) return fail(WUN_ERR_INVALID, "wun_spectral_loss: mse_weight negative or not finite");
    Res res[WUN_SPEC_MAX_RES];
    for (int j = 0; j < nres; ++j) {
        if ((rc = make_res("wun_spectral_loss", S, B, Tout, C, n_fft[j], hop[j], &res[j]))) return rc;
        if (!(weights[j] >= 0.f) || !std::isfinite(weights[j])) return fail(WUN_ERR_INVALID, "wun_spectral_loss: a weight negative or not finite");
        if (!tables_dev[j]) return fail(WUN_ERR_INVALID, "wun_spectral_loss: null table");
    }

    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(WUN_STFT_BLOCK);
    const long long R = (long long)S * B * C, N = R * Tout;
    const bool grad = d_outputs != nullptr;
    // scratch: per resolution [M_est | M_tgt | Re -> cre | Im -> cim | dframe], then the float64 partials on an 8-byte boundary
    long long floats = 0;
    for (int j = 0; j < nres; ++j) floats += res_floats(res[j]);
    double* part = f64_tail(scratch, floats);

    SpecGradArgs g;
    SpecFinishArgs fin;
    g.out = outputs; g.tgt = targets; g.dout = d_outputs; g.T = Tout; g.N = N; g.C = C; g.nres = nres;
    g.cm = (float)((double)mse_weight * 2.0 / (double)N);
    fin.nres = nres; fin.losses = losses;
    for (int k = 0; k <= WUN_SPEC_MAX_RES; ++k) { fin.part[k] = part; fin.nparts[k] = 0; fin.count[k] = 1.0; fin.weight[k] = 0.f; }
    for (int j = 0; j < WUN_SPEC_MAX_RES; ++j) { g.n_fft[j] = 64; g.hop[j] = 64; g.F[j] = 0; g.scale[j] = 0.f; g.dframe[j] = nullptr; }
    g.part = part;
    fin.part[0] = part; fin.nparts[0] = parts_of(N); fin.count[0] = (double)N; fin.weight[0] = mse_weight;
    double* pnext = part + fin.nparts[0];

    float* base = scratch;
    for (int j = 0; j < nres; ++j) {
        const Res& r = res[j];
        const long long E = r.M * r.K;
        float* me = base; float* mt = base + E; float* re = base + 2 * E; float* im = base + 3 * E; float* df = base + 4 * E;
        base += res_floats(r);
        launch_fwd(outputs, targets, me, mt, grad ? re : nullptr, grad ? im : nullptr, tables_dev[j], Tout, C, r, s);
        hipLaunchKernelGGL(spec_l1_kernel, dim3((unsigned)parts_of(E)), blk, 0, s, me, mt, grad ? re : nullptr, grad ? im : nullptr,
                           pnext, E);
        if (grad) {
            StftBwdArgs b;
            b.cre = re; b.cim = im; b.table = tables_dev[j]; b.dframe = df; b.M = r.M; b.n_fft = r.n_fft; b.K = r.K;
            hipLaunchKernelGGL(stft_bwd_kernel, dim3((unsigned)((r.M + WUN_STFT_BM - 1) / WUN_STFT_BM), (unsigned)(r.n_fft / WUN_STFT_BN)),
                               blk, 0, s, b);
        }
        g.n_fft[j] = r.n_fft; g.hop[j] = r.hop; g.F[j] = (int)r.F; g.dframe[j] = df;
        g.scale[j] = (float)((double)weights[j] / ((double)r.M * (double)r.K));
        fin.part[1 + j] = pnext; fin.nparts[1 + j] = parts_of(E); fin.count[1 + j] = (double)E; fin.weight[1 + j] = weights[j];
        pnext += parts_of(E);
    }
    const dim3 ggrid((unsigned)parts_of(N));
    if (grad) hipLaunchKernelGGL(spec_grad_kernel<true>, ggrid, blk, 0, s, g);
    else hipLaunchKernelGGL(spec_grad_kernel<false>, ggrid, blk, 0, s, g);
    hipLaunchKernelGGL(spec_finish_kernel, dim3(1), dim3(64 * (1 + WUN_SPEC_MAX_RES)), 0, s, fin);
    return launch_status("wun_spectral_loss");
}
