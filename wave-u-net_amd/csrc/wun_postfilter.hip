// gfx950 (MI355X / CDNA4): the complex STFT, its inverse, the soft-mask post-filter and the multichannel Wiener (EM) filter
// (include/wun.h: wun_stft_complex, wun_istft, wun_mask_filter, wun_wiener_filter) -- the synthesis half
// of wun_spectral.hip's analysis, on the same table.
//
//   forward    Re / Im[r][f][k] = sum_n frame_f[n] * Cb / Sb[n][k], frame_f[n] = x[f hop - lead + n], zero outside [0, T):
//              the forward tile of wun_stft.h (stft_fwd_kernel's, wun_spectral.hip) with a bounds-checked gather
//   mask       mask_s = (A_s + eps / S) / (sum_j A_j + eps), A = |E|^p: one lane per bin reads the S estimate spectra and
//              the mix spectrum once and writes mask_s X over E_s
//   inverse    frame[m][n] = sum_k (c_k / n_fft) (Re[m][k] Cb[n][k] + Im[m][k] Sb[n][k]): the inverse tile of wun_stft.h
//              (stft_bwd_kernel's); the factor c_k / n_fft is a power of two, applied while the spectra are staged (exact)
//   overlap    y[t] = sum_f frame_f[t + lead - f hop] / sum_f w^2[t + lead - f hop]: one lane per output float, the covering
//              frames in ascending f, the window squares in float64 from a table the call computes first
//   EM         (wun_wiener_filter) per iteration: statistics sum_f y y^H and sum_f v per (source, bin) in float64 -- partial sums
//              over chunks of WUN_WF_CHUNK frames aligned to absolute frame numbers, then one reduction in ascending chunk order
//              -- and the per-bin C x C complex algebra v_s R_s Cxx^-1 X in float64 registers, one lane per (frame, bin)
//
// Frames are processed in blocks of WUN_PF_FRAMES (plus the ceil(n_fft / hop) - 1 frames before a block that its samples also
// lie in), so scratch does not grow with the track.  A frame's floats do not depend on the block or tile it is computed in (one
// accumulation order per output), and every output sample belongs to exactly one block (that of its last covering frame):
// the bits do not depend on the blocking, the grid, the scratch contents or pointer alignment.  No atomics.
//
// Every entry exists a second time with the frame transforms computed by an FFT (wun_*_fft): the bodies below
// take a selector `tr`, which launch_cfwd / launch_gemm turn into the GEMM kernels here or the FFT kernels of wun_fft.hip;
// blocks, mask, EM, overlap-add and scratch are the same code.  wun_griffin_lim iterates on the same blocks and
// overlap-add around gl_frame_kernel of wun_fft.hip.
//
// Built WITHOUT the packed fp32 VALU instructions (csrc/Makefile NO_PK_FP32): the filter runs beside inference of
// either compute mode.  Every argument check runs before any GPU work; nothing allocates or synchronises.
#include "wun_stft.h"

#include <cmath>

using namespace wun;

#define WUN_PF_FRAMES 256            // new frames per block of wun_istft / wun_mask_filter
#define WUN_PF_MAX_SOURCES 8
#define WUN_WF_CHUNK 16              // frames per partial sum of the EM statistics; divides WUN_PF_FRAMES
#define WUN_WF_MAX_ITERS 4

namespace wun {      // the kernels carry the library's wun:: prefix in profiler output

// (StftCfwdArgs, the frame rows of one launch: wun_fft.h)

// grid: x = tile of 64 frame rows, y = tile of 32 bins, z = signal.  stft_fwd_tile (wun_stft.h) with the bounds check -- a frame
// may reach outside [0, T) -- storing Re / Im at the frame's row of the spectra.
__global__ __launch_bounds__(WUN_STFT_BLOCK) void stft_cfwd_kernel(StftCfwdArgs p) {
    const int z = blockIdx.z;
    const long long M = p.M[z];
    if ((long long)blockIdx.x * WUN_STFT_BM >= M) return;    // (the grid is sized by the larger signal)
    float* __restrict__ re = p.re[z];
    float* __restrict__ im = p.im[z];
    stft_fwd_tile<true>(
        p.x[z], p.table, M, p.T, p.C, p.n_fft, p.K,
        [&](long long m, long long& base, long long& t0) {
            const long long r = m / p.nb, fl = m - r * p.nb;
            const long long sb = r / p.C, c = r - sb * p.C;
            base = sb * p.T * p.C + c;
            t0 = (p.f0 + fl) * p.hop - p.lead;
        },
        [&](long long m, int k, float vre, float vim) {
            const long long r = m / p.nb, fl = m - r * p.nb;
            const long long o = (r * p.fstride + p.foff + fl) * p.K + k;
            re[o] = vre;
            im[o] = vim;
        });
}

// One lane per bin (c, frame, k) of a block: xre / xim [C][nb][K] is the mix spectrum, ere / eim [S][C][nb][K] the estimates',
// which mask_s * X replaces.  E = C * nb * K bins.  POWER 2: A = Re^2 + Im^2, no square root; POWER 1: its root.
template <int POWER>
__global__ __launch_bounds__(WUN_STFT_BLOCK) void mask_kernel(const float* __restrict__ xre, const float* __restrict__ xim, float* ere,
                                                            float* eim, long long E, int S, float eps, float eps_s) {
    const long long e = (long long)blockIdx.x * WUN_STFT_BLOCK + threadIdx.x;
    if (e >= E) return;
    float A[WUN_PF_MAX_SOURCES];
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < WUN_PF_MAX_SOURCES; ++s) {           // j ascending
        A[s] = 0.f;
        if (s < S) {
            const float re = ere[s * E + e], im = eim[s * E + e];
            const float a = re * re + im * im;
            A[s] = POWER == 2 ? a : sqrtf(a);
            sum += A[s];
        }
    }
    const float den = sum + eps;
    const float xr = xre[e], xi = xim[e];
#pragma unroll
    for (int s = 0; s < WUN_PF_MAX_SOURCES; ++s)
        if (s < S) {
            const float mask = (A[s] + eps_s) / den;
            ere[s * E + e] = mask * xr;
            eim[s * E + e] = mask * xi;
        }
}

// grid: x = tile of 64 frame rows, y = tile of 32 samples of the frame.  stft_inv_tile (wun_stft.h) with the spectra scaled by
// c_k / n_fft while staged, on the frame rows' places in the spectra.
__global__ __launch_bounds__(WUN_STFT_BLOCK) void istft_gemm_kernel(IstftGemmArgs p) {
    stft_inv_tile<true>(p.re, p.im, p.table, p.frames, p.M, p.n_fft, p.K, p.c_edge, p.c_mid, [&](long long m) {
        const long long r = m / p.nb, fl = m - r * p.nb;
        return (r * p.fstride + p.foff + fl) * p.K;
    });
}

// wsq[n] = w[n]^2 in float64, w the periodic Hann window (cospi: the argument n / n_fft is exact, no range reduction)
__global__ __launch_bounds__(WUN_STFT_BLOCK) void window_sq_kernel(double* __restrict__ wsq, int n_fft) {
    const int n = blockIdx.x * WUN_STFT_BLOCK + threadIdx.x;
    if (n >= n_fft) return;
    const double w = 0.5 - 0.5 * cospi(2.0 * (double)n / (double)n_fft);
    wsq[n] = w * w;
}

struct OlaArgs {
    const float* frames;                     // [R][nb][n_fft]: frames fb0 .. fb0 + nb - 1 of every row
    const double* wsq;                       // [n_fft]
    float* y;                                // [SB, T, C]
    long long T, F, nb, fb0, t_lo, t_hi, N;  // this launch writes the samples [t_lo, t_hi) of every row: N floats
    int C, n_fft, hop, lead;
};

// one lane per output float: the frames that cover the sample in ascending f, over the window squares of the same frames;
// 0 where those sum to less than 1e-8 (librosa's rule).  Grid-stride: the grid is capped, one writer per float all the same.
// STEADY (wun_istft_tf): the denominator is the steady-state window-square sum D[u mod hop] = sum_i w^2[u mod hop + i hop] over
// the places inside the frame, i ascending -- what tf.contrib.signal.inverse_stft_window_fn divides by, at the track's edges too.
template <bool STEADY>
__global__ __launch_bounds__(WUN_STFT_BLOCK) void istft_ola_kernel(OlaArgs p) {
    const long long span = (p.t_hi - p.t_lo) * p.C;
    for (long long e = (long long)blockIdx.x * WUN_STFT_BLOCK + threadIdx.x; e < p.N; e += (long long)gridDim.x * WUN_STFT_BLOCK) {
        const long long sb = e / span, rest = e - sb * span;
        const long long tl = rest / p.C, c = rest - tl * p.C;
        const long long t = p.t_lo + tl, u = t + p.lead;     // u - f hop is the sample's place in frame f
        const long long f_lo = u >= p.n_fft ? (u - p.n_fft) / p.hop + 1 : 0;
        long long f_hi = u / p.hop;
        if (f_hi > p.F - 1) f_hi = p.F - 1;
        const float* __restrict__ fr = p.frames + (sb * p.C + c) * p.nb * p.n_fft;
        float a = 0.f;
        double ws = 0.0;
        for (long long f = f_lo; f <= f_hi; ++f) {
            const long long n = u - f * p.hop;
            a += fr[(f - p.fb0) * p.n_fft + n];
            if (!STEADY) ws += p.wsq[n];
        }
        if (STEADY)
            for (long long n = u % p.hop; n < p.n_fft; n += p.hop) ws += p.wsq[n];
        p.y[(sb * p.T + t) * p.C + c] = ws < 1e-8 ? 0.f : a / (float)ws;
    }
}

// ---- the multichannel Wiener filter's EM iterations ----
// Statistics of one (source, bin): Q = CH^2 + 1 doubles, stored [S][Q][K].  CH = 2: sum |y_0|^2, sum |y_1|^2, Re and Im of
// sum y_0 conj(y_1), sum v;  CH = 1: sum |y|^2, sum v.  Divided by eps + sum v they are R_s[k] (Hermitian: its CH^2 real
// numbers); the last entry keeps sum v.

// One lane per (source, chunk of WUN_WF_CHUNK frames, bin), the bin fastest: walks its frames in ascending order and writes the
// chunk's partial sums to part [nch][S][Q][K].  yre / yim [S][CH][nf][K] are the block's spectra; the block starts at a
// multiple of WUN_PF_FRAMES, so chunk c holds the absolute frames [f0 + 16 c, f0 + 16 c + 16) whatever the track's length.
template <int CH>
__global__ __launch_bounds__(WUN_STFT_BLOCK) void wiener_stats_kernel(const float* __restrict__ yre, const float* __restrict__ yim,
                                                                    double* __restrict__ part, int S, int nf, int K) {
    constexpr int Q = CH * CH + 1;
    const int nch = (nf + WUN_WF_CHUNK - 1) / WUN_WF_CHUNK;
    const long long e = (long long)blockIdx.x * WUN_STFT_BLOCK + threadIdx.x;
    if (e >= (long long)S * nch * K) return;
    const int k = (int)(e % K);
    const int t = (int)(e / K), ch = t % nch, s = t / nch;
    const long long NK = (long long)nf * K;
    double acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.0;
    const int fl1 = (ch + 1) * WUN_WF_CHUNK < nf ? (ch + 1) * WUN_WF_CHUNK : nf;
    for (int fl = ch * WUN_WF_CHUNK; fl < fl1; ++fl) {       // ascending f
        const long long i0 = (long long)s * CH * NK + (long long)fl * K + k;
        const double ar = yre[i0], ai = yim[i0];
        const double p0 = ar * ar + ai * ai;
        if constexpr (CH == 1) {
            acc[0] += p0;
            acc[1] += p0;
        } else {
            const double br = yre[i0 + NK], bi = yim[i0 + NK];
            const double p1 = br * br + bi * bi;
            acc[0] += p0;
            acc[1] += p1;
            acc[2] += ar * br + ai * bi;                     // y_0 conj(y_1)
            acc[3] += ai * br - ar * bi;
            acc[CH * CH] += 0.5 * (p0 + p1);
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) part[(((long long)ch * S + s) * Q + q) * K + k] = acc[q];
}

// One lane per (source, bin): adds the block's nch partial sums, in ascending chunk order, to the running sums (`first`: the
// track's first block starts them from 0, so nothing is read that this call did not write).  `last`: the track's last block
// then divides by eps + sum v, leaving R_s[k] and sum v.
template <int Q>
__global__ __launch_bounds__(WUN_STFT_BLOCK) void wiener_reduce_kernel(const double* __restrict__ part, double* __restrict__ stat, int S,
                                                                     int K, int nch, int first, int last, double eps) {
    const int e = blockIdx.x * WUN_STFT_BLOCK + threadIdx.x;
    if (e >= S * K) return;
    const int s = e / K, k = e - s * K;
    double a[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const long long o = ((long long)s * Q + q) * K + k;
        a[q] = first ? 0.0 : stat[o];
        for (int c = 0; c < nch; ++c) a[q] += part[(long long)c * S * Q * K + o];
    }
    if (last) {
        const double den = eps + a[Q - 1];
#pragma unroll
        for (int q = 0; q < Q - 1; ++q) a[q] /= den;
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) stat[((long long)s * Q + q) * K + k] = a[q];
}

// One lane per (frame, bin) of a block, mask_kernel's access pattern: reads X (xre / xim [CH][nb][K]) and the S masked spectra
// (yre / yim [S][CH][nb][K]) once, applies the `niter` filters R [niter][S][Q][K] one after the other -- v_s, Cxx = sum_s v_s
// R_s + sq I, its closed-form inverse and y_s = v_s R_s Cxx^-1 X in float64, each y rounded to float32 (a stored spectrum) --
// and writes the last y over the masked spectra.  NK = nb * K.
template <int CH>
__global__ __launch_bounds__(WUN_STFT_BLOCK) void wiener_apply_kernel(const float* __restrict__ xre, const float* __restrict__ xim,
                                                                    float* yre, float* yim, const double* __restrict__ R, long long NK,
                                                                    int S, int K, int niter, double sq) {
    constexpr int Q = CH * CH + 1;
    const long long e = (long long)blockIdx.x * WUN_STFT_BLOCK + threadIdx.x;
    if (e >= NK) return;
    const int k = (int)(e % K);
    float yr[WUN_PF_MAX_SOURCES][CH], yi[WUN_PF_MAX_SOURCES][CH];
    double xr[CH], xi[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) { xr[c] = xre[c * NK + e]; xi[c] = xim[c * NK + e]; }
#pragma unroll
    for (int s = 0; s < WUN_PF_MAX_SOURCES; ++s)
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            yr[s][c] = 0.f; yi[s][c] = 0.f;
            if (s < S) { yr[s][c] = yre[(s * CH + c) * NK + e]; yi[s][c] = yim[(s * CH + c) * NK + e]; }
        }
    for (int it = 0; it < niter; ++it) {
        const double* __restrict__ Rt = R + (long long)it * S * Q * K + k;
        double v[WUN_PF_MAX_SOURCES];
        double a = 0.0, d = 0.0, br = 0.0, bi = 0.0;         // Cxx = [a, b; conj(b), d]  (CH = 1: a alone)
#pragma unroll
        for (int s = 0; s < WUN_PF_MAX_SOURCES; ++s) {       // s ascending
            v[s] = 0.0;
            if (s < S) {
                const double p0 = (double)yr[s][0] * yr[s][0] + (double)yi[s][0] * yi[s][0];
                if constexpr (CH == 1) {
                    v[s] = p0;
                    a += v[s] * Rt[(long long)s * Q * K];
                } else {
                    const double p1 = (double)yr[s][CH - 1] * yr[s][CH - 1] + (double)yi[s][CH - 1] * yi[s][CH - 1];
                    v[s] = 0.5 * (p0 + p1);
                    a += v[s] * Rt[((long long)s * Q + 0) * K];
                    d += v[s] * Rt[((long long)s * Q + 1) * K];
                    br += v[s] * Rt[((long long)s * Q + 2) * K];
                    bi += v[s] * Rt[((long long)s * Q + 3) * K];
                }
            }
        }
        a += sq; d += sq;
        double zr[CH], zi[CH];                               // z = Cxx^-1 X
        if constexpr (CH == 1) {
            zr[0] = xr[0] / a; zi[0] = xi[0] / a;
        } else {
            const double det = a * d - (br * br + bi * bi);
            zr[0] = (d * xr[0] - (br * xr[CH - 1] - bi * xi[CH - 1])) / det;       // d X_0 - b X_1
            zi[0] = (d * xi[0] - (br * xi[CH - 1] + bi * xr[CH - 1])) / det;
            zr[CH - 1] = (a * xr[CH - 1] - (br * xr[0] + bi * xi[0])) / det;       // a X_1 - conj(b) X_0
            zi[CH - 1] = (a * xi[CH - 1] - (br * xi[0] - bi * xr[0])) / det;
        }
#pragma unroll
        for (int s = 0; s < WUN_PF_MAX_SOURCES; ++s)
            if (s < S) {
                if constexpr (CH == 1) {
                    const double g = v[s] * Rt[(long long)s * Q * K];
                    yr[s][0] = (float)(g * zr[0]); yi[s][0] = (float)(g * zi[0]);
                } else {
                    const double r00 = Rt[((long long)s * Q + 0) * K], r11 = Rt[((long long)s * Q + 1) * K];
                    const double r01r = Rt[((long long)s * Q + 2) * K], r01i = Rt[((long long)s * Q + 3) * K];
                    // R z: [r00 z_0 + r01 z_1; conj(r01) z_0 + r11 z_1]
                    const double g0r = r00 * zr[0] + (r01r * zr[CH - 1] - r01i * zi[CH - 1]);
                    const double g0i = r00 * zi[0] + (r01r * zi[CH - 1] + r01i * zr[CH - 1]);
                    const double g1r = (r01r * zr[0] + r01i * zi[0]) + r11 * zr[CH - 1];
                    const double g1i = (r01r * zi[0] - r01i * zr[0]) + r11 * zi[CH - 1];
                    yr[s][0] = (float)(v[s] * g0r); yi[s][0] = (float)(v[s] * g0i);
                    yr[s][CH - 1] = (float)(v[s] * g1r); yi[s][CH - 1] = (float)(v[s] * g1i);
                }
            }
    }
#pragma unroll
    for (int s = 0; s < WUN_PF_MAX_SOURCES; ++s)
        if (s < S)
#pragma unroll
            for (int c = 0; c < CH; ++c) { yre[(s * CH + c) * NK + e] = yr[s][c]; yim[(s * CH + c) * NK + e] = yi[s][c]; }
}

}  // namespace wun

namespace {

int check_framing(const char* who, int32_t S, int32_t B, int32_t C, int32_t n_fft, int32_t lead, int64_t F) {
    if (lead < 0 || lead >= n_fft) return fail(WUN_ERR_INVALID, std::string(who) + ": lead outside [0, n_fft)");
    if (F < 1) return fail(WUN_ERR_INVALID, std::string(who) + ": F < 1");
    if (F > ((int64_t)1 << 30) / ((int64_t)S * B * C))
        return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 2^30 frames in all");
    return WUN_OK;
}

bool overlaps(const void* a, long long na, const void* b, long long nb) {      // float counts
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + 4 * (uintptr_t)na, b0 = (uintptr_t)b, b1 = b0 + 4 * (uintptr_t)nb;
    return a0 < b1 && b0 < a1;
}

long long centered_frames(int64_t T, int32_t n_fft, int32_t hop) { return (T + (n_fft - hop) + hop - 1) / hop; }
int overlap_frames(int32_t n_fft, int32_t hop) { return (n_fft + hop - 1) / hop - 1; }
// frames a block holds at most: its own and the overlap before them (or the whole transform, when that is shorter)
long long block_frames(int64_t F, int32_t n_fft, int32_t hop) {
    const long long nb = WUN_PF_FRAMES + overlap_frames(n_fft, hop);
    return F < nb ? F : nb;
}

// the block of frames [f0, f1): the frames computed for it start at fb0, and its samples are [t_lo, t_hi) -- those whose last
// covering frame lies in the block (the last block also takes the samples behind the last frame)
struct Blk { long long fb0, nb, t_lo, t_hi; };
Blk block_of(long long f0, int64_t F, int64_t T, int32_t n_fft, int32_t hop, int32_t lead) {
    Blk b;
    const long long f1 = f0 + WUN_PF_FRAMES < F ? f0 + WUN_PF_FRAMES : F;
    b.fb0 = f0 - overlap_frames(n_fft, hop);
    if (b.fb0 < 0) b.fb0 = 0;
    b.nb = f1 - b.fb0;
    auto clampT = [T](long long t) { return t < 0 ? 0 : (t > T ? (long long)T : t); };
    b.t_lo = f0 == 0 ? 0 : clampT(f0 * hop - lead);
    b.t_hi = f1 == F ? (long long)T : clampT(f1 * hop - lead);
    return b;
}

// (both launchers: WUN_OK, or the FFT path's refusal of an n_fft it has no kernel for -- unreachable behind check_res)
int launch_cfwd(int tr, const float* x0, long long rows0, float* re0, float* im0, const float* x1, long long rows1, float* re1,
                float* im1, const float* table, int64_t T, int32_t C, int32_t n_fft, int32_t hop, int32_t lead, long long nb,
                long long f0, long long fstride, long long foff, hipStream_t s) {
    StftCfwdArgs a;
    a.x[0] = x0; a.re[0] = re0; a.im[0] = im0; a.M[0] = rows0 * nb;
    a.x[1] = x1; a.re[1] = re1; a.im[1] = im1; a.M[1] = rows1 * nb;
    a.table = table; a.T = T; a.nb = nb; a.f0 = f0; a.fstride = fstride; a.foff = foff;
    a.C = C; a.n_fft = n_fft; a.hop = hop; a.lead = lead; a.K = n_fft / 2 + 1;
    if (tr == WUN_TR_FFT) return fft_launch_forward(a, x1 ? 2 : 1, s);
    const long long M = a.M[0] > a.M[1] ? a.M[0] : a.M[1];
    const dim3 grid((unsigned)((M + WUN_STFT_BM - 1) / WUN_STFT_BM), (unsigned)((a.K + WUN_STFT_BN - 1) / WUN_STFT_BN), x1 ? 2u : 1u);
    hipLaunchKernelGGL(stft_cfwd_kernel, grid, dim3(WUN_STFT_BLOCK), 0, s, a);
    return WUN_OK;
}

int launch_gemm(int tr, const float* re, const float* im, const float* table, float* frames, long long rows, long long nb,
                long long fstride, long long foff, int32_t n_fft, hipStream_t s) {
    IstftGemmArgs g;
    g.re = re; g.im = im; g.table = table; g.frames = frames; g.M = rows * nb; g.nb = nb; g.fstride = fstride; g.foff = foff;
    g.n_fft = n_fft; g.K = n_fft / 2 + 1; g.c_edge = 1.f / (float)n_fft; g.c_mid = 2.f / (float)n_fft;
    if (tr == WUN_TR_FFT) return fft_launch_inverse(g, s);
    hipLaunchKernelGGL(istft_gemm_kernel, dim3((unsigned)((g.M + WUN_STFT_BM - 1) / WUN_STFT_BM), (unsigned)(n_fft / WUN_STFT_BN)),
                       dim3(WUN_STFT_BLOCK), 0, s, g);
    return WUN_OK;
}

void launch_ola(const float* frames, const double* wsq, float* y, long long SB, int64_t T, int32_t C, int64_t F, const Blk& b,
                int32_t n_fft, int32_t hop, int32_t lead, hipStream_t s, bool steady = false) {
    OlaArgs o;
    o.frames = frames; o.wsq = wsq; o.y = y; o.T = T; o.F = F; o.nb = b.nb; o.fb0 = b.fb0; o.t_lo = b.t_lo; o.t_hi = b.t_hi;
    o.N = SB * (b.t_hi - b.t_lo) * C; o.C = C; o.n_fft = n_fft; o.hop = hop; o.lead = lead;
    long long grid = (o.N + WUN_STFT_BLOCK - 1) / WUN_STFT_BLOCK;
    if (grid > (1 << 20)) grid = 1 << 20;
    hipLaunchKernelGGL(steady ? istft_ola_kernel<true> : istft_ola_kernel<false>, dim3((unsigned)grid), dim3(WUN_STFT_BLOCK), 0, s, o);
}

void launch_window(double* wsq, int32_t n_fft, hipStream_t s) {
    hipLaunchKernelGGL(window_sq_kernel, dim3((unsigned)((n_fft + WUN_STFT_BLOCK - 1) / WUN_STFT_BLOCK)), dim3(WUN_STFT_BLOCK), 0, s, wsq,
                       n_fft);
}

// mask_s X over the estimates' spectra of one block: E = C nb K bins per source
void launch_mask(const float* xre, const float* xim, float* ere, float* eim, long long E, int32_t S, int32_t power, float eps,
                 hipStream_t s) {
    const dim3 grid((unsigned)((E + WUN_STFT_BLOCK - 1) / WUN_STFT_BLOCK)), blk(WUN_STFT_BLOCK);
    if (power == 2) hipLaunchKernelGGL(mask_kernel<2>, grid, blk, 0, s, xre, xim, ere, eim, E, S, eps, eps / (float)S);
    else hipLaunchKernelGGL(mask_kernel<1>, grid, blk, 0, s, xre, xim, ere, eim, E, S, eps, eps / (float)S);
}

int check_filter(const char* who, int tr, int32_t S, int64_t n, int32_t C, int32_t n_fft, int32_t hop) {
    int rc;
    if ((rc = check_audio(who, S, 1, n, C))) return rc;
    if ((rc = check_res(who, tr, n_fft, hop))) return rc;
    if ((hop & (hop - 1)) || hop > n_fft / 2)
        return fail(WUN_ERR_INVALID, std::string(who) + ": hop must be a power of two, at most n_fft / 2");
    if (S > WUN_PF_MAX_SOURCES) return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 8 sources");
    return check_framing(who, S + 1, 1, C, n_fft, n_fft - hop, centered_frames(n, n_fft, hop));
}

}  // namespace

// Every entry below exists twice, on the GEMM and on the FFT (`tr`): one body, the transform picked in launch_cfwd / launch_gemm.
namespace {

int64_t centered_frames_entry(const char* who, int tr, int64_t T, int32_t n_fft, int32_t hop) {
    int rc;
    if ((rc = check_res(who, tr, n_fft, hop))) return rc;
    if (T < 1 || T > ((int64_t)1 << 40)) return fail(WUN_ERR_INVALID, std::string(who) + ": T outside 1..2^40");
    return centered_frames(T, n_fft, hop);
}

int stft_complex_entry(const char* who, int tr, const float* x, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                       int32_t lead, int64_t F, const float* table_dev, float* re, float* im, void* stream) {
    if (!x || !table_dev || !re || !im) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    int rc;
    if ((rc = check_audio(who, S, B, T, C))) return rc;
    if ((rc = check_res(who, tr, n_fft, hop))) return rc;
    if ((rc = check_framing(who, S, B, C, n_fft, lead, F))) return rc;
    const long long R = (long long)S * B * C, E = R * F * (n_fft / 2 + 1);
    if (overlaps(re, E, x, R * T) || overlaps(im, E, x, R * T) || overlaps(re, E, im, E))
        return fail(WUN_ERR_INVALID, std::string(who) + ": re / im overlap the audio or each other");
    if ((rc = launch_cfwd(tr, x, R, re, im, nullptr, 0, nullptr, nullptr, table_dev, T, C, n_fft, hop, lead, F, 0, F, 0, (hipStream_t)stream))) return rc;
    return launch_status(who);
}

int64_t istft_scratch_entry(const char* who, int tr, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                            int32_t lead, int64_t F) {
    int rc;
    if ((rc = check_audio(who, S, B, T, C))) return rc;
    if ((rc = check_res(who, tr, n_fft, hop))) return rc;
    if ((rc = check_framing(who, S, B, C, n_fft, lead, F))) return rc;
    return (int64_t)S * B * C * block_frames(F, n_fft, hop) * n_fft + 2 * (int64_t)n_fft + 2;
}

// the smallest steady-state window-square sum D[p] = sum_i w^2[p + i hop] of a resolution (float64, host): wun_istft_tf divides
// by D and refuses a resolution where some D[p] is below 1e-8
double steady_min(int32_t n_fft, int32_t hop) {
    double dmin = INFINITY;
    for (int p = 0; p < hop; ++p) {
        double d = 0.0;
        for (int n = p; n < n_fft; n += hop) {
            const double w = 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)n / (double)n_fft);
            d += w * w;
        }
        if (d < dmin) dmin = d;
    }
    return dmin;
}

int check_steady(const char* who, int32_t n_fft, int32_t hop) {
    if (steady_min(n_fft, hop) < 1e-8)
        return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": a steady-state window-square sum of this n_fft / hop is below 1e-8");
    return WUN_OK;
}

// steady: wun_istft_tf's normaliser (istft_ola_kernel<true>) in place of the sum over the covering frames
int istft_entry(const char* who, int tr, const float* re, const float* im, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft,
                int32_t hop, int32_t lead, int64_t F, const float* table_dev, float* y, float* scratch, void* stream,
                bool steady = false) {
    if (!re || !im || !table_dev || !y || !scratch) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    int rc;
    if ((rc = check_audio(who, S, B, T, C))) return rc;
    if ((rc = check_res(who, tr, n_fft, hop))) return rc;
    if ((rc = check_framing(who, S, B, C, n_fft, lead, F))) return rc;
    if (steady && (rc = check_steady(who, n_fft, hop))) return rc;
    const long long R = (long long)S * B * C, E = R * F * (n_fft / 2 + 1);
    if (overlaps(y, R * T, re, E) || overlaps(y, R * T, im, E))
        return fail(WUN_ERR_INVALID, std::string(who) + ": y overlaps re or im");

    hipStream_t s = (hipStream_t)stream;
    float* frames = scratch;
    double* wsq = f64_tail(scratch, R * block_frames(F, n_fft, hop) * n_fft);
    launch_window(wsq, n_fft, s);
    for (long long f0 = 0; f0 < F; f0 += WUN_PF_FRAMES) {
        const Blk b = block_of(f0, F, T, n_fft, hop, lead);
        if (b.t_lo >= b.t_hi) continue;                      // no sample ends in this block
        if ((rc = launch_gemm(tr, re, im, table_dev, frames, R, b.nb, F, b.fb0, n_fft, s))) return rc;
        launch_ola(frames, wsq, y, (long long)S * B, T, C, F, b, n_fft, hop, lead, s, steady);
    }
    return launch_status(who);
}

int64_t mask_scratch_entry(const char* who, int tr, int32_t S, int64_t n, int32_t C, int32_t n_fft, int32_t hop) {
    int rc;
    if ((rc = check_filter(who, tr, S, n, C, n_fft, hop))) return rc;
    const long long nb = block_frames(centered_frames(n, n_fft, hop), n_fft, hop);
    // spectra of the S estimates and the mix (Re and Im), the frames of the S outputs, the window squares, alignment room
    return 2 * (int64_t)(S + 1) * C * nb * (n_fft / 2 + 1) + (int64_t)S * C * nb * n_fft + 2 * (int64_t)n_fft + 2;
}

// doubles of the EM statistics: R of every iteration, and the partial sums of one block
long long wiener_doubles(int32_t S, int32_t C, int32_t n_fft, int32_t iterations) {
    const long long SQK = (long long)S * (C * C + 1) * (n_fft / 2 + 1);
    return iterations ? (iterations + WUN_PF_FRAMES / WUN_WF_CHUNK) * SQK : 0;
}

int64_t wiener_scratch_entry(const char* who, int tr, int32_t S, int64_t n, int32_t C, int32_t n_fft, int32_t hop, int32_t iterations) {
    const int64_t floats = mask_scratch_entry(who, tr, S, n, C, n_fft, hop);
    if (floats < 0) return floats;
    if (iterations < 0 || iterations > WUN_WF_MAX_ITERS) return fail(WUN_ERR_INVALID, std::string(who) + ": iterations outside 0..4");
    return floats + 2 * wiener_doubles(S, C, n_fft, iterations);
}

// the kernels of C channels (C is 1 or 2: check_audio)
void launch_apply(int32_t C, const float* xre, const float* xim, float* yre, float* yim, const double* R, long long NK, int32_t S, int K,
                  int niter, double sq, hipStream_t s) {
    hipLaunchKernelGGL(C == 2 ? wiener_apply_kernel<2> : wiener_apply_kernel<1>, dim3((unsigned)((NK + WUN_STFT_BLOCK - 1) / WUN_STFT_BLOCK)),
                       dim3(WUN_STFT_BLOCK), 0, s, xre, xim, yre, yim, R, NK, S, K, niter, sq);
}

void launch_stats(int32_t C, const float* yre, const float* yim, double* part, double* stat, int32_t S, int nf, int K, bool first,
                  bool last, double eps, hipStream_t s) {
    const int nch = (nf + WUN_WF_CHUNK - 1) / WUN_WF_CHUNK;
    const long long lanes = (long long)S * nch * K;
    hipLaunchKernelGGL(C == 2 ? wiener_stats_kernel<2> : wiener_stats_kernel<1>, dim3((unsigned)((lanes + WUN_STFT_BLOCK - 1) / WUN_STFT_BLOCK)),
                       dim3(WUN_STFT_BLOCK), 0, s, yre, yim, part, S, nf, K);
    hipLaunchKernelGGL(C == 2 ? wiener_reduce_kernel<5> : wiener_reduce_kernel<2>, dim3((unsigned)((S * K + WUN_STFT_BLOCK - 1) / WUN_STFT_BLOCK)),
                       dim3(WUN_STFT_BLOCK), 0, s, part, stat, S, K, nch, first ? 1 : 0, last ? 1 : 0, eps);
}

// what the two filters check first, in this order; `eps_name` is the entry's own name of the mask's eps
int check_mask_args(const char* who, int tr, const float* mix_tc, const float* ests, int32_t S, int64_t n, int32_t C, int32_t n_fft,
                    int32_t hop, int32_t power, float eps, const char* eps_name, const float* table_dev, const float* out,
                    const float* scratch) {
    if (!mix_tc || !ests || !table_dev || !out || !scratch) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    int rc;
    if ((rc = check_filter(who, tr, S, n, C, n_fft, hop))) return rc;
    if (power != 1 && power != 2) return fail(WUN_ERR_INVALID, std::string(who) + ": power must be 1 or 2");
    if (!(eps > 0.f) || !std::isfinite(eps)) return fail(WUN_ERR_INVALID, std::string(who) + ": " + eps_name + " not positive or not finite");
    const long long N = (long long)S * n * C;
    if (overlaps(out, N, mix_tc, n * C) || overlaps(out, N, ests, N))
        return fail(WUN_ERR_INVALID, std::string(who) + ": out overlaps an input");
    return WUN_OK;
}

// The one body of wun_mask_filter and wun_wiener_filter, arguments checked: `iterations` EM steps between the mask and the
// inverse.  With none it launches the soft mask alone -- no statistics, no apply -- and never reads em_eps.
int filter_body(const char* who, int tr, const float* mix_tc, const float* ests, int32_t S, int64_t n, int32_t C, int32_t n_fft,
                int32_t hop, int32_t power, float mask_eps, int32_t iterations, float em_eps, const float* table_dev, float* out,
                float* scratch, void* stream) {
    int rc;
    hipStream_t s = (hipStream_t)stream;
    const int K = n_fft / 2 + 1, lead = n_fft - hop;
    const long long F = centered_frames(n, n_fft, hop), nbmax = block_frames(F, n_fft, hop);
    const long long Ee = (long long)S * C * nbmax * K, Ex = (long long)C * nbmax * K;
    float* ere = scratch; float* eim = ere + Ee; float* xre = eim + Ee; float* xim = xre + Ex; float* frames = xim + Ex;
    double* wsq = f64_tail(frames, (long long)S * C * nbmax * n_fft);
    const long long SQK = (long long)S * (C * C + 1) * K;
    double* R = wsq + n_fft;                                  // [iterations][S][Q][K]
    double* part = R + iterations * SQK;                      // [WUN_PF_FRAMES / WUN_WF_CHUNK][S][Q][K]
    const double eps_d = (double)em_eps, sq = std::sqrt(eps_d);
    launch_window(wsq, n_fft, s);
    // pass i < iterations: y^(i) of every frame, block by block (no overlap frames: each frame counts once), into the
    // statistics of R^(i+1); a frame's y^(i) depends on that frame and the R's alone, so nothing track-long is kept
    for (int it = 0; it < iterations; ++it)
        for (long long f0 = 0; f0 < F; f0 += WUN_PF_FRAMES) {
            const long long f1 = f0 + WUN_PF_FRAMES < F ? f0 + WUN_PF_FRAMES : F, nb = f1 - f0;
            if ((rc = launch_cfwd(tr, ests, (long long)S * C, ere, eim, mix_tc, C, xre, xim, table_dev, n, C, n_fft, hop, lead, nb, f0, nb, 0, s))) return rc;
            launch_mask(xre, xim, ere, eim, (long long)C * nb * K, S, power, mask_eps, s);
            if (it) launch_apply(C, xre, xim, ere, eim, R, nb * K, S, K, it, sq, s);
            launch_stats(C, ere, eim, part, R + it * SQK, S, (int)nb, K, f0 == 0, f1 == F, eps_d, s);
        }
    // the last pass: forward, mask, all the filters, inverse, overlap-add of every block in which a sample ends
    for (long long f0 = 0; f0 < F; f0 += WUN_PF_FRAMES) {
        const Blk b = block_of(f0, F, n, n_fft, hop, lead);
        if (b.t_lo >= b.t_hi) continue;
        if ((rc = launch_cfwd(tr, ests, (long long)S * C, ere, eim, mix_tc, C, xre, xim, table_dev, n, C, n_fft, hop, lead, b.nb, b.fb0, b.nb, 0, s))) return rc;
        // (a short last block packs its spectra: the source stride is C nb K)
        launch_mask(xre, xim, ere, eim, (long long)C * b.nb * K, S, power, mask_eps, s);
        if (iterations) launch_apply(C, xre, xim, ere, eim, R, b.nb * K, S, K, iterations, sq, s);
        if ((rc = launch_gemm(tr, ere, eim, table_dev, frames, (long long)S * C, b.nb, b.nb, 0, n_fft, s))) return rc;
        launch_ola(frames, wsq, out, S, n, C, F, b, n_fft, hop, lead, s);
    }
    return launch_status(who);
}

int mask_filter_entry(const char* who, int tr, const float* mix_tc, const float* ests, int32_t S, int64_t n, int32_t C, int32_t n_fft,
                      int32_t hop, int32_t power, float eps, const float* table_dev, float* out, float* scratch, void* stream) {
    int rc;
    if ((rc = check_mask_args(who, tr, mix_tc, ests, S, n, C, n_fft, hop, power, eps, "eps", table_dev, out, scratch))) return rc;
    return filter_body(who, tr, mix_tc, ests, S, n, C, n_fft, hop, power, eps, 0, 0.f, table_dev, out, scratch, stream);
}

int wiener_filter_entry(const char* who, int tr, const float* mix_tc, const float* ests, int32_t S, int64_t n, int32_t C, int32_t n_fft,
                        int32_t hop, int32_t power, float mask_eps, int32_t iterations, float eps, const float* table_dev, float* out,
                        float* scratch, void* stream) {
    int rc;
    if ((rc = check_mask_args(who, tr, mix_tc, ests, S, n, C, n_fft, hop, power, mask_eps, "mask_eps", table_dev, out, scratch))) return rc;
    if (iterations < 0 || iterations > WUN_WF_MAX_ITERS) return fail(WUN_ERR_INVALID, std::string(who) + ": iterations outside 0..4");
    if (!(eps > 0.f) || !std::isfinite(eps)) return fail(WUN_ERR_INVALID, std::string(who) + ": eps not positive or not finite");
    return filter_body(who, tr, mix_tc, ests, S, n, C, n_fft, hop, power, mask_eps, iterations, eps, table_dev, out, scratch, stream);
}

}  // namespace

// ---- the C ABI: every entry on the GEMM (the table of wun_stft_design, n_fft <= 2048) and on the FFT (wun_fft_design, <= 8192) ----
extern "C" int64_t wun_stft_centered_frames(int64_t T, int32_t n_fft, int32_t hop) {
    return centered_frames_entry("wun_stft_centered_frames", WUN_TR_GEMM, T, n_fft, hop);
}
extern "C" int64_t wun_fft_frames(int64_t T, int32_t n_fft, int32_t hop) {      // wun_stft_frames for the FFT's n_fft list
    int rc;
    if ((rc = check_res("wun_fft_frames", WUN_TR_FFT, n_fft, hop))) return rc;
    if (T < n_fft || T > ((int64_t)1 << 40)) return fail(WUN_ERR_INVALID, "wun_fft_frames: T below n_fft or above 2^40");
    return 1 + (T - n_fft) / hop;
}
extern "C" int64_t wun_fft_centered_frames(int64_t T, int32_t n_fft, int32_t hop) {
    return centered_frames_entry("wun_fft_centered_frames", WUN_TR_FFT, T, n_fft, hop);
}

extern "C" int wun_stft_complex(const float* x, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                                int32_t lead, int64_t F, const float* table_dev, float* re, float* im, void* stream) {
    return stft_complex_entry("wun_stft_complex", WUN_TR_GEMM, x, S, B, T, C, n_fft, hop, lead, F, table_dev, re, im, stream);
}
extern "C" int wun_stft_complex_fft(const float* x, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                                    int32_t lead, int64_t F, const float* table_dev, float* re, float* im, void* stream) {
    return stft_complex_entry("wun_stft_complex_fft", WUN_TR_FFT, x, S, B, T, C, n_fft, hop, lead, F, table_dev, re, im, stream);
}

extern "C" int64_t wun_istft_scratch_floats(int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop, int32_t lead,
                                            int64_t F) {
    return istft_scratch_entry("wun_istft_scratch_floats", WUN_TR_GEMM, S, B, T, C, n_fft, hop, lead, F);
}
extern "C" int64_t wun_istft_fft_scratch_floats(int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop, int32_t lead,
                                                int64_t F) {
    return istft_scratch_entry("wun_istft_fft_scratch_floats", WUN_TR_FFT, S, B, T, C, n_fft, hop, lead, F);
}

extern "C" int wun_istft(const float* re, const float* im, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                         int32_t lead, int64_t F, const float* table_dev, float* y, float* scratch, void* stream) {
    return istft_entry("wun_istft", WUN_TR_GEMM, re, im, S, B, T, C, n_fft, hop, lead, F, table_dev, y, scratch, stream);
}
extern "C" int wun_istft_fft(const float* re, const float* im, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                             int32_t lead, int64_t F, const float* table_dev, float* y, float* scratch, void* stream) {
    return istft_entry("wun_istft_fft", WUN_TR_FFT, re, im, S, B, T, C, n_fft, hop, lead, F, table_dev, y, scratch, stream);
}

// tf.contrib.signal.inverse_stft with inverse_stft_window_fn(hop): wun_istft in the loss's framing (lead 0) with the
// steady-state normaliser; the scratch is wun_istft's
namespace {
int64_t istft_tf_scratch_entry(const char* who, int tr, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop, int64_t F) {
    const int64_t n = istft_scratch_entry(who, tr, S, B, T, C, n_fft, hop, 0, F);
    if (n < 0) return n;
    const int rc = check_steady(who, n_fft, hop);
    return rc ? rc : n;
}
}  // namespace
extern "C" int64_t wun_istft_tf_scratch_floats(int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop, int64_t F) {
    return istft_tf_scratch_entry("wun_istft_tf_scratch_floats", WUN_TR_GEMM, S, B, T, C, n_fft, hop, F);
}
extern "C" int64_t wun_istft_tf_fft_scratch_floats(int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop, int64_t F) {
    return istft_tf_scratch_entry("wun_istft_tf_fft_scratch_floats", WUN_TR_FFT, S, B, T, C, n_fft, hop, F);
}
extern "C" int wun_istft_tf(const float* re, const float* im, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                            int64_t F, const float* table_dev, float* y, float* scratch, void* stream) {
    return istft_entry("wun_istft_tf", WUN_TR_GEMM, re, im, S, B, T, C, n_fft, hop, 0, F, table_dev, y, scratch, stream, true);
}
extern "C" int wun_istft_tf_fft(const float* re, const float* im, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                                int64_t F, const float* table_dev, float* y, float* scratch, void* stream) {
    return istft_entry("wun_istft_tf_fft", WUN_TR_FFT, re, im, S, B, T, C, n_fft, hop, 0, F, table_dev, y, scratch, stream, true);
}

// ---- Griffin-Lim (include/wun.h): istft_entry's blocks, window squares and overlap-add around gl_frame_kernel ----
// scratch: the frames of one block, the second audio buffer, c_{i-1} (Re, Im) with momentum; float64 tail: the window squares,
// then the frames' partial sums [R][F][2]
namespace {
int check_griffin_lim(const char* who, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop, int32_t lead, int64_t F) {
    int rc;
    if ((rc = check_audio(who, S, B, T, C))) return rc;
    if ((rc = check_res(who, WUN_TR_FFT, n_fft, hop))) return rc;
    return check_framing(who, S, B, C, n_fft, lead, F);
}
}  // namespace

extern "C" int64_t wun_griffin_lim_scratch_floats(int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop, int32_t lead,
                                                  int64_t F, int32_t momentum_nonzero) {
    const int rc = check_griffin_lim("wun_griffin_lim_scratch_floats", S, B, T, C, n_fft, hop, lead, F);
    if (rc) return rc;
    const int64_t R = (int64_t)S * B * C, K = n_fft / 2 + 1;
    return R * block_frames(F, n_fft, hop) * n_fft + R * T + (momentum_nonzero ? 2 * R * F * K : 0) + 2 * (int64_t)n_fft + 4 * R * F + 2;
}

extern "C" int wun_griffin_lim(const float* mag, const float* init_re, const float* init_im, const float* y_init, int32_t S, int32_t B,
                               int64_t T, int32_t C, int32_t n_fft, int32_t hop, int32_t lead, int64_t F, int32_t iterations,
                               float momentum, const float* table_dev, float* y, double* inconsistency, float* scratch, void* stream) {
    const char* who = "wun_griffin_lim";
    if (!mag || !table_dev || !y || !scratch) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    int rc;
    if ((rc = check_griffin_lim(who, S, B, T, C, n_fft, hop, lead, F))) return rc;
    if (iterations < 1) return fail(WUN_ERR_INVALID, std::string(who) + ": iterations < 1");
    if (!(momentum >= 0.f && momentum < 1.f)) return fail(WUN_ERR_INVALID, std::string(who) + ": momentum outside [0, 1)");
    const bool given = init_re && init_im;
    if ((init_re != nullptr) != (init_im != nullptr) || given == (y_init != nullptr))
        return fail(WUN_ERR_INVALID, std::string(who) + ": exactly one of (init_re and init_im) and y_init must be given");
    const long long R = (long long)S * B * C, K = n_fft / 2 + 1, E = R * F * K, NT = R * T;
    if (overlaps(y, NT, mag, E) || (given && (overlaps(y, NT, init_re, E) || overlaps(y, NT, init_im, E))))
        return fail(WUN_ERR_INVALID, std::string(who) + ": y overlaps mag or the initial spectrum");

    hipStream_t s = (hipStream_t)stream;
    const long long fr_floats = R * block_frames(F, n_fft, hop) * n_fft;
    float* frames = scratch;
    float* alt = scratch + fr_floats;
    float* pre = momentum != 0.f ? alt + NT : nullptr;
    float* pim = pre ? pre + E : nullptr;
    double* wsq = f64_tail(scratch, fr_floats + NT + (pre ? 2 * E : 0));
    double* part = wsq + n_fft;
    launch_window(wsq, n_fft, s);
    // iteration i writes y when an even number of iterations follows it, the second buffer otherwise
    const float* src = y_init;
    if (!given && (iterations & 1) && overlaps(y_init, NT, y, NT)) {         // iteration 0 would write what it reads
        const hipError_t e = hipMemcpyAsync(alt, y_init, 4 * (size_t)NT, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return fail(WUN_ERR_HIP, std::string(who) + " copy: " + hipGetErrorString(e));
        src = alt;
    }
    const int ov = overlap_frames(n_fft, hop);
    for (int it = 0; it < iterations; ++it) {
        float* dst = ((iterations - 1 - it) & 1) ? alt : y;
        const bool giv = given && it == 0;
        for (long long f0 = 0; f0 < F; f0 += WUN_PF_FRAMES) {                // (every block: its frames' c_i and sums are needed
            const Blk b = block_of(f0, F, T, n_fft, hop, lead);              //  even where no sample ends in it)
            GlArgs a;
            a.x = giv ? nullptr : src; a.cre = giv ? init_re : nullptr; a.cim = giv ? init_im : nullptr; a.mag = mag;
            a.pre = pre; a.pim = pim; a.part = inconsistency && !giv ? part : nullptr; a.table = table_dev; a.frames = frames;
            a.M = R * b.nb; a.nb = b.nb; a.f0 = b.fb0; a.F = F; a.T = T;
            a.last_below = f0 + WUN_PF_FRAMES < F ? f0 + WUN_PF_FRAMES - ov : (long long)F;
            a.C = C; a.n_fft = n_fft; a.hop = hop; a.lead = lead; a.K = (int)K; a.first = it == 0;
            a.momentum = momentum; a.scale = 1.f / (float)n_fft;
            if ((rc = fft_launch_griffin_lim(a, giv, s))) return rc;
            if (b.t_lo < b.t_hi) launch_ola(frames, wsq, dst, (long long)S * B, T, C, F, b, n_fft, hop, lead, s);
        }
        if (inconsistency) launch_gl_finish(part, giv ? -1 : R * F, inconsistency + 2 * it, s);
        src = dst;
    }
    return launch_status(who);
}

extern "C" int64_t wun_mask_filter_scratch_floats(int32_t S, int64_t n, int32_t C, int32_t n_fft, int32_t hop) {
    return mask_scratch_entry("wun_mask_filter_scratch_floats", WUN_TR_GEMM, S, n, C, n_fft, hop);
}
extern "C" int64_t wun_mask_filter_fft_scratch_floats(int32_t S, int64_t n, int32_t C, int32_t n_fft, int32_t hop) {
    return mask_scratch_entry("wun_mask_filter_fft_scratch_floats", WUN_TR_FFT, S, n, C, n_fft, hop);
}

extern "C" int wun_mask_filter(const float* mix_tc, const float* ests, int32_t S, int64_t n, int32_t C, int32_t n_fft, int32_t hop,
                               int32_t power, float eps, const float* table_dev, float* out, float* scratch, void* stream) {
    return mask_filter_entry("wun_mask_filter", WUN_TR_GEMM, mix_tc, ests, S, n, C, n_fft, hop, power, eps, table_dev, out, scratch,
                             stream);
}
extern "C" int wun_mask_filter_fft(const float* mix_tc, const float* ests, int32_t S, int64_t n, int32_t C, int32_t n_fft, int32_t hop,
                                   int32_t power, float eps, const float* table_dev, float* out, float* scratch, void* stream) {
    return mask_filter_entry("wun_mask_filter_fft", WUN_TR_FFT, mix_tc, ests, S, n, C, n_fft, hop, power, eps, table_dev, out, scratch,
                             stream);
}

extern "C" int64_t wun_wiener_filter_scratch_floats(int32_t S, int64_t n, int32_t C, int32_t n_fft, int32_t hop, int32_t iterations) {
    return wiener_scratch_entry("wun_wiener_filter_scratch_floats", WUN_TR_GEMM, S, n, C, n_fft, hop, iterations);
}
extern "C" int64_t wun_wiener_filter_fft_scratch_floats(int32_t S, int64_t n, int32_t C, int32_t n_fft, int32_t hop,
                                                        int32_t iterations) {
    return wiener_scratch_entry("wun_wiener_filter_fft_scratch_floats", WUN_TR_FFT, S, n, C, n_fft, hop, iterations);
}

extern "C" int wun_wiener_filter(const float* mix_tc, const float* ests, int32_t S, int64_t n, int32_t C, int32_t n_fft, int32_t hop,
                                 int32_t power, float mask_eps, int32_t iterations, float eps, const float* table_dev, float* out,
                                 float* scratch, void* stream) {
    return wiener_filter_entry("wun_wiener_filter", WUN_TR_GEMM, mix_tc, ests, S, n, C, n_fft, hop, power, mask_eps, iterations, eps,
                               table_dev, out, scratch, stream);
}
extern "C" int wun_wiener_filter_fft(const float* mix_tc, const float* ests, int32_t S, int64_t n, int32_t C, int32_t n_fft,
                                     int32_t hop, int32_t power, float mask_eps, int32_t iterations, float eps,
                                     const float* table_dev, float* out, float* scratch, void* stream) {
    return wiener_filter_entry("wun_wiener_filter_fft", WUN_TR_FFT, mix_tc, ests, S, n, C, n_fft, hop, power, mask_eps, iterations, eps,
                               table_dev, out, scratch, stream);
}
