// gfx950 (MI355X / CDNA4): the FFT path of the complex STFT and its inverse (include/wun.h: wun_fft_design, wun_stft_complex_fft,
// wun_istft_fft and the *_fft filters).  Same definitions and layouts as stft_cfwd_kernel / istft_gemm_kernel of
// wun_postfilter.hip, whose host code launches these through wun_fft.h; O(n log n) per frame instead of O(n^2).  The spectral
// loss's two frame transforms (wun_spectral_loss_fft and its kin) are the same two bodies: the forward one with
// the magnitude as its epilogue, the inverse one as the unscaled adjoint.  The spectrogram U-Net's backward from an audio gradient
// (wun_spec_backward) is the forward body once more, on d_audio / D, with the mask gradient as its epilogue.
// Griffin-Lim (wun_griffin_lim) runs both transforms of a frame in one workgroup, the projection between them.
// The phase vocoder's analysis (wun_time_stretch) is the forward body twice per frame, one hop apart.
//
//   real transform   a frame of n_fft real samples is one complex FFT of M = n_fft / 2 points, z[m] = y[2m] + i y[2m+1], and a
//                    split step:  E = (Z[k] + conj Z[M-k]) / 2,  O = (Z[k] - conj Z[M-k]) / 2i,  X[k] = E + W_N^k O,  k = 0..M
//   complex FFT      Stockham autosort, radix 4 with one radix-2 stage last when log2 M is odd.  Stage Ns (1, 4, 16, ..):
//                    butterfly j reads in[j + r M/4], multiplies by W^(r (j mod Ns) M / 4Ns), r = 1..3, and writes
//                    out[(j / Ns) 4 Ns + (j mod Ns) + p Ns].  The radix points live in registers, the stages ping-pong between
//                    two LDS images: one barrier per stage.  The first stage takes its points straight from global memory.
//   inverse          Z'[k] = (X[k] + conj X[M-k]) + i conj(W_N^k) (X[k] - conj X[M-k]) (twice the Z of the forward), the
//                    same FFT on Z' with Re and Im swapped (that is the inverse transform with Re and Im swapped), then
//                    frame[2m], frame[2m+1] = Im, Re of the result, times 1 / n_fft (a power of two) and the window.
//   LDS              Re and Im planes of floats (ds_read_b32 / ds_write_b32: 32 banks, lane groups of 32).  Float a of a plane
//                    lies at a ^ f(a >> 5), f(b) = 5 (b & 3) ^ ((b & 2) << 3): a permutation inside each aligned run of 32
//                    floats, so the stride-1 stage reads stay conflict-free, and the scattered stage writes (stride 4 at
//                    Ns = 1, runs of 4 at stride 16 at Ns = 4, runs of 16 at stride 64 at Ns = 16) land on 32 different banks.
//                    No padding: 8192 points take 2 x 2 x 4096 floats = 64 KB.  (DESIGN.md 5.13 has the conflict degrees.)
//   mapping          min(256, M / 4) lanes per frame: 32 .. 2 frames per 256-lane workgroup at n_fft 64 .. 1024, one frame
//                    (1 .. 4 butterflies per lane and stage) above.  A frame's lanes and LDS region are its own and the
//                    instruction sequence is one: its bits do not depend on the frames beside it, the grid or alignment.
//
// Twiddles and the window come from the host's table (float64, rounded once); no sincosf, no recurrence, no atomics.
// Built WITHOUT the packed fp32 VALU instructions, as wun_postfilter.hip (csrc/Makefile NO_PK_FP32).
#include "wun_fft.h"
#include "../../include/wun.h"

#include <atomic>
#include <cmath>
#include <string>
#include <type_traits>

using namespace wun;
int fail(int code, const std::string& msg);      // wun_plan.hip

#define WUN_FFT_BLOCK 256

namespace wun {

template <int LOGM>
struct FftGeom {
    static constexpr int M = 1 << LOGM, N = 2 * M;
    static constexpr int TPF = M / 4 < WUN_FFT_BLOCK ? M / 4 : WUN_FFT_BLOCK;      // lanes per frame
    static constexpr int FPW = WUN_FFT_BLOCK / TPF;                                 // frames per workgroup
    static constexpr int BPT = M / 4 / TPF;                                         // radix-4 butterflies per lane and stage
    static constexpr int PLANE = FPW * M;                                           // floats of one LDS plane
    static constexpr int STAGES = (LOGM + 1) / 2;
    static constexpr int RESULT = (STAGES - 1) & 1;                                 // the image the last stage writes
};

__device__ __forceinline__ int fft_swz(int a) {
    const int b = a >> 5;
    return a ^ (((b & 3) * 5) ^ ((b & 2) << 3));
}

// The M-point FFT of one frame: `load(a, re, im)` gives point a (the first stage reads nothing else); the result lies in image
// FftGeom::RESULT at fft_swz(base + k), natural order, behind a barrier.  tw: cos(2 pi t / N) at [t], -sin at [N + t].
// FLIP = 1 swaps the roles of the two images (the first stage writes image 1, the result lies in RESULT ^ 1): the same
// instructions on the same values.
template <int LOGM, int FLIP = 0, class Load>
__device__ __forceinline__ void fft_run(Load load, float (*sre)[FftGeom<LOGM>::PLANE], float (*sim)[FftGeom<LOGM>::PLANE], int base,
                                        int tl, const float* __restrict__ tw) {
    using G = FftGeom<LOGM>;
    constexpr int M = G::M, N = G::N, TPF = G::TPF;
#pragma unroll
    for (int s = 0; s < LOGM / 2; ++s) {
        const int Ns = 1 << (2 * s);
        const float* __restrict__ ir = sre[(s & 1) ^ 1 ^ FLIP];
        const float* __restrict__ ii = sim[(s & 1) ^ 1 ^ FLIP];
        float* __restrict__ outr = sre[(s & 1) ^ FLIP];
        float* __restrict__ outi = sim[(s & 1) ^ FLIP];
#pragma unroll
        for (int i = 0; i < G::BPT; ++i) {
            const int j = tl + i * TPF, k = j & (Ns - 1);
            float vr[4], vi[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int a = j + r * (M / 4);
                if (s == 0) load(a, vr[r], vi[r]);
                else { vr[r] = ir[fft_swz(base + a)]; vi[r] = ii[fft_swz(base + a)]; }
            }
            if (s > 0) {
#pragma unroll
                for (int r = 1; r < 4; ++r) {
                    const int t = 2 * r * k * (M / (4 * Ns));                // W_M^(..) in the table of W_N
                    const float c = tw[t], sn = tw[N + t];
                    const float xr = vr[r] * c - vi[r] * sn, xi = vr[r] * sn + vi[r] * c;
                    vr[r] = xr; vi[r] = xi;
                }
            }
            const float a0r = vr[0] + vr[2], a0i = vi[0] + vi[2], a1r = vr[0] - vr[2], a1i = vi[0] - vi[2];
            const float a2r = vr[1] + vr[3], a2i = vi[1] + vi[3];
            const float a3r = vi[1] - vi[3], a3i = vr[3] - vr[1];            // -i (v1 - v3)
            const int j0 = ((j - k) << 2) + k + base;
            outr[fft_swz(j0)] = a0r + a2r;           outi[fft_swz(j0)] = a0i + a2i;
            outr[fft_swz(j0 + Ns)] = a1r + a3r;      outi[fft_swz(j0 + Ns)] = a1i + a3i;
            outr[fft_swz(j0 + 2 * Ns)] = a0r - a2r;  outi[fft_swz(j0 + 2 * Ns)] = a0i - a2i;
            outr[fft_swz(j0 + 3 * Ns)] = a1r - a3r;  outi[fft_swz(j0 + 3 * Ns)] = a1i - a3i;
        }
        __syncthreads();
    }
    if (LOGM & 1) {                                                          // the radix-2 stage, Ns = M / 2
        constexpr int s = LOGM / 2;
        const float* __restrict__ ir = sre[(s & 1) ^ 1 ^ FLIP];
        const float* __restrict__ ii = sim[(s & 1) ^ 1 ^ FLIP];
        float* __restrict__ outr = sre[(s & 1) ^ FLIP];
        float* __restrict__ outi = sim[(s & 1) ^ FLIP];
#pragma unroll
        for (int i = 0; i < 2 * G::BPT; ++i) {
            const int j = tl + i * TPF;
            const float ar = ir[fft_swz(base + j)], ai = ii[fft_swz(base + j)];
            const float br = ir[fft_swz(base + j + M / 2)], bi = ii[fft_swz(base + j + M / 2)];
            const float c = tw[2 * j], sn = tw[N + 2 * j];
            const float xr = br * c - bi * sn, xi = br * sn + bi * c;
            outr[fft_swz(base + j)] = ar + xr;          outi[fft_swz(base + j)] = ai + xi;
            outr[fft_swz(base + j + M / 2)] = ar - xr;  outi[fft_swz(base + j + M / 2)] = ai - xi;
        }
        __syncthreads();
    }
}

// The forward transform of workgroup blockIdx.x's FPW frame rows of signal z = blockIdx.z (frame row m of StftCfwdArgs, as
// stft_cfwd_kernel): store(z, e, re, im) is called once for every frame row m < M[z] and bin k = 0..n_fft / 2, e = the float
// index of that bin in the [.][K] arrays; im of the bins 0 and n_fft / 2 is exactly 0.  The whole kernel body: it returns for
// the workgroups and frame slots behind the last row.
template <int LOGM, class Store>
__device__ __forceinline__ void fft_fwd_frames(const StftCfwdArgs& p, Store store) {
    using G = FftGeom<LOGM>;
    constexpr int M = G::M, N = G::N, TPF = G::TPF;
    __shared__ float sre[2][G::PLANE];
    __shared__ float sim[2][G::PLANE];
    const int z = blockIdx.z;
    const long long Mrows = p.M[z];
    const long long m0 = (long long)blockIdx.x * G::FPW;
    if (m0 >= Mrows) return;                                 // (the grid is sized by the larger signal; uniform)
    const int g = threadIdx.x / TPF, tl = threadIdx.x - g * TPF, base = g * M;
    const long long m = m0 + g;
    const bool valid = m < Mrows;                            // a frame slot behind the last row runs on zeros, stores nothing
    long long rbase = 0, t0 = 0, o = 0;
    if (valid) {
        const long long r = m / p.nb, fl = m - r * p.nb;
        const long long sb = r / p.C, c = r - sb * p.C;
        rbase = sb * p.T * p.C + c;
        t0 = (p.f0 + fl) * p.hop - p.lead;
        o = (r * p.fstride + p.foff + fl) * p.K;
    }
    const float* __restrict__ x = p.x[z];
    const float* __restrict__ tw = p.table;
    const float* __restrict__ win = p.table + 2 * N;
    const long long T = p.T;
    const int C = p.C;
    fft_run<LOGM>([&](int a, float& re, float& im) {
        const long long t = t0 + 2 * a;
        re = (valid && t >= 0 && t < T) ? x[rbase + t * C] * win[2 * a] : 0.f;
        im = (valid && t + 1 >= 0 && t + 1 < T) ? x[rbase + (t + 1) * C] * win[2 * a + 1] : 0.f;
    }, sre, sim, base, tl, tw);
    if (!valid) return;                                      // (no barrier follows)
    const float* __restrict__ Zr = sre[G::RESULT];
    const float* __restrict__ Zi = sim[G::RESULT];
#pragma unroll
    for (int i = 0; i <= M / TPF; ++i) {
        const int k = tl + i * TPF;                          // 0 .. M: the last round is lane 0's k = M
        if (k > M) break;
        const int ka = base + (k & (M - 1)), kb = base + ((M - k) & (M - 1));
        const float ar = Zr[fft_swz(ka)], ai = Zi[fft_swz(ka)], cr = Zr[fft_swz(kb)], ci = Zi[fft_swz(kb)];
        const float er = 0.5f * (ar + cr), ei = 0.5f * (ai - ci), odr = 0.5f * (ai + ci), odi = 0.5f * (cr - ar);
        const float wc = tw[k], ws = tw[N + k];
        const float xr = er + (wc * odr - ws * odi);
        const float xi = (k == 0 || k == M) ? 0.f : ei + (wc * odi + ws * odr);
        store(z, o + k, xr, xi);
    }
}

// grid: x = group of FPW frame rows, z = signal.  Re and Im of every bin: wun_stft_complex_fft and the filters' analysis.
template <int LOGM>
__global__ __launch_bounds__(WUN_FFT_BLOCK) void stft_fft_kernel(StftCfwdArgs p) {
    fft_fwd_frames<LOGM>(p, [&](int z, long long e, float re, float im) { p.re[z][e] = re; p.im[z][e] = im; });
}

// The same grid and body with the loss's epilogue (stft_fwd_kernel / stft_fwd_parts_kernel of wun_spectral.hip): the magnitude
// of every bin, and Re / Im of the signals whose p.a.re[z] is not null.  The framing is p.a's (the loss: lead 0, whole frames).
template <int LOGM>
__global__ __launch_bounds__(WUN_FFT_BLOCK) void stft_fft_mag_kernel(StftMagArgs p) {
    fft_fwd_frames<LOGM>(p.a, [&](int z, long long e, float re, float im) {
        p.mag[z][e] = sqrtf(fmaf(re, re, im * im));          // (spelled out as in wun_spectral.hip: which product is fused decides the bits)
        if (p.a.re[z] != nullptr) { p.a.re[z][e] = re; p.a.im[z][e] = im; }
    });
}

// The same grid and body on u = d_audio / D with the mask gradient of the spectrogram U-Net as its epilogue (SpecHeadArgs,
// DESIGN.md 5.20): G = STFT(u) is consumed in registers; the epilogue adds loads of X, M, the mask and d_mags at the lane's own
// bin, no LDS and no barrier.
template <int LOGM>
__global__ __launch_bounds__(WUN_FFT_BLOCK) void spec_head_fft_kernel(SpecHeadArgs p) {
    const int K = p.a.K;
    fft_fwd_frames<LOGM>(p.a, [&](int, long long e, float re, float im) {
        const long long bf = e / K;
        const int k = (int)(e - bf * K);
        if (k == K - 1) return;                              // the dropped bin: no gradient
        const float ga = (k == 0 ? p.c_edge : p.c_mid) * fmaf(p.xre[e], re, p.xim[e] * im);
        const float dm = p.dmags != nullptr ? fmaf(p.dmags[e], p.mag[e], ga) : ga;
        const float mk = p.mask[bf * (K - 1) + k];
        p.dz[bf * (K - 1) + k] = dm * (mk * (1.0f - mk));
    });
}

// D[p] of wun_istft_tf: window_sq_kernel's squares (cospi, float64) summed over the places p + i hop of a frame, i ascending,
// rounded once -- the float istft_ola_kernel<true> divides by
__global__ __launch_bounds__(WUN_FFT_BLOCK) void steady_den_kernel(float* __restrict__ D, int n_fft, int hop) {
    const int p = blockIdx.x * WUN_FFT_BLOCK + threadIdx.x;
    if (p >= hop) return;
    double ws = 0.0;
    for (int n = p; n < n_fft; n += hop) {
        const double w = 0.5 - 0.5 * cospi(2.0 * (double)n / (double)n_fft);
        ws += w * w;
    }
    D[p] = (float)ws;
}

// one lane per sample (grid-stride, one writer per float): u = g / D[t mod hop]
__global__ __launch_bounds__(WUN_FFT_BLOCK) void steady_divide_kernel(const float* __restrict__ g, const float* __restrict__ D,
                                                                     float* __restrict__ u, long long N, long long T, int hop) {
    for (long long e = (long long)blockIdx.x * WUN_FFT_BLOCK + threadIdx.x; e < N; e += (long long)gridDim.x * WUN_FFT_BLOCK) {
        const long long t = e % T;
        u[e] = g[e] / D[t % hop];
    }
}

// grid: x = group of FPW frame rows of IstftGemmArgs.  frames[m][n] = w[n] irfft(Re + i Im)[n]; Im of the bins 0 and M is
// never read.  ADJ: the unscaled adjoint of the forward transform instead (stft_bwd_kernel's definition, every bin k = 0..M
// counted ONCE): frames[m][n] = w[n] sum_k re[k] cos(2 pi n k / N) - im[k] sin(2 pi n k / N).  That is the inverse of the spectrum
// whose bins 0 and M are doubled, times N / 2: the k = 0 point takes 2 re[0] and 2 re[M], and the host passes c_edge = 1 / 2
// in place of 1 / N -- powers of two, so exact.
template <int LOGM, bool ADJ>
__global__ __launch_bounds__(WUN_FFT_BLOCK) void istft_fft_kernel(IstftGemmArgs p) {
    using G = FftGeom<LOGM>;
    constexpr int M = G::M, N = G::N, TPF = G::TPF;
    __shared__ float sre[2][G::PLANE];
    __shared__ float sim[2][G::PLANE];
    const int g = threadIdx.x / TPF, tl = threadIdx.x - g * TPF, base = g * M;
    const long long m = (long long)blockIdx.x * G::FPW + g;
    const bool valid = m < p.M;
    long long srow = 0;
    if (valid) {
        const long long r = m / p.nb, fl = m - r * p.nb;
        srow = (r * p.fstride + p.foff + fl) * p.K;
    }
    const float* __restrict__ xr = p.re + srow;
    const float* __restrict__ xi = p.im + srow;
    const float* __restrict__ tw = p.table;
    const float* __restrict__ win = p.table + 2 * N;
    fft_run<LOGM>([&](int k, float& re, float& im) {         // (Re, Im) = (Im Z', Re Z'): the swap that inverts
        if (!valid) { re = 0.f; im = 0.f; return; }
        if (k == 0) {
            const float x0 = ADJ ? 2.f * xr[0] : xr[0], xm = ADJ ? 2.f * xr[M] : xr[M];
            re = x0 - xm; im = x0 + xm;
            return;
        }
        const float ar = xr[k], ai = xi[k], cr = xr[M - k], ci = xi[M - k];
        const float dr = ar - cr, di = ai + ci;
        const float wc = tw[k], ws = tw[N + k];
        const float pr = wc * dr + ws * di, pi = wc * di - ws * dr;          // conj(W_N^k) (X[k] - conj X[M-k])
        re = (ai - ci) + pr; im = (ar + cr) - pi;
    }, sre, sim, base, tl, tw);
    if (!valid) return;
    const float* __restrict__ Yr = sre[G::RESULT];
    const float* __restrict__ Yi = sim[G::RESULT];
    float* __restrict__ fr = p.frames + m * N;
    const float scale = p.c_edge;                            // 1 / n_fft (ADJ: 1 / 2)
#pragma unroll
    for (int i = 0; i < M / TPF; ++i) {
        const int mm = tl + i * TPF;
        fr[2 * mm] = (Yi[fft_swz(base + mm)] * scale) * win[2 * mm];
        fr[2 * mm + 1] = (Yr[fft_swz(base + mm)] * scale) * win[2 * mm + 1];
    }
}

// unit(c) of wun_griffin_lim (include/wun.h), spelled out: which operation is fused decides the bits.  Scaled by the larger
// of |re| and |im|, so nothing overflows or flushes; a NaN (fmaxf drops it, the division brings it back) stays NaN.
__device__ __forceinline__ void gl_unit(float re, float im, float& ur, float& ui) {
    if (re == 0.f && im == 0.f) { ur = 1.f; ui = 0.f; return; }
    const float s = fmaxf(fabsf(re), fabsf(im));
    const float a = re / s, b = im / s;
    const float n = sqrtf(fmaf(a, a, b * b));
    ur = a / n;
    ui = b / n;
}

// One Griffin-Lim iteration of the workgroup's FPW frame rows (GlArgs, wun_fft.h): fft_fwd_frames' transform of
// the windowed samples of y_{i-1}, the split step per bin in registers, the momentum epilogue and the projection
// S = mag unit(t), then istft_fft_kernel's inverse of S -- the spectrum never leaves the workgroup.  S goes to the LDS image the
// forward transform's last stage left free (RESULT ^ 1; bin M is real and takes the imaginary slot of bin 0, so 8192 points
// still take 64 KB); behind ONE barrier the inverse pre-step reads S[k] and S[M-k] from there while its first stage writes the
// image the forward result lay in (fft_run<.., FLIP = RESULT>): the inverse's result is image 0 for every LOGM.  The reads of
// S run along k and against it, both a permutation inside each aligned run of 32 floats under fft_swz: conflict-free but for
// the one lane across a run's edge, as the forward split step.
// GIVEN: c_0 comes from p.cre / p.cim, no forward transform and no partial sums.
// With p.part the frame's two float64 sums leave through image 1, free behind the inverse's last barrier (two more barriers).
template <int LOGM, bool GIVEN>
__global__ __launch_bounds__(WUN_FFT_BLOCK) void gl_frame_kernel(GlArgs p) {
    using G = FftGeom<LOGM>;
    constexpr int M = G::M, N = G::N, TPF = G::TPF, SI = G::RESULT ^ 1;
    __shared__ __attribute__((aligned(16))) float sre[2][G::PLANE];
    __shared__ __attribute__((aligned(16))) float sim[2][G::PLANE];
    const int g = threadIdx.x / TPF, tl = threadIdx.x - g * TPF, base = g * M;
    const long long m = (long long)blockIdx.x * G::FPW + g;
    const bool valid = m < p.M;                              // a frame slot behind the last row runs on zeros, stores nothing
    long long rbase = 0, t0 = 0, row = 0;
    bool last = false;
    if (valid) {
        const long long r = m / p.nb, f = p.f0 + (m - r * p.nb);
        const long long sb = r / p.C, c = r - sb * p.C;
        rbase = sb * p.T * p.C + c;
        t0 = f * p.hop - p.lead;
        row = r * p.F + f;
        last = f < p.last_below;
    }
    const long long o = row * p.K;
    const float* __restrict__ tw = p.table;
    const float* __restrict__ win = p.table + 2 * N;
    if (!GIVEN) {
        const float* __restrict__ x = p.x;
        const long long T = p.T;
        const int C = p.C;
        fft_run<LOGM>([&](int a, float& re, float& im) {     // (fft_fwd_frames' load)
            const long long t = t0 + 2 * a;
            re = (valid && t >= 0 && t < T) ? x[rbase + t * C] * win[2 * a] : 0.f;
            im = (valid && t + 1 >= 0 && t + 1 < T) ? x[rbase + (t + 1) * C] * win[2 * a + 1] : 0.f;
        }, sre, sim, base, tl, tw);
    }
    const float* __restrict__ Zr = sre[G::RESULT];
    const float* __restrict__ Zi = sim[G::RESULT];
    float* Sr = sre[SI];
    float* Si = sim[SI];
    const bool mom = p.pre != nullptr && valid;
    const bool sums = !GIVEN && p.part != nullptr;           // (uniform)
    double d0 = 0.0, d1 = 0.0;
#pragma unroll
    for (int i = 0; i <= M / TPF; ++i) {
        const int k = tl + i * TPF;                          // 0 .. M: the last round is lane 0's k = M
        if (k > M) break;
        float cr, ci;
        if (GIVEN) {
            cr = valid ? p.cre[o + k] : 0.f;
            ci = (valid && k != 0 && k != M) ? p.cim[o + k] : 0.f;
        } else {                                             // (fft_fwd_frames' split step)
            const int ka = base + (k & (M - 1)), kb = base + ((M - k) & (M - 1));
            const float ar = Zr[fft_swz(ka)], ai = Zi[fft_swz(ka)], br = Zr[fft_swz(kb)], bi = Zi[fft_swz(kb)];
            const float er = 0.5f * (ar + br), ei = 0.5f * (ai - bi), odr = 0.5f * (ai + bi), odi = 0.5f * (br - ar);
            const float wc = tw[k], ws = tw[N + k];
            cr = er + (wc * odr - ws * odi);
            ci = (k == 0 || k == M) ? 0.f : ei + (wc * odi + ws * odr);
        }
        const float mg = valid ? p.mag[o + k] : 0.f;
        float tr = cr, ti = ci;
        if (mom) {
            if (!p.first) {
                tr = fmaf(p.momentum, cr - p.pre[o + k], cr);
                ti = fmaf(p.momentum, ci - p.pim[o + k], ci);
            }
            if (last) { p.pre[o + k] = cr; p.pim[o + k] = ci; }
        }
        if (sums) {
            const double a = (double)cr, b = (double)ci, mm = (double)mg;
            const double d = sqrt(a * a + b * b) - mm;
            d0 += d * d;
            d1 += mm * mm;
        }
        float ur, ui;
        gl_unit(tr, ti, ur, ui);
        const float sr = mg * ur, si = mg * ui;
        if (k == M) Si[fft_swz(base)] = sr;
        else {
            Sr[fft_swz(base + k)] = sr;
            if (k != 0) Si[fft_swz(base + k)] = si;
        }
    }
    __syncthreads();
    fft_run<LOGM, G::RESULT>([&](int k, float& re, float& im) {      // (istft_fft_kernel's pre-step, S from LDS)
        if (k == 0) {
            const float x0 = Sr[fft_swz(base)], xm = Si[fft_swz(base)];
            re = x0 - xm; im = x0 + xm;
            return;
        }
        const float ar = Sr[fft_swz(base + k)], ai = Si[fft_swz(base + k)];
        const float cr = Sr[fft_swz(base + M - k)], ci = Si[fft_swz(base + M - k)];
        const float dr = ar - cr, di = ai + ci;
        const float wc = tw[k], ws = tw[N + k];
        const float pr = wc * dr + ws * di, pi = wc * di - ws * dr;
        re = (ai - ci) + pr; im = (ar + cr) - pi;
    }, sre, sim, base, tl, tw);
    if (valid) {
        const float* __restrict__ Yr = sre[0];
        const float* __restrict__ Yi = sim[0];
        float* __restrict__ fr = p.frames + m * N;
        const float scale = p.scale;
#pragma unroll
        for (int i = 0; i < M / TPF; ++i) {
            const int mm = tl + i * TPF;
            fr[2 * mm] = (Yi[fft_swz(base + mm)] * scale) * win[2 * mm];
            fr[2 * mm + 1] = (Yr[fft_swz(base + mm)] * scale) * win[2 * mm + 1];
        }
    }
    if (sums) {                                              // lanes in groups of 8, then the groups, ascending
        double* dp = reinterpret_cast<double*>(&sre[1][0]);  // 2 x 256 doubles <= PLANE floats
        dp[2 * threadIdx.x] = d0;
        dp[2 * threadIdx.x + 1] = d1;
        __syncthreads();
        if ((tl & 7) == 0) {
            double a0 = dp[2 * threadIdx.x], a1 = dp[2 * threadIdx.x + 1];
#pragma unroll
            for (int j = 1; j < 8; ++j) { a0 += dp[2 * (threadIdx.x + j)]; a1 += dp[2 * (threadIdx.x + j) + 1]; }
            dp[2 * threadIdx.x] = a0;
            dp[2 * threadIdx.x + 1] = a1;
        }
        __syncthreads();
        if (tl == 0 && valid && last) {
            double a0 = dp[2 * threadIdx.x], a1 = dp[2 * threadIdx.x + 1];
            for (int j = 8; j < TPF; j += 8) { a0 += dp[2 * (threadIdx.x + j)]; a1 += dp[2 * (threadIdx.x + j) + 1]; }
            p.part[2 * row] = a0;
            p.part[2 * row + 1] = a1;
        }
    }
}

// The analysis of the phase vocoder (wun_time_stretch; VocArgs, wun_fft.h): the workgroup owns FPW synthesis
// frames of one (job, channel), found from the workgroup prefix in the arguments (uniform: scalar loads).  Frame f is analysed at
// a_f = (f hop num) / den and one hop before it: P_f first, fft_fwd_frames' transform and split step with the bins kept in
// registers, then X_f through the same LDS behind one barrier, and per bin the magnitude, the product X conj(P) in float64 (the
// four products of float32 values are exact there, each sum is rounded once whether it is fused or not), its angle in turns less
// the hop's advance, wrapped to [-1/2, 1/2] and rounded to float32.  Only |X_f| and that increment are stored: the spectra
// never reach memory.  A frame slot behind the job's last frame runs on zeros and stores nothing; no lane leaves before the
// last barrier.  Nothing outside [0, n_in) of the job's span is read.
template <int LOGM>
__global__ __launch_bounds__(WUN_FFT_BLOCK) void voc_analysis_kernel(VocArgs p) {
    using G = FftGeom<LOGM>;
    constexpr int M = G::M, N = G::N, TPF = G::TPF, NB = M / TPF + 1;
    __shared__ float sre[2][G::PLANE];
    __shared__ float sim[2][G::PLANE];
    const long long wg = blockIdx.x;
    int j = 0;
    while (j + 1 < p.J && wg >= p.gp[j + 1]) ++j;
    const wun_stretch_job jb = p.job[j];
    const long long F = p.fp[j + 1] - p.fp[j];
    const long long groups = (F + G::FPW - 1) / G::FPW, local = wg - p.gp[j];
    const long long c = local / groups;                      // < C: the host sized gp
    const int g = threadIdx.x / TPF, tl = threadIdx.x - g * TPF, base = g * M;
    const long long f = (local - c * groups) * G::FPW + g;
    const bool valid = f < F;
    const long long t0 = valid ? (f * p.hop * jb.num) / jb.den - (N - p.hop) : 0;
    const long long o = valid ? (p.C * p.fp[j] + c * F + f) * p.K : 0;
    const float* __restrict__ x = jb.x + c;
    const float* __restrict__ tw = p.table;
    const float* __restrict__ win = p.table + 2 * N;
    const long long T = jb.n_in;
    const int C = p.C;
    float pr[NB], pi[NB];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const long long ts = pass ? t0 : t0 - p.hop;
        fft_run<LOGM>([&](int a, float& re, float& im) {     // (fft_fwd_frames' load at the frame's own start)
            const long long t = ts + 2 * a;
            re = (valid && t >= 0 && t < T) ? x[t * C] * win[2 * a] : 0.f;
            im = (valid && t + 1 >= 0 && t + 1 < T) ? x[(t + 1) * C] * win[2 * a + 1] : 0.f;
        }, sre, sim, base, tl, tw);
        const float* __restrict__ Zr = sre[G::RESULT];
        const float* __restrict__ Zi = sim[G::RESULT];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int k = tl + i * TPF;                      // 0 .. M: the last round is lane 0's k = M
            if (k <= M) {                                    // (fft_fwd_frames' split step)
                const int ka = base + (k & (M - 1)), kb = base + ((M - k) & (M - 1));
                const float ar = Zr[fft_swz(ka)], ai = Zi[fft_swz(ka)], cr = Zr[fft_swz(kb)], ci = Zi[fft_swz(kb)];
                const float er = 0.5f * (ar + cr), ei = 0.5f * (ai - ci), odr = 0.5f * (ai + ci), odi = 0.5f * (cr - ar);
                const float wc = tw[k], ws = tw[N + k];
                const float xr = er + (wc * odr - ws * odi);
                const float xi = (k == 0 || k == M) ? 0.f : ei + (wc * odi + ws * odr);
                if (pass == 0) { pr[i] = xr; pi[i] = xi; }
                else if (valid) {
                    double qr = (double)xr, qi = (double)xi, adv = 0.0;
                    if (f > 0) {
                        const double a = (double)xr, b = (double)xi, u = (double)pr[i], v = (double)pi[i];
                        qr = a * u + b * v;
                        qi = b * u - a * v;
                        adv = (double)((k * p.hop) & (N - 1)) / (double)N;
                    }
                    const double ang = (qr == 0.0 && qi == 0.0) ? 0.0 : atan2(qi, qr) / 6.283185307179586476925286766559;
                    const double d = ang - adv;
                    p.mag[o + k] = sqrtf(fmaf(xr, xr, xi * xi));
                    p.dlt[o + k] = f > 0 ? (float)(d - rint(d)) : (float)ang;
                }
            }
        }
        if (pass == 0) __syncthreads();                      // every lane has read P_f: the next first stage may write that image
    }
}

// one workgroup: chunks of 256 frames through LDS, lane 0 adds slot 0 and lane 64 slot 1 in ascending frame order
__global__ __launch_bounds__(WUN_FFT_BLOCK) void gl_finish_kernel(const double* __restrict__ part, long long n, double* __restrict__ out) {
    __shared__ double buf[2][WUN_FFT_BLOCK];
    const int tid = threadIdx.x;
    if (n < 0) {
        if (tid < 2) out[tid] = __builtin_nan("");
        return;
    }
    const int slot = tid == 64 ? 1 : 0;
    double acc = 0.0;
    for (long long e0 = 0; e0 < n; e0 += WUN_FFT_BLOCK) {
        const long long e = e0 + tid;
        if (e < n) { buf[0][tid] = part[2 * e]; buf[1][tid] = part[2 * e + 1]; }
        __syncthreads();
        if (tid == 0 || tid == 64) {
            const int cnt = n - e0 < WUN_FFT_BLOCK ? (int)(n - e0) : WUN_FFT_BLOCK;
            for (int j = 0; j < cnt; ++j) acc += buf[slot][j];
        }
        __syncthreads();
    }
    if (tid == 0 || tid == 64) out[slot] = acc;
}

// The launch ledger of the test entries wun_fft_launch_counts / wun_fft_launch_counts_reset (include/wun.h): launches per kernel
// body (WUN_FFT_FAMILY_*) and size (log2(n_fft / 2) - 5).  Host code only, written by fft_dispatch and read by nothing else here.
static std::atomic<long long> g_fft_launches[WUN_FFT_FAMILY_COUNT][WUN_FFT_SIZE_COUNT];

// f(std::integral_constant<int, log2(n_fft / 2)>) for an n_fft with a kernel, then one more launch of `family` in the ledger if
// the runtime took it; else WUN_ERR_UNSUPPORTED, nothing launched and nothing counted
template <class F>
static int fft_dispatch(const char* who, int family, int n_fft, F f) {
    int logm = 0;
    switch (n_fft) {
        case 64: f(std::integral_constant<int, 5>()); logm = 5; break;
        case 128: f(std::integral_constant<int, 6>()); logm = 6; break;
        case 256: f(std::integral_constant<int, 7>()); logm = 7; break;
        case 512: f(std::integral_constant<int, 8>()); logm = 8; break;
        case 1024: f(std::integral_constant<int, 9>()); logm = 9; break;
        case 2048: f(std::integral_constant<int, 10>()); logm = 10; break;
        case 4096: f(std::integral_constant<int, 11>()); logm = 11; break;
        case 8192: f(std::integral_constant<int, 12>()); logm = 12; break;
        default: return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": no kernel for this n_fft");
    }
    static_assert(WUN_FFT_SIZE_COUNT == 12 - 5 + 1, "one ledger column per case above");
    if (hipPeekAtLastError() == hipSuccess) g_fft_launches[family][logm - 5].fetch_add(1, std::memory_order_relaxed);
    return WUN_OK;
}

template <int LOGM>
static dim3 fwd_grid(const StftCfwdArgs& a, int signals) {
    const long long M = a.M[0] > a.M[1] || signals < 2 ? a.M[0] : a.M[1];
    return dim3((unsigned)((M + FftGeom<LOGM>::FPW - 1) / FftGeom<LOGM>::FPW), 1u, (unsigned)signals);
}

template <int LOGM>
static dim3 inv_grid(const IstftGemmArgs& g) { return dim3((unsigned)((g.M + FftGeom<LOGM>::FPW - 1) / FftGeom<LOGM>::FPW)); }

int fft_launch_forward(const StftCfwdArgs& a, int signals, hipStream_t s) {
    return fft_dispatch("fft_launch_forward", WUN_FFT_FAMILY_FORWARD, a.n_fft, [&](auto L) {
        constexpr int LM = decltype(L)::value;
        hipLaunchKernelGGL(stft_fft_kernel<LM>, fwd_grid<LM>(a, signals), dim3(WUN_FFT_BLOCK), 0, s, a);
    });
}

int fft_launch_magnitude(const StftMagArgs& a, int signals, hipStream_t s) {
    return fft_dispatch("fft_launch_magnitude", WUN_FFT_FAMILY_MAGNITUDE, a.a.n_fft, [&](auto L) {
        constexpr int LM = decltype(L)::value;
        hipLaunchKernelGGL(stft_fft_mag_kernel<LM>, fwd_grid<LM>(a.a, signals), dim3(WUN_FFT_BLOCK), 0, s, a);
    });
}

int fft_launch_spec_head(const SpecHeadArgs& a, hipStream_t s) {
    return fft_dispatch("fft_launch_spec_head", WUN_FFT_FAMILY_SPEC_HEAD, a.a.n_fft, [&](auto L) {
        constexpr int LM = decltype(L)::value;
        hipLaunchKernelGGL(spec_head_fft_kernel<LM>, fwd_grid<LM>(a.a, 1), dim3(WUN_FFT_BLOCK), 0, s, a);
    });
}

void launch_steady_den(float* D, int n_fft, int hop, hipStream_t s) {
    hipLaunchKernelGGL(steady_den_kernel, dim3((unsigned)((hop + WUN_FFT_BLOCK - 1) / WUN_FFT_BLOCK)), dim3(WUN_FFT_BLOCK), 0, s, D, n_fft, hop);
}

void launch_steady_divide(const float* g, const float* D, float* u, long long N, long long T, int hop, hipStream_t s) {
    long long grid = (N + WUN_FFT_BLOCK - 1) / WUN_FFT_BLOCK;
    if (grid > (1 << 16)) grid = 1 << 16;
    hipLaunchKernelGGL(steady_divide_kernel, dim3((unsigned)(grid < 1 ? 1 : grid)), dim3(WUN_FFT_BLOCK), 0, s, g, D, u, N, T, hop);
}

int fft_launch_inverse(const IstftGemmArgs& g, hipStream_t s) {
    return fft_dispatch("fft_launch_inverse", WUN_FFT_FAMILY_INVERSE, g.n_fft, [&](auto L) {
        constexpr int LM = decltype(L)::value;
        hipLaunchKernelGGL((istft_fft_kernel<LM, false>), inv_grid<LM>(g), dim3(WUN_FFT_BLOCK), 0, s, g);
    });
}

int fft_launch_griffin_lim(const GlArgs& g, bool given, hipStream_t s) {
    return fft_dispatch("fft_launch_griffin_lim", given ? WUN_FFT_FAMILY_GRIFFIN_LIM_GIVEN : WUN_FFT_FAMILY_GRIFFIN_LIM, g.n_fft, [&](auto L) {
        constexpr int LM = decltype(L)::value;
        const dim3 grid((unsigned)((g.M + FftGeom<LM>::FPW - 1) / FftGeom<LM>::FPW));
        if (given) hipLaunchKernelGGL((gl_frame_kernel<LM, true>), grid, dim3(WUN_FFT_BLOCK), 0, s, g);
        else hipLaunchKernelGGL((gl_frame_kernel<LM, false>), grid, dim3(WUN_FFT_BLOCK), 0, s, g);
    });
}

int fft_frames_per_workgroup(int n_fft) {
    int fpw = 0;
    if (n_fft >= 64 && n_fft <= 8192 && !(n_fft & (n_fft - 1))) fpw = n_fft / 8 < WUN_FFT_BLOCK ? WUN_FFT_BLOCK / (n_fft / 8) : 1;
    return fpw;
}

int fft_launch_voc_analysis(const VocArgs& v, hipStream_t s) {
    return fft_dispatch("fft_launch_voc_analysis", WUN_FFT_FAMILY_VOC_ANALYSIS, v.n_fft, [&](auto L) {
        constexpr int LM = decltype(L)::value;
        static_assert(FftGeom<LM>::FPW == (FftGeom<LM>::N / 8 < WUN_FFT_BLOCK ? WUN_FFT_BLOCK / (FftGeom<LM>::N / 8) : 1), "fft_frames_per_workgroup");
        hipLaunchKernelGGL(voc_analysis_kernel<LM>, dim3((unsigned)v.gp[v.J]), dim3(WUN_FFT_BLOCK), 0, s, v);
    });
}

void launch_gl_finish(const double* part, long long n, double* out, hipStream_t s) {
    hipLaunchKernelGGL(gl_finish_kernel, dim3(1), dim3(WUN_FFT_BLOCK), 0, s, part, n, out);
}

int fft_launch_adjoint(const IstftGemmArgs& g, hipStream_t s) {
    return fft_dispatch("fft_launch_adjoint", WUN_FFT_FAMILY_ADJOINT, g.n_fft, [&](auto L) {
        constexpr int LM = decltype(L)::value;
        hipLaunchKernelGGL((istft_fft_kernel<LM, true>), inv_grid<LM>(g), dim3(WUN_FFT_BLOCK), 0, s, g);
    });
}

}  // namespace wun

extern "C" int wun_fft_launch_counts(int64_t* counts, int32_t cap) {
    if (!counts) return fail(WUN_ERR_INVALID, "wun_fft_launch_counts: null counts");
    if (cap < WUN_FFT_FAMILY_COUNT * WUN_FFT_SIZE_COUNT)
        return fail(WUN_ERR_INVALID, "wun_fft_launch_counts: cap below WUN_FFT_FAMILY_COUNT * WUN_FFT_SIZE_COUNT");
    for (int f = 0; f < WUN_FFT_FAMILY_COUNT; ++f)
        for (int j = 0; j < WUN_FFT_SIZE_COUNT; ++j)
            counts[f * WUN_FFT_SIZE_COUNT + j] = (int64_t)g_fft_launches[f][j].load(std::memory_order_relaxed);
    return WUN_OK;
}

extern "C" void wun_fft_launch_counts_reset(void) {
    for (int f = 0; f < WUN_FFT_FAMILY_COUNT; ++f)
        for (int j = 0; j < WUN_FFT_SIZE_COUNT; ++j) g_fft_launches[f][j].store(0, std::memory_order_relaxed);
}

extern "C" int64_t wun_fft_table_floats(int32_t n_fft) {
    if (n_fft < 64 || n_fft > 8192 || (n_fft & (n_fft - 1)))
        return fail(WUN_ERR_UNSUPPORTED, "wun_fft_table_floats: n_fft must be a power of two in 64..8192");
    return 3 * (int64_t)n_fft;
}

extern "C" int wun_fft_design(int32_t n_fft, float* table_host, int64_t cap) {
    const int64_t need = wun_fft_table_floats(n_fft);
    if (need < 0) return (int)need;
    if (!table_host) return fail(WUN_ERR_INVALID, "wun_fft_design: null table");
    if (cap < need) return fail(WUN_ERR_INVALID, "wun_fft_design: cap below wun_fft_table_floats");
    // the angle reduced in integers to [0, pi / 2): t = q n_fft / 4 + i, then the quadrant's rotation, which is exact -- so
    // the entries at the multiples of pi / 2 are exactly 0 and +-1
    const int Q = n_fft / 4;
    const double step = 2.0 * 3.14159265358979323846 / (double)n_fft;
    for (int t = 0; t < n_fft; ++t) {
        const int q = t / Q, i = t - q * Q;
        const double c0 = std::cos(step * i), s0 = i ? std::sin(step * i) : 0.0;
        const double c = q == 0 ? c0 : q == 1 ? -s0 : q == 2 ? -c0 : s0;
        const double sn = q == 0 ? s0 : q == 1 ? c0 : q == 2 ? -s0 : -c0;
        table_host[t] = (float)c;
        table_host[n_fft + t] = (float)(0.0 - sn);
        table_host[2 * n_fft + t] = (float)(0.5 - 0.5 * c);              // periodic Hann
    }
    return WUN_OK;
}
