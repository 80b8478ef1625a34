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
//   terms      wun_spectral_loss_terms puts four terms where the loss pass has one: per bin of resolution j, with
//              E = Re_e + i Im_e and T the STFTs of estimates and targets, Me = |E|, Mt = |T| (the floats of wun_stft_magnitude),
//              d = Me - Mt in fp32, sg = sgn(d), sgn(0) = 0:
//                mag_l1      mean |d|                                            coefficient sg (Re_e, Im_e) / Me
//                log_mag_l1  mean |log(Me + log_eps) - log(Mt + log_eps)|        sg / (Me + log_eps) (Re_e, Im_e) / Me
//                sc          mean over the sources s of sqrt(D_s / (N_s + sc_eps)), D_s = sum d^2, N_s = sum Mt^2 over the
//                            source's B C F K bins, in float64        d / (sqrt(D_s) sqrt(N_s + sc_eps)) / S (Re_e, Im_e) / Me
//                complex_l1  mean |E - T| = sqrt(fmaf(a, a, b b)), a = Re_e - Re_t, b = Im_e - Im_t        (a, b) / |E - T|
//              every coefficient 0 where its denominator is (Me == 0, D_s == 0, |E - T| == 0); signs and zero cases are
//              constants of the gradient.  L_j = sum_t termweight_t term_t(j).  The three means keep the loss pass's partition
//              (1024 consecutive bins per partial); the per-source sums run over 1024-bin blocks of EACH SOURCE's own range
//              first, one block then adds them source by source, and only then the coefficients are formed.
//
//   transforms the two frame transforms of a resolution are GEMMs (the kernels below) or, in the *_fft entries, FFTs (wun_fft.hip,
//              launched through wun_fft.h: the forward body with this loss's magnitude epilogue, the inverse body as the unscaled
//              adjoint).  The host code is ONE body per entry with a transform selector: checks, scratch layout,
//              the point-wise kernels, the float64 partition and the finish kernels do not know who filled the arrays.
//
// ONE forward kernel per transform serves the magnitude entry and the losses: the magnitudes the loss takes its signs from are
// the floats wun_stft_magnitude (wun_stft_magnitude_fft) returns.  Every reduction index runs in ascending order inside one lane's accumulator, whatever the
// tile a frame falls in: the bits of a row do not depend on the batch around it, the grid, the scratch contents or pointer
// alignment.  No atomics.
//
// Built WITHOUT the packed fp32 VALU instructions (csrc/Makefile NO_PK_FP32): the loss runs between the forward
// and the backward pass of either compute mode.  Every argument check runs before any GPU work; nothing allocates or synchronises.
#include "wun_stft.h"

#include <cmath>
#include <vector>

using namespace wun;

// (WUN_STFT_ITEMS, stft_block_sum, parts_of -- 1024 elements per partial, THE summation constant: wun_sum.h)
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

// ---- wun_spectral_loss_terms: the loss pass with four terms (the definitions are in the header comment) ----

struct StftFwdPartsArgs {            // StftFwdArgs with Re and Im of BOTH signals (complex_l1 needs the targets')
    const float* x[2];
    float* mag[2]; float* re[2]; float* im[2];
    const float* table;
    long long T, M;
    int F, C, n_fft, hop, K;
};

// stft_fwd_kernel's grid, tile and epilogue -- the magnitudes are the same floats -- storing Re and Im of either signal
__global__ __launch_bounds__(WUN_STFT_BLOCK) void stft_fwd_parts_kernel(StftFwdPartsArgs p) {
    float* __restrict__ mag = p.mag[blockIdx.z];
    float* __restrict__ pre = p.re[blockIdx.z];
    float* __restrict__ pim = p.im[blockIdx.z];
    stft_fwd_tile<false>(
        p.x[blockIdx.z], p.table, p.M, p.T, p.C, p.n_fft, p.K,
        [&](long long m, long long& base, long long& t0) {
            const long long r = m / p.F, f = m - r * p.F;
            const long long sb = r / p.C, c = r - sb * p.C;
            base = sb * p.T * p.C + c;
            t0 = f * p.hop;
        },
        [&](long long m, int k, float re, float im) {
            mag[m * p.K + k] = sqrtf(fmaf(re, re, im * im));
            pre[m * p.K + k] = re; pim[m * p.K + k] = im;
        });
}

// sc, first pass: block b = (source s = b / ps, 1024-bin block b - s ps of THAT source's Es bins) -> part[2 b] = sum d^2,
// part[2 b + 1] = sum Mt^2, every square formed and added in float64.  No block crosses a source boundary.
__global__ __launch_bounds__(WUN_STFT_BLOCK) void spec_sc_sums_kernel(const float* __restrict__ me, const float* __restrict__ mt,
                                                                      double* __restrict__ part, long long Es, long long ps) {
    __shared__ double red[2][WUN_STFT_BLOCK];
    const int tid = threadIdx.x;
    const long long s = (long long)blockIdx.x / ps, pb = (long long)blockIdx.x - s * ps;
    double D = 0.0, N = 0.0;
#pragma unroll
    for (int it = 0; it < WUN_STFT_ITEMS; ++it) {
        const long long el = (pb * WUN_STFT_ITEMS + it) * WUN_STFT_BLOCK + tid;
        if (el >= Es) continue;
        const float t = mt[s * Es + el];
        const float d = me[s * Es + el] - t;
        D += (double)d * (double)d;
        N += (double)t * (double)t;
    }
    D = stft_block_sum(red[0], D, tid);
    N = stft_block_sum(red[1], N, tid);
    if (tid == 0) { part[2 * (long long)blockIdx.x] = D; part[2 * (long long)blockIdx.x + 1] = N; }
}

// sc, second pass, ONE block: source after source, lane l adds the source's partials l, l + 256, ... in ascending order and one
// tree adds the lanes.  src[3 s] = D_s, [3 s + 1] = N_s, [3 s + 2] = Es / (sqrt(D_s) sqrt(N_s + sc_eps)), 0 where D_s == 0: the
// coefficient's factor, pre-scaled by R F K / S so that spec_grad_kernel's scale of the resolution stays weight / (R F K).
__global__ __launch_bounds__(WUN_STFT_BLOCK) void spec_sc_reduce_kernel(const double* __restrict__ part, double* __restrict__ src,
                                                                        int S, long long ps, double es, float sc_eps) {
    __shared__ double red[2][WUN_STFT_BLOCK];
    const int tid = threadIdx.x;
    for (int s = 0; s < S; ++s) {
        double D = 0.0, N = 0.0;
        for (long long i = tid; i < ps; i += WUN_STFT_BLOCK) { D += part[2 * (s * ps + i)]; N += part[2 * (s * ps + i) + 1]; }
        D = stft_block_sum(red[0], D, tid);
        N = stft_block_sum(red[1], N, tid);
        if (tid == 0) {
            src[3 * s] = D; src[3 * s + 1] = N;
            src[3 * s + 2] = D > 0.0 ? es / (sqrt(D) * sqrt(N + (double)sc_eps)) : 0.0;
        }
        __syncthreads();                                     // red[0] is read by every lane before the next source writes it
    }
}

struct SpecTermsArgs {
    const float* me; const float* mt;        // [M][K]
    float* re; float* im;                    // Re, Im of the estimates; with grad the coefficients replace them in place
    const float* ret; const float* imt;      // Re, Im of the targets (complex_l1 only)
    double* part[3];                         // [ceil(E / 1024)] each: mag_l1, log_mag_l1, complex_l1 (unused without the term)
    const double* src;                       // [S][3] of spec_sc_reduce_kernel (sc only)
    long long E, Es;                         // bins in all, bins per source
    float w_mag, w_log, w_sc, w_cx, log_eps;
    int grad;
};

// ---- mel-scale terms (include/wun.h): the table's five arrays, the adjoint of one bin ----
struct MelTable { const int* b0; const float* w0; const float* w1; const int* lo; const int* hi; };

__host__ __device__ __forceinline__ MelTable mel_table(const float* t, int K) {
    MelTable m;      // (hi = lo + n_mels is set by the projection, the one reader of it: the adjoint needs no n_mels here)
    m.b0 = (const int*)t; m.w0 = t + K; m.w1 = t + 2 * K; m.lo = (const int*)(t + 3 * K); m.hi = m.lo;
    return m;
}

// q[k] = fmaf(w1[k], g[b0[k] + 1], w0[k] * g[b0[k]]) of one frame's g [n_mels]: a band whose weight is 0 or whose index is
// outside 0 .. n_mels - 1 is not read
__device__ __forceinline__ float mel_adjoint(const MelTable& t, const float* __restrict__ g, int k, int n_mels) {
    const int b = t.b0[k];
    const float w0 = t.w0[k], w1 = t.w1[k];
    const float g0 = (w0 != 0.f && b >= 0 && b < n_mels) ? g[b] : 0.f;
    const float g1 = (w1 != 0.f && b + 1 >= 0 && b + 1 < n_mels) ? g[b + 1] : 0.f;
    return fmaf(w1, g1, w0 * g0);
}

struct SpecMelAdjArgs {
    const float* g;                          // [M][n_mels] of mel_terms_kernel
    const float* table;                      // the mel table of this resolution
    float kn;                                // K / n_mels: the mel means' 1 / (R F n_mels) on the resolution's 1 / (R F K)
    int K, n_mels;
};

// spec_l1_kernel with the four terms: 1024 bins per block, the same partition and tree for each of the three means, and the
// coefficient of (Re_e, Im_e) / Me summed over the terms before the one division -- with mag_l1 = 1 alone, spec_l1_kernel's bits.
// MEL: the mel terms' part of that coefficient, (K / n_mels) times the adjoint of g at this bin, added before the division.
template <bool MEL>
__device__ __forceinline__ void spec_terms_body(const SpecTermsArgs& p, const SpecMelAdjArgs& ma) {
    __shared__ double red[3][WUN_STFT_BLOCK];
    const int tid = threadIdx.x;
    const bool mag = p.w_mag > 0.f, lg = p.w_log > 0.f, sc = p.w_sc > 0.f, cx = p.w_cx > 0.f;
    double am = 0.0, al = 0.0, ac = 0.0;
    long long mel_m0 = 0;
    int mel_r0 = 0;
    if (MEL) {
        const long long e0 = (long long)blockIdx.x * WUN_STFT_ITEMS * WUN_STFT_BLOCK;
        mel_m0 = e0 / ma.K;
        mel_r0 = (int)(e0 - mel_m0 * ma.K);
    }
#pragma unroll
    for (int it = 0; it < WUN_STFT_ITEMS; ++it) {
        const long long e = ((long long)blockIdx.x * WUN_STFT_ITEMS + it) * WUN_STFT_BLOCK + tid;
        if (e >= p.E) continue;
        const float a = p.me[e], t = p.mt[e];
        const float d = a - t;
        const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        float q = 0.f;                                       // the coefficient of (Re_e, Im_e) / Me
        if (mag) { am += (double)fabsf(d); q = p.w_mag * sg; }
        if (lg) {
            const float ea = a + p.log_eps, et = t + p.log_eps;
            al += (double)fabsf(logf(ea) - logf(et));
            q += p.w_log * (sg / ea);
        }
        if (sc) q += p.w_sc * (d * (float)p.src[3 * (e / p.Es) + 2]);
        if (MEL) {
            // (frame, bin) of e: the block's first element divided once in 64 bits, its 1024 elements in 32
            const unsigned r = (unsigned)(mel_r0 + it * WUN_STFT_BLOCK + tid), dm = r / (unsigned)ma.K;
            q += ma.kn * mel_adjoint(mel_table(ma.table, ma.K), ma.g + (mel_m0 + dm) * ma.n_mels, (int)(r - dm * (unsigned)ma.K), ma.n_mels);
        }
        float cr = 0.f, ci = 0.f;
        if (p.grad && q != 0.f && a > 0.f) { cr = q * p.re[e] / a; ci = q * p.im[e] / a; }
        if (cx) {
            const float x = p.re[e] - p.ret[e], y = p.im[e] - p.imt[e];
            const float m = sqrtf(fmaf(x, x, y * y));        // (spelled out, as the forward epilogue)
            ac += (double)m;
            if (p.grad && m > 0.f) { cr += p.w_cx * (x / m); ci += p.w_cx * (y / m); }
        }
        if (p.grad) { p.re[e] = cr; p.im[e] = ci; }
    }
    if (mag) { const double s = stft_block_sum(red[0], am, tid); if (tid == 0) p.part[0][blockIdx.x] = s; }
    if (lg) { const double s = stft_block_sum(red[1], al, tid); if (tid == 0) p.part[1][blockIdx.x] = s; }
    if (cx) { const double s = stft_block_sum(red[2], ac, tid); if (tid == 0) p.part[2][blockIdx.x] = s; }
}

__global__ __launch_bounds__(WUN_STFT_BLOCK) void spec_terms_kernel(SpecTermsArgs p) { spec_terms_body<false>(p, SpecMelAdjArgs()); }
__global__ __launch_bounds__(WUN_STFT_BLOCK) void spec_terms_mel_kernel(SpecTermsArgs p, SpecMelAdjArgs ma) {
    spec_terms_body<true>(p, ma);
}

struct SpecTermsFinishArgs {
    const double* part[1 + WUN_SPEC_MAX_RES][3]; // slot 0: MSE (sum 0 only); slot 1 + j: mag_l1, log_mag_l1, complex_l1 of resolution j
    long long nparts[1 + WUN_SPEC_MAX_RES][3];   // 0: the sum is not taken
    double count[1 + WUN_SPEC_MAX_RES];
    float weight[1 + WUN_SPEC_MAX_RES];
    const double* src[WUN_SPEC_MAX_RES];         // [S][3] per resolution (sc only)
    float w[4], sc_eps;                          // term weights in the order of the losses: mag_l1, log_mag_l1, sc, complex_l1
    int S, nres;
    float* losses;                               // [2 + 5 nres]
};

// spec_finish_kernel over the new slots: one wave per slot takes its (up to) three sums one after the other, each as there --
// lane l adds the partials l, l + 64, ... in ascending order, one tree over the 64 lanes -- and thread 0 forms the terms, L_j
// and the total in slot order.
// MEL: two more sums per resolution slot (mel_l1, log_mel_l1), taken the same way behind the three; L_j and the total gain the
// two weighted terms behind the four, and the terms go to the slots behind the 2 + 5 nres.
struct SpecMelFinishArgs {
    const double* part[WUN_SPEC_MAX_RES][2];     // mel_l1, log_mel_l1 of resolution j
    long long nparts[WUN_SPEC_MAX_RES][2];       // 0: the sum is not taken
    double count[WUN_SPEC_MAX_RES];              // R F n_mels
    float w[2];
};

template <bool MEL>
__device__ __forceinline__ void spec_terms_finish_body(const SpecTermsFinishArgs& p, const SpecMelFinishArgs& q) {
    constexpr int NS = MEL ? 5 : 3;
    __shared__ double red[1 + WUN_SPEC_MAX_RES][64];
    __shared__ double sums[1 + WUN_SPEC_MAX_RES][NS];
    const int slot = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int t = 0; t < NS; ++t) {
        double s = 0.0;
        if (MEL && t >= 3) {
            if (slot >= 1 && slot <= p.nres)
                for (long long i = lane; i < q.nparts[slot - 1][t - 3]; i += 64) s += q.part[slot - 1][t - 3][i];
        } else if (slot <= p.nres)
            for (long long i = lane; i < p.nparts[slot][t]; i += 64) s += p.part[slot][t][i];
        red[slot][lane] = s;
        __syncthreads();
        for (int h = 32; h > 0; h >>= 1) {
            if (lane < h) red[slot][lane] += red[slot][lane + h];
            __syncthreads();
        }
        if (lane == 0) sums[slot][t] = red[slot][0];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double mse = sums[0][0] / p.count[0];
        p.losses[1] = (float)mse;
        double total = (double)p.weight[0] * mse;
        for (int j = 0; j < p.nres; ++j) {
            double term[4] = {0.0, 0.0, 0.0, 0.0};
            if (p.w[0] > 0.f) term[0] = sums[1 + j][0] / p.count[1 + j];
            if (p.w[1] > 0.f) term[1] = sums[1 + j][1] / p.count[1 + j];
            if (p.w[2] > 0.f) {
                double a = 0.0;
                for (int s = 0; s < p.S; ++s) a += sqrt(p.src[j][3 * s] / (p.src[j][3 * s + 1] + (double)p.sc_eps));
                term[2] = a / (double)p.S;
            }
            if (p.w[3] > 0.f) term[3] = sums[1 + j][2] / p.count[1 + j];
            double L = 0.0;
            for (int t = 0; t < 4; ++t) {
                p.losses[2 + p.nres + 4 * j + t] = (float)term[t];
                if (p.w[t] > 0.f) L += (double)p.w[t] * term[t];
            }
            if (MEL)
                for (int t = 0; t < 2; ++t) {
                    const double mt = q.w[t] > 0.f ? sums[1 + j][3 + t] / q.count[j] : 0.0;
                    p.losses[2 + 5 * p.nres + 2 * j + t] = (float)mt;
                    if (q.w[t] > 0.f) L += (double)q.w[t] * mt;
                }
            p.losses[2 + j] = (float)L;
            total += (double)p.weight[1 + j] * L;
        }
        p.losses[0] = (float)total;
    }
}

__global__ __launch_bounds__(64 * (1 + WUN_SPEC_MAX_RES)) void spec_terms_finish_kernel(SpecTermsFinishArgs p) {
    spec_terms_finish_body<false>(p, SpecMelFinishArgs());
}
__global__ __launch_bounds__(64 * (1 + WUN_SPEC_MAX_RES)) void spec_mel_finish_kernel(SpecTermsFinishArgs p, SpecMelFinishArgs q) {
    spec_terms_finish_body<true>(p, q);
}

// ---- the mel projection and its terms (include/wun.h: the definitions) ----
#define WUN_MEL_MAX 512              // bands
#define WUN_MEL_TILE_FLOATS 2048     // magnitudes a workgroup stages: frames per workgroup = clamp(2048 / K, 1, 16)
#define WUN_MEL_UNROLL 8             // bins whose loads are in flight together in the projection's chain

struct MelProjArgs {
    const float* mag[2];             // [M][K]; blockIdx.y picks one (estimates, targets)
    float* out[2];                   // [M][n_mels]
    const float* table;
    long long M;
    int K, n_mels, FR;               // FR frames per workgroup: FR * K floats of LDS
};

// grid: x = tile of FR frames, y = signal.  The tile's magnitudes are contiguous: they go to LDS with coalesced 4-byte loads;
// then one lane per (frame, band) walks the band's bins lo .. hi - 1 in ONE accumulator, one fmaf per bin, ascending.  The
// weight of bin k in band b is w0[k] where b0[k] == b, else w1[k] (then b0[k] + 1 == b: the table's two-bands property).
__global__ __launch_bounds__(WUN_STFT_BLOCK) void mel_project_kernel(MelProjArgs p) {
    extern __shared__ float mel_rows[];
    const int tid = threadIdx.x;
    const long long m0 = (long long)blockIdx.x * p.FR;
    const int nfr = p.M - m0 < p.FR ? (int)(p.M - m0) : p.FR;
    const float* __restrict__ src = p.mag[blockIdx.y] + m0 * p.K;
    for (int i = tid; i < nfr * p.K; i += WUN_STFT_BLOCK) mel_rows[i] = src[i];
    __syncthreads();
    MelTable t = mel_table(p.table, p.K);
    t.hi = t.lo + p.n_mels;
    float* __restrict__ out = p.out[blockIdx.y] + m0 * p.n_mels;
    for (int o = tid; o < nfr * p.n_mels; o += WUN_STFT_BLOCK) {
        const int fr = o / p.n_mels, b = o - fr * p.n_mels;
        int lo = t.lo[b], hi = t.hi[b];
        if (lo < 0) lo = 0;
        if (hi > p.K) hi = p.K;                              // (a table of another K must not reach outside the tile)
        const float* row = mel_rows + fr * p.K;
        float acc = 0.f;
        // eight bins at a time: their table words and magnitudes are loaded together (independent loads: one memory latency per
        // eight bins, not two per bin), then the fmafs run in ascending k.  Behind the band's end the loads repeat bin hi - 1 and
        // the fmaf is skipped: no bin outside [lo, hi) is read for this band.
        for (int k = lo; k < hi; k += WUN_MEL_UNROLL) {
            int bb[WUN_MEL_UNROLL];
            float wa[WUN_MEL_UNROLL], wb[WUN_MEL_UNROLL], mv[WUN_MEL_UNROLL];
#pragma unroll
            for (int u = 0; u < WUN_MEL_UNROLL; ++u) {
                const int kk = k + u < hi ? k + u : hi - 1;
                bb[u] = t.b0[kk]; wa[u] = t.w0[kk]; wb[u] = t.w1[kk]; mv[u] = row[kk];
            }
#pragma unroll
            for (int u = 0; u < WUN_MEL_UNROLL; ++u)
                if (k + u < hi) acc = fmaf(bb[u] == b ? wa[u] : wb[u], mv[u], acc);
        }
        out[o] = acc;
    }
}

struct MelTermsArgs {
    float* pe; const float* pt;      // [M][n_mels]; with grad g replaces Pe in place
    double* part[2];                 // mel_l1, log_mel_l1 (unused without the term)
    long long E;                     // M n_mels
    float w_mel, w_log, log_eps;
    int grad;
};

// the loss pass's partition on the mel values: 1024 per block, the same tree for either mean; g = w_mel sg + w_log sg / (Pe + eps)
__global__ __launch_bounds__(WUN_STFT_BLOCK) void mel_terms_kernel(MelTermsArgs p) {
    __shared__ double red[2][WUN_STFT_BLOCK];
    const int tid = threadIdx.x;
    const bool ml = p.w_mel > 0.f, lg = p.w_log > 0.f;
    double am = 0.0, al = 0.0;
#pragma unroll
    for (int it = 0; it < WUN_STFT_ITEMS; ++it) {
        const long long e = ((long long)blockIdx.x * WUN_STFT_ITEMS + it) * WUN_STFT_BLOCK + tid;
        if (e >= p.E) continue;
        const float a = p.pe[e], t = p.pt[e];
        const float d = a - t;
        const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        float q = 0.f;
        if (ml) { am += (double)fabsf(d); q = p.w_mel * sg; }
        if (lg) {
            const float ea = a + p.log_eps, et = t + p.log_eps;
            al += (double)fabsf(logf(ea) - logf(et));
            q = fmaf(p.w_log, sg / ea, q);
        }
        if (p.grad) p.pe[e] = q;
    }
    if (ml) { const double s = stft_block_sum(red[0], am, tid); if (tid == 0) p.part[0][blockIdx.x] = s; }
    if (lg) { const double s = stft_block_sum(red[1], al, tid); if (tid == 0) p.part[1][blockIdx.x] = s; }
}

// the single operator: one lane per bin of q [M][K]
__global__ __launch_bounds__(WUN_STFT_BLOCK) void mel_transpose_kernel(const float* __restrict__ g, const float* table,
                                                                       float* __restrict__ q, long long E, int K, int n_mels) {
    const long long e = (long long)blockIdx.x * WUN_STFT_BLOCK + threadIdx.x;
    if (e >= E) return;
    const long long m = e / K;
    q[e] = mel_adjoint(mel_table(table, K), g + m * n_mels, (int)(e - m * K), n_mels);
}

}  // namespace wun

namespace {

struct Res { int n_fft, hop, K; long long F, M; };

int make_res(const char* who, int tr, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop, Res* r) {
    int rc;
    if ((rc = check_res(who, tr, n_fft, hop, T))) return rc;
    r->n_fft = n_fft; r->hop = hop; r->K = n_fft / 2 + 1;
    r->F = 1 + (T - n_fft) / hop;
    r->M = (long long)S * B * C * r->F;
    if (r->M > ((long long)1 << 30)) return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 2^30 frames in all");
    return WUN_OK;
}

// floats of one resolution's slice of the scratch: magnitudes of both signals, Re and Im of the estimates, the frame gradients
long long res_floats(const Res& r) { return 4 * r.M * r.K + r.M * r.n_fft; }

// the argument checks of the two loss entries, in one order; fills res[0 .. nres)
int check_loss(const char* who, int tr, const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
               float mse_weight, int32_t nres, const int32_t* n_fft, const int32_t* hop, const float* weights,
               const float* const* tables_dev, const float* losses, const float* scratch, Res* res) {
    const std::string w(who);
    if (!outputs || !targets || !losses || !scratch) return fail(WUN_ERR_INVALID, w + ": null argument");
    int rc;
    if ((rc = check_audio(who, S, B, Tout, C))) return rc;
    if (nres < 0 || nres > WUN_SPEC_MAX_RES) return fail(WUN_ERR_INVALID, w + ": nres outside 0..8");
    if (nres > 0 && (!n_fft || !hop || !weights || !tables_dev)) return fail(WUN_ERR_INVALID, w + ": null resolution table");
    if (!(mse_weight >= 0.f) || !std::isfinite(mse_weight)) return fail(WUN_ERR_INVALID, w + ": mse_weight negative or not finite");
    for (int j = 0; j < nres; ++j) {
        if ((rc = make_res(who, tr, S, B, Tout, C, n_fft[j], hop[j], &res[j]))) return rc;
        if (!(weights[j] >= 0.f) || !std::isfinite(weights[j])) return fail(WUN_ERR_INVALID, w + ": a weight negative or not finite");
        if (!tables_dev[j]) return fail(WUN_ERR_INVALID, w + ": null table");
    }
    return WUN_OK;
}

int check_terms(const char* who, const wun_spectral_terms* t) {
    const std::string w(who);
    if (!t) return fail(WUN_ERR_INVALID, w + ": null terms");
    for (float x : {t->mag_l1, t->log_mag_l1, t->sc, t->complex_l1})
        if (!(x >= 0.f) || !std::isfinite(x)) return fail(WUN_ERR_INVALID, w + ": a term weight negative or not finite");
    if (!(t->log_eps > 0.f) || !std::isfinite(t->log_eps)) return fail(WUN_ERR_INVALID, w + ": log_eps must be finite and > 0");
    if (!(t->sc_eps > 0.f) || !std::isfinite(t->sc_eps)) return fail(WUN_ERR_INVALID, w + ": sc_eps must be finite and > 0");
    return WUN_OK;
}

// what wun_spectral_loss_terms adds to a resolution: floats behind its slice (Re and Im of the targets), and float64s behind the
// partials of the MSE -- one run of partials per mean term in use, then for sc [S][ps][2] partials and [S][3] scalars
long long terms_floats(const Res& r, const wun_spectral_terms& t) { return t.complex_l1 > 0.f ? 2 * r.M * r.K : 0; }
long long terms_doubles(const Res& r, int32_t S, const wun_spectral_terms& t) {
    const long long E = r.M * r.K;
    const int means = (t.mag_l1 > 0.f) + (t.log_mag_l1 > 0.f) + (t.complex_l1 > 0.f);
    return means * parts_of(E) + (t.sc > 0.f ? 2 * S * parts_of(E / S) + 3 * (long long)S : 0);
}

// ---- the mel terms' arguments of the *_mel entries (null: the entries without them) ----
struct MelCall { const wun_mel_terms* mel; const int32_t* n_mels; const float* const* tables; };

int check_mel(const char* who, const MelCall& mc, int32_t nres, bool tables) {
    const std::string w(who);
    if (!mc.mel) return fail(WUN_ERR_INVALID, w + ": null mel terms");
    for (float x : {mc.mel->mel_l1, mc.mel->log_mel_l1})
        if (!(x >= 0.f) || !std::isfinite(x)) return fail(WUN_ERR_INVALID, w + ": a mel weight negative or not finite");
    if (!(mc.mel->log_eps > 0.f) || !std::isfinite(mc.mel->log_eps)) return fail(WUN_ERR_INVALID, w + ": mel log_eps must be finite and > 0");
    if (nres > 0 && (!mc.n_mels || (tables && !mc.tables))) return fail(WUN_ERR_INVALID, w + ": null n_mels or mel table list");
    for (int j = 0; j < nres; ++j) {
        if (mc.n_mels[j] < 1 || mc.n_mels[j] > WUN_MEL_MAX) return fail(WUN_ERR_INVALID, w + ": n_mels outside 1..512");
        if (tables && !mc.tables[j]) return fail(WUN_ERR_INVALID, w + ": null mel table");
    }
    return WUN_OK;
}

bool mel_on(const wun_mel_terms& m) { return m.mel_l1 > 0.f || m.log_mel_l1 > 0.f; }
// what the mel terms add to a resolution: Pe (g in place) and Pt behind its floats, one run of partials per mel term in use
long long mel_floats(const Res& r, int n_mels, const wun_mel_terms& m) { return mel_on(m) ? 2 * r.M * n_mels : 0; }
long long mel_doubles(const Res& r, int n_mels, const wun_mel_terms& m) {
    return ((m.mel_l1 > 0.f) + (m.log_mel_l1 > 0.f)) * parts_of(r.M * n_mels);
}

int mel_frames_per_block(int K) {
    const int fr = WUN_MEL_TILE_FLOATS / K;
    return fr < 1 ? 1 : (fr > 16 ? 16 : fr);
}

// P of one or two [M][K] arrays in one launch
void launch_mel_project(const float* mag0, const float* mag1, float* out0, float* out1, const float* table, long long M, int K,
                        int n_mels, hipStream_t s) {
    MelProjArgs a;
    a.mag[0] = mag0; a.mag[1] = mag1; a.out[0] = out0; a.out[1] = out1; a.table = table; a.M = M; a.K = K; a.n_mels = n_mels;
    a.FR = mel_frames_per_block(K);
    hipLaunchKernelGGL(mel_project_kernel, dim3((unsigned)((M + a.FR - 1) / a.FR), mag1 ? 2u : 1u), dim3(WUN_STFT_BLOCK),
                       (size_t)a.FR * K * sizeof(float), s, a);
}

// The forward transform of one resolution on transform tr (the GEMM tile or the FFT body, one epilogue): the magnitudes of x0
// (and of x1 unless null), Re / Im of x0 into re0 / im0 and of x1 into re1 / im1 where those are not null.  The GEMM has two
// kernels: stft_fwd_parts_kernel where the targets' Re / Im are wanted, stft_fwd_kernel otherwise.
int launch_fwd(int tr, const float* x0, const float* x1, float* mag0, float* mag1, float* re0, float* im0, float* re1, float* im1,
               const float* table, int64_t T, int32_t C, const Res& r, hipStream_t s) {
    if (tr == WUN_TR_FFT) {
        StftMagArgs a;
        a.a.x[0] = x0; a.a.x[1] = x1; a.a.re[0] = re0; a.a.re[1] = re1; a.a.im[0] = im0; a.a.im[1] = im1;
        a.a.M[0] = r.M; a.a.M[1] = x1 ? r.M : 0; a.a.table = table;
        a.a.T = T; a.a.nb = r.F; a.a.f0 = 0; a.a.fstride = r.F; a.a.foff = 0;      // the loss's framing: lead 0, whole frames
        a.a.C = C; a.a.n_fft = r.n_fft; a.a.hop = r.hop; a.a.lead = 0; a.a.K = r.K;
        a.mag[0] = mag0; a.mag[1] = mag1;
        return fft_launch_magnitude(a, x1 ? 2 : 1, s);
    }
    const dim3 grid((unsigned)((r.M + WUN_STFT_BM - 1) / WUN_STFT_BM), (unsigned)((r.K + WUN_STFT_BN - 1) / WUN_STFT_BN), x1 ? 2u : 1u);
    if (re1) {
        StftFwdPartsArgs a;
        a.x[0] = x0; a.x[1] = x1; a.mag[0] = mag0; a.mag[1] = mag1; a.re[0] = re0; a.re[1] = re1; a.im[0] = im0; a.im[1] = im1;
        a.table = table; a.T = T; a.M = r.M; a.F = (int)r.F; a.C = C; a.n_fft = r.n_fft; a.hop = r.hop; a.K = r.K;
        hipLaunchKernelGGL(stft_fwd_parts_kernel, grid, dim3(WUN_STFT_BLOCK), 0, s, a);
        return WUN_OK;
    }
    StftFwdArgs a;
    a.x[0] = x0; a.x[1] = x1; a.mag[0] = mag0; a.mag[1] = mag1; a.re = re0; a.im = im0; a.table = table;
    a.T = T; a.M = r.M; a.F = (int)r.F; a.C = C; a.n_fft = r.n_fft; a.hop = r.hop; a.K = r.K;
    hipLaunchKernelGGL(stft_fwd_kernel, grid, dim3(WUN_STFT_BLOCK), 0, s, a);
    return WUN_OK;
}

// dframe[m][n] = sum_k cre[m][k] Cb[n][k] + cim[m][k] Sb[n][k] on transform tr: the transposed GEMM, or the FFT's inverse body
// as the unscaled adjoint (every bin once, final scale 1 / 2)
int launch_bwd(int tr, const float* cre, const float* cim, const float* table, float* dframe, const Res& r, hipStream_t s) {
    if (tr == WUN_TR_FFT) {
        IstftGemmArgs g;
        g.re = cre; g.im = cim; g.table = table; g.frames = dframe;
        g.M = r.M; g.nb = r.M; g.fstride = 0; g.foff = 0;                          // dense rows: the spectrum of row m at m K
        g.n_fft = r.n_fft; g.K = r.K; g.c_edge = 0.5f; g.c_mid = 0.5f;
        return fft_launch_adjoint(g, s);
    }
    StftBwdArgs b;
    b.cre = cre; b.cim = cim; b.table = table; b.dframe = dframe; b.M = r.M; b.n_fft = r.n_fft; b.K = r.K;
    hipLaunchKernelGGL(stft_bwd_kernel, dim3((unsigned)((r.M + WUN_STFT_BM - 1) / WUN_STFT_BM), (unsigned)(r.n_fft / WUN_STFT_BN)),
                       dim3(WUN_STFT_BLOCK), 0, s, b);
    return WUN_OK;
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

// ---- the entries: one body each, `who` and the transform tr (WUN_TR_GEMM / WUN_TR_FFT: the n_fft list, the table and the two
// frame transforms; every check, the scratch layout, the point-wise kernels and the summation order are shared) ----
namespace {

int magnitude_entry(const char* who, int tr, const float* x, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                    const float* table_dev, float* mags, void* stream) {
    if (!x || !table_dev || !mags) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    int rc;
    Res r;
    if ((rc = check_audio(who, S, B, T, C))) return rc;
    if ((rc = make_res(who, tr, S, B, T, C, n_fft, hop, &r))) return rc;
    if ((rc = launch_fwd(tr, x, nullptr, mags, nullptr, nullptr, nullptr, nullptr, nullptr, table_dev, T, C, r, (hipStream_t)stream)))
        return rc;
    return launch_status(who);
}

int64_t scratch_entry(const char* who, int tr, int32_t S, int32_t B, int64_t Tout, int32_t C, int32_t nres, const int32_t* n_fft,
                      const int32_t* hop) {
    int rc;
    if ((rc = check_audio(who, S, B, Tout, C))) return rc;
    if (nres < 0 || nres > WUN_SPEC_MAX_RES) return fail(WUN_ERR_INVALID, std::string(who) + ": nres outside 0..8");
    if (nres > 0 && (!n_fft || !hop)) return fail(WUN_ERR_INVALID, std::string(who) + ": null resolution table");
    long long floats = 0, parts = parts_of((long long)S * B * Tout * C);
    for (int j = 0; j < nres; ++j) {
        Res r;
        if ((rc = make_res(who, tr, S, B, Tout, C, n_fft[j], hop[j], &r))) return rc;
        floats += res_floats(r);
        parts += parts_of(r.M * r.K);
    }
    return floats + 2 * parts + 2;                           // float64 partials, and room to align them to 8 bytes
}

int loss_entry(const char* who, int tr, const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
               float mse_weight, int32_t nres, const int32_t* n_fft, const int32_t* hop, const float* weights,
               const float* const* tables_dev, float* d_outputs, float* losses, float* scratch, void* stream) {
    int rc;
    Res res[WUN_SPEC_MAX_RES];
    if ((rc = check_loss(who, tr, outputs, targets, S, B, Tout, C, mse_weight, nres, n_fft, hop, weights, tables_dev, losses, scratch,
                         res)))
        return rc;

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
        if ((rc = launch_fwd(tr, outputs, targets, me, mt, grad ? re : nullptr, grad ? im : nullptr, nullptr, nullptr, tables_dev[j],
                             Tout, C, r, s)))
            return rc;
        hipLaunchKernelGGL(spec_l1_kernel, dim3((unsigned)parts_of(E)), blk, 0, s, me, mt, grad ? re : nullptr, grad ? im : nullptr,
                           pnext, E);
        if (grad && (rc = launch_bwd(tr, re, im, tables_dev[j], df, r, s))) return rc;
        g.n_fft[j] = r.n_fft; g.hop[j] = r.hop; g.F[j] = (int)r.F; g.dframe[j] = df;
        g.scale[j] = (float)((double)weights[j] / ((double)r.M * (double)r.K));
        fin.part[1 + j] = pnext; fin.nparts[1 + j] = parts_of(E); fin.count[1 + j] = (double)E; fin.weight[1 + j] = weights[j];
        pnext += parts_of(E);
    }
    const dim3 ggrid((unsigned)parts_of(N));
    if (grad) hipLaunchKernelGGL(spec_grad_kernel<true>, ggrid, blk, 0, s, g);
    else hipLaunchKernelGGL(spec_grad_kernel<false>, ggrid, blk, 0, s, g);
    hipLaunchKernelGGL(spec_finish_kernel, dim3(1), dim3(64 * (1 + WUN_SPEC_MAX_RES)), 0, s, fin);
    return launch_status(who);
}

int64_t terms_scratch_entry(const char* who, int tr, int32_t S, int32_t B, int64_t Tout, int32_t C, int32_t nres, const int32_t* n_fft,
                            const int32_t* hop, const wun_spectral_terms* terms, const MelCall* mc = nullptr) {
    int rc;
    if ((rc = check_audio(who, S, B, Tout, C))) return rc;
    if (nres < 0 || nres > WUN_SPEC_MAX_RES) return fail(WUN_ERR_INVALID, std::string(who) + ": nres outside 0..8");
    if (nres > 0 && (!n_fft || !hop)) return fail(WUN_ERR_INVALID, std::string(who) + ": null resolution table");
    Res res[WUN_SPEC_MAX_RES];
    for (int j = 0; j < nres; ++j)
        if ((rc = make_res(who, tr, S, B, Tout, C, n_fft[j], hop[j], &res[j]))) return rc;
    if ((rc = check_terms(who, terms))) return rc;
    if (mc && (rc = check_mel(who, *mc, nres, false))) return rc;
    long long floats = 0, doubles = parts_of((long long)S * B * Tout * C);
    for (int j = 0; j < nres; ++j) {
        floats += res_floats(res[j]) + terms_floats(res[j], *terms);
        doubles += terms_doubles(res[j], S, *terms);
        if (mc) { floats += mel_floats(res[j], mc->n_mels[j], *mc->mel); doubles += mel_doubles(res[j], mc->n_mels[j], *mc->mel); }
    }
    return floats + 2 * doubles + 2;
}

int terms_entry(const char* who, int tr, const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
                float mse_weight, int32_t nres, const int32_t* n_fft, const int32_t* hop, const float* weights,
                const wun_spectral_terms* terms, const float* const* tables_dev, float* d_outputs, float* losses, float* scratch,
                void* stream, const MelCall* mc = nullptr) {
    int rc;
    Res res[WUN_SPEC_MAX_RES];
    if ((rc = check_loss(who, tr, outputs, targets, S, B, Tout, C, mse_weight, nres, n_fft, hop, weights, tables_dev, losses, scratch, res)))
        return rc;
    if ((rc = check_terms(who, terms))) return rc;
    if (mc && (rc = check_mel(who, *mc, nres, true))) return rc;
    const wun_spectral_terms tw = *terms;
    // mel: the *_mel entries with a mel weight > 0 -- otherwise every launch below but the finish kernel is the old entry's
    wun_mel_terms mw = {0.f, 0.f, 1.f};
    if (mc) mw = *mc->mel;
    const bool mel = mel_on(mw);

    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(WUN_STFT_BLOCK);
    const long long R = (long long)S * B * C, N = R * Tout;
    const bool grad = d_outputs != nullptr, cx = tw.complex_l1 > 0.f, sc = tw.sc > 0.f;
    // scratch: per resolution [M_est | M_tgt | Re -> cre | Im -> cim | dframe | Re_tgt | Im_tgt (complex_l1 only)], then on an
    // 8-byte boundary the float64s: the MSE's partials, then per resolution those of terms_doubles
    long long floats = 0;
    for (int j = 0; j < nres; ++j)
        floats += res_floats(res[j]) + terms_floats(res[j], tw) + (mel ? mel_floats(res[j], mc->n_mels[j], mw) : 0);
    double* part = f64_tail(scratch, floats);

    SpecGradArgs g;
    SpecTermsFinishArgs fin;
    SpecMelFinishArgs mfin;
    mfin.w[0] = mw.mel_l1; mfin.w[1] = mw.log_mel_l1;
    for (int j = 0; j < WUN_SPEC_MAX_RES; ++j) {
        mfin.count[j] = 1.0;
        for (int t = 0; t < 2; ++t) { mfin.part[j][t] = part; mfin.nparts[j][t] = 0; }
    }
    g.out = outputs; g.tgt = targets; g.dout = d_outputs; g.T = Tout; g.N = N; g.C = C; g.nres = nres;
    g.cm = (float)((double)mse_weight * 2.0 / (double)N);
    fin.nres = nres; fin.losses = losses; fin.S = S; fin.sc_eps = tw.sc_eps;
    fin.w[0] = tw.mag_l1; fin.w[1] = tw.log_mag_l1; fin.w[2] = tw.sc; fin.w[3] = tw.complex_l1;
    for (int k = 0; k <= WUN_SPEC_MAX_RES; ++k) {
        for (int t = 0; t < 3; ++t) { fin.part[k][t] = part; fin.nparts[k][t] = 0; }
        fin.count[k] = 1.0; fin.weight[k] = 0.f;
    }
    for (int j = 0; j < WUN_SPEC_MAX_RES; ++j) {
        g.n_fft[j] = 64; g.hop[j] = 64; g.F[j] = 0; g.scale[j] = 0.f; g.dframe[j] = nullptr; fin.src[j] = part;
    }
    g.part = part;
    fin.nparts[0][0] = parts_of(N); fin.count[0] = (double)N; fin.weight[0] = mse_weight;
    double* pnext = part + parts_of(N);

    float* base = scratch;
    for (int j = 0; j < nres; ++j) {
        const Res& r = res[j];
        const long long E = r.M * r.K, Es = E / S, np = parts_of(E);
        float* me = base; float* mt = base + E; float* re = base + 2 * E; float* im = base + 3 * E; float* df = base + 4 * E;
        float* ret = base + res_floats(r); float* imt = ret + E;
        float* pe = ret + terms_floats(r, tw);                // mel: Pe (then g) and Pt [M][n_mels]
        base += res_floats(r) + terms_floats(r, tw) + (mel ? mel_floats(r, mc->n_mels[j], mw) : 0);
        // complex_l1 reads Re / Im of both signals, with or without a gradient; the other terms those of the estimates for the gradient
        const bool parts = cx || grad;
        if ((rc = launch_fwd(tr, outputs, targets, me, mt, parts ? re : nullptr, parts ? im : nullptr, cx ? ret : nullptr,
                             cx ? imt : nullptr, tables_dev[j], Tout, C, r, s)))
            return rc;
        SpecTermsArgs t;
        t.me = me; t.mt = mt; t.re = re; t.im = im; t.ret = ret; t.imt = imt; t.src = part; t.E = E; t.Es = Es;
        t.w_mag = tw.mag_l1; t.w_log = tw.log_mag_l1; t.w_sc = tw.sc; t.w_cx = tw.complex_l1; t.log_eps = tw.log_eps;
        t.grad = grad ? 1 : 0;
        const bool on[3] = {tw.mag_l1 > 0.f, tw.log_mag_l1 > 0.f, cx};
        for (int k = 0; k < 3; ++k) {
            t.part[k] = pnext;
            if (!on[k]) continue;
            fin.part[1 + j][k] = pnext; fin.nparts[1 + j][k] = np;
            pnext += np;
        }
        if (sc) {
            const long long ps = parts_of(Es);
            double* scpart = pnext; double* src = pnext + 2 * S * ps;
            pnext = src + 3 * (long long)S;
            hipLaunchKernelGGL(spec_sc_sums_kernel, dim3((unsigned)(S * ps)), blk, 0, s, me, mt, scpart, Es, ps);
            hipLaunchKernelGGL(spec_sc_reduce_kernel, dim3(1), blk, 0, s, scpart, src, S, ps, (double)Es, tw.sc_eps);
            t.src = src; fin.src[j] = src;
        }
        if (mel) {
            // the projection of both magnitudes, the two mel means and g; with a gradient the coefficient pass takes g's adjoint
            const int nm = mc->n_mels[j];
            const long long Em = r.M * nm, npm = parts_of(Em);
            launch_mel_project(me, mt, pe, pe + Em, mc->tables[j], r.M, r.K, nm, s);
            MelTermsArgs m;
            m.pe = pe; m.pt = pe + Em; m.E = Em; m.w_mel = mw.mel_l1; m.w_log = mw.log_mel_l1; m.log_eps = mw.log_eps;
            m.grad = grad ? 1 : 0;
            const bool mon[2] = {mw.mel_l1 > 0.f, mw.log_mel_l1 > 0.f};
            for (int k = 0; k < 2; ++k) {
                m.part[k] = pnext;
                if (!mon[k]) continue;
                mfin.part[j][k] = pnext; mfin.nparts[j][k] = npm;
                pnext += npm;
            }
            mfin.count[j] = (double)Em;
            hipLaunchKernelGGL(mel_terms_kernel, dim3((unsigned)npm), blk, 0, s, m);
            if (grad) {
                SpecMelAdjArgs ma;
                ma.g = pe; ma.table = mc->tables[j]; ma.kn = (float)((double)r.K / (double)nm); ma.K = r.K; ma.n_mels = nm;
                hipLaunchKernelGGL(spec_terms_mel_kernel, dim3((unsigned)np), blk, 0, s, t, ma);
            }
        }
        if (!mel || !grad) hipLaunchKernelGGL(spec_terms_kernel, dim3((unsigned)np), blk, 0, s, t);
        if (grad && (rc = launch_bwd(tr, re, im, tables_dev[j], df, r, s))) return rc;
        g.n_fft[j] = r.n_fft; g.hop[j] = r.hop; g.F[j] = (int)r.F; g.dframe[j] = df;
        g.scale[j] = (float)((double)weights[j] / ((double)r.M * (double)r.K));
        fin.count[1 + j] = (double)E; fin.weight[1 + j] = weights[j];
    }
    const dim3 ggrid((unsigned)parts_of(N));
    if (grad) hipLaunchKernelGGL(spec_grad_kernel<true>, ggrid, blk, 0, s, g);
    else hipLaunchKernelGGL(spec_grad_kernel<false>, ggrid, blk, 0, s, g);
    if (mc) hipLaunchKernelGGL(spec_mel_finish_kernel, dim3(1), dim3(64 * (1 + WUN_SPEC_MAX_RES)), 0, s, fin, mfin);
    else hipLaunchKernelGGL(spec_terms_finish_kernel, dim3(1), dim3(64 * (1 + WUN_SPEC_MAX_RES)), 0, s, fin);
    return launch_status(who);
}

}  // namespace

extern "C" int wun_stft_magnitude(const float* x, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                                  const float* table_dev, float* mags, void* stream) {
    return magnitude_entry("wun_stft_magnitude", WUN_TR_GEMM, x, S, B, T, C, n_fft, hop, table_dev, mags, stream);
}
extern "C" int wun_stft_magnitude_fft(const float* x, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                                      const float* table_dev, float* mags, void* stream) {
    return magnitude_entry("wun_stft_magnitude_fft", WUN_TR_FFT, x, S, B, T, C, n_fft, hop, table_dev, mags, stream);
}

extern "C" int64_t wun_spectral_scratch_floats(int32_t S, int32_t B, int64_t Tout, int32_t C, int32_t nres, const int32_t* n_fft,
                                               const int32_t* hop) {
    return scratch_entry("wun_spectral_scratch_floats", WUN_TR_GEMM, S, B, Tout, C, nres, n_fft, hop);
}
extern "C" int64_t wun_spectral_fft_scratch_floats(int32_t S, int32_t B, int64_t Tout, int32_t C, int32_t nres, const int32_t* n_fft,
                                                   const int32_t* hop) {
    return scratch_entry("wun_spectral_fft_scratch_floats", WUN_TR_FFT, S, B, Tout, C, nres, n_fft, hop);
}

extern "C" int wun_spectral_loss(const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
                                 float mse_weight, int32_t nres, const int32_t* n_fft, const int32_t* hop, const float* weights,
                                 const float* const* tables_dev, float* d_outputs, float* losses, float* scratch, void* stream) {
    return loss_entry("wun_spectral_loss", WUN_TR_GEMM, outputs, targets, S, B, Tout, C, mse_weight, nres, n_fft, hop, weights,
                      tables_dev, d_outputs, losses, scratch, stream);
}
extern "C" int wun_spectral_loss_fft(const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
                                     float mse_weight, int32_t nres, const int32_t* n_fft, const int32_t* hop, const float* weights,
                                     const float* const* tables_dev, float* d_outputs, float* losses, float* scratch, void* stream) {
    return loss_entry("wun_spectral_loss_fft", WUN_TR_FFT, outputs, targets, S, B, Tout, C, mse_weight, nres, n_fft, hop, weights,
                      tables_dev, d_outputs, losses, scratch, stream);
}

extern "C" int64_t wun_spectral_terms_scratch_floats(int32_t S, int32_t B, int64_t Tout, int32_t C, int32_t nres, const int32_t* n_fft,
                                                     const int32_t* hop, const wun_spectral_terms* terms) {
    return terms_scratch_entry("wun_spectral_terms_scratch_floats", WUN_TR_GEMM, S, B, Tout, C, nres, n_fft, hop, terms);
}
extern "C" int64_t wun_spectral_terms_fft_scratch_floats(int32_t S, int32_t B, int64_t Tout, int32_t C, int32_t nres,
                                                         const int32_t* n_fft, const int32_t* hop, const wun_spectral_terms* terms) {
    return terms_scratch_entry("wun_spectral_terms_fft_scratch_floats", WUN_TR_FFT, S, B, Tout, C, nres, n_fft, hop, terms);
}

extern "C" int wun_spectral_loss_terms(const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
                                       float mse_weight, int32_t nres, const int32_t* n_fft, const int32_t* hop,
                                       const float* weights, const wun_spectral_terms* terms, const float* const* tables_dev,
                                       float* d_outputs, float* losses, float* scratch, void* stream) {
    return terms_entry("wun_spectral_loss_terms", WUN_TR_GEMM, outputs, targets, S, B, Tout, C, mse_weight, nres, n_fft, hop, weights,
                       terms, tables_dev, d_outputs, losses, scratch, stream);
}
extern "C" int wun_spectral_loss_terms_fft(const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
                                           float mse_weight, int32_t nres, const int32_t* n_fft, const int32_t* hop,
                                           const float* weights, const wun_spectral_terms* terms, const float* const* tables_dev,
                                           float* d_outputs, float* losses, float* scratch, void* stream) {
    return terms_entry("wun_spectral_loss_terms_fft", WUN_TR_FFT, outputs, targets, S, B, Tout, C, mse_weight, nres, n_fft, hop,
                       weights, terms, tables_dev, d_outputs, losses, scratch, stream);
}

// ---- the mel-scale terms' entries (include/wun.h) ----
extern "C" int64_t wun_mel_abi_size(void) { return (int64_t)sizeof(wun_mel_terms); }

extern "C" int64_t wun_mel_table_floats(int32_t n_fft, int32_t n_mels) {
    int rc;
    if ((rc = check_res("wun_mel_table_floats", WUN_TR_FFT, n_fft, 1))) return rc;
    if (n_mels < 1 || n_mels > WUN_MEL_MAX) return fail(WUN_ERR_INVALID, "wun_mel_table_floats: n_mels outside 1..512");
    return 3 * (int64_t)(n_fft / 2 + 1) + 2 * (int64_t)n_mels;
}

extern "C" int wun_mel_design(int32_t n_fft, double sample_rate, int32_t n_mels, double fmin, double fmax, int32_t norm,
                              float* table_host, int64_t cap) {
    const std::string w("wun_mel_design");
    const int64_t need = wun_mel_table_floats(n_fft, n_mels);
    if (need < 0) return (int)need;
    if (!(sample_rate > 0.0) || !std::isfinite(sample_rate)) return fail(WUN_ERR_INVALID, w + ": sample_rate must be finite and > 0");
    if (fmax == 0.0) fmax = 0.5 * sample_rate;
    if (!std::isfinite(fmin) || !std::isfinite(fmax) || fmin < 0.0 || !(fmin < fmax) || fmax > 0.5 * sample_rate)
        return fail(WUN_ERR_INVALID, w + ": need 0 <= fmin < fmax <= sample_rate / 2");
    if (norm != 0 && norm != 1) return fail(WUN_ERR_INVALID, w + ": norm must be 0 (none) or 1 (area)");
    if (!table_host) return fail(WUN_ERR_INVALID, w + ": null table");
    if (cap < need) return fail(WUN_ERR_INVALID, w + ": cap below wun_mel_table_floats");
    const int K = n_fft / 2 + 1;
    // the n_mels + 2 corner frequencies: equally spaced in mel, the two ends fmin and fmax themselves
    const double m0 = 2595.0 * std::log10(1.0 + fmin / 700.0), m1 = 2595.0 * std::log10(1.0 + fmax / 700.0);
    std::vector<double> c(n_mels + 2);
    for (int i = 0; i < n_mels + 2; ++i) c[i] = 700.0 * (std::pow(10.0, (m0 + (m1 - m0) * i / (n_mels + 1)) / 2595.0) - 1.0);
    c[0] = fmin; c[n_mels + 1] = fmax;
    std::vector<int32_t> b0(K, 0), lo(n_mels, K), hi(n_mels, 0), cnt(n_mels, 0);
    std::vector<float> w0(K, 0.f), w1(K, 0.f);
    for (int k = 0; k < K; ++k) {
        const double f = (double)k * sample_rate / (double)n_fft;
        int found = 0;
        for (int b = 0; b < n_mels; ++b) {
            const double up = (f - c[b]) / (c[b + 1] - c[b]), down = (c[b + 2] - f) / (c[b + 2] - c[b + 1]);
            double v = up < down ? up : down;
            if (!(v > 0.0)) continue;
            if (norm == 1) v *= 2.0 / (c[b + 2] - c[b]);
            const float v32 = (float)v;                          // the one rounding
            if (!(v32 > 0.f)) continue;
            if (found == 0) { b0[k] = b; w0[k] = v32; }
            else if (found == 1 && b == b0[k] + 1) w1[k] = v32;
            else return fail(WUN_ERR_INVALID, w + ": a bin weighted by more than two adjacent bands");
            ++found;
            if (k < lo[b]) lo[b] = k;
            hi[b] = k + 1;
            ++cnt[b];
        }
    }
    for (int b = 0; b < n_mels; ++b) {
        if (cnt[b] == 0)
            return fail(WUN_ERR_INVALID, w + ": band " + std::to_string(b) + " of " + std::to_string(n_mels) +
                        " weights no bin (it lies between two bins of this n_fft): fewer bands, a longer window or a higher fmin");
        if (cnt[b] != hi[b] - lo[b]) return fail(WUN_ERR_INVALID, w + ": band " + std::to_string(b) + " is not one run of bins");
    }
    int32_t* ti = (int32_t*)table_host;
    for (int k = 0; k < K; ++k) { ti[k] = b0[k]; table_host[K + k] = w0[k]; table_host[2 * K + k] = w1[k]; }
    for (int b = 0; b < n_mels; ++b) { ti[3 * K + b] = lo[b]; ti[3 * K + n_mels + b] = hi[b]; }
    return WUN_OK;
}

namespace {

int check_mel_op(const char* who, const void* a, const void* table, const void* out, int64_t M, int32_t K, int32_t n_mels) {
    const std::string w(who);
    if (!a || !table || !out) return fail(WUN_ERR_INVALID, w + ": null argument");
    if (M < 1 || M > ((int64_t)1 << 30)) return fail(WUN_ERR_INVALID, w + ": M outside 1..2^30");
    const int32_t n_fft = 2 * (K - 1);
    if (K < 33 || K > 4097 || (n_fft & (n_fft - 1))) return fail(WUN_ERR_INVALID, w + ": K must be n_fft / 2 + 1 of a power of two in 64..8192");
    if (n_mels < 1 || n_mels > WUN_MEL_MAX) return fail(WUN_ERR_INVALID, w + ": n_mels outside 1..512");
    return WUN_OK;
}

}  // namespace

extern "C" int wun_op_mel_project(const float* mags, int64_t M, int32_t K, int32_t n_mels, const float* mel_table_dev, float* out,
                                  void* stream) {
    int rc;
    if ((rc = check_mel_op("wun_op_mel_project", mags, mel_table_dev, out, M, K, n_mels))) return rc;
    launch_mel_project(mags, nullptr, out, nullptr, mel_table_dev, M, K, n_mels, (hipStream_t)stream);
    return launch_status("wun_op_mel_project");
}

extern "C" int wun_op_mel_project_transpose(const float* g, int64_t M, int32_t K, int32_t n_mels, const float* mel_table_dev,
                                            float* q, void* stream) {
    int rc;
    if ((rc = check_mel_op("wun_op_mel_project_transpose", g, mel_table_dev, q, M, K, n_mels))) return rc;
    const long long E = (long long)M * K;
    hipLaunchKernelGGL(mel_transpose_kernel, dim3((unsigned)((E + WUN_STFT_BLOCK - 1) / WUN_STFT_BLOCK)), dim3(WUN_STFT_BLOCK), 0,
                       (hipStream_t)stream, g, mel_table_dev, q, E, K, n_mels);
    return launch_status("wun_op_mel_project_transpose");
}

extern "C" int64_t wun_spectral_mel_scratch_floats(int32_t S, int32_t B, int64_t Tout, int32_t C, int32_t nres, const int32_t* n_fft,
                                                   const int32_t* hop, const wun_spectral_terms* terms, const wun_mel_terms* mel,
                                                   const int32_t* n_mels) {
    const MelCall mc = {mel, n_mels, nullptr};
    return terms_scratch_entry("wun_spectral_mel_scratch_floats", WUN_TR_GEMM, S, B, Tout, C, nres, n_fft, hop, terms, &mc);
}
extern "C" int64_t wun_spectral_mel_fft_scratch_floats(int32_t S, int32_t B, int64_t Tout, int32_t C, int32_t nres,
                                                       const int32_t* n_fft, const int32_t* hop, const wun_spectral_terms* terms,
                                                       const wun_mel_terms* mel, const int32_t* n_mels) {
    const MelCall mc = {mel, n_mels, nullptr};
    return terms_scratch_entry("wun_spectral_mel_fft_scratch_floats", WUN_TR_FFT, S, B, Tout, C, nres, n_fft, hop, terms, &mc);
}

extern "C" int wun_spectral_loss_mel(const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
                                     float mse_weight, int32_t nres, const int32_t* n_fft, const int32_t* hop, const float* weights,
                                     const wun_spectral_terms* terms, const float* const* tables_dev, float* d_outputs,
                                     float* losses, float* scratch, void* stream, const wun_mel_terms* mel, const int32_t* n_mels,
                                     const float* const* mel_tables_dev) {
    const MelCall mc = {mel, n_mels, mel_tables_dev};
    return terms_entry("wun_spectral_loss_mel", WUN_TR_GEMM, outputs, targets, S, B, Tout, C, mse_weight, nres, n_fft, hop, weights,
                       terms, tables_dev, d_outputs, losses, scratch, stream, &mc);
}
extern "C" int wun_spectral_loss_mel_fft(const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
                                         float mse_weight, int32_t nres, const int32_t* n_fft, const int32_t* hop,
                                         const float* weights, const wun_spectral_terms* terms, const float* const* tables_dev,
                                         float* d_outputs, float* losses, float* scratch, void* stream, const wun_mel_terms* mel,
                                         const int32_t* n_mels, const float* const* mel_tables_dev) {
    const MelCall mc = {mel, n_mels, mel_tables_dev};
    return terms_entry("wun_spectral_loss_mel_fft", WUN_TR_FFT, outputs, targets, S, B, Tout, C, mse_weight, nres, n_fft, hop,
                       weights, terms, tables_dev, d_outputs, losses, scratch, stream, &mc);
}
