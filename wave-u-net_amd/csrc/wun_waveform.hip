// gfx950 (MI355X / CDNA4): the waveform training losses (include/wun.h: wun_waveform_*) -- MSE and L1 over all
// floats, scale-invariant SDR and SNR per excerpt, their weighted total and its gradient with respect to the estimates.
//
//   row sums   per row r = (s, b), n = Tout C contiguous floats: sum e, t, e e, t t, e t, (e - t)^2 in float64 from the fp32
//              samples, over 1024-float chunks of the row's OWN floats (no block crosses a row: spec_sc_sums_kernel's pattern)
//   row coef   one block per row: the chunk partials strided over the lanes in ascending order, one tree per sum; thread 0 forms
//              the row's float64 scalars mu_e, mu_t, A, B, G, SI, SNR (the definitions are in the header)
//   gradient   one lane per output float (four per lane, 1024 per block, spec_grad_kernel's partition): the flat float64
//              partials of d^2 and |d|, and  g = cm d  (+ cl sgn d)  (+ (float)(A e' + B t' + G d'))  (+ old), each + one fp32 add
//   finish     one block: the flat partials strided over 64 lanes and one tree (spec_finish_kernel's), the per-source means of
//              SI and SNR, the terms and the total in slot order
//
// The flat sums are wun_spectral.hip's (wun_sum.h): with {mse: w} alone the losses and the gradient are wun_spectral_loss's at
// nres = 0, bit for bit.  No atomics, no allocation, no synchronisation; every argument check runs before any GPU work; scalar
// loads and stores, so any 4-byte alignment.  Built WITHOUT the packed fp32 VALU instructions (csrc/Makefile NO_PK_FP32, DESIGN.md
// 5.3): the loss runs between the forward and the backward pass of either compute mode.
#include "wun_stft.h"

#include <cmath>

using namespace wun;

#define WUN_WAVE_SUMS 6              // float64 sums per row: e, t, ee, tt, et, dd
#define WUN_WAVE_SCALARS 8           // float64 scalars per row: mu_e, mu_t, A, B, G, SI, SNR, (unused)

namespace wun {      // the kernels carry the library's wun:: prefix in profiler output

// grid: R * pc blocks; block b = (row r = b / pc, 1024-float chunk b - r pc of THAT row's n floats) -> part[6 b + q].  Every
// product is formed in float64 (exact for fp32 factors); for dd the difference is formed in float64 too.
__global__ __launch_bounds__(WUN_STFT_BLOCK) void wave_row_sums_kernel(const float* __restrict__ out, const float* __restrict__ tgt,
                                                                       double* __restrict__ part, long long n, long long pc) {
    __shared__ double red[WUN_WAVE_SUMS][WUN_STFT_BLOCK];
    const int tid = threadIdx.x;
    const long long r = (long long)blockIdx.x / pc, cb = (long long)blockIdx.x - r * pc;
    double a[WUN_WAVE_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int it = 0; it < WUN_STFT_ITEMS; ++it) {
        const long long el = (cb * WUN_STFT_ITEMS + it) * WUN_STFT_BLOCK + tid;
        if (el >= n) continue;
        const double e = (double)out[r * n + el], t = (double)tgt[r * n + el];
        const double d = e - t;
        a[0] += e; a[1] += t; a[2] += e * e; a[3] += t * t; a[4] += e * t; a[5] += d * d;
    }
    stft_block_sums<WUN_WAVE_SUMS>(red, a, tid);
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < WUN_WAVE_SUMS; ++q) part[WUN_WAVE_SUMS * (long long)blockIdx.x + q] = a[q];
    }
}

struct WaveCoefArgs {
    const double* part;              // [R][pc][6]
    double* scal;                    // [R][8]
    long long n, pc;
    double inv_r;                    // 1 / R
    float w_si, w_snr, eps;
    int zero_mean;
};

// grid: one block per row.  For each sum, lane l adds the row's chunk partials l, l + 256, ... in ascending order and one tree
// adds the lanes (the six trees share their barriers); thread 0 then forms the row's scalars, every operation in float64 and unfused, in the order written here.
__global__ __launch_bounds__(WUN_STFT_BLOCK) void wave_row_coef_kernel(WaveCoefArgs p) {
#pragma clang fp contract(off)
    __shared__ double red[WUN_WAVE_SUMS][WUN_STFT_BLOCK];
    const int tid = threadIdx.x;
    const long long r = blockIdx.x;
    const double* __restrict__ rp = p.part + WUN_WAVE_SUMS * r * p.pc;
    double s[WUN_WAVE_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long i = tid; i < p.pc; i += WUN_STFT_BLOCK) {
#pragma unroll
        for (int q = 0; q < WUN_WAVE_SUMS; ++q) s[q] += rp[WUN_WAVE_SUMS * i + q];
    }
    stft_block_sums<WUN_WAVE_SUMS>(red, s, tid);
    if (tid != 0) return;
    const double k = 4.342944819032518;                     // 10 / ln 10
    const double n = (double)p.n, eps = (double)p.eps;
    double mue = 0.0, mut = 0.0, See = s[2], Stt = s[3], Set = s[4], Dd = s[5];
    if (p.zero_mean) {
        mue = s[0] / n; mut = s[1] / n;
        const double dm = s[0] - s[1];
        See = fmax(s[2] - s[0] * mue, 0.0);
        Stt = fmax(s[3] - s[1] * mut, 0.0);
        Set = s[4] - s[0] * mut;
        Dd = fmax(s[5] - dm * dm / n, 0.0);
    }
    double A = 0.0, B = 0.0, G = 0.0, SI = 0.0, SNR = 0.0;
    if (p.w_si > 0.f) {
        const double w = (double)p.w_si;
        const double P = Set * Set / (Stt + eps);
        const double Nn = fmax(See - P, 0.0);
        SI = 10.0 * log10((P + eps) / (Nn + eps));
        A = 2.0 * k * w * p.inv_r / (Nn + eps);
        B = -(w * k * p.inv_r) * (2.0 * Set / (Stt + eps)) * (1.0 / (P + eps) + 1.0 / (Nn + eps));
    }
    if (p.w_snr > 0.f) {
        SNR = 10.0 * log10((Stt + eps) / (Dd + eps));
        G = 2.0 * k * (double)p.w_snr * p.inv_r / (Dd + eps);
    }
    double* __restrict__ o = p.scal + WUN_WAVE_SCALARS * r;
    o[0] = mue; o[1] = mut; o[2] = A; o[3] = B; o[4] = G; o[5] = SI; o[6] = SNR; o[7] = 0.0;
}

struct WaveGradArgs {
    const float* out; const float* tgt;      // [S, B, Tout, C]
    float* dout;                             // the same shape (GRAD only)
    double* part_sq; double* part_ab;        // [ceil(N / 1024)] each: sums of d^2 and of |d|
    const double* scal;                      // [R][8] (rows only)
    long long N, n;                          // floats in all, floats per row
    float cm, cl;                            // mse * 2 / N, l1 / N
    int mse, l1, rows;                       // which parts are computed
};

// spec_grad_kernel's partition: block b covers the floats 1024 b ..; lane tid takes tid + 256 it.  d = out - tgt in fp32.  The
// gradient in fp32, unfused and in this order: cm d (mse), + cl sgn(d) (l1), + (float)v (row terms), + the old value (ACC), where
// v = (A e' + B t') + G d' in float64, e' = e - mu_e, t' = t - mu_t, d' = e' - t', every operation rounded on its own.
template <bool GRAD, bool ACC>
__global__ __launch_bounds__(WUN_STFT_BLOCK) void wave_grad_kernel(WaveGradArgs p) {
#pragma clang fp contract(off)
    __shared__ double red[2][WUN_STFT_BLOCK];
    const int tid = threadIdx.x;
    double sq = 0.0, ab = 0.0;
    // the row of this lane's first float and the float's place in it: one 64-bit division per lane, then steps of 256
    long long row = 0, at = 0;
    if (GRAD && p.rows) {
        const long long e0 = (long long)blockIdx.x * WUN_STFT_ITEMS * WUN_STFT_BLOCK + tid;
        row = e0 / p.n; at = e0 - row * p.n;
    }
#pragma unroll
    for (int it = 0; it < WUN_STFT_ITEMS; ++it) {
        const long long e = ((long long)blockIdx.x * WUN_STFT_ITEMS + it) * WUN_STFT_BLOCK + tid;
        if (e >= p.N) continue;
        if (GRAD && p.rows && it > 0) {
            at += WUN_STFT_BLOCK;
            if (at >= p.n) {
                if (p.n >= WUN_STFT_BLOCK) { at -= p.n; ++row; }             // at most one row further
                else { const long long q = at / p.n; row += q; at -= q * p.n; }
            }
        }
        const float eo = p.out[e], et = p.tgt[e];
        const float d = eo - et;
        if (p.mse) sq += (double)d * (double)d;
        if (p.l1) ab += (double)fabsf(d);
        if (GRAD) {
            float g = p.cm != 0.f ? p.cm * d : 0.f;
            if (p.l1) g += p.cl * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
            if (p.rows) {
                const double* __restrict__ c = p.scal + WUN_WAVE_SCALARS * row;
                const double ep = (double)eo - c[0], tp = (double)et - c[1];
                const double dp = ep - tp;
                const double v = (c[2] * ep + c[3] * tp) + c[4] * dp;
                g += (float)v;
            }
            grad_st<ACC>(p.dout + e, g);
        }
    }
    if (p.mse && p.l1) {                                     // (both trees behind one set of barriers: the same adds)
        double v[2] = {sq, ab};
        stft_block_sums<2>(red, v, tid);
        if (tid == 0) { p.part_sq[blockIdx.x] = v[0]; p.part_ab[blockIdx.x] = v[1]; }
    } else if (p.mse) {
        const double s = stft_block_sum(red[0], sq, tid);
        if (tid == 0) p.part_sq[blockIdx.x] = s;
    } else if (p.l1) {
        const double s = stft_block_sum(red[1], ab, tid);
        if (tid == 0) p.part_ab[blockIdx.x] = s;
    }
}

struct WaveFinishArgs {
    const double* part[2];           // the flat partials of d^2 and |d|
    long long nparts[2];             // 0: the sum is not taken
    const double* scal;              // [R][8] (rows only)
    double count;                    // N
    float w[4];                      // mse, l1, si_sdr, snr
    int S, B, rows;
    float* losses;                   // [5 + 2 S]
};

// One block of 256.  Wave 0 takes the partials of d^2 and wave 1 those of |d| as spec_finish_kernel does: lane l adds the
// partials l, l + 64, ... in ascending order, one tree over the 64 lanes.  Then source after source lane l of the block adds SI_r
// and SNR_r of the rows b = l, l + 256, ... of that source, one tree each; thread 0 forms the terms and the total in slot order.
__global__ __launch_bounds__(WUN_STFT_BLOCK) void wave_finish_kernel(WaveFinishArgs p) {
#pragma clang fp contract(off)
    __shared__ double red[2][WUN_STFT_BLOCK];
    __shared__ double flat[2];
    const int tid = threadIdx.x, slot = tid >> 6, lane = tid & 63;
    double s = 0.0;
    if (slot < 2)
        for (long long i = lane; i < p.nparts[slot]; i += 64) s += p.part[slot][i];
    red[0][tid] = s;
    __syncthreads();
    for (int h = 32; h > 0; h >>= 1) {
        if (lane < h) red[0][tid] += red[0][tid + h];
        __syncthreads();
    }
    if (slot < 2 && lane == 0) flat[slot] = red[0][tid];
    __syncthreads();
    double si_all = 0.0, snr_all = 0.0;                      // the sums over all rows, source after source (thread 0's copy counts)
    for (int src = 0; src < p.S; ++src) {
        double a = 0.0, b = 0.0;
        if (p.rows)
            for (int i = tid; i < p.B; i += WUN_STFT_BLOCK) {
                const double* __restrict__ c = p.scal + WUN_WAVE_SCALARS * ((long long)src * p.B + i);
                a += c[5]; b += c[6];
            }
        if (p.rows) {                                        // (uniform: every lane takes the trees or none does)
            a = stft_block_sum(red[0], a, tid);
            b = stft_block_sum(red[1], b, tid);
            __syncthreads();                                 // red[.][0] is read by every lane before the next source writes it
        }
        if (tid == 0) {
            p.losses[5 + src] = (float)(a / (double)p.B);
            p.losses[5 + p.S + src] = (float)(b / (double)p.B);
        }
        si_all += a; snr_all += b;
    }
    if (tid == 0) {
        const double R = (double)p.S * (double)p.B;
        double term[4] = {0.0, 0.0, 0.0, 0.0};
        if (p.w[0] > 0.f) term[0] = flat[0] / p.count;
        if (p.w[1] > 0.f) term[1] = flat[1] / p.count;
        if (p.w[2] > 0.f) term[2] = -(si_all / R);
        if (p.w[3] > 0.f) term[3] = -(snr_all / R);
        double total = 0.0;
        for (int t = 0; t < 4; ++t) {
            p.losses[1 + t] = (float)term[t];
            if (p.w[t] > 0.f) total += (double)p.w[t] * term[t];
        }
        p.losses[0] = (float)total;
    }
}

}  // namespace wun

namespace {

int check_wave_terms(const char* who, const wun_waveform_terms* t) {
    const std::string w(who);
    if (!t) return fail(WUN_ERR_INVALID, w + ": null terms");
    for (float x : {t->mse, t->l1, t->si_sdr, t->snr})
        if (!(x >= 0.f) || !std::isfinite(x)) return fail(WUN_ERR_INVALID, w + ": a term weight negative or not finite");
    if (!(t->eps > 0.f) || !std::isfinite(t->eps)) return fail(WUN_ERR_INVALID, w + ": eps must be finite and > 0");
    return WUN_OK;
}

}  // namespace

extern "C" int64_t wun_waveform_scratch_floats(int32_t S, int32_t B, int64_t Tout, int32_t C, const wun_waveform_terms* terms) {
    const char* who = "wun_waveform_scratch_floats";
    int rc;
    if ((rc = check_audio(who, S, B, Tout, C))) return rc;
    if ((rc = check_wave_terms(who, terms))) return rc;
    const long long R = (long long)S * B, n = (long long)Tout * C;
    const long long doubles = 2 * parts_of(R * n) + WUN_WAVE_SUMS * R * parts_of(n) + WUN_WAVE_SCALARS * R;
    return 2 * doubles + 2;                                  // and room to align them to 8 bytes
}

extern "C" int wun_waveform_loss(const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
                                 const wun_waveform_terms* terms, int32_t accumulate, float* d_outputs, float* losses,
                                 float* scratch, void* stream) {
    const char* who = "wun_waveform_loss";
    const std::string w(who);
    if (!outputs || !targets || !losses || !scratch) return fail(WUN_ERR_INVALID, w + ": null argument");
    int rc;
    if ((rc = check_audio(who, S, B, Tout, C))) return rc;
    if ((rc = check_wave_terms(who, terms))) return rc;
    if (accumulate != 0 && accumulate != 1) return fail(WUN_ERR_INVALID, w + ": accumulate must be 0 or 1");
    if (accumulate == 1 && !d_outputs) return fail(WUN_ERR_INVALID, w + ": accumulate needs d_outputs");
    const wun_waveform_terms tw = *terms;

    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(WUN_STFT_BLOCK);
    const long long R = (long long)S * B, n = (long long)Tout * C, N = R * n;
    const long long pN = parts_of(N), pc = parts_of(n);
    const bool grad = d_outputs != nullptr, rows = tw.si_sdr > 0.f || tw.snr > 0.f;
    // scratch, float64 on an 8-byte boundary: [pN] partials of d^2 | [pN] of |d| | [R][pc][6] row partials | [R][8] row scalars
    double* part = f64_tail(scratch, 0);
    double* rpart = part + 2 * pN;
    double* scal = rpart + WUN_WAVE_SUMS * R * pc;

    if (rows) {
        hipLaunchKernelGGL(wave_row_sums_kernel, dim3((unsigned)(R * pc)), blk, 0, s, outputs, targets, rpart, n, pc);
        WaveCoefArgs c;
        c.part = rpart; c.scal = scal; c.n = n; c.pc = pc; c.inv_r = 1.0 / (double)R;
        c.w_si = tw.si_sdr; c.w_snr = tw.snr; c.eps = tw.eps; c.zero_mean = tw.zero_mean != 0;
        hipLaunchKernelGGL(wave_row_coef_kernel, dim3((unsigned)R), blk, 0, s, c);
    }
    WaveGradArgs g;
    g.out = outputs; g.tgt = targets; g.dout = d_outputs; g.part_sq = part; g.part_ab = part + pN; g.scal = scal;
    g.N = N; g.n = n;
    g.cm = (float)((double)tw.mse * 2.0 / (double)N);
    g.cl = (float)((double)tw.l1 / (double)N);
    g.mse = tw.mse > 0.f; g.l1 = tw.l1 > 0.f; g.rows = rows;
    const dim3 ggrid((unsigned)pN);
    if (!grad) hipLaunchKernelGGL((wave_grad_kernel<false, false>), ggrid, blk, 0, s, g);
    else if (accumulate) hipLaunchKernelGGL((wave_grad_kernel<true, true>), ggrid, blk, 0, s, g);
    else hipLaunchKernelGGL((wave_grad_kernel<true, false>), ggrid, blk, 0, s, g);

    WaveFinishArgs f;
    f.part[0] = part; f.part[1] = part + pN;
    f.nparts[0] = g.mse ? pN : 0; f.nparts[1] = g.l1 ? pN : 0;
    f.scal = scal; f.count = (double)N;
    f.w[0] = tw.mse; f.w[1] = tw.l1; f.w[2] = tw.si_sdr; f.w[3] = tw.snr;
    f.S = S; f.B = B; f.rows = rows; f.losses = losses;
    hipLaunchKernelGGL(wave_finish_kernel, dim3(1), blk, 0, s, f);
    return launch_status(who);
}
