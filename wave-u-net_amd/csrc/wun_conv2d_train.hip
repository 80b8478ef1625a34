// gfx950 (MI355X / CDNA4): one training step of the spectrogram U-Net for the magnitude objective (include/wun.h:
// wun_spec_train_forward, wun_spec_loss_backward, wun_spec_adam_step, wun_op_conv2d_s2_wgrad, wun_op_conv2d_transpose_s2_wgrad,
// wun_op_bn2d_stats; Models/UnetSpectrogramSeparator.py:63-92 at training = True, Training.py:47-77), and the same
// backward pass from any upstream gradient on the magnitudes, the audio or both (wun_spec_backward, wun_spec_train_audio,
// wun_spec_update_moving_averages, wun_op_spec_head_backward).
//
//   forward    every layer with a batch norm: z = conv + bias (wun_conv2d.hip's kernels, act 0), per channel mu = mean z and
//              var = mean (z - mu)^2 (biased, two passes), a = act((z - mu) / sqrt(var + 1e-3) + beta).  Dropout multiplies the
//              concatenation [skip, up] of the up levels i < 3 by a stored mask (0 or 1 / (1 - rate)); those three small
//              concatenations are materialised, every other one stays virtual.
//   loss       (1 / S) sum_s mean |R_s - M mask_s| over all K bins; dz of the mask layer for k < K - 1
//   backward   batch norm without gamma: dz = rstd (g' - mean g' - xh mean(g' xh)), g' the gradient behind the activation.
//              Data gradients are wun_conv2d.hip's two kernels with the weights read the other way round.  Weight gradients:
//              G[ky][kx][p][q] = sum_{b,y,x} Big[b][2y + ky - 1][2x + kx - 1][p] Small[b][y][x][q] (zeros outside Big) as a
//              GEMM of 25 C_big rows, C_small columns and a reduction over the B Hs Ws pixels of the small map.  The reduction
//              is cut into chunks of WUN_WG_CHUNK pixels (a function of the shapes alone), one workgroup per (tile, chunk)
//              writes its partial tile to scratch, a second pass adds the chunks in ascending order.  Exact-fp32 MFMA on
//              wun_stft.h's tile where both channel counts exceed 1, one lane per output on the VALU otherwise.
//   head       wun_spec_backward's first launches per source in place of the loss's: dz of the mask layer from d_mags (one lane
//              per bin) and / or d_audio (u = d_audio / D, then wun_fft.hip's forward FFT with the mask gradient as its epilogue);
//              everything behind dz is network_backward, the one body of both entries
//   sums       per-channel sums (statistics, the two means of the batch-norm backward, bias gradients) and the loss are float64
//              partials over 1024 consecutive pixels / bins, added in ascending order by one fixed tree.  No atomics anywhere:
//              the bits depend on neither the grid, what the workspace held nor pointer alignment beyond 4 bytes.
//   Adam       wun_adam_step_select's kernel over the runs of kernels, biases and betas (the moving statistics and their slots
//              are not touched), then the moving averages from the batch statistics of the last forward.
//
// Built WITHOUT the packed fp32 VALU instructions (csrc/Makefile NO_PK_FP32).  Every argument check runs before
// any GPU work; nothing allocates or synchronises.
#include "wun_conv2d.h"
#include "wun_fft.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace wun;

#define WUN_WG_CHUNK 256             // pixels of the small map per split-reduction chunk (a multiple of WUN_STFT_KC)
#define WUN_SUM_ROWS (WUN_STFT_BLOCK * WUN_STFT_ITEMS)     // 1024 pixels / bins per float64 partial
#define WUN_SPEC_DROP_LEVELS 3       // tf.layers.dropout on the concatenation of up levels i < 3 (UnetSpectrogramSeparator.py:82)

namespace wun {

// ---- dropout: the keep bit of include/wun.h ----
__host__ __device__ __forceinline__ unsigned long long drop_mix(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ unsigned long long drop_key(long long seed, long long step, int source, int level) {
    return drop_mix(drop_mix(drop_mix((unsigned long long)seed) + (unsigned long long)step) +
                    (((unsigned long long)source << 8) | (unsigned long long)level));
}
__device__ __forceinline__ bool drop_keep(unsigned long long key, long long e, float rate) {
    const unsigned u = (unsigned)(drop_mix(key + (unsigned long long)e) >> 40);        // 24 bits
    return (float)u * 5.9604644775390625e-08f >= rate;                                  // u 2^-24, exact
}

// THE factor between the batch variance and what the moving average receives (TF's fused batch norm: n / max(n - 1, 1))
__device__ __forceinline__ float bn_unbiased(float var, long long n) {
    return var * (float)((double)n / (double)(n > 1 ? n - 1 : 1));
}

// ---- the weight gradient ----
struct WgArgs {
    const float* big;                        // [B][2 Hs][2 Ws][Cb]
    const float* s0;                         // [B][Hs][Ws][c0]
    const float* s1;                         // [B][Hs][Ws][c1] or null: the small operand is the virtual concatenation
    float* part;                             // [chunks][25 Cb][c0 + c1]
    long long nred;                          // B Hs Ws
    int Hs, Ws, Cb, c0, c1;
};

__device__ __forceinline__ float wg_small(const WgArgs& a, long long px, int q) {
    return q < a.c0 ? a.s0[px * a.c0 + q] : a.s1[px * a.c1 + (q - a.c0)];
}

// grid: x = tile of 64 rows (ky, kx, p), y = tile of 32 columns q, z = chunk of the reduction
__global__ __launch_bounds__(WUN_STFT_BLOCK) void wgrad2d_mfma_kernel(WgArgs a) {
    __shared__ float As[WUN_STFT_BM * WUN_STFT_PA];
    __shared__ float Bs[WUN_STFT_KC * WUN_STFT_PB];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int sc = tid & 31, sr = tid >> 5;                  // B staging: column, first reduction index
    const int M = 25 * a.Cb, N = a.c0 + a.c1;
    const int m0 = (int)blockIdx.x * WUN_STFT_BM, n0 = (int)blockIdx.y * WUN_STFT_BN;
    const int wm = (w & 1) * 32, wn = (w >> 1) * 16;
    const long long cbeg = (long long)blockIdx.z * WUN_WG_CHUNK;
    const long long cend = cbeg + WUN_WG_CHUNK < a.nred ? cbeg + WUN_WG_CHUNK : a.nred;
    const int Hb = 2 * a.Hs, Wb = 2 * a.Ws;

    // A staging: this lane's row (consecutive lanes read consecutive channels of Big), the wave's reduction indices w + 4 it
    const int ar = m0 + lane;
    const bool rin = ar < M;
    const int tap = rin ? ar / a.Cb : 0, ky = tap / 5, kx = tap - 5 * ky, p = rin ? ar - tap * a.Cb : 0;
    const bool nin = n0 + sc < N;

    f32x4 acc[2];
    acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
    for (long long k0 = cbeg; k0 < cend; k0 += WUN_STFT_KC) {        // ascending pixels: the one accumulation order of a chunk
        __syncthreads();
#pragma unroll
        for (int it = 0; it < WUN_STFT_KC / 4; ++it) {
            const int kl = w + 4 * it;
            const long long px = k0 + kl;
            float v = 0.f;
            if (rin && px < cend) {
                const long long b = px / ((long long)a.Hs * a.Ws), rest = px - b * a.Hs * a.Ws;
                const int yy = 2 * (int)(rest / a.Ws) + ky - 1, xx = 2 * (int)(rest % a.Ws) + kx - 1;
                if ((unsigned)yy < (unsigned)Hb && (unsigned)xx < (unsigned)Wb) v = a.big[((b * Hb + yy) * Wb + xx) * a.Cb + p];
            }
            As[lane * WUN_STFT_PA + kl] = v;
        }
#pragma unroll
        for (int it = 0; it < WUN_STFT_KC / 8; ++it) {
            const int kl = sr + 8 * it;
            const long long px = k0 + kl;
            Bs[kl * WUN_STFT_PB + sc] = (nin && px < cend) ? wg_small(a, px, n0 + sc) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < WUN_STFT_KC / 4; ++s) {
            const int kq = 4 * s + lq;
            const float a0 = As[(wm + lr) * WUN_STFT_PA + kq], a1 = As[(wm + 16 + lr) * WUN_STFT_PA + kq];
            const float b = Bs[kq * WUN_STFT_PB + wn + lr];
            acc[0] = stft_mfma(a0, b, acc[0]);
            acc[1] = stft_mfma(a1, b, acc[1]);
        }
    }
    const int n = n0 + wn + lr;
    if (n >= N) return;
    float* out = a.part + (long long)blockIdx.z * M * N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wm + 16 * i + 4 * lq + r;
            if (m < M) out[(long long)m * N + n] = acc[i][r];
        }
}

// the thin layers (C_big == 1: the first down layer; C_small == 1): one lane per output, the same chunks
// grid: x = 256 outputs (row-major [25 Cb][Cs]), y = chunk
__global__ __launch_bounds__(WUN_STFT_BLOCK) void wgrad2d_valu_kernel(WgArgs a) {
    const int N = a.c0 + a.c1;
    const long long MN = 25LL * a.Cb * N;
    const long long o = (long long)blockIdx.x * WUN_STFT_BLOCK + threadIdx.x;
    if (o >= MN) return;
    const int r = (int)(o / N), q = (int)(o - (long long)r * N);
    const int tap = r / a.Cb, ky = tap / 5, kx = tap - 5 * ky, p = r - tap * a.Cb;
    const long long cbeg = (long long)blockIdx.y * WUN_WG_CHUNK;
    const long long cend = cbeg + WUN_WG_CHUNK < a.nred ? cbeg + WUN_WG_CHUNK : a.nred;
    const int Hb = 2 * a.Hs, Wb = 2 * a.Ws;
    float acc = 0.f;
    for (long long px = cbeg; px < cend; ++px) {
        const long long b = px / ((long long)a.Hs * a.Ws), rest = px - b * a.Hs * a.Ws;
        const int yy = 2 * (int)(rest / a.Ws) + ky - 1, xx = 2 * (int)(rest % a.Ws) + kx - 1;
        float v = 0.f;
        if ((unsigned)yy < (unsigned)Hb && (unsigned)xx < (unsigned)Wb) v = a.big[((b * Hb + yy) * Wb + xx) * a.Cb + p];
        acc = fmaf(v, wg_small(a, px, q), acc);
    }
    a.part[(long long)blockIdx.y * MN + o] = acc;
}

// the second pass: out[o] = sum of the chunks' partials in ascending order
__global__ __launch_bounds__(WUN_STFT_BLOCK) void wgrad2d_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                                       long long MN, int chunks) {
    for (long long o = (long long)blockIdx.x * WUN_STFT_BLOCK + threadIdx.x; o < MN; o += (long long)gridDim.x * WUN_STFT_BLOCK) {
        float acc = part[o];
        for (int c = 1; c < chunks; ++c) acc += part[(long long)c * MN + o];
        out[o] = acc;
    }
}

// ---- per-channel sums over [n][C] tensors ----
enum { CH_SUM = 0, CH_SQDEV = 1, CH_BNBWD = 2 };

struct ChanArgs {
    const float* x;                          // SUM: the tensor;  SQDEV: z;  BNBWD: g
    const float* g2;                         // BNBWD: a second gradient added to g, or null
    const float* z;                          // BNBWD
    const float* mean;                       // SQDEV, BNBWD
    const float* var;                        // BNBWD
    const float* beta;                       // BNBWD
    double* part;                            // [2][blocks][C]
    long long n;
    int C, CT, act;
};

// the gradient behind the activation: ReLU passes where zhat > 0; LeakyReLU = max(0.2 x, x) has slope 1 where zhat > 0, 0.2 elsewhere
__device__ __forceinline__ float act_grad(int act, float zhat, float g) {
    if (act == C2D_ACT_LRELU) return zhat > 0.f ? g : 0.2f * g;
    return zhat > 0.f ? g : 0.f;
}

// grid: x = block of 1024 pixels, y = tile of CT channels (CT a power of two <= 64: lane = channel, 256 / CT pixel rows at once)
template <int MODE>
__global__ __launch_bounds__(WUN_STFT_BLOCK) void chan_sums_kernel(ChanArgs a) {
    __shared__ double red[2][WUN_STFT_BLOCK];
    const int tid = threadIdx.x, cl = tid & (a.CT - 1), rr = tid / a.CT, RS = WUN_STFT_BLOCK / a.CT;
    const int c = (int)blockIdx.y * a.CT + cl;
    const long long p0 = (long long)blockIdx.x * WUN_SUM_ROWS;
    double v0 = 0.0, v1 = 0.0;
    if (c < a.C) {
        float mu = 0.f, rstd = 0.f, be = 0.f;
        if (MODE != CH_SUM) mu = a.mean[c];
        if (MODE == CH_BNBWD) { rstd = 1.0f / sqrtf(a.var[c] + WUN_C2D_EPS); be = a.beta[c]; }
        for (int j = rr; j < WUN_SUM_ROWS; j += RS) {        // ascending pixels
            const long long px = p0 + j;
            if (px >= a.n) break;
            const long long e = px * a.C + c;
            if (MODE == CH_SUM) v0 += (double)a.x[e];
            else if (MODE == CH_SQDEV) { const double d = (double)a.x[e] - (double)mu; v0 += d * d; }
            else {
                const float xh = (a.z[e] - mu) * rstd;
                float g = a.x[e];
                if (a.g2) g += a.g2[e];
                const float gp = act_grad(a.act, xh + be, g);
                v0 += (double)gp;
                v1 += (double)gp * (double)xh;
            }
        }
    }
    red[0][tid] = v0; red[1][tid] = v1;
    __syncthreads();
    if (rr == 0 && c < a.C) {
        double s0 = 0.0, s1 = 0.0;
        for (int r = 0; r < RS; ++r) { s0 += red[0][r * a.CT + cl]; s1 += red[1][r * a.CT + cl]; }      // ascending rows
        a.part[(long long)blockIdx.x * a.C + c] = s0;
        a.part[((long long)gridDim.x + blockIdx.x) * a.C + c] = s1;
    }
}

// grid: x = channel.  s_q = the blocks' partials of sum q, lane tid taking tid + 256 j in ascending order, then the fixed tree.
// o0 = (float)(s_0 scale), o1 = (float)(s_1 scale), o2 = (float)s_0; null outputs are not written.
__global__ __launch_bounds__(WUN_STFT_BLOCK) void chan_finish_kernel(const double* __restrict__ part, long long blocks, int C,
                                                                    double scale, float* o0, float* o1, float* o2) {
    __shared__ double red[2][WUN_STFT_BLOCK];
    const int tid = threadIdx.x, c = (int)blockIdx.x;
    double v[2] = {0.0, 0.0};
    for (long long j = tid; j < blocks; j += WUN_STFT_BLOCK) {
        v[0] += part[j * C + c];
        v[1] += part[(blocks + j) * C + c];
    }
    stft_block_sums<2>(red, v, tid);
    if (tid == 0) {
        if (o0) o0[c] = (float)(v[0] * scale);
        if (o1) o1[c] = (float)(v[1] * scale);
        if (o2) o2[c] = (float)v[0];
    }
}

// a = act((z - mean) / sqrt(var + 1e-3) + beta): the epilogue of wun_conv2d.hip on batch statistics.  E = n C.
__global__ __launch_bounds__(WUN_STFT_BLOCK) void bn_apply_kernel(const float* __restrict__ z, const float* __restrict__ mean,
                                                                 const float* __restrict__ var, const float* __restrict__ beta,
                                                                 float* __restrict__ y, long long E, int C, int act) {
    for (long long e = (long long)blockIdx.x * WUN_STFT_BLOCK + threadIdx.x; e < E; e += (long long)gridDim.x * WUN_STFT_BLOCK) {
        const int c = (int)(e % C);
        float v = (z[e] - mean[c]) * (1.0f / sqrtf(var[c] + WUN_C2D_EPS)) + beta[c];
        if (act == C2D_ACT_LRELU) v = v > 0.f ? v : 0.2f * v;
        else v = v > 0.f ? v : (v != v ? v : 0.f);
        y[e] = v;
    }
}

// dz = rstd (g' - mean g' - xh mean(g' xh)); mg, mgx: the two means, per channel
__global__ __launch_bounds__(WUN_STFT_BLOCK) void bn_bwd_kernel(const float* __restrict__ g1, const float* g2,
                                                               const float* __restrict__ z, const float* __restrict__ mean,
                                                               const float* __restrict__ var, const float* __restrict__ beta,
                                                               const float* __restrict__ mg, const float* __restrict__ mgx,
                                                               float* __restrict__ dz, long long E, int C, int act) {
    for (long long e = (long long)blockIdx.x * WUN_STFT_BLOCK + threadIdx.x; e < E; e += (long long)gridDim.x * WUN_STFT_BLOCK) {
        const int c = (int)(e % C);
        const float rstd = 1.0f / sqrtf(var[c] + WUN_C2D_EPS);
        const float xh = (z[e] - mean[c]) * rstd;
        float g = g1[e];
        if (g2) g += g2[e];
        const float gp = act_grad(act, xh + beta[c], g);
        dz[e] = rstd * ((gp - mg[c]) - xh * mgx[c]);
    }
}

// the dropped concatenation: cat = [s0, s1] * dmask, dmask = keep ? scale : 0.  E = n (c0 + c1).
__global__ __launch_bounds__(WUN_STFT_BLOCK) void dropout_concat_kernel(const float* __restrict__ s0, const float* __restrict__ s1,
                                                                       float* __restrict__ dmask, float* __restrict__ cat,
                                                                       long long E, int c0, int c1, unsigned long long key,
                                                                       float rate, float scale) {
    const int Cc = c0 + c1;
    for (long long e = (long long)blockIdx.x * WUN_STFT_BLOCK + threadIdx.x; e < E; e += (long long)gridDim.x * WUN_STFT_BLOCK) {
        const long long px = e / Cc;
        const int c = (int)(e - px * Cc);
        const float v = c < c0 ? s0[px * c0 + c] : s1[px * c1 + (c - c0)];
        const float mk = drop_keep(key, e, rate) ? scale : 0.f;
        dmask[e] = mk;
        cat[e] = v * mk;
    }
}

// the gradient of a concatenation [n][c0 + c1], times the dropout mask where there is one: the first c0 channels to the skip's
// gradient, the rest to the up layer's
__global__ __launch_bounds__(WUN_STFT_BLOCK) void concat_split_kernel(const float* __restrict__ g, const float* dmask,
                                                                     float* __restrict__ gskip, float* __restrict__ gup,
                                                                     long long E, int c0, int c1) {
    const int Cc = c0 + c1;
    for (long long e = (long long)blockIdx.x * WUN_STFT_BLOCK + threadIdx.x; e < E; e += (long long)gridDim.x * WUN_STFT_BLOCK) {
        const long long px = e / Cc;
        const int c = (int)(e - px * Cc);
        const float v = dmask ? g[e] * dmask[e] : g[e];
        if (c < c0) gskip[px * c0 + c] = v;
        else gup[px * c1 + (c - c0)] = v;
    }
}

// The loss of one source: block `blockIdx.x` sums |R - M mask| over its 1024 bins (lane tid: tid + 256 it, ascending; the fixed
// tree) into part[blockIdx.x] and writes dz of the mask layer for k < K - 1: -sign(d) M cm mask (1 - mask).
__global__ __launch_bounds__(WUN_STFT_BLOCK) void spec_loss_kernel(const float* __restrict__ R, const float* __restrict__ mag,
                                                                  const float* __restrict__ mask, float* __restrict__ dz,
                                                                  double* __restrict__ part, long long E, int K, float cm) {
    __shared__ double red[WUN_STFT_BLOCK];
    const int tid = threadIdx.x;
    double v = 0.0;
#pragma unroll
    for (int it = 0; it < WUN_STFT_ITEMS; ++it) {
        const long long e = (long long)blockIdx.x * WUN_SUM_ROWS + tid + WUN_STFT_BLOCK * it;
        if (e < E) {
            const long long bf = e / K;
            const int k = (int)(e - bf * K);
            const float mk = k < K - 1 ? mask[bf * (K - 1) + k] : 0.5f;
            const float m = mag[e];
            const float d = R[e] - m * mk;
            v += (double)fabsf(d);
            if (k < K - 1) {
                const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
                dz[bf * (K - 1) + k] = (-sg * m * cm) * (mk * (1.0f - mk));
            }
        }
    }
    const double s = stft_block_sum(red, v, tid);
    if (tid == 0) part[blockIdx.x] = s;
}

// The head of wun_spec_backward for an upstream gradient on the magnitudes alone: one lane per bin (grid-stride),
// dz = (d_mags M) * (mask (1 - mask)) for k < K - 1.  With d_mags = -sign(R - M mask) cm it writes spec_loss_kernel's bits.
__global__ __launch_bounds__(WUN_STFT_BLOCK) void spec_head_mags_kernel(const float* __restrict__ dmags, const float* __restrict__ mag,
                                                                       const float* __restrict__ mask, float* __restrict__ dz,
                                                                       long long E, int K) {
    for (long long e = (long long)blockIdx.x * WUN_STFT_BLOCK + threadIdx.x; e < E; e += (long long)gridDim.x * WUN_STFT_BLOCK) {
        const long long bf = e / K;
        const int k = (int)(e - bf * K);
        if (k == K - 1) continue;
        const float mk = mask[bf * (K - 1) + k];
        dz[bf * (K - 1) + k] = (dmags[e] * mag[e]) * (mk * (1.0f - mk));
    }
}

// one block: losses[1 + s] = mean of source s, losses[0] = their mean
__global__ __launch_bounds__(WUN_STFT_BLOCK) void spec_loss_finish_kernel(const double* __restrict__ part, long long blocks, int S,
                                                                         double inv_e, float* __restrict__ losses) {
    __shared__ double red[WUN_STFT_BLOCK];
    const int tid = threadIdx.x;
    double total = 0.0;
    for (int s = 0; s < S; ++s) {
        double v = 0.0;
        for (long long j = tid; j < blocks; j += WUN_STFT_BLOCK) v += part[(long long)s * blocks + j];
        const double sum = stft_block_sum(red, v, tid) * inv_e;
        __syncthreads();
        if (tid == 0) losses[1 + s] = (float)sum;
        total += sum;
    }
    if (tid == 0) losses[0] = (float)(total / (double)S);
}

// the UPDATE_OPS of one source's batch norms (Training.py:74-75): moving -= (1 - decay) (moving - batch value)
#define WUN_SPEC_BN_LAYERS (2 * WUN_SPEC_MAX_LAYERS - 1)
struct MovingArgs {
    long long pmean[WUN_SPEC_BN_LAYERS], pvar[WUN_SPEC_BN_LAYERS];       // floats into params
    long long wmean[WUN_SPEC_BN_LAYERS], wvar[WUN_SPEC_BN_LAYERS];       // floats into the workspace
    long long n[WUN_SPEC_BN_LAYERS];
    int C[WUN_SPEC_BN_LAYERS];
};
// grid: x = 256 channels, y = layer
__global__ __launch_bounds__(WUN_STFT_BLOCK) void moving_average_kernel(MovingArgs a, float* __restrict__ params,
                                                                       const float* __restrict__ ws, float om) {
    const int j = (int)blockIdx.y, c = (int)blockIdx.x * WUN_STFT_BLOCK + threadIdx.x;
    if (c >= a.C[j]) return;
    const float mm = params[a.pmean[j] + c], mv = params[a.pvar[j] + c];
    params[a.pmean[j] + c] = mm - om * (mm - ws[a.wmean[j] + c]);
    params[a.pvar[j] + c] = mv - om * (mv - bn_unbiased(ws[a.wvar[j] + c], a.n[j]));
}

}  // namespace wun

namespace {

int pow2_tile(int C) {                                       // lanes per pixel row of chan_sums_kernel
    int t = 1;
    while (t < C && t < 64) t <<= 1;
    return t;
}

long long sum_blocks(long long n) { return (n + WUN_SUM_ROWS - 1) / WUN_SUM_ROWS; }
long long wg_chunks(long long nred) { return (nred + WUN_WG_CHUNK - 1) / WUN_WG_CHUNK; }

double* align8(float* p) { return (double*)(((uintptr_t)p + 7) & ~(uintptr_t)7); }

// per-channel sums of an [n][C] tensor into part (2 blocks C doubles), then chan_finish
void launch_chan_sums(int mode, ChanArgs a, hipStream_t s) {
    a.CT = pow2_tile(a.C);
    const dim3 grid((unsigned)sum_blocks(a.n), (unsigned)((a.C + a.CT - 1) / a.CT));
    if (mode == CH_SUM) hipLaunchKernelGGL(chan_sums_kernel<CH_SUM>, grid, dim3(WUN_STFT_BLOCK), 0, s, a);
    else if (mode == CH_SQDEV) hipLaunchKernelGGL(chan_sums_kernel<CH_SQDEV>, grid, dim3(WUN_STFT_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(chan_sums_kernel<CH_BNBWD>, grid, dim3(WUN_STFT_BLOCK), 0, s, a);
}

void launch_chan_finish(const double* part, long long n, int C, double scale, float* o0, float* o1, float* o2, hipStream_t s) {
    hipLaunchKernelGGL(chan_finish_kernel, dim3((unsigned)C), dim3(WUN_STFT_BLOCK), 0, s, part, sum_blocks(n), C, scale, o0, o1, o2);
}

// out[c] = sum over the n pixels of x[.][c]
void channel_sum(const float* x, long long n, int C, double* part, float* out, hipStream_t s) {
    ChanArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.part = part; a.n = n; a.C = C;
    launch_chan_sums(CH_SUM, a, s);
    launch_chan_finish(part, n, C, 1.0, nullptr, nullptr, out, s);
}

// mean and biased variance of z [n][C]
void bn_stats(const float* z, long long n, int C, double* part, float* mean, float* var, hipStream_t s) {
    ChanArgs a;
    memset(&a, 0, sizeof(a));
    a.x = z; a.part = part; a.n = n; a.C = C;
    launch_chan_sums(CH_SUM, a, s);
    launch_chan_finish(part, n, C, 1.0 / (double)n, mean, nullptr, nullptr, s);
    a.mean = mean;
    launch_chan_sums(CH_SQDEV, a, s);
    launch_chan_finish(part, n, C, 1.0 / (double)n, var, nullptr, nullptr, s);
}

// dw [25 Cb][Cs] from its operands; part: wg_chunks(nred) 25 Cb Cs floats
void launch_wgrad(WgArgs a, float* dw, hipStream_t s) {
    const int N = a.c0 + a.c1;
    const long long MN = 25LL * a.Cb * N, chunks = wg_chunks(a.nred);
    if (a.Cb == 1 || N == 1) {
        hipLaunchKernelGGL(wgrad2d_valu_kernel, dim3((unsigned)((MN + WUN_STFT_BLOCK - 1) / WUN_STFT_BLOCK), (unsigned)chunks),
                           dim3(WUN_STFT_BLOCK), 0, s, a);
    } else {
        const dim3 grid((unsigned)((25 * a.Cb + WUN_STFT_BM - 1) / WUN_STFT_BM), (unsigned)((N + WUN_STFT_BN - 1) / WUN_STFT_BN),
                        (unsigned)chunks);
        hipLaunchKernelGGL(wgrad2d_mfma_kernel, grid, dim3(WUN_STFT_BLOCK), 0, s, a);
    }
    hipLaunchKernelGGL(wgrad2d_reduce_kernel, dim3(capped_grid(MN)), dim3(WUN_STFT_BLOCK), 0, s, a.part, dw, MN, (int)chunks);
}

// sizes of a weight-gradient operator: the small map B Hs Ws, channels on both sides
int check_wgrad(const char* who, int B, int Hs, int Ws, int cb, int cs) {
    if (B < 1 || Hs < 1 || Ws < 1 || cb < 1 || cs < 1) return fail(WUN_ERR_INVALID, std::string(who) + ": a size below 1");
    if (cb > (1 << 16) || cs > (1 << 17)) return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 65536 channels");
    if ((long long)B * Hs * Ws > ((long long)1 << 26)) return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 2^28 pixels in the big map");
    if (wg_chunks((long long)B * Hs * Ws) > 65535) return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 65535 reduction chunks");
    if (25LL * cb * cs > ((long long)1 << 31) / 4) return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 2^29 weights");
    return WUN_OK;
}

// floats of a weight-gradient operator's scratch: the chunks' partial tiles, then the float64 partials of db
long long wgrad_scratch(long long nred, long long ndz, int cb, int cs, int cdz) {
    return wg_chunks(nred) * 25 * cb * cs + 4 * sum_blocks(ndz) * cdz + 2;
}

// ---- the model ----
struct Geo { int H, W, C; long long n; };                    // an output map: n = B H W pixels

struct TrainLayout {
    int L, S, K, W0, nif;
    long long B, F;
    int64_t re, im, mag, a0, R, stat, gA, gB, dzb, part, f64, total;
    int64_t mask[WUN_SPEC_MAX_SOURCES];
    int64_t z[WUN_SPEC_MAX_SOURCES][WUN_SPEC_BN_LAYERS], act[WUN_SPEC_MAX_SOURCES][WUN_SPEC_BN_LAYERS];
    int64_t mean[WUN_SPEC_MAX_SOURCES][WUN_SPEC_BN_LAYERS], var[WUN_SPEC_MAX_SOURCES][WUN_SPEC_BN_LAYERS];
    int64_t dmask[WUN_SPEC_MAX_SOURCES][WUN_SPEC_DROP_LEVELS], cat[WUN_SPEC_MAX_SOURCES][WUN_SPEC_DROP_LEVELS];
    int64_t gskip[WUN_SPEC_MAX_LAYERS];
    long long f64_sums;                                      // doubles from the aligned float64 base: the loss partials come first

    // batch-norm layer j: 0 .. L-1 the down path, L .. 2L-2 the up path
    Geo bn(int j) const {
        Geo g;
        if (j < L) { g.H = (int)(F >> (j + 1)); g.W = W0 >> (j + 1); g.C = nif << j; }
        else { const int i = j - L; g.H = (int)(F >> (L - 1 - i)); g.W = W0 >> (L - 1 - i); g.C = nif << (L - i - 2); }
        g.n = B * g.H * g.W;
        return g;
    }
    // transposed layer i (0 .. L-1, the last is the mask layer): its INPUT map, the two channel ranges (c1 = 0: no skip)
    void up_in(int i, int* H, int* W, int* c0, int* c1, int* cout) const {
        *H = (int)(F >> (L - i)); *W = W0 >> (L - i);
        if (i == 0) { *c0 = nif << (L - 1); *c1 = 0; }
        else { *c0 = nif << (L - 1 - i); *c1 = nif << (L - 1 - i); }
        *cout = i < L - 1 ? nif << (L - i - 2) : 1;
    }
};

// does the input of transposed layer i pass through dropout?  (the concatenation of up level i - 1 < 3)
bool dropped(const wun_spec_train_config& t, int i) { return i > 0 && i - 1 < WUN_SPEC_DROP_LEVELS && t.dropout_rate > 0.f; }

int64_t train_layout(const wun_spec_config& c, int64_t B, int64_t F, TrainLayout* out) {
    TrainLayout l;
    memset(&l, 0, sizeof(l));
    l.L = c.num_layers; l.S = c.num_sources; l.K = c.n_fft / 2 + 1; l.W0 = l.K - 1; l.nif = c.num_initial_filters;
    l.B = B; l.F = F;
    const int L = l.L, S = l.S;
    int64_t off = 0;
    auto take = [&](int64_t n) { const int64_t o = off; off += (n + 3) & ~(int64_t)3; return o; };
    const int64_t E = B * F * l.K;
    l.re = take(E); l.im = take(E); l.mag = take(E); l.a0 = take(B * F * l.W0); l.R = take((int64_t)S * E);
    int64_t maxact = B * F * l.W0, maxcat = 0, maxpart = 0, maxsum = sum_blocks(B * F * l.W0), maxc = 1;
    for (int j = 0; j < 2 * L - 1; ++j) {
        const Geo g = l.bn(j);
        maxact = std::max<int64_t>(maxact, g.n * g.C);
        maxsum = std::max<int64_t>(maxsum, sum_blocks(g.n) * g.C);
        maxc = std::max<int64_t>(maxc, g.C);
    }
    for (int i = 0; i < L; ++i) {                            // weight-gradient partials and data-gradient outputs
        const Geo g = l.bn(i);
        const int cin = i ? l.nif << (i - 1) : 1;
        maxpart = std::max<int64_t>(maxpart, wg_chunks(g.n) * 25 * cin * g.C);
        int H, W, c0, c1, cout;
        l.up_in(i, &H, &W, &c0, &c1, &cout);
        maxpart = std::max<int64_t>(maxpart, wg_chunks(B * H * W) * 25 * cout * (c0 + c1));
        maxcat = std::max<int64_t>(maxcat, B * H * W * (c0 + c1));
    }
    for (int s = 0; s < S; ++s) {
        l.mask[s] = take(B * F * l.W0);
        for (int j = 0; j < 2 * L - 1; ++j) {
            const Geo g = l.bn(j);
            l.z[s][j] = take(g.n * g.C); l.act[s][j] = take(g.n * g.C); l.mean[s][j] = take(g.C); l.var[s][j] = take(g.C);
        }
        for (int i = 1; i < L && i - 1 < WUN_SPEC_DROP_LEVELS; ++i) {
            int H, W, c0, c1, cout;
            l.up_in(i, &H, &W, &c0, &c1, &cout);
            l.dmask[s][i - 1] = take(B * H * W * (c0 + c1)); l.cat[s][i - 1] = take(B * H * W * (c0 + c1));
        }
    }
    for (int i = 0; i < L - 1; ++i) { const Geo g = l.bn(i); l.gskip[i] = take(g.n * g.C); }
    l.stat = take(2 * maxc);
    l.gA = take(maxact); l.gB = take(maxcat); l.dzb = take(maxact); l.part = take(maxpart);
    l.f64_sums = (long long)S * sum_blocks(E);
    l.f64 = take(2 * (l.f64_sums + 2 * maxsum) + 2);
    l.total = off;
    if (out) *out = l;
    return off;
}

// (cfg, B, T) as the inference entries check them, plus the grid limit of the split reduction: -> F
int64_t check_train_shape(const char* who, const wun_spec_config* cfg, int32_t B, int64_t T) {
    const int64_t F = check_spec_shape(who, cfg, B, T);
    if (F < 0) return F;
    if (wg_chunks((long long)B * (F / 2) * (cfg->n_fft / 4)) > 65535)
        return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 65535 reduction chunks in the largest weight gradient");
    return F;
}

int check_train_config(const char* who, const wun_spec_train_config* t) {
    if (!t) return fail(WUN_ERR_INVALID, std::string(who) + ": null training config");
    if (!(t->bn_decay >= 0.f && t->bn_decay <= 1.f)) return fail(WUN_ERR_INVALID, std::string(who) + ": bn_decay outside [0, 1]");
    if (!(t->dropout_rate >= 0.f && t->dropout_rate < 1.f)) return fail(WUN_ERR_INVALID, std::string(who) + ": dropout_rate outside [0, 1)");
    return WUN_OK;
}

// offsets (floats into params) of one source's variables, in the table's order
struct SrcVars {
    int64_t dw[WUN_SPEC_MAX_LAYERS], db[WUN_SPEC_MAX_LAYERS], dbeta[WUN_SPEC_MAX_LAYERS], dmean[WUN_SPEC_MAX_LAYERS], dvar[WUN_SPEC_MAX_LAYERS];
    int64_t uw[WUN_SPEC_MAX_LAYERS], ub[WUN_SPEC_MAX_LAYERS], ubeta[WUN_SPEC_MAX_LAYERS], umean[WUN_SPEC_MAX_LAYERS], uvar[WUN_SPEC_MAX_LAYERS];
};

SrcVars source_vars(const std::vector<SpecTensor>& tab, int L, int src) {
    SrcVars v;
    memset(&v, 0, sizeof(v));
    size_t ti = (size_t)src * (size_t)(5 * L + 5 * (L - 1) + 2);
    for (int i = 0; i < L; ++i) {
        v.dw[i] = tab[ti++].offset; v.db[i] = tab[ti++].offset; v.dbeta[i] = tab[ti++].offset;
        v.dmean[i] = tab[ti++].offset; v.dvar[i] = tab[ti++].offset;
    }
    for (int i = 0; i < L - 1; ++i) {
        v.uw[i] = tab[ti++].offset; v.ub[i] = tab[ti++].offset; v.ubeta[i] = tab[ti++].offset;
        v.umean[i] = tab[ti++].offset; v.uvar[i] = tab[ti++].offset;
    }
    v.uw[L - 1] = tab[ti++].offset; v.ub[L - 1] = tab[ti++].offset;
    return v;
}

// Everything of one source's backward pass behind the head: dz of the mask layer is in dzb; the retained tensors
// are read, gA / gB / dzb / gskip / part / stat / sums are scratch, every gradient of the source's kernels, biases and betas is written.
void network_backward(const TrainLayout& l, const wun_spec_train_config* tcfg, const float* params, float* grads, float* ws,
                      double* sums, int src, const SrcVars& v, hipStream_t s) {
    const int L = l.L, nif = l.nif;
    const long long B = l.B;
    float* gA = ws + l.gA; float* gB = ws + l.gB; float* dzb = ws + l.dzb;
    float* mg = ws + l.stat;
    // dz of batch-norm layer j from the gradient(s) behind its activation; dbeta on the way
    auto bn_backward = [&](int j, const float* g1, const float* g2, const float* beta, float* dbeta, int act) {
        const Geo g = l.bn(j);
        ChanArgs a;
        memset(&a, 0, sizeof(a));
        a.x = g1; a.g2 = g2; a.z = ws + l.z[src][j]; a.mean = ws + l.mean[src][j]; a.var = ws + l.var[src][j]; a.beta = beta;
        a.part = sums; a.n = g.n; a.C = g.C; a.act = act;
        launch_chan_sums(CH_BNBWD, a, s);
        launch_chan_finish(sums, g.n, g.C, 1.0 / (double)g.n, mg, mg + g.C, dbeta, s);
        hipLaunchKernelGGL(bn_bwd_kernel, dim3(capped_grid(g.n * g.C)), dim3(WUN_STFT_BLOCK), 0, s, g1, g2, a.z, a.mean, a.var, beta,
                           mg, mg + g.C, dzb, g.n * g.C, g.C, act);
    };
    for (int i = L - 1; i >= 0; --i) {                   // the transposed layers, the mask layer first; dz is in dzb
        int Hi, Wi, c0, c1, cout;
        l.up_in(i, &Hi, &Wi, &c0, &c1, &cout);
        const bool drop = dropped(*tcfg, i);
        const float* x0 = i ? ws + l.act[src][L - 1 - i] : ws + l.act[src][L - 1];
        const float* x1 = i ? ws + l.act[src][L + i - 1] : nullptr;
        const long long nin = (long long)B * Hi * Wi, nout = 4 * nin;
        WgArgs wa;
        wa.big = dzb; wa.part = ws + l.part; wa.nred = nin; wa.Hs = Hi; wa.Ws = Wi; wa.Cb = cout;
        if (drop) { wa.s0 = ws + l.cat[src][i - 1]; wa.s1 = nullptr; wa.c0 = c0 + c1; wa.c1 = 0; }
        else { wa.s0 = x0; wa.s1 = x1; wa.c0 = c0; wa.c1 = c1; }
        launch_wgrad(wa, grads + v.uw[i], s);
        channel_sum(dzb, nout, cout, sums, grads + v.ub[i], s);
        // the data gradient: conv2d_s2(dz, W) with W [5][5][cout][cin] read as [5][5][cin' = cout][cout' = cin]
        C2dArgs a;
        a.x0 = dzb; a.x1 = nullptr; a.w = params + v.uw[i]; a.y = i ? gB : gA;
        a.epi.bias = nullptr; a.epi.beta = nullptr; a.epi.mean = nullptr; a.epi.var = nullptr; a.epi.act = C2D_ACT_NONE;
        a.H = 2 * Hi; a.W = 2 * Wi; a.c0 = cout; a.c1 = 0; a.Cout = c0 + c1;
        a.M = nin;
        launch_conv(a, s);
        if (i) {
            const long long Ec = nin * (c0 + c1);
            hipLaunchKernelGGL(concat_split_kernel, dim3(capped_grid(Ec)), dim3(WUN_STFT_BLOCK), 0, s, gB,
                               drop ? ws + l.dmask[src][i - 1] : nullptr, ws + l.gskip[L - 1 - i], gA, Ec, c0, c1);
            bn_backward(L + i - 1, gA, nullptr, params + v.ubeta[i - 1], grads + v.ubeta[i - 1], C2D_ACT_RELU);
        }
    }
    for (int i = L - 1; i >= 0; --i) {                   // the down path; the gradient from below is in gA
        const Geo g = l.bn(i);
        const int cin = i ? nif << (i - 1) : 1;
        bn_backward(i, gA, i < L - 1 ? ws + l.gskip[i] : nullptr, params + v.dbeta[i], grads + v.dbeta[i], C2D_ACT_LRELU);
        WgArgs wa;
        wa.big = i ? ws + l.act[src][i - 1] : ws + l.a0; wa.part = ws + l.part; wa.nred = g.n; wa.Hs = g.H; wa.Ws = g.W; wa.Cb = cin;
        wa.s0 = dzb; wa.s1 = nullptr; wa.c0 = g.C; wa.c1 = 0;
        launch_wgrad(wa, grads + v.dw[i], s);
        channel_sum(dzb, g.n, g.C, sums, grads + v.db[i], s);
        if (i) {                                         // conv2d_transpose_s2(dz, W): W [5][5][cin][cout] read as [5][5][cout' = cin][cin' = cout]
            C2dArgs a;
            a.x0 = dzb; a.x1 = nullptr; a.w = params + v.dw[i]; a.y = gA;
            a.epi.bias = nullptr; a.epi.beta = nullptr; a.epi.mean = nullptr; a.epi.var = nullptr; a.epi.act = C2D_ACT_NONE;
            a.H = g.H; a.W = g.W; a.c0 = g.C; a.c1 = 0; a.Cout = cin;
            a.M = g.n;
            launch_transpose(a, s);
        }
    }
}

// the UPDATE_OPS of source src from the batch statistics in the workspace
void launch_moving_averages(const TrainLayout& l, const wun_spec_train_config* tcfg, float* params, const float* workspace, int src,
                            const SrcVars& sv, hipStream_t s) {
    const int L = l.L;
    MovingArgs a;
    memset(&a, 0, sizeof(a));
    int cmax = 1;
    for (int j = 0; j < 2 * L - 1; ++j) {
        const Geo g = l.bn(j);
        a.pmean[j] = j < L ? sv.dmean[j] : sv.umean[j - L]; a.pvar[j] = j < L ? sv.dvar[j] : sv.uvar[j - L];
        a.wmean[j] = l.mean[src][j]; a.wvar[j] = l.var[src][j]; a.n[j] = g.n; a.C[j] = g.C;
        cmax = std::max(cmax, g.C);
    }
    hipLaunchKernelGGL(moving_average_kernel, dim3((unsigned)((cmax + WUN_STFT_BLOCK - 1) / WUN_STFT_BLOCK), (unsigned)(2 * L - 1)),
                       dim3(WUN_STFT_BLOCK), 0, s, a, params, workspace, 1.0f - tcfg->bn_decay);
}

// floats of the head's scratch: D [hop] (padded to 4 floats), then u [B T]
long long head_scratch(long long B, long long T, int hop) { return (((long long)hop + 3) & ~3LL) + B * T; }

// dz of one source's mask layer from the upstream gradient(s): D is in scratch (launch_steady_den) when dau is given
int launch_head(const float* re, const float* im, const float* mag, const float* mask, const float* dmg, const float* dau,
                long long B, long long T, long long F, int n_fft, int hop, const float* table_dev, float* dz, float* scratch,
                hipStream_t s) {
    const int K = n_fft / 2 + 1;
    if (!dau) {
        hipLaunchKernelGGL(spec_head_mags_kernel, dim3(capped_grid(B * F * K)), dim3(WUN_STFT_BLOCK), 0, s, dmg, mag, mask, dz, B * F * K, K);
        return WUN_OK;
    }
    float* u = scratch + (((long long)hop + 3) & ~3LL);
    launch_steady_divide(dau, scratch, u, B * T, T, hop, s);
    SpecHeadArgs h;
    memset(&h, 0, sizeof(h));
    h.a.x[0] = u; h.a.M[0] = B * F; h.a.table = table_dev;
    h.a.T = T; h.a.nb = F; h.a.f0 = 0; h.a.fstride = F; h.a.foff = 0;
    h.a.C = 1; h.a.n_fft = n_fft; h.a.hop = hop; h.a.lead = 0; h.a.K = K;
    h.xre = re; h.xim = im; h.mag = mag; h.mask = mask; h.dmags = dmg; h.dz = dz;
    h.c_edge = 1.0f / (float)n_fft; h.c_mid = 2.0f / (float)n_fft;
    return fft_launch_spec_head(h, s);
}

}  // namespace

// ---- the C ABI ----
extern "C" int64_t wun_spec_train_abi_size(void) { return (int64_t)sizeof(wun_spec_train_config); }

extern "C" int64_t wun_spec_train_workspace_floats(const wun_spec_config* cfg, int32_t B, int64_t T) {
    const int64_t F = check_train_shape("wun_spec_train_workspace_floats", cfg, B, T);
    if (F < 0) return F;
    return train_layout(*cfg, B, F, nullptr);
}

extern "C" int wun_spec_train_tensor(const wun_spec_config* cfg, int32_t B, int64_t T, int32_t kind, int32_t source, int32_t layer,
                                     int64_t* offset, int64_t* count) {
    const char* who = "wun_spec_train_tensor";
    const int64_t F = check_train_shape(who, cfg, B, T);
    if (F < 0) return (int)F;
    if (!offset || !count) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    TrainLayout l;
    train_layout(*cfg, B, F, &l);
    const int L = l.L;
    if (source < 0 || source >= l.S) return fail(WUN_ERR_INVALID, std::string(who) + ": source outside the config");
    if (kind == WUN_SPEC_TT_DROPOUT) {
        if (layer < 0 || layer >= L - 1) return fail(WUN_ERR_INVALID, std::string(who) + ": no such up level");
        if (layer >= WUN_SPEC_DROP_LEVELS) { *offset = 0; *count = 0; return WUN_OK; }       // levels i >= 3 have no dropout
        int H, W, c0, c1, cout;
        l.up_in(layer + 1, &H, &W, &c0, &c1, &cout);
        *offset = l.dmask[source][layer]; *count = (int64_t)B * H * W * (c0 + c1);
        return WUN_OK;
    }
    if (kind == WUN_SPEC_TT_ACT && layer == 2 * L - 1) {     // the sigmoid mask [B][F][K - 1]
        *offset = l.mask[source]; *count = (int64_t)B * F * l.W0;
        return WUN_OK;
    }
    if (layer < 0 || layer >= 2 * L - 1) return fail(WUN_ERR_INVALID, std::string(who) + ": layer outside 0 .. 2 L - 2");
    const Geo g = l.bn(layer);
    switch (kind) {
    case WUN_SPEC_TT_Z: *offset = l.z[source][layer]; *count = g.n * g.C; break;
    case WUN_SPEC_TT_MEAN: *offset = l.mean[source][layer]; *count = g.C; break;
    case WUN_SPEC_TT_VAR: *offset = l.var[source][layer]; *count = g.C; break;
    case WUN_SPEC_TT_ACT: *offset = l.act[source][layer]; *count = g.n * g.C; break;
    default: return fail(WUN_ERR_INVALID, std::string(who) + ": unknown kind");
    }
    return WUN_OK;
}

extern "C" int wun_spec_train_forward(const wun_spec_config* cfg, const wun_spec_train_config* tcfg, const float* params,
                                      const float* mix, int32_t B, int64_t T, const float* table_dev, int64_t step, float* mags,
                                      float* workspace, void* stream) {
    const char* who = "wun_spec_train_forward";
    if (!cfg || !tcfg || !params || !mix || !table_dev || !mags || !workspace) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    int rc;
    if ((rc = check_train_config(who, tcfg))) return rc;
    const int64_t F = check_train_shape(who, cfg, B, T);
    if (F < 0) return (int)F;
    if (step < 0) return fail(WUN_ERR_INVALID, std::string(who) + ": step below 0");
    TrainLayout l;
    const int64_t total = train_layout(*cfg, B, F, &l);
    const int L = l.L, S = l.S, K = l.K, W0 = l.W0, nif = l.nif;
    const int64_t np = wun_spec_param_floats(cfg);
    if (overlap(workspace, total, mix, (int64_t)B * T) || overlap(workspace, total, params, np) ||
        overlap(workspace, total, mags, (int64_t)S * B * F * K))
        return fail(WUN_ERR_INVALID, std::string(who) + ": the workspace overlaps another buffer");

    hipStream_t s = (hipStream_t)stream;
    float* ws = workspace;
    double* sums = align8(ws + l.f64) + l.f64_sums;
    const std::vector<SpecTensor> tab = spec_tensors(*cfg);
    if ((rc = wun_stft_complex_fft(mix, 1, B, T, 1, cfg->n_fft, cfg->hop, 0, F, table_dev, ws + l.re, ws + l.im, stream))) return rc;
    const long long E = (long long)B * F * K;
    launch_spec_prepare(ws + l.re, ws + l.im, ws + l.mag, ws + l.a0, E, K, s);

    for (int src = 0; src < S; ++src) {
        const SrcVars v = source_vars(tab, L, src);
        const float* cur = ws + l.a0;
        int H = (int)F, W = W0, C = 1;
        // z = conv + bias, the batch statistics, the activation
        auto norm = [&](int j, const float* beta, int act) {
            const Geo g = l.bn(j);
            bn_stats(ws + l.z[src][j], g.n, g.C, sums, ws + l.mean[src][j], ws + l.var[src][j], s);
            hipLaunchKernelGGL(bn_apply_kernel, dim3(capped_grid(g.n * g.C)), dim3(WUN_STFT_BLOCK), 0, s, ws + l.z[src][j],
                               ws + l.mean[src][j], ws + l.var[src][j], beta, ws + l.act[src][j], g.n * g.C, g.C, act);
        };
        for (int i = 0; i < L; ++i) {
            C2dArgs a;
            a.x0 = cur; a.x1 = nullptr; a.w = params + v.dw[i]; a.y = ws + l.z[src][i];
            a.epi.bias = params + v.db[i]; a.epi.beta = nullptr; a.epi.mean = nullptr; a.epi.var = nullptr; a.epi.act = C2D_ACT_NONE;
            a.H = H; a.W = W; a.c0 = C; a.c1 = 0; a.Cout = nif << i;
            a.M = (long long)B * (H / 2) * (W / 2);
            launch_conv(a, s);
            norm(i, params + v.dbeta[i], C2D_ACT_LRELU);
            cur = ws + l.act[src][i]; H /= 2; W /= 2; C = a.Cout;
        }
        for (int i = 0; i < L; ++i) {                        // the transposed layers; i = L - 1: the mask
            int Hi, Wi, c0, c1, cout;
            l.up_in(i, &Hi, &Wi, &c0, &c1, &cout);
            const float* x0 = i ? ws + l.act[src][L - 1 - i] : cur;      // the skip first
            const float* x1 = i ? cur : nullptr;
            C2dArgs a;
            if (dropped(*tcfg, i)) {
                const long long Ec = (long long)B * Hi * Wi * (c0 + c1);
                hipLaunchKernelGGL(dropout_concat_kernel, dim3(capped_grid(Ec)), dim3(WUN_STFT_BLOCK), 0, s, x0, x1,
                                   ws + l.dmask[src][i - 1], ws + l.cat[src][i - 1], Ec, c0, c1,
                                   drop_key(tcfg->dropout_seed, step, src, i - 1), tcfg->dropout_rate,
                                   1.0f / (1.0f - tcfg->dropout_rate));
                a.x0 = ws + l.cat[src][i - 1]; a.x1 = nullptr; a.c0 = c0 + c1; a.c1 = 0;
            } else {
                a.x0 = x0; a.x1 = x1; a.c0 = c0; a.c1 = c1;
            }
            a.w = params + v.uw[i];
            a.epi.bias = params + v.ub[i]; a.epi.beta = nullptr; a.epi.mean = nullptr; a.epi.var = nullptr;
            a.H = Hi; a.W = Wi; a.Cout = cout;
            a.M = (long long)B * Hi * Wi;
            if (i < L - 1) {
                a.y = ws + l.z[src][L + i]; a.epi.act = C2D_ACT_NONE;
                launch_transpose(a, s);
                norm(L + i, params + v.ubeta[i], C2D_ACT_RELU);
                cur = ws + l.act[src][L + i];
            } else {
                a.y = ws + l.mask[src]; a.epi.act = C2D_ACT_SIGMOID;
                launch_transpose(a, s);
            }
        }
        launch_spec_mask(ws + l.mask[src], ws + l.mag, ws + l.re, ws + l.im, mags + (long long)src * E, nullptr, nullptr, E, K, s);
    }
    return launch_status(who);
}

extern "C" int wun_spec_loss_backward(const wun_spec_config* cfg, const wun_spec_train_config* tcfg, const float* params,
                                      const float* targets, int32_t B, int64_t T, const float* table_dev, float* grads,
                                      float* losses, float* workspace, void* stream) {
    const char* who = "wun_spec_loss_backward";
    if (!cfg || !tcfg || !params || !targets || !table_dev || !grads || !losses || !workspace)
        return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    int rc;
    if ((rc = check_train_config(who, tcfg))) return rc;
    const int64_t F = check_train_shape(who, cfg, B, T);
    if (F < 0) return (int)F;
    TrainLayout l;
    const int64_t total = train_layout(*cfg, B, F, &l);
    const int L = l.L, S = l.S, K = l.K;
    const int64_t np = wun_spec_param_floats(cfg);
    if (overlap(workspace, total, targets, (int64_t)S * B * T) || overlap(workspace, total, params, np) ||
        overlap(workspace, total, grads, np) || overlap(workspace, total, losses, 1 + S) || overlap(grads, np, params, np) ||
        overlap(grads, np, losses, 1 + S))
        return fail(WUN_ERR_INVALID, std::string(who) + ": the workspace or the gradients overlap another buffer");

    hipStream_t s = (hipStream_t)stream;
    float* ws = workspace;
    double* f64 = align8(ws + l.f64);
    double* sums = f64 + l.f64_sums;
    const std::vector<SpecTensor> tab = spec_tensors(*cfg);
    const long long E = (long long)B * F * K, lblocks = sum_blocks(E);
    // R_s = |STFT(target_s)| in the model's framing, the same transform as the forward's
    if ((rc = wun_stft_magnitude_fft(targets, S, B, T, 1, cfg->n_fft, cfg->hop, table_dev, ws + l.R, stream))) return rc;
    if (hipMemsetAsync(grads, 0, (size_t)np * sizeof(float), s) != hipSuccess)          // the moving statistics keep 0
        return fail(WUN_ERR_HIP, std::string(who) + ": memset failed");
    const float cm = (float)(1.0 / ((double)S * (double)E));
    float* dzb = ws + l.dzb;

    for (int src = 0; src < S; ++src) {
        const SrcVars v = source_vars(tab, L, src);
        hipLaunchKernelGGL(spec_loss_kernel, dim3((unsigned)lblocks), dim3(WUN_STFT_BLOCK), 0, s, ws + l.R + (long long)src * E,
                           ws + l.mag, ws + l.mask[src], dzb, f64 + (long long)src * lblocks, E, K, cm);
        network_backward(l, tcfg, params, grads, ws, sums, src, v, s);
    }
    hipLaunchKernelGGL(spec_loss_finish_kernel, dim3(1), dim3(WUN_STFT_BLOCK), 0, s, f64, lblocks, S, 1.0 / (double)E, losses);
    return launch_status(who);
}

extern "C" int wun_spec_adam_step(const wun_spec_config* cfg, const wun_spec_train_config* tcfg, float* params, const float* grads,
                                  float* m, float* v, const float* workspace, int32_t B, int64_t T, int64_t step, float lr,
                                  float beta1, float beta2, float eps, float grad_scale, void* stream) {
    const char* who = "wun_spec_adam_step";
    if (!cfg || !tcfg || !params || !grads || !m || !v || !workspace) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    int rc;
    if ((rc = check_train_config(who, tcfg))) return rc;
    const int64_t F = check_train_shape(who, cfg, B, T);
    if (F < 0) return (int)F;
    if (step < 1) return fail(WUN_ERR_INVALID, std::string(who) + ": step is 1-based");
    TrainLayout l;
    const int64_t total = train_layout(*cfg, B, F, &l);
    const int64_t np = wun_spec_param_floats(cfg);
    if (overlap(workspace, total, params, np) || overlap(workspace, total, grads, np) || overlap(workspace, total, m, np) ||
        overlap(workspace, total, v, np) || overlap(params, np, grads, np) || overlap(params, np, m, np) || overlap(params, np, v, np) ||
        overlap(m, np, v, np) || overlap(m, np, grads, np) || overlap(v, np, grads, np))
        return fail(WUN_ERR_INVALID, std::string(who) + ": two buffers overlap");
    hipStream_t s = (hipStream_t)stream;
    // wun_adam_step's update: the optimizer's kernel with no clip prologue, no decay and no EMA
    OptimArgs a;
    memset(&a, 0, sizeof(a));
    a.p = params; a.g = grads; a.m = m; a.v = v;
    a.lr_t = adam_lr_t(step, lr, beta1, beta2);
    a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.gscale = grad_scale;
    a.vec = same_alignment({params, grads, m, v}) ? 1 : 0;
    const std::vector<SpecTensor> tab = spec_tensors(*cfg);
    const int L = l.L;
    for (int src = 0; src < l.S; ++src) {
        const SrcVars sv = source_vars(tab, L, src);
        // kernels, biases and betas: per layer one run of consecutive floats (kernel, bias, beta); the moving statistics
        // between the runs are not touched, nor are their slots
        AdamRanges r;
        memset(&r, 0, sizeof(r));
        auto run = [&](int64_t first, int64_t end) { r.off[r.n] = first; r.cum[r.n + 1] = r.cum[r.n] + (end - first); ++r.n; };
        for (int i = 0; i < L; ++i) run(sv.dw[i], sv.dmean[i]);
        for (int i = 0; i < L - 1; ++i) run(sv.uw[i], sv.umean[i]);
        run(sv.uw[L - 1], sv.ub[L - 1] + 1);
        if (launch_optim_ranges(a, r, s) != hipSuccess)
            return fail(WUN_ERR_HIP, std::string(who) + ": launch failed");
        launch_moving_averages(l, tcfg, params, workspace, src, sv, s);
    }
    return launch_status(who);
}

// ---- the backward pass from any upstream gradient, the audio of a training forward ----
namespace {
// (cfg, tcfg, B, T) of the entries below, and the resolution as wun_istft_tf_fft takes it: -> F
int64_t check_backward_shape(const char* who, const wun_spec_config* cfg, const wun_spec_train_config* tcfg, int32_t B, int64_t T) {
    int rc;
    if ((rc = check_train_config(who, tcfg))) return rc;
    const int64_t F = check_train_shape(who, cfg, B, T);
    if (F < 0) return F;
    const int64_t is = wun_istft_tf_fft_scratch_floats(cfg->num_sources, B, T, 1, cfg->n_fft, cfg->hop, F);
    return is < 0 ? is : F;
}
}  // namespace

extern "C" int64_t wun_spec_train_audio_scratch_floats(const wun_spec_config* cfg, int32_t B, int64_t T) {
    const int64_t F = check_train_shape("wun_spec_train_audio_scratch_floats", cfg, B, T);
    if (F < 0) return F;
    const int64_t is = wun_istft_tf_fft_scratch_floats(cfg->num_sources, B, T, 1, cfg->n_fft, cfg->hop, F);
    if (is < 0) return is;
    const int64_t E = (int64_t)cfg->num_sources * B * F * (cfg->n_fft / 2 + 1);
    return 2 * ((E + 3) & ~(int64_t)3) + is;
}

extern "C" int wun_spec_train_audio(const wun_spec_config* cfg, const wun_spec_train_config* tcfg, int32_t B, int64_t T,
                                    const float* table_dev, float* audio, const float* workspace, float* scratch, void* stream) {
    const char* who = "wun_spec_train_audio";
    if (!cfg || !tcfg || !table_dev || !audio || !workspace || !scratch) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    const int64_t F = check_backward_shape(who, cfg, tcfg, B, T);
    if (F < 0) return (int)F;
    TrainLayout l;
    const int64_t total = train_layout(*cfg, B, F, &l);
    const int64_t ns = wun_spec_train_audio_scratch_floats(cfg, B, T);
    const int S = l.S, K = l.K;
    if (overlap(workspace, total, audio, (int64_t)S * B * T) || overlap(workspace, total, scratch, ns) ||
        overlap(scratch, ns, audio, (int64_t)S * B * T))
        return fail(WUN_ERR_INVALID, std::string(who) + ": the workspace, the scratch and the audio overlap");
    hipStream_t s = (hipStream_t)stream;
    const long long E = (long long)B * F * K, SE = ((long long)S * E + 3) & ~3LL;
    float* yre = scratch; float* yim = scratch + SE;
    for (int src = 0; src < S; ++src)
        launch_spec_mask(workspace + l.mask[src], workspace + l.mag, workspace + l.re, workspace + l.im, nullptr, yre + src * E,
                         yim + src * E, E, K, s);
    int rc;
    if ((rc = wun_istft_tf_fft(yre, yim, S, B, T, 1, cfg->n_fft, cfg->hop, F, table_dev, audio, scratch + 2 * SE, stream))) return rc;
    return launch_status(who);
}

extern "C" int64_t wun_spec_backward_scratch_floats(const wun_spec_config* cfg, int32_t B, int64_t T) {
    const char* who = "wun_spec_backward_scratch_floats";
    const int64_t F = check_train_shape(who, cfg, B, T);
    if (F < 0) return F;
    const int64_t is = wun_istft_tf_fft_scratch_floats(cfg->num_sources, B, T, 1, cfg->n_fft, cfg->hop, F);
    if (is < 0) return is;
    return head_scratch(B, T, cfg->hop);
}

extern "C" int wun_spec_backward(const wun_spec_config* cfg, const wun_spec_train_config* tcfg, const float* params,
                                 const float* d_mags, const float* d_audio, int32_t B, int64_t T, const float* table_dev,
                                 float* grads, float* workspace, float* scratch, void* stream) {
    const char* who = "wun_spec_backward";
    if (!cfg || !tcfg || !params || !table_dev || !grads || !workspace || !scratch)
        return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    if (!d_mags && !d_audio) return fail(WUN_ERR_INVALID, std::string(who) + ": d_mags and d_audio are both null");
    const int64_t F = check_backward_shape(who, cfg, tcfg, B, T);
    if (F < 0) return (int)F;
    TrainLayout l;
    const int64_t total = train_layout(*cfg, B, F, &l);
    const int L = l.L, S = l.S, K = l.K;
    const int64_t np = wun_spec_param_floats(cfg), ns = head_scratch(B, T, cfg->hop);
    const int64_t nm = (int64_t)S * B * F * K, na = (int64_t)S * B * T;
    const void* bufs[5] = {workspace, scratch, grads, params, nullptr};
    const int64_t lens[4] = {total, ns, np, np};
    for (int i = 0; i < 3; ++i) {                            // the workspace, the scratch and the gradients against everything else
        for (int j = i + 1; j < 4; ++j)
            if (overlap(bufs[i], lens[i], bufs[j], lens[j])) return fail(WUN_ERR_INVALID, std::string(who) + ": two buffers overlap");
        if ((d_mags && overlap(bufs[i], lens[i], d_mags, nm)) || (d_audio && overlap(bufs[i], lens[i], d_audio, na)))
            return fail(WUN_ERR_INVALID, std::string(who) + ": an upstream gradient overlaps the workspace, the scratch or the gradients");
    }

    hipStream_t s = (hipStream_t)stream;
    float* ws = workspace;
    double* sums = align8(ws + l.f64) + l.f64_sums;
    const std::vector<SpecTensor> tab = spec_tensors(*cfg);
    const long long E = (long long)B * F * K;
    if (hipMemsetAsync(grads, 0, (size_t)np * sizeof(float), s) != hipSuccess)          // the moving statistics keep 0
        return fail(WUN_ERR_HIP, std::string(who) + ": memset failed");
    if (d_audio) launch_steady_den(scratch, cfg->n_fft, cfg->hop, s);
    int rc;
    for (int src = 0; src < S; ++src) {
        const SrcVars v = source_vars(tab, L, src);
        if ((rc = launch_head(ws + l.re, ws + l.im, ws + l.mag, ws + l.mask[src], d_mags ? d_mags + (long long)src * E : nullptr,
                              d_audio ? d_audio + (long long)src * B * T : nullptr, B, T, F, cfg->n_fft, cfg->hop, table_dev,
                              ws + l.dzb, scratch, s)))
            return rc;
        network_backward(l, tcfg, params, grads, ws, sums, src, v, s);
    }
    return launch_status(who);
}

extern "C" int wun_spec_update_moving_averages(const wun_spec_config* cfg, const wun_spec_train_config* tcfg, float* params,
                                               const float* workspace, int32_t B, int64_t T, void* stream) {
    const char* who = "wun_spec_update_moving_averages";
    if (!cfg || !tcfg || !params || !workspace) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    int rc;
    if ((rc = check_train_config(who, tcfg))) return rc;
    const int64_t F = check_train_shape(who, cfg, B, T);
    if (F < 0) return (int)F;
    TrainLayout l;
    const int64_t total = train_layout(*cfg, B, F, &l);
    if (overlap(workspace, total, params, wun_spec_param_floats(cfg)))
        return fail(WUN_ERR_INVALID, std::string(who) + ": the workspace overlaps the parameters");
    const std::vector<SpecTensor> tab = spec_tensors(*cfg);
    for (int src = 0; src < l.S; ++src)
        launch_moving_averages(l, tcfg, params, workspace, src, source_vars(tab, l.L, src), (hipStream_t)stream);
    return launch_status(who);
}

// ---- single operators ----
extern "C" int64_t wun_op_spec_head_backward_scratch(int32_t B, int64_t T, int32_t n_fft, int32_t hop) {
    const char* who = "wun_op_spec_head_backward_scratch";
    if (B < 1) return fail(WUN_ERR_INVALID, std::string(who) + ": B < 1");
    const int64_t F = wun_fft_frames(T, n_fft, hop);          // the n_fft list, hop in 1..n_fft, T >= n_fft
    if (F < 0) return F;
    if (T != (F - 1) * hop + n_fft) return fail(WUN_ERR_INVALID, std::string(who) + ": T is not (F - 1) hop + n_fft");
    if ((int64_t)B * F > ((int64_t)1 << 28) / (n_fft / 2)) return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 2^28 bins in a batch");
    const int64_t is = wun_istft_tf_fft_scratch_floats(1, B, T, 1, n_fft, hop, F);      // the resolution as wun_istft_tf_fft takes it
    if (is < 0) return is;
    return head_scratch(B, T, hop);
}

extern "C" int wun_op_spec_head_backward(const float* re, const float* im, const float* mag, const float* mask, const float* d_mags,
                                         const float* d_audio, int32_t B, int64_t T, int32_t n_fft, int32_t hop,
                                         const float* table_dev, float* dz, float* scratch, void* stream) {
    const char* who = "wun_op_spec_head_backward";
    if (!re || !im || !mag || !mask || !table_dev || !dz || !scratch) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    if (!d_mags && !d_audio) return fail(WUN_ERR_INVALID, std::string(who) + ": d_mags and d_audio are both null");
    const int64_t ns = wun_op_spec_head_backward_scratch(B, T, n_fft, hop);
    if (ns < 0) return (int)ns;
    const int64_t F = 1 + (T - n_fft) / hop, K = n_fft / 2 + 1, E = (int64_t)B * F * K, Ez = (int64_t)B * F * (K - 1);
    const float* in[6] = {re, im, mag, mask, d_mags, d_audio};
    const int64_t len[6] = {E, E, E, Ez, E, (int64_t)B * T};
    for (int i = 0; i < 6; ++i)
        if (in[i] && (overlap(scratch, ns, in[i], len[i]) || overlap(dz, Ez, in[i], len[i])))
            return fail(WUN_ERR_INVALID, std::string(who) + ": the scratch or dz overlaps an operand");
    if (overlap(scratch, ns, dz, Ez)) return fail(WUN_ERR_INVALID, std::string(who) + ": the scratch overlaps dz");
    hipStream_t s = (hipStream_t)stream;
    if (d_audio) launch_steady_den(scratch, n_fft, hop, s);
    int rc;
    if ((rc = launch_head(re, im, mag, mask, d_mags, d_audio, B, T, F, n_fft, hop, table_dev, dz, scratch, s))) return rc;
    return launch_status(who);
}

extern "C" int64_t wun_op_conv2d_s2_wgrad_scratch(int B, int H, int W, int cin, int cout) {
    const char* who = "wun_op_conv2d_s2_wgrad_scratch";
    if ((H | W) & 1) return fail(WUN_ERR_INVALID, std::string(who) + ": H and W must be even");
    int rc;
    if ((rc = check_wgrad(who, B, H / 2, W / 2, cin, cout))) return rc;
    const long long n = (long long)B * (H / 2) * (W / 2);
    return wgrad_scratch(n, n, cin, cout, cout);
}

extern "C" int wun_op_conv2d_s2_wgrad(const float* x, const float* dz, float* dw, float* db, float* scratch, int B, int H, int W,
                                      int cin, int cout, void* stream) {
    const char* who = "wun_op_conv2d_s2_wgrad";
    if (!x || !dz || !dw || !scratch) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    if ((H | W) & 1) return fail(WUN_ERR_INVALID, std::string(who) + ": H and W must be even");
    int rc;
    if ((rc = check_wgrad(who, B, H / 2, W / 2, cin, cout))) return rc;
    const long long n = (long long)B * (H / 2) * (W / 2), nw = 25LL * cin * cout, ns = wgrad_scratch(n, n, cin, cout, cout);
    if (overlap(scratch, ns, x, 4 * n * cin) || overlap(scratch, ns, dz, n * cout) || overlap(scratch, ns, dw, nw) ||
        (db && overlap(scratch, ns, db, cout)))
        return fail(WUN_ERR_INVALID, std::string(who) + ": the scratch overlaps another buffer");
    hipStream_t s = (hipStream_t)stream;
    WgArgs a;
    a.big = x; a.s0 = dz; a.s1 = nullptr; a.part = scratch; a.nred = n; a.Hs = H / 2; a.Ws = W / 2; a.Cb = cin; a.c0 = cout; a.c1 = 0;
    launch_wgrad(a, dw, s);
    if (db) channel_sum(dz, n, cout, align8(scratch + wg_chunks(n) * nw), db, s);
    return launch_status(who);
}

extern "C" int64_t wun_op_conv2d_transpose_s2_wgrad_scratch(int B, int H, int W, int cin, int cout) {
    const char* who = "wun_op_conv2d_transpose_s2_wgrad_scratch";
    int rc;
    if ((rc = check_wgrad(who, B, H, W, cout, cin))) return rc;
    const long long n = (long long)B * H * W;
    return wgrad_scratch(n, 4 * n, cout, cin, cout);
}

extern "C" int wun_op_conv2d_transpose_s2_wgrad(const float* x0, int c0, const float* x1, int c1, const float* dz, float* dw,
                                                float* db, float* scratch, int B, int H, int W, int cout, void* stream) {
    const char* who = "wun_op_conv2d_transpose_s2_wgrad";
    if (!x0 || !dz || !dw || !scratch) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    if (c0 < 1 || c1 < 0 || (x1 != nullptr) != (c1 > 0))
        return fail(WUN_ERR_INVALID, std::string(who) + ": c0 < 1, c1 < 0, or x1 and c1 disagree");
    if (c0 > (1 << 16) || c1 > (1 << 16)) return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 65536 channels");
    int rc;
    if ((rc = check_wgrad(who, B, H, W, cout, c0 + c1))) return rc;
    const long long n = (long long)B * H * W, nw = 25LL * cout * (c0 + c1), ns = wgrad_scratch(n, 4 * n, cout, c0 + c1, cout);
    if (overlap(scratch, ns, x0, n * c0) || (x1 && overlap(scratch, ns, x1, n * c1)) || overlap(scratch, ns, dz, 4 * n * cout) ||
        overlap(scratch, ns, dw, nw) || (db && overlap(scratch, ns, db, cout)))
        return fail(WUN_ERR_INVALID, std::string(who) + ": the scratch overlaps another buffer");
    hipStream_t s = (hipStream_t)stream;
    WgArgs a;
    a.big = dz; a.s0 = x0; a.s1 = x1; a.part = scratch; a.nred = n; a.Hs = H; a.Ws = W; a.Cb = cout; a.c0 = c0; a.c1 = c1;
    launch_wgrad(a, dw, s);
    if (db) channel_sum(dz, 4 * n, cout, align8(scratch + wg_chunks(n) * nw), db, s);
    return launch_status(who);
}

extern "C" int64_t wun_op_bn2d_stats_scratch(int B, int H, int W, int C) {
    const char* who = "wun_op_bn2d_stats_scratch";
    if (B < 1 || H < 1 || W < 1 || C < 1) return fail(WUN_ERR_INVALID, std::string(who) + ": a size below 1");
    if (C > (1 << 16) || (long long)B * H * W > ((long long)1 << 28)) return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 65536 channels or 2^28 pixels");
    return 4 * sum_blocks((long long)B * H * W) * C + 2;
}

extern "C" int wun_op_bn2d_stats(const float* z, float* mean, float* var, float* scratch, int B, int H, int W, int C, void* stream) {
    const char* who = "wun_op_bn2d_stats";
    if (!z || !mean || !var || !scratch) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    const int64_t ns = wun_op_bn2d_stats_scratch(B, H, W, C);
    if (ns < 0) return (int)ns;
    const long long n = (long long)B * H * W;
    if (overlap(scratch, ns, z, n * C) || overlap(scratch, ns, mean, C) || overlap(scratch, ns, var, C) || overlap(mean, C, var, C))
        return fail(WUN_ERR_INVALID, std::string(who) + ": two buffers overlap");
    bn_stats(z, n, C, align8(scratch), mean, var, (hipStream_t)stream);
    return launch_status(who);
}
