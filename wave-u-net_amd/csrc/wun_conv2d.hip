// gfx950 (MI355X / CDNA4): the spectrogram U-Net baseline in inference mode (include/wun.h: wun_spec_forward, wun_op_conv2d_s2,
// wun_op_conv2d_transpose_s2; Models/UnetSpectrogramSeparator.py:40-108 at training = False).
//
//   conv       Z[b][y][x][co] = sum_{ky,kx,ci} A[b][2y + ky - 1][2x + kx - 1][ci] W[ky][kx][ci][co]: 5 x 5, stride 2, TF's "same"
//              (1 before, 2 after), zeros outside the map.  An implicit GEMM on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32):
//              M = B Ho Wo output pixels, N = Cout, reduction r = (ky 5 + kx) Cin + ci.  The input window is gathered while the A
//              tile is staged in LDS; no im2col matrix goes to HBM.
//   transposed the gradient of that conv with respect to its input: out[ty][tx][co] = sum over 2 jy + ky - 1 == ty, 2 jx + kx - 1
//              == tx, ci of A[jy][jx][ci] W[ky][kx][co][ci].  Destination-driven, one GEMM per output parity class (py, px):
//              even outputs take the taps {1, 3}, odd ones {0, 2, 4}, so the classes reduce over 2 x 2, 2 x 3, 3 x 2 and 3 x 3
//              taps; M = B Hi Wi outputs of a class, every output float written once.  The input is the virtual channel
//              concatenation of x0 [.., c0] and x1 [.., c1] (skip first): the concatenation is never materialised.
//   epilogue   + bias, inference batch norm (z - mean) / sqrt(var + 1e-3) + beta (no gamma), LeakyReLU(0.2) | ReLU | sigmoid
//              (a NaN stays NaN through each of them)
//   thin       the first down layer (Cin = 1: a reduction of 25) and the mask layer (Cout = 1: one GEMM column in 16) are poor
//              MFMA shapes and run on the VALU, one lane per output, the same gather, the same order, fmaf in place of the MFMA
//
// One workgroup of 256 lanes computes 64 rows x 32 columns with wun_stft.h's tile: 2 x 2 waves of 32 x 16, LDS pitches 36 (A,
// read [row = lane & 15][k = lane >> 4]) and 48 (B, read [k][col]), 32 reduction indices per step.  The reduction index runs in
// ascending (ky, kx, ci) order inside one accumulator per output; a tap outside the map enters as a zero operand (fma(0, w, acc)
// = acc).  The MFMA is a k-ordered fmaf chain, so the VALU kernels give the bits the MFMA kernels would, and an excerpt's bits do
// not depend on the batch around it, the grid or pointer alignment beyond 4 bytes.  No atomics.
//
// Built WITHOUT the packed fp32 VALU instructions (csrc/Makefile NO_PK_FP32): inference runs beside plans of either
// compute mode.  Every argument check runs before any GPU work; nothing allocates or synchronises.
#include "wun_conv2d.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace wun;

namespace wun {

// (C2dEpilogue, C2dArgs and the activation codes: wun_conv2d.h)

__device__ __forceinline__ float c2d_finish(const C2dEpilogue& e, float z, int n) {
    if (e.bias) z += e.bias[n];
    if (e.mean) z = (z - e.mean[n]) * (1.0f / sqrtf(e.var[n] + WUN_C2D_EPS)) + e.beta[n];
    if (e.act == C2D_ACT_LRELU) z = z > 0.f ? z : 0.2f * z;
    else if (e.act == C2D_ACT_RELU) z = z > 0.f ? z : (z != z ? z : 0.f);      // NaN stays NaN; -0.0 and below give +0.0
    else if (e.act == C2D_ACT_SIGMOID) z = 1.0f / (1.0f + expf(-z));
    return z;
}

struct C2dRow { long long base; int y, x; };             // a GEMM row: the excerpt's first pixel and the row's place in the map
struct C2dRed { int dy, dx, ci; long long wofs; };       // a reduction index: the tap's offset from the row's place, the channel

// The GEMM tile of workgroup (blockIdx.x = tile of 64 rows, blockIdx.y = tile of 32 columns): row_of(m), red_of(r) decode a row
// and a reduction index, load_a(row, red) gathers one input (0 outside the map), load_b(red, n) one weight, store(m, n, acc) is
// called once for every row m < M and column n < N of the tile.
template <class RowOf, class RedOf, class LoadA, class LoadB, class Store>
__device__ __forceinline__ void c2d_mfma_tile(long long M, int N, int Rd, RowOf row_of, RedOf red_of, LoadA load_a, LoadB load_b,
                                              Store store) {
    __shared__ float As[WUN_STFT_BM * WUN_STFT_PA];
    __shared__ float Bs[WUN_STFT_KC * WUN_STFT_PB];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int sc = tid & 31, sr = tid >> 5;                  // staging: A column / B column, and the first row of this lane
    const long long m0 = (long long)blockIdx.x * WUN_STFT_BM;
    const int n0 = (int)blockIdx.y * WUN_STFT_BN;
    const int wm = (w & 1) * 32, wn = (w >> 1) * 16;

    C2dRow rows[WUN_STFT_BM / 8];
    bool rin[WUN_STFT_BM / 8];
#pragma unroll
    for (int it = 0; it < WUN_STFT_BM / 8; ++it) {
        const long long m = m0 + sr + 8 * it;
        rin[it] = m < M;
        rows[it] = row_of(rin[it] ? m : 0);
    }
    const bool nin = n0 + sc < N;

    f32x4 acc[2];
    acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
    for (int r0 = 0; r0 < Rd; r0 += WUN_STFT_KC) {           // ascending (ky, kx, ci): the one accumulation order
        __syncthreads();                                     // the previous step is read
        {
            const int r = r0 + sc;                           // A: this lane's reduction index, its 8 rows
            const bool rok = r < Rd;
            const C2dRed rd = red_of(rok ? r : 0);
#pragma unroll
            for (int it = 0; it < WUN_STFT_BM / 8; ++it)
                As[(sr + 8 * it) * WUN_STFT_PA + sc] = (rok && rin[it]) ? load_a(rows[it], rd) : 0.f;
        }
#pragma unroll
        for (int it = 0; it < WUN_STFT_KC / 8; ++it) {       // B: this lane's column, 4 reduction indices
            const int kl = sr + 8 * it, r = r0 + kl;
            const bool rok = r < Rd;
            const C2dRed rd = red_of(rok ? r : 0);
            Bs[kl * WUN_STFT_PB + sc] = (rok && nin) ? load_b(rd, r, n0 + sc) : 0.f;
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
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long m = m0 + wm + 16 * i + 4 * lq + r;
            if (m < M) store(m, n, acc[i][r]);
        }
}

// The same GEMM on the VALU, one lane per output (column fastest), grid-stride: the thin layers.
template <class RowOf, class RedOf, class LoadA, class LoadB, class Store>
__device__ __forceinline__ void c2d_valu(long long M, int N, int Rd, RowOf row_of, RedOf red_of, LoadA load_a, LoadB load_b,
                                         Store store) {
    const long long E = M * N;
    for (long long e = (long long)blockIdx.x * WUN_STFT_BLOCK + threadIdx.x; e < E; e += (long long)gridDim.x * WUN_STFT_BLOCK) {
        const long long m = e / N;
        const int n = (int)(e - m * N);
        const C2dRow row = row_of(m);
        float acc = 0.f;
        for (int r = 0; r < Rd; ++r) {                       // ascending (ky, kx, ci)
            const C2dRed rd = red_of(r);
            acc = fmaf(load_a(row, rd), load_b(rd, r, n), acc);
        }
        store(m, n, acc);
    }
}

// conv: rows are output pixels (b, y, x) of the [H/2][W/2] map
template <bool MFMA>
__device__ __forceinline__ void c2d_conv_body(const C2dArgs& p) {
    const int Ho = p.H >> 1, Wo = p.W >> 1, Cin = p.c0, Cout = p.Cout;
    auto row_of = [&](long long m) {
        const long long b = m / ((long long)Ho * Wo), rest = m - b * Ho * Wo;
        C2dRow r;
        r.base = b * p.H * p.W;
        r.y = 2 * (int)(rest / Wo) - 1;
        r.x = 2 * (int)(rest % Wo) - 1;
        return r;
    };
    auto red_of = [&](int r) {
        const int tap = r / Cin, ky = tap / 5;
        C2dRed d;
        d.dy = ky; d.dx = tap - 5 * ky; d.ci = r - tap * Cin; d.wofs = 0;
        return d;
    };
    auto load_a = [&](const C2dRow& r, const C2dRed& d) {
        const int yy = r.y + d.dy, xx = r.x + d.dx;
        if ((unsigned)yy >= (unsigned)p.H || (unsigned)xx >= (unsigned)p.W) return 0.f;
        return p.x0[(r.base + (long long)yy * p.W + xx) * Cin + d.ci];
    };
    auto load_b = [&](const C2dRed&, int r, int n) { return p.w[(long long)r * Cout + n]; };
    auto store = [&](long long m, int n, float v) { p.y[m * Cout + n] = c2d_finish(p.epi, v, n); };
    if (MFMA) c2d_mfma_tile(p.M, Cout, 25 * Cin, row_of, red_of, load_a, load_b, store);
    else c2d_valu(p.M, Cout, 25 * Cin, row_of, red_of, load_a, load_b, store);
}

// transposed: rows are the outputs (b, 2 oy + py, 2 ox + px) of parity class cls = 2 py + px, (oy, ox) on the input map
template <bool MFMA>
__device__ __forceinline__ void c2d_transpose_body(const C2dArgs& p, int cls) {
    const int py = cls >> 1, px = cls & 1, nkx = px ? 3 : 2, nky = py ? 3 : 2;
    const int Cin = p.c0 + p.c1, Cout = p.Cout;
    auto row_of = [&](long long m) {
        const long long b = m / ((long long)p.H * p.W), rest = m - b * p.H * p.W;
        C2dRow r;
        r.base = b * p.H * p.W;
        r.y = (int)(rest / p.W);
        r.x = (int)(rest % p.W);
        return r;
    };
    auto red_of = [&](int r) {                               // tap (iy, ix) of the class: ky = 2 iy + 1 - py, jy = oy + py - iy
        const int tap = r / Cin, iy = tap / nkx, ix = tap - iy * nkx;
        C2dRed d;
        d.dy = py - iy; d.dx = px - ix; d.ci = r - tap * Cin;
        d.wofs = (long long)((2 * iy + 1 - py) * 5 + (2 * ix + 1 - px)) * Cout * Cin + d.ci;
        return d;
    };
    auto load_a = [&](const C2dRow& r, const C2dRed& d) {
        const int jy = r.y + d.dy, jx = r.x + d.dx;
        if ((unsigned)jy >= (unsigned)p.H || (unsigned)jx >= (unsigned)p.W) return 0.f;
        const long long pix = r.base + (long long)jy * p.W + jx;
        return d.ci < p.c0 ? p.x0[pix * p.c0 + d.ci] : p.x1[pix * p.c1 + (d.ci - p.c0)];
    };
    auto load_b = [&](const C2dRed& d, int, int n) { return p.w[d.wofs + (long long)n * Cin]; };
    auto store = [&](long long m, int n, float v) {
        const long long b = m / ((long long)p.H * p.W), rest = m - b * p.H * p.W;
        const long long ty = 2 * (rest / p.W) + py, tx = 2 * (rest % p.W) + px;
        p.y[((b * 2 * p.H + ty) * 2 * p.W + tx) * Cout + n] = c2d_finish(p.epi, v, n);
    };
    if (MFMA) c2d_mfma_tile(p.M, Cout, nky * nkx * Cin, row_of, red_of, load_a, load_b, store);
    else c2d_valu(p.M, Cout, nky * nkx * Cin, row_of, red_of, load_a, load_b, store);
}

// grid: x = tile of 64 output pixels, y = tile of 32 output channels
__global__ __launch_bounds__(WUN_STFT_BLOCK) void conv2d_s2_mfma_kernel(C2dArgs p) { c2d_conv_body<true>(p); }
// grid: x = capped, grid-stride over the outputs
__global__ __launch_bounds__(WUN_STFT_BLOCK) void conv2d_s2_valu_kernel(C2dArgs p) { c2d_conv_body<false>(p); }
// grid: x, y as above over one parity class, z = the class
__global__ __launch_bounds__(WUN_STFT_BLOCK) void conv2d_transpose_s2_mfma_kernel(C2dArgs p) { c2d_transpose_body<true>(p, (int)blockIdx.z); }
// grid: x = capped, grid-stride over the outputs of one class, y = the class
__global__ __launch_bounds__(WUN_STFT_BLOCK) void conv2d_transpose_s2_valu_kernel(C2dArgs p) { c2d_transpose_body<false>(p, (int)blockIdx.y); }

// One lane per bin of X = re + i im [B][F][K]: mag = |X| as the magnitude entries form it, a0 [B][F][K - 1] = log1p(mag) without
// the last bin (UnetSpectrogramSeparator.py:55,59-60).  E = B F K.
__global__ __launch_bounds__(WUN_STFT_BLOCK) void spec_prepare_kernel(const float* __restrict__ re, const float* __restrict__ im,
                                                                    float* __restrict__ mag, float* __restrict__ a0, long long E, int K) {
    for (long long e = (long long)blockIdx.x * WUN_STFT_BLOCK + threadIdx.x; e < E; e += (long long)gridDim.x * WUN_STFT_BLOCK) {
        const long long bf = e / K;
        const int k = (int)(e - bf * K);
        const float a = re[e], b = im[e];
        const float m = sqrtf(fmaf(a, a, b * b));
        mag[e] = m;
        if (k < K - 1) a0[bf * (K - 1) + k] = log1pf(m);
    }
}

// One lane per bin: the mask [B][F][K - 1] of one source, 0.5 at the dropped bin K - 1 (:86-88), times the mixture's magnitude
// (mags, :91) and / or times X (yre, yim: mag exp(i angle X) of :100 is mask X).  Null outputs are not written.
__global__ __launch_bounds__(WUN_STFT_BLOCK) void spec_mask_kernel(const float* __restrict__ mask, const float* __restrict__ mag,
                                                                 const float* __restrict__ re, const float* __restrict__ im,
                                                                 float* __restrict__ mags, float* __restrict__ yre,
                                                                 float* __restrict__ yim, long long E, int K) {
    for (long long e = (long long)blockIdx.x * WUN_STFT_BLOCK + threadIdx.x; e < E; e += (long long)gridDim.x * WUN_STFT_BLOCK) {
        const long long bf = e / K;
        const int k = (int)(e - bf * K);
        const float mk = k < K - 1 ? mask[bf * (K - 1) + k] : 0.5f;
        if (mags) mags[e] = mag[e] * mk;
        if (yre) { yre[e] = mk * re[e]; yim[e] = mk * im[e]; }
    }
}

// the launchers, the variable table and the shape checks are shared with the training unit (wun_conv2d.h)
// the first down layer (Cin == 1) and the mask layer (Cout == 1) run on the VALU
void launch_conv(const C2dArgs& a, hipStream_t s) {
    if (a.c0 == 1) {
        hipLaunchKernelGGL(conv2d_s2_valu_kernel, dim3(capped_grid(a.M * a.Cout)), dim3(WUN_STFT_BLOCK), 0, s, a);
        return;
    }
    const dim3 grid((unsigned)((a.M + WUN_STFT_BM - 1) / WUN_STFT_BM), (unsigned)((a.Cout + WUN_STFT_BN - 1) / WUN_STFT_BN));
    hipLaunchKernelGGL(conv2d_s2_mfma_kernel, grid, dim3(WUN_STFT_BLOCK), 0, s, a);
}

void launch_transpose(const C2dArgs& a, hipStream_t s) {
    if (a.Cout == 1) {
        hipLaunchKernelGGL(conv2d_transpose_s2_valu_kernel, dim3(capped_grid(a.M), 4), dim3(WUN_STFT_BLOCK), 0, s, a);
        return;
    }
    const dim3 grid((unsigned)((a.M + WUN_STFT_BM - 1) / WUN_STFT_BM), (unsigned)((a.Cout + WUN_STFT_BN - 1) / WUN_STFT_BN), 4);
    hipLaunchKernelGGL(conv2d_transpose_s2_mfma_kernel, grid, dim3(WUN_STFT_BLOCK), 0, s, a);
}

void launch_spec_prepare(const float* re, const float* im, float* mag, float* a0, long long E, int K, hipStream_t s) {
    hipLaunchKernelGGL(spec_prepare_kernel, dim3(capped_grid(E)), dim3(WUN_STFT_BLOCK), 0, s, re, im, mag, a0, E, K);
}

void launch_spec_mask(const float* mask, const float* mag, const float* re, const float* im, float* mags, float* yre, float* yim,
                      long long E, int K, hipStream_t s) {
    hipLaunchKernelGGL(spec_mask_kernel, dim3(capped_grid(E)), dim3(WUN_STFT_BLOCK), 0, s, mask, mag, re, im, mags, yre, yim, E, K);
}

}  // namespace wun

namespace {

// sizes of one 2-D layer: B H W pixels of the input map, channels on both sides
int check_c2d(const char* who, int B, int H, int W, int cin, int cout, int act, const float* mean, const float* var, const float* beta) {
    if (B < 1 || H < 1 || W < 1 || cin < 1 || cout < 1) return fail(WUN_ERR_INVALID, std::string(who) + ": a size below 1");
    if (cin > (1 << 16) || cout > (1 << 16)) return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 65536 channels");
    if ((long long)B * H * W > ((long long)1 << 28)) return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 2^28 input pixels");
    if (act < 0 || act > 3) return fail(WUN_ERR_INVALID, std::string(who) + ": act outside 0..3");
    if ((mean != nullptr) != (var != nullptr) || (mean != nullptr) != (beta != nullptr))
        return fail(WUN_ERR_INVALID, std::string(who) + ": batch norm needs mean, variance and beta, or none of them");
    return WUN_OK;
}

}  // namespace

// ---- the model: variables and workspace ----
namespace wun {

int check_spec_config(const char* who, const wun_spec_config* c) {
    if (!c) return fail(WUN_ERR_INVALID, std::string(who) + ": null config");
    if (c->num_layers < 1 || c->num_initial_filters < 1 || c->num_sources < 1)
        return fail(WUN_ERR_INVALID, std::string(who) + ": num_layers, num_initial_filters or num_sources below 1");
    if (c->num_layers > WUN_SPEC_MAX_LAYERS || c->num_sources > WUN_SPEC_MAX_SOURCES ||
        ((long long)c->num_initial_filters << (c->num_layers - 1)) > (1 << 16))
        return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 10 layers, 8 sources or 65536 channels");
    int rc;
    if ((rc = check_res(who, WUN_TR_FFT, c->n_fft, c->hop))) return rc;
    return WUN_OK;
}

static std::string tf_name(const char* stem, int index, const char* leaf) {      // an index 0 has no suffix
    std::string s = std::string("separator/") + stem;
    if (index) s += "_" + std::to_string(index);
    return s + "/" + leaf;
}

// tf.layers / tf.contrib.layers names in graph-construction order (UnetSpectrogramSeparator.py:63-86), packed without padding
std::vector<SpecTensor> spec_tensors(const wun_spec_config& c) {
    std::vector<SpecTensor> v;
    int64_t off = 0;
    auto add = [&](const std::string& name, int ndim, int64_t s0, int64_t s1, int64_t s2, int64_t s3) {
        SpecTensor t;
        t.name = name; t.offset = off; t.ndim = ndim;
        t.shape[0] = s0; t.shape[1] = s1; t.shape[2] = s2; t.shape[3] = s3;
        int64_t n = 1;
        for (int i = 0; i < ndim; ++i) n *= t.shape[i];
        off += n;
        v.push_back(t);
    };
    const int L = c.num_layers;
    const int64_t nif = c.num_initial_filters;
    auto norm = [&](int index, int64_t ch) {
        add(tf_name("BatchNorm", index, "beta"), 1, ch, 0, 0, 0);
        add(tf_name("BatchNorm", index, "moving_mean"), 1, ch, 0, 0, 0);
        add(tf_name("BatchNorm", index, "moving_variance"), 1, ch, 0, 0, 0);
    };
    for (int s = 0; s < c.num_sources; ++s) {
        for (int i = 0; i < L; ++i) {
            const int64_t cin = i ? nif << (i - 1) : 1, cout = nif << i;
            add(tf_name("conv2d", s * L + i, "kernel"), 4, 5, 5, cin, cout);
            add(tf_name("conv2d", s * L + i, "bias"), 1, cout, 0, 0, 0);
            norm(s * (2 * L - 1) + i, cout);
        }
        for (int i = 0; i < L - 1; ++i) {
            const int64_t cout = nif << (L - i - 2), cin = i ? 4 * cout : 2 * cout;      // (i > 0: skip and up, 2 cout each)
            add(tf_name("conv2d_transpose", s * L + i, "kernel"), 4, 5, 5, cout, cin);
            add(tf_name("conv2d_transpose", s * L + i, "bias"), 1, cout, 0, 0, 0);
            norm(s * (2 * L - 1) + L + i, cout);
        }
        add(tf_name("conv2d_transpose", s * L + L - 1, "kernel"), 4, 5, 5, 1, L > 1 ? 2 * nif : nif);
        add(tf_name("conv2d_transpose", s * L + L - 1, "bias"), 1, 1, 0, 0, 0);
    }
    return v;
}

}  // namespace wun

namespace {

// F for T samples, or the refusal of a shape the network cannot halve num_layers times (UnetSpectrogramSeparator.py:69)
int64_t spec_frames(const char* who, const wun_spec_config& c, int64_t T) {
    if (T < c.n_fft || T > ((int64_t)1 << 40)) return fail(WUN_ERR_INVALID, std::string(who) + ": T below n_fft or above 2^40");
    const int64_t F = 1 + (T - c.n_fft) / c.hop, m = (int64_t)1 << c.num_layers;
    if ((F - 1) * c.hop + c.n_fft != T) return fail(WUN_ERR_INVALID, std::string(who) + ": T is not (F - 1) hop + n_fft");
    if (F % m || (c.n_fft / 2) % m)
        return fail(WUN_ERR_INVALID, std::string(who) + ": frames and n_fft / 2 must be multiples of 2^num_layers");
    return F;
}

// floats from the workspace base
struct SpecLayout {
    int64_t re, im, mag, a0, mask, yre, yim, istft, total;
    int64_t down[WUN_SPEC_MAX_LAYERS], up[WUN_SPEC_MAX_LAYERS];
};

int64_t spec_layout(const char* who, const wun_spec_config& c, int64_t B, int64_t T, int64_t F, SpecLayout* lay) {
    const int L = c.num_layers, K = c.n_fft / 2 + 1, W0 = K - 1, S = c.num_sources;
    const int64_t nif = c.num_initial_filters;
    int64_t off = 0;
    auto take = [&](int64_t n) { const int64_t o = off; off += (n + 3) & ~(int64_t)3; return o; };
    SpecLayout l;
    l.re = take(B * F * K); l.im = take(B * F * K); l.mag = take(B * F * K); l.a0 = take(B * F * W0); l.mask = take(B * F * W0);
    for (int i = 0; i < L; ++i) l.down[i] = take(B * (F >> (i + 1)) * (W0 >> (i + 1)) * (nif << i));
    for (int i = 0; i < L - 1; ++i) l.up[i] = take(B * (F >> (L - 1 - i)) * (W0 >> (L - 1 - i)) * (nif << (L - i - 2)));
    l.yre = take(S * B * F * K); l.yim = take(S * B * F * K);
    const int64_t is = wun_istft_tf_fft_scratch_floats(S, (int32_t)B, T, 1, c.n_fft, c.hop, F);
    if (is < 0) return is;
    l.istft = take(is);
    l.total = off;
    if (lay) *lay = l;
    return off;
}

}  // namespace

namespace wun {

// what wun_spec_workspace_floats and wun_spec_forward check of (cfg, B, T): -> F
int64_t check_spec_shape(const char* who, const wun_spec_config* cfg, int32_t B, int64_t T) {
    int rc;
    if ((rc = check_spec_config(who, cfg))) return rc;
    if (B < 1) return fail(WUN_ERR_INVALID, std::string(who) + ": B < 1");
    const int64_t F = spec_frames(who, *cfg, T);
    if (F < 0) return F;
    if ((rc = check_audio(who, cfg->num_sources, B, T, 1))) return rc;
    if (B * F > ((int64_t)1 << 28) / (cfg->n_fft / 2)) return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 2^28 bins in a batch");
    return F;
}

}  // namespace wun

// ---- the C ABI ----
extern "C" int64_t wun_spec_abi_size(void) { return (int64_t)sizeof(wun_spec_config); }

extern "C" int64_t wun_spec_num_tensors(const wun_spec_config* cfg) {
    int rc;
    if ((rc = check_spec_config("wun_spec_num_tensors", cfg))) return rc;
    return (int64_t)cfg->num_sources * (5 * cfg->num_layers + 5 * (cfg->num_layers - 1) + 2);
}

extern "C" int64_t wun_spec_param_floats(const wun_spec_config* cfg) {
    int rc;
    if ((rc = check_spec_config("wun_spec_param_floats", cfg))) return rc;
    const std::vector<SpecTensor> v = spec_tensors(*cfg);
    int64_t n = 1;
    for (int i = 0; i < v.back().ndim; ++i) n *= v.back().shape[i];
    return v.back().offset + n;
}

extern "C" int wun_spec_tensor(const wun_spec_config* cfg, int64_t index, wun_tensor_info* info) {
    int rc;
    if ((rc = check_spec_config("wun_spec_tensor", cfg))) return rc;
    if (!info) return fail(WUN_ERR_INVALID, "wun_spec_tensor: null info");
    const std::vector<SpecTensor> v = spec_tensors(*cfg);
    if (index < 0 || index >= (int64_t)v.size()) return fail(WUN_ERR_INVALID, "wun_spec_tensor: index outside the table");
    const SpecTensor& t = v[(size_t)index];
    std::memset(info, 0, sizeof(*info));
    std::snprintf(info->name, sizeof(info->name), "%s", t.name.c_str());
    info->offset = t.offset;
    info->ndim = t.ndim;
    for (int i = 0; i < 4; ++i) info->shape[i] = i < t.ndim ? t.shape[i] : 0;
    return WUN_OK;
}

extern "C" int64_t wun_spec_frames(const wun_spec_config* cfg, int64_t T) {
    int rc;
    if ((rc = check_spec_config("wun_spec_frames", cfg))) return rc;
    return spec_frames("wun_spec_frames", *cfg, T);
}

extern "C" int64_t wun_spec_workspace_floats(const wun_spec_config* cfg, int32_t B, int64_t T) {
    const int64_t F = check_spec_shape("wun_spec_workspace_floats", cfg, B, T);
    if (F < 0) return F;
    return spec_layout("wun_spec_workspace_floats", *cfg, B, T, F, nullptr);
}

extern "C" int wun_spec_forward(const wun_spec_config* cfg, const float* params, const float* mix, int32_t B, int64_t T,
                                const float* table_dev, float* audio, float* mags, float* workspace, void* stream) {
    const char* who = "wun_spec_forward";
    if (!cfg || !params || !mix || !table_dev || !workspace) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    if (!audio && !mags) return fail(WUN_ERR_INVALID, std::string(who) + ": audio and mags are both null");
    const int64_t F = check_spec_shape(who, cfg, B, T);
    if (F < 0) return (int)F;
    SpecLayout l;
    const int64_t total = spec_layout(who, *cfg, B, T, F, &l);
    if (total < 0) return (int)total;
    const int L = cfg->num_layers, S = cfg->num_sources, K = cfg->n_fft / 2 + 1, W0 = K - 1;
    const int nif = cfg->num_initial_filters;
    const int64_t np = wun_spec_param_floats(cfg);
    if (overlap(workspace, total, mix, (int64_t)B * T) || overlap(workspace, total, params, np) ||
        (audio && overlap(workspace, total, audio, (int64_t)S * B * T)) || (mags && overlap(workspace, total, mags, (int64_t)S * B * F * K)))
        return fail(WUN_ERR_INVALID, std::string(who) + ": the workspace overlaps another buffer");

    hipStream_t s = (hipStream_t)stream;
    float* ws = workspace;
    const std::vector<SpecTensor> tab = spec_tensors(*cfg);
    int rc;
    // X = STFT(mix) in the loss's framing (through the FFT: its rounding grows with log n_fft, the GEMM's with n_fft, and the
    // largest bins carry that error into the outputs), M = |X|, the network's input log1p(M) without the last bin
    if ((rc = wun_stft_complex_fft(mix, 1, B, T, 1, cfg->n_fft, cfg->hop, 0, F, table_dev, ws + l.re, ws + l.im, stream))) return rc;
    const long long E = (long long)B * F * K;
    hipLaunchKernelGGL(spec_prepare_kernel, dim3(capped_grid(E)), dim3(WUN_STFT_BLOCK), 0, s, ws + l.re, ws + l.im, ws + l.mag, ws + l.a0, E, K);

    size_t ti = 0;                                           // walks the table in its own order
    auto next = [&]() { return params + tab[ti++].offset; };
    for (int src = 0; src < S; ++src) {                      // one network per source (:63)
        const float* cur = ws + l.a0;
        int H = (int)F, W = W0, C = 1;
        for (int i = 0; i < L; ++i) {                        // down: conv, batch norm, LeakyReLU (:68-74)
            C2dArgs a;
            a.x0 = cur; a.x1 = nullptr; a.w = next(); a.y = ws + l.down[i];
            a.epi.bias = next(); a.epi.beta = next(); a.epi.mean = next(); a.epi.var = next(); a.epi.act = C2D_ACT_LRELU;
            a.H = H; a.W = W; a.c0 = C; a.c1 = 0; a.Cout = nif << i;
            a.M = (long long)B * (H / 2) * (W / 2);
            launch_conv(a, s);
            cur = a.y; H /= 2; W /= 2; C = a.Cout;
        }
        const float* skip = nullptr;                         // the second channel range of the next layer's input is `cur`
        int Cs = 0;
        for (int i = 0; i < L - 1; ++i) {                    // up: transposed conv, batch norm, ReLU, concat skip first (:77-83)
            C2dArgs a;
            a.x0 = skip ? skip : cur; a.x1 = skip ? cur : nullptr; a.c0 = skip ? Cs : C; a.c1 = skip ? C : 0;
            a.w = next(); a.y = ws + l.up[i];
            a.epi.bias = next(); a.epi.beta = next(); a.epi.mean = next(); a.epi.var = next(); a.epi.act = C2D_ACT_RELU;
            a.H = H; a.W = W; a.Cout = nif << (L - i - 2);
            a.M = (long long)B * H * W;
            launch_transpose(a, s);
            cur = a.y; H *= 2; W *= 2; C = a.Cout;
            skip = ws + l.down[L - 2 - i]; Cs = nif << (L - 2 - i);
        }
        {                                                    // the mask (:86)
            C2dArgs a;
            a.x0 = skip ? skip : cur; a.x1 = skip ? cur : nullptr; a.c0 = skip ? Cs : C; a.c1 = skip ? C : 0;
            a.w = next(); a.y = ws + l.mask;
            a.epi.bias = next(); a.epi.beta = nullptr; a.epi.mean = nullptr; a.epi.var = nullptr; a.epi.act = C2D_ACT_SIGMOID;
            a.H = H; a.W = W; a.Cout = 1;
            a.M = (long long)B * H * W;
            launch_transpose(a, s);
        }
        hipLaunchKernelGGL(spec_mask_kernel, dim3(capped_grid(E)), dim3(WUN_STFT_BLOCK), 0, s, ws + l.mask, ws + l.mag, ws + l.re, ws + l.im,
                           mags ? mags + (long long)src * E : nullptr, audio ? ws + l.yre + (long long)src * E : nullptr,
                           audio ? ws + l.yim + (long long)src * E : nullptr, E, K);
    }
    if (audio && (rc = wun_istft_tf_fft(ws + l.yre, ws + l.yim, S, B, T, 1, cfg->n_fft, cfg->hop, F, table_dev, audio, ws + l.istft, stream)))
        return rc;
    return launch_status(who);
}

extern "C" int wun_op_conv2d_s2(const float* x, const float* w, const float* bias, const float* bn_mean, const float* bn_var,
                                const float* bn_beta, float* y, int B, int H, int W, int cin, int cout, int act, void* stream) {
    const char* who = "wun_op_conv2d_s2";
    if (!x || !w || !y) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    int rc;
    if ((rc = check_c2d(who, B, H, W, cin, cout, act, bn_mean, bn_var, bn_beta))) return rc;
    if ((H | W) & 1) return fail(WUN_ERR_INVALID, std::string(who) + ": H and W must be even");
    C2dArgs a;
    a.x0 = x; a.x1 = nullptr; a.w = w; a.y = y;
    a.epi.bias = bias; a.epi.mean = bn_mean; a.epi.var = bn_var; a.epi.beta = bn_beta; a.epi.act = act;
    a.H = H; a.W = W; a.c0 = cin; a.c1 = 0; a.Cout = cout;
    a.M = (long long)B * (H / 2) * (W / 2);
    launch_conv(a, (hipStream_t)stream);
    return launch_status(who);
}

extern "C" int wun_op_conv2d_transpose_s2(const float* x0, int c0, const float* x1, int c1, const float* w, const float* bias,
                                          const float* bn_mean, const float* bn_var, const float* bn_beta, float* y, int B, int H,
                                          int W, int cout, int act, void* stream) {
    const char* who = "wun_op_conv2d_transpose_s2";
    if (!x0 || !w || !y) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    if (c0 < 1 || c1 < 0 || (x1 != nullptr) != (c1 > 0))
        return fail(WUN_ERR_INVALID, std::string(who) + ": c0 < 1, c1 < 0, or x1 and c1 disagree");
    if (c0 > (1 << 16) || c1 > (1 << 16)) return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 65536 channels");
    int rc;
    if ((rc = check_c2d(who, B, H, W, c0 + c1, cout, act, bn_mean, bn_var, bn_beta))) return rc;
    C2dArgs a;
    a.x0 = x0; a.x1 = x1; a.w = w; a.y = y;
    a.epi.bias = bias; a.epi.mean = bn_mean; a.epi.var = bn_var; a.epi.beta = bn_beta; a.epi.act = act;
    a.H = H; a.W = W; a.c0 = c0; a.c1 = c1; a.Cout = cout;
    a.M = (long long)B * H * W;
    launch_transpose(a, (hipStream_t)stream);
    return launch_status(who);
}
