// What the STFT family shares (wun_spectral.hip: the loss; wun_postfilter.hip: the complex STFT, its inverse and the filters):
// the GEMM tile of a forward and of an inverse frame transform on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32), its constants,
// and the host helpers of the entries -- argument checks, the float64 tail of a scratch, the check after the launches.
//
//   forward    Re / Im[m][k] = sum_n frame_m[n] * Cb / Sb[n][k]: the frames are gathered from the channel-last audio while the
//              A tile is staged in LDS (stride C, scalar loads: any 4-byte alignment); no frame matrix in HBM
//   inverse    frame[m][n] = sum_k re[m][k] * Cb[n][k] + im[m][k] * Sb[n][k]: the transposed GEMM on the same table
//
// One workgroup of 256 lanes computes 64 frame rows x 32 columns: 2 x 2 waves, each 32 rows x 16 columns.  Lane layout of the MFMA
// (wun_op_mfma_probe): A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15], D[row = 4 (lane >> 4) + reg]
// [col = lane & 15].  Every reduction index runs in ascending order inside one lane's accumulator, whatever the tile a frame
// falls in: the bits of a frame do not depend on the rows around it, the grid, or pointer alignment.
#pragma once
#include "wun_fft.h"
#include "wun_sum.h"
#include "../../include/wun.h"

#include <cstdint>
#include <string>

int fail(int code, const std::string& msg);      // wun_plan.hip: sets wun_last_error(), returns code

// (WUN_STFT_BLOCK, the 256 threads per workgroup of every kernel of the family: wun_sum.h)
#define WUN_STFT_BM 64               // frames per GEMM workgroup
#define WUN_STFT_BN 32               // columns per GEMM workgroup (forward: bins, re and im each; inverse: samples of a frame)
#define WUN_STFT_KC 32               // reduction indices staged per step
#define WUN_STFT_PA 36               // LDS pitch of a tile read as [row = lane & 15][k = lane >> 4]: 36 r + k hits 64 banks once
#define WUN_STFT_PB 48               // LDS pitch of a tile read as [k = lane >> 4][col = lane & 15]: 48 k + c hits 64 banks once

namespace wun {

__device__ __forceinline__ f32x4 stft_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// The forward tile of workgroup (blockIdx.x = tile of 64 frame rows, blockIdx.y = tile of 32 bins) over the M frame rows of x.
// row(m, base, t0): the offset of sample 0 of the frame row's audio row, and the sample index of the frame's n = 0; sample t of
// that row lies at x[base + t * C].  BOUNDED: a frame may reach outside [0, T), every gathered sample is checked and reads as 0
// there; otherwise every frame lies inside and the check (and its registers) are left out.  store(m, k, re, im) is called once
// for every frame row m < M and bin k < K of the tile.  table: Cb [n_fft][K], then Sb [n_fft][K].
template <bool BOUNDED, class Row, class Store>
__device__ __forceinline__ void stft_fwd_tile(const float* __restrict__ x, const float* __restrict__ table, long long M,
                                              long long T, int C, int n_fft, int K, Row row, Store store) {
    __shared__ float As[WUN_STFT_BM * WUN_STFT_PA];
    __shared__ float Bc[WUN_STFT_KC * WUN_STFT_PB];
    __shared__ float Bs[WUN_STFT_KC * WUN_STFT_PB];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int sc = tid & 31, sr = tid >> 5;                  // staging: column and first row of this lane
    const long long m0 = (long long)blockIdx.x * WUN_STFT_BM;
    const int k0 = (int)blockIdx.y * WUN_STFT_BN;
    const int wm = (w & 1) * 32, wk = (w >> 1) * 16;

    // BOUNDED: the row's sample 0 and the frame's first sample index (may be negative); else the frame's first sample itself.
    long long aoff[WUN_STFT_BM / 8], t0[BOUNDED ? WUN_STFT_BM / 8 : 1];      // aoff -1: behind the last frame row
#pragma unroll
    for (int it = 0; it < WUN_STFT_BM / 8; ++it) {
        const long long m = m0 + sr + 8 * it;
        aoff[it] = -1;
        if (BOUNDED) t0[it] = 0;
        if (m < M) {
            long long base, t;
            row(m, base, t);
            if (BOUNDED) { aoff[it] = base; t0[it] = t; }
            else aoff[it] = base + t * C;
        }
    }
    const bool kin = k0 + sc < K;
    const float* __restrict__ tc = table + k0 + sc;
    const float* __restrict__ ts = tc + (long long)n_fft * K;

    f32x4 are[2], aim[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) { are[i] = (f32x4){0.f, 0.f, 0.f, 0.f}; aim[i] = are[i]; }

    for (int n0 = 0; n0 < n_fft; n0 += WUN_STFT_KC) {        // ascending n: the one accumulation order
        __syncthreads();                                     // the previous step is read
#pragma unroll
        for (int it = 0; it < WUN_STFT_BM / 8; ++it) {
            if (BOUNDED) {
                const long long t = t0[it] + n0 + sc;
                const bool in = aoff[it] >= 0 && t >= 0 && t < T;
                As[(sr + 8 * it) * WUN_STFT_PA + sc] = in ? x[aoff[it] + t * C] : 0.f;
            } else {
                As[(sr + 8 * it) * WUN_STFT_PA + sc] = aoff[it] >= 0 ? x[aoff[it] + (long long)(n0 + sc) * C] : 0.f;
            }
        }
#pragma unroll
        for (int it = 0; it < WUN_STFT_KC / 8; ++it) {
            const int nl = sr + 8 * it;
            const long long idx = (long long)(n0 + nl) * K;
            Bc[nl * WUN_STFT_PB + sc] = kin ? tc[idx] : 0.f;
            Bs[nl * WUN_STFT_PB + sc] = kin ? ts[idx] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < WUN_STFT_KC / 4; ++s) {
            const int kq = 4 * s + lq;
            const float a0 = As[(wm + lr) * WUN_STFT_PA + kq], a1 = As[(wm + 16 + lr) * WUN_STFT_PA + kq];
            const float bc = Bc[kq * WUN_STFT_PB + wk + lr], bs = Bs[kq * WUN_STFT_PB + wk + lr];
            are[0] = stft_mfma(a0, bc, are[0]);
            aim[0] = stft_mfma(a0, bs, aim[0]);
            are[1] = stft_mfma(a1, bc, are[1]);
            aim[1] = stft_mfma(a1, bs, aim[1]);
        }
    }
    const int k = k0 + wk + lr;
    if (k >= K) return;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long m = m0 + wm + 16 * i + 4 * lq + r;
            if (m < M) store(m, k, are[i][r], aim[i][r]);
        }
}

// The inverse tile of workgroup (blockIdx.x = tile of 64 frame rows, blockIdx.y = tile of 32 samples of the frame):
// frames[m][n] for the M frame rows whose spectra start at re / im[srow(m)].  The reduction runs over the bins in ascending order,
// a bin's real part before its imaginary part; bins behind K are staged as zeros.  SCALED: bin k is multiplied by c_edge
// (k = 0 and k = K - 1) or c_mid while it is staged -- powers of two, so exact; otherwise nothing is multiplied.
template <bool SCALED, class SpecRow>
__device__ __forceinline__ void stft_inv_tile(const float* re, const float* im, const float* table, float* frames, long long M,
                                              int n_fft, int K, float c_edge, float c_mid, SpecRow srow_of) {
    __shared__ float Ar[WUN_STFT_BM * WUN_STFT_PA];
    __shared__ float Ai[WUN_STFT_BM * WUN_STFT_PA];
    __shared__ float Bc[WUN_STFT_BN * WUN_STFT_PA];
    __shared__ float Bs[WUN_STFT_BN * WUN_STFT_PA];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int sc = tid & 31, sr = tid >> 5;
    const long long m0 = (long long)blockIdx.x * WUN_STFT_BM;
    const int n0 = (int)blockIdx.y * WUN_STFT_BN;
    const int wm = (w & 1) * 32, wn = (w >> 1) * 16;
    const float* __restrict__ tc = table;
    const float* __restrict__ ts = table + (long long)n_fft * K;

    long long srow[WUN_STFT_BM / 8];                         // first float of this lane's spectrum rows (-1: behind the last)
#pragma unroll
    for (int it = 0; it < WUN_STFT_BM / 8; ++it) {
        const long long m = m0 + sr + 8 * it;
        srow[it] = m < M ? srow_of(m) : -1;
    }

    f32x4 acc[2];
    acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
    for (int k0 = 0; k0 < K; k0 += WUN_STFT_KC) {            // ascending k
        __syncthreads();
        const int k = k0 + sc;
        const bool kin = k < K;
        const float ck = (k == 0 || k == K - 1) ? c_edge : c_mid;
#pragma unroll
        for (int it = 0; it < WUN_STFT_BM / 8; ++it) {
            const bool in = kin && srow[it] >= 0;
            Ar[(sr + 8 * it) * WUN_STFT_PA + sc] = in ? (SCALED ? ck * re[srow[it] + k] : re[srow[it] + k]) : 0.f;
            Ai[(sr + 8 * it) * WUN_STFT_PA + sc] = in ? (SCALED ? ck * im[srow[it] + k] : im[srow[it] + k]) : 0.f;
        }
#pragma unroll
        for (int it = 0; it < WUN_STFT_BN / 8; ++it) {
            const int nl = sr + 8 * it;
            const long long idx = (long long)(n0 + nl) * K + k;
            Bc[nl * WUN_STFT_PA + sc] = kin ? tc[idx] : 0.f;
            Bs[nl * WUN_STFT_PA + sc] = kin ? ts[idx] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < WUN_STFT_KC / 4; ++s) {
            const int kq = 4 * s + lq;
            const float bc = Bc[(wn + lr) * WUN_STFT_PA + kq], bs = Bs[(wn + lr) * WUN_STFT_PA + kq];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                acc[i] = stft_mfma(Ar[(wm + 16 * i + lr) * WUN_STFT_PA + kq], bc, acc[i]);
                acc[i] = stft_mfma(Ai[(wm + 16 * i + lr) * WUN_STFT_PA + kq], bs, acc[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long m = m0 + wm + 16 * i + 4 * lq + r;
            if (m < M) frames[m * n_fft + n0 + wn + lr] = acc[i][r];
        }
}

}  // namespace wun

// ---- host helpers of the entries: every check runs before any GPU work, `who` names the entry in wun_last_error() ----
namespace {

int check_audio(const char* who, int32_t S, int32_t B, int64_t T, int32_t C) {
    if (S < 1 || B < 1) return fail(WUN_ERR_INVALID, std::string(who) + ": S < 1 or B < 1");
    if (C != 1 && C != 2) return fail(WUN_ERR_INVALID, std::string(who) + ": C must be 1 or 2");
    if (T < 1) return fail(WUN_ERR_INVALID, std::string(who) + ": no frames");
    if ((int64_t)S * B > ((int64_t)1 << 24) || T > ((int64_t)1 << 40) / ((int64_t)S * B * C))
        return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 2^24 rows or 2^40 floats");
    return WUN_OK;
}

// n_fft (UNSUPPORTED), then hop (INVALID); tr: the GEMM's table grows as n_fft^2 / 2 and stops at 2048, the FFT path goes on to
// 8192.  T: the samples a whole frame must fit in (the loss's framing has no padding); the centred framing passes none -- a
// track shorter than a frame is legal there.
int check_res(const char* who, int tr, int32_t n_fft, int32_t hop, int64_t T = INT64_MAX) {
    const int32_t n_max = tr == wun::WUN_TR_FFT ? 8192 : 2048;
    if (n_fft < 64 || n_fft > n_max || (n_fft & (n_fft - 1)))
        return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": n_fft must be a power of two in 64.." + (tr == wun::WUN_TR_FFT ? "8192" : "2048"));
    if (hop < 1 || hop > n_fft) return fail(WUN_ERR_INVALID, std::string(who) + ": hop outside 1..n_fft");
    if (T < n_fft) return fail(WUN_ERR_INVALID, std::string(who) + ": fewer frames than n_fft (no padding)");
    return WUN_OK;
}

// the float64 tail of a scratch: behind `floats` floats, on an 8-byte boundary (the *_scratch_floats counts leave 2 floats for it)
double* f64_tail(float* scratch, long long floats) {
    uintptr_t pa = (uintptr_t)(scratch + floats);
    pa = (pa + 7) & ~(uintptr_t)7;
    return (double*)pa;
}

// after the launches of an entry: WUN_OK, or WUN_ERR_HIP with the runtime's message
int launch_status(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(WUN_ERR_HIP, std::string(who) + " launch: " + hipGetErrorString(e));
    return WUN_OK;
}

}  // namespace
