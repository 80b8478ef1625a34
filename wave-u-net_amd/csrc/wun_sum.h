// THE summation constants of the loss entries (wun_spectral.hip: the STFT losses; wun_waveform.hip: the waveform losses): every
// float64 partial sum covers 1024 consecutive elements -- lane `tid` of a 256-lane block takes the items tid + 256 it, it = 0..3,
// in ascending order, and one fixed tree adds the lanes.  One copy, so that the two units' sums of the same floats are the same
// bits (wun_waveform_loss with {mse} alone IS wun_spectral_loss at nres = 0, bit for bit).
#pragma once

#define WUN_STFT_BLOCK 256           // threads per workgroup of every kernel of the STFT family and of the loss sums (4 waves)
#define WUN_STFT_ITEMS 4             // elements per lane of the loss / gradient kernels: 1024 per partial

namespace wun {

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

// Q sums at once: the tree above for each of v[0 .. Q), sharing its barriers -- every sum takes the adds of stft_block_sum in
// the same order, so the same bits.  v[q] holds sum q afterwards, in every lane.
template <int Q>
__device__ __forceinline__ void stft_block_sums(double (*red)[WUN_STFT_BLOCK], double* v, int tid) {
#pragma unroll
    for (int q = 0; q < Q; ++q) red[q][tid] = v[q];
    __syncthreads();
    for (int s = WUN_STFT_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < Q; ++q) red[q][tid] += red[q][tid + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = red[q][0];
}

}  // namespace wun

namespace {

// float64 partials of n elements: one per 1024
long long parts_of(long long n) { return (n + WUN_STFT_BLOCK * WUN_STFT_ITEMS - 1) / (WUN_STFT_BLOCK * WUN_STFT_ITEMS); }

}  // namespace
