// What the two units of the spectrogram U-Net share (wun_conv2d.hip: the convolutions, the variable table, inference;
// wun_conv2d_train.hip: the training step): the argument blocks of the two convolution kernels, their launchers,
// the variable table and the shape checks.  The kernels themselves live in wun_conv2d.hip only.
#pragma once
#include "wun_stft.h"

#include <string>
#include <vector>

#define WUN_C2D_EPS 1e-3f            // tf.contrib.layers.batch_norm's epsilon
#define WUN_SPEC_MAX_LAYERS 10
#define WUN_SPEC_MAX_SOURCES 8

namespace wun {

enum { C2D_ACT_NONE = 0, C2D_ACT_LRELU = 1, C2D_ACT_RELU = 2, C2D_ACT_SIGMOID = 3 };

struct C2dEpilogue {
    const float* bias;                       // [Cout] or null
    const float* mean;                       // [Cout] each, or all three null: no batch norm
    const float* var;
    const float* beta;
    int act;
};

struct C2dArgs {
    const float* x0;                         // conv: [B][H][W][Cin];  transposed: [B][H][W][c0]
    const float* x1;                         // transposed: [B][H][W][c1] or null
    const float* w;                          // conv: [5][5][Cin][Cout];  transposed: [5][5][Cout][Cin]
    float* y;                                // conv: [B][H/2][W/2][Cout];  transposed: [B][2H][2W][Cout]
    C2dEpilogue epi;
    long long M;                             // conv: B (H/2) (W/2);  transposed: B H W
    int H, W, c0, c1, Cout;                  // the INPUT map (Cin = c0 + c1)
};

struct SpecTensor { std::string name; int64_t offset; int ndim; int64_t shape[4]; };

// wun_conv2d.hip -- the launchers of its four convolution kernels (the first down layer, Cin == 1, and the mask layer, Cout == 1,
// run on the VALU) and of the two point-wise kernels around the network; a bias alone with act 0 stores z = conv + bias
void launch_conv(const C2dArgs& a, hipStream_t s);
void launch_transpose(const C2dArgs& a, hipStream_t s);
// mag = |re + i im| [B F K], a0 = log1p(mag) without the last bin; E = B F K
void launch_spec_prepare(const float* re, const float* im, float* mag, float* a0, long long E, int K, hipStream_t s);
// mags = mag * mask (0.5 at the dropped bin) and / or (yre, yim) = mask * (re, im); null outputs are not written
void launch_spec_mask(const float* mask, const float* mag, const float* re, const float* im, float* mags, float* yre, float* yim,
                      long long E, int K, hipStream_t s);
int check_spec_config(const char* who, const wun_spec_config* c);
std::vector<SpecTensor> spec_tensors(const wun_spec_config& c);
// what wun_spec_workspace_floats and wun_spec_forward check of (cfg, B, T): -> F, or a negative wun_status
int64_t check_spec_shape(const char* who, const wun_spec_config* cfg, int32_t B, int64_t T);

inline unsigned capped_grid(long long lanes) {
    long long g = (lanes + WUN_STFT_BLOCK - 1) / WUN_STFT_BLOCK;
    if (g > (1 << 16)) g = 1 << 16;
    return (unsigned)(g < 1 ? 1 : g);
}

inline bool overlap(const void* a, long long na, const void* b, long long nb) {       // float counts
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + 4 * (uintptr_t)na, b0 = (uintptr_t)b, b1 = b0 + 4 * (uintptr_t)nb;
    return a0 < b1 && b0 < a1;
}

}  // namespace wun
