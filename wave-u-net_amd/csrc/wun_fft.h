// What wun_postfilter.hip (the host orchestration of the transforms and filters) and wun_fft.hip (the FFT kernels) share: the
// argument blocks of a forward and an inverse frame transform, and the launchers of the FFT path.  Both transforms of one
// direction take the same block, so the orchestration picks one by a selector and nothing else changes.  wun_spectral.hip (the
// spectral loss) launches the forward body with its magnitude epilogue and the inverse body as an adjoint the same way.
#pragma once
#include "wun_device.h"
#include "../../include/wun.h"

namespace wun {

enum { WUN_TR_GEMM = 0, WUN_TR_FFT = 1 };

// Frame rows of one launch: m = r * nb + fl is frame f0 + fl of row r; its spectrum lies at row r * fstride + foff + fl of
// re / im [.][K] (a whole transform: nb = fstride = F, f0 = foff = 0; a block of the filter: fstride = nb, foff = 0).
struct StftCfwdArgs {
    const float* x[2];               // [SB, T, C]; blockIdx.z picks one (the estimates, the mix)
    float* re[2]; float* im[2];
    long long M[2];                  // frame rows of the signal: rows * nb
    const float* table;              // GEMM: Cb [n_fft][K], then Sb [n_fft][K];  FFT: wun_fft_design's table
    long long T, nb, f0, fstride, foff;
    int C, n_fft, hop, lead, K;
};

struct IstftGemmArgs {
    const float* re; const float* im;        // the spectrum of frame row m = r * nb + fl at row r * fstride + foff + fl
    const float* table;
    float* frames;                           // [M][n_fft]
    long long M, nb, fstride, foff;
    int n_fft, K;
    float c_edge, c_mid;                     // 1 / n_fft for k = 0 and k = n_fft / 2, 2 / n_fft between
};

// The forward transform with the spectral loss's epilogue: mag[z][e] = sqrt(re^2 + im^2) of every bin of signal z, and Re / Im
// into a.re[z] / a.im[z] where those are not null.
struct StftMagArgs {
    StftCfwdArgs a;
    float* mag[2];
};

// The forward transform with the spectrogram U-Net's mask-gradient epilogue: a.x[0] is u = d_audio / D, G = STFT(u)
// stays in registers, and for every bin k < K - 1 of frame row bf
//   ga = c_k fmaf(xre, Re G, xim Im G)  (c_k = c_edge at k = 0, c_mid elsewhere),  dmask = dmags ? fmaf(dmags, mag, ga) : ga,
//   dz[bf (K - 1) + k] = dmask * (mask * (1 - mask)).
// a.re / a.im are not read; bin K - 1 stores nothing.
struct SpecHeadArgs {
    StftCfwdArgs a;
    const float* xre; const float* xim; const float* mag;        // [B F][K]: the mix's spectrum and its magnitude
    const float* mask;                                           // [B F][K - 1]
    const float* dmags;                                          // [B F][K] or null
    float* dz;                                                   // [B F][K - 1]
    float c_edge, c_mid;                                         // 1 / n_fft, 2 / n_fft
};

// One Griffin-Lim iteration on the frame rows of a block (wun_griffin_lim): frame row m = r * nb + fl is frame
// f = f0 + fl of row r; its bins lie at (r * F + f) * K of mag, cre / cim and pre / pim, its partial sums at (r * F + f) * 2.
struct GlArgs {
    const float* x;                          // y_{i-1} [SB, T, C] (not read when the spectrum is given)
    const float* cre; const float* cim;      // the given spectrum c_0 (read only then)
    const float* mag;
    float* pre; float* pim;                  // c_{i-1}, or null: momentum 0
    double* part;                            // [R][F][2], or null: no inconsistency asked for (never written from a given spectrum)
    const float* table;
    float* frames;                           // [M][n_fft]
    long long M, nb, f0, F, T;
    long long last_below;                    // frames f < last_below are computed for the last time in this iteration: they
                                             // alone store c_i and their partial sums (a later block computes the others again)
    int C, n_fft, hop, lead, K;
    int first;                               // iteration 0: t_0 = c_0, c_{i-1} is not read
    float momentum, scale;                   // scale = 1 / n_fft
};

// One launch set of the phase vocoder (wun_time_stretch): up to WUN_STRETCH_JOBS jobs by value.  Job j owns the
// frames [fp[j], fp[j + 1]) of each of its C rows: frame f of (j, c) is frame row C fp[j] + c F_j + f of mag / dlt [rows][K] and
// of the synthesis frames; the analysis workgroups [gp[j], gp[j + 1]) are its C ceil(F_j / FPW) groups of FPW frames, c-major.
struct VocArgs {
    wun_stretch_job job[WUN_STRETCH_JOBS];
    long long fp[WUN_STRETCH_JOBS + 1];
    long long gp[WUN_STRETCH_JOBS + 1];
    const float* table;                      // wun_fft_design's
    float* mag; float* dlt;                  // [rows][K]: |X_f| and the phase increment in turns; the phase kernel leaves Re Y, Im Y
    int J, C, n_fft, hop, K;
};
static_assert(sizeof(VocArgs) <= 4096, "the argument block must fit HIP's kernel-argument limit");

// wun_fft.hip: stft_fft_kernel / istft_fft_kernel of a.n_fft (a power of two in 64..8192) on stream s.  WUN_OK, or
// WUN_ERR_UNSUPPORTED (wun_last_error() set, nothing launched) for an n_fft without a kernel.
//   magnitude   the forward body with StftMagArgs' epilogue (the spectral loss and wun_stft_magnitude_fft)
//   adjoint     the inverse body as the UNSCALED adjoint of the forward transform, every bin counted once (stft_bwd_kernel's
//               definition): g.c_edge must be 1 / 2, g.c_mid is not read
// Each launcher below adds 1 to the host-side ledger [WUN_FFT_FAMILY_*][log2(n_fft) - 6] once the runtime has taken its launch
// (wun_fft_launch_counts, include/wun.h: test entries; nothing else reads it).
int fft_launch_forward(const StftCfwdArgs& a, int signals, hipStream_t s);
int fft_launch_magnitude(const StftMagArgs& a, int signals, hipStream_t s);
int fft_launch_inverse(const IstftGemmArgs& g, hipStream_t s);
int fft_launch_adjoint(const IstftGemmArgs& g, hipStream_t s);
//   spec_head   the forward body on a.x[0] with SpecHeadArgs' epilogue, one signal
int fft_launch_spec_head(const SpecHeadArgs& a, hipStream_t s);
//   griffin_lim gl_frame_kernel on the frame rows of g; given: c_0 is g.cre / g.cim and no forward transform runs
int fft_launch_griffin_lim(const GlArgs& g, bool given, hipStream_t s);
//   voc_analysis voc_analysis_kernel on the jobs of v: |X_f| and the phase increment of every frame row of v.fp, on v.gp[v.J]
//               workgroups of fft_frames_per_workgroup(n_fft) frames (0 for an n_fft without a kernel)
int fft_frames_per_workgroup(int n_fft);
int fft_launch_voc_analysis(const VocArgs& v, hipStream_t s);
// out[0], out[1] = the sums of part[e][0] and part[e][1] over e = 0 .. n - 1 in ascending e (one workgroup); n < 0: NaN into both
void launch_gl_finish(const double* part, long long n, double* out, hipStream_t s);
// D[p] = (float) sum_i w^2[p + i hop] over p + i hop < n_fft (float64, i ascending: istft_ola_kernel<true>'s normaliser), p < hop
void launch_steady_den(float* D, int n_fft, int hop, hipStream_t s);
// u[e] = g[e] / D[(e mod T) mod hop] for the N = rows T samples of [rows][T]
void launch_steady_divide(const float* g, const float* D, float* u, long long N, long long T, int hop, hipStream_t s);

}  // namespace wun
