// Internal: kernel argument blocks + launcher prototypes shared by the device units (wun_kernels.hip, ...) and the
// host units (wun_plan.hip and the files of wun_plan_impl.h: plan, dispatch, the step's passes, tuner, C ABI).  Host declarations only:
// the device helpers of the kernel units live in wun_device.h.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>
#include <string>

namespace wun {

enum { LOADER_DIRECT = 0, LOADER_DEINT = 1 };

// Every environment switch the library reads (debugging / experiment switches; the defaults are the shipped schedule),
// parsed in ONE place: wun_switches_from_env (wun_plan.hip).  wun_plan_create stores a snapshot in the plan and every
// later decision for that plan reads it; the single-operator entry points take a fresh snapshot per call; the launchers
// below receive it as a parameter.
enum WunEarlyWindow { EW_DEFAULT, EW_OFF, EW_DEEP, EW_ALL };     // (EW_DEFAULT: all levels on dedup plans, else deep)
enum WunEventScope { EV_DEFAULT, EV_SYSTEM, EV_DEVICE };
enum WunSidePrio { PRIO_DEFAULT, PRIO_LOW, PRIO_HIGH, PRIO_NORMAL };
struct WunSwitches {
    // ---- schedule ----
    bool no_dedup = false;              // WUN_NO_DEDUP (set): rounds 1 - 5's down-level launch sequence on context plans
    WunEarlyWindow early_window = EW_DEFAULT;   // WUN_EARLY_WINDOW: first char '0' = off, 'a' = all, any other = deep
    bool odd_fuse_set = false;          // WUN_ODD_FUSE_MIN (set): fuse floor of the odd-window input gradients ...
    int odd_fuse_min = 64;              // ... atoi of its value (default 64)
    bool no_odd_align = false;          // WUN_NO_ODD_ALIGN (set): odd-window launches keep their odd start (no shifted filter)
    bool no_fuse_ups = false;           // WUN_NO_FUSE_UPS (set): separate (adjoint) upsampling kernels, never the fused epilogue
    bool bf16_head_serial = false;      // WUN_BF16_HEAD_SERIAL (set): bf16 mode, LDS-staged narrow launch on the caller's stream
    // ---- streams ----
    bool single_stream = false;         // WUN_SINGLE_STREAM (set): everything on the caller's stream
    WunSidePrio side_prio = PRIO_DEFAULT;   // WUN_SIDE_PRIO: first char 'l' = lowest, 'h' = highest, anything else = 0
    WunEventScope event_scope = EV_DEFAULT;  // WUN_EVENT_SCOPE: first char 's' = system fence, 'd' = device release
    // ---- kernel selection ----
    bool no_win = false;                // WUN_NO_WIN (set): no register-window weight-gradient kernel
    bool no_narrow = false;             // WUN_NO_NARROW (set): MFMA weight gradients for the output head / audio-input conv
    bool no_narrow_down0 = false;       // WUN_NO_NARROW_DOWN0 (set): ... for the audio-input conv only
    bool no_narrow_stream = false;      // WUN_NO_NARROW_STREAM: atoi != 0 -- LDS-staged narrow kernel, never the streaming form
    int narrow_splits = 0;              // WUN_NARROW_SPLITS: split cap of the narrow kernels, max(1, atoi) (0 = unset)
    bool no_dma = false;                // WUN_NO_DMA (set): register staging for every conv tile (no DMA instantiation)
    bool no_k3 = false;                 // WUN_NO_K3: atoi != 0 -- no in-workgroup split-K conv tiles
    int win_tk = 64;                    // WUN_WIN_TK: register-window positions per unit, only 16 / 32 / 64 / 128 accepted
    int bf16_lds_cap = 80;              // WUN_BF16_LDS_CAP: KiB of LDS a bf16 conv tile may take (atoi, default 80)
    // ---- tuner ----
    int tune_rounds = 4;                // WUN_TUNE_ROUNDS: round-robin timing rounds per launch position, max(1, atoi)
    bool tune_log = false;              // WUN_TUNE_LOG (set): one stderr line per tuned launch position
    std::string tune_alts;              // WUN_TUNE_ALTS: file the near-best candidates are appended to (empty = off)
    int tune_alts_max = 6;              // WUN_TUNE_ALTS_MAX: candidates per position, atoi (<= 0 gives 6)
    float tune_alts_tol = 1.15f;        // WUN_TUNE_ALTS_TOL: "near" = within this factor of the best, atof (<= 1 gives 1.15)
    // ---- diagnostics ----
    bool dump_layout = false;           // WUN_DUMP_LAYOUT (set): workspace map on stderr at plan creation
    bool profile_detail = false;        // WUN_PROFILE_DETAIL (set): per-launch list in the profile JSON (read at wun_profile_begin)
    bool win_occ = false;               // WUN_WIN_OCC (set): occupancy line on stderr per register-window launch
};
WunSwitches wun_switches_from_env();

// Epilogue flag bits
enum { F_LRELU = 1, F_ACCUM = 2, F_VEC4 = 4, F_PHASE2 = 8 };

// One implicit-GEMM 1-D convolution launch.  The input is a virtual channel-concat of
// up to two NCW sources, zero outside [0, Tin) (this is how crop+concat, 'same' zero
// padding and the halo of valid convolutions are expressed without copies).
//   DIRECT: out[b][n][q] = epi( sum_{j<J, c} W[j][c][n] * in[b][c][q + j - shift] )
//   DEINT : out[b][n][q] = epi( sum_{k<KW,c} W[k][c][n] * in[b][c][2q + k - shift] )
// Outputs n < N0 go to dst0, the rest to dst1 (dgrad of a concat).  Output element q is
// stored at dst[b*obs + n*opitch + ooff + q*ostride]; msk (same geometry as dst) applies
// the LeakyReLU derivative of the forward activation stored there; dec receives a
// compact copy of the even q (the [:, ::2, :] decimation) of dst0.
struct ConvArgs {
    const float* src0; const float* src1;
    long long bs0, bs1;
    int pitch0, pitch1;
    int off0, off1;
    int C0, C1;
    int Tin;
    int shift;
    const float* W;
    const float* bias;
    int KW;          // taps (DIRECT: J = KW; DEINT: J = ceil(KW/2))
    int N;           // output channels
    int N0;          // split point between dst0 / dst1
    float* dst0; float* dst1;
    long long obs0, obs1;
    int opitch0, opitch1;
    int ooff0, ooff1;
    const float* msk0; const float* msk1;
    int ostride;
    int Tout;
    float* dec; long long decbs; int decpitch;
    // Round 6 (context plans of the exact-fp32 mode: the decimated stream IS a slice of the encoder output,
    // UnetAudioSeparator.py:98-100, computed once): two more copies of dst0, same validity rules as `dec`.
    //   dec_exp != 0: `dec` is an EXPANDED copy instead of a compact one -- output q goes to dec[b][n][2q - dec_lo] when
    //                 0 <= 2q - dec_lo < dec_len (the stride-2 conv of a down level writes the even positions of the skip window);
    //   dec1        : compact copy of the ODD q of dst0, dec1[b][n][q >> 1] (an up level's input gradient splits the skip
    //                 window's gradient by the parity of the absolute conv position: one half is added to the decimated
    //                 stream's gradient, the other feeds the odd-position launches).
    int dec_exp; int dec_lo; unsigned dec_len;
    float* dec1; long long dec1bs; int dec1pitch;
    int dec_off, dec1_off;       // first element of the copies inside their rows, in ELEMENTS of the copy's tensor (fp32 or bf16)
    int flags;
    int B;
    int loader;
    int Tlim;        // F_PHASE2: true output length (outputs t = 2q+p < Tlim)
    int kw_full;     // F_PHASE2: taps of the forward conv (FLOP accounting)
    int force_variant;   // autotuner: tile variant index + 1 (0 = heuristic)
    int force_ksplit;    // autotuner: split-K factor (0 = heuristic)
    int cps;         // split-K: channel chunks per split (set by the launcher)
    float* part;     // split-K partial buffer (set by the launcher) or null
    int wb_c8p, wb_npad;   // bf16 mode: W points at the packed image [KW][wb_c8p][wb_npad][8] (wun_bf16.hip)
    // F_ACCUM applies to the row positions pos = ooff + q*ostride with acc_lo <= pos < acc_lo + acc_len only; elsewhere
    // the result is stored.  (A down level's input gradient = transposed stride-2 conv over the whole row + the
    // skip-window conv over the crop window: the window part is computed EARLY on a side stream, the row-wide part
    // adds it inside the window.)  acc_len == 0 is normalised by conv_output_setup to "the whole row".  Every conv kernel
    // applies msk, F_ACCUM and the copies through the one epilogue of wun_device.h (conv_out_vec / conv_out1).
    int acc_lo; unsigned acc_len;
    // Fused 2x upsampling of the dst0 output (UnetAudioSeparator.py:109-118, InterpolationLayer.py:19-39): when the launch
    // ends in the split-K epilogue kernel, that kernel also writes ups_y[b][c][0 .. ups_tup) = {y[i], interp(y[i], y[i+1])}
    // (ups_w: learned per-channel weights before the sigmoid, or null = linear; ups_tup = 2n - 1 with context, 2n without)
    // -- the same arithmetic as upsample_vec_kernel, which the caller then does not launch (conv_last_fused_ups()).
    float* ups_y; long long ups_bs; int ups_pitch; int ups_tup; const float* ups_w;
    // ... and its adjoint for the dst1 columns of an up conv's input gradient (linear interpolation only): instead of
    // storing d_up, the split-K epilogue writes ubw_dz[b][c][i] = (d_up[2i] + wa d_up[2i+1] + 1/2 d_up[2i-1]) *
    // LeakyReLU'(ubw_x[b][c][i]) -- the arithmetic of upsample_bwd_vec_kernel; rows of ubw_dz / ubw_x share one geometry.
    float* ubw_dz; const float* ubw_x; long long ubw_bs; int ubw_pitch; int ubw_n;
    // bf16 storage (compute_dtype = 1, section "bf16 activations in HBM" of DESIGN.md): xbf -- src0 / src1 point at bf16
    // elements; obf -- dst0 / dst1 / msk0 / msk1 / dec point at bf16 elements.  All pitches, batch strides and offsets of a
    // tensor are in ITS elements.  Only the bf16 kernels (wun_bf16.hip) read these.
    int xbf, obf;
};
// Conv tile variants [42, 56) were the register-window conv tiles of round 4 (per launch on par with the DMA-staged
// conv_mfma_kernel tiles, 0.5 % slower per step; removed in round 5).  The index range stays RETIRED -- never a legal
// choice -- so that the in-workgroup split-K tiles keep their numbers (56 ..) and committed tuning tables stay valid.
#define WUN_FIRST_RETIRED_VARIANT 42
#define WUN_NUM_RETIRED_VARIANTS 14
// did the last launch_conv() on this thread write the fused upsampled copy?  (only split-K launches do)
int conv_last_fused_ups();
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// A kernel may take more than 64 KiB of dynamic LDS only once its attribute is raised.  `allowed` is the caller's high-water
// mark for `kernel` (a function-local static starting at 64 KiB): one runtime call per kernel and size.  Every launcher's.
static inline hipError_t raise_lds_limit(const void* kernel, size_t lds, size_t& allowed) {
    if (lds <= allowed) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) allowed = lds;
    return e;
}
// output side of a conv launch, shared by launch_conv and launch_conv_bf16: normalises acc_len == 0 to the whole row and
// sets F_VEC4 when every destination / mask row allows the 16-byte vector epilogue
void conv_output_setup(ConvArgs& a);

// Weight/bias gradient launch:  P[split][ (k*C + c)*N + n ] and bias row P[split][KW*C*N + n]
//   = sum over this split's (b, q-tile) units of in[b][c][q*SI + k - shift] * dz[b][n][q]
struct WgradArgs {
    const float* src0; const float* src1;
    long long bs0, bs1;
    int pitch0, pitch1;
    int off0, off1;
    int C0, C1;
    int Tin;
    int shift;
    int KW;
    int loader;      // DIRECT (SI = 1) / DEINT (SI = 2)
    const float* dz; long long dzbs; int dzpitch; int N; int Tq;
    float* out;      // direct: final [K][Cin][Cout](+bias row) block; else base of the tile-major split partials
    int direct;      // 1: single split, write the final layout
    int split_base;  // index of this launch's first split in the partial buffer
    int nsplit; int units_per_split; int nQT; int B;
    int ablate;      // debugging switches (only read when built with -DWUN_ABLATION)
    int force_mtw, force_nw;   // autotuner: geometry overrides (0 = heuristic)
    int bf16;        // speed mode: operands rounded to bf16 in LDS, v_mfma_f32_16x16x32_bf16 (wun_wgrad_bf16.hip)
    int win;         // exact fp32, register-window form (wun_wgrad_win.hip) instead of the LDS-tiled wgrad_mfma_kernel
    int sbf;         // bf16 kernel: src0 / src1 AND dz point at bf16 elements (pitches / strides / offsets in elements)
    int accum;       // final stores ADD to what the gradient arena holds (wun_*backward_accumulate): the launchers pick the
                     // accumulating instantiations (direct epilogue and split reduction); the kernels never read this field
};
// canonical layout the LDS-tiled and bf16 weight-gradient kernels stage from: 16-byte aligned rows of >= 4 elements
static inline bool wgrad_rows_aligned(const WgradArgs& a) {
    if ((a.pitch0 & 3) || (a.bs0 & 3) || !aligned16(a.src0) || a.pitch0 < 4) return false;
    if (a.C1 > 0 && ((a.pitch1 & 3) || (a.bs1 & 3) || !aligned16(a.src1) || a.pitch1 < 4)) return false;
    return !((a.dzpitch & 3) || (a.dzbs & 3) || !aligned16(a.dz) || a.dzpitch < 4);
}
// What the three MFMA weight-gradient launchers derive from the caller's split count: units of TK positions per split, the
// accumulating instantiation (only a single-split launch stores final values; split launches write partials with the plain
// kernel), the grid.  nsplit 0 = not picked yet -- the *_launch_ok questions come before the pick -- and is not divided by.
struct WgradSplit { int nQT, units_per_split; bool acc; long long grid; };
static inline WgradSplit wgrad_split(const WgradArgs& a, int TK, long long tiles) {
    WgradSplit sp;
    sp.nQT = (a.Tq + TK - 1) / TK;
    const int ns = a.nsplit > 0 ? a.nsplit : 1;
    sp.units_per_split = (int)(((long long)a.B * sp.nQT + ns - 1) / ns);
    sp.acc = a.accum && a.direct;
    sp.grid = tiles * a.nsplit;
    return sp;
}

// tile geometry of an exact-fp32 weight-gradient launch
struct WgradGeom { int MTW, NW, nMG, nNG, TK, XP, ZP, nChMax, ONESP, XW4; size_t lds; };
WgradGeom wgrad_geom(const WgradArgs& a);
// register-window weight gradient (wun_wgrad_win.hip; WgradArgs.win): aligned 16-byte operand reads, DMA staging,
// split partials in the final layout
bool wgrad_win_supported(const WgradArgs& a);
long long wgrad_win_partial_floats(const WgradArgs& a, const WunSwitches& sw);
int wgrad_win_units(const WgradArgs& a, const WunSwitches& sw);
int wgrad_win_tiles(const WgradArgs& a, const WunSwitches& sw);
hipError_t launch_wgrad_win(const WgradArgs& a, hipStream_t s, const WunSwitches& sw);
hipError_t launch_wgrad_win_reduce(const WgradArgs& a, const float* partial, int nsplit, float* out_w, float* out_b,
                                   hipStream_t s, const WunSwitches& sw);
// bf16 speed mode (wun_wgrad_bf16.hip): own tiling -- MFMA rows = 16 input channels of one tap; a workgroup holds
// 4*MTW slots = NCB channel blocks x KW taps + the bias slot
struct WgradBfGeom { int MTW, NW, NCB, nCB, nMG, nNG, TK, XW4, XROWS, ZPe; size_t lds; };
bool wgrad_bf16_supported(const WgradArgs& a);
WgradBfGeom wgrad_bf16_geom(const WgradArgs& a);
hipError_t launch_wgrad_bf16(const WgradArgs& a, hipStream_t s);
hipError_t launch_wgrad_bf16_reduce(const WgradArgs& a, const float* partial, int nsplit, float* out_w, float* out_b,
                                    hipStream_t s);

// Narrow weight gradient (wun_narrow.hip): audio-input conv / output head.  Input = virtual concat of two
// NCW sources as in WgradArgs; dz row n = (s, c), s = n / Nper, at dz + s*zss + b*dzbs + c*dzpitch.
struct NarrowWgradArgs {
    const float* src0; const float* src1;
    long long bs0, bs1;
    int pitch0, pitch1, off0, off1, C0, C1;
    int Tin, shift, KW, stride;
    const float* dz; long long zss, dzbs; int dzpitch;
    int N, Nper, Tq, B;
    float* partial;      // [splits][(KW*Ctot + 1) * N]
    int split_base, nsplit, units_per_split, nQT;
    int et;              // element types: bit 0 src0, bit 1 src1, bit 2 dz stored as bf16 (geometry in elements)
    int nrow0;           // streaming form: first dz row of this launch (set by the launcher)
};

struct ConvChoice { int variant; int ksplit; };
// bf16 conv (wun_bf16.hip): tile choices share the tuning tables with the fp32 variants, offset by kBf16VariantBase
static const int kBf16VariantBase = 1000;
bool conv_bf16_choice_ok(const ConvArgs& a, int variant);
int conv_bf16_list_candidates(const ConvArgs& a, ConvChoice* out, int maxn);
struct WgradChoice { int mtw, nw, nsplit[2]; };   // per layer: shared tile geometry, split count per part

struct UpsampleArgs {
    const float* x; long long xbs; int xpitch; int n;     // [B][C][n]
    float* y; long long ybs; int ypitch; int tup;          // [B][C][tup]
    const float* w;                                        // interp weights [C] or null (linear)
    int C; int B; int context;
    int bf;                                                // x and y hold bf16 elements
};

struct UpsampleBwdArgs {
    const float* dy; long long ybs; int ypitch; int tup;   // gradient wrt upsampled tensor
    const float* x; long long xbs; int xpitch; int n;      // forward input (post-activation)
    float* dz;                                             // out: dL/d(pre-activation of x), geometry of x
    const float* w; float* dw;                             // interp weights / their gradient (or null)
    float* dw_partial;                                     // [B][C] scratch of the two-stage interp-weight gradient (or null: one workgroup per channel)
    int C; int B; int context;
    int bf;                                                // dy, x and dz hold bf16 elements
};

struct HeadArgs {
    const float* mix_ncw; long long mbs; int mpitch; int moff_feat; int moff_diff; // crop offsets
    const float* feat; long long fbs; int fpitch;          // last up-conv output [B][F][Tfeat]
    const float* Wh;                                       // head params: per source {kernel [Ko][C+F][C], bias [C]}
    int C, F, S, Sh, Ko, padl;
    int Tfeat, Tout, B;
    int tanh_act, difference, training;
    float* out;                                            // [S][B][Tout][C]
    // backward only
    const float* tgt;                                      // [S][B][Tout][C]
    float* dpre; long long dps; long long dpbs; int dppitch; // [Sh][B][C][ToutP]
    float* dzfeat;                                         // geometry of feat
    float* loss_partial;                                   // [gridDim.x]
    float gscale;                                          // 2 / (S*B*Tout*C)
    int featbf;                                            // feat and dzfeat hold bf16 elements (fbs / fpitch in elements)
    const float* dout;                                     // wun_backward: dL/d outputs [S][B][Tout][C] (instead of tgt)
};

// Gradient of the loss w.r.t. the mix (wun_backward, wun_narrow.hip): dmix[b][t][c] = the transposed conv of down conv 0's
// d(pre-activation) (up to two parts, each the geometry of one forward launch of that conv:
//   z[b][n][q] = sum_{k,c} W[k][c][n] * x[b][c][off0 + stride*q + k - shift],  0 <= stride*q + k - shift < Tin)
// + the head's transposed conv of dpre over the mix-channel rows of every source's output kernel (OutputLayer.py:8,15)
// + dlast inside the difference crop (OutputLayer.py:20).  Every element written once; 0 where nothing reads the mix.
struct MixGradPart { const float* dz; long long dzbs; int dzpitch; int Tq, stride, off0, shift, Tin; };
struct MixGradArgs {
    MixGradPart part[2]; int nparts;
    int dzbf;                                              // the parts' dz rows hold bf16 elements (strides in elements)
    const float* W; int KW, F;                             // down conv 0 kernel [KW][C][F]
    int C, B, Tin;
    const float* dpre; long long dps, dpbs; int dppitch;   // head: [Sh][B][C][pitch]
    const float* Wh; long long hoff[4]; int Sh, Ko, padl, Tfeat, Tout, moff_feat;
    const float* dlast; int moff_diff;                     // difference output: dL/d out[S-1] [B][Tout][C], or null
    float* dmix;                                           // [B][Tin][C]
};

// bf16 mode: one conv's weights, fp32 [KW][C][N] (from the parameter arena or a transposed copy in
// the workspace) -> packed bf16 image [KW][C8p][Npad][8] in the workspace
struct PackDesc {
    long long src_off;   // floats, into params (src_in_ws = 0) or the workspace (1)
    long long dst_off;   // floats, into the workspace (the image holds KW*C8p*Npad*8 bf16 = half as many floats)
    int KW, C, N, C8p, Npad;
    int src_in_ws;
};

struct WtDesc {      // mode 0: dst[j][n][c] = src[k_last - j*k_step][c][n]
                     // mode 1: dst[j][n][p][c] = src[k_last - 2j + p][c][n] (0 if tap >= k_step (= KW))
    long long src_off;   // into params
    long long dst_off;   // into workspace
    int J, C, N, k_last, k_step;
    int mode;
};

// ---- launchers (wun_kernels.hip) ---------------------------------------------------
// Every launcher family below resolves a launch in ONE host function of its unit (conv_resolve, conv_bf16_resolve,
// wgrad_resolve, wgrad_win_resolve, wgrad_bf16_resolve, narrow_wgrad_resolve): args -> instantiation, geometry, split, LDS
// bytes and grid, or a refusal.  launch_* launches the result; the host-only *_ok questions are "it resolved" (for the convs:
// within the tuner's limits), so neither can accept what the other computes differently.
int  conv_pick_variant(const ConvArgs& a);
hipError_t launch_conv(const ConvArgs& a, float* part, long long part_cap, hipStream_t s, const WunSwitches& sw);
double conv_flops(const ConvArgs& a);        // useful FLOPs (2*MACs) of the launch
long long conv_natural_wgs_phase2(const ConvArgs& a);
int conv_list_candidates(const ConvArgs& a, long long part_cap, ConvChoice* out, int maxn, const WunSwitches& sw);
bool conv_choice_ok(const ConvArgs& a, long long part_cap, int variant, int ksplit, const WunSwitches& sw);
int conv_num_variants();
int wgrad_max_units(const WgradArgs& a, const WunSwitches& sw);

int  wgrad_pick_nsplit(const WgradArgs& a, const WunSwitches& sw);
hipError_t launch_wgrad(const WgradArgs& a, hipStream_t s, const WunSwitches& sw);
// host only: would launch_wgrad accept `a` (family by a.bf16 / a.win; pointers, shape, resolved geometry)?  The family's
// resolve step without the launch, asked before any GPU work (wun_op_wgrad_ex); a.nsplit need not be set yet.
bool wgrad_launch_ok(const WgradArgs& a, const WunSwitches& sw);
bool wgrad_bf16_launch_ok(const WgradArgs& a);
bool wgrad_win_launch_ok(const WgradArgs& a, const WunSwitches& sw);
void wgrad_resolved_geom(const WgradArgs& a, int& mtw, int& nw);
long long wgrad_partial_floats(const WgradArgs& a, const WunSwitches& sw);
hipError_t launch_wgrad_reduce(const WgradArgs& a, const float* partial, int nsplit, float* out_w, float* out_b,
                               hipStream_t s, const WunSwitches& sw);
// Which form the last launch of an elementwise operator took on this thread (wun_op_last_path): the host launchers of
// wun_elementwise.hip record it, because one ProfScope name covers every form of an operator.  Values = the WUN_PATH_* of
// include/wun.h; 0 before the first launch.
enum { EW_UPSAMPLE = 0, EW_UPSAMPLE_BWD, EW_INTERP_GRAD, EW_HEAD_FWD, EW_HEAD_DFEAT, EW_BTC_TO_NCW, EW_NUM_OPS };
enum { EW_PATH_NONE = 0, EW_PATH_SCALAR, EW_PATH_VEC4, EW_PATH_VEC8_BF16, EW_PATH_ONE_STAGE, EW_PATH_TWO_STAGE,
       EW_PATH_GENERIC, EW_PATH_FOUR_POSITION };
int elementwise_last_path(int op);
hipError_t launch_upsample(const UpsampleArgs& a, hipStream_t s);
hipError_t launch_upsample_bwd(const UpsampleBwdArgs& a, hipStream_t s);
hipError_t launch_interp_grad(const UpsampleBwdArgs& a, hipStream_t s, bool accum = false);   // dw of the learned interpolation weights
hipError_t launch_head_fwd_off(const HeadArgs& a, const long long* hoff, hipStream_t s);
int head_bwd_blocks(const HeadArgs& a);
hipError_t launch_head_bwd_off(const HeadArgs& a, const long long* hoff, hipStream_t s);
hipError_t launch_head_grad_off(const HeadArgs& a, const long long* hoff, hipStream_t s);   // dpre from a.dout, then d(feature map)
hipError_t launch_loss_finish(const float* partial, int n, float scale, float* loss, hipStream_t s);
hipError_t launch_btc_to_ncw(const float* src, float* dst, int B, int T, int C, int pitch,
                             hipStream_t s);
// ---- track windows (wun_track.hip): the mix rows of a forward pass read straight from a [track_frames, C] track, and the
// estimates of a batch of hops written straight into [S, pred_frames, C] ----
// Row b < npos of the batch is track[pos[b] .. pos[b] + Tin) (frames; host table, every window checked against the track by
// the caller); rows >= npos are zeros.
struct MixWindows { const float* track; const int64_t* pos; int npos; };
// what launch_btc_to_ncw writes for the materialised batch: the same floats at the same NCW elements (dst 16-byte aligned,
// pitch a multiple of 4 floats; the floats of a row's last quad beyond T -- row padding nothing reads -- are written as 0)
hipError_t launch_gather_windows(const MixWindows& w, float* dst, int B, int T, int C, int pitch, hipStream_t s);
// One run of frames of one hop: preds[s][dst .. dst + len) = outputs[s][row][src .. src + len) for every source s (frames)
struct ScatterSeg { long long dst; int row, src, len; };
hipError_t launch_scatter_segments(const float* outputs, float* preds, const ScatterSeg* segs, int nsegs, int S, int B,
                                   int Tout, int C, long long pred_frames, hipStream_t s);
// One run of frames with a constant covering set, and up to WUN_BLEND_COVER of its covering rows in ascending window order:
// for every frame f of [dst, dst + len), source s and channel c, j = 0 .. n - 1 in turn
//   preds[s][f][c] = fmaf(w_j(t0[j] + f - dst), outputs[s][row[j]][t0[j] + f - dst][c], preds[s][f][c]);  den[f] += w_j(..)
// meta: bits 0-2 = n, bits 4 + 2j / 5 + 2j = WUN_BLEND_NO_RISE / WUN_BLEND_NO_FALL of cover j.  A covering set larger than the
// cap is cut into successive pieces of the same run, launched one after the other on the stream.
#define WUN_BLEND_COVER 4
struct BlendRun { long long dst; int len; unsigned meta; int row[WUN_BLEND_COVER]; int t0[WUN_BLEND_COVER]; };
hipError_t launch_blend_runs(const float* outputs, float* preds, float* den, const BlendRun* runs, int nruns, int S, int B,
                             int Tout, int C, int overlap, long long pred_frames, hipStream_t s);
// preds[s][f][c] = den[f] != 0 ? preds[s][f][c] / den[f] : +0
hipError_t launch_blend_finish(float* preds, const float* den, int S, long long pred_frames, int C, hipStream_t s);
hipError_t launch_make_wt(const float* params, float* ws, const WtDesc* dev_descs, int ndesc,
                          int max_elems, hipStream_t s);
// Runs of consecutive arena floats, passed by value to the optimizer's kernels: run k = floats [off[k], off[k] + cum[k+1] - cum[k])
#define WUN_ADAM_RANGES 32
struct AdamRanges { long long off[WUN_ADAM_RANGES]; long long cum[WUN_ADAM_RANGES + 1]; int n; };
// Gradient norm (wun_grad_norm): the arena cut into chunks of at most WUN_NORM_CHUNK floats that never cross a tensor
// boundary (plan-owned device table, chunks of tensor k = [first[k], first[k+1])); one float64 sum of squares per chunk,
// then per tensor and over the selected tensors, in a fixed order (no atomics: bitwise reproducible, grid-independent).
#define WUN_NORM_CHUNK 8192
#define WUN_NORM_MAX_TENSORS 256
struct NormChunk { long long off; int len; int tensor; };
struct NormSelect { unsigned bits[WUN_NORM_MAX_TENSORS / 32]; };       // by value: bit k = tensor k selected
hipError_t launch_grad_norm(const float* g, const NormChunk* chunks, const int* first, int nchunks, int ntensors,
                            const NormSelect& sel, long long nfloats, float gscale, float* norms, double* partial,
                            hipStream_t s);
// The optimizer step over runs (every Adam entry, wun_optim_step, wun_spec_adam_step): gi = g * gscale, times clip / N when the
// global norm N = *gnorm (device) > clip; m and v by TF-Adam; theta times wdf first in the runs whose bit of `decay` is set,
// then the step of size lr_t; ema (may be null) -= emaw * (ema - new theta).  skip != 0 and N not finite: nothing written,
// *skipped += 1 (when non-null) by one lane.  gnorm null: no clip prologue (nothing clips, nothing skips).  vec: the arenas
// share one alignment modulo 16 bytes (same_alignment), so the 16-byte path may run; the bits are the scalar path's.
float adam_lr_t(int64_t step, float lr, float beta1, float beta2);      // TF-Adam's step size (wun_optim.hip)
static inline bool same_alignment(std::initializer_list<const void*> ptrs) {       // null pointers do not count
    uintptr_t a = 0;
    bool have = false;
    for (const void* q : ptrs) {
        if (!q) continue;
        const uintptr_t x = reinterpret_cast<uintptr_t>(q) & 15;
        if (have && x != a) return false;
        a = x; have = true;
    }
    return true;
}
struct OptimArgs {
    float* p; const float* g; float* m; float* v; float* ema;
    float lr_t, b1, b2, eps, gscale, wdf, emaw;
    const float* gnorm; float clip; int skip; long long* skipped;
    unsigned decay; int vec;
};
hipError_t launch_optim_ranges(const OptimArgs& a, const AdamRanges& r, hipStream_t s);
// the EMA line alone over selected runs (wun_ema_update)
hipError_t launch_ema_ranges(float* ema, const float* p, float emaw, int vec, const AdamRanges& r, hipStream_t s);
hipError_t launch_fill(float* p, long long n, float val, hipStream_t s);
hipError_t launch_mfma_probe(const float* a, const float* b, float* d, hipStream_t s);
void prof_begin(bool detail);                 // detail: per-launch list in the JSON (WUN_PROFILE_DETAIL)
std::string prof_end();
void prof_scope_begin(const char* name, double flops, hipStream_t s, const char* tag, double bytes = 0.0);   // HIP-event bracket of the next launch (bytes: algorithmic HBM bytes of a bandwidth-bound launch)
void prof_scope_end(hipStream_t s);

// ---- narrow weight gradients (wun_narrow.hip) ----
bool narrow_wgrad_supported(const NarrowWgradArgs& a);
bool narrow_wgrad_uses_lds(const NarrowWgradArgs& a, const WunSwitches& sw);      // the LDS-staged kernel (else the streaming form)
int narrow_wgrad_units(const NarrowWgradArgs& a);
int narrow_wgrad_pick_nsplit(const NarrowWgradArgs& a, const WunSwitches& sw);
long long narrow_wgrad_partial_floats(const NarrowWgradArgs& a);
hipError_t launch_narrow_wgrad(NarrowWgradArgs a, hipStream_t s, const WunSwitches& sw);
bool narrow_wgrad_launch_ok(const NarrowWgradArgs& a, const WunSwitches& sw);      // host only: would launch_narrow_wgrad accept `a`?
hipError_t launch_narrow_wgrad_reduce(const NarrowWgradArgs& a, const float* partial, int nsplit, float* grads,
                                      const long long* woff, const long long* boff, hipStream_t s, bool accum = false);
size_t mix_grad_lds_bytes(const MixGradArgs& a);
hipError_t launch_mix_grad(const MixGradArgs& a, hipStream_t s);

// ---- bf16-MFMA speed mode (wun_bf16.hip) ----
// 8-channel groups of a packed bf16 weight image for C input channels: the conv kernel reads whole stages of
// 4, 8 or 12 groups (1..3 chunks of 32 channels), so the image is zero-padded to the next multiple of each
static inline int bf16_image_groups(int C) {
    const int g = (C + 7) / 8;
    int best = 0;
    for (int m = 4; m <= 12; m += 4) { const int r = (g + m - 1) / m * m; best = r > best ? r : best; }
    return best;
}
bool conv_bf16_supported(const ConvArgs& a);
hipError_t launch_conv_bf16(const ConvArgs& a, hipStream_t s, const WunSwitches& sw);
bool first_conv_supported(const ConvArgs& a);
hipError_t launch_first_conv(const ConvArgs& a, hipStream_t s);                 // audio-input conv of the bf16 mode
hipError_t launch_cast_rows_bf16(const float* src, void* dst, long long rows, int T, long long spitch, long long dpitch, hipStream_t s);
hipError_t launch_pack_bf16(const float* params, float* ws, const PackDesc* dev_descs, int ndesc, long long max_items,
                            hipStream_t s);
hipError_t launch_mfma_bf16_probe(const float* a, const float* b, float* d, hipStream_t s);

}  // namespace wun
