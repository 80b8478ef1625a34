// Internal: the plan object (struct wun_plan) and the host helpers its units share -- wun_plan.hip (builder, queries),
// wun_dispatch.hip (argument blocks, streams, autotuned dispatch), the training step by pass -- wun_forward.hip (forward),
// wun_backward.hip (loss + backward), wun_optim.hip (Adam, gradient norm) --, wun_tune.hip (tuner, tuning tables),
// wun_op.hip (single-operator entry points).  Host code only.
#pragma once
#include "../../include/wun.h"
#include "wun_internal.h"

#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace wun;

// A workspace tensor [B][C][pitch] of fp32 (eb = 4) or bf16 (eb = 2: the activations and their gradients of the bf16
// mode) elements; `off` is in FLOATS from the workspace base, pitch and bs are in ELEMENTS; rows are 16-byte aligned.
struct Buf { long long off = -1; int C = 0; int T = 0; int pitch = 0; long long bs = 0; int eb = 4; };
struct ConvLayer { long long woff = 0, boff = 0; int KW = 0, Cin = 0, Cout = 0;
                   long long wt_full = -1, wt_ph[2] = {-1, -1}, wt_ph2 = -1; int Jp[2] = {0, 0}; int J0 = 0;
                   // dedup plans: the two-phase image of the filter SHIFTED by one tap (W''[k + 1] = W[k], W''[0] = 0), for the
                   // odd-window input gradient: its outputs start at an odd row position; with the shifted filter the launch
                   // starts one position earlier, on a 16-byte boundary, and takes the vector epilogue
                   long long wt_ph2s = -1; int J0s = 0; };
// tc / cs: length / start of the centre crop the skip connection takes (Utils.py:104-123), in conv-output positions.
// Round 6 (dedup plans): the crop window split by the parity of the ABSOLUTE conv position -- even positions are elements
// of the decimated stream (computed once, by the stride-2 launch), odd positions get their own stride-2 launches:
// t_ev0 / n_even, t_odd0 / n_odd = first position and count of each parity inside [cs, cs + tc).
struct DownShape { int cin, cout, t_in, t_conv, t_dec, tc, cs, t_ev0, n_even, t_odd0, n_odd; };
struct UpShape { int c_skip, c_cur, cout, t_cur, t_up, t_conv, crop_start; };

struct wun_plan {
    wun_config cfg;
    WunSwitches sw;                             // environment switches, read once at wun_plan_create
    WunEarlyWindow early_window = EW_DEEP;      // sw.early_window resolved against the plan's default (all on dedup plans)
    bool fuse_ups = false;                      // fused (adjoint) upsampling in the split-K epilogues (fp32 mode, !WUN_NO_FUSE_UPS)
    int B = 0, Tin = 0, Tout = 0;
    int L = 0, C = 0, S = 0, Sh = 0;
    bool same = false;
    std::vector<wun_tensor_info> tensors;
    long long arena = 0, ws = 0;
    std::vector<DownShape> dsh;
    std::vector<UpShape> ush;
    int t_b_in = 0, t_b = 0, c_b = 0;
    int t_feat = 0, in_crop_start = 0, mix_diff_off = 0;
    std::vector<ConvLayer> down, up, head;
    ConvLayer bott;
    std::vector<long long> interp;
    Buf mix_ncw, bott_out, dz_bott;
    // bf16 mode, output layer too wide for ONE narrow weight-gradient launch ((C + F) * Sh * C > 256: the deep variant):
    // its weight gradient runs on the bf16 MFMA kernel, which reads bf16 rows only -- bf16 copies of the audio (made in the
    // forward pass) and of the head's d(pre-activation) (made after head_bwd_kernel); both are a few rows
    bool head16 = false;
    Buf mix16;
    long long dpre16_off = -1; int dp16_pitch = 0;
    std::vector<Buf> dec, skip, ups, upo, dz_dec, dz_skip, d_ups, dz_upo;
    // Round 6, context plans of the exact-fp32 mode ("dedup"): the reference's decimated stream is a SLICE of the encoder
    // output (UnetAudioSeparator.py:98-100: one tensor, one rounding).  The stride-2 launch of a down level writes its
    // outputs into dec[i] AND into the even positions of the skip window; a second stride-2 launch computes only the odd
    // window positions (rounds 1 - 5 ran a stride-1 conv over the whole window: every even window position was computed
    // twice, 7.8 % of the step's FLOPs).  Backward: an up level's input gradient splits the window's gradient by parity --
    // even part stored into dz_dec[i] (the transposed conv that fills the rest of dz_dec[i] later ADDS inside that range),
    // odd part compact in dz_odd[i] -- and the window's input gradient / weight gradient run over the odd positions only.
    bool dedup = false;
    std::vector<Buf> dz_odd;
    long long dpre_off = -1; int dp_pitch = 0;
    long long partial_off = -1, partial_floats = 0;
    long long loss_partial_off = -1;
    std::vector<long long> interp_partial_off;
    long long conv_part_off = -1, conv_part_floats = 0;
    std::vector<WtDesc> wt;
    WtDesc* dev_wt = nullptr;
    int wt_max = 0;
    double fwd_flops = 0, bwd_flops = 0, fwd_dense = 0, fwd_unique = 0, bwd_unique = 0;
    // second HIP stream: independent launches (weight gradients vs the input-gradient chain;
    // skip-window convs vs the decimating convs) run concurrently so that one kernel's tail and
    // epilogue overlap another kernel's MFMA phase
    // autotuner state: per-launch choices in launch order (forward / backward), filled by wun_plan_tune
    mutable int tune_mode = 0;                  // 0 = heuristics, 1 = measuring, 2 = tuned
    mutable std::vector<ConvChoice> conv_fwd, conv_bwd;
    mutable std::vector<WgradChoice> wg_bwd;
    mutable size_t ci = 0, wi = 0;
    mutable bool in_bwd = false;
    mutable hipEvent_t tev0 = nullptr, tev1 = nullptr;
    mutable hipStream_t side = nullptr, side2 = nullptr;
    mutable std::vector<hipEvent_t> events;
    mutable size_t ev_next = 0;
    // transposed weight copies for the input-gradient convs: produced on the side stream during the
    // forward pass (training mode) so that the backward pass does not start with a 50 us transpose
    mutable hipEvent_t wt_ev = nullptr;
    mutable bool wt_ready = false;
    mutable std::vector<hipEvent_t> skip_ev;             // forward: skip window i is complete (deferred window convs)
    mutable std::vector<hipEvent_t> win_ev;              // backward: the early skip-window input gradient of level i is complete
    // bf16-MFMA speed mode (cfg.compute_dtype == 1): packed bf16 images of the conv weights in the
    // workspace, keyed by where the fp32 weights of a launch live (params arena / transposed copy in ws)
    struct BfImg { long long off; int c8p, npad; };
    bool bf16 = false;
    std::map<std::pair<int, long long>, BfImg> bf_img;       // (1 = in workspace, float offset) -> image
    std::vector<PackDesc> pack;                              // forward images first, then the dgrad images
    int npack_fwd = 0;
    long long pack_max = 0;
    PackDesc* dev_pack = nullptr;
    // wun_grad_norm: the chunk -> tensor map (host copy and device table: chunks, then num_tensors + 1 first-chunk indices)
    std::vector<NormChunk> norm_chunks;
    std::vector<int> norm_first;
    NormChunk* dev_norm_chunks = nullptr;
    int* dev_norm_first = nullptr;
    mutable const float* cur_params = nullptr;
    mutable const float* cur_ws = nullptr;
};

// The forward conv of down level i as its one or two launch geometries over the level's input x ("parts"):
//   z[q] = sum_k W[k] x[off + stride * q + k - shift]   (0 <= stride * q + k - shift < Tin, q < Tq),
// and `dz`, where the backward pass keeps that part's d(pre-activation).  'same' plans: the one full-rate conv.  Context plans:
// part 0 = the stride-2 conv into the decimated stream; part 1 = the rest of the skip window -- dedup plans: its odd positions
// (a second stride-2 conv over x shifted by t_odd0 samples; none when the window holds no odd position), else the full-rate
// conv over the whole window (its even positions are computed a second time, both contributions add in the backward pass).
// The level's weight gradient (MFMA and narrow form), the mix gradient and the forward window conv are all built from this.
struct DownPart { int off, Tin, shift, stride, loader; const Buf* dz; int Tq; };
// returns the number of parts that launch; on context plans out[1] is filled even when it does not
inline int down_parts(const wun_plan* p, int i, DownPart out[2]) {
    const DownShape& d = p->dsh[i];
    const int Kd = p->cfg.filter_size;
    if (p->same) {
        out[0] = DownPart{0, d.t_in, (Kd - 1) / 2, 1, LOADER_DIRECT, &p->dz_skip[i], d.t_conv};
        return 1;
    }
    out[0] = DownPart{0, d.t_in, 0, 2, LOADER_DEINT, &p->dz_dec[i], d.t_dec};
    if (p->dedup) {
        out[1] = DownPart{d.t_odd0, d.t_in - d.t_odd0, 0, 2, LOADER_DEINT, &p->dz_odd[i], d.n_odd};
        return d.n_odd > 0 ? 2 : 1;
    }
    out[1] = DownPart{d.cs, d.tc + Kd - 1, 0, 1, LOADER_DIRECT, &p->dz_skip[i], d.tc};
    return 2;
}

// ---- shared host state and helpers ----
extern thread_local std::string g_err;   // wun_last_error()
extern bool g_profiling;                 // while wun_profile_* is active everything runs on the caller's stream
int fail(int code, const std::string& msg);

// select / nselect of the wun_*_select entries: one byte per tensor (wun_plan_tensor order), or NULL = every tensor
inline int check_nselect(const wun_plan* p, const uint8_t* select, int64_t nselect) {
    const int64_t nt = (int64_t)p->tensors.size();
    if (!select && nselect != 0 && nselect != nt) return fail(WUN_ERR_INVALID, "nselect must be 0 or num_tensors when select is NULL");
    if (select && nselect != nt) return fail(WUN_ERR_INVALID, "nselect must equal num_tensors");
    return WUN_OK;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess)                                                                 \
            return fail(WUN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));      \
    } while (0)

inline WgradArgs wgrad_shape_only(int B, int C0, int C1, int KW, int loader, int N, int Tq) {
    WgradArgs w;
    memset(&w, 0, sizeof(w));
    w.B = B; w.C0 = C0; w.C1 = C1; w.KW = KW; w.loader = loader; w.N = N; w.Tq = Tq;
    return w;
}

// wun_forward.hip: the forward pass behind wun_forward (win == nullptr: rows from mix_btc) and wun_forward_windows
int forward_pass(const wun_plan* p, const float* params, const float* mix_btc, const MixWindows* win, float* ws,
                 float* outputs, int training, hipStream_t s);

// wun_dispatch.hip
ConvArgs conv_base(const wun_plan* p);
void set_src0(ConvArgs& a, const float* ws, const Buf& b, int off, int C);
void set_src1(ConvArgs& a, const float* ws, const Buf& b, int off, int C);
void set_dst0(ConvArgs& a, float* ws, const Buf& b, int off, const Buf* mask);
void set_dst1(ConvArgs& a, float* ws, const Buf& b, int off, const Buf* mask);
WgradArgs wgrad_base(const wun_plan* p);
void wset_src0(WgradArgs& a, const float* ws, const Buf& b, int off, int C);
void wset_src1(WgradArgs& a, const float* ws, const Buf& b, int off, int C);
void wset_dz(WgradArgs& a, const float* base, long long bs, int pitch, int N, int Tq);
HeadArgs head_args(const wun_plan* p, const float* params, float* ws, float* outputs, int training);
unsigned event_flags(const wun_plan* p);
int side_init(const wun_plan* p);
int stream_dep(const wun_plan* p, hipStream_t from, hipStream_t to);
hipError_t conv_dispatch(const wun_plan* p, ConvArgs a, float* part, long long cap, hipStream_t s, long long at = -1);
// forces (mtw, nw) on every part; false if the parts do not resolve to one tile geometry (run_wgrad, wun_op_wgrad_ex)
bool wgrad_common_geom(WgradArgs* parts, int nparts, int mtw, int nw);
// accum: the final stores add to `grads` (wun_*backward_accumulate); same launches, tilings and split counts
int run_wgrad(const wun_plan* p, WgradArgs* parts, int nparts, const ConvLayer& cl, float* ws, float* grads,
              hipStream_t main, hipStream_t s, bool dep = true, bool accum = false);
int run_narrow_wgrad(const wun_plan* p, NarrowWgradArgs* parts, int nparts, const long long* woff, const long long* boff,
                     float* ws, float* grads, hipStream_t main, hipStream_t s, bool accum = false);
