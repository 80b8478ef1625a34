// Host side of libwun.so: static plan (the equivalent of the reference building its TF
// graph once, /root/reference/Training.py:47) -- shape solver, builder, queries -- the environment switches, the
// profiler and the remaining C ABI entries of include/wun.h (the other host units: wun_plan_impl.h).
#include "wun_plan_impl.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

thread_local std::string g_err;
bool g_profiling = false;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// The one place the library reads its environment (the fields and their parses: struct WunSwitches, wun_internal.h).
WunSwitches wun::wun_switches_from_env() {
    WunSwitches w;
    auto set = [](const char* name) { return getenv(name) != nullptr; };
    auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
    w.no_dedup = set("WUN_NO_DEDUP");
    if (const char* e = getenv("WUN_EARLY_WINDOW")) w.early_window = e[0] == '0' ? EW_OFF : e[0] == 'a' ? EW_ALL : EW_DEEP;
    w.odd_fuse_set = set("WUN_ODD_FUSE_MIN");
    w.odd_fuse_min = num("WUN_ODD_FUSE_MIN", 64);
    w.no_odd_align = set("WUN_NO_ODD_ALIGN");
    w.no_fuse_ups = set("WUN_NO_FUSE_UPS");
    w.bf16_head_serial = set("WUN_BF16_HEAD_SERIAL");
    w.single_stream = set("WUN_SINGLE_STREAM");
    if (const char* e = getenv("WUN_SIDE_PRIO")) w.side_prio = e[0] == 'l' ? PRIO_LOW : e[0] == 'h' ? PRIO_HIGH : PRIO_NORMAL;
    if (const char* e = getenv("WUN_EVENT_SCOPE")) w.event_scope = e[0] == 's' ? EV_SYSTEM : e[0] == 'd' ? EV_DEVICE : EV_DEFAULT;
    w.no_win = set("WUN_NO_WIN");
    w.no_narrow = set("WUN_NO_NARROW");
    w.no_narrow_down0 = set("WUN_NO_NARROW_DOWN0");
    w.no_narrow_stream = num("WUN_NO_NARROW_STREAM", 0) != 0;
    if (set("WUN_NARROW_SPLITS")) w.narrow_splits = std::max(1, num("WUN_NARROW_SPLITS", 0));   // (a cap <= 1 means one split)
    w.no_dma = set("WUN_NO_DMA");
    w.no_k3 = num("WUN_NO_K3", 0) != 0;
    { const int v = num("WUN_WIN_TK", 64); if (v == 16 || v == 32 || v == 64 || v == 128) w.win_tk = v; }
    w.bf16_lds_cap = num("WUN_BF16_LDS_CAP", 80);
    w.tune_rounds = std::max(1, num("WUN_TUNE_ROUNDS", 4));
    w.tune_log = set("WUN_TUNE_LOG");
    if (const char* e = getenv("WUN_TUNE_ALTS")) w.tune_alts = e;
    { const int v = num("WUN_TUNE_ALTS_MAX", 6); w.tune_alts_max = v > 0 ? v : 6; }
    if (const char* e = getenv("WUN_TUNE_ALTS_TOL")) { const float v = (float)atof(e); w.tune_alts_tol = v > 1.f ? v : 1.15f; }
    w.dump_layout = set("WUN_DUMP_LAYOUT");
    w.profile_detail = set("WUN_PROFILE_DETAIL");
    w.win_occ = set("WUN_WIN_OCC");
    return w;
}

// ---------------------------------------------------------------------------------------
// shapes (UnetAudioSeparator.py:34-83, Utils.py:104-123)
// ---------------------------------------------------------------------------------------
static int check_config(const wun_config* c) {
    if (!c) return fail(WUN_ERR_INVALID, "config is null");
    if (c->num_layers < 1 || c->num_layers > 24) return fail(WUN_ERR_INVALID, "num_layers out of range");
    if (c->num_initial_filters < 1) return fail(WUN_ERR_INVALID, "num_initial_filters < 1");
    if (c->filter_size < 1 || c->merge_filter_size < 1 || c->output_filter_size < 1 || c->input_filter_size < 1)
        return fail(WUN_ERR_INVALID, "filter sizes must be >= 1");
    if (c->filter_size > 15 || c->merge_filter_size > 15)
        return fail(WUN_ERR_UNSUPPORTED, "filter_size / merge_filter_size > 15 not supported by the gfx950 kernels");
    if (c->upsampling != 0 && c->upsampling != 1) return fail(WUN_ERR_UNSUPPORTED, "upsampling must be linear|learned");
    if (c->output_type != 0 && c->output_type != 1) return fail(WUN_ERR_UNSUPPORTED, "output_type must be direct|difference");
    if (c->output_activation != 0 && c->output_activation != 1)
        return fail(WUN_ERR_UNSUPPORTED, "output_activation must be tanh|linear");   // UnetAudioSeparator.py:136
    if (c->num_channels != 1 && c->num_channels != 2) return fail(WUN_ERR_INVALID, "num_channels must be 1 or 2");
    if (c->num_sources < 1 || c->num_sources > 4) return fail(WUN_ERR_UNSUPPORTED, "num_sources must be 1..4");
    if (c->output_type == 1 && c->num_sources < 2) return fail(WUN_ERR_INVALID, "difference output needs >= 2 sources");
    if (c->compute_dtype != 0 && c->compute_dtype != 1) return fail(WUN_ERR_UNSUPPORTED, "compute_dtype must be 0 (f32) or 1 (bf16)");
    {
        // the head kernels keep every source's output filter in LDS (default 64 KiB dynamic limit)
        const long long sh = c->output_type == 0 ? c->num_sources : c->num_sources - 1;
        const long long cin = (long long)c->num_channels + c->num_initial_filters;
        const long long head_lds = 4 * sh * ((long long)c->output_filter_size * cin * c->num_channels + c->num_channels);
        if (head_lds > 64 * 1024)
            return fail(WUN_ERR_UNSUPPORTED, "output_filter_size x (num_channels + num_initial_filters) too large for the head kernels' LDS");
    }
    return WUN_OK;
}

extern "C" int wun_get_padding(const wun_config* cfg, int64_t desired, int64_t* in_frames, int64_t* out_frames) {
    int rc = check_config(cfg);
    if (rc) return rc;
    if (!in_frames || !out_frames) return fail(WUN_ERR_INVALID, "null output pointer");
    if (!cfg->context) { *in_frames = desired; *out_frames = desired; return WUN_OK; }   // :83
    double rem = (double)desired;                       // :43
    rem = rem - cfg->output_filter_size + 1;            // :46
    for (int i = 0; i < cfg->num_layers; ++i) {         // :49-51
        rem = rem + cfg->merge_filter_size - 1;
        rem = (rem + 1.0) / 2.0;
    }
    const int64_t x = (int64_t)std::ceil(rem);          // :54
    if (x < 2) return fail(WUN_ERR_INVALID, "get_padding: bottleneck feature map < 2 (reference assert)");
    int64_t out = x, inp = x + cfg->filter_size - 1;    // :58-62
    for (int i = 0; i < cfg->num_layers; ++i) {         // :65-73
        out = 2 * out - 1;
        out = out - cfg->merge_filter_size + 1;
        inp = 2 * inp - 1;
        inp += (i < cfg->num_layers - 1 ? cfg->filter_size : cfg->input_filter_size) - 1;
    }
    out = out - cfg->output_filter_size + 1;            // :76
    *in_frames = inp;
    *out_frames = out;
    return WUN_OK;
}

// ---------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------

static long long bump(long long& cur, long long n) {
    const long long off = (cur + 63) / 64 * 64;
    cur = off + n;
    return off;
}

static Buf make_buf(const WunSwitches& sw, long long& cur, int B, int C, int T, const char* name = nullptr, int idx = 0, int eb = 4) {
    Buf b;
    const int per16 = 16 / eb;                                        // elements per 16 bytes
    b.C = C; b.T = T; b.pitch = (T + per16 - 1) / per16 * per16; b.eb = eb;
    b.bs = (long long)C * b.pitch;
    b.off = bump(cur, ((long long)B * b.bs * eb + 3) / 4);
    if (name != nullptr && sw.dump_layout)      // (tools/ws_diff.py: workspace map for debugging)
        fprintf(stderr, "[wun-layout] %s %d off=%lld B=%d C=%d T=%d pitch=%d eb=%d\n", name, idx, b.off, B, C, T, b.pitch, eb);
    return b;
}

// Can this plan run the bf16 mode (compute_dtype = 1)?  Every conv from level 1 on must be served by the bf16 MFMA
// kernels -- the activations then live in HBM as bf16 and nothing but those kernels (and the element-type aware
// elementwise / head / audio-input kernels) reads them: channel counts in whole groups of 8 (num_initial_filters % 8 == 0;
// every shipped config: 24, the deep variant 48), no tap-less conv phase (a 1-tap filter with context), rows and tensors
// inside the kernels' 32-bit offsets.  A plan that does not qualify is the exact-fp32 plan (wun_plan_query reports it).
static bool bf16_plan_ok(const wun_config* c, int B, const std::vector<DownShape>& dsh, int t_b,
                         const std::vector<UpShape>& ush, int c_b, int Sh) {
    if ((c->num_initial_filters & 7) != 0) return false;
    if (c->context && (c->filter_size < 2)) return false;
    if (c->filter_size > 15 || c->merge_filter_size > 15 || c->output_filter_size > 15) return false;
    (void)B;
    // a row of `t` elements (+ halo) inside the kernels' 23-bit row elements, an excerpt's tensor inside 32-bit byte offsets
    auto fits = [](long long ch, long long t) { return t + 64 < (1ll << 23) && ch * ((t + 15) & ~7ll) * 2 < (1ll << 31); };
    for (const DownShape& d : dsh)
        if (!fits(d.cout, d.t_conv) || !fits(d.cin, d.t_in)) return false;
    if (!fits(c_b, t_b)) return false;
    // up path (these were only checked at launch): the two sources of an up conv -- skip window and upsampled
    // tensor, twice the channels of the down level at the same length --, its output and the gradient tensors of the same shapes
    for (const UpShape& u : ush) {
        if (!fits(u.c_skip, u.t_up) || !fits(u.c_cur, u.t_up) || !fits(u.cout, u.t_conv)) return false;
        if ((u.c_skip & 7) != 0) return false;                  // an 8-channel group must not straddle the two sources
    }
    // output head: the narrow weight-gradient kernels (all sources in one launch, or one launch per source), or -- even
    // channel counts -- the bf16 MFMA weight gradient on bf16 copies of the audio and the head's d(pre-activation)
    if (Sh > 0) {
        const int C = c->num_channels, F = c->num_initial_filters;
        NarrowWgradArgs t;
        memset(&t, 0, sizeof(t));
        t.C0 = C; t.C1 = F; t.KW = c->output_filter_size; t.stride = 1; t.N = Sh * C; t.Nper = C;
        bool ok = narrow_wgrad_supported(t);
        if (!ok && (C & 1) == 0) {
            WgradArgs w;
            memset(&w, 0, sizeof(w));
            w.C0 = C; w.C1 = F; w.KW = c->output_filter_size; w.N = C;
            ok = wgrad_bf16_supported(w);
        }
        if (!ok) { t.N = t.Nper = C; ok = narrow_wgrad_supported(t); }
        if (!ok) return false;
    }
    // audio-input conv: the narrow kernels read fp32 audio against bf16 gradients
    {
        NarrowWgradArgs t;
        memset(&t, 0, sizeof(t));
        t.C0 = c->num_channels; t.KW = c->filter_size; t.stride = c->context ? 2 : 1; t.N = t.Nper = dsh.empty() ? 0 : dsh[0].cout;
        if (!narrow_wgrad_supported(t)) return false;
    }
    return true;
}

static void crop_offsets(int from, int to, int& start, int& end) {   // Utils.py:120-121
    const int diff = from - to;
    start = diff / 2;
    end = diff - start;
}

static void add_tensor(wun_plan* p, const std::string& name, std::vector<int64_t> shape, long long& cur,
                       long long* off_out) {
    wun_tensor_info t;
    memset(&t, 0, sizeof(t));
    snprintf(t.name, sizeof(t.name), "%s", name.c_str());
    t.offset = cur;
    t.ndim = (int)shape.size();
    long long n = 1;
    for (size_t i = 0; i < shape.size(); ++i) { t.shape[i] = shape[i]; n *= shape[i]; }
    *off_out = cur;
    cur += n;
    p->tensors.push_back(t);
}

static void add_conv(wun_plan* p, int& counter, int K, int cin, int cout, long long& cur, ConvLayer* out) {
    std::string base = counter == 0 ? "separator/conv1d" : "separator/conv1d_" + std::to_string(counter);
    ++counter;
    out->KW = K; out->Cin = cin; out->Cout = cout;
    add_tensor(p, base + "/kernel", {K, cin, cout}, cur, &out->woff);
    add_tensor(p, base + "/bias", {cout}, cur, &out->boff);
}


extern "C" int wun_plan_create(const wun_config* cfg, int64_t batch, int64_t input_frames, wun_plan** out) {
    int rc = check_config(cfg);
    if (rc) return rc;
    if (!out) return fail(WUN_ERR_INVALID, "out is null");
    if (batch < 1 || input_frames < 1 || input_frames > (1ll << 30)) return fail(WUN_ERR_INVALID, "bad batch / input_frames");
    wun_plan* p = new (std::nothrow) wun_plan();
    if (!p) return fail(WUN_ERR_NOMEM, "out of host memory");
    p->cfg = *cfg;
    p->sw = wun_switches_from_env();
    p->B = (int)batch; p->Tin = (int)input_frames;
    const int L = p->L = cfg->num_layers, F = cfg->num_initial_filters;
    const int Kd = cfg->filter_size, Ku = cfg->merge_filter_size, Ko = cfg->output_filter_size;
    const int C = p->C = cfg->num_channels;
    p->S = cfg->num_sources;
    p->Sh = cfg->output_type == 0 ? p->S : p->S - 1;
    const bool same = p->same = !cfg->context;

    // ---- shape walk of get_output (UnetAudioSeparator.py:97-142) ----
    auto conv_len = [&](int t, int k) { return same ? t : t - k + 1; };
    p->dsh.resize(L);
    int t = p->Tin, cin = C;
    for (int i = 0; i < L; ++i) {
        DownShape& d = p->dsh[i];
        d.cin = cin; d.cout = F + F * i; d.t_in = t; d.t_conv = conv_len(t, Kd);
        if (d.t_conv < 1) { delete p; return fail(WUN_ERR_INVALID, "input too short for the down path"); }
        d.t_dec = (d.t_conv + 1) / 2;                       // [:, ::2, :]  :100
        t = d.t_dec; cin = d.cout;
    }
    p->c_b = F + F * L; p->t_b_in = t; p->t_b = conv_len(t, Kd);
    if (p->t_b < 1) { delete p; return fail(WUN_ERR_INVALID, "input too short for the bottleneck conv"); }
    p->ush.resize(L);
    t = p->t_b; int ccur = p->c_b;
    for (int j = 0; j < L; ++j) {
        UpShape& u = p->ush[j];
        const DownShape& d = p->dsh[L - 1 - j];
        u.c_skip = d.cout; u.c_cur = ccur; u.cout = F + F * (L - j - 1);
        u.t_cur = t; u.t_up = cfg->context ? 2 * t - 1 : 2 * t;      // :115/:117, InterpolationLayer.py:32
        if (same && d.t_conv != u.t_up) {                             // :121
            delete p;
            return fail(WUN_ERR_INVALID, "same-padding input length must be divisible by 2^num_layers (reference assert UnetAudioSeparator.py:121)");
        }
        if (d.t_conv < u.t_up) { delete p; return fail(WUN_ERR_INVALID, "crop with negative difference (Utils.py:117)"); }
        int ce;
        crop_offsets(d.t_conv, u.t_up, u.crop_start, ce);
        u.t_conv = conv_len(u.t_up, Ku);
        if (u.t_conv < 1) { delete p; return fail(WUN_ERR_INVALID, "input too short for the up path"); }
        t = u.t_conv; ccur = u.cout;
    }
    for (int i = 0; i < L; ++i) {
        DownShape& d = p->dsh[i];
        d.tc = p->ush[L - 1 - i].t_up;
        d.cs = p->ush[L - 1 - i].crop_start;
        d.t_ev0 = d.cs + (d.cs & 1); d.t_odd0 = d.cs + 1 - (d.cs & 1);
        d.n_even = d.cs + d.tc > d.t_ev0 ? (d.cs + d.tc - d.t_ev0 + 1) / 2 : 0;
        d.n_odd = d.tc - d.n_even;
    }
    p->t_feat = t;
    if (p->Tin < p->t_feat) { delete p; return fail(WUN_ERR_INVALID, "crop with negative difference (Utils.py:117)"); }
    { int ce; crop_offsets(p->Tin, p->t_feat, p->in_crop_start, ce); }     // :127
    p->Tout = conv_len(p->t_feat, Ko);
    if (p->Tout < 1) { delete p; return fail(WUN_ERR_INVALID, "input too short for the output layer"); }
    { int s2, e2; crop_offsets(p->t_feat, p->Tout, s2, e2); p->mix_diff_off = p->in_crop_start + s2; }  // OutputLayer.py:20

    // ---- variable arena in TF creation order ----
    long long cur = 0;
    int counter = 0;
    p->down.resize(L); p->up.resize(L); p->head.resize(p->Sh);
    for (int i = 0; i < L; ++i) add_conv(p, counter, Kd, p->dsh[i].cin, p->dsh[i].cout, cur, &p->down[i]);
    add_conv(p, counter, Kd, p->dsh[L - 1].cout, p->c_b, cur, &p->bott);
    p->interp.assign(L, -1);
    for (int j = 0; j < L; ++j) {
        if (cfg->upsampling == 1)
            add_tensor(p, "separator/interp_" + std::to_string(j), {p->ush[j].c_cur}, cur, &p->interp[j]);
        add_conv(p, counter, Ku, p->ush[j].c_skip + p->ush[j].c_cur, p->ush[j].cout, cur, &p->up[j]);
    }
    for (int s = 0; s < p->Sh; ++s) add_conv(p, counter, Ko, C + F, C, cur, &p->head[s]);
    p->arena = cur;

    // ---- workspace ----
    long long w = 0;
    const int B = p->B;
    // bf16 mode: every activation and activation-gradient tensor is born bf16 (the audio itself, the head's
    // d(pre-activation), weights, weight gradients and all scratch stay fp32)
    p->bf16 = cfg->compute_dtype == 1 && bf16_plan_ok(cfg, B, p->dsh, p->t_b, p->ush, p->c_b, p->Sh);
    const int eb = p->bf16 ? 2 : 4;
    // (exact-fp32 mode only.  The bf16 mode was built and measured with it at the end of round 6 -- bf16 epilogues with the
    //  expanded / parity copies, the audio-input conv with a strided output, the emulation restated; all 62 bf16-mode tests
    //  green -- and was 3 - 4 % SLOWER (M4 3.27 -> 3.39 ms): its kernels are bound by the instruction stream around the MFMAs,
    //  the scalar strided epilogues of the odd-position launches cost more than the halved window work saves.  Not adopted.)
    p->dedup = !same && !p->bf16 && !p->sw.no_dedup;
    p->early_window = p->sw.early_window != EW_DEFAULT ? p->sw.early_window : p->dedup ? EW_ALL : EW_DEEP;
    p->fuse_ups = !p->bf16 && !p->sw.no_fuse_ups;
    p->mix_ncw = make_buf(p->sw, w, B, C, p->Tin, "mix_ncw");
    p->dec.resize(L); p->skip.resize(L); p->dz_dec.resize(L); p->dz_skip.resize(L);
    for (int i = 0; i < L; ++i) {
        p->dec[i] = make_buf(p->sw, w, B, p->dsh[i].cout, p->dsh[i].t_dec, "dec", i, eb);
        p->skip[i] = make_buf(p->sw, w, B, p->dsh[i].cout, p->dsh[i].tc, "skip", i, eb);
        if (!same) p->dz_dec[i] = make_buf(p->sw, w, B, p->dsh[i].cout, p->dsh[i].t_dec, "dz_dec", i, eb);
        p->dz_skip[i] = make_buf(p->sw, w, B, p->dsh[i].cout, p->dsh[i].tc, "dz_skip", i, eb);
    }
    if (p->dedup) {
        p->dz_odd.resize(L);
        for (int i = 0; i < L; ++i) p->dz_odd[i] = make_buf(p->sw, w, B, p->dsh[i].cout, std::max(p->dsh[i].n_odd, 1), "dz_odd", i, eb);
    }
    p->bott_out = make_buf(p->sw, w, B, p->c_b, p->t_b, "bott_out", 0, eb);
    p->dz_bott = make_buf(p->sw, w, B, p->c_b, p->t_b, "dz_bott", 0, eb);
    p->ups.resize(L); p->upo.resize(L); p->d_ups.resize(L); p->dz_upo.resize(L);
    for (int j = 0; j < L; ++j) {
        p->ups[j] = make_buf(p->sw, w, B, p->ush[j].c_cur, p->ush[j].t_up, "ups", j, eb);
        p->d_ups[j] = make_buf(p->sw, w, B, p->ush[j].c_cur, p->ush[j].t_up, "d_ups", j, eb);
        p->upo[j] = make_buf(p->sw, w, B, p->ush[j].cout, p->ush[j].t_conv, "upo", j, eb);
        p->dz_upo[j] = make_buf(p->sw, w, B, p->ush[j].cout, p->ush[j].t_conv, "dz_upo", j, eb);
    }
    p->dp_pitch = (p->Tout + 3) / 4 * 4;
    p->dpre_off = bump(w, (long long)p->Sh * B * C * p->dp_pitch);
    if (p->bf16 && p->Sh > 0) {
        NarrowWgradArgs t;
        memset(&t, 0, sizeof(t));
        t.C0 = C; t.C1 = F; t.KW = Ko; t.stride = 1; t.N = p->Sh * C; t.Nper = C;
        if (!narrow_wgrad_supported(t) && (C & 1) == 0) {
            p->head16 = true;
            p->mix16 = make_buf(p->sw, w, B, C, p->Tin, "mix16", 0, 2);
            p->dp16_pitch = (p->Tout + 7) / 8 * 8;
            p->dpre16_off = bump(w, ((long long)p->Sh * B * C * p->dp16_pitch + 1) / 2);
        }
    }
    p->loss_partial_off = bump(w, 1024);
    if (cfg->upsampling == 1) {                                   // [B][C] partials of every interp_<j> gradient (own block per
        p->interp_partial_off.assign(L, -1);                      // level: consecutive levels run on different side streams)
        for (int j = 0; j < L; ++j) p->interp_partial_off[j] = bump(w, (long long)B * p->ush[j].c_cur);
    }
    p->conv_part_floats = 16ll << 20;                       // split-K scratch (64 MiB)
    p->conv_part_off = bump(w, p->conv_part_floats);

    // ---- transposed / tap-flipped weights for the input-gradient convs ----
    auto add_wt = [&](const ConvLayer& cl, int J, int k_last, int k_step) -> long long {
        WtDesc d;
        d.src_off = cl.woff; d.J = J; d.C = cl.Cin; d.N = cl.Cout; d.k_last = k_last; d.k_step = k_step; d.mode = 0;
        d.dst_off = bump(w, (long long)J * cl.Cin * cl.Cout);
        p->wt.push_back(d);
        const long long n = (long long)J * cl.Cin * cl.Cout;
        if (n > p->wt_max) p->wt_max = (int)n;
        return d.dst_off;
    };
    // both output phases of the transposed stride-2 conv side by side: [J0][Cout][2][Cin]
    auto add_wt2 = [&](const ConvLayer& cl, int J0) -> long long {
        WtDesc d;
        d.src_off = cl.woff; d.J = J0; d.C = cl.Cin; d.N = cl.Cout; d.k_last = 2 * (J0 - 1); d.k_step = cl.KW; d.mode = 1;
        const long long n = (long long)J0 * cl.Cin * cl.Cout * 2;
        d.dst_off = bump(w, n);
        p->wt.push_back(d);
        if (n > p->wt_max) p->wt_max = (int)n;
        return d.dst_off;
    };
    for (int i = 1; i < L; ++i) {
        ConvLayer& cl = p->down[i];
        cl.wt_full = add_wt(cl, cl.KW, cl.KW - 1, 1);
        if (!same) {
            for (int ph = 0; ph < 2; ++ph) {
                const int Jp = (cl.KW - ph + 1) / 2;          // taps k = 2j + ph < KW
                cl.Jp[ph] = Jp;
                cl.wt_ph[ph] = add_wt(cl, Jp, 2 * (Jp - 1) + ph, 2);
            }
            cl.J0 = (cl.KW + 1) / 2;
            cl.wt_ph2 = add_wt2(cl, cl.J0);
            if (p->dedup) {
                cl.J0s = (cl.KW + 2) / 2;
                cl.wt_ph2s = add_wt2(cl, cl.J0s);
                p->wt.back().k_last = 2 * (cl.J0s - 1) - 1;      // tap of W behind tap 2 (J0s - 1) of the shifted filter
            }
        }
    }
    p->bott.wt_full = add_wt(p->bott, Kd, Kd - 1, 1);
    for (int j = 0; j < L; ++j) p->up[j].wt_full = add_wt(p->up[j], Ku, Ku - 1, 1);

    // ---- bf16 mode: packed weight images (every conv with >= 8 input channels; the audio-input conv and the
    // output head stay exact fp32) ----
    if (p->bf16) {
        auto add_img = [&](int in_ws, long long src_off, int K, int Cc, int Nn, int slack = 0) {
            if (Cc < 8 || K < 1) return;
            PackDesc d;
            d.src_off = src_off; d.src_in_ws = in_ws; d.KW = K; d.C = Cc; d.N = Nn;
            d.C8p = bf16_image_groups(Cc); d.Npad = (Nn + slack + 63) / 64 * 64;
            const long long items = (long long)K * d.C8p * d.Npad;
            d.dst_off = bump(w, items * 4);                     // 8 bf16 = 4 floats per item
            p->pack.push_back(d);
            p->pack_max = std::max(p->pack_max, items);
            p->bf_img[{in_ws, src_off}] = wun_plan::BfImg{d.dst_off, d.C8p, d.Npad};
        };
        for (int i = 0; i < L; ++i) add_img(0, p->down[i].woff, Kd, p->down[i].Cin, p->down[i].Cout);
        add_img(0, p->bott.woff, Kd, p->bott.Cin, p->bott.Cout);
        for (int j = 0; j < L; ++j) add_img(0, p->up[j].woff, Ku, p->up[j].Cin, p->up[j].Cout);
        p->npack_fwd = (int)p->pack.size();
        // input-gradient convs: "input channels" = the forward conv's Cout, outputs = its Cin
        for (int i = 1; i < L; ++i) {
            const ConvLayer& cl = p->down[i];
            add_img(1, cl.wt_full, cl.KW, cl.Cout, cl.Cin);
            if (!same) for (int ph = 0; ph < 2; ++ph) add_img(1, cl.wt_ph[ph], cl.Jp[ph], cl.Cout, cl.Cin);
            // fused two-phase image: the transposed copy [J0][Cout][2][Cin] read as a [J0][Cout][2*Cin] matrix
            if (!same) add_img(1, cl.wt_ph2, cl.J0, cl.Cout, 2 * cl.Cin, 32);   // (+32: a phase-1 column tile may overhang)
        }
        add_img(1, p->bott.wt_full, Kd, p->bott.Cout, p->bott.Cin);
        for (int j = 0; j < L; ++j) add_img(1, p->up[j].wt_full, Ku, p->up[j].Cout, p->up[j].Cin);
    }

    // ---- wgrad partial buffer: max over layers of (total splits) * (kernel + bias floats) ----
    long long pmax = 0;
    // floats per split in the tile-major partial buffer, worst-case tile padding (384 rows x 80 columns)
    // (bf16 speed mode: rows come in slots of 16 channels x 1 tap, up to 32 slots per row group)
    const long long rowpad = p->bf16 ? 1024 : 384;
    auto blockf = [rowpad](const ConvLayer& cl) { return ((long long)cl.KW * (cl.Cin + 15) + 1 + rowpad) * (cl.Cout + 80); };
    // one part of a layer's weight gradient under BOTH exact-fp32 kernels: the LDS-tiled one (tile-major partial
    // blocks) and -- where it serves the shape -- the register-window one, whose split policy differs (it always aims
    // at 1024 workgroups and counts units of its own length) and whose partial blocks have the final layout
    auto need = [&](const WgradArgs& w, const ConvLayer& cl) {
        long long n = (long long)wgrad_pick_nsplit(w, p->sw) * blockf(cl);
        WgradArgs ww = w;
        ww.win = 1;
        if (!p->bf16 && wgrad_win_supported(ww)) n = std::max(n, (long long)wgrad_pick_nsplit(ww, p->sw) * wgrad_win_partial_floats(ww, p->sw));
        return n;
    };
    for (int i = 0; i < L; ++i) {
        const DownShape& d = p->dsh[i];
        long long n;
        if (same) {
            n = need(wgrad_shape_only(B, d.cin, 0, Kd, LOADER_DIRECT, d.cout, d.t_conv), p->down[i]);
        } else {
            n = need(wgrad_shape_only(B, d.cin, 0, Kd, LOADER_DEINT, d.cout, d.t_dec), p->down[i]);
            if (!p->dedup) n += need(wgrad_shape_only(B, d.cin, 0, Kd, LOADER_DIRECT, d.cout, d.tc), p->down[i]);
            else if (d.n_odd > 0) n += need(wgrad_shape_only(B, d.cin, 0, Kd, LOADER_DEINT, d.cout, d.n_odd), p->down[i]);
        }
        pmax = std::max(pmax, n);
    }
    pmax = std::max(pmax, need(wgrad_shape_only(B, p->bott.Cin, 0, Kd, LOADER_DIRECT, p->c_b, p->t_b), p->bott));
    for (int j = 0; j < L; ++j)
        pmax = std::max(pmax, need(wgrad_shape_only(B, p->ush[j].c_skip, p->ush[j].c_cur, Ku, LOADER_DIRECT, p->ush[j].cout, p->ush[j].t_conv), p->up[j]));
    if (p->Sh > 0)
        pmax = std::max(pmax, need(wgrad_shape_only(B, C, F, Ko, LOADER_DIRECT, C, p->Tout), p->head[0]));
    pmax *= 4;                                              // two streams' halves, each with 2x headroom for the autotuner's split counts
    p->partial_floats = pmax;
    p->partial_off = bump(w, pmax);
    p->ws = (w + 63) / 64 * 64;

    // ---- FLOP accounting (2*MAC of the conv contractions) ----
    auto cf = [&](int K, double ci, double co, double tt) { return 2.0 * K * ci * co * tt * B; };
    double fwd = 0, dense = 0, bwd = 0, uniq_f = 0, uniq_b = 0;
    for (int i = 0; i < L; ++i) {
        const DownShape& d = p->dsh[i];
        dense += cf(Kd, d.cin, d.cout, d.t_conv);
        // every observed conv output once: the even positions + the odd positions inside the crop window
        const double once = same ? cf(Kd, d.cin, d.cout, d.t_conv) : cf(Kd, d.cin, d.cout, d.t_dec) + cf(Kd, d.cin, d.cout, d.n_odd);
        const double live = (same || p->dedup) ? once : cf(Kd, d.cin, d.cout, d.t_dec) + cf(Kd, d.cin, d.cout, d.tc);
        fwd += live; uniq_f += once;
        bwd += live * (i > 0 ? 2.0 : 1.0); uniq_b += once * (i > 0 ? 2.0 : 1.0);
    }
    { const double f = cf(Kd, p->bott.Cin, p->c_b, p->t_b); fwd += f; dense += f; bwd += 2 * f; uniq_f += f; uniq_b += 2 * f; }
    for (int j = 0; j < L; ++j) {
        const double f = cf(Ku, p->ush[j].c_skip + p->ush[j].c_cur, p->ush[j].cout, p->ush[j].t_conv);
        fwd += f; dense += f; bwd += 2 * f; uniq_f += f; uniq_b += 2 * f;
    }
    { const double f = p->Sh * cf(Ko, C + F, C, p->Tout); fwd += f; dense += f; bwd += 2 * f; uniq_f += f; uniq_b += 2 * f; }
    p->fwd_flops = fwd; p->bwd_flops = bwd; p->fwd_dense = dense; p->fwd_unique = uniq_f; p->bwd_unique = uniq_b;

    // ---- device-side descriptor table (the only device memory the plan owns) ----
    if (!p->wt.empty()) {
        hipError_t e = hipMalloc((void**)&p->dev_wt, p->wt.size() * sizeof(WtDesc));
        if (e == hipSuccess) e = hipMemcpy(p->dev_wt, p->wt.data(), p->wt.size() * sizeof(WtDesc), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            // no device available (e.g. CPU-only build box): the plan is still usable for queries
            p->dev_wt = nullptr;
            (void)hipGetLastError();
        }
    }
    if (!p->pack.empty()) {
        hipError_t e = hipMalloc((void**)&p->dev_pack, p->pack.size() * sizeof(PackDesc));
        if (e == hipSuccess) e = hipMemcpy(p->dev_pack, p->pack.data(), p->pack.size() * sizeof(PackDesc), hipMemcpyHostToDevice);
        if (e != hipSuccess) { p->dev_pack = nullptr; (void)hipGetLastError(); }
    }
    // wun_grad_norm's chunk table: each tensor cut into WUN_NORM_CHUNK-float chunks in arena order
    p->norm_first.assign(1, 0);
    for (size_t k = 0; k < p->tensors.size(); ++k) {
        const wun_tensor_info& t = p->tensors[k];
        long long n = 1;
        for (int d = 0; d < t.ndim; ++d) n *= t.shape[d];
        for (long long o = 0; o < n; o += WUN_NORM_CHUNK)
            p->norm_chunks.push_back({t.offset + o, (int)std::min<long long>(WUN_NORM_CHUNK, n - o), (int)k});
        p->norm_first.push_back((int)p->norm_chunks.size());
    }
    if (!p->norm_chunks.empty()) {
        const size_t cb = p->norm_chunks.size() * sizeof(NormChunk), fb = p->norm_first.size() * sizeof(int);
        hipError_t e = hipMalloc((void**)&p->dev_norm_chunks, cb + fb);
        if (e == hipSuccess) e = hipMemcpy(p->dev_norm_chunks, p->norm_chunks.data(), cb, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            p->dev_norm_first = reinterpret_cast<int*>(p->dev_norm_chunks + p->norm_chunks.size());
            e = hipMemcpy(p->dev_norm_first, p->norm_first.data(), fb, hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) {
            if (p->dev_norm_chunks) (void)hipFree(p->dev_norm_chunks);
            p->dev_norm_chunks = nullptr; p->dev_norm_first = nullptr;
            (void)hipGetLastError();
        }
    }
    *out = p;
    return WUN_OK;
}

extern "C" void wun_plan_destroy(wun_plan* p) {
    if (!p) return;
    if (p->dev_wt) (void)hipFree(p->dev_wt);
    if (p->dev_pack) (void)hipFree(p->dev_pack);
    if (p->dev_norm_chunks) (void)hipFree(p->dev_norm_chunks);
    for (auto e : p->events) (void)hipEventDestroy(e);
    if (p->tev0) { (void)hipEventDestroy(p->tev0); (void)hipEventDestroy(p->tev1); }
    if (p->wt_ev) (void)hipEventDestroy(p->wt_ev);
    for (auto e : p->skip_ev) (void)hipEventDestroy(e);
    for (auto e : p->win_ev) (void)hipEventDestroy(e);
    if (p->side) (void)hipStreamDestroy(p->side);
    if (p->side2) (void)hipStreamDestroy(p->side2);
    delete p;
}

extern "C" int wun_plan_query(const wun_plan* p, wun_plan_info* info) {
    if (!p || !info) return fail(WUN_ERR_INVALID, "null argument");
    info->batch = p->B; info->input_frames = p->Tin; info->output_frames = p->Tout;
    long long n = 0;
    for (const auto& t : p->tensors) { long long k = 1; for (int i = 0; i < t.ndim; ++i) k *= t.shape[i]; n += k; }
    info->num_params = n; info->arena_floats = p->arena; info->workspace_floats = p->ws;
    info->num_tensors = (int64_t)p->tensors.size(); info->num_outputs = p->S;
    info->fwd_flops = p->fwd_flops; info->bwd_flops = p->bwd_flops; info->fwd_flops_dense = p->fwd_dense;
    info->fwd_flops_unique = p->fwd_unique; info->bwd_flops_unique = p->bwd_unique;
    info->compute_dtype_effective = p->bf16 ? 1 : 0;
    return WUN_OK;
}

extern "C" int wun_plan_tensor(const wun_plan* p, int64_t index, wun_tensor_info* info) {
    if (!p || !info) return fail(WUN_ERR_INVALID, "null argument");
    if (index < 0 || index >= (int64_t)p->tensors.size()) return fail(WUN_ERR_INVALID, "tensor index out of range");
    *info = p->tensors[(size_t)index];
    return WUN_OK;
}

extern "C" int wun_plan_activation(const wun_plan* p, int32_t kind, int32_t index, wun_activation_info* info) {
    if (!p || !info) return fail(WUN_ERR_INVALID, "null argument");
    const Buf* b = nullptr;
    long long t0 = 0, tstep = 1;
    if (kind == 0 && index >= 0 && index < p->L) { b = &p->dec[(size_t)index]; tstep = 2; }
    else if (kind == 1 && index >= 0 && index < p->L) { b = &p->skip[(size_t)index]; t0 = p->same ? 0 : p->dsh[(size_t)index].cs; }
    else if (kind == 2 && index == 0) b = &p->bott_out;
    else if (kind == 3 && index >= 0 && index < p->L) b = &p->upo[(size_t)index];
    else if (kind == 4 && index >= 0 && index < p->L) b = &p->ups[(size_t)index];
    else if (kind == 5 && index >= 0 && index < p->L) b = &p->dz_upo[(size_t)index];
    else if (kind == 6 && index >= 0 && index < p->L) b = &p->d_ups[(size_t)index];
    else if (kind == 7 && index >= 0 && index < p->L) { b = &p->dz_skip[(size_t)index]; t0 = p->same ? 0 : p->dsh[(size_t)index].cs; }
    else if (kind == 8 && index >= 0 && index < p->L && !p->same) { b = &p->dz_dec[(size_t)index]; tstep = 2; }
    else if (kind == 9 && index == 0) b = &p->dz_bott;
    if (b == nullptr) return fail(WUN_ERR_INVALID, "wun_plan_activation: unknown kind / index");
    info->offset = b->off; info->batch_stride = b->bs; info->pitch = b->pitch;
    info->channels = b->C; info->frames = b->T; info->t0 = t0; info->tstep = tstep; info->elem_bytes = b->eb;
    return WUN_OK;
}

extern "C" int wun_profile_begin(void) { g_profiling = true; prof_begin(wun_switches_from_env().profile_detail); return WUN_OK; }

extern "C" int wun_profile_end(char* json_out, int64_t capacity) {
    const std::string js = prof_end();
    g_profiling = false;
    if (!json_out || capacity < (int64_t)js.size() + 1) return fail(WUN_ERR_INVALID, "profile buffer too small");
    memcpy(json_out, js.c_str(), js.size() + 1);
    return WUN_OK;
}

extern "C" int wun_abi_sizes(int64_t* sizes, int n) {
    const int64_t v[3] = {(int64_t)sizeof(wun_config), (int64_t)sizeof(wun_plan_info), (int64_t)sizeof(wun_tensor_info)};
    for (int i = 0; i < 3 && i < n && sizes != nullptr; ++i) sizes[i] = v[i];
    return 3;
}

extern "C" const char* wun_last_error(void) { return g_err.c_str(); }
extern "C" const char* wun_version(void) { return "wun 0.5 (gfx950, fp32 MFMA 16x16x4 + bf16 MFMA 16x16x32 speed mode)"; }
