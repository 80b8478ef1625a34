// Host side of libwun.so: the single-operator entry points (wun_op_*) the tests and tools call, their test hooks and
// the MFMA lane-layout probes.
#include "wun_plan_impl.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace wun {
hipError_t launch_make_wt_one(const float* src, float* dst, WtDesc d, hipStream_t s);
}

// ---------------------------------------------------------------------------------------
// single operators
// ---------------------------------------------------------------------------------------
// the single-operator entry points use a lazily allocated split-K scratch of their own
static const long long kOpScratchFloats = 8ll << 20;
static int g_op_variant = -1, g_op_ksplit = 0;          // wun_op_force_conv_variant (test hook)
static int g_op_wg_mtw = 0, g_op_wg_nw = 0, g_op_wg_nsplit = 0;   // wun_op_force_wgrad_variant (test hook)
static int g_op_wg_bf16 = 0;                                       // wun_op_set_wgrad_bf16 (test hook)
static int g_op_wg_narrow = 0;                                     // wun_op_set_wgrad_narrow (test hook)
static int g_op_wg_win = 0;                                        // wun_op_set_wgrad_win (test hook)
static float* g_op_copy0 = nullptr; static float* g_op_copy1 = nullptr;   // wun_op_set_conv_copies (test hook)
static int g_op_copy_t0 = 0, g_op_copy_t1 = 0, g_op_copy_exp = 0, g_op_copy_lo = 0, g_op_copy_len = 0, g_op_acc_lo = 0, g_op_acc_len = 0;
static float* g_op_ups_y = nullptr; static const float* g_op_ups_w = nullptr;   // wun_op_set_conv_upsample (test hook)
static int g_op_ups_pitch = 0, g_op_ups_tup = 0;
static thread_local int t_op_epilogue_path = WUN_PATH_NONE;                     // wun_op_last_path(WUN_OP_CONV_EPILOGUE)
static thread_local int t_op_first_conv_path = WUN_PATH_NONE;                   // wun_op_last_path(WUN_OP_FIRST_CONV)
static thread_local int t_op_wgrad_path = WUN_PATH_NONE, t_op_wgrad_splits = 0;  // wun_op_last_path(WUN_OP_WGRAD), wun_op_wgrad_last_splits
static float* op_scratch() {
    static float* buf = nullptr;
    if (!buf && hipMalloc((void**)&buf, kOpScratchFloats * sizeof(float)) != hipSuccess) {
        buf = nullptr;
        (void)hipGetLastError();
    }
    return buf;
}

// The bf16 kernels read bf16 rows (the plan's activations are born bf16); the single-operator entry points receive fp32
// tensors and convert them first -- rounding to nearest even, exactly what "operands rounded to bf16" means -- into a
// process-wide temporary (slot 0 / 1) that grows on demand.  Rows are re-pitched to 16 bytes.
static void* op_bf16_tmp(int slot, size_t bytes) {
    static void* buf[2] = {nullptr, nullptr};
    static size_t cap[2] = {0, 0};
    if (bytes > cap[slot]) {
        (void)hipDeviceSynchronize();
        if (buf[slot]) (void)hipFree(buf[slot]);
        buf[slot] = nullptr; cap[slot] = 0;
        const size_t want = bytes + (bytes >> 2) + 4096;
        if (hipMalloc(&buf[slot], want) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        cap[slot] = want;
    }
    return buf[slot];
}
static inline int pad8(int t) { return (t + 7) / 8 * 8; }
// fp32 [rows][spitch] (T valid) -> bf16 [rows][pad8(T)] in temporary `slot`; returns the bf16 base or null
static const float* op_to_bf16(int slot, const float* src, long long rows, int T, long long spitch, hipStream_t s) {
    void* dst = op_bf16_tmp(slot, (size_t)rows * pad8(T) * 2 + 64);
    if (!dst) return nullptr;
    if (launch_cast_rows_bf16(src, dst, rows, T, spitch, pad8(T), s) != hipSuccess) return nullptr;
    return reinterpret_cast<const float*>(dst);
}

static hipError_t op_launch_conv(ConvArgs a, hipStream_t s) {
    // (a forced bf16 tile code, >= kBf16VariantBase, is for the bf16 entries: op_force_bf16)
    if (g_op_variant >= 0 && g_op_variant < kBf16VariantBase) {
        a.force_variant = g_op_variant + 1; a.force_ksplit = (a.flags & F_PHASE2) ? 0 : g_op_ksplit;
    }
    return launch_conv(a, op_scratch(), kOpScratchFloats, s, wun_switches_from_env());
}

// the bf16 entries under wun_op_force_conv_variant: a forced tile code goes into the launch; false = the launcher would refuse it
// (the caller returns WUN_ERR_UNSUPPORTED before any GPU work).  Forced fp32 variants are not for these entries.
static bool op_force_bf16(ConvArgs& a) {
    if (g_op_variant < kBf16VariantBase) return true;
    if (!conv_bf16_choice_ok(a, g_op_variant)) return false;
    a.force_variant = g_op_variant + 1;
    return true;
}
static_assert(WUN_BF16_VARIANT_BASE == kBf16VariantBase, "wun.h tile code base");

static void op_src(ConvArgs& a, const float* x, int C, int T) {
    const int pitch = T;
    a.src0 = x; a.bs0 = (long long)C * pitch; a.pitch0 = pitch; a.off0 = 0; a.C0 = C;
}

extern "C" int wun_op_conv1d(const float* x, const float* w, const float* bias, float* y, int batch, int cin,
                             int cout, int k, int t_in, int t_out, int stride, int pad_left, int lrelu,
                             void* stream) {
    if (!x || !w || !y) return fail(WUN_ERR_INVALID, "null argument");
    if (stride != 1 && stride != 2) return fail(WUN_ERR_UNSUPPORTED, "stride must be 1 or 2");
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.B = batch; a.ostride = 1;
    op_src(a, x, cin, t_in);
    a.loader = stride == 2 ? LOADER_DEINT : LOADER_DIRECT;
    a.Tin = t_in; a.shift = pad_left; a.W = w; a.bias = bias; a.KW = k; a.N = a.N0 = cout; a.Tout = t_out;
    a.flags = lrelu ? F_LRELU : 0;
    a.dst0 = y; a.obs0 = (long long)cout * t_out; a.opitch0 = t_out;
    HIP_TRY(op_launch_conv(a, (hipStream_t)stream));
    return WUN_OK;
}

static inline int pad4(int t) { return (t + 3) / 4 * 4; }

static WgradArgs op_wgrad_args(const float* x, const float* dz, int batch, int cin, int cout, int k, int t_in,
                               int t_out, int stride, int pad_left, int xp, int zp) {
    WgradArgs w;
    memset(&w, 0, sizeof(w));
    w.B = batch; w.loader = stride == 2 ? LOADER_DEINT : LOADER_DIRECT;
    w.src0 = x; w.bs0 = (long long)cin * xp; w.pitch0 = xp; w.C0 = cin;
    w.Tin = t_in; w.shift = pad_left; w.KW = k;
    w.dz = dz; w.dzbs = (long long)cout * zp; w.dzpitch = zp; w.N = cout; w.Tq = t_out;
    return w;
}

// split partials of one loader kind under the current (possibly forced) geometry / split count
static long long op_wgrad_part_floats(int batch, int cin, int cout, int k, int t_out, int loader, const WunSwitches& sw) {
    WgradArgs a = wgrad_shape_only(batch, cin, 0, k, loader, cout, t_out);
    a.bf16 = (g_op_wg_bf16 && wgrad_bf16_supported(a)) ? 1 : 0;
    a.win = (g_op_wg_win && !a.bf16) ? 1 : 0;
    if (a.win && !wgrad_win_supported(a)) a.win = 0;
    if (g_op_wg_mtw > 0) { a.force_mtw = g_op_wg_mtw; a.force_nw = g_op_wg_nw; }
    long long ns = wgrad_pick_nsplit(a, sw);
    if (g_op_wg_nsplit > 0) ns = std::min(g_op_wg_nsplit, wgrad_max_units(a, sw));
    if (g_op_wg_nsplit < 0 && a.win) ns = std::min(std::max(1, -g_op_wg_nsplit / wgrad_win_tiles(a, sw)), wgrad_max_units(a, sw));
    return ns * wgrad_partial_floats(a, sw);
}

extern "C" int64_t wun_op_conv1d_wgrad_scratch(int batch, int cin, int cout, int k, int t_out) {
    const WunSwitches sw = wun_switches_from_env();
    // split partials (worst case over both loaders) + repacked copies of x (t_in <= 2*t_out + k) and dz
    long long part = std::max(op_wgrad_part_floats(batch, cin, cout, k, t_out, LOADER_DIRECT, sw),
                              op_wgrad_part_floats(batch, cin, cout, k, t_out, LOADER_DEINT, sw));
    if (g_op_wg_narrow) {
        // wun_op_set_wgrad_narrow(1): the direct-reduction kernels keep one (k * cin + 1) * cout vector per split
        NarrowWgradArgs nw;
        memset(&nw, 0, sizeof(nw));
        nw.C0 = cin; nw.KW = k; nw.N = nw.Nper = cout; nw.Tq = t_out; nw.B = batch;
        for (int stride = 1; stride <= 2; ++stride) {
            nw.stride = stride;
            part = std::max(part, (long long)narrow_wgrad_pick_nsplit(nw, sw) * narrow_wgrad_partial_floats(nw));
        }
    }
    const long long tin_max = 2ll * t_out + k + 8;
    return part + (long long)batch * cin * pad4((int)tin_max) + (long long)batch * cout * pad4(t_out) + 512;
}

extern "C" int wun_op_conv1d_wgrad(const float* x, const float* dz, float* dw, float* db, float* scratch,
                                   int batch, int cin, int cout, int k, int t_in, int t_out, int stride,
                                   int pad_left, void* stream) {
    if (!x || !dz || !dw || !db || !scratch) return fail(WUN_ERR_INVALID, "null argument");
    if (stride != 1 && stride != 2) return fail(WUN_ERR_UNSUPPORTED, "stride must be 1 or 2");
    if (t_in > 2ll * t_out + k + 8) return fail(WUN_ERR_INVALID, "t_in larger than the conv can consume");
    hipStream_t s = (hipStream_t)stream;
    const WunSwitches sw = wun_switches_from_env();
    // repack x / dz into the canonical 4-padded row layout the kernels use
    const int xp = pad4(t_in), zp = pad4(t_out);
    float* xs = scratch;                                   // 64-float aligned by construction below
    xs = (float*)(((uintptr_t)xs + 255) & ~(uintptr_t)255);
    float* zs = xs + (long long)batch * cin * xp;
    float* part = zs + (long long)batch * cout * zp;
    HIP_TRY(hipMemcpy2DAsync(xs, (size_t)xp * 4, x, (size_t)t_in * 4, (size_t)t_in * 4, (size_t)batch * cin,
                             hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpy2DAsync(zs, (size_t)zp * 4, dz, (size_t)t_out * 4, (size_t)t_out * 4, (size_t)batch * cout,
                             hipMemcpyDeviceToDevice, s));
    if (g_op_wg_narrow) {
        // the direct-reduction kernels of wun_narrow.hip (what the plan runs for the audio-input conv and the head)
        NarrowWgradArgs nw;
        memset(&nw, 0, sizeof(nw));
        nw.src0 = xs; nw.bs0 = (long long)cin * xp; nw.pitch0 = xp; nw.off0 = 0; nw.C0 = cin;
        nw.Tin = t_in; nw.shift = pad_left; nw.KW = k; nw.stride = stride;
        nw.dz = zs; nw.zss = 0; nw.dzbs = (long long)cout * zp; nw.dzpitch = zp;
        nw.N = nw.Nper = cout; nw.Tq = t_out; nw.B = batch;
        if (!narrow_wgrad_supported(nw)) return fail(WUN_ERR_UNSUPPORTED, "shape not served by the narrow weight-gradient kernels");
        nw.nsplit = narrow_wgrad_pick_nsplit(nw, sw);
        part = (float*)(((uintptr_t)part + 255) & ~(uintptr_t)255);
        nw.partial = part; nw.split_base = 0;
        HIP_TRY(launch_narrow_wgrad(nw, s, sw));
        const long long woff[4] = {0, 0, 0, 0}, boff[4] = {(long long)(db - dw), 0, 0, 0};
        HIP_TRY(launch_narrow_wgrad_reduce(nw, part, nw.nsplit, dw, woff, boff, s));
        return WUN_OK;
    }
    WgradArgs w = op_wgrad_args(xs, zs, batch, cin, cout, k, t_in, t_out, stride, pad_left, xp, zp);
    if (g_op_wg_bf16 && !wgrad_bf16_supported(w)) return fail(WUN_ERR_UNSUPPORTED, "shape not served by the bf16 weight-gradient kernel");
    w.bf16 = g_op_wg_bf16;
    w.win = (g_op_wg_win && !w.bf16) ? 1 : 0;
    if (w.win && !wgrad_win_supported(w)) return fail(WUN_ERR_UNSUPPORTED, "shape not served by the register-window weight-gradient kernel");
    if (g_op_wg_mtw > 0) {
        w.force_mtw = g_op_wg_mtw; w.force_nw = g_op_wg_nw;
        int m, n;
        wgrad_resolved_geom(w, m, n);
        if (m != g_op_wg_mtw || n != g_op_wg_nw)
            return fail(WUN_ERR_UNSUPPORTED, "forced weight-gradient tile geometry is not available for this shape");
    }
    w.nsplit = wgrad_pick_nsplit(w, sw);
    if (g_op_wg_nsplit > 0) {
        w.nsplit = std::min(g_op_wg_nsplit, wgrad_max_units(w, sw));
    }
    if (g_op_wg_nsplit < 0 && w.win)       // (window kernel: a negative count is a target grid size)
        w.nsplit = std::min(std::max(1, -g_op_wg_nsplit / wgrad_win_tiles(w, sw)), wgrad_max_units(w, sw));
    part = (float*)(((uintptr_t)part + 255) & ~(uintptr_t)255);
    w.out = part; w.direct = 0; w.split_base = 0;      // always through the split reduction (dw and db are separate buffers)
    if (w.bf16) {
        // the bf16 kernel reads bf16 rows: convert the repacked copies of x and dz
        w.src0 = op_to_bf16(0, xs, (long long)batch * cin, t_in, xp, s);
        w.dz = op_to_bf16(1, zs, (long long)batch * cout, t_out, zp, s);
        if (!w.src0 || !w.dz) return fail(WUN_ERR_NOMEM, "bf16 temporary");
        w.pitch0 = pad8(t_in); w.bs0 = (long long)cin * w.pitch0;
        w.dzpitch = pad8(t_out); w.dzbs = (long long)cout * w.dzpitch;
        w.sbf = 1;
    }
    HIP_TRY(launch_wgrad(w, s, sw));
    HIP_TRY(launch_wgrad_reduce(w, part, w.nsplit, dw, db, s, sw));
    return WUN_OK;
}

extern "C" int wun_op_conv1d_dgrad(const float* dz, const float* w, float* dx, float* wt_scratch, int batch,
                                   int cin, int cout, int k, int t_in, int t_out, int stride, int pad_left,
                                   void* stream) {
    if (!dz || !w || !dx || !wt_scratch) return fail(WUN_ERR_INVALID, "null argument");
    if (stride != 1 && stride != 2) return fail(WUN_ERR_UNSUPPORTED, "stride must be 1 or 2");
    hipStream_t s = (hipStream_t)stream;
    if (stride == 1) {
        WtDesc d; d.src_off = 0; d.dst_off = 0; d.J = k; d.C = cin; d.N = cout; d.k_last = k - 1; d.k_step = 1; d.mode = 0;
        HIP_TRY(launch_make_wt_one(w, wt_scratch, d, s));
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        a.B = batch; a.ostride = 1;
        op_src(a, dz, cout, t_out);
        a.Tin = t_out; a.shift = k - 1 - pad_left; a.W = wt_scratch; a.KW = k; a.N = a.N0 = cin; a.Tout = t_in;
        a.dst0 = dx; a.obs0 = (long long)cin * t_in; a.opitch0 = t_in;
        HIP_TRY(op_launch_conv(a, s));
    } else {
        if (pad_left != 0) return fail(WUN_ERR_UNSUPPORTED, "stride-2 dgrad supports pad_left == 0 only");
        const int J0 = (k + 1) / 2;
        ConvArgs f;
        memset(&f, 0, sizeof(f));
        f.B = batch; f.ostride = 1;
        op_src(f, dz, cout, t_out);
        f.Tin = t_out; f.KW = J0; f.kw_full = k; f.shift = J0 - 1; f.W = wt_scratch; f.N = f.N0 = cin;
        f.Tout = (t_in + 1) / 2; f.Tlim = t_in; f.flags = F_PHASE2;
        f.dst0 = dx; f.obs0 = (long long)cin * t_in; f.opitch0 = t_in;
        if ((cin & 3) == 0 && conv_natural_wgs_phase2(f) >= 64) {
            WtDesc d; d.src_off = 0; d.dst_off = 0; d.J = J0; d.C = cin; d.N = cout; d.k_last = 2 * (J0 - 1);
            d.k_step = k; d.mode = 1;
            HIP_TRY(launch_make_wt_one(w, wt_scratch, d, s));
            HIP_TRY(op_launch_conv(f, s));
            return WUN_OK;
        }
        for (int ph = 0; ph < 2; ++ph) {
            const int Jp = (k - ph + 1) / 2;
            float* wt = wt_scratch + (long long)ph * k * cin * cout;
            WtDesc d; d.src_off = 0; d.dst_off = 0; d.J = Jp; d.C = cin; d.N = cout;
            d.k_last = 2 * (Jp - 1) + ph; d.k_step = 2; d.mode = 0;
            if (Jp > 0) HIP_TRY(launch_make_wt_one(w, wt, d, s));
            ConvArgs a;
            memset(&a, 0, sizeof(a));
            a.B = batch; a.ostride = 2;
            op_src(a, dz, cout, t_out);
            a.Tin = t_out; a.KW = Jp; a.shift = Jp - 1; a.W = wt; a.N = a.N0 = cin; a.Tout = (t_in - ph + 1) / 2;
            a.dst0 = dx; a.obs0 = (long long)cin * t_in; a.opitch0 = t_in; a.ooff0 = ph;
            HIP_TRY(op_launch_conv(a, s));
        }
    }
    return WUN_OK;
}

extern "C" int wun_op_force_conv_variant(int variant, int ksplit) {
    g_op_variant = variant; g_op_ksplit = ksplit;
    return WUN_OK;
}

extern "C" int wun_op_num_conv_variants(void) { return conv_num_variants(); }

extern "C" int wun_op_set_wgrad_bf16(int on) { g_op_wg_bf16 = on ? 1 : 0; return WUN_OK; }
extern "C" int wun_op_set_wgrad_win(int on) { g_op_wg_win = on ? 1 : 0; return WUN_OK; }
extern "C" int wun_op_set_wgrad_narrow(int on) { g_op_wg_narrow = on ? 1 : 0; return WUN_OK; }

extern "C" int wun_op_force_wgrad_variant(int mtw, int nw, int nsplit) {
    g_op_wg_mtw = mtw; g_op_wg_nw = nw; g_op_wg_nsplit = nsplit;
    return WUN_OK;
}

// General form of the conv launch the plan uses: virtual channel-concat of two sources (crop_and_concat,
// Utils.py:11-24), accumulate into the destination, LeakyReLU-derivative mask, output stride / offset.
extern "C" int wun_op_conv1d_ex(const float* x0, int c0, const float* x1, int c1, const float* w, const float* bias,
                                float* y, const float* mask, int batch, int cout, int k, int t_in, int t_out,
                                int t_y, int stride, int pad_left, int lrelu, int accumulate, int ostride, int ooff,
                                void* stream) {
    if (!x0 || !w || !y) return fail(WUN_ERR_INVALID, "null argument");
    if (stride != 1 && stride != 2) return fail(WUN_ERR_UNSUPPORTED, "stride must be 1 or 2");
    if (c0 < 1 || c1 < 0 || (c1 > 0 && !x1)) return fail(WUN_ERR_INVALID, "bad source channels");
    if (ostride < 1 || ooff < 0 || (long long)(t_out - 1) * ostride + ooff >= t_y) return fail(WUN_ERR_INVALID, "output does not fit t_y");
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.B = batch; a.ostride = ostride;
    a.src0 = x0; a.bs0 = (long long)c0 * t_in; a.pitch0 = t_in; a.C0 = c0;
    if (c1 > 0) { a.src1 = x1; a.bs1 = (long long)c1 * t_in; a.pitch1 = t_in; a.C1 = c1; }
    a.loader = stride == 2 ? LOADER_DEINT : LOADER_DIRECT;
    a.Tin = t_in; a.shift = pad_left; a.W = w; a.bias = bias; a.KW = k; a.N = a.N0 = cout; a.Tout = t_out;
    a.flags = (lrelu ? F_LRELU : 0) | (accumulate ? F_ACCUM : 0);
    a.dst0 = y; a.obs0 = (long long)cout * t_y; a.opitch0 = t_y; a.ooff0 = ooff; a.msk0 = mask;
    if (g_op_copy0 != nullptr) {
        a.dec = g_op_copy0; a.decpitch = g_op_copy_t0; a.decbs = (long long)cout * g_op_copy_t0;
        a.dec_exp = g_op_copy_exp; a.dec_lo = g_op_copy_lo; a.dec_len = (unsigned)g_op_copy_len;
    }
    if (g_op_copy1 != nullptr) { a.dec1 = g_op_copy1; a.dec1pitch = g_op_copy_t1; a.dec1bs = (long long)cout * g_op_copy_t1; }
    if (accumulate && g_op_acc_len > 0) { a.acc_lo = g_op_acc_lo; a.acc_len = (unsigned)g_op_acc_len; }
    if (g_op_ups_y != nullptr) {
        // wun_op_set_conv_upsample: what the plan asks of a level's last conv (wun_forward.hip) -- the split-K epilogue also
        // writes the 2x upsampled copy; a launch that does not end there is followed by the stand-alone kernel, as in the plan
        if (g_op_ups_tup != 2 * t_out - 1 && g_op_ups_tup != 2 * t_out) return fail(WUN_ERR_INVALID, "ups_tup must be 2 t_out - 1 or 2 t_out");
        if (stride != 1 || ostride != 1 || ooff != 0 || accumulate || mask) return fail(WUN_ERR_INVALID, "fused upsampling: plain forward launches only");
        if ((reinterpret_cast<uintptr_t>(g_op_ups_y) & 15) != 0) return fail(WUN_ERR_INVALID, "fused upsampling: ups_y must be 16-byte aligned");
        a.ups_y = g_op_ups_y; a.ups_pitch = g_op_ups_pitch; a.ups_bs = (long long)cout * g_op_ups_pitch;
        a.ups_tup = g_op_ups_tup; a.ups_w = g_op_ups_w;
    }
    HIP_TRY(op_launch_conv(a, (hipStream_t)stream));
    if (a.ups_y != nullptr) {
        t_op_epilogue_path = conv_last_fused_ups() ? WUN_PATH_FUSED : WUN_PATH_NOT_FUSED;
        if (!conv_last_fused_ups()) {
            UpsampleArgs u;
            memset(&u, 0, sizeof(u));
            u.x = y; u.xpitch = t_y; u.xbs = (long long)cout * t_y; u.n = t_out;
            u.y = a.ups_y; u.ypitch = a.ups_pitch; u.ybs = a.ups_bs; u.tup = a.ups_tup; u.w = a.ups_w;
            u.C = cout; u.B = batch; u.context = (a.ups_tup & 1);
            HIP_TRY(launch_upsample(u, (hipStream_t)stream));
        }
    }
    return WUN_OK;
}

extern "C" int wun_op_set_conv_upsample(float* ups_y, int ups_pitch, int ups_tup, const float* ups_w) {
    if (ups_y && (ups_tup < 1 || ups_pitch < ups_tup)) return fail(WUN_ERR_INVALID, "bad upsampled-copy geometry");
    g_op_ups_y = ups_y; g_op_ups_pitch = ups_pitch; g_op_ups_tup = ups_tup; g_op_ups_w = ups_y ? ups_w : nullptr;
    return WUN_OK;
}

// Input gradient of an up conv whose input is concat(skip, upsampled) with LINEAR upsampling, as the plan launches it
// (wun_backward.hip): a bias-free, activation-free stride-1 conv over dz with the transposed weights wt [k][cin][n_skip + n_cur];
// output columns < n_skip go to d_skip, the others are d(upsampled tensor).  A launch that ends in the split-K epilogue applies
// the adjoint of the upsampling there (ConvArgs.ubw_*) and never stores d_up; any other launch stores d_up and is followed by
// the stand-alone adjoint kernel.  Either way dz_prev[b][c][0 .. n) is written.
extern "C" int wun_op_conv1d_upsample_adjoint(const float* dz, const float* wt, float* d_skip, float* d_up, float* dz_prev,
                                              const float* x_prev, int batch, int cin, int n_skip, int n_cur, int k, int t_in,
                                              int tup, int pad_left, int n, int prev_pitch, void* stream) {
    if (!dz || !wt || !d_skip || !d_up || !dz_prev || !x_prev) return fail(WUN_ERR_INVALID, "null argument");
    if (batch < 1 || cin < 1 || n_skip < 1 || n_cur < 1 || k < 1 || t_in < 1 || n < 1) return fail(WUN_ERR_INVALID, "bad shape");
    if (tup != 2 * n - 1 && tup != 2 * n) return fail(WUN_ERR_INVALID, "tup must be 2n - 1 or 2n");
    if (prev_pitch < n) return fail(WUN_ERR_INVALID, "pitch below length");
    hipStream_t s = (hipStream_t)stream;
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.B = batch; a.ostride = 1;
    op_src(a, dz, cin, t_in);
    a.loader = LOADER_DIRECT;
    a.Tin = t_in; a.shift = pad_left; a.W = wt; a.KW = k; a.N = n_skip + n_cur; a.N0 = n_skip; a.Tout = tup;
    a.dst0 = d_skip; a.obs0 = (long long)n_skip * tup; a.opitch0 = tup;
    a.dst1 = d_up; a.obs1 = (long long)n_cur * tup; a.opitch1 = tup;
    a.ubw_dz = dz_prev; a.ubw_x = x_prev; a.ubw_pitch = prev_pitch; a.ubw_bs = (long long)n_cur * prev_pitch; a.ubw_n = n;
    HIP_TRY(op_launch_conv(a, s));
    t_op_epilogue_path = conv_last_fused_ups() ? WUN_PATH_FUSED : WUN_PATH_NOT_FUSED;
    if (!conv_last_fused_ups()) {
        UpsampleBwdArgs ub;
        memset(&ub, 0, sizeof(ub));
        ub.dy = d_up; ub.ypitch = tup; ub.ybs = (long long)n_cur * tup; ub.tup = tup;
        ub.x = x_prev; ub.xpitch = prev_pitch; ub.xbs = (long long)n_cur * prev_pitch; ub.n = n;
        ub.dz = dz_prev; ub.C = n_cur; ub.B = batch; ub.context = (tup & 1);
        HIP_TRY(launch_upsample_bwd(ub, s));
    }
    return WUN_OK;
}

// ---------------------------------------------------------------------------------------
// the elementwise family (wun_elementwise.hip) as single operators: thin wrappers that fill the launchers' argument structs.
// Every check runs before any GPU work; no alignment is asked of pointers or pitches (the scalar forms serve those).
// ---------------------------------------------------------------------------------------
static const char* op_updown_check(const void* a, const void* b, int B, int C, int n, int tup, int xpitch, int ypitch) {
    if (!a || !b) return "null argument";
    if (B < 1 || C < 1 || n < 1) return "bad shape";
    if (tup != 2 * n - 1 && tup != 2 * n) return "tup must be 2n - 1 or 2n";
    if (tup < 1) return "bad shape";
    if (xpitch < n || ypitch < tup) return "pitch below length";
    return nullptr;
}

extern "C" int wun_op_upsample(const void* x, void* y, const float* w, int B, int C, int n, int tup, int xpitch, int ypitch,
                               int bf16, void* stream) {
    if (const char* why = op_updown_check(x, y, B, C, n, tup, xpitch, ypitch)) return fail(WUN_ERR_INVALID, why);
    UpsampleArgs u;
    memset(&u, 0, sizeof(u));
    u.x = reinterpret_cast<const float*>(x); u.xpitch = xpitch; u.xbs = (long long)C * xpitch; u.n = n;
    u.y = reinterpret_cast<float*>(y); u.ypitch = ypitch; u.ybs = (long long)C * ypitch; u.tup = tup;
    u.w = w; u.C = C; u.B = B; u.context = (tup & 1); u.bf = bf16 ? 1 : 0;
    HIP_TRY(launch_upsample(u, (hipStream_t)stream));
    return WUN_OK;
}

extern "C" int wun_op_upsample_backward(const void* dy, const void* x, void* dz, const float* w, float* dw, float* dw_partial,
                                        int B, int C, int n, int tup, int ypitch, int xpitch, int bf16, int accumulate,
                                        void* stream) {
    if (const char* why = op_updown_check(dy, x, B, C, n, tup, xpitch, ypitch)) return fail(WUN_ERR_INVALID, why);
    if (!dz) return fail(WUN_ERR_INVALID, "null argument");
    if (dw && !w) return fail(WUN_ERR_INVALID, "dw without w");
    UpsampleBwdArgs ub;
    memset(&ub, 0, sizeof(ub));
    ub.dy = reinterpret_cast<const float*>(dy); ub.ypitch = ypitch; ub.ybs = (long long)C * ypitch; ub.tup = tup;
    ub.x = reinterpret_cast<const float*>(x); ub.xpitch = xpitch; ub.xbs = (long long)C * xpitch; ub.n = n;
    ub.dz = reinterpret_cast<float*>(dz); ub.w = w; ub.dw = dw; ub.dw_partial = dw ? dw_partial : nullptr;
    ub.C = C; ub.B = B; ub.context = (tup & 1); ub.bf = bf16 ? 1 : 0;
    HIP_TRY(launch_upsample_bwd(ub, (hipStream_t)stream));
    if (w && dw) HIP_TRY(launch_interp_grad(ub, (hipStream_t)stream, accumulate != 0));
    return WUN_OK;
}

extern "C" int32_t wun_op_head_abi_size(void) { return (int32_t)sizeof(wun_op_head_desc); }

// fills HeadArgs from the descriptor; null = fine, else why not
static const char* op_head_args(const wun_op_head_desc* d, const float* mix, const void* feat, const float* params,
                                const int64_t* hoff, HeadArgs& h, long long* off) {
    if (!d || !feat || !params || !hoff) return "null argument";
    if (d->difference != 0 && d->difference != 1) return "difference must be 0 or 1";
    const int Sh = d->S - d->difference;
    if (d->C < 1 || d->C > 2 || Sh < 1 || Sh > 4 || Sh * d->C > 8) return "C must be 1 or 2, 1..4 head sources, Sh * C <= 8";
    if (d->F < 1 || d->Ko < 1 || d->padl < 0 || d->padl >= d->Ko || d->Tfeat < 1 || d->Tout < 1 || d->B < 1) return "bad shape";
    if (d->feat_pitch < d->Tfeat || d->dpre_pitch < d->Tout) return "pitch below length";
    if (mix && (d->mix_off_feat < 0 || d->mix_off_diff < 0 || d->mix_pitch < d->mix_off_feat + d->Tfeat ||
                (d->difference && d->mix_pitch < d->mix_off_diff + d->Tout))) return "pitch below length";
    if ((long long)Sh * ((long long)d->Ko * (d->C + d->F) * d->C + d->C) * 4 > 64 * 1024) return "head parameters exceed the LDS";
    for (int i = 0; i < Sh; ++i)
        if (hoff[i] < 0) return "negative parameter offset";
    memset(&h, 0, sizeof(h));
    h.mix_ncw = mix; h.mpitch = d->mix_pitch; h.mbs = (long long)d->C * d->mix_pitch;
    h.moff_feat = d->mix_off_feat; h.moff_diff = d->mix_off_diff;
    h.feat = reinterpret_cast<const float*>(feat); h.fpitch = d->feat_pitch; h.fbs = (long long)d->F * d->feat_pitch;
    h.Wh = params;
    h.C = d->C; h.F = d->F; h.S = d->S; h.Sh = Sh; h.Ko = d->Ko; h.padl = d->padl;
    h.Tfeat = d->Tfeat; h.Tout = d->Tout; h.B = d->B;
    h.tanh_act = d->tanh ? 1 : 0; h.difference = d->difference; h.training = d->training ? 1 : 0;
    h.dppitch = d->dpre_pitch; h.dpbs = (long long)d->C * d->dpre_pitch; h.dps = (long long)d->B * h.dpbs;
    h.gscale = 2.0f / ((float)d->S * (float)d->B * (float)d->Tout * (float)d->C);
    h.featbf = d->feat_bf16 ? 1 : 0;
    for (int i = 0; i < 4; ++i) off[i] = i < Sh ? (long long)hoff[i] : 0;
    return nullptr;
}

extern "C" int wun_op_head_forward(const wun_op_head_desc* desc, const float* mix, const void* feat, const float* params,
                                   const int64_t* hoff, float* out, void* stream) {
    HeadArgs h;
    long long off[4];
    if (!mix || !out) return fail(WUN_ERR_INVALID, "null argument");
    if (const char* why = op_head_args(desc, mix, feat, params, hoff, h, off)) return fail(WUN_ERR_INVALID, why);
    h.out = out;
    HIP_TRY(launch_head_fwd_off(h, off, (hipStream_t)stream));
    return WUN_OK;
}

extern "C" int wun_op_head_loss_backward(const wun_op_head_desc* desc, const void* feat, const float* params, const int64_t* hoff,
                                         const float* out, const float* targets, float* dpre, void* dzfeat, float* loss,
                                         void* stream) {
    HeadArgs h;
    long long off[4];
    if (!out || !targets || !dpre || !dzfeat || !loss) return fail(WUN_ERR_INVALID, "null argument");
    if (const char* why = op_head_args(desc, nullptr, feat, params, hoff, h, off)) return fail(WUN_ERR_INVALID, why);
    h.out = const_cast<float*>(out); h.tgt = targets; h.dpre = dpre; h.dzfeat = reinterpret_cast<float*>(dzfeat);
    h.loss_partial = op_scratch();
    if (!h.loss_partial) return fail(WUN_ERR_NOMEM, "operator scratch");
    HIP_TRY(launch_head_bwd_off(h, off, (hipStream_t)stream));
    HIP_TRY(launch_loss_finish(h.loss_partial, head_bwd_blocks(h),
                               1.0f / ((float)h.S * (float)h.B * (float)h.Tout * (float)h.C), loss, (hipStream_t)stream));
    return WUN_OK;
}

extern "C" int wun_op_head_backward(const wun_op_head_desc* desc, const void* feat, const float* params, const int64_t* hoff,
                                    const float* out, const float* d_outputs, float* dpre, void* dzfeat, void* stream) {
    HeadArgs h;
    long long off[4];
    if (!out || !d_outputs || !dpre || !dzfeat) return fail(WUN_ERR_INVALID, "null argument");
    if (const char* why = op_head_args(desc, nullptr, feat, params, hoff, h, off)) return fail(WUN_ERR_INVALID, why);
    h.out = const_cast<float*>(out); h.dout = d_outputs; h.dpre = dpre; h.dzfeat = reinterpret_cast<float*>(dzfeat);
    HIP_TRY(launch_head_grad_off(h, off, (hipStream_t)stream));
    return WUN_OK;
}

extern "C" int wun_op_btc_to_ncw(const float* src, float* dst, int B, int T, int C, int pitch, void* stream) {
    if (!src || !dst) return fail(WUN_ERR_INVALID, "null argument");
    if (B < 1 || T < 1 || C < 1) return fail(WUN_ERR_INVALID, "bad shape");
    if (pitch < T) return fail(WUN_ERR_INVALID, "pitch below length");
    HIP_TRY(launch_btc_to_ncw(src, dst, B, T, C, pitch, (hipStream_t)stream));
    return WUN_OK;
}

extern "C" int wun_op_last_path(int op) {
    switch (op) {
        case WUN_OP_UPSAMPLE: return elementwise_last_path(EW_UPSAMPLE);
        case WUN_OP_UPSAMPLE_BACKWARD: return elementwise_last_path(EW_UPSAMPLE_BWD);
        case WUN_OP_INTERP_GRAD: return elementwise_last_path(EW_INTERP_GRAD);
        case WUN_OP_HEAD_FORWARD: return elementwise_last_path(EW_HEAD_FWD);
        case WUN_OP_HEAD_DFEAT: return elementwise_last_path(EW_HEAD_DFEAT);
        case WUN_OP_BTC_TO_NCW: return elementwise_last_path(EW_BTC_TO_NCW);
        case WUN_OP_CONV_EPILOGUE: return t_op_epilogue_path;
        case WUN_OP_FIRST_CONV: return t_op_first_conv_path;
        case WUN_OP_WGRAD: return t_op_wgrad_path;
        default: return fail(WUN_ERR_INVALID, "unknown operator");
    }
}
static_assert(EW_PATH_SCALAR == WUN_PATH_SCALAR && EW_PATH_VEC4 == WUN_PATH_VEC4 && EW_PATH_VEC8_BF16 == WUN_PATH_VEC8_BF16 &&
              EW_PATH_ONE_STAGE == WUN_PATH_ONE_STAGE && EW_PATH_TWO_STAGE == WUN_PATH_TWO_STAGE &&
              EW_PATH_GENERIC == WUN_PATH_GENERIC && EW_PATH_FOUR_POSITION == WUN_PATH_FOUR_POSITION, "wun.h path values");

extern "C" int wun_op_set_conv_copies(float* copy0, int t0, int expand, int exp_lo, int exp_len, float* copy1, int t1,
                                      int acc_lo, int acc_len) {
    if ((copy0 && t0 < 1) || (copy1 && t1 < 1) || exp_len < 0 || acc_len < 0) return fail(WUN_ERR_INVALID, "bad copy geometry");
    g_op_copy0 = copy0; g_op_copy_t0 = t0; g_op_copy_exp = expand ? 1 : 0; g_op_copy_lo = exp_lo; g_op_copy_len = exp_len;
    g_op_copy1 = copy1; g_op_copy_t1 = t1; g_op_acc_lo = acc_lo; g_op_acc_len = acc_len;
    return WUN_OK;
}

// bf16-MFMA conv as a single operator: packs w (fp32 [K][Cin][Cout]) into the bf16 image in `scratch`
// (>= wun_op_conv1d_bf16_scratch floats), then runs the bf16 kernel.  Same semantics as wun_op_conv1d.
extern "C" int64_t wun_op_conv1d_bf16_scratch(int cin, int cout, int k) {
    return (int64_t)k * bf16_image_groups(cin) * ((cout + 63) / 64 * 64) * 4 + 64;
}

extern "C" int wun_op_conv1d_bf16(const float* x, const float* w, const float* bias, float* y, float* scratch,
                                  int batch, int cin, int cout, int k, int t_in, int t_out, int stride, int pad_left,
                                  int lrelu, void* stream) {
    if (!x || !w || !y || !scratch) return fail(WUN_ERR_INVALID, "null argument");
    if (stride != 1 && stride != 2) return fail(WUN_ERR_UNSUPPORTED, "stride must be 1 or 2");
    hipStream_t s = (hipStream_t)stream;
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.B = batch; a.ostride = 1;
    op_src(a, x, cin, t_in);
    a.loader = stride == 2 ? LOADER_DEINT : LOADER_DIRECT;
    a.Tin = t_in; a.shift = pad_left; a.bias = bias; a.KW = k; a.N = a.N0 = cout; a.Tout = t_out;
    a.flags = lrelu ? F_LRELU : 0;
    a.dst0 = y; a.obs0 = (long long)cout * t_out; a.opitch0 = t_out;
    // the kernel reads bf16 rows: convert x (fp32 output, obf = 0, keeps the comparison with float64 sharp)
    a.pitch0 = pad8(t_in); a.bs0 = (long long)cin * a.pitch0; a.xbf = 1; a.obf = 0;
    if (!conv_bf16_supported(a)) return fail(WUN_ERR_UNSUPPORTED, "shape not served by the bf16 kernel (cin < 8 or k > 15)");
    if (!op_force_bf16(a)) return fail(WUN_ERR_UNSUPPORTED, "forced bf16 tile code refused for this launch");
    a.src0 = op_to_bf16(0, x, (long long)batch * cin, t_in, t_in, s);
    if (!a.src0) return fail(WUN_ERR_NOMEM, "bf16 temporary");
    float* img = (float*)(((uintptr_t)scratch + 255) & ~(uintptr_t)255);
    PackDesc d;
    d.src_off = 0; d.src_in_ws = 0; d.dst_off = 0; d.KW = k; d.C = cin; d.N = cout;
    d.C8p = bf16_image_groups(cin); d.Npad = (cout + 63) / 64 * 64;
    PackDesc* dd = nullptr;
    HIP_TRY(hipMalloc((void**)&dd, sizeof(PackDesc)));
    hipError_t e = hipMemcpyAsync(dd, &d, sizeof(d), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_pack_bf16(w, img, dd, 1, (long long)k * d.C8p * d.Npad, s);
    a.W = img; a.wb_c8p = d.C8p; a.wb_npad = d.Npad;
    if (e == hipSuccess) e = launch_conv_bf16(a, s, wun_switches_from_env());
    (void)hipStreamSynchronize(s);
    (void)hipFree(dd);
    HIP_TRY(e);
    return WUN_OK;
}

// Input gradient of the bf16 speed mode as a single operator (wun_op_conv1d_dgrad semantics): stride 1 = the
// bf16 conv on tap-flipped / transposed weights, stride 2 = the fused two-phase transposed conv (a lane owns 8
// consecutive outputs).  scratch: >= wun_op_conv1d_dgrad_bf16_scratch floats.  Synchronises the stream.
extern "C" int64_t wun_op_conv1d_dgrad_bf16_scratch(int cin, int cout, int k) {
    const int64_t wt = 2ll * (k + 1) * cin * cout + 64;                                       // transposed fp32 copy
    const int64_t img = (int64_t)(k + 1) * bf16_image_groups(cout) * ((2 * cin + 32 + 63) / 64 * 64) * 4 + 64;
    return wt + img + 128;
}

extern "C" int wun_op_conv1d_dgrad_bf16(const float* dz, const float* w, float* dx, float* scratch, int batch, int cin,
                                        int cout, int k, int t_in, int t_out, int stride, int pad_left, void* stream) {
    if (!dz || !w || !dx || !scratch) return fail(WUN_ERR_INVALID, "null argument");
    if (stride != 1 && stride != 2) return fail(WUN_ERR_UNSUPPORTED, "stride must be 1 or 2");
    if (stride == 2 && (pad_left != 0 || (cin & 3) != 0)) return fail(WUN_ERR_UNSUPPORTED, "stride-2: pad_left 0 and cin % 4 == 0 only");
    hipStream_t s = (hipStream_t)stream;
    float* wt = (float*)(((uintptr_t)scratch + 255) & ~(uintptr_t)255);
    float* img = (float*)(((uintptr_t)(wt + 2ll * (k + 1) * cin * cout) + 255) & ~(uintptr_t)255);
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.B = batch; a.ostride = 1;
    op_src(a, dz, cout, t_out);
    a.Tin = t_out; a.N = a.N0 = cin;
    a.dst0 = dx; a.obs0 = (long long)cin * t_in; a.opitch0 = t_in;
    WtDesc d; d.src_off = 0; d.dst_off = 0; d.C = cin; d.N = cout;
    PackDesc pd; pd.src_off = 0; pd.src_in_ws = 0; pd.dst_off = 0; pd.C = cout;
    if (stride == 1) {
        d.J = k; d.k_last = k - 1; d.k_step = 1; d.mode = 0;
        a.shift = k - 1 - pad_left; a.KW = k; a.Tout = t_in;
        pd.KW = k; pd.N = cin; pd.Npad = (cin + 63) / 64 * 64;
    } else {
        const int J0 = (k + 1) / 2;
        d.J = J0; d.k_last = 2 * (J0 - 1); d.k_step = k; d.mode = 1;
        a.KW = J0; a.kw_full = k; a.shift = J0 - 1; a.Tout = (t_in + 1) / 2; a.Tlim = t_in; a.flags = F_PHASE2;
        pd.KW = J0; pd.N = 2 * cin; pd.Npad = (2 * cin + 32 + 63) / 64 * 64;
    }
    pd.C8p = bf16_image_groups(cout);
    a.pitch0 = pad8(t_out); a.bs0 = (long long)cout * a.pitch0; a.xbf = 1; a.obf = 0;
    if (!conv_bf16_supported(a)) return fail(WUN_ERR_UNSUPPORTED, "shape not served by the bf16 kernel");
    if (!op_force_bf16(a)) return fail(WUN_ERR_UNSUPPORTED, "forced bf16 tile code refused for this launch");
    a.src0 = op_to_bf16(0, dz, (long long)batch * cout, t_out, t_out, s);
    if (!a.src0) return fail(WUN_ERR_NOMEM, "bf16 temporary");
    HIP_TRY(launch_make_wt_one(w, wt, d, s));
    PackDesc* dd = nullptr;
    HIP_TRY(hipMalloc((void**)&dd, sizeof(PackDesc)));
    hipError_t e = hipMemcpyAsync(dd, &pd, sizeof(pd), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_pack_bf16(wt, img, dd, 1, (long long)pd.KW * pd.C8p * pd.Npad, s);
    a.W = img; a.wb_c8p = pd.C8p; a.wb_npad = pd.Npad;
    if (e == hipSuccess) e = launch_conv_bf16(a, s, wun_switches_from_env());
    (void)hipStreamSynchronize(s);
    (void)hipFree(dd);
    HIP_TRY(e);
    return WUN_OK;
}

// ---------------------------------------------------------------------------------------
// The plan's bf16 conv launch as a single operator on rows the caller made (wun.h: wun_op_conv_bf16_desc), and the
// audio-input conv.  Test hooks: what the plan runs -- bf16 stores, masks, ranged accumulate, the column split, the compact
// copy, crop windows at any first-element offset -- reachable tile by tile.
// ---------------------------------------------------------------------------------------
extern "C" int32_t wun_op_conv_bf16_abi_size(void) { return (int32_t)sizeof(wun_op_conv_bf16_desc); }

// fills the shape side of ConvArgs (no pointers) from the descriptor; null = fine, else why not (WUN_ERR_INVALID)
static const char* op_conv_bf16_shape(const wun_op_conv_bf16_desc* d, ConvArgs& a) {
    if (!d) return "null argument";
    if (d->mode < 0 || d->mode > 2) return "mode must be 0, 1 or 2";
    if (d->B < 1 || d->C0 < 1 || d->C1 < 0 || d->N < 1 || d->K < 1 || d->Tin < 1 || d->Tout < 1) return "bad shape";
    if (d->N0 < 1 || d->N0 > d->N) return "N0 must be in 1..N";
    if (d->x_off < 0 || d->y0_off < 0 || d->y1_off < 0 || d->acc_len < 0) return "negative offset or length";
    if ((long long)d->x_off + d->Tin > d->x0_pitch || (d->C1 > 0 && (long long)d->x_off + d->Tin > d->x1_pitch)) return "input row does not fit its pitch";
    if ((long long)d->y0_off + d->Tout > d->y0_pitch || (d->N0 < d->N && (long long)d->y1_off + d->Tout > d->y1_pitch)) return "output row does not fit its pitch";
    if (d->dec_pitch != 0 && d->dec_pitch < (d->Tout + 1) / 2) return "dec_pitch below the copy's length";
    if (d->mode == 2 && (d->shift != 0 || d->C1 != 0 || d->N0 != d->N || (d->N & 3) != 0 || d->lrelu || d->dec_pitch != 0))
        return "two-phase form: shift 0, one source, one destination, N % 4 == 0, no lrelu, no dec";
    if (d->mode == 2 && d->Tout > 2ll * d->Tin + d->K) return "Tout larger than the transposed conv produces";
    memset(&a, 0, sizeof(a));
    a.B = d->B; a.ostride = 1;
    a.C0 = d->C0; a.pitch0 = d->x0_pitch; a.bs0 = (long long)d->C0 * d->x0_pitch; a.off0 = d->x_off;
    if (d->C1 > 0) { a.C1 = d->C1; a.pitch1 = d->x1_pitch; a.bs1 = (long long)d->C1 * d->x1_pitch; a.off1 = d->x_off; }
    a.loader = d->mode == 1 ? LOADER_DEINT : LOADER_DIRECT;
    a.Tin = d->Tin; a.N = d->N; a.N0 = d->N0;
    if (d->mode == 2) {          // as wun_op_conv1d_dgrad_bf16 sets it up
        const int J0 = (d->K + 1) / 2;
        a.KW = J0; a.kw_full = d->K; a.shift = J0 - 1; a.Tout = (d->Tout + 1) / 2; a.Tlim = d->Tout; a.flags = F_PHASE2;
    } else {
        a.KW = d->K; a.shift = d->shift; a.Tout = d->Tout;
        a.flags = d->lrelu ? F_LRELU : 0;
    }
    if (d->accumulate) { a.flags |= F_ACCUM; a.acc_lo = d->acc_lo; a.acc_len = (unsigned)d->acc_len; }
    a.opitch0 = d->y0_pitch; a.obs0 = (long long)d->N0 * d->y0_pitch; a.ooff0 = d->y0_off;
    if (d->N0 < d->N) { a.opitch1 = d->y1_pitch; a.obs1 = (long long)(d->N - d->N0) * d->y1_pitch; a.ooff1 = d->y1_off; }
    if (d->dec_pitch != 0) { a.decpitch = d->dec_pitch; a.decbs = (long long)d->N0 * d->dec_pitch; }
    a.xbf = 1; a.obf = d->out_bf16 ? 1 : 0;
    return nullptr;
}

extern "C" int wun_op_conv_bf16_choice_ok(const wun_op_conv_bf16_desc* desc, int code) {
    ConvArgs a;
    if (const char* why = op_conv_bf16_shape(desc, a)) return fail(WUN_ERR_INVALID, why);
    if (code < 0 || code >= 27) return 0;
    return conv_bf16_choice_ok(a, kBf16VariantBase + code) ? 1 : 0;
}

extern "C" int64_t wun_op_conv_bf16_ex_scratch(const wun_op_conv_bf16_desc* d) {
    if (!d) return fail(WUN_ERR_INVALID, "null argument");
    return d->mode == 2 ? wun_op_conv1d_dgrad_bf16_scratch(d->N, d->C0, d->K) : wun_op_conv1d_bf16_scratch(d->C0 + d->C1, d->N, d->K);
}

extern "C" int wun_op_conv_bf16_ex(const wun_op_conv_bf16_desc* d, const void* x0, const void* x1, const float* w, const float* bias,
                                   void* y0, void* y1, const void* mask0, const void* mask1, void* dec, float* scratch,
                                   void* stream) {
    ConvArgs a;
    if (const char* why = op_conv_bf16_shape(d, a)) return fail(WUN_ERR_INVALID, why);
    if (!x0 || !w || !y0 || !scratch || (d->C1 > 0 && !x1) || (d->N0 < d->N && !y1)) return fail(WUN_ERR_INVALID, "null argument");
    if ((dec != nullptr) != (d->dec_pitch != 0)) return fail(WUN_ERR_INVALID, "dec and dec_pitch go together");
    if (d->mode == 2 && bias) return fail(WUN_ERR_INVALID, "two-phase form: no bias");
    if (mask1 && !(d->N0 < d->N)) return fail(WUN_ERR_INVALID, "mask1 without a second destination");
    if (!aligned16(x0) || (d->C1 > 0 && !aligned16(x1))) return fail(WUN_ERR_INVALID, "input rows must be 16-byte aligned");
    const int esz = d->out_bf16 ? 2 : 4;
    if ((reinterpret_cast<uintptr_t>(y0) % esz) || (y1 && reinterpret_cast<uintptr_t>(y1) % esz) ||
        (dec && reinterpret_cast<uintptr_t>(dec) % esz)) return fail(WUN_ERR_INVALID, "output not aligned to its element");
    a.src0 = reinterpret_cast<const float*>(x0);
    if (d->C1 > 0) a.src1 = reinterpret_cast<const float*>(x1);
    a.bias = bias;
    a.dst0 = reinterpret_cast<float*>(y0); a.msk0 = reinterpret_cast<const float*>(mask0);
    if (d->N0 < d->N) { a.dst1 = reinterpret_cast<float*>(y1); a.msk1 = reinterpret_cast<const float*>(mask1); }
    a.dec = reinterpret_cast<float*>(dec);
    if (!conv_bf16_supported(a)) return fail(WUN_ERR_UNSUPPORTED, "shape not served by the bf16 kernel");
    if (!op_force_bf16(a)) return fail(WUN_ERR_UNSUPPORTED, "forced bf16 tile code refused for this launch");
    hipStream_t s = (hipStream_t)stream;
    const int Ctot = d->C0 + d->C1;
    PackDesc pd; pd.src_off = 0; pd.src_in_ws = 0; pd.dst_off = 0;
    const float* wsrc = w;
    float* img;
    if (d->mode == 2) {
        // forward weights [K][cin = N][cout = C0] -> the two-phase transposed copy -> its packed image (wun_op_conv1d_dgrad_bf16)
        const int cin = d->N, cout = d->C0, k = d->K;
        float* wt = (float*)(((uintptr_t)scratch + 255) & ~(uintptr_t)255);
        img = (float*)(((uintptr_t)(wt + 2ll * (k + 1) * cin * cout) + 255) & ~(uintptr_t)255);
        WtDesc wd; wd.src_off = 0; wd.dst_off = 0; wd.C = cin; wd.N = cout;
        wd.J = a.KW; wd.k_last = 2 * (a.KW - 1); wd.k_step = k; wd.mode = 1;
        HIP_TRY(launch_make_wt_one(w, wt, wd, s));
        wsrc = wt;
        pd.C = cout; pd.KW = a.KW; pd.N = 2 * cin; pd.Npad = (2 * cin + 32 + 63) / 64 * 64;
    } else {
        img = (float*)(((uintptr_t)scratch + 255) & ~(uintptr_t)255);
        pd.C = Ctot; pd.KW = d->K; pd.N = d->N; pd.Npad = (d->N + 63) / 64 * 64;
    }
    pd.C8p = bf16_image_groups(pd.C);
    PackDesc* dd = nullptr;
    HIP_TRY(hipMalloc((void**)&dd, sizeof(PackDesc)));
    hipError_t e = hipMemcpyAsync(dd, &pd, sizeof(pd), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_pack_bf16(wsrc, img, dd, 1, (long long)pd.KW * pd.C8p * pd.Npad, s);
    a.W = img; a.wb_c8p = pd.C8p; a.wb_npad = pd.Npad;
    if (e == hipSuccess) e = launch_conv_bf16(a, s, wun_switches_from_env());
    (void)hipStreamSynchronize(s);
    (void)hipFree(dd);
    HIP_TRY(e);
    return WUN_OK;
}

extern "C" int wun_op_first_conv(const float* x, const float* w, const float* bias, void* y, void* dec, int batch, int cin,
                                 int cout, int k, int t_in, int t_out, int stride, int pad_left, int lrelu, int out_bf16,
                                 int x_pitch, int y_pitch, int dec_pitch, void* stream) {
    if (!x || !w || !y) return fail(WUN_ERR_INVALID, "null argument");
    if (batch < 1 || cin < 1 || cout < 1 || k < 1 || t_in < 1 || t_out < 1 || pad_left < 0) return fail(WUN_ERR_INVALID, "bad shape");
    if (stride != 1 && stride != 2) return fail(WUN_ERR_UNSUPPORTED, "stride must be 1 or 2");
    if (x_pitch < t_in || y_pitch < t_out || (dec && dec_pitch < (t_out + 1) / 2)) return fail(WUN_ERR_INVALID, "pitch below length");
    if (dec && (reinterpret_cast<uintptr_t>(dec) % (out_bf16 ? 2 : 4))) return fail(WUN_ERR_INVALID, "dec not aligned to its element");
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.B = batch; a.ostride = 1;
    a.src0 = x; a.bs0 = (long long)cin * x_pitch; a.pitch0 = x_pitch; a.C0 = cin;
    a.loader = stride == 2 ? LOADER_DEINT : LOADER_DIRECT;
    a.Tin = t_in; a.shift = pad_left; a.W = w; a.bias = bias; a.KW = k; a.N = a.N0 = cout; a.Tout = t_out;
    a.flags = lrelu ? F_LRELU : 0;
    a.dst0 = reinterpret_cast<float*>(y); a.obs0 = (long long)cout * y_pitch; a.opitch0 = y_pitch;
    if (dec) { a.dec = reinterpret_cast<float*>(dec); a.decpitch = dec_pitch; a.decbs = (long long)cout * dec_pitch; }
    a.obf = out_bf16 ? 1 : 0;
    if (!first_conv_supported(a)) return fail(WUN_ERR_UNSUPPORTED, "shape not served by the audio-input conv kernel");
    HIP_TRY(launch_first_conv(a, (hipStream_t)stream));
    t_op_first_conv_path = WUN_PATH_FIRST_CONV;
    return WUN_OK;
}

// ---------------------------------------------------------------------------------------
// A layer's weight gradient as the plan launches it (run_wgrad / run_narrow_wgrad of wun_dispatch.hip) on rows the caller made
// (wun.h: wun_op_wgrad_desc).  Test hook: two sources with crop offsets, windows inside longer rows, two-part launches into
// one partial buffer, the direct epilogue, the accumulating instantiations, bf16 rows, the narrow kernels' plane / et forms.
// ---------------------------------------------------------------------------------------
extern "C" int32_t wun_op_wgrad_abi_size(void) { return (int32_t)sizeof(wun_op_wgrad_desc); }

struct OpWgrad {                 // a checked descriptor as the launchers' argument blocks
    bool narrow;
    int nparts, total, units[2];
    WgradArgs w[2];
    NarrowWgradArgs nw[2];
    long long woff[4], boff[4];
    long long part_floats;       // floats of one split in the partial buffer
};

// Every check of wun_op_wgrad_ex but the null pointers, then the argument blocks with geometry and split counts as run_wgrad /
// run_narrow_wgrad settle them.  Null row pointers count as aligned (the host-only callers pass none).  0 = fine.
static int op_wgrad_build(const wun_op_wgrad_desc* d, const void* x0, const void* x1, const void* dz0, const void* dz1,
                          const WunSwitches& sw, OpWgrad& o) {
    if (!d) return fail(WUN_ERR_INVALID, "null argument");
    if (d->family < WUN_WGRAD_LDS || d->family > WUN_WGRAD_NARROW) return fail(WUN_ERR_INVALID, "unknown kernel family");
    if (d->B < 1 || d->C0 < 1 || d->C1 < 0 || d->N < 1 || d->K < 1) return fail(WUN_ERR_INVALID, "bad shape");
    if (d->nparts != 1 && d->nparts != 2) return fail(WUN_ERR_INVALID, "nparts must be 1 or 2");
    const bool narrow = d->family == WUN_WGRAD_NARROW;
    if ((d->rows_bf16 != 0) != (d->family == WUN_WGRAD_BF16)) return fail(WUN_ERR_INVALID, "rows_bf16 goes with the bf16 family and no other");
    if ((d->x0_pitch & 3) || (d->C1 > 0 && (d->x1_pitch & 3))) return fail(WUN_ERR_INVALID, "row pitches must be multiples of 4 elements");
    if (!aligned16(x0) || (d->C1 > 0 && !aligned16(x1)) || !aligned16(dz0) || (d->nparts == 2 && !aligned16(dz1)))
        return fail(WUN_ERR_INVALID, "x0 / x1 / dz must be 16-byte aligned");
    for (int i = 0; i < d->nparts; ++i) {
        if (d->loader[i] != LOADER_DIRECT && d->loader[i] != LOADER_DEINT) return fail(WUN_ERR_INVALID, "loader must be 0 or 1");
        if (d->x0_off[i] < 0 || d->x1_off[i] < 0 || d->shift[i] < 0 || d->nsplit[i] < 0) return fail(WUN_ERR_INVALID, "negative offset, shift or split request");
        if (d->Tin[i] < 1 || d->Tq[i] < 1) return fail(WUN_ERR_INVALID, "bad shape");
        if (d->shift[i] >= d->K) return fail(WUN_ERR_INVALID, "shift must be below K");
        if ((long long)d->x0_off[i] + d->Tin[i] > d->x0_pitch || (d->C1 > 0 && (long long)d->x1_off[i] + d->Tin[i] > d->x1_pitch))
            return fail(WUN_ERR_INVALID, "window does not fit its pitch");
        if (d->Tq[i] > d->dz_pitch[i] || (d->dz_pitch[i] & 3)) return fail(WUN_ERR_INVALID, "dz_pitch must hold Tq and be a multiple of 4 elements");
    }
    int Nper = d->N;
    if (narrow) {
        if (d->planes < 1 || d->planes > 4 || d->N % d->planes != 0) return fail(WUN_ERR_INVALID, "planes must be in 1..4 and divide N");
        if (d->et & ~7) return fail(WUN_ERR_INVALID, "unknown et bits");
        if (d->zss < 0 || (d->zss & 3)) return fail(WUN_ERR_INVALID, "zss must be a non-negative multiple of 4 elements");
        if (d->force_mtw != 0 || d->force_nw != 0) return fail(WUN_ERR_INVALID, "the narrow family has no geometry to force");
        for (int s = 0; s < d->planes; ++s)
            if (d->plane_off[s] < 0) return fail(WUN_ERR_INVALID, "negative plane offset");
        Nper = d->N / d->planes;
    }
    // ---- what the plan never builds ----
    if (d->nparts == 2 && d->C1 > 0) return fail(WUN_ERR_UNSUPPORTED, "two parts with two sources: no layer of the plan launches this");
    for (int i = 0; i < d->nparts; ++i)
        if (d->shift[i] > 0 && (d->x0_off[i] != 0 || (d->C1 > 0 && d->x1_off[i] != 0)))
            return fail(WUN_ERR_UNSUPPORTED, "shift > 0 with a nonzero window offset: no layer of the plan launches this");
    memset(&o, 0, sizeof(o));
    o.narrow = narrow; o.nparts = d->nparts;
    const int Ctot = d->C0 + d->C1;
    if (narrow) {
        for (int i = 0; i < d->nparts; ++i) {
            NarrowWgradArgs& n = o.nw[i];
            n.src0 = reinterpret_cast<const float*>(x0); n.bs0 = (long long)d->C0 * d->x0_pitch; n.pitch0 = d->x0_pitch; n.off0 = d->x0_off[i]; n.C0 = d->C0;
            if (d->C1 > 0) { n.src1 = reinterpret_cast<const float*>(x1); n.bs1 = (long long)d->C1 * d->x1_pitch; n.pitch1 = d->x1_pitch; n.off1 = d->x1_off[i]; n.C1 = d->C1; }
            n.Tin = d->Tin[i]; n.shift = d->shift[i]; n.KW = d->K; n.stride = d->loader[i] == LOADER_DEINT ? 2 : 1;
            n.dz = reinterpret_cast<const float*>(i == 0 ? dz0 : dz1); n.zss = d->zss; n.dzbs = (long long)Nper * d->dz_pitch[i]; n.dzpitch = d->dz_pitch[i];
            n.N = d->N; n.Nper = Nper; n.Tq = d->Tq[i]; n.B = d->B; n.et = d->et;
            if (!narrow_wgrad_launch_ok(n, sw)) return fail(WUN_ERR_UNSUPPORTED, "shape or element types not served by the narrow weight-gradient kernels");
            o.units[i] = narrow_wgrad_units(n);
            n.nsplit = d->nsplit[i] > 0 ? std::min(d->nsplit[i], o.units[i]) : narrow_wgrad_pick_nsplit(n, sw);
            o.total += n.nsplit;
        }
        for (int s = 0; s < d->planes; ++s) { o.woff[s] = d->plane_off[s]; o.boff[s] = d->plane_off[s] + (long long)d->K * Ctot * Nper; }
        o.part_floats = narrow_wgrad_partial_floats(o.nw[0]);
        return WUN_OK;
    }
    for (int i = 0; i < d->nparts; ++i) {
        WgradArgs& w = o.w[i];
        w.B = d->B; w.loader = d->loader[i];
        w.src0 = reinterpret_cast<const float*>(x0); w.bs0 = (long long)d->C0 * d->x0_pitch; w.pitch0 = d->x0_pitch; w.off0 = d->x0_off[i]; w.C0 = d->C0;
        if (d->C1 > 0) { w.src1 = reinterpret_cast<const float*>(x1); w.bs1 = (long long)d->C1 * d->x1_pitch; w.pitch1 = d->x1_pitch; w.off1 = d->x1_off[i]; w.C1 = d->C1; }
        w.Tin = d->Tin[i]; w.shift = d->shift[i]; w.KW = d->K;
        w.dz = reinterpret_cast<const float*>(i == 0 ? dz0 : dz1); w.dzbs = (long long)d->N * d->dz_pitch[i]; w.dzpitch = d->dz_pitch[i]; w.N = d->N; w.Tq = d->Tq[i];
        w.bf16 = w.sbf = d->family == WUN_WGRAD_BF16 ? 1 : 0;
        w.win = d->family == WUN_WGRAD_WIN ? 1 : 0;
        w.accum = d->accumulate ? 1 : 0;
        if (w.bf16 && !wgrad_bf16_supported(w)) return fail(WUN_ERR_UNSUPPORTED, "shape not served by the bf16 weight-gradient kernel");
        if (w.win && !wgrad_win_supported(w)) return fail(WUN_ERR_UNSUPPORTED, "shape not served by the register-window weight-gradient kernel");
    }
    if (d->force_mtw < 0 || d->force_nw < 0) return fail(WUN_ERR_INVALID, "negative forced geometry");
    if (d->family == WUN_WGRAD_WIN) {
        // own geometry per part (split partials are in the final layout): column groups per workgroup, column tiles per wave
        if (d->force_mtw > 2 || d->force_nw > (d->K == 15 ? 5 : 6))
            return fail(WUN_ERR_UNSUPPORTED, "forced weight-gradient tile geometry is not available for this shape");
        for (int i = 0; i < d->nparts; ++i) { o.w[i].force_mtw = d->force_mtw; o.w[i].force_nw = d->force_nw; }
    } else if (d->force_mtw > 0 || d->force_nw > 0) {
        int m, n;
        if (!wgrad_common_geom(o.w, d->nparts, d->force_mtw, d->force_nw)) return fail(WUN_ERR_UNSUPPORTED, "the parts do not resolve to one forced tile geometry");
        wgrad_resolved_geom(o.w[0], m, n);
        if (m != d->force_mtw || n != d->force_nw) return fail(WUN_ERR_UNSUPPORTED, "forced weight-gradient tile geometry is not available for this shape");
    } else {
        // the plan's default: the heuristic geometry of the first part, lowered until every part agrees
        int m, n;
        wgrad_resolved_geom(o.w[0], m, n);
        while (!wgrad_common_geom(o.w, d->nparts, m, n) && m > 1) m = m == 6 ? 4 : m / 2;
        if (!wgrad_common_geom(o.w, d->nparts, m, n)) return fail(WUN_ERR_UNSUPPORTED, "the parts do not resolve to one tile geometry");
    }
    for (int i = 0; i < d->nparts; ++i) {
        WgradArgs& w = o.w[i];
        if (!wgrad_launch_ok(w, sw)) return fail(WUN_ERR_UNSUPPORTED, "the weight-gradient launcher refuses this shape under the resolved geometry");
        o.units[i] = wgrad_max_units(w, sw);
        w.nsplit = d->nsplit[i] > 0 ? std::min(d->nsplit[i], o.units[i]) : wgrad_pick_nsplit(w, sw);
        o.total += w.nsplit;
    }
    o.part_floats = wgrad_partial_floats(o.w[0], sw);
    // (one reduction reads every part's splits through the first part's layout)
    for (int i = 1; i < d->nparts; ++i)
        if (wgrad_partial_floats(o.w[i], sw) != o.part_floats) return fail(WUN_ERR_UNSUPPORTED, "the parts do not share one partial layout");
    return WUN_OK;
}

extern "C" int64_t wun_op_wgrad_ex_scratch(const wun_op_wgrad_desc* d) {
    OpWgrad o;
    if (int rc = op_wgrad_build(d, nullptr, nullptr, nullptr, nullptr, wun_switches_from_env(), o)) return rc;
    return (int64_t)o.total * o.part_floats + 128;
}

extern "C" int wun_op_wgrad_max_units(const wun_op_wgrad_desc* d, int part) {
    OpWgrad o;
    if (int rc = op_wgrad_build(d, nullptr, nullptr, nullptr, nullptr, wun_switches_from_env(), o)) return rc;
    if (part < 0 || part >= o.nparts) return fail(WUN_ERR_INVALID, "no such part");
    return o.units[part];
}

extern "C" int wun_op_wgrad_last_splits(void) { return t_op_wgrad_splits; }

extern "C" int wun_op_wgrad_ex(const wun_op_wgrad_desc* d, const void* x0, const void* x1, const void* dz_part0,
                               const void* dz_part1, float* grads, float* scratch, void* stream) {
    if (!d || !x0 || !dz_part0 || !grads || !scratch || (d->C1 > 0 && !x1) || (d->nparts == 2 && !dz_part1))
        return fail(WUN_ERR_INVALID, "null argument");
    if (reinterpret_cast<uintptr_t>(grads) & 3) return fail(WUN_ERR_INVALID, "grads not aligned to a float");
    const WunSwitches sw = wun_switches_from_env();
    OpWgrad o;
    if (int rc = op_wgrad_build(d, x0, x1, dz_part0, dz_part1, sw, o)) return rc;
    hipStream_t s = (hipStream_t)stream;
    float* partial = (float*)(((uintptr_t)scratch + 255) & ~(uintptr_t)255);
    if (o.narrow) {
        // run_narrow_wgrad: consecutive splits of one partial list, one reduction (no direct form)
        int done = 0;
        for (int i = 0; i < o.nparts; ++i) {
            o.nw[i].partial = partial; o.nw[i].split_base = done;
            HIP_TRY(launch_narrow_wgrad(o.nw[i], s, sw));
            done += o.nw[i].nsplit;
        }
        HIP_TRY(launch_narrow_wgrad_reduce(o.nw[0], partial, o.total, grads, o.woff, o.boff, s, d->accumulate != 0));
        t_op_wgrad_path = WUN_PATH_WGRAD_SPLIT; t_op_wgrad_splits = o.total;
        return WUN_OK;
    }
    float* out_w = grads;
    float* out_b = out_w + (long long)d->K * (d->C0 + d->C1) * d->N;
    if (o.total == 1) {
        // run_wgrad: one split in all -- the direct epilogue writes the final block
        o.w[0].out = out_w; o.w[0].direct = 1; o.w[0].split_base = 0;
        HIP_TRY(launch_wgrad(o.w[0], s, sw));
        t_op_wgrad_path = WUN_PATH_WGRAD_DIRECT; t_op_wgrad_splits = 1;
        return WUN_OK;
    }
    int done = 0;
    for (int i = 0; i < o.nparts; ++i) {
        o.w[i].out = partial; o.w[i].direct = 0; o.w[i].split_base = done;
        HIP_TRY(launch_wgrad(o.w[i], s, sw));
        done += o.w[i].nsplit;
    }
    HIP_TRY(launch_wgrad_reduce(o.w[0], partial, o.total, out_w, out_b, s, sw));
    t_op_wgrad_path = WUN_PATH_WGRAD_SPLIT; t_op_wgrad_splits = o.total;
    return WUN_OK;
}

/* Lane layout probe of v_mfma_f32_16x16x32_bf16: d[16][16] = bf16(a[16][32]) * bf16(b[32][16]). */
extern "C" int wun_op_mfma_bf16_probe(const float* a, const float* b, float* d, void* stream) {
    if (!a || !b || !d) return fail(WUN_ERR_INVALID, "null argument");
    HIP_TRY(launch_mfma_bf16_probe(a, b, d, (hipStream_t)stream));
    return WUN_OK;
}

extern "C" int wun_op_mfma_probe(const float* a, const float* b, float* d, void* stream) {
    if (!a || !b || !d) return fail(WUN_ERR_INVALID, "null argument");
    HIP_TRY(launch_mfma_probe(a, b, d, (hipStream_t)stream));
    return WUN_OK;
}
