// Host side of libwun.so: the forward pass of the training step (and of inference) as a launch sequence on the caller's
// stream and the plan's side streams.
#include "wun_plan_impl.h"

#include <cstring>
#include <vector>

// The 2x upsampling that opens up level j reads only the producer's output (bottleneck conv for j = 0, up conv
// j - 1 otherwise).  A producer launch that ends in the split-K epilogue kernel -- 10 of the 12 on the headline
// configuration -- writes the upsampled copy from there (ConvArgs.ups_*): one launch less on the dependent chain per
// level; the others still launch upsample_vec_kernel.  WUN_NO_FUSE_UPS=1: always the separate kernel.
static void want_ups(const wun_plan* p, const float* params, float* ws, ConvArgs& a, int j) {
    a.ups_y = ws + p->ups[j].off; a.ups_bs = p->ups[j].bs; a.ups_pitch = p->ups[j].pitch; a.ups_tup = p->ush[j].t_up;
    a.ups_w = p->interp[j] >= 0 ? params + p->interp[j] : nullptr;
}

// the up path (:107-125); ups_done: the bottleneck's launch wrote ups[0]; skip windows of levels < defer_below are awaited
static int forward_up_path(const wun_plan* p, const float* params, float* ws, hipStream_t s, bool ups_done, int defer_below) {
    const int L = p->L, Ku = p->cfg.merge_filter_size, padU = p->same ? (Ku - 1) / 2 : 0;
    const Buf* cur = &p->bott_out;
    for (int j = 0; j < L; ++j) {
        const UpShape& u = p->ush[j];
        if (!ups_done) {
            // (the producer's launch did not end in the split-K epilogue kernel, which writes this copy itself)
            UpsampleArgs ua;
            memset(&ua, 0, sizeof(ua));
            ua.x = ws + cur->off; ua.xbs = cur->bs; ua.xpitch = cur->pitch; ua.n = u.t_cur;
            ua.y = ws + p->ups[j].off; ua.ybs = p->ups[j].bs; ua.ypitch = p->ups[j].pitch; ua.tup = u.t_up;
            ua.w = p->interp[j] >= 0 ? params + p->interp[j] : nullptr;
            ua.C = u.c_cur; ua.B = p->B; ua.context = p->cfg.context; ua.bf = p->bf16 ? 1 : 0;
            HIP_TRY(launch_upsample(ua, s));
        }
        if (L - 1 - j < defer_below) HIP_TRY(hipStreamWaitEvent(s, p->skip_ev[(size_t)(L - 1 - j)], 0));
        ConvArgs a = conv_base(p);
        set_src0(a, ws, p->skip[L - 1 - j], 0, u.c_skip);          // crop already applied when it was written
        set_src1(a, ws, p->ups[j], 0, u.c_cur);
        a.Tin = u.t_up; a.shift = padU; a.W = params + p->up[j].woff; a.bias = params + p->up[j].boff;
        a.KW = Ku; a.N = a.N0 = u.cout; a.Tout = u.t_conv; a.flags = F_LRELU;
        set_dst0(a, ws, p->upo[j], 0, nullptr);
        if (p->fuse_ups && j + 1 < L) want_ups(p, params, ws, a, j + 1);
        HIP_TRY(conv_dispatch(p, a, ws + p->conv_part_off, p->conv_part_floats / 2, s));
        ups_done = p->fuse_ups && j + 1 < L && conv_last_fused_ups() != 0;
        cur = &p->upo[j];
    }
    return WUN_OK;
}

// forward: get_output (UnetAudioSeparator.py:85-144).  The mix rows come from mix_btc, or -- win != nullptr, wun_forward_windows --
// are gathered from a track (wun_track.hip); everything after that first pass is the same launch sequence.
int forward_pass(const wun_plan* p, const float* params, const float* mix_btc, const MixWindows* win, float* ws,
                 float* outputs, int training, hipStream_t s) {
    const int L = p->L, Kd = p->cfg.filter_size;
    const bool same = p->same;
    const int padD = same ? (Kd - 1) / 2 : 0;
    int rc0;
    if ((rc0 = side_init(p))) return rc0;
    p->ci = 0; p->in_bwd = false;
    hipStream_t s2 = (p->side && !g_profiling && p->tune_mode != 1) ? p->side : s;   // side stream (skip-window convs)
    bool side_used = false;

    p->cur_params = params; p->cur_ws = ws;
    if (p->bf16) {
        if (!p->dev_pack) return fail(WUN_ERR_HIP, "plan was created without a usable HIP device");
        HIP_TRY(launch_pack_bf16(params, ws, p->dev_pack, p->npack_fwd, p->pack_max, s));
    }
    p->wt_ready = false;
    if (training && !p->wt.empty() && p->dev_wt && s2 != s) {
        // the backward pass will need tap-flipped / transposed copies of every kernel: make them now,
        // beside the forward convs (they depend on the parameters only)
        if (!p->wt_ev) HIP_TRY(hipEventCreateWithFlags(&p->wt_ev, event_flags(p)));
        if ((rc0 = stream_dep(p, s, s2))) return rc0;
        HIP_TRY(launch_make_wt(params, ws, p->dev_wt, (int)p->wt.size(), p->wt_max, s2));
        if (p->bf16)
            HIP_TRY(launch_pack_bf16(params, ws, p->dev_pack + p->npack_fwd, (int)p->pack.size() - p->npack_fwd, p->pack_max, s2));
        HIP_TRY(hipEventRecord(p->wt_ev, s2));
        p->wt_ready = true;
        side_used = true;
    }
    if (win) HIP_TRY(launch_gather_windows(*win, ws + p->mix_ncw.off, p->B, p->Tin, p->C, p->mix_ncw.pitch, s));
    else HIP_TRY(launch_btc_to_ncw(mix_btc, ws + p->mix_ncw.off, p->B, p->Tin, p->C, p->mix_ncw.pitch, s));
    if (p->head16 && training)
        HIP_TRY(launch_cast_rows_bf16(ws + p->mix_ncw.off, ws + p->mix16.off, (long long)p->B * p->C, p->Tin, p->mix_ncw.pitch,
                                      p->mix16.pitch, s));

    // Context mode: the skip-window conv of level i is only consumed by up level L-1-i, i.e. the windows of the
    // shallow, FLOP-heavy levels are needed LAST.  The deep levels (few positions per excerpt) form a dependent
    // chain of launch-latency-bound kernels that leaves most CUs idle, so the window convs are deferred: queued on a
    // third stream (deepest-needed first) and awaited per level by the up path.  They fill the idle CUs instead of
    // competing with their own level's decimating conv.
    int defer_below = 0;                                            // levels [0, defer_below) are deferred
    hipStream_t s3 = (p->side2 && s2 != s) ? p->side2 : s2;
    if (!same && s3 != s2) {
        while (defer_below < L && (long long)p->B * p->dsh[defer_below].t_dec >= 16384) ++defer_below;
        if (L - defer_below < 3) defer_below = 0;                   // no deep chain to hide them under
        // ... and then the deep levels' (small) window convs are deferred as well: ONE event on the caller's stream
        // starts all of them instead of one event per level (each event holds the dependent chain for ~6 us); same-box
        // A/B 9.085 -> 9.04 ms.  (Awaiting the deep ones in groups instead of per level stalls the up path: 9.10-9.16.)
        if (defer_below > 0) defer_below = L;
        if (defer_below > 0 && p->skip_ev.size() < (size_t)L) {
            p->skip_ev.resize(L, nullptr);
            for (auto& e : p->skip_ev)
                if (!e) HIP_TRY(hipEventCreateWithFlags(&e, event_flags(p)));
        }
    }
    std::vector<ConvArgs> deferred((size_t)defer_below);
    std::vector<long long> deferred_pos((size_t)defer_below, -1);
    const long long part_half = p->conv_part_floats / 2, part_q = p->conv_part_floats / 4;

    const Buf* x = &p->mix_ncw;
    for (int i = 0; i < L; ++i) {                                   // :97-100
        const DownShape& d = p->dsh[i];
        const ConvLayer& cl = p->down[i];
        if (same) {
            ConvArgs a = conv_base(p);
            set_src0(a, ws, *x, 0, d.cin);
            a.Tin = d.t_in; a.shift = padD; a.W = params + cl.woff; a.bias = params + cl.boff;
            a.KW = Kd; a.N = a.N0 = d.cout; a.Tout = d.t_conv; a.flags = F_LRELU;
            set_dst0(a, ws, p->skip[i], 0, nullptr);
            a.dec = ws + p->dec[i].off; a.decbs = p->dec[i].bs; a.decpitch = p->dec[i].pitch;
            HIP_TRY(conv_dispatch(p, a, ws + p->conv_part_off, p->conv_part_floats / 2, s));
        } else {
            // x (written on `s`) is ready for both convs of this level: the side stream may start.  (Levels whose
            // window conv is deferred queue nothing on s2: no event -- every record / wait on the caller's stream is a
            // barrier packet that holds the dependent chain for ~7 us.)
            if (i >= defer_below && (rc0 = stream_dep(p, s, s2))) return rc0;
            // stride-2 conv straight into the decimated stream (odd outputs are never observed)
            ConvArgs a = conv_base(p);
            set_src0(a, ws, *x, 0, d.cin);
            a.loader = LOADER_DEINT;
            a.Tin = d.t_in; a.shift = 0; a.W = params + cl.woff; a.bias = params + cl.boff;
            a.KW = Kd; a.N = a.N0 = d.cout; a.Tout = d.t_dec; a.flags = F_LRELU;
            set_dst0(a, ws, p->dec[i], 0, nullptr);
            if (p->dedup) {
                // ... and, where 2q lies inside the crop window, into the skip window as well: the decimated stream IS a
                // slice of the encoder output (:98-100), one value, one rounding
                a.dec = ws + p->skip[i].off; a.decbs = p->skip[i].bs; a.decpitch = p->skip[i].pitch;
                a.dec_exp = 1; a.dec_lo = d.cs; a.dec_len = (unsigned)d.tc;
            }
            HIP_TRY(conv_dispatch(p, a, ws + p->conv_part_off, p->conv_part_floats / 2, s));
            // the rest of the window the skip connection crops (Utils.py:104-123) -- dedup plans: its ODD positions, a second
            // stride-2 conv over x shifted by one sample, stored with stride 2; else a full-rate conv over the whole window;
            // independent of the decimating conv -> side stream, own half of the split-K scratch
            DownPart part[2];
            const bool have_b = down_parts(p, i, part) == 2;
            const DownPart& win = part[1];
            ConvArgs b = conv_base(p);
            set_src0(b, ws, *x, win.off, d.cin);
            b.loader = win.loader;
            b.Tin = win.Tin; b.shift = win.shift; b.W = params + cl.woff; b.bias = params + cl.boff;
            b.KW = Kd; b.N = b.N0 = d.cout; b.Tout = win.Tq; b.flags = F_LRELU;
            set_dst0(b, ws, p->skip[i], win.off - d.cs, nullptr);      // (window element = conv position - cs)
            b.ostride = win.stride;
            if (i < defer_below) {
                deferred[(size_t)i] = b;
                deferred_pos[(size_t)i] = have_b ? (long long)p->ci++ : -2;   // its position in the canonical launch order
            } else if (have_b) {
                HIP_TRY(conv_dispatch(p, b, ws + p->conv_part_off + part_half, part_q, s2));
                side_used = side_used || (s2 != s);
            }
            if (defer_below > 0 && i == defer_below - 1) {
                // every input the deferred windows read has been issued on `s`: start them on the third stream
                if ((rc0 = stream_dep(p, s, s3))) return rc0;
                for (int k = defer_below - 1; k >= 0; --k) {
                    if (deferred_pos[(size_t)k] != -2)
                        HIP_TRY(conv_dispatch(p, deferred[(size_t)k], ws + p->conv_part_off + part_half + part_q, part_q, s3,
                                              deferred_pos[(size_t)k]));
                    HIP_TRY(hipEventRecord(p->skip_ev[(size_t)k], s3));
                }
            }
        }
        x = &p->dec[i];
    }
    ConvArgs a = conv_base(p);                                      // :102
    set_src0(a, ws, *x, 0, p->bott.Cin);
    a.Tin = p->t_b_in; a.shift = padD; a.W = params + p->bott.woff; a.bias = params + p->bott.boff;
    a.KW = Kd; a.N = a.N0 = p->c_b; a.Tout = p->t_b; a.flags = F_LRELU;
    set_dst0(a, ws, p->bott_out, 0, nullptr);
    if (p->fuse_ups) want_ups(p, params, ws, a, 0);
    HIP_TRY(conv_dispatch(p, a, ws + p->conv_part_off, p->conv_part_floats / 2, s));
    const bool ups_done = p->fuse_ups && conv_last_fused_ups() != 0;
    if (side_used && (rc0 = stream_dep(p, s2, s))) return rc0;     // the up path reads the skip windows
    if ((rc0 = forward_up_path(p, params, ws, s, ups_done, defer_below))) return rc0;
    HeadArgs h = head_args(p, params, ws, outputs, training);
    long long hoff[4] = {0, 0, 0, 0};
    for (int i = 0; i < p->Sh; ++i) hoff[i] = p->head[i].woff;
    HIP_TRY(launch_head_fwd_off(h, hoff, s));
    return WUN_OK;
}

extern "C" int wun_forward(const wun_plan* p, const float* params, const float* mix_btc, float* ws,
                           float* outputs, int training, void* stream) {
    if (!p || !params || !mix_btc || !ws || !outputs) return fail(WUN_ERR_INVALID, "null argument");
    return forward_pass(p, params, mix_btc, nullptr, ws, outputs, training, (hipStream_t)stream);
}
