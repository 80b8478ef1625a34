// Host side of libwun.so: the training step -- forward pass, loss + backward pass, Adam -- as launch sequences on the
// caller's stream and the plan's side streams.
#include "wun_plan_impl.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>

// ---------------------------------------------------------------------------------------
// forward: get_output (UnetAudioSeparator.py:85-144)
// ---------------------------------------------------------------------------------------
extern "C" int wun_forward(const wun_plan* p, const float* params, const float* mix_btc, float* ws,
                           float* outputs, int training, void* stream) {
    if (!p || !params || !mix_btc || !ws || !outputs) return fail(WUN_ERR_INVALID, "null argument");
    hipStream_t s = (hipStream_t)stream;
    const int L = p->L, Kd = p->cfg.filter_size, Ku = p->cfg.merge_filter_size;
    const bool same = p->same;
    const int padD = same ? (Kd - 1) / 2 : 0, padU = same ? (Ku - 1) / 2 : 0;
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
    HIP_TRY(launch_btc_to_ncw(mix_btc, ws + p->mix_ncw.off, p->B, p->Tin, p->C, p->mix_ncw.pitch, s));
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

    // The 2x upsampling that opens up level j reads only the producer's output (bottleneck conv for j = 0, up conv
    // j - 1 otherwise).  A producer launch that ends in the split-K epilogue kernel -- 10 of the 12 on the headline
    // configuration -- writes the upsampled copy from there (ConvArgs.ups_*): one launch less on the dependent chain per
    // level; the others still launch upsample_vec_kernel.  WUN_NO_FUSE_UPS=1: always the separate kernel.
    const bool fuse_ups = p->fuse_ups;
    bool ups_done = false;
    auto want_ups = [&](ConvArgs& a, int j) {
        a.ups_y = ws + p->ups[j].off; a.ups_bs = p->ups[j].bs; a.ups_pitch = p->ups[j].pitch; a.ups_tup = p->ush[j].t_up;
        a.ups_w = p->interp[j] >= 0 ? params + p->interp[j] : nullptr;
    };

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
            ConvArgs b = conv_base(p);
            bool have_b = true;
            if (p->dedup) {
                have_b = d.n_odd > 0;
                set_src0(b, ws, *x, d.t_odd0, d.cin);
                b.loader = LOADER_DEINT;
                b.Tin = d.t_in - d.t_odd0; b.shift = 0; b.W = params + cl.woff; b.bias = params + cl.boff;
                b.KW = Kd; b.N = b.N0 = d.cout; b.Tout = d.n_odd; b.flags = F_LRELU;
                set_dst0(b, ws, p->skip[i], d.t_odd0 - d.cs, nullptr);
                b.ostride = 2;
            } else {
                set_src0(b, ws, *x, d.cs, d.cin);
                b.Tin = d.tc + Kd - 1; b.shift = 0; b.W = params + cl.woff; b.bias = params + cl.boff;
                b.KW = Kd; b.N = b.N0 = d.cout; b.Tout = d.tc; b.flags = F_LRELU;
                set_dst0(b, ws, p->skip[i], 0, nullptr);
            }
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
    {                                                               // :102
        ConvArgs a = conv_base(p);
        set_src0(a, ws, *x, 0, p->bott.Cin);
        a.Tin = p->t_b_in; a.shift = padD; a.W = params + p->bott.woff; a.bias = params + p->bott.boff;
        a.KW = Kd; a.N = a.N0 = p->c_b; a.Tout = p->t_b; a.flags = F_LRELU;
        set_dst0(a, ws, p->bott_out, 0, nullptr);
        if (fuse_ups) want_ups(a, 0);
        HIP_TRY(conv_dispatch(p, a, ws + p->conv_part_off, p->conv_part_floats / 2, s));
        ups_done = fuse_ups && conv_last_fused_ups() != 0;
    }
    if (side_used && (rc0 = stream_dep(p, s2, s))) return rc0;     // the up path reads the skip windows
    const Buf* cur = &p->bott_out;
    for (int j = 0; j < L; ++j) {                                   // :107-125
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
        if (fuse_ups && j + 1 < L) want_ups(a, j + 1);
        HIP_TRY(conv_dispatch(p, a, ws + p->conv_part_off, p->conv_part_floats / 2, s));
        ups_done = fuse_ups && j + 1 < L && conv_last_fused_ups() != 0;
        cur = &p->upo[j];
    }
    HeadArgs h = head_args(p, params, ws, outputs, training);
    long long hoff[4] = {0, 0, 0, 0};
    for (int i = 0; i < p->Sh; ++i) hoff[i] = p->head[i].woff;
    HIP_TRY(launch_head_fwd_off(h, hoff, s));
    return WUN_OK;
}

struct BucketSignal {
    const int64_t* starts; void* const* events; int n; int next;   // buckets in descending start order
    // every gradient at arena offset >= floor is final with respect to stream `st`
    int ready(long long floor, hipStream_t st) {
        while (next < n && starts[next] >= floor) {
            hipError_t e = hipEventRecord((hipEvent_t)events[next], st);
            if (e != hipSuccess) return fail(WUN_ERR_HIP, std::string("hipEventRecord(bucket): ") + hipGetErrorString(e));
            ++next;
        }
        return WUN_OK;
    }
};

extern "C" int wun_loss_backward(const wun_plan* p, const float* params, const float* mix_btc, float* ws,
                                 const float* outputs, const float* targets, float* grads, float* loss,
                                 void* stream) {
    return wun_loss_backward_ex(p, params, mix_btc, ws, outputs, targets, grads, loss, stream, nullptr, nullptr, 0);
}

static int check_buckets(const int64_t* bucket_starts, void* const* bucket_events, int32_t nbuckets) {
    if (nbuckets < 0 || (nbuckets > 0 && (!bucket_starts || !bucket_events))) return fail(WUN_ERR_INVALID, "bad bucket arguments");
    for (int k = 1; k < nbuckets; ++k)
        if (bucket_starts[k] >= bucket_starts[k - 1]) return fail(WUN_ERR_INVALID, "bucket_starts must be strictly descending");
    return WUN_OK;
}

// The head of the backward pass: "MSE against targets" (wun_loss_backward: head_bwd_kernel + loss_finish) or "upstream gradient"
// (wun_backward: head_grad_kernel from d_outputs).  Everything after the head's d(pre-activation) is one body.
struct BackwardHead { const float* targets; float* loss; const float* d_outputs; };

// Which parts of the backward pass a call runs (wun_*_select).  Layers in the order the forward pass runs them:
// the mix (0), down level i (1 + i), the bottleneck (L + 1), interp_j (L + 2 + 2j), up level j (L + 3 + 2j), the head (3L + 2).
// wgrad[k]: layer k's weight-gradient launches run.  first: the earliest layer whose d(pre-activation) is needed -- the
// input-gradient launches of layer k (which produce the d(pre-activation) of the layers before it) run iff k > first.
// The full pass: every layer, first = the mix with d_mix, else down level 0 (whose input gradient is d_mix only).
struct BackwardSelect {
    std::vector<char> wgrad;
    int first = 0;
    int down(int i) const { return 1 + i; }
    int bott(int L) const { return L + 1; }
    int interp(int L, int j) const { return L + 2 + 2 * j; }
    int up(int L, int j) const { return L + 3 + 2 * j; }
    int head(int L) const { return 3 * L + 2; }
    bool wg(int k) const { return wgrad[(size_t)k] != 0; }
    bool ig(int k) const { return k > first; }
};

// select[k] != 0: tensor k (wun_plan_tensor order) is wanted; NULL = all.  A conv's kernel and bias come from one launch and
// must agree; so must the output layer's convs (one launch serves every source).  Host work only: fails before any GPU work.
static int parse_select(const wun_plan* p, const uint8_t* select, int64_t nselect, bool want_mix, BackwardSelect& sel,
                        bool& any) {
    const int L = p->L;
    const int64_t nt = (int64_t)p->tensors.size();
    sel.wgrad.assign((size_t)(3 * L + 3), 0);
    if (!select && nselect != 0 && nselect != nt) return fail(WUN_ERR_INVALID, "nselect must be 0 or num_tensors when select is NULL");
    if (select && nselect != nt) return fail(WUN_ERR_INVALID, "nselect must equal num_tensors");
    int64_t k = 0;
    int rc = WUN_OK;
    auto take = [&]() { return select ? select[k++] != 0 : (++k, true); };
    auto conv = [&]() {
        const bool w = take(), b = take();
        if (w != b && rc == WUN_OK)
            rc = fail(WUN_ERR_UNSUPPORTED, std::string("select: ") + p->tensors[(size_t)k - 2].name +
                                           " and its bias must be selected together (one launch computes both)");
        return w;
    };
    for (int i = 0; i < L; ++i) sel.wgrad[(size_t)sel.down(i)] = conv();
    sel.wgrad[(size_t)sel.bott(L)] = conv();
    for (int j = 0; j < L; ++j) {
        if (p->interp[(size_t)j] >= 0) sel.wgrad[(size_t)sel.interp(L, j)] = take();
        sel.wgrad[(size_t)sel.up(L, j)] = conv();
    }
    int nhead = 0;
    for (int s = 0; s < p->Sh; ++s) nhead += conv() ? 1 : 0;
    if (rc) return rc;
    if (nhead != 0 && nhead != p->Sh)
        return fail(WUN_ERR_UNSUPPORTED, "select: the output layer's convs (every source) must be selected together (one launch computes them)");
    sel.wgrad[(size_t)sel.head(L)] = nhead > 0;
    sel.first = -1;
    for (int l = 0; l <= sel.head(L) && sel.first < 0; ++l)
        if (sel.wgrad[(size_t)l]) sel.first = l;
    any = sel.first >= 0;
    if (want_mix) sel.first = 0;
    if (sel.first < 0) return fail(WUN_ERR_INVALID, "nothing to compute: no tensor selected and no d_mix");
    return WUN_OK;
}

static int backward_body(const wun_plan* p, const float* params, float* ws, const float* outputs, const BackwardHead& head,
                         float* grads, const MixGradArgs* mix, void* stream, const int64_t* bucket_starts,
                         void* const* bucket_events, int32_t nbuckets, const BackwardSelect& sel, bool accum);

extern "C" int wun_loss_backward_ex(const wun_plan* p, const float* params, const float* mix_btc, float* ws,
                                    const float* outputs, const float* targets, float* grads, float* loss,
                                    void* stream, const int64_t* bucket_starts, void* const* bucket_events,
                                    int32_t nbuckets) {
    return wun_loss_backward_select(p, params, mix_btc, ws, outputs, targets, grads, loss, stream, bucket_starts, bucket_events,
                                    nbuckets, nullptr, 0);
}

// accum: the final gradient stores add to `grads` (wun_loss_backward_accumulate); everything else is the overwriting call
static int loss_backward_select(const wun_plan* p, const float* params, float* ws, const float* outputs, const float* targets,
                                float* grads, float* loss, void* stream, const int64_t* bucket_starts, void* const* bucket_events,
                                int32_t nbuckets, const uint8_t* select, int64_t nselect, bool accum) {
    int rc;
    if ((rc = check_buckets(bucket_starts, bucket_events, nbuckets))) return rc;
    if (!p || !params || !ws || !outputs || !targets || !grads || !loss) return fail(WUN_ERR_INVALID, "null argument");
    BackwardSelect sel;
    bool any = false;
    if ((rc = parse_select(p, select, nselect, false, sel, any))) return rc;
    const BackwardHead head{targets, loss, nullptr};
    return backward_body(p, params, ws, outputs, head, grads, nullptr, stream, bucket_starts, bucket_events, nbuckets, sel, accum);
}

extern "C" int wun_loss_backward_select(const wun_plan* p, const float* params, const float* mix_btc, float* ws,
                                        const float* outputs, const float* targets, float* grads, float* loss,
                                        void* stream, const int64_t* bucket_starts, void* const* bucket_events,
                                        int32_t nbuckets, const uint8_t* select, int64_t nselect) {
    (void)mix_btc;
    return loss_backward_select(p, params, ws, outputs, targets, grads, loss, stream, bucket_starts, bucket_events, nbuckets,
                                select, nselect, false);
}

extern "C" int wun_loss_backward_accumulate(const wun_plan* p, const float* params, const float* mix_btc, float* ws,
                                            const float* outputs, const float* targets, float* grads, float* loss,
                                            void* stream, const int64_t* bucket_starts, void* const* bucket_events,
                                            int32_t nbuckets, const uint8_t* select, int64_t nselect) {
    (void)mix_btc;
    return loss_backward_select(p, params, ws, outputs, targets, grads, loss, stream, bucket_starts, bucket_events, nbuckets,
                                select, nselect, true);
}

// d_mix: where the audio's gradient lives after the backward pass -- down conv 0's d(pre-activation) in the launch geometries of
// its forward pass (the same parts the level-0 weight gradient reads, see the end of backward_body), the head's d(pre-activation)
// and the difference output's upstream gradient
static int mix_grad_args(const wun_plan* p, const float* params, float* ws, const float* d_outputs, float* d_mix, MixGradArgs& m) {
    memset(&m, 0, sizeof(m));
    const DownShape& d = p->dsh[0];
    const int Kd = p->cfg.filter_size;
    auto part = [&](int k, const Buf& z, int Tq, int stride, int off0, int shift, int Tin) {
        m.part[k].dz = ws + z.off; m.part[k].dzbs = z.bs; m.part[k].dzpitch = z.pitch;
        m.part[k].Tq = Tq; m.part[k].stride = stride; m.part[k].off0 = off0; m.part[k].shift = shift; m.part[k].Tin = Tin;
    };
    const Buf* z1 = nullptr;
    if (p->same) {
        part(0, p->dz_skip[0], d.t_conv, 1, 0, (Kd - 1) / 2, d.t_in);
        m.nparts = 1;
    } else {
        part(0, p->dz_dec[0], d.t_dec, 2, 0, 0, d.t_in);
        m.nparts = 1;
        if (p->dedup) {
            // dz_dec[0] holds the even window positions too; the odd ones are compact in dz_odd[0]
            if (d.n_odd > 0) { part(1, p->dz_odd[0], d.n_odd, 2, d.t_odd0, 0, d.t_in - d.t_odd0); z1 = &p->dz_odd[0]; m.nparts = 2; }
        } else {
            // full-rate window conv (bf16 mode): its even positions are computed a second time, both contributions add
            part(1, p->dz_skip[0], d.tc, 1, d.cs, 0, d.tc + Kd - 1); z1 = &p->dz_skip[0]; m.nparts = 2;
        }
    }
    const Buf& z0 = p->same ? p->dz_skip[0] : p->dz_dec[0];
    if (z1 && z1->eb != z0.eb) return fail(WUN_ERR_UNSUPPORTED, "d_mix: level-0 gradient parts of different element types");
    m.dzbf = z0.eb == 2 ? 1 : 0;
    m.W = params + p->down[0].woff; m.KW = Kd; m.F = p->cfg.num_initial_filters;
    m.C = p->C; m.B = p->B; m.Tin = p->Tin;
    const HeadArgs h = head_args(p, params, ws, nullptr, 1);
    m.dpre = h.dpre; m.dps = h.dps; m.dpbs = h.dpbs; m.dppitch = h.dppitch;
    m.Wh = params;
    for (int i = 0; i < p->Sh; ++i) m.hoff[i] = p->head[i].woff;
    m.Sh = p->Sh; m.Ko = h.Ko; m.padl = h.padl; m.Tfeat = h.Tfeat; m.Tout = h.Tout; m.moff_feat = h.moff_feat;
    m.dlast = h.difference ? d_outputs + (long long)(p->S - 1) * p->B * p->Tout * p->C : nullptr;
    m.moff_diff = h.moff_diff;
    m.dmix = d_mix;
    if (m.C != 1 && m.C != 2) return fail(WUN_ERR_UNSUPPORTED, "d_mix: only 1 or 2 audio channels are served");
    if (mix_grad_lds_bytes(m) > 64 * 1024) return fail(WUN_ERR_UNSUPPORTED, "d_mix: down conv 0 / head weights exceed the kernel's 64 KiB of LDS");
    return WUN_OK;
}

extern "C" int wun_backward(const wun_plan* p, const float* params, const float* mix_btc, float* ws,
                            const float* outputs, const float* d_outputs, float* grads, float* d_mix, void* stream) {
    return wun_backward_ex(p, params, mix_btc, ws, outputs, d_outputs, grads, d_mix, stream, nullptr, nullptr, 0);
}

extern "C" int wun_backward_ex(const wun_plan* p, const float* params, const float* mix_btc, float* ws,
                               const float* outputs, const float* d_outputs, float* grads, float* d_mix, void* stream,
                               const int64_t* bucket_starts, void* const* bucket_events, int32_t nbuckets) {
    int rc;
    if ((rc = check_buckets(bucket_starts, bucket_events, nbuckets))) return rc;
    if (!p || !params || !ws || !outputs || !d_outputs || !grads) return fail(WUN_ERR_INVALID, "null argument");
    return wun_backward_select(p, params, mix_btc, ws, outputs, d_outputs, grads, d_mix, stream, bucket_starts, bucket_events,
                               nbuckets, nullptr, 0);
}

static int backward_select(const wun_plan* p, const float* params, float* ws, const float* outputs, const float* d_outputs,
                           float* grads, float* d_mix, void* stream, const int64_t* bucket_starts, void* const* bucket_events,
                           int32_t nbuckets, const uint8_t* select, int64_t nselect, bool accum) {
    int rc;
    if ((rc = check_buckets(bucket_starts, bucket_events, nbuckets))) return rc;
    if (!p || !params || !ws || !outputs || !d_outputs) return fail(WUN_ERR_INVALID, "null argument");
    BackwardSelect sel;
    bool any = false;
    if ((rc = parse_select(p, select, nselect, d_mix != nullptr, sel, any))) return rc;
    if (any && !grads) return fail(WUN_ERR_INVALID, "null argument: grads (may be NULL only when no tensor is selected)");
    MixGradArgs mix;
    if (d_mix && (rc = mix_grad_args(p, params, ws, d_outputs, d_mix, mix))) return rc;
    const BackwardHead head{nullptr, nullptr, d_outputs};
    return backward_body(p, params, ws, outputs, head, grads, d_mix ? &mix : nullptr, stream, bucket_starts, bucket_events,
                         nbuckets, sel, accum);
}

extern "C" int wun_backward_select(const wun_plan* p, const float* params, const float* mix_btc, float* ws,
                                   const float* outputs, const float* d_outputs, float* grads, float* d_mix, void* stream,
                                   const int64_t* bucket_starts, void* const* bucket_events, int32_t nbuckets,
                                   const uint8_t* select, int64_t nselect) {
    (void)mix_btc;
    return backward_select(p, params, ws, outputs, d_outputs, grads, d_mix, stream, bucket_starts, bucket_events, nbuckets,
                           select, nselect, false);
}

extern "C" int wun_backward_accumulate(const wun_plan* p, const float* params, const float* mix_btc, float* ws,
                                       const float* outputs, const float* d_outputs, float* grads, float* d_mix, void* stream,
                                       const int64_t* bucket_starts, void* const* bucket_events, int32_t nbuckets,
                                       const uint8_t* select, int64_t nselect) {
    (void)mix_btc;
    return backward_select(p, params, ws, outputs, d_outputs, grads, d_mix, stream, bucket_starts, bucket_events, nbuckets,
                           select, nselect, true);
}

static int backward_body(const wun_plan* p, const float* params, float* ws, const float* outputs, const BackwardHead& head,
                         float* grads, const MixGradArgs* mix, void* stream, const int64_t* bucket_starts,
                         void* const* bucket_events, int32_t nbuckets, const BackwardSelect& sel, bool accum) {
    BucketSignal sig{bucket_starts, bucket_events, nbuckets, 0};
    if (!p->wt.empty() && !p->dev_wt) return fail(WUN_ERR_HIP, "plan was created without a usable HIP device");
    hipStream_t s = (hipStream_t)stream;
    const int L = p->L, Kd = p->cfg.filter_size, Ku = p->cfg.merge_filter_size, Ko = p->cfg.output_filter_size;
    const bool same = p->same;
    const int padD = same ? (Kd - 1) / 2 : 0, padU = same ? (Ku - 1) / 2 : 0;
    const int F = p->cfg.num_initial_filters, C = p->C;
    int rc;
    if ((rc = side_init(p))) return rc;
    p->ci = 0; p->wi = 0; p->in_bwd = true;
    // side streams: weight gradients + their reductions, alternating between two streams so the
    // ramp-up / drain of consecutive (independent) weight-gradient kernels overlap
    hipStream_t s2 = (p->side && !g_profiling && p->tune_mode != 1) ? p->side : s;
    hipStream_t s3 = (p->side2 && s2 != s) ? p->side2 : s2;
    int wg_rr = 0;
    auto wstream = [&]() { return (wg_rr++ & 1) ? s3 : s2; };
    // A launch a selection leaves out (live == false) still takes its launch position, so that every launch that does run
    // gets the tuned choice of the full pass; a left-out weight gradient also takes its turn of the side streams
    auto dispatch = [&](bool live, const ConvArgs& a, float* part, long long cap, hipStream_t st) -> hipError_t {
        if (!live) { ++p->ci; return hipSuccess; }
        return conv_dispatch(p, a, part, cap, st);
    };
    // bucket events are recorded on s2 once it has also seen everything queued on s3
    auto ready2 = [&](long long floor) -> int {
        if (s3 != s2 && sig.next < sig.n && sig.starts[sig.next] >= floor) {
            int rcj = stream_dep(p, s3, s2);
            if (rcj) return rcj;
        }
        return sig.ready(floor, s2);
    };
    // Weight gradients are queued and flushed one layer at a time: one event on the caller's stream per layer, both side
    // streams wait on it.  (Batching several deep levels behind one event -- every event is a barrier packet that holds
    // the dependent chain for ~7 us -- was measured in round 2: 41 -> 26 stalls per step, but the delayed weight gradients
    // lengthen the tail after the last input gradient by more: 9.12 ms per step with one layer per event, 9.19 - 9.23 with 2 - 5.)
    struct PendingWgrad { WgradArgs w[2]; int n; const ConvLayer* cl; bool live; };
    std::vector<PendingWgrad> pend;
    // Early skip-window input gradients (context mode).  The input gradient of down level i is the transposed stride-2
    // conv of dz_dec[i] over the whole row PLUS the full-rate conv of dz_skip[i] over the crop window.  dz_skip[i] is
    // final as soon as up level L-1-i's input gradient has run -- the shallow, FLOP-heavy levels' at the very start of
    // the backward pass -- while the row-wide part can only run when the dependent chain reaches level i at its very
    // end.  The window part is therefore launched as soon as its input exists, on the side streams (it fills the
    // launch-latency-bound deep part of the chain instead of lengthening the FLOP-bound end of it), stores into the
    // window of dz_dec[i-1], and the row-wide conv later ADDS inside the window (ConvArgs.acc_lo / acc_len) and stores
    // outside it: a + b == b + a, results are bit-identical to the old order.  Queued here, issued by the next flush
    // (whose event already orders the side streams behind the producing kernels: no extra packet on the chain).
    // Only the deep levels (input gradient = separate phase launches on a launch-latency-bound chain): same-box A/B
    // 8.84 -> 8.82 ms; moving the FLOP-heavy levels' window parts too changed nothing (8.98 vs 8.99: the end of the backward
    // pass is throughput-bound, not chain-bound).  WUN_EARLY_WINDOW=0 restores the old order (other launch order: the
    // tuning-table header records it).
    const bool early_win = !same && !p->bf16 && p->early_window != EW_OFF;
    auto level_fused = [&](int i) {                                  // (the rule of the down-path loop below)
        const DownShape& d = p->dsh[i];
        ConvArgs f = conv_base(p);
        f.Tin = d.t_dec; f.KW = p->down[i].J0; f.kw_full = Kd; f.N = f.N0 = d.cin; f.Tout = (d.t_in + 1) / 2; f.Tlim = d.t_in;
        f.flags = F_PHASE2; f.C0 = d.cout; f.B = p->B;
        return (d.cin & 3) == 0 && f.Tout >= 256 && conv_natural_wgs_phase2(f) >= 256;
    };
    // dedup plans: ranges of dz_dec[i - 1] that two more writers touch before / beside the row-wide transposed conv of level i --
    // E = the even half of skip window i - 1's gradient (stored by up level L - i's input gradient), W = the input gradient of
    // level i's odd window positions.  The early form of W (it ADDS inside E and stores elsewhere; the row-wide conv then adds
    // inside W) needs E inside W, which the centred crops of every shipped config give; else W runs after the row-wide conv.
    auto e_range = [&](int i, int& lo, int& len) { lo = p->dsh[i].t_ev0 / 2; len = p->dsh[i].n_even; };
    auto w_range = [&](int i, int& lo, int& len) {
        const DownShape& d = p->dsh[i];
        if (p->dedup) { lo = d.t_odd0; len = d.n_odd > 0 ? 2 * (d.n_odd - 1) + Kd : 0; }
        else { lo = d.cs; len = d.tc + Kd - 1; }
    };
    // Which levels' window input gradients leave the dependent chain.  Dedup plans (round 6): ALL of them -- the odd-window
    // launches are half the size of the old window convs, and for the middle levels (row-wide part fused, window part too
    // small to fuse) the chain otherwise carries two phase launches + their split-K epilogues per level: same-box A/B, each arm
    // autotuned, 8.14 -> 8.03 ms per step, 7.94 together with the lower fuse floor below (profiles/round6_ab_dedup_schedule.txt).
    // Rounds 3 - 5 (full-window convs): only the deep levels, moving the FLOP-heavy ones changed nothing (8.98 vs 8.99).
    // WUN_EARLY_WINDOW=deep | all | 0 overrides (a non-default mode is part of the tuning-table header).
    const bool early_all = p->early_window == EW_ALL;
    auto level_early = [&](int i) {
        if (!(early_win && i > 0 && (early_all || !level_fused(i)))) return false;
        if (!p->dedup) return true;
        int elo, elen, wlo, wlen;
        e_range(i - 1, elo, elen); w_range(i, wlo, wlen);
        return wlen > 0 && (elen == 0 || (wlo <= elo && elo + elen <= wlo + wlen));
    };
    if (early_win && p->win_ev.size() < (size_t)L) {
        p->win_ev.resize(L, nullptr);
        for (auto& e : p->win_ev)
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e, event_flags(p)));
    }
    struct PendingWin { int i; bool live; };
    std::vector<PendingWin> pend_win;
    std::vector<UpsampleBwdArgs> pend_interp;
    const long long cpart_half = p->conv_part_floats / 2, cpart_q = p->conv_part_floats / 4;
    auto window_dgrad_args = [&](int i) {
        const DownShape& d = p->dsh[i];
        const ConvLayer& cl = p->down[i];
        ConvArgs a = conv_base(p);
        set_src0(a, ws, p->dz_skip[i], 0, d.cout);
        a.Tin = d.tc; a.shift = Kd - 1; a.W = ws + cl.wt_full; a.KW = Kd;
        a.N = a.N0 = d.cin; a.Tout = d.tc + Kd - 1;
        set_dst0(a, ws, p->dz_dec[i - 1], d.cs, &p->dec[i - 1]);
        return a;
    };
    // Transposed stride-2 conv of down level i into dz_dec[i - 1] (masked with dec[i - 1]'s LeakyReLU branch): of the decimated
    // stream's gradient dz_dec[i] over the whole row (odd = false), or -- dedup plans -- of the odd window positions' gradient
    // dz_odd[i] into [t_odd0, t_odd0 + 2 (n_odd - 1) + Kd) (odd = true).  Both output phases fused in one launch (a lane owns 8
    // consecutive outputs) when the launch fills the chip, else one phase at a time (those launches can use split-K).
    // accum: add to what the row holds inside [acc_lo, acc_lo + acc_len) (acc_len == 0: everywhere), store elsewhere.
    auto tconv2 = [&](bool live, int i, bool odd, bool accum, int acc_lo, unsigned acc_len, hipStream_t st, float* part,
                      long long cap) -> int {
        const DownShape& d = p->dsh[i];
        const ConvLayer& cl = p->down[i];
        const Buf& src = odd ? p->dz_odd[i] : p->dz_dec[i];
        const int n_in = odd ? d.n_odd : d.t_dec;
        const int out_off = odd ? d.t_odd0 : 0;
        const int out_len = odd ? 2 * (d.n_odd - 1) + Kd : d.t_in;
        ConvArgs f = conv_base(p);
        set_src0(f, ws, src, 0, d.cout);
        f.Tin = n_in; f.KW = cl.J0; f.kw_full = Kd; f.shift = cl.J0 - 1; f.W = ws + cl.wt_ph2;
        f.N = f.N0 = d.cin; f.Tout = (out_len + 1) / 2; f.Tlim = out_len; f.flags = F_PHASE2;
        set_dst0(f, ws, p->dz_dec[i - 1], out_off, &p->dec[i - 1]);
        if (accum) { f.flags |= F_ACCUM; f.acc_lo = acc_lo; f.acc_len = acc_len; }
        // Odd-window part: its outputs start at the odd row position t_odd0 -- scalar read-modify-write stores.  With the
        // filter shifted by one tap (wt_ph2s: the same sums, one leading zero tap) the launch starts at t_odd0 - 1, and -- one
        // more (zero) input position in front when that is not a multiple of 4 -- at t_odd0 - 3: a 16-byte boundary, the vector
        // epilogue.  The leading outputs it adds are sums over zero taps / positions before the first sample: +0 where it
        // accumulates, 0 where it stores (positions the row-wide conv then stores over: they lie outside its accumulate range).
        if (odd && cl.wt_ph2s >= 0 && !p->sw.no_odd_align) {
            const int base = d.t_odd0 - 1, extra = (base & 3) ? 2 : 0;
            if (base - extra >= 0) {
                f.KW = cl.J0s; f.shift = cl.J0s - 1 + (extra ? 1 : 0); f.W = ws + cl.wt_ph2s;
                const int len2 = out_len + 1 + extra;
                f.Tout = (len2 + 1) / 2; f.Tlim = len2;
                set_dst0(f, ws, p->dz_dec[i - 1], base - extra, &p->dec[i - 1]);
            }
        }
        // (bf16 mode: always fused when the channel count allows -- one launch, the gradient tile staged once,
        //  contiguous 32-byte stores instead of two stride-2 scatter passes)
        // (the odd-window launches fuse from 64 workgroups / 64 output pairs on: they run on the side streams, where one
        //  launch beats two phase launches + two split-K epilogues; WUN_ODD_FUSE_MIN overrides the floor)
        const int odd_min = p->sw.odd_fuse_min;
        const int tmin = odd ? std::min(256, odd_min) : 256, wmin = odd ? odd_min : 256;
        if ((d.cin & 3) == 0 && (p->bf16 || (f.Tout >= tmin && conv_natural_wgs_phase2(f) >= wmin))) {
            HIP_TRY(dispatch(live, f, part, cap, st));
            return WUN_OK;
        }
        for (int ph = 0; ph < 2; ++ph) {
            ConvArgs a = conv_base(p);
            set_src0(a, ws, src, 0, d.cout);
            a.Tin = n_in; a.KW = cl.Jp[ph]; a.shift = cl.Jp[ph] - 1; a.W = ws + cl.wt_ph[ph];
            a.N = a.N0 = d.cin; a.Tout = (out_len - ph + 1) / 2;
            set_dst0(a, ws, p->dz_dec[i - 1], out_off + ph, &p->dec[i - 1]);
            a.ostride = 2;
            if (accum) { a.flags |= F_ACCUM; a.acc_lo = acc_lo; a.acc_len = acc_len; }
            if (a.Tout > 0) HIP_TRY(dispatch(live, a, part, cap, st));
        }
        return WUN_OK;
    };
    auto flush_wgrads = [&]() -> int {
        if (pend.empty() && pend_win.empty() && pend_interp.empty()) return WUN_OK;
        bool work = !pend_interp.empty();
        for (auto& q : pend) work = work || q.live;
        for (auto& w : pend_win) work = work || w.live;
        if (s2 != s && work) {
            hipEvent_t e = p->events[p->ev_next++ % p->events.size()];
            HIP_TRY(hipEventRecord(e, s));
            HIP_TRY(hipStreamWaitEvent(s2, e, 0));
            if (s3 != s2) HIP_TRY(hipStreamWaitEvent(s3, e, 0));
        }
        for (auto& ub : pend_interp) HIP_TRY(launch_interp_grad(ub, wstream(), accum));
        pend_interp.clear();
        for (auto& q : pend) {
            int rcq = WUN_OK;
            if (q.live) rcq = run_wgrad(p, q.w, q.n, *q.cl, ws, grads, s, wstream(), false, accum);
            else { wstream(); ++p->wi; }
            if (rcq) return rcq;
            if ((rcq = ready2(q.cl->woff))) return rcq;        // (a bucket without a selected tensor: signalled here)
        }
        pend.clear();
        for (const PendingWin& pw : pend_win) {
            const int i = pw.i;
            // own quarter of the split-K scratch per side stream (the chain on `s` uses the first half)
            hipStream_t sw = wstream();
            float* part = ws + p->conv_part_off + cpart_half + ((sw == s3 && s3 != s2) ? cpart_q : 0);
            if (p->dedup) {
                int elo, elen;
                e_range(i - 1, elo, elen);
                int rcw = tconv2(pw.live, i, true, elen > 0, elo, (unsigned)elen, sw, sw == s ? ws + p->conv_part_off : part,
                                 sw == s ? cpart_half : cpart_q);
                if (rcw) return rcw;
            } else {
                HIP_TRY(dispatch(pw.live, window_dgrad_args(i), sw == s ? ws + p->conv_part_off : part, sw == s ? cpart_half : cpart_q, sw));
            }
            if (sw != s && pw.live) HIP_TRY(hipEventRecord(p->win_ev[(size_t)i], sw));
        }
        pend_win.clear();
        return WUN_OK;
    };
    auto submit_wgrad = [&](const WgradArgs* w, int n, const ConvLayer& cl, bool live) -> int {
        PendingWgrad q;
        for (int k = 0; k < n; ++k) q.w[k] = w[k];
        q.n = n; q.cl = &cl; q.live = live;
        pend.push_back(q);
        return flush_wgrads();
    };

    if (p->wt_ready) {
        HIP_TRY(hipStreamWaitEvent(s, p->wt_ev, 0));       // made during the forward pass
        p->wt_ready = false;
    } else {
        HIP_TRY(launch_make_wt(params, ws, p->dev_wt, (int)p->wt.size(), p->wt_max, s));
        if (p->bf16)
            HIP_TRY(launch_pack_bf16(params, ws, p->dev_pack + p->npack_fwd, (int)p->pack.size() - p->npack_fwd, p->pack_max, s));
    }
    p->cur_params = params; p->cur_ws = ws;

    // ---- head: loss, d(pre-activation), d(feature map) ----
    HeadArgs h = head_args(p, params, ws, const_cast<float*>(outputs), 1);
    long long hoff[4] = {0, 0, 0, 0};
    for (int i = 0; i < p->Sh; ++i) hoff[i] = p->head[i].woff;
    if (head.d_outputs) {
        h.dout = head.d_outputs;
        HIP_TRY(launch_head_grad_off(h, hoff, s));
    } else {
        h.tgt = head.targets;
        HIP_TRY(launch_head_bwd_off(h, hoff, s));
        HIP_TRY(launch_loss_finish(h.loss_partial, head_bwd_blocks(h),
                                   1.0f / ((float)p->S * (float)p->B * (float)p->Tout * (float)p->C), head.loss, s));
    }
    bool head_done = false;
    const bool wg_head = sel.wg(sel.head(L));
    if (p->head16 && wg_head)
        HIP_TRY(launch_cast_rows_bf16(h.dpre, ws + p->dpre16_off, (long long)p->Sh * p->B * C, p->Tout, h.dppitch, p->dp16_pitch, s));
    if (p->Sh > 0 && !p->head16) {
        // every source's output conv in ONE direct-reduction launch (OutputLayer.py:8,15): dz rows = (source, channel)
        NarrowWgradArgs nw;
        memset(&nw, 0, sizeof(nw));
        nw.src0 = ws + p->mix_ncw.off; nw.bs0 = p->mix_ncw.bs; nw.pitch0 = p->mix_ncw.pitch; nw.off0 = p->in_crop_start; nw.C0 = C;
        nw.src1 = ws + p->upo[L - 1].off; nw.bs1 = p->upo[L - 1].bs; nw.pitch1 = p->upo[L - 1].pitch; nw.off1 = 0; nw.C1 = F;
        nw.Tin = p->t_feat; nw.shift = h.padl; nw.KW = Ko; nw.stride = 1;
        nw.dz = h.dpre; nw.zss = h.dps; nw.dzbs = h.dpbs; nw.dzpitch = h.dppitch;
        nw.N = p->Sh * C; nw.Nper = C; nw.Tq = p->Tout; nw.B = p->B;
        nw.et = p->bf16 ? 2 : 0;                                  // fp32 audio + (bf16) feature map, fp32 d(pre-activation)
        if (narrow_wgrad_supported(nw) && (p->bf16 || !p->sw.no_narrow)) {
            long long woff[4] = {0, 0, 0, 0}, boff[4] = {0, 0, 0, 0};
            for (int sh = 0; sh < p->Sh; ++sh) { woff[sh] = p->head[sh].woff; boff[sh] = p->head[sh].boff; }
            hipStream_t sw = wstream();
            if (wg_head && (rc = run_narrow_wgrad(p, &nw, 1, woff, boff, ws, grads, s, sw, accum))) return rc;
            head_done = true;
        } else if (p->bf16) {
            // bf16 mode: the head's inputs are the fp32 audio and the bf16 feature map -- only the narrow kernels read
            // that mix.  More (input channel, output row) pairs than one launch holds (the deep variant: 50 x 6): one
            // launch per source
            nw.N = nw.Nper = C;
            if (!narrow_wgrad_supported(nw)) return fail(WUN_ERR_UNSUPPORTED, "bf16 mode: output-layer shape not served by the narrow weight-gradient kernels");
            for (int sh = 0; sh < p->Sh; ++sh) {
                NarrowWgradArgs one = nw;
                one.dz = h.dpre + (long long)sh * h.dps;
                const long long woff[4] = {p->head[sh].woff, 0, 0, 0}, boff[4] = {p->head[sh].boff, 0, 0, 0};
                hipStream_t sw = wstream();
                if (wg_head && (rc = run_narrow_wgrad(p, &one, 1, woff, boff, ws, grads, s, sw, accum))) return rc;
            }
            head_done = true;
        }
    }
    for (int sh = 0; sh < p->Sh && !head_done; ++sh) {
        if (!wg_head) { wstream(); ++p->wi; continue; }
        WgradArgs w = wgrad_base(p);
        wset_src0(w, ws, p->head16 ? p->mix16 : p->mix_ncw, p->in_crop_start, C);
        wset_src1(w, ws, p->upo[L - 1], 0, F);
        w.Tin = p->t_feat; w.shift = h.padl; w.KW = Ko;
        if (p->head16)       // (bf16 rows: element strides; the float* base advances by half as many floats)
            wset_dz(w, ws + p->dpre16_off + ((long long)sh * p->B * C * p->dp16_pitch) / 2, (long long)C * p->dp16_pitch, p->dp16_pitch, C, p->Tout);
        else
            wset_dz(w, h.dpre + (long long)sh * h.dps, h.dpbs, h.dppitch, C, p->Tout);
        if ((rc = run_wgrad(p, &w, 1, p->head[sh], ws, grads, s, wstream(), true, accum))) return rc;
    }
    if (p->Sh > 0 && (rc = ready2(p->head[0].woff))) return rc;

    // ---- up path, last level first ----
    const bool fuse_ups = p->fuse_ups;
    bool adj_done = false;
    for (int j = L - 1; j >= 0; --j) {
        const UpShape& u = p->ush[j];
        const int i = L - 1 - j;
        {
            WgradArgs w = wgrad_base(p);
            wset_src0(w, ws, p->skip[i], 0, u.c_skip);
            wset_src1(w, ws, p->ups[j], 0, u.c_cur);
            w.Tin = u.t_up; w.shift = padU; w.KW = Ku;
            wset_dz(w, ws + p->dz_upo[j].off, p->dz_upo[j].bs, p->dz_upo[j].pitch, u.cout, u.t_conv);
            // (interp_j, written on `s` by the previous level's upsample_bwd, sits above up[j] in
            // the arena; the flush makes the side streams wait for everything issued on `s` so far)
            if ((rc = submit_wgrad(&w, 1, p->up[j], sel.wg(sel.up(L, j))))) return rc;
        }
        {
            ConvArgs a = conv_base(p);
            set_src0(a, ws, p->dz_upo[j], 0, u.cout);
            a.Tin = u.t_conv; a.shift = Ku - 1 - padU; a.W = ws + p->up[j].wt_full; a.KW = Ku;
            a.N = u.c_skip + u.c_cur; a.N0 = u.c_skip; a.Tout = u.t_up;
            set_dst0(a, ws, p->dz_skip[i], 0, &p->skip[i]);
            set_dst1(a, ws, p->d_ups[j], 0, nullptr);
            if (p->dedup) {
                // window element q sits at absolute conv position cs + q: the even positions are elements of the decimated
                // stream -- their gradient goes into dz_dec[i] (index (cs + q) / 2), the odd ones compact into dz_odd[i]
                const DownShape& d = p->dsh[i];
                float* ev = ws + p->dz_dec[i].off;
                float* od = ws + p->dz_odd[i].off;
                const bool cs_even = (d.cs & 1) == 0;
                a.dec = cs_even ? ev : od;  a.decbs = cs_even ? p->dz_dec[i].bs : p->dz_odd[i].bs;
                a.decpitch = cs_even ? p->dz_dec[i].pitch : p->dz_odd[i].pitch; a.dec_off = cs_even ? d.t_ev0 / 2 : 0;
                a.dec1 = cs_even ? od : ev; a.dec1bs = cs_even ? p->dz_odd[i].bs : p->dz_dec[i].bs;
                a.dec1pitch = cs_even ? p->dz_odd[i].pitch : p->dz_dec[i].pitch; a.dec1_off = cs_even ? 0 : d.t_ev0 / 2;
            }
            const Buf& prev = (j == 0) ? p->bott_out : p->upo[j - 1];
            const Buf& dzprev = (j == 0) ? p->dz_bott : p->dz_upo[j - 1];
            // linear interpolation: a launch that ends in the split-K epilogue kernel applies the adjoint of the 2x
            // upsampling there (ConvArgs.ubw_*) instead of storing d_ups[j] for upsample_bwd_vec_kernel
            if (fuse_ups && p->interp[j] < 0 && dzprev.bs == prev.bs && dzprev.pitch == prev.pitch) {
                a.ubw_dz = ws + dzprev.off; a.ubw_x = ws + prev.off; a.ubw_bs = prev.bs; a.ubw_pitch = prev.pitch;
                a.ubw_n = u.t_cur;
            }
            const bool live = sel.ig(sel.up(L, j));
            HIP_TRY(dispatch(live, a, ws + p->conv_part_off, p->conv_part_floats / 2, s));
            adj_done = a.ubw_dz != nullptr && conv_last_fused_ups() != 0;
            // dz_skip[i] is final: its window input gradient can start
            if (level_early(i)) pend_win.push_back(PendingWin{i, sel.ig(sel.down(i))});
            if (!live) continue;                                // (interp_j and everything before it are not needed)
        }
        if (!adj_done) {
            const Buf& prev = (j == 0) ? p->bott_out : p->upo[j - 1];
            const Buf& dzprev = (j == 0) ? p->dz_bott : p->dz_upo[j - 1];
            UpsampleBwdArgs ub;
            memset(&ub, 0, sizeof(ub));
            ub.dy = ws + p->d_ups[j].off; ub.ybs = p->d_ups[j].bs; ub.ypitch = p->d_ups[j].pitch; ub.tup = u.t_up;
            ub.x = ws + prev.off; ub.xbs = prev.bs; ub.xpitch = prev.pitch; ub.n = u.t_cur;
            ub.dz = ws + dzprev.off;
            ub.w = p->interp[j] >= 0 ? params + p->interp[j] : nullptr;
            const bool wg_interp = p->interp[j] >= 0 && sel.wg(sel.interp(L, j));
            ub.dw = wg_interp ? grads + p->interp[j] : nullptr;
            ub.dw_partial = (wg_interp && !p->interp_partial_off.empty()) ? ws + p->interp_partial_off[(size_t)j] : nullptr;
            ub.C = u.c_cur; ub.B = p->B; ub.context = p->cfg.context; ub.bf = p->bf16 ? 1 : 0;
            if (sel.ig(sel.interp(L, j))) HIP_TRY(launch_upsample_bwd(ub, s));
            // the interpolation weights' gradient is nobody's input on the chain: with the next flush, on a side stream
            // (interp_<j> lies just below up[j]'s kernel in the arena: complete before the next layer's bucket signal)
            if (ub.dw != nullptr) pend_interp.push_back(ub);
        }
    }

    // ---- bottleneck ----
    {
        WgradArgs w = wgrad_base(p);
        wset_src0(w, ws, p->dec[L - 1], 0, p->bott.Cin);
        w.Tin = p->t_b_in; w.shift = padD; w.KW = Kd;
        wset_dz(w, ws + p->dz_bott.off, p->dz_bott.bs, p->dz_bott.pitch, p->c_b, p->t_b);
        if ((rc = submit_wgrad(&w, 1, p->bott, sel.wg(sel.bott(L))))) return rc;
        ConvArgs a = conv_base(p);
        set_src0(a, ws, p->dz_bott, 0, p->c_b);
        a.Tin = p->t_b; a.shift = Kd - 1 - padD; a.W = ws + p->bott.wt_full; a.KW = Kd;
        a.N = a.N0 = p->bott.Cin; a.Tout = p->t_b_in;
        if (same) {
            set_dst0(a, ws, p->dz_skip[L - 1], 0, &p->skip[L - 1]);
            a.ostride = 2; a.flags = F_ACCUM;
        } else {
            set_dst0(a, ws, p->dz_dec[L - 1], 0, &p->dec[L - 1]);
            if (p->dedup && p->dsh[L - 1].n_even > 0) {
                // (the even half of skip window L-1's gradient is already there)
                int elo, elen;
                e_range(L - 1, elo, elen);
                a.flags = F_ACCUM; a.acc_lo = elo; a.acc_len = (unsigned)elen;
            }
        }
        HIP_TRY(dispatch(sel.ig(sel.bott(L)), a, ws + p->conv_part_off, p->conv_part_floats / 2, s));
    }

    // ---- down path ----
    for (int i = L - 1; i >= 0; --i) {
        const DownShape& d = p->dsh[i];
        const ConvLayer& cl = p->down[i];
        const Buf& x = (i == 0) ? p->mix_ncw : p->dec[i - 1];
        // the audio-input conv (1 or 2 input channels): direct reduction instead of MFMA tiles (10 TFLOP/s of mostly
        // padding); WUN_NO_NARROW_DOWN0=1 keeps the MFMA kernel (A/B: 9.36 -> 9.32 ms per step with the narrow kernel)
        NarrowWgradArgs nw[2];
        bool narrow = false;
        if (i == 0) {
            memset(nw, 0, sizeof(nw));
            for (int k = 0; k < 2; ++k) {
                nw[k].src0 = ws + x.off; nw[k].bs0 = x.bs; nw[k].pitch0 = x.pitch; nw[k].C0 = d.cin;
                nw[k].KW = Kd; nw[k].N = nw[k].Nper = d.cout; nw[k].B = p->B;
                nw[k].et = p->bf16 ? 4 : 0;                       // fp32 audio, (bf16) dz
            }
            if (same) {
                nw[0].Tin = d.t_in; nw[0].shift = padD; nw[0].stride = 1; nw[0].off0 = 0;
                nw[0].dz = ws + p->dz_skip[0].off; nw[0].dzbs = p->dz_skip[0].bs; nw[0].dzpitch = p->dz_skip[0].pitch; nw[0].Tq = d.t_conv;
            } else {
                nw[0].Tin = d.t_in; nw[0].shift = 0; nw[0].stride = 2; nw[0].off0 = 0;
                nw[0].dz = ws + p->dz_dec[0].off; nw[0].dzbs = p->dz_dec[0].bs; nw[0].dzpitch = p->dz_dec[0].pitch; nw[0].Tq = d.t_dec;
                if (p->dedup) {
                    nw[1].Tin = d.t_in - d.t_odd0; nw[1].shift = 0; nw[1].stride = 2; nw[1].off0 = d.t_odd0;
                    nw[1].dz = ws + p->dz_odd[0].off; nw[1].dzbs = p->dz_odd[0].bs; nw[1].dzpitch = p->dz_odd[0].pitch; nw[1].Tq = d.n_odd;
                } else {
                    nw[1].Tin = d.tc + Kd - 1; nw[1].shift = 0; nw[1].stride = 1; nw[1].off0 = d.cs;
                    nw[1].dz = ws + p->dz_skip[0].off; nw[1].dzbs = p->dz_skip[0].bs; nw[1].dzpitch = p->dz_skip[0].pitch; nw[1].Tq = d.tc;
                }
            }
            const int nparts0 = same ? 1 : ((p->dedup && d.n_odd == 0) ? 1 : 2);
            narrow = narrow_wgrad_supported(nw[0]) && (nparts0 == 1 || narrow_wgrad_supported(nw[1])) &&
                     (p->bf16 || (!p->sw.no_narrow && !p->sw.no_narrow_down0));
            // (bf16 mode: the narrow kernels are the only ones that read fp32 audio against bf16 gradients)
            if (p->bf16 && !narrow) return fail(WUN_ERR_UNSUPPORTED, "bf16 mode: audio-input conv shape not served by the narrow weight-gradient kernels");
        }
        const bool wg_down = sel.wg(sel.down(i)), ig_down = sel.ig(sel.down(i));
        if (narrow) {
            if ((rc = flush_wgrads())) return rc;
            const long long woff[4] = {cl.woff, 0, 0, 0}, boff[4] = {cl.boff, 0, 0, 0};
            hipStream_t sw = wstream();
            if (wg_down && (rc = run_narrow_wgrad(p, nw, (same || (p->dedup && d.n_odd == 0)) ? 1 : 2, woff, boff, ws, grads, s, sw,
                                                 accum)))
                return rc;
            if ((rc = ready2(cl.woff))) return rc;
        } else if (same) {
            WgradArgs w = wgrad_base(p);
            wset_src0(w, ws, x, 0, d.cin);
            w.Tin = d.t_in; w.shift = padD; w.KW = Kd;
            wset_dz(w, ws + p->dz_skip[i].off, p->dz_skip[i].bs, p->dz_skip[i].pitch, d.cout, d.t_conv);
            if ((rc = submit_wgrad(&w, 1, cl, wg_down))) return rc;
            if (i > 0) {
                ConvArgs a = conv_base(p);
                set_src0(a, ws, p->dz_skip[i], 0, d.cout);
                a.Tin = d.t_conv; a.shift = Kd - 1 - padD; a.W = ws + cl.wt_full; a.KW = Kd;
                a.N = a.N0 = d.cin; a.Tout = d.t_in;
                set_dst0(a, ws, p->dz_skip[i - 1], 0, &p->skip[i - 1]);
                a.ostride = 2; a.flags = F_ACCUM;
                HIP_TRY(dispatch(ig_down, a, ws + p->conv_part_off, p->conv_part_floats / 2, s));
            }
        } else {
            WgradArgs w[2];
            w[0] = wgrad_base(p);
            wset_src0(w[0], ws, x, 0, d.cin);
            w[0].loader = LOADER_DEINT; w[0].Tin = d.t_in; w[0].shift = 0; w[0].KW = Kd;
            wset_dz(w[0], ws + p->dz_dec[i].off, p->dz_dec[i].bs, p->dz_dec[i].pitch, d.cout, d.t_dec);
            w[1] = wgrad_base(p);
            int nparts = 2;
            if (p->dedup) {
                // the odd window positions: the same stride-2 geometry over x shifted by t_odd0 samples
                nparts = d.n_odd > 0 ? 2 : 1;
                wset_src0(w[1], ws, x, d.t_odd0, d.cin);
                w[1].loader = LOADER_DEINT; w[1].Tin = d.t_in - d.t_odd0; w[1].shift = 0; w[1].KW = Kd;
                wset_dz(w[1], ws + p->dz_odd[i].off, p->dz_odd[i].bs, p->dz_odd[i].pitch, d.cout, d.n_odd);
            } else {
                wset_src0(w[1], ws, x, d.cs, d.cin);
                w[1].Tin = d.tc + Kd - 1; w[1].shift = 0; w[1].KW = Kd;
                wset_dz(w[1], ws + p->dz_skip[i].off, p->dz_skip[i].bs, p->dz_skip[i].pitch, d.cout, d.tc);
            }
            if ((rc = submit_wgrad(w, nparts, cl, wg_down))) return rc;
            if (i > 0) {
                const bool win_early = level_early(i) && !p->win_ev.empty();
                int alo = 0, alen = 0;
                bool acc = false;
                if (win_early) {
                    // the window part is already in dz_dec[i-1] (side stream): wait for it, add inside the window (a
                    // launch still sitting in the queue -- win_ev[i] would be last step's record -- is issued now)
                    bool queued = false;
                    for (const PendingWin& pw : pend_win) queued = queued || pw.i == i;
                    if (ig_down && queued && (rc = flush_wgrads())) return rc;
                    if (ig_down && s2 != s) HIP_TRY(hipStreamWaitEvent(s, p->win_ev[(size_t)i], 0));
                    w_range(i, alo, alen);
                    acc = true;
                } else if (p->dedup) {
                    e_range(i - 1, alo, alen);        // the even half of skip window i-1's gradient is already there
                    acc = alen > 0;
                }
                if ((rc = tconv2(ig_down, i, false, acc, alo, (unsigned)alen, s, ws + p->conv_part_off, p->conv_part_floats / 2))) return rc;
                if (!win_early) {
                    if (p->dedup) {
                        if (d.n_odd > 0 && (rc = tconv2(ig_down, i, true, true, 0, 0u, s, ws + p->conv_part_off, p->conv_part_floats / 2)))
                            return rc;
                    } else {
                        ConvArgs a = window_dgrad_args(i);
                        a.flags = F_ACCUM;
                        HIP_TRY(dispatch(ig_down, a, ws + p->conv_part_off, p->conv_part_floats / 2, s));
                    }
                }
            }
        }
    }
    // d_mix: every writer of level 0's d(pre-activation) -- level 1's input gradient, including the early window launches whose
    // win_ev the caller's stream has waited for -- is complete on `s`.  Not a tuned launch position (no conv_dispatch).
    if (mix) HIP_TRY(launch_mix_grad(*mix, s));
    if ((rc = flush_wgrads())) return rc;
    if ((rc = stream_dep(p, s3, s))) return rc;
    if ((rc = stream_dep(p, s2, s))) return rc;      // all gradients are complete w.r.t. `stream`
    if ((rc = sig.ready(0, s))) return rc;           // any bucket not yet signalled (e.g. single-stream mode)
    return WUN_OK;
}

// TF-Adam's step size (Training.py:77): lr * sqrt(1 - b2^t) / (1 - b1^t)
static float adam_lr_t(int64_t step, float lr, float beta1, float beta2) {
    const double lr_t = (double)lr * std::sqrt(1.0 - std::pow((double)beta2, (double)step)) /
                        (1.0 - std::pow((double)beta1, (double)step));
    return (float)lr_t;
}

extern "C" int wun_adam_step(const wun_plan* p, float* params, const float* grads, float* m, float* v,
                             int64_t step, float lr, float beta1, float beta2, float eps, float grad_scale,
                             void* stream) {
    if (!p || !params || !grads || !m || !v) return fail(WUN_ERR_INVALID, "null argument");
    if (step < 1) return fail(WUN_ERR_INVALID, "step is 1-based");
    HIP_TRY(launch_adam(params, grads, m, v, p->arena, adam_lr_t(step, lr, beta1, beta2), beta1, beta2, eps, grad_scale,
                        (hipStream_t)stream));
    return WUN_OK;
}

// The selected tensors' floats as runs of consecutive arena floats (adjacent tensors merge), WUN_ADAM_RANGES runs per launch.
extern "C" int wun_adam_step_select(const wun_plan* p, float* params, const float* grads, float* m, float* v,
                                    int64_t step, float lr, float beta1, float beta2, float eps, float grad_scale,
                                    void* stream, const uint8_t* select, int64_t nselect) {
    if (!p || !params || !grads || !m || !v) return fail(WUN_ERR_INVALID, "null argument");
    if (step < 1) return fail(WUN_ERR_INVALID, "step is 1-based");
    const int64_t nt = (int64_t)p->tensors.size();
    if (!select) {
        if (nselect != 0 && nselect != nt) return fail(WUN_ERR_INVALID, "nselect must be 0 or num_tensors when select is NULL");
        return wun_adam_step(p, params, grads, m, v, step, lr, beta1, beta2, eps, grad_scale, stream);
    }
    if (nselect != nt) return fail(WUN_ERR_INVALID, "nselect must equal num_tensors");
    const float lr_t = adam_lr_t(step, lr, beta1, beta2);
    hipStream_t s = (hipStream_t)stream;
    AdamRanges r;
    memset(&r, 0, sizeof(r));
    for (int64_t k = 0; k < nt; ++k) {
        if (!select[k]) continue;
        const wun_tensor_info& t = p->tensors[(size_t)k];
        long long n = 1;
        for (int d = 0; d < t.ndim; ++d) n *= t.shape[d];
        if (r.n > 0 && r.off[r.n - 1] + (r.cum[r.n] - r.cum[r.n - 1]) == t.offset) { r.cum[r.n] += n; continue; }
        if (r.n == WUN_ADAM_RANGES) {
            HIP_TRY(launch_adam_ranges(params, grads, m, v, r, lr_t, beta1, beta2, eps, grad_scale, s));
            memset(&r, 0, sizeof(r));
        }
        r.off[r.n] = t.offset; r.cum[r.n + 1] = r.cum[r.n] + n; ++r.n;
    }
    if (r.n > 0) HIP_TRY(launch_adam_ranges(params, grads, m, v, r, lr_t, beta1, beta2, eps, grad_scale, s));
    return WUN_OK;
}


// ---------------------------------------------------------------------------------------
// global gradient norm and the clipped Adam step (tf.clip_by_global_norm + AdamOptimizer)
// ---------------------------------------------------------------------------------------
// norm workspace: [0, nt) per-tensor norms, [nt] the global norm, float64 chunk partials from the next even float on
static long long norm_partial_off(const wun_plan* p) { return ((long long)p->tensors.size() + 2) & ~1LL; }

extern "C" int64_t wun_grad_norm_workspace_floats(const wun_plan* p) {
    if (!p) return fail(WUN_ERR_INVALID, "null plan");
    return norm_partial_off(p) + 2 * (long long)p->norm_chunks.size();
}

// host-side checks of the norm's arguments (no GPU work): the selection as a bit set and its float count
static int norm_args(const wun_plan* p, const float* grads, const float* norm_ws, const uint8_t* select, int64_t nselect,
                     NormSelect& sel, long long& nfloats) {
    if (!grads || !norm_ws) return fail(WUN_ERR_INVALID, "null argument");
    if (reinterpret_cast<uintptr_t>(norm_ws) & 7) return fail(WUN_ERR_INVALID, "norm_ws must be 8-byte aligned");
    const int64_t nt = (int64_t)p->tensors.size();
    if (!select && nselect != 0 && nselect != nt) return fail(WUN_ERR_INVALID, "nselect must be 0 or num_tensors when select is NULL");
    if (select && nselect != nt) return fail(WUN_ERR_INVALID, "nselect must equal num_tensors");
    if (nt > WUN_NORM_MAX_TENSORS) return fail(WUN_ERR_UNSUPPORTED, "wun_grad_norm: more than 256 tensors");
    memset(&sel, 0, sizeof(sel));
    nfloats = 0;
    for (int64_t k = 0; k < nt; ++k) {
        if (select && !select[k]) continue;
        sel.bits[k >> 5] |= 1u << (k & 31);
        for (int c = p->norm_first[(size_t)k]; c < p->norm_first[(size_t)k + 1]; ++c) nfloats += p->norm_chunks[(size_t)c].len;
    }
    return WUN_OK;
}

static int grad_norm_launch(const wun_plan* p, const float* grads, float grad_scale, float* norm_ws, const NormSelect& sel,
                            long long nfloats, hipStream_t s) {
    if (!p->dev_norm_chunks) return fail(WUN_ERR_HIP, "plan was created without a usable HIP device");
    HIP_TRY(launch_grad_norm(grads, p->dev_norm_chunks, p->dev_norm_first, (int)p->norm_chunks.size(), (int)p->tensors.size(),
                             sel, nfloats, grad_scale, norm_ws, reinterpret_cast<double*>(norm_ws + norm_partial_off(p)), s));
    return WUN_OK;
}

extern "C" int wun_grad_norm(const wun_plan* p, const float* grads, float grad_scale, float* norm_ws, void* stream,
                             const uint8_t* select, int64_t nselect) {
    if (!p) return fail(WUN_ERR_INVALID, "null plan");
    NormSelect sel;
    long long nfloats;
    int rc;
    if ((rc = norm_args(p, grads, norm_ws, select, nselect, sel, nfloats))) return rc;
    return grad_norm_launch(p, grads, grad_scale, norm_ws, sel, nfloats, (hipStream_t)stream);
}

extern "C" int wun_adam_step_clip(const wun_plan* p, float* params, const float* grads, float* m, float* v,
                                  int64_t step, float lr, float beta1, float beta2, float eps, float grad_scale,
                                  float clip_norm, int32_t flags, float* norm_ws, int64_t* skipped,
                                  void* stream, const uint8_t* select, int64_t nselect) {
    if (!p || !params || !grads || !m || !v) return fail(WUN_ERR_INVALID, "null argument");
    if (step < 1) return fail(WUN_ERR_INVALID, "step is 1-based");
    if (!(clip_norm > 0.f)) return fail(WUN_ERR_INVALID, "clip_norm must be > 0 (+INFINITY = no clipping)");
    if (flags & ~WUN_CLIP_SKIP_NONFINITE) return fail(WUN_ERR_INVALID, "unknown flags");
    const int skip = (flags & WUN_CLIP_SKIP_NONFINITE) ? 1 : 0;
    if (skip && !skipped) return fail(WUN_ERR_INVALID, "skipped is required with WUN_CLIP_SKIP_NONFINITE");
    NormSelect sel;
    long long nfloats;
    int rc;
    if ((rc = norm_args(p, grads, norm_ws, select, nselect, sel, nfloats))) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = grad_norm_launch(p, grads, grad_scale, norm_ws, sel, nfloats, s))) return rc;
    const float lr_t = adam_lr_t(step, lr, beta1, beta2);
    const float* gnorm = norm_ws + p->tensors.size();
    long long* cnt = skip ? reinterpret_cast<long long*>(skipped) : nullptr;
    if (!select) {
        HIP_TRY(launch_adam_clip(params, grads, m, v, p->arena, lr_t, beta1, beta2, eps, grad_scale, gnorm, clip_norm, skip, cnt, s));
        return WUN_OK;
    }
    // the runs of wun_adam_step_select; only the first launch counts a skipped step
    AdamRanges r;
    memset(&r, 0, sizeof(r));
    for (size_t k = 0; k < p->tensors.size(); ++k) {
        if (!select[k]) continue;
        const wun_tensor_info& t = p->tensors[k];
        long long n = 1;
        for (int d = 0; d < t.ndim; ++d) n *= t.shape[d];
        if (r.n > 0 && r.off[r.n - 1] + (r.cum[r.n] - r.cum[r.n - 1]) == t.offset) { r.cum[r.n] += n; continue; }
        if (r.n == WUN_ADAM_RANGES) {
            HIP_TRY(launch_adam_clip_ranges(params, grads, m, v, r, lr_t, beta1, beta2, eps, grad_scale, gnorm, clip_norm, skip,
                                            cnt, s));
            cnt = nullptr;
            memset(&r, 0, sizeof(r));
        }
        r.off[r.n] = t.offset; r.cum[r.n + 1] = r.cum[r.n] + n; ++r.n;
    }
    if (r.n > 0)
        HIP_TRY(launch_adam_clip_ranges(params, grads, m, v, r, lr_t, beta1, beta2, eps, grad_scale, gnorm, clip_norm, skip, cnt, s));
    return WUN_OK;
}
