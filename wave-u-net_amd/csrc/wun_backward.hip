// Host side of libwun.so: the backward pass of the training step -- loss + backward (wun_loss_backward*) or backward from an
// upstream gradient (wun_backward*), for all variables or a selection, overwriting or accumulating -- as a launch sequence
// on the caller's stream and the plan's side streams.
#include "wun_plan_impl.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

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

static int check_buckets(const int64_t* bucket_starts, void* const* bucket_events, int32_t nbuckets) {
    if (nbuckets < 0 || (nbuckets > 0 && (!bucket_starts || !bucket_events))) return fail(WUN_ERR_INVALID, "bad bucket arguments");
    for (int k = 1; k < nbuckets; ++k)
        if (bucket_starts[k] >= bucket_starts[k - 1]) return fail(WUN_ERR_INVALID, "bucket_starts must be strictly descending");
    return WUN_OK;
}

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
    sel.wgrad.assign((size_t)(3 * L + 3), 0);
    int rc;
    if ((rc = check_nselect(p, select, nselect))) return rc;
    int64_t k = 0;
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

// d_mix: where the audio's gradient lives after the backward pass -- down conv 0's d(pre-activation) in the launch geometries of
// its forward pass (down_parts: the parts the level-0 weight gradient reads), the head's d(pre-activation) and the difference
// output's upstream gradient
static int mix_grad_args(const wun_plan* p, const float* params, float* ws, const float* d_outputs, float* d_mix, MixGradArgs& m) {
    memset(&m, 0, sizeof(m));
    DownPart part[2];
    m.nparts = down_parts(p, 0, part);
    for (int k = 0; k < m.nparts; ++k) {
        const Buf& z = *part[k].dz;
        m.part[k] = MixGradPart{ws + z.off, z.bs, z.pitch, part[k].Tq, part[k].stride, part[k].off, part[k].shift, part[k].Tin};
        if (z.eb != part[0].dz->eb) return fail(WUN_ERR_UNSUPPORTED, "d_mix: level-0 gradient parts of different element types");
    }
    m.dzbf = part[0].dz->eb == 2 ? 1 : 0;
    m.W = params + p->down[0].woff; m.KW = p->cfg.filter_size; m.F = p->cfg.num_initial_filters;
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

// What one backward call asks for.  The head of the pass is "MSE against targets" (loss_head: head_bwd_kernel + loss_finish,
// needs targets and loss) or "upstream gradient" (head_grad_kernel from d_outputs); everything after the head's
// d(pre-activation) is one pass.  grads_optional: grads may be NULL when no tensor is selected (the input-only gradient of
// wun_backward_select / _accumulate); every other entry refuses a NULL grads outright.  accum: the final gradient stores add
// to `grads` (wun_*_accumulate); everything else is the overwriting call.
struct BackwardRequest {
    bool loss_head; const float* targets; float* loss; const float* d_outputs;
    float* grads; bool grads_optional; float* d_mix;
    const int64_t* bucket_starts; void* const* bucket_events; int32_t nbuckets;
    const uint8_t* select; int64_t nselect;
    bool accum;
};

// The pass itself: the state its steps share and the steps in the order run() calls them.  Three invariants every step keeps:
//  * launch positions -- p->ci counts the conv launches and p->wi the weight-gradient layers of the FULL pass, in order: a
//    launch a selection leaves out (live == false) still takes its position, so that every launch that does run gets the
//    tuned choice of the full pass;
//  * side-stream rotation -- every weight-gradient layer, interpolation-weight gradient and early window launch takes the
//    next turn of wstream(), left out or not;
//  * flushes -- side-stream work is queued (pend, pend_win, pend_interp) and issued by flush_wgrads() behind ONE event on the
//    caller's stream, once per layer (submit_wgrad), before level 0's narrow weight gradient, and at the end.
struct BackwardPass {
    const wun_plan* p; const float* params; float* ws; float* grads;
    hipStream_t s, s2, s3;          // the caller's stream; the side streams (== s when there are none)
    const BackwardSelect& sel; const bool accum;
    BucketSignal sig;
    const int L, Kd, Ku, padD, padU;
    const long long cpart_half, cpart_q;
    bool early_win = false, early_all = false;
    int wg_rr = 0;
    struct PendingWgrad { WgradArgs w[2]; int n; const ConvLayer* cl; bool live; };
    struct PendingWin { int i; bool live; };
    std::vector<PendingWgrad> pend; std::vector<PendingWin> pend_win; std::vector<UpsampleBwdArgs> pend_interp;   // queued side-stream work

    BackwardPass(const wun_plan* p_, const float* params_, float* ws_, float* grads_, hipStream_t s_, const BackwardSelect& sel_,
                 bool accum_, BucketSignal sig_)
        : p(p_), params(params_), ws(ws_), grads(grads_), s(s_), s2(s_), s3(s_), sel(sel_), accum(accum_), sig(sig_), L(p_->L),
          Kd(p_->cfg.filter_size), Ku(p_->cfg.merge_filter_size), padD(p_->same ? (Kd - 1) / 2 : 0),
          padU(p_->same ? (Ku - 1) / 2 : 0), cpart_half(p_->conv_part_floats / 2),
          cpart_q(p_->conv_part_floats / 4) {}

    float* chain_part() const { return ws + p->conv_part_off; }       // split-K scratch of the chain on `s`: the first half
    // side streams: weight gradients + their reductions, alternating between two streams so the
    // ramp-up / drain of consecutive (independent) weight-gradient kernels overlap
    hipStream_t wstream() { return (wg_rr++ & 1) ? s3 : s2; }
    hipError_t dispatch(bool live, const ConvArgs& a, float* part, long long cap, hipStream_t st) {
        if (!live) { ++p->ci; return hipSuccess; }
        return conv_dispatch(p, a, part, cap, st);
    }
    // bucket events are recorded on s2 once it has also seen everything queued on s3
    int ready2(long long floor) {
        if (s3 != s2 && sig.next < sig.n && sig.starts[sig.next] >= floor) {
            int rcj = stream_dep(p, s3, s2);
            if (rcj) return rcj;
        }
        return sig.ready(floor, s2);
    }

    struct Range { int lo = 0, len = 0; };                             // positions [lo, lo + len) of a dz_dec row
    Range e_range(int i) const { return {p->dsh[i].t_ev0 / 2, p->dsh[i].n_even}; }
    Range w_range(int i) const;
    bool level_fused(int i) const;
    bool level_early(int i) const;
    ConvArgs window_dgrad_args(int i) const;
    int tconv2(bool live, int i, bool odd, bool acc, int acc_lo, unsigned acc_len, hipStream_t st, float* part, long long cap);
    int flush_wgrads();
    int submit_wgrad(const WgradArgs* w, int n, const ConvLayer& cl, bool live);

    int begin();
    int head(const float* outputs, const BackwardRequest& rq);
    int up_level(int j);
    int bottleneck();
    int down_level(int i), down_dgrad(int i);
    int finish(const MixGradArgs* mix);
    int run(const float* outputs, const BackwardRequest& rq, const MixGradArgs* mix);
};

// Early skip-window input gradients (context mode).  The input gradient of down level i is the transposed stride-2
// conv of dz_dec[i] over the whole row PLUS the full-rate conv of dz_skip[i] over the crop window.  dz_skip[i] is
// final as soon as up level L-1-i's input gradient has run -- the shallow, FLOP-heavy levels' at the very start of
// the backward pass -- while the row-wide part can only run when the dependent chain reaches level i at its very
// end.  The window part is therefore launched as soon as its input exists, on the side streams (it fills the
// launch-latency-bound deep part of the chain instead of lengthening the FLOP-bound end of it), stores into the
// window of dz_dec[i-1], and the row-wide conv later ADDS inside the window (ConvArgs.acc_lo / acc_len) and stores
// outside it: a + b == b + a, results are bit-identical to the old order.  Queued in pend_win, issued by the next flush
// (whose event already orders the side streams behind the producing kernels: no extra packet on the chain).
// Only the deep levels (input gradient = separate phase launches on a launch-latency-bound chain): same-box A/B
// 8.84 -> 8.82 ms; moving the FLOP-heavy levels' window parts too changed nothing (8.98 vs 8.99: the end of the backward
// pass is throughput-bound, not chain-bound).  WUN_EARLY_WINDOW=0 restores the old order (other launch order: the
// tuning-table header records it).
bool BackwardPass::level_fused(int i) const {                        // (the rule of tconv2 for the row-wide conv)
    const DownShape& d = p->dsh[i];
    ConvArgs f = conv_base(p);
    f.Tin = d.t_dec; f.KW = p->down[i].J0; f.kw_full = Kd; f.N = f.N0 = d.cin; f.Tout = (d.t_in + 1) / 2; f.Tlim = d.t_in;
    f.flags = F_PHASE2; f.C0 = d.cout; f.B = p->B;
    return (d.cin & 3) == 0 && f.Tout >= 256 && conv_natural_wgs_phase2(f) >= 256;
}

// dedup plans: ranges of dz_dec[i - 1] that two more writers touch before / beside the row-wide transposed conv of level i --
// E (e_range) = the even half of skip window i - 1's gradient (stored by up level L - i's input gradient), W (w_range) = the
// input gradient of level i's odd window positions.  The early form of W (it ADDS inside E and stores elsewhere; the row-wide
// conv then adds inside W) needs E inside W, which the centred crops of every shipped config give; else W runs after the
// row-wide conv.
BackwardPass::Range BackwardPass::w_range(int i) const {
    const DownShape& d = p->dsh[i];
    if (p->dedup) return {d.t_odd0, d.n_odd > 0 ? 2 * (d.n_odd - 1) + Kd : 0};
    return {d.cs, d.tc + Kd - 1};
}

// Which levels' window input gradients leave the dependent chain.  Dedup plans (round 6): ALL of them -- the odd-window
// launches are half the size of the old window convs, and for the middle levels (row-wide part fused, window part too
// small to fuse) the chain otherwise carries two phase launches + their split-K epilogues per level: same-box A/B, each arm
// autotuned, 8.14 -> 8.03 ms per step, 7.94 together with the lower fuse floor of tconv2 (profiles/round6_ab_dedup_schedule.txt).
// Rounds 3 - 5 (full-window convs): only the deep levels, moving the FLOP-heavy ones changed nothing (8.98 vs 8.99).
// WUN_EARLY_WINDOW=deep | all | 0 overrides (a non-default mode is part of the tuning-table header).
bool BackwardPass::level_early(int i) const {
    if (!(early_win && i > 0 && (early_all || !level_fused(i)))) return false;
    if (!p->dedup) return true;
    const Range e = e_range(i - 1), w = w_range(i);
    return w.len > 0 && (e.len == 0 || (w.lo <= e.lo && e.lo + e.len <= w.lo + w.len));
}

// the full-rate window part of level i's input gradient (plans without dedup)
ConvArgs BackwardPass::window_dgrad_args(int i) const {
    const DownShape& d = p->dsh[i];
    const ConvLayer& cl = p->down[i];
    ConvArgs a = conv_base(p);
    set_src0(a, ws, p->dz_skip[i], 0, d.cout);
    a.Tin = d.tc; a.shift = Kd - 1; a.W = ws + cl.wt_full; a.KW = Kd;
    a.N = a.N0 = d.cin; a.Tout = d.tc + Kd - 1;
    set_dst0(a, ws, p->dz_dec[i - 1], d.cs, &p->dec[i - 1]);
    return a;
}

// Transposed stride-2 conv of down level i into dz_dec[i - 1] (masked with dec[i - 1]'s LeakyReLU branch): of the decimated
// stream's gradient dz_dec[i] over the whole row (odd = false), or -- dedup plans -- of the odd window positions' gradient
// dz_odd[i] into [t_odd0, t_odd0 + 2 (n_odd - 1) + Kd) (odd = true).  Both output phases fused in one launch (a lane owns 8
// consecutive outputs) when the launch fills the chip, else one phase at a time (those launches can use split-K).
// acc: add to what the row holds inside [acc_lo, acc_lo + acc_len) (acc_len == 0: everywhere), store elsewhere.
int BackwardPass::tconv2(bool live, int i, bool odd, bool acc, int acc_lo, unsigned acc_len, hipStream_t st, float* part,
                         long long cap) {
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
    if (acc) { f.flags |= F_ACCUM; f.acc_lo = acc_lo; f.acc_len = acc_len; }
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
        if (acc) { a.flags |= F_ACCUM; a.acc_lo = acc_lo; a.acc_len = acc_len; }
        if (a.Tout > 0) HIP_TRY(dispatch(live, a, part, cap, st));
    }
    return WUN_OK;
}

// Weight gradients are queued and flushed one layer at a time: one event on the caller's stream per layer, both side
// streams wait on it.  (Batching several deep levels behind one event -- every event is a barrier packet that holds
// the dependent chain for ~7 us -- was measured in round 2: 41 -> 26 stalls per step, but the delayed weight gradients
// lengthen the tail after the last input gradient by more: 9.12 ms per step with one layer per event, 9.19 - 9.23 with 2 - 5.)
// Order behind the event: the interpolation-weight gradients, the weight-gradient layers (each followed by its bucket signal),
// the early window input gradients.
int BackwardPass::flush_wgrads() {
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
        float* part = sw == s ? chain_part() : chain_part() + cpart_half + ((sw == s3 && s3 != s2) ? cpart_q : 0);
        const long long cap = sw == s ? cpart_half : cpart_q;
        if (p->dedup) {
            const Range e = e_range(i - 1);
            int rcw = tconv2(pw.live, i, true, e.len > 0, e.lo, (unsigned)e.len, sw, part, cap);
            if (rcw) return rcw;
        } else {
            HIP_TRY(dispatch(pw.live, window_dgrad_args(i), part, cap, sw));
        }
        if (sw != s && pw.live) HIP_TRY(hipEventRecord(p->win_ev[(size_t)i], sw));
    }
    pend_win.clear();
    return WUN_OK;
}

int BackwardPass::submit_wgrad(const WgradArgs* w, int n, const ConvLayer& cl, bool live) {
    PendingWgrad q;
    for (int k = 0; k < n; ++k) q.w[k] = w[k];
    q.n = n; q.cl = &cl; q.live = live;
    pend.push_back(q);
    return flush_wgrads();
}

// streams, launch positions, the events of the early windows, the transposed weight copies
int BackwardPass::begin() {
    if (!p->wt.empty() && !p->dev_wt) return fail(WUN_ERR_HIP, "plan was created without a usable HIP device");
    int rc;
    if ((rc = side_init(p))) return rc;
    p->ci = 0; p->wi = 0; p->in_bwd = true;
    s2 = (p->side && !g_profiling && p->tune_mode != 1) ? p->side : s;
    s3 = (p->side2 && s2 != s) ? p->side2 : s2;
    early_win = !p->same && !p->bf16 && p->early_window != EW_OFF;
    early_all = p->early_window == EW_ALL;
    if (early_win && p->win_ev.size() < (size_t)L) {
        p->win_ev.resize(L, nullptr);
        for (auto& e : p->win_ev)
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e, event_flags(p)));
    }
    if (p->wt_ready) {
        HIP_TRY(hipStreamWaitEvent(s, p->wt_ev, 0));       // made during the forward pass
        p->wt_ready = false;
    } else {
        HIP_TRY(launch_make_wt(params, ws, p->dev_wt, (int)p->wt.size(), p->wt_max, s));
        if (p->bf16)
            HIP_TRY(launch_pack_bf16(params, ws, p->dev_pack + p->npack_fwd, (int)p->pack.size() - p->npack_fwd, p->pack_max, s));
    }
    p->cur_params = params; p->cur_ws = ws;
    return WUN_OK;
}

// ---- head: loss, d(pre-activation), d(feature map); the output layer's weight gradient ----
int BackwardPass::head(const float* outputs, const BackwardRequest& rq) {
    const int F = p->cfg.num_initial_filters, C = p->C, Ko = p->cfg.output_filter_size;
    int rc;
    HeadArgs h = head_args(p, params, ws, const_cast<float*>(outputs), 1);
    long long hoff[4] = {0, 0, 0, 0};
    for (int i = 0; i < p->Sh; ++i) hoff[i] = p->head[i].woff;
    if (rq.loss_head) {
        h.tgt = rq.targets;
        HIP_TRY(launch_head_bwd_off(h, hoff, s));
        HIP_TRY(launch_loss_finish(h.loss_partial, head_bwd_blocks(h),
                                   1.0f / ((float)p->S * (float)p->B * (float)p->Tout * (float)p->C), rq.loss, s));
    } else {
        h.dout = rq.d_outputs;
        HIP_TRY(launch_head_grad_off(h, hoff, s));
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
    return WUN_OK;
}

// ---- up level j: weight gradient, input gradient (skip window i = L - 1 - j and the upsampled tensor), adjoint upsampling ----
int BackwardPass::up_level(int j) {
    const UpShape& u = p->ush[j];
    const int i = L - 1 - j;
    const Buf& prev = (j == 0) ? p->bott_out : p->upo[j - 1];
    const Buf& dzprev = (j == 0) ? p->dz_bott : p->dz_upo[j - 1];
    int rc;
    WgradArgs w = wgrad_base(p);
    wset_src0(w, ws, p->skip[i], 0, u.c_skip);
    wset_src1(w, ws, p->ups[j], 0, u.c_cur);
    w.Tin = u.t_up; w.shift = padU; w.KW = Ku;
    wset_dz(w, ws + p->dz_upo[j].off, p->dz_upo[j].bs, p->dz_upo[j].pitch, u.cout, u.t_conv);
    // (interp_j, written on `s` by the previous level's upsample_bwd, sits above up[j] in
    // the arena; the flush makes the side streams wait for everything issued on `s` so far)
    if ((rc = submit_wgrad(&w, 1, p->up[j], sel.wg(sel.up(L, j))))) return rc;

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
    // linear interpolation: a launch that ends in the split-K epilogue kernel applies the adjoint of the 2x
    // upsampling there (ConvArgs.ubw_*) instead of storing d_ups[j] for upsample_bwd_vec_kernel
    if (p->fuse_ups && p->interp[j] < 0 && dzprev.bs == prev.bs && dzprev.pitch == prev.pitch) {
        a.ubw_dz = ws + dzprev.off; a.ubw_x = ws + prev.off; a.ubw_bs = prev.bs; a.ubw_pitch = prev.pitch;
        a.ubw_n = u.t_cur;
    }
    const bool live = sel.ig(sel.up(L, j));
    HIP_TRY(dispatch(live, a, chain_part(), cpart_half, s));
    const bool adj_done = a.ubw_dz != nullptr && conv_last_fused_ups() != 0;
    // dz_skip[i] is final: its window input gradient can start
    if (level_early(i)) pend_win.push_back(PendingWin{i, sel.ig(sel.down(i))});
    if (!live || adj_done) return WUN_OK;                  // (!live: interp_j and everything before it are not needed)

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
    return WUN_OK;
}

int BackwardPass::bottleneck() {
    int rc;
    WgradArgs w = wgrad_base(p);
    wset_src0(w, ws, p->dec[L - 1], 0, p->bott.Cin);
    w.Tin = p->t_b_in; w.shift = padD; w.KW = Kd;
    wset_dz(w, ws + p->dz_bott.off, p->dz_bott.bs, p->dz_bott.pitch, p->c_b, p->t_b);
    if ((rc = submit_wgrad(&w, 1, p->bott, sel.wg(sel.bott(L))))) return rc;
    ConvArgs a = conv_base(p);
    set_src0(a, ws, p->dz_bott, 0, p->c_b);
    a.Tin = p->t_b; a.shift = Kd - 1 - padD; a.W = ws + p->bott.wt_full; a.KW = Kd;
    a.N = a.N0 = p->bott.Cin; a.Tout = p->t_b_in;
    if (p->same) {
        set_dst0(a, ws, p->dz_skip[L - 1], 0, &p->skip[L - 1]);
        a.ostride = 2; a.flags = F_ACCUM;
    } else {
        set_dst0(a, ws, p->dz_dec[L - 1], 0, &p->dec[L - 1]);
        if (p->dedup && p->dsh[L - 1].n_even > 0) {
            // (the even half of skip window L-1's gradient is already there)
            const Range e = e_range(L - 1);
            a.flags = F_ACCUM; a.acc_lo = e.lo; a.acc_len = (unsigned)e.len;
        }
    }
    HIP_TRY(dispatch(sel.ig(sel.bott(L)), a, chain_part(), cpart_half, s));
    return WUN_OK;
}

// ---- down level i: the weight gradient over its forward parts (down_parts), then its input gradient ----
int BackwardPass::down_level(int i) {
    const DownShape& d = p->dsh[i];
    const ConvLayer& cl = p->down[i];
    const Buf& x = (i == 0) ? p->mix_ncw : p->dec[i - 1];
    const bool wg_down = sel.wg(sel.down(i));
    DownPart part[2];
    const int nparts = down_parts(p, i, part);
    int rc;
    // the audio-input conv (1 or 2 input channels): direct reduction instead of MFMA tiles (10 TFLOP/s of mostly
    // padding); WUN_NO_NARROW_DOWN0=1 keeps the MFMA kernel (A/B: 9.36 -> 9.32 ms per step with the narrow kernel)
    if (i == 0) {
        NarrowWgradArgs nw[2];
        memset(nw, 0, sizeof(nw));
        bool narrow = p->bf16 || (!p->sw.no_narrow && !p->sw.no_narrow_down0);
        for (int k = 0; k < nparts; ++k) {
            const Buf& z = *part[k].dz;
            nw[k].src0 = ws + x.off; nw[k].bs0 = x.bs; nw[k].pitch0 = x.pitch; nw[k].C0 = d.cin; nw[k].off0 = part[k].off;
            nw[k].Tin = part[k].Tin; nw[k].shift = part[k].shift; nw[k].stride = part[k].stride; nw[k].KW = Kd;
            nw[k].dz = ws + z.off; nw[k].dzbs = z.bs; nw[k].dzpitch = z.pitch; nw[k].Tq = part[k].Tq;
            nw[k].N = nw[k].Nper = d.cout; nw[k].B = p->B;
            nw[k].et = p->bf16 ? 4 : 0;                           // fp32 audio, (bf16) dz
            narrow = narrow && narrow_wgrad_supported(nw[k]);
        }
        // (bf16 mode: the narrow kernels are the only ones that read fp32 audio against bf16 gradients)
        if (p->bf16 && !narrow) return fail(WUN_ERR_UNSUPPORTED, "bf16 mode: audio-input conv shape not served by the narrow weight-gradient kernels");
        if (narrow) {
            if ((rc = flush_wgrads())) return rc;
            const long long woff[4] = {cl.woff, 0, 0, 0}, boff[4] = {cl.boff, 0, 0, 0};
            hipStream_t sw = wstream();
            if (wg_down && (rc = run_narrow_wgrad(p, nw, nparts, woff, boff, ws, grads, s, sw, accum))) return rc;
            return ready2(cl.woff);
        }
    }
    WgradArgs w[2];
    for (int k = 0; k < nparts; ++k) {
        const Buf& z = *part[k].dz;
        w[k] = wgrad_base(p);
        wset_src0(w[k], ws, x, part[k].off, d.cin);
        w[k].loader = part[k].loader; w[k].Tin = part[k].Tin; w[k].shift = part[k].shift; w[k].KW = Kd;
        wset_dz(w[k], ws + z.off, z.bs, z.pitch, d.cout, part[k].Tq);
    }
    if ((rc = submit_wgrad(w, nparts, cl, wg_down))) return rc;
    return i > 0 ? down_dgrad(i) : WUN_OK;
}

// input gradient of down level i > 0, into the d(pre-activation) of level i - 1
int BackwardPass::down_dgrad(int i) {
    const DownShape& d = p->dsh[i];
    const ConvLayer& cl = p->down[i];
    const bool ig_down = sel.ig(sel.down(i));
    int rc;
    if (p->same) {
        ConvArgs a = conv_base(p);
        set_src0(a, ws, p->dz_skip[i], 0, d.cout);
        a.Tin = d.t_conv; a.shift = Kd - 1 - padD; a.W = ws + cl.wt_full; a.KW = Kd;
        a.N = a.N0 = d.cin; a.Tout = d.t_in;
        set_dst0(a, ws, p->dz_skip[i - 1], 0, &p->skip[i - 1]);
        a.ostride = 2; a.flags = F_ACCUM;
        HIP_TRY(dispatch(ig_down, a, chain_part(), cpart_half, s));
        return WUN_OK;
    }
    const bool win_early = level_early(i) && !p->win_ev.empty();
    Range at;                             // where the row-wide conv adds to what the row holds
    bool acc = false;
    if (win_early) {
        // the window part is already in dz_dec[i-1] (side stream): wait for it, add inside the window (a
        // launch still sitting in the queue -- win_ev[i] would be last step's record -- is issued now)
        bool queued = false;
        for (const PendingWin& pw : pend_win) queued = queued || pw.i == i;
        if (ig_down && queued && (rc = flush_wgrads())) return rc;
        if (ig_down && s2 != s) HIP_TRY(hipStreamWaitEvent(s, p->win_ev[(size_t)i], 0));
        at = w_range(i);
        acc = true;
    } else if (p->dedup) {
        at = e_range(i - 1);              // the even half of skip window i-1's gradient is already there
        acc = at.len > 0;
    }
    if ((rc = tconv2(ig_down, i, false, acc, at.lo, (unsigned)at.len, s, chain_part(), cpart_half))) return rc;
    if (win_early) return WUN_OK;
    if (p->dedup) {
        if (d.n_odd > 0 && (rc = tconv2(ig_down, i, true, true, 0, 0u, s, chain_part(), cpart_half))) return rc;
    } else {
        ConvArgs a = window_dgrad_args(i);
        a.flags = F_ACCUM;
        HIP_TRY(dispatch(ig_down, a, chain_part(), cpart_half, s));
    }
    return WUN_OK;
}

int BackwardPass::finish(const MixGradArgs* mix) {
    int rc;
    // d_mix: every writer of level 0's d(pre-activation) -- level 1's input gradient, including the early window launches whose
    // win_ev the caller's stream has waited for -- is complete on `s`.  Not a tuned launch position (no conv_dispatch).
    if (mix) HIP_TRY(launch_mix_grad(*mix, s));
    if ((rc = flush_wgrads())) return rc;
    if ((rc = stream_dep(p, s3, s))) return rc;
    if ((rc = stream_dep(p, s2, s))) return rc;      // all gradients are complete w.r.t. `stream`
    return sig.ready(0, s);                          // any bucket not yet signalled (e.g. single-stream mode)
}

int BackwardPass::run(const float* outputs, const BackwardRequest& rq, const MixGradArgs* mix) {
    int rc;
    if ((rc = begin())) return rc;
    if ((rc = head(outputs, rq))) return rc;
    for (int j = L - 1; j >= 0; --j)                 // up path, last level first
        if ((rc = up_level(j))) return rc;
    if ((rc = bottleneck())) return rc;
    for (int i = L - 1; i >= 0; --i)
        if ((rc = down_level(i))) return rc;
    return finish(mix);
}

// The one path every backward entry takes: argument checks (host work only, before any GPU work), then the pass.
static int backward(const wun_plan* p, const float* params, float* ws, const float* outputs, void* stream,
                    const BackwardRequest& rq) {
    int rc;
    if ((rc = check_buckets(rq.bucket_starts, rq.bucket_events, rq.nbuckets))) return rc;
    if (!p || !params || !ws || !outputs || (rq.loss_head ? (!rq.targets || !rq.loss) : !rq.d_outputs) ||
        (!rq.grads && !rq.grads_optional))
        return fail(WUN_ERR_INVALID, "null argument");
    BackwardSelect sel;
    bool any = false;
    if ((rc = parse_select(p, rq.select, rq.nselect, rq.d_mix != nullptr, sel, any))) return rc;
    if (any && !rq.grads) return fail(WUN_ERR_INVALID, "null argument: grads (may be NULL only when no tensor is selected)");
    MixGradArgs mix;
    if (rq.d_mix && (rc = mix_grad_args(p, params, ws, rq.d_outputs, rq.d_mix, mix))) return rc;
    BackwardPass pass(p, params, ws, rq.grads, (hipStream_t)stream, sel, rq.accum,
                      BucketSignal{rq.bucket_starts, rq.bucket_events, rq.nbuckets, 0});
    return pass.run(outputs, rq, rq.d_mix ? &mix : nullptr);
}

// ---- the C ABI: mix_btc is accepted (the forward pass left the audio in the workspace) and not read ----
extern "C" int wun_loss_backward(const wun_plan* p, const float* params, const float*, float* ws, const float* outputs,
                                 const float* targets, float* grads, float* loss, void* stream) {
    return backward(p, params, ws, outputs, stream,
                    {true, targets, loss, nullptr, grads, false, nullptr, nullptr, nullptr, 0, nullptr, 0, false});
}

extern "C" int wun_loss_backward_ex(const wun_plan* p, const float* params, const float*, float* ws, const float* outputs,
                                    const float* targets, float* grads, float* loss, void* stream,
                                    const int64_t* bucket_starts, void* const* bucket_events, int32_t nbuckets) {
    return backward(p, params, ws, outputs, stream,
                    {true, targets, loss, nullptr, grads, false, nullptr, bucket_starts, bucket_events, nbuckets, nullptr, 0, false});
}

extern "C" int wun_loss_backward_select(const wun_plan* p, const float* params, const float*, float* ws, const float* outputs,
                                        const float* targets, float* grads, float* loss, void* stream,
                                        const int64_t* bucket_starts, void* const* bucket_events, int32_t nbuckets,
                                        const uint8_t* select, int64_t nselect) {
    return backward(p, params, ws, outputs, stream,
                    {true, targets, loss, nullptr, grads, false, nullptr, bucket_starts, bucket_events, nbuckets, select, nselect, false});
}

extern "C" int wun_loss_backward_accumulate(const wun_plan* p, const float* params, const float*, float* ws,
                                            const float* outputs, const float* targets, float* grads, float* loss,
                                            void* stream, const int64_t* bucket_starts, void* const* bucket_events,
                                            int32_t nbuckets, const uint8_t* select, int64_t nselect) {
    return backward(p, params, ws, outputs, stream,
                    {true, targets, loss, nullptr, grads, false, nullptr, bucket_starts, bucket_events, nbuckets, select, nselect, true});
}

extern "C" int wun_backward(const wun_plan* p, const float* params, const float*, float* ws, const float* outputs,
                            const float* d_outputs, float* grads, float* d_mix, void* stream) {
    return backward(p, params, ws, outputs, stream,
                    {false, nullptr, nullptr, d_outputs, grads, false, d_mix, nullptr, nullptr, 0, nullptr, 0, false});
}

extern "C" int wun_backward_ex(const wun_plan* p, const float* params, const float*, float* ws, const float* outputs,
                               const float* d_outputs, float* grads, float* d_mix, void* stream,
                               const int64_t* bucket_starts, void* const* bucket_events, int32_t nbuckets) {
    return backward(p, params, ws, outputs, stream,
                    {false, nullptr, nullptr, d_outputs, grads, false, d_mix, bucket_starts, bucket_events, nbuckets, nullptr, 0, false});
}

extern "C" int wun_backward_select(const wun_plan* p, const float* params, const float*, float* ws, const float* outputs,
                                   const float* d_outputs, float* grads, float* d_mix, void* stream,
                                   const int64_t* bucket_starts, void* const* bucket_events, int32_t nbuckets,
                                   const uint8_t* select, int64_t nselect) {
    return backward(p, params, ws, outputs, stream,
                    {false, nullptr, nullptr, d_outputs, grads, true, d_mix, bucket_starts, bucket_events, nbuckets, select, nselect, false});
}

extern "C" int wun_backward_accumulate(const wun_plan* p, const float* params, const float*, float* ws, const float* outputs,
                                       const float* d_outputs, float* grads, float* d_mix, void* stream,
                                       const int64_t* bucket_starts, void* const* bucket_events, int32_t nbuckets,
                                       const uint8_t* select, int64_t nselect) {
    return backward(p, params, ws, outputs, stream,
                    {false, nullptr, nullptr, d_outputs, grads, true, d_mix, bucket_starts, bucket_events, nbuckets, select, nselect, true});
}
