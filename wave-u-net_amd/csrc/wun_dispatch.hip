// Host side of libwun.so: kernel argument blocks, the plan's side streams and events, and the autotuned dispatch of
// every conv / weight-gradient launch (its position in the step's launch order selects the tuned choice).
#include "wun_plan_impl.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

// ---------------------------------------------------------------------------------------
// helpers to fill argument blocks
// ---------------------------------------------------------------------------------------
ConvArgs conv_base(const wun_plan* p) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.B = p->B; a.ostride = 1; a.loader = LOADER_DIRECT;
    return a;
}
void set_src0(ConvArgs& a, const float* ws, const Buf& b, int off, int C) {
    a.src0 = ws + b.off; a.bs0 = b.bs; a.pitch0 = b.pitch; a.off0 = off; a.C0 = C;
}
void set_src1(ConvArgs& a, const float* ws, const Buf& b, int off, int C) {
    a.src1 = ws + b.off; a.bs1 = b.bs; a.pitch1 = b.pitch; a.off1 = off; a.C1 = C;
}
void set_dst0(ConvArgs& a, float* ws, const Buf& b, int off, const Buf* mask) {
    a.dst0 = ws + b.off; a.obs0 = b.bs; a.opitch0 = b.pitch; a.ooff0 = off;
    a.msk0 = mask ? ws + mask->off : nullptr;
}
void set_dst1(ConvArgs& a, float* ws, const Buf& b, int off, const Buf* mask) {
    a.dst1 = ws + b.off; a.obs1 = b.bs; a.opitch1 = b.pitch; a.ooff1 = off;
    a.msk1 = mask ? ws + mask->off : nullptr;
}
WgradArgs wgrad_base(const wun_plan* p) {
    WgradArgs w;
    memset(&w, 0, sizeof(w));
    w.B = p->B; w.loader = LOADER_DIRECT;
    return w;
}
void wset_src0(WgradArgs& a, const float* ws, const Buf& b, int off, int C) {
    a.src0 = ws + b.off; a.bs0 = b.bs; a.pitch0 = b.pitch; a.off0 = off; a.C0 = C;
}
void wset_src1(WgradArgs& a, const float* ws, const Buf& b, int off, int C) {
    a.src1 = ws + b.off; a.bs1 = b.bs; a.pitch1 = b.pitch; a.off1 = off; a.C1 = C;
}
void wset_dz(WgradArgs& a, const float* base, long long bs, int pitch, int N, int Tq) {
    a.dz = base; a.dzbs = bs; a.dzpitch = pitch; a.N = N; a.Tq = Tq;
}

HeadArgs head_args(const wun_plan* p, const float* params, float* ws, float* outputs, int training) {
    HeadArgs h;
    memset(&h, 0, sizeof(h));
    const int L = p->L;
    h.mix_ncw = ws + p->mix_ncw.off; h.mbs = p->mix_ncw.bs; h.mpitch = p->mix_ncw.pitch;
    h.moff_feat = p->in_crop_start; h.moff_diff = p->mix_diff_off;
    h.feat = ws + p->upo[L - 1].off; h.fbs = p->upo[L - 1].bs; h.fpitch = p->upo[L - 1].pitch;
    h.Wh = params;
    h.C = p->C; h.F = p->cfg.num_initial_filters; h.S = p->S; h.Sh = p->Sh; h.Ko = p->cfg.output_filter_size;
    h.padl = p->same ? (h.Ko - 1) / 2 : 0;
    h.Tfeat = p->t_feat; h.Tout = p->Tout; h.B = p->B;
    h.tanh_act = p->cfg.output_activation == 0; h.difference = p->cfg.output_type == 1; h.training = training;
    h.out = outputs;
    h.dpre = ws + p->dpre_off; h.dppitch = p->dp_pitch; h.dpbs = (long long)p->C * p->dp_pitch;
    h.dps = (long long)p->B * h.dpbs;
    h.dzfeat = ws + p->dz_upo[L - 1].off;
    h.loss_partial = ws + p->loss_partial_off;
    h.gscale = 2.0f / ((float)p->S * (float)p->B * (float)p->Tout * (float)p->C);
    h.featbf = p->bf16 ? 1 : 0;
    return h;
}


// ---------------------------------------------------------------------------------------
// two-stream helpers
// ---------------------------------------------------------------------------------------
// Flags of the plan's cross-stream events.  They only order kernels of ONE device against each other: the kernel
// packets' own end-of-kernel release / start-of-kernel acquire (agent scope, needed between any two dependent kernels
// on a part whose 8 L2s are not coherent) already make the data visible, so the event itself carries no system-scope
// fence (hipEventDisableSystemFence; host-side consumers synchronise through the caller's stream, never through
// these events).  A/B with pinned tilings: 9.25 -> 9.14 ms per step; the whole GPU suite (bit-exact determinism,
// B=16 vs oracle) passes in both modes.  WUN_EVENT_SCOPE=system|device: fall-back switch.
unsigned event_flags(const wun_plan* p) {
    if (p->sw.event_scope == EV_SYSTEM) return (unsigned)hipEventDisableTiming;
    if (p->sw.event_scope == EV_DEVICE) return (unsigned)(hipEventDisableTiming | hipEventReleaseToDevice);
    return (unsigned)(hipEventDisableTiming | hipEventDisableSystemFence);
}

int side_init(const wun_plan* p) {
    if (p->side != nullptr) return WUN_OK;
    if (p->sw.single_stream) return WUN_OK;      // debugging: everything on one stream
    // The side streams carry the off-critical-path work (weight gradients, deferred skip-window convs): lowest queue
    // priority, so their workgroups fill the drain of the dependent chain on the caller's stream instead of sharing the
    // CUs with it (A/B, pinned tilings: 9.32 -> 9.21 ms per step; "high" 9.39).  WUN_SIDE_PRIO=normal|high: experiment switch.
    // Only with wun_config.exclusive_streams: beside a communication stream (RCCL all-reduce on one GPU, same box) the
    // low-priority queues made the step 13.1 ms instead of 9.2 -- and a process that has ever created them stays slow.
    int least = 0, greatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
    int prio = p->cfg.exclusive_streams ? least : 0;
    if (p->sw.side_prio != PRIO_DEFAULT) prio = p->sw.side_prio == PRIO_LOW ? least : p->sw.side_prio == PRIO_HIGH ? greatest : 0;
    HIP_TRY(hipStreamCreateWithPriority(&p->side, hipStreamNonBlocking, prio));
    HIP_TRY(hipStreamCreateWithPriority(&p->side2, hipStreamNonBlocking, prio));
    p->events.resize(160);
    for (auto& e : p->events) HIP_TRY(hipEventCreateWithFlags(&e, event_flags(p)));
    return WUN_OK;
}
// `to` waits for everything issued so far on `from`
int stream_dep(const wun_plan* p, hipStream_t from, hipStream_t to) {
    if (from == to) return WUN_OK;
    hipEvent_t e = p->events[p->ev_next++ % p->events.size()];
    HIP_TRY(hipEventRecord(e, from));
    HIP_TRY(hipStreamWaitEvent(to, e, 0));
    return WUN_OK;
}


// ---------------------------------------------------------------------------------------
// autotuned dispatch: every conv / wgrad launch of a step has a fixed position in the launch
// order; wun_plan_tune measures candidate (tile variant, split-K) / (geometry, split count)
// choices for each position on the real buffers and caches the fastest.
// ---------------------------------------------------------------------------------------
static float time_launch(const wun_plan* p, hipStream_t s, const std::function<hipError_t()>& fn) {
    if (fn() != hipSuccess) { (void)hipGetLastError(); return 1e30f; }      // warm-up / validity
    float best = 1e30f;
    for (int r = 0; r < 2; ++r) {
        (void)hipEventRecord(p->tev0, s);
        if (fn() != hipSuccess) { (void)hipGetLastError(); return 1e30f; }
        (void)hipEventRecord(p->tev1, s);
        if (hipEventSynchronize(p->tev1) != hipSuccess) return 1e30f;
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, p->tev0, p->tev1);
        if (ms < best) best = ms;
    }
    return best;
}

// One event-bracketed run (no warm-up); 1e30 on failure.
static float time_once(const wun_plan* p, hipStream_t s, const std::function<hipError_t()>& fn) {
    (void)hipEventRecord(p->tev0, s);
    if (fn() != hipSuccess) { (void)hipGetLastError(); return 1e30f; }
    (void)hipEventRecord(p->tev1, s);
    if (hipEventSynchronize(p->tev1) != hipSuccess) return 1e30f;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, p->tev0, p->tev1);
    return ms;
}

// WUN_TUNE_ALTS log: the near-best candidates of one launch position (isolated timing) for the whole-step tuner,
// tools/step_tune.py -- at most WUN_TUNE_ALTS_MAX of them within WUN_TUNE_ALTS_TOL of the best, fastest first, after the
// line `head` (or none); line(f, i) writes candidate i
static void tune_alts(const wun_plan* p, const char* head, const float* tms, size_t n, float best, float base,
                      const std::function<void(FILE*, size_t)>& line) {
    if (p->sw.tune_alts.empty()) return;
    FILE* f = fopen(p->sw.tune_alts.c_str(), "a");
    if (!f) return;
    if (head) fputs(head, f);
    const float lim = std::min(best, base) * p->sw.tune_alts_tol;
    std::vector<size_t> order;
    for (size_t i = 0; i < n; ++i) if (tms[i] <= lim) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return tms[x] < tms[y]; });
    for (size_t k = 0; k < order.size() && k < (size_t)p->sw.tune_alts_max; ++k) line(f, order[k]);
    fclose(f);
}

// Times `n` candidate launches of ONE launch position against each other: every candidate is warmed up once, then
// the candidates are run round-robin for WUN_TUNE_ROUNDS rounds (default 4) and each keeps its fastest run.  The shader
// clock of a busy MI355X drifts by ~10 % over milliseconds (DVFS); timing candidates one after the other in a single
// pass -- the round-1/2 tuner -- lets that drift decide between tiles that differ by a few per cent.  best[i] = 1e30 for
// candidates that failed.
static void time_candidates(const wun_plan* p, hipStream_t s, int n, const std::function<hipError_t(int)>& launch, float* best) {
    const int rounds = p->sw.tune_rounds;
    for (int i = 0; i < n; ++i) {
        best[i] = 1e30f;
        if (launch(i) != hipSuccess) { (void)hipGetLastError(); best[i] = -1.f; }    // warm-up / validity
    }
    for (int r = 0; r < rounds; ++r)
        for (int i = 0; i < n; ++i) {
            if (best[i] < 0.f) continue;
            const float ms = time_once(p, s, [&]() { return launch(i); });
            if (ms < best[i]) best[i] = ms;
        }
    for (int i = 0; i < n; ++i)
        if (best[i] < 0.f) best[i] = 1e30f;
}

// at < 0: the launch takes the next position of the step's launch order; at >= 0: a position reserved earlier
// (deferred launches keep the position they have in the canonical order, so tuned tables stay aligned)
hipError_t conv_dispatch(const wun_plan* p, ConvArgs a, float* part, long long cap, hipStream_t s, long long at) {
    std::vector<ConvChoice>& vec = p->in_bwd ? p->conv_bwd : p->conv_fwd;
    const size_t idx = at >= 0 ? (size_t)at : p->ci++;
    if (p->bf16) {
        // bf16 mode: every tensor this launch touches holds bf16 elements; the bf16 MFMA kernel is the ONLY kernel that can
        // serve it (bf16_plan_ok admitted the plan on that condition) -- weights from the packed image
        if (a.C0 + a.C1 < 8) {
            // the audio-input conv: fp32 audio in, bf16 activations out, direct conv on the vector pipe (wun_bf16.hip)
            a.xbf = 0; a.obf = 1;
            return launch_first_conv(a, s);
        }
        a.xbf = 1; a.obf = 1;
        if (!conv_bf16_supported(a)) return hipErrorInvalidValue;
        const bool in_ws = a.W >= p->cur_ws && a.W < p->cur_ws + p->ws;
        auto it = p->bf_img.find({in_ws ? 1 : 0, (long long)(a.W - (in_ws ? p->cur_ws : p->cur_params))});
        if (it == p->bf_img.end()) return hipErrorInvalidValue;
        {
            a.W = p->cur_ws + it->second.off;
            a.wb_c8p = it->second.c8p; a.wb_npad = it->second.npad;
            // tile (positions x columns x channel chunks per stage) autotuned like the fp32 variants
            if (p->tune_mode == 1) {
                if (vec.size() <= idx) vec.resize(idx + 1, ConvChoice{-1, 0});
                ConvChoice cands[32];
                const int n = conv_bf16_list_candidates(a, cands, 32);
                float best = time_launch(p, s, [&]() { return launch_conv_bf16(a, s, p->sw); });
                const float base = best;
                ConvChoice bc{-1, 0};
                for (int i = 0; i < n; ++i) {
                    ConvArgs b = a;
                    b.force_variant = cands[i].variant + 1;
                    const float ms = time_launch(p, s, [&]() { return launch_conv_bf16(b, s, p->sw); });
                    if (ms < best * 0.98f) { best = ms; bc = cands[i]; }
                }
                vec[idx] = bc;
                if (p->sw.tune_log)
                    fprintf(stderr, "[tune conv-bf16 %s#%zu] C=%d N=%d T=%d K=%d ld=%d ph2=%d cands=%d base %.3f ms -> code=%d %.3f ms\n",
                            p->in_bwd ? "bwd" : "fwd", idx, a.C0 + a.C1, a.N, a.Tout, a.KW, a.loader, (a.flags & F_PHASE2) ? 1 : 0, n,
                            base, bc.variant, best);
            }
            if (p->tune_mode >= 1 && idx < vec.size() && vec[idx].variant >= kBf16VariantBase && conv_bf16_choice_ok(a, vec[idx].variant))
                a.force_variant = vec[idx].variant + 1;
            return launch_conv_bf16(a, s, p->sw);
        }
    }
    if (p->tune_mode == 1) {
        if (vec.size() <= idx) vec.resize(idx + 1, ConvChoice{-1, 0});
        std::vector<ConvChoice> cands_v(640);               // (per call: two plans may be tuned from different threads)
        std::vector<float> tms_v(641);
        ConvChoice* cands = cands_v.data();
        float* tms = tms_v.data();
        const int n = conv_list_candidates(a, part ? cap : 0, cands, 640, p->sw);
        // candidate n = the heuristic choice (the baseline); a candidate has to beat it by > 2 %
        time_candidates(p, s, n + 1, [&](int i) {
            ConvArgs b = a;
            b.ups_y = nullptr; b.ubw_dz = nullptr;   // (candidates are compared without the fused extras only split-K ones write)
            if (i < n) { b.force_variant = cands[i].variant + 1; b.force_ksplit = cands[i].ksplit; }
            return launch_conv(b, part, cap, s, p->sw);
        }, tms);
        const float base = tms[n];
        float best = base;
        ConvChoice bc{-1, 0};
        int bi = -1;
        for (int i = 0; i < n; ++i)
            if (bi < 0 ? tms[i] < 1e29f : tms[i] < tms[bi]) bi = i;
        if (bi >= 0 && tms[bi] < base * 0.98f) { best = tms[bi]; bc = cands[bi]; }
        vec[idx] = bc;
        char head[96];
        snprintf(head, sizeof(head), "%s %zu %d %d %.4f\n", p->in_bwd ? "cb" : "cf", idx, -1, 0, base);
        tune_alts(p, head, tms, (size_t)n, best, base, [&](FILE* f, size_t i) {
            fprintf(f, "%s %zu %d %d %.4f\n", p->in_bwd ? "cb" : "cf", idx, cands[i].variant, cands[i].ksplit, tms[i]);
        });
        if (p->sw.tune_log)
            fprintf(stderr, "[tune conv %s#%zu] C=%d N=%d T=%d K=%d ld=%d ph2=%d cands=%d base %.3f ms -> v=%d ks=%d %.3f ms\n",
                    p->in_bwd ? "bwd" : "fwd", idx, a.C0 + a.C1, a.N, a.Tout, a.KW, a.loader, (a.flags & F_PHASE2) ? 1 : 0, n,
                    base, bc.variant, bc.ksplit, best);
    }
    if (p->tune_mode >= 1 && idx < vec.size() && vec[idx].variant >= 0 &&
        conv_choice_ok(a, part ? cap : 0, vec[idx].variant, vec[idx].ksplit > 0 ? vec[idx].ksplit : 1, p->sw)) {
        // (an entry that is not a legal choice for this launch -- a stale or edited table -- is ignored)
        a.force_variant = vec[idx].variant + 1; a.force_ksplit = vec[idx].ksplit;
    }
    return launch_conv(a, part, cap, s, p->sw);
}

// ---------------------------------------------------------------------------------------
// loss + backward
// ---------------------------------------------------------------------------------------
// All parts of one layer's weight gradient (a down level has two: the decimated and the window
// positions) use ONE tile geometry, so their splits land in one tile-major partial buffer that a
// single reduction sums.  Returns false if the parts do not resolve to the same geometry.
bool wgrad_common_geom(WgradArgs* parts, int nparts, int mtw, int nw) {
    int m0 = 0, n0 = 0;
    for (int i = 0; i < nparts; ++i) {
        parts[i].force_mtw = mtw; parts[i].force_nw = nw;
        int m, n;
        wgrad_resolved_geom(parts[i], m, n);
        if (i == 0) { m0 = m; n0 = n; }
        else if (m != m0 || n != n0) return false;
    }
    return true;
}

int run_wgrad(const wun_plan* p, WgradArgs* parts, int nparts, const ConvLayer& cl, float* ws,
                     float* grads, hipStream_t main, hipStream_t s, bool dep, bool accum) {
    // everything this weight gradient reads (dz, activations) has been issued on `main`
    // (dep == false: the caller already made `s` wait -- one event for a batch of weight gradients)
    if (dep) {
        int rcd = stream_dep(p, main, s);
        if (rcd) return rcd;
    }
    // bf16 speed mode: operands rounded to bf16 in LDS (same tiles, same partial layout); launches with few
    // positions are latency-bound and stay exact fp32
    if (p->bf16) {
        // bf16 mode: inputs and gradients are bf16 tensors, the bf16 kernel is the only reader
        if (!wgrad_bf16_supported(parts[0])) return fail(WUN_ERR_UNSUPPORTED, "bf16 mode: weight-gradient shape not served by the bf16 kernel");
        for (int i = 0; i < nparts; ++i) { parts[i].bf16 = 1; parts[i].sbf = 1; }
    }
    // weight gradients alternate between two side streams; each has its own half of the partial buffer
    const long long pcap = p->partial_floats / 2;
    float* partial = ws + p->partial_off + ((p->side2 && s == p->side2) ? pcap : 0);
    float* out_w = grads + cl.woff;
    float* out_b = out_w + (long long)cl.KW * cl.Cin * cl.Cout;
    const size_t idx = p->wi++;
    // exact fp32: the register-window kernel (wun_wgrad_win.hip) where every part qualifies (15 / 5 taps, channel counts
    // in whole row tiles); its split partials are in the final layout, so the parts need not share a tile geometry
    bool win_ok = !p->sw.no_win && !parts[0].bf16;
    for (int i = 0; i < nparts && win_ok; ++i) { WgradArgs t = parts[i]; t.win = 1; win_ok = wgrad_win_supported(t); }
    auto set_win = [&](WgradArgs* q, int cgw, int nw) {
        for (int i = 0; i < nparts; ++i) { q[i].win = 1; q[i].force_mtw = cgw; q[i].force_nw = nw; }
    };
    if (win_ok) {
        set_win(parts, 0, 0);
    } else {
        // default: the heuristic geometry of the largest part, lowered until every part agrees
        int m, n;
        parts[0].force_mtw = parts[0].force_nw = 0;
        wgrad_resolved_geom(parts[0], m, n);
        while (!wgrad_common_geom(parts, nparts, m, n) && m > 1) m = m == 6 ? 4 : m / 2;   // (bf16: 8 -> 4)
    }
    for (int i = 0; i < nparts; ++i) parts[i].nsplit = wgrad_pick_nsplit(parts[i], p->sw);
    for (int i = 0; i < nparts; ++i) parts[i].accum = accum ? 1 : 0;   // (read by the launchers only: direct epilogue, reduction)

    auto run = [&](WgradArgs* q) -> hipError_t {
        int total = 0;
        for (int i = 0; i < nparts; ++i) total += q[i].nsplit;
        if (total == 1) {
            q[0].out = out_w; q[0].direct = 1; q[0].split_base = 0;
            return launch_wgrad(q[0], s, p->sw);
        }
        // the arena is sized at plan creation for the heuristic split counts with 2x headroom; a policy that asks for
        // more on some shape gets fewer splits, not a failed step
        for (int guard = 0; (long long)total * wgrad_partial_floats(q[0], p->sw) > pcap && total > nparts && guard < 32; ++guard) {
            total = 0;
            for (int i = 0; i < nparts; ++i) { q[i].nsplit = (q[i].nsplit + 1) / 2; total += q[i].nsplit; }
        }
        if ((long long)total * wgrad_partial_floats(q[0], p->sw) > pcap) return hipErrorOutOfMemory;
        if (total == 1) {
            q[0].out = out_w; q[0].direct = 1; q[0].split_base = 0;
            return launch_wgrad(q[0], s, p->sw);
        }
        int done = 0;
        for (int i = 0; i < nparts; ++i) {
            q[i].out = partial; q[i].direct = 0; q[i].split_base = done;
            hipError_t e = launch_wgrad(q[i], s, p->sw);
            if (e != hipSuccess) return e;
            done += q[i].nsplit;
        }
        return launch_wgrad_reduce(q[0], partial, total, out_w, out_b, s, p->sw);
    };

    if (p->tune_mode == 1) {
        if (p->wg_bwd.size() <= idx) p->wg_bwd.resize(idx + 1, WgradChoice{0, 0, {0, 0}});
        // candidates: shared geometry x per-part split counts, timed with the split reduction (round-robin, see
        // time_candidates); candidate 0 = the heuristic choice
        struct Cand { WgradArgs g[2]; WgradChoice c; };
        std::vector<Cand> cv;
        { Cand c0; for (int i = 0; i < nparts; ++i) c0.g[i] = parts[i]; c0.c = WgradChoice{0, 0, {0, 0}}; cv.push_back(c0); }
        static const int mtws[] = {8, 6, 4, 2, 1};         // (8: bf16 kernel only; 6, 2, 1: exact-fp32 kernel only)
        WgradArgs g[2];
        if (win_ok) {
            // register-window kernel: column tiles per wave x split counts (choice code: mtw = 16 + column groups per workgroup)
            const int ntile = (parts[0].N + 15) / 16;
            int bestpad = 1 << 30;
            for (int nw = 2; nw <= 6; ++nw) bestpad = std::min(bestpad, (ntile + nw - 1) / nw * nw);
            for (int nw = (parts[0].KW == 15 ? 3 : 2); nw <= (parts[0].KW == 15 ? 5 : 6); ++nw) {
                if ((ntile + nw - 1) / nw * nw > bestpad + (bestpad >= 8 ? 1 : 0) && nw != 3) continue;
                for (int i = 0; i < nparts; ++i) g[i] = parts[i];
                set_win(g, 1, nw);
                int basens[2] = {0, 0}, units[2] = {0, 0};
                for (int i = 0; i < nparts; ++i) { basens[i] = wgrad_pick_nsplit(g[i], p->sw); units[i] = wgrad_max_units(g[i], p->sw); }
                static const int num[5] = {4, 2, 6, 8, 3};          // split factor / 4: 1, 1/2, 3/2, 2, 3/4
                for (int oi = 0; oi < 5; ++oi) {
                    for (int i = 0; i < nparts; ++i) {
                        int ns = basens[i] * num[oi] / 4;
                        if (ns < 1) ns = 1;
                        if (ns > units[i]) ns = units[i];
                        g[i].nsplit = ns;
                    }
                    Cand c;
                    for (int i = 0; i < nparts; ++i) c.g[i] = g[i];
                    c.c = WgradChoice{17, nw, {g[0].nsplit, nparts > 1 ? g[1].nsplit : 0}};
                    cv.push_back(c);
                }
            }
        }
        for (int mi = 0; mi < 5; ++mi)
            for (int nw = 5; nw >= 1; --nw) {
                if (nw > 3 && (mtws[mi] == 6 || parts[0].N <= 48)) continue;
                for (int i = 0; i < nparts; ++i) { g[i] = parts[i]; g[i].win = 0; }
                if (!wgrad_common_geom(g, nparts, mtws[mi], nw)) continue;
                int m, n;
                wgrad_resolved_geom(g[0], m, n);
                if (m != mtws[mi] || n != nw) continue;          // lowered by the staging limit: duplicate
                int basens[2] = {0, 0}, units[2] = {0, 0};
                for (int i = 0; i < nparts; ++i) { basens[i] = wgrad_pick_nsplit(g[i], p->sw); units[i] = wgrad_max_units(g[i], p->sw); }
                static const int num[4] = {4, 2, 8, 1};            // split factor / 4: 1, 1/2, 2, 1/4
                for (int oi = 0; oi < 4; ++oi) {
                    bool same = oi > 0;
                    for (int i = 0; i < nparts; ++i) {
                        int ns = basens[i] * num[oi] / 4;
                        if (ns < 1) ns = 1;
                        if (ns > units[i]) ns = units[i];
                        if (ns != basens[i]) same = false;
                        g[i].nsplit = ns;
                    }
                    if (same) continue;
                    Cand c;
                    for (int i = 0; i < nparts; ++i) c.g[i] = g[i];
                    c.c = WgradChoice{mtws[mi], nw, {g[0].nsplit, nparts > 1 ? g[1].nsplit : 0}};
                    cv.push_back(c);
                }
            }
        std::vector<float> tms(cv.size());
        time_candidates(p, s, (int)cv.size(), [&](int i) { return run(cv[(size_t)i].g); }, tms.data());
        const float base = tms[0];
        float best = base;
        WgradChoice bc{0, 0, {0, 0}};
        size_t bi = 0;
        for (size_t i = 1; i < cv.size(); ++i)
            if (tms[i] < tms[bi]) bi = i;
        if (bi > 0 && tms[bi] < base * 0.98f) { best = tms[bi]; bc = cv[bi].c; }
        tune_alts(p, nullptr, tms.data(), cv.size(), best, base, [&](FILE* f, size_t i) {
            const WgradChoice& c = cv[i].c;
            fprintf(f, "wg %zu %d %d %d %d %.4f\n", idx, c.mtw, c.nw, c.nsplit[0], c.nsplit[1], tms[i]);
        });
        p->wg_bwd[idx] = bc;
        if (p->sw.tune_log)
            fprintf(stderr, "[tune wgrad #%zu] C=%d N=%d T=%d K=%d ld=%d parts=%d base(ns=%d) %.3f ms -> mtw=%d nw=%d ns=%d,%d %.3f ms\n",
                    idx, parts[0].C0 + parts[0].C1, parts[0].N, parts[0].Tq, parts[0].KW, parts[0].loader, nparts,
                    parts[0].nsplit, base, bc.mtw, bc.nw, bc.nsplit[0], bc.nsplit[1], best);
    }
    if (p->tune_mode >= 1 && idx < p->wg_bwd.size() && p->wg_bwd[idx].nsplit[0] > 0) {
        const WgradChoice& c = p->wg_bwd[idx];
        const bool cwin = c.mtw == 17;
        bool ok = cwin ? (win_ok && c.nw >= 1 && c.nw <= 6)
                       : ((c.mtw == 1 || c.mtw == 2 || c.mtw == 4 || c.mtw == 6 || c.mtw == 8) && c.nw >= 1 && c.nw <= 5);
        for (int i = 0; ok && i < nparts; ++i) ok = c.nsplit[i] >= 1;
        WgradArgs g[2];
        for (int i = 0; i < nparts; ++i) { g[i] = parts[i]; g[i].win = 0; }
        if (ok && cwin) {
            set_win(g, 1, c.nw);
            for (int i = 0; ok && i < nparts; ++i) ok = c.nsplit[i] <= wgrad_max_units(g[i], p->sw);
            if (ok)
                for (int i = 0; i < nparts; ++i) { parts[i] = g[i]; parts[i].nsplit = c.nsplit[i]; }
        } else if (ok && wgrad_common_geom(g, nparts, c.mtw, c.nw)) {
            for (int i = 0; ok && i < nparts; ++i) ok = c.nsplit[i] <= wgrad_max_units(g[i], p->sw);
            if (ok)
                for (int i = 0; i < nparts; ++i) { parts[i] = g[i]; parts[i].nsplit = c.nsplit[i]; }
        }
    }
    hipError_t e = run(parts);
    if (e == hipErrorOutOfMemory) return fail(WUN_ERR_INVALID, "internal: wgrad partial buffer too small");
    HIP_TRY(e);
    return WUN_OK;
}

// Narrow layers (audio-input conv, output head): direct reduction kernel instead of MFMA tiles.  All parts
// (a down level's decimated + window positions) write consecutive splits of one partial list; one reduction.
int run_narrow_wgrad(const wun_plan* p, NarrowWgradArgs* parts, int nparts, const long long* woff,
                            const long long* boff, float* ws, float* grads, hipStream_t main, hipStream_t s, bool accum) {
    int rcd = WUN_OK;
    hipStream_t side_of_caller = s;                            // (bucket events of the data-parallel path are recorded there)
    // bf16 mode, history (round 5): built WITH packed fp32 VALU instructions, narrow_wgrad_kernel (the LDS-staged
    // form: the output head, audio-input convs with < 4 taps) returned different accumulators from run to run whenever bf16 MFMA
    // kernels ran beside it; round 5 built the unit without them AND, as a second line, ran this launch alone on the caller's
    // stream.  Round 6: tools/probes/pk_fma_probe.hip reproduces the defect stand-alone (the compiler's packed instruction mix beside a
    // v_mfma_f32_16x16x32_bf16 spinner: 2085 of 10000 launches differ; alone, beside an fp32-MFMA spinner, or built without
    // packed ops: 0), the library with packed ops + overlap differs in 60 of 60 probe steps, the shipped build with overlap in
    // 0 of 600 -- so the launch is back on the side stream (~1 % of the bf16 step).  WUN_BF16_HEAD_SERIAL=1: round 5's placement.
    if (p->bf16 && s != main && p->sw.bf16_head_serial) {
        bool lds_form = false;
        for (int i = 0; i < nparts; ++i) lds_form = lds_form || narrow_wgrad_uses_lds(parts[i], p->sw);
        if (lds_form) {
            if (p->side != nullptr && (rcd = stream_dep(p, p->side, main))) return rcd;
            if (p->side2 != nullptr && (rcd = stream_dep(p, p->side2, main))) return rcd;
            s = main;
        }
    }
    if (s != main && (rcd = stream_dep(p, main, s))) return rcd;      // everything this launch reads has been issued on `main`
    const long long pcap = p->partial_floats / 2;
    float* partial = ws + p->partial_off + ((p->side2 && s == p->side2) ? pcap : 0);
    int total = 0;
    for (int i = 0; i < nparts; ++i) { parts[i].nsplit = narrow_wgrad_pick_nsplit(parts[i], p->sw); total += parts[i].nsplit; }
    const long long P = narrow_wgrad_partial_floats(parts[0]);
    while (total * P > pcap && total > nparts) {               // (never in practice: P is a few hundred floats)
        total = 0;
        for (int i = 0; i < nparts; ++i) { parts[i].nsplit = (parts[i].nsplit + 1) / 2; total += parts[i].nsplit; }
    }
    int done = 0;
    for (int i = 0; i < nparts; ++i) {
        parts[i].partial = partial; parts[i].split_base = done;
        HIP_TRY(launch_narrow_wgrad(parts[i], s, p->sw));
        done += parts[i].nsplit;
    }
    HIP_TRY(launch_narrow_wgrad_reduce(parts[0], partial, total, grads, woff, boff, s, accum));
    // (moved to `main`: the side stream the caller named is where it records "gradients complete" -- it follows)
    if (s != side_of_caller && (rcd = stream_dep(p, s, side_of_caller))) return rcd;
    return WUN_OK;
}

