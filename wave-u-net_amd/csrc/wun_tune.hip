// Host side of libwun.so: the autotuner (one measuring step) and the tuning-table format.
#include "wun_plan_impl.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" int wun_plan_tune(const wun_plan* p, const float* params, const float* mix_btc, float* ws,
                             float* outputs, const float* targets, float* grads, float* loss, void* stream) {
    if (!p) return fail(WUN_ERR_INVALID, "null argument");
    if (!p->tev0) {
        HIP_TRY(hipEventCreate(&p->tev0));
        HIP_TRY(hipEventCreate(&p->tev1));
    }
    p->conv_fwd.clear(); p->conv_bwd.clear(); p->wg_bwd.clear();
    p->tune_mode = 1;
    int rc = wun_forward(p, params, mix_btc, ws, outputs, 1, stream);
    if (rc == WUN_OK) rc = wun_loss_backward(p, params, mix_btc, ws, outputs, targets, grads, loss, stream);
    const hipError_t sync = hipStreamSynchronize((hipStream_t)stream);
    p->tune_mode = (rc == WUN_OK && sync == hipSuccess) ? 2 : 0;     // never left in measuring mode
    if (rc == WUN_OK && sync != hipSuccess)
        return fail(WUN_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(sync));
    return rc;
}

// Tuning-table header: identifies the plan (every config key that changes a launch), the launch
// order of this library build and the number of entries per section, so a table written for
// another plan, another library build or truncated on disk is rejected at import.
#define WUN_TUNE_ORDER "r6a"      /* bump whenever the order / number of conv or wgrad launches changes */
#define WUN_TUNE_ORDER_BF16 "r5b" /* ... of the bf16 mode (round 5: bf16 activations in HBM, other tile menu limits) */
static std::string tune_header(const wun_plan* p, size_t ncf, size_t ncb, size_t nwg) {
    char line[320];
    const wun_config& c = p->cfg;
    snprintf(line, sizeof(line),
             "wun-tune 2 order=%s variants=%d B=%d Tin=%lld L=%d F=%d K=%d,%d,%d ups=%d out=%d ctx=%d S=%d C=%d act=%d "
             "dt=%d arena=%lld cf=%zu cb=%zu wg=%zu",
             p->bf16 ? WUN_TUNE_ORDER_BF16 : WUN_TUNE_ORDER, conv_num_variants(), p->B, (long long)p->Tin, p->L, c.num_initial_filters, c.filter_size,
             c.merge_filter_size, c.output_filter_size, c.upsampling, c.output_type, c.context, c.num_sources,
             c.num_channels, c.output_activation, c.compute_dtype, (long long)p->arena, ncf, ncb, nwg);
    std::string h = line;
    // a non-default early-window mode changes the order of the backward conv launches: such tables only match themselves
    if (p->early_window != (p->dedup ? EW_ALL : EW_DEEP))
        h += p->early_window == EW_OFF ? " ew=0" : p->early_window == EW_ALL ? " ew=all" : " ew=deep";
    if (p->sw.odd_fuse_set) h += " oddfuse=" + std::to_string(p->sw.odd_fuse_min);
    if (p->sw.no_odd_align && p->dedup) h += " oddalign=0";
    if (!p->same && !p->bf16 && !p->dedup) h += " dedup=0";       // (WUN_NO_DEDUP=1: rounds 1 - 5's launch sequence)
    return h;
}

extern "C" int wun_plan_tune_export(const wun_plan* p, char* buf, int64_t cap) {
    if (!p || !buf) return fail(WUN_ERR_INVALID, "null argument");
    if (p->tune_mode != 2) return fail(WUN_ERR_INVALID, "plan has not been tuned");
    std::string out = tune_header(p, p->conv_fwd.size(), p->conv_bwd.size(), p->wg_bwd.size()) + "\n";
    char line[128];
    auto dump = [&](const char* tag, const std::vector<ConvChoice>& v) {
        for (const ConvChoice& c : v) { snprintf(line, sizeof(line), "%s %d %d\n", tag, c.variant, c.ksplit); out += line; }
    };
    dump("cf", p->conv_fwd);
    dump("cb", p->conv_bwd);
    for (const WgradChoice& c : p->wg_bwd) {
        snprintf(line, sizeof(line), "wg %d %d %d %d\n", c.mtw, c.nw, c.nsplit[0], c.nsplit[1]);
        out += line;
    }
    out += "end\n";
    if ((int64_t)out.size() + 1 > cap) return fail(WUN_ERR_INVALID, "buffer too small for the tuning table");
    memcpy(buf, out.c_str(), out.size() + 1);
    return WUN_OK;
}

extern "C" int wun_plan_tune_import(const wun_plan* p, const char* text) {
    if (!p || !text) return fail(WUN_ERR_INVALID, "null argument");
    const char* nl = strchr(text, '\n');
    if (!nl) return fail(WUN_ERR_INVALID, "malformed tuning table");
    const std::string head(text, (size_t)(nl - text));
    size_t ncf = 0, ncb = 0, nwg = 0;
    {
        const size_t pos = head.rfind(" cf=");
        if (pos == std::string::npos || sscanf(head.c_str() + pos, " cf=%zu cb=%zu wg=%zu", &ncf, &ncb, &nwg) != 3)
            return fail(WUN_ERR_INVALID, "tuning table belongs to a different plan or library build");
    }
    if (head != tune_header(p, ncf, ncb, nwg))
        return fail(WUN_ERR_INVALID, "tuning table belongs to a different plan or library build");
    std::vector<ConvChoice> cf, cb;
    std::vector<WgradChoice> wg;
    const char* q = nl + 1;
    bool ended = false;
    const int nvar = conv_num_variants();
    while (*q) {
        int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        if (strncmp(q, "end", 3) == 0) { ended = true; break; }
        if (sscanf(q, "cf %d %d", &a0, &a1) == 2 && q[1] == 'f') cf.push_back(ConvChoice{a0, a1});
        else if (sscanf(q, "cb %d %d", &a0, &a1) == 2 && q[1] == 'b') cb.push_back(ConvChoice{a0, a1});
        else if (sscanf(q, "wg %d %d %d %d", &a0, &a1, &a2, &a3) == 4) wg.push_back(WgradChoice{a0, a1, {a2, a3}});
        else return fail(WUN_ERR_INVALID, "malformed tuning table");
        const char* e = strchr(q, '\n');
        if (!e) break;
        q = e + 1;
    }
    if (!ended || cf.size() != ncf || cb.size() != ncb || wg.size() != nwg)
        return fail(WUN_ERR_INVALID, "truncated tuning table");
    for (const std::vector<ConvChoice>* v : {&cf, &cb})
        for (const ConvChoice& c : *v)
            if (c.variant < -1 || (c.variant >= nvar && !(c.variant >= kBf16VariantBase && c.variant < kBf16VariantBase + 27)) ||
                c.ksplit < 0 || c.ksplit > 64)
                return fail(WUN_ERR_INVALID, "tuning table entry out of range");
    for (const WgradChoice& c : wg)
        if (c.nsplit[0] < 0 || c.nsplit[1] < 0 || c.mtw < 0 || (c.mtw > 8 && c.mtw != 17) || c.nw < 0 || c.nw > 6)
            return fail(WUN_ERR_INVALID, "tuning table entry out of range");
    // (whether each entry is a legal choice for the launch at its position is checked when it is used)
    p->conv_fwd = cf; p->conv_bwd = cb; p->wg_bwd = wg;
    p->tune_mode = 2;
    return WUN_OK;
}

