// Host side of libwun.so: the optimizer of the training step -- the global gradient norm, and one step function behind every
// entry that steps weights: TF-Adam over the whole arena or a selection of its tensors (wun_adam_step, _select), clipped by the
// global norm and skipping (wun_adam_step_clip), and extended by decoupled weight decay and an EMA of the weights
// (wun_optim_step); wun_ema_update is the EMA line alone.
#include "wun_plan_impl.h"

#include <cmath>
#include <cstring>

// TF-Adam's step size (Training.py:77): lr * sqrt(1 - b2^t) / (1 - b1^t)
float wun::adam_lr_t(int64_t step, float lr, float beta1, float beta2) {
    const double lr_t = (double)lr * std::sqrt(1.0 - std::pow((double)beta2, (double)step)) /
                        (1.0 - std::pow((double)beta1, (double)step));
    return (float)lr_t;
}

// what every Adam entry checks first
static int adam_args(const wun_plan* p, const float* params, const float* grads, const float* m, const float* v, int64_t step) {
    if (!p || !params || !grads || !m || !v) return fail(WUN_ERR_INVALID, "null argument");
    if (step < 1) return fail(WUN_ERR_INVALID, "step is 1-based");
    return WUN_OK;
}

// ---------------------------------------------------------------------------------------
// global gradient norm (tf.clip_by_global_norm's)
// ---------------------------------------------------------------------------------------
// norm workspace: [0, nt) per-tensor norms, [nt] the global norm, float64 chunk partials from the next even float on
static long long norm_partial_off(const wun_plan* p) { return ((long long)p->tensors.size() + 2) & ~1LL; }

extern "C" int64_t wun_grad_norm_workspace_floats(const wun_plan* p) {
    if (!p) return fail(WUN_ERR_INVALID, "null plan");
    return norm_partial_off(p) + 2 * (long long)p->norm_chunks.size();
}

// host-side checks of the norm's arguments (no GPU work): the selection as a bit set and its float count
struct NormWhat { NormSelect sel; long long nfloats; };
static int norm_args(const wun_plan* p, const float* grads, const float* norm_ws, const uint8_t* select, int64_t nselect,
                     NormWhat& w) {
    if (!grads || !norm_ws) return fail(WUN_ERR_INVALID, "null argument");
    if (reinterpret_cast<uintptr_t>(norm_ws) & 7) return fail(WUN_ERR_INVALID, "norm_ws must be 8-byte aligned");
    int rc;
    if ((rc = check_nselect(p, select, nselect))) return rc;
    const int64_t nt = (int64_t)p->tensors.size();
    if (nt > WUN_NORM_MAX_TENSORS) return fail(WUN_ERR_UNSUPPORTED, "wun_grad_norm: more than 256 tensors");
    memset(&w.sel, 0, sizeof(w.sel));
    w.nfloats = 0;
    for (int64_t k = 0; k < nt; ++k) {
        if (select && !select[k]) continue;
        w.sel.bits[k >> 5] |= 1u << (k & 31);
        for (int c = p->norm_first[(size_t)k]; c < p->norm_first[(size_t)k + 1]; ++c) w.nfloats += p->norm_chunks[(size_t)c].len;
    }
    return WUN_OK;
}

static int grad_norm_launch(const wun_plan* p, const float* grads, float grad_scale, float* norm_ws, const NormWhat& w,
                            hipStream_t s) {
    if (!p->dev_norm_chunks) return fail(WUN_ERR_HIP, "plan was created without a usable HIP device");
    HIP_TRY(launch_grad_norm(grads, p->dev_norm_chunks, p->dev_norm_first, (int)p->norm_chunks.size(), (int)p->tensors.size(),
                             w.sel, w.nfloats, grad_scale, norm_ws, reinterpret_cast<double*>(norm_ws + norm_partial_off(p)), s));
    return WUN_OK;
}

extern "C" int wun_grad_norm(const wun_plan* p, const float* grads, float grad_scale, float* norm_ws, void* stream,
                             const uint8_t* select, int64_t nselect) {
    if (!p) return fail(WUN_ERR_INVALID, "null plan");
    NormWhat w;
    int rc;
    if ((rc = norm_args(p, grads, norm_ws, select, nselect, w))) return rc;
    return grad_norm_launch(p, grads, grad_scale, norm_ws, w, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------
// the step: TF-Adam, clipped by the global norm, with decoupled weight decay (AdamW) and an EMA of the weights, in one kernel
// ---------------------------------------------------------------------------------------
extern "C" int64_t wun_optim_abi_size(void) { return (int64_t)sizeof(wun_optim_config); }

// The selected tensors' floats as runs of consecutive arena floats with a per-run decay bit, handed to
// launch(const AdamRanges&, unsigned decay_bits, bool first) -> int in batches of at most WUN_ADAM_RANGES runs; first: the walk's
// first batch.  Adjacent tensors merge into a run when they agree on the bit.  select NULL = every tensor: add_tensor packs the
// tensors end to end, so with no decay the whole arena is one run of exactly p->arena floats, and no float outside it is visited.
template <class Launch>
static int for_each_optim_batch(const wun_plan* p, const uint8_t* select, const uint8_t* decay, bool decay_all, Launch launch) {
    AdamRanges r;
    memset(&r, 0, sizeof(r));
    unsigned bits = 0;
    bool first = true;
    int rc;
    for (size_t k = 0; k < p->tensors.size(); ++k) {
        if (select && !select[k]) continue;
        const wun_tensor_info& t = p->tensors[k];
        const bool dk = decay_all || (decay && decay[k]);
        long long n = 1;
        for (int d = 0; d < t.ndim; ++d) n *= t.shape[d];
        if (r.n > 0 && r.off[r.n - 1] + (r.cum[r.n] - r.cum[r.n - 1]) == t.offset && (((bits >> (r.n - 1)) & 1u) != 0) == dk) {
            r.cum[r.n] += n;
            continue;
        }
        if (r.n == WUN_ADAM_RANGES) {
            if ((rc = launch(r, bits, first))) return rc;
            first = false;
            memset(&r, 0, sizeof(r));
            bits = 0;
        }
        r.off[r.n] = t.offset; r.cum[r.n + 1] = r.cum[r.n] + n;
        if (dk) bits |= 1u << r.n;
        ++r.n;
    }
    return r.n > 0 ? launch(r, bits, first) : WUN_OK;
}

// 1 - d_t of the EMA, formed in float64 and rounded once: d_t = decay, or min(decay, (1 + step) / (10 + step)) with warm-up
static float ema_weight(float ema_decay, int64_t step, bool warmup) {
    double d = (double)ema_decay;
    if (warmup) d = std::min(d, (1.0 + (double)step) / (10.0 + (double)step));
    return (float)(1.0 - d);
}

// What every stepping entry does once its arguments are checked.  norm (from norm_args) non-null: the global norm is launched
// into norm_ws first and the kernel clips and skips by it; null: no norm, no clip prologue.  ema NULL: no EMA; c.weight_decay 0:
// no decay.  Whether the norm is wanted is the entry's decision (wun_adam_step_clip always wants it: norm_ws is its output).
static int optim_step(const wun_plan* p, float* params, const float* grads, float* m, float* v, float* ema, int64_t step, float lr,
                      float grad_scale, const wun_optim_config& c, const NormWhat* norm, float* norm_ws, int64_t* skipped,
                      hipStream_t s, const uint8_t* select, const uint8_t* decay_select) {
    int rc;
    if (norm && (rc = grad_norm_launch(p, grads, grad_scale, norm_ws, *norm, s))) return rc;
    OptimArgs a;
    memset(&a, 0, sizeof(a));
    a.p = params; a.g = grads; a.m = m; a.v = v; a.ema = ema;
    a.lr_t = adam_lr_t(step, lr, c.beta1, c.beta2);
    a.b1 = c.beta1; a.b2 = c.beta2; a.eps = c.eps; a.gscale = grad_scale;
    a.wdf = (float)(1.0 - (double)lr * (double)c.weight_decay);
    a.emaw = ema ? ema_weight(c.ema_decay, step, (c.flags & WUN_OPTIM_EMA_WARMUP) != 0) : 0.f;
    a.gnorm = norm ? norm_ws + p->tensors.size() : nullptr;
    a.clip = c.clip_norm; a.skip = (c.flags & WUN_CLIP_SKIP_NONFINITE) ? 1 : 0;
    a.vec = same_alignment({params, grads, m, v, ema}) ? 1 : 0;
    const bool decaying = c.weight_decay > 0.f;
    long long* cnt = a.skip ? reinterpret_cast<long long*>(skipped) : nullptr;
    return for_each_optim_batch(p, select, decaying ? decay_select : nullptr, decaying && !decay_select,
                                [&](const AdamRanges& r, unsigned bits, bool first) -> int {
        OptimArgs b = a;
        b.decay = bits;
        b.skipped = first ? cnt : nullptr;            // every launch of a skipped step returns at once; the first counts it
        HIP_TRY(launch_optim_ranges(b, r, s));
        return WUN_OK;
    });
}

extern "C" int wun_adam_step(const wun_plan* p, float* params, const float* grads, float* m, float* v,
                             int64_t step, float lr, float beta1, float beta2, float eps, float grad_scale,
                             void* stream) {
    return wun_adam_step_select(p, params, grads, m, v, step, lr, beta1, beta2, eps, grad_scale, stream, nullptr, 0);
}

extern "C" int wun_adam_step_select(const wun_plan* p, float* params, const float* grads, float* m, float* v,
                                    int64_t step, float lr, float beta1, float beta2, float eps, float grad_scale,
                                    void* stream, const uint8_t* select, int64_t nselect) {
    int rc;
    if ((rc = adam_args(p, params, grads, m, v, step))) return rc;
    if ((rc = check_nselect(p, select, nselect))) return rc;
    const wun_optim_config c = {beta1, beta2, eps, 0.f, 0.f, INFINITY, 0};
    return optim_step(p, params, grads, m, v, nullptr, step, lr, grad_scale, c, nullptr, nullptr, nullptr, (hipStream_t)stream,
                      select, nullptr);
}

extern "C" int wun_adam_step_clip(const wun_plan* p, float* params, const float* grads, float* m, float* v,
                                  int64_t step, float lr, float beta1, float beta2, float eps, float grad_scale,
                                  float clip_norm, int32_t flags, float* norm_ws, int64_t* skipped,
                                  void* stream, const uint8_t* select, int64_t nselect) {
    int rc;
    if ((rc = adam_args(p, params, grads, m, v, step))) return rc;
    if (!(clip_norm > 0.f)) return fail(WUN_ERR_INVALID, "clip_norm must be > 0 (+INFINITY = no clipping)");
    if (flags & ~WUN_CLIP_SKIP_NONFINITE) return fail(WUN_ERR_INVALID, "unknown flags");
    if ((flags & WUN_CLIP_SKIP_NONFINITE) && !skipped) return fail(WUN_ERR_INVALID, "skipped is required with WUN_CLIP_SKIP_NONFINITE");
    NormWhat w;
    if ((rc = norm_args(p, grads, norm_ws, select, nselect, w))) return rc;
    // the norm always: norm_ws is this entry's output, also when nothing clips and nothing skips
    const wun_optim_config c = {beta1, beta2, eps, 0.f, 0.f, clip_norm, flags};
    return optim_step(p, params, grads, m, v, nullptr, step, lr, grad_scale, c, &w, norm_ws, skipped, (hipStream_t)stream, select,
                      nullptr);
}

extern "C" int wun_optim_step(const wun_plan* p, float* params, const float* grads, float* m, float* v, float* ema,
                              int64_t step, float lr, float grad_scale, const wun_optim_config* cfg, float* norm_ws,
                              int64_t* skipped, void* stream, const uint8_t* select, int64_t nselect,
                              const uint8_t* decay_select, int64_t ndecay) {
    int rc;
    if ((rc = adam_args(p, params, grads, m, v, step))) return rc;
    if (!cfg) return fail(WUN_ERR_INVALID, "null argument");
    if (!(cfg->weight_decay >= 0.f)) return fail(WUN_ERR_INVALID, "weight_decay must be >= 0");
    if (ema && !(cfg->ema_decay >= 0.f && cfg->ema_decay < 1.f)) return fail(WUN_ERR_INVALID, "ema_decay must be in [0, 1)");
    if (!(cfg->clip_norm > 0.f)) return fail(WUN_ERR_INVALID, "clip_norm must be > 0 (+INFINITY = no clipping)");
    if (cfg->flags & ~(WUN_CLIP_SKIP_NONFINITE | WUN_OPTIM_EMA_WARMUP)) return fail(WUN_ERR_INVALID, "unknown flags");
    const bool skip = (cfg->flags & WUN_CLIP_SKIP_NONFINITE) != 0;
    if (skip && !skipped) return fail(WUN_ERR_INVALID, "skipped is required with WUN_CLIP_SKIP_NONFINITE");
    if ((rc = check_nselect(p, select, nselect))) return rc;
    if ((rc = check_nselect(p, decay_select, ndecay))) return rc;
    // the norm is needed to clip or to decide a skip: with neither it is not launched and norm_ws may be NULL
    const bool need_norm = skip || !std::isinf(cfg->clip_norm);
    NormWhat w;
    if (need_norm && (rc = norm_args(p, grads, norm_ws, select, nselect, w))) return rc;
    return optim_step(p, params, grads, m, v, ema, step, lr, grad_scale, *cfg, need_norm ? &w : nullptr, norm_ws, skipped,
                      (hipStream_t)stream, select, decay_select);
}

extern "C" int wun_ema_update(const wun_plan* p, float* ema, const float* params, float ema_decay, int64_t step, int32_t flags,
                              void* stream, const uint8_t* select, int64_t nselect) {
    if (!p || !ema || !params) return fail(WUN_ERR_INVALID, "null argument");
    if (!(ema_decay >= 0.f && ema_decay < 1.f)) return fail(WUN_ERR_INVALID, "ema_decay must be in [0, 1)");
    if (step < 0) return fail(WUN_ERR_INVALID, "step must be >= 0");
    if (flags & ~WUN_OPTIM_EMA_WARMUP) return fail(WUN_ERR_INVALID, "unknown flags");
    int rc;
    if ((rc = check_nselect(p, select, nselect))) return rc;
    const float w = ema_weight(ema_decay, step, (flags & WUN_OPTIM_EMA_WARMUP) != 0);
    const int vec = same_alignment({ema, params}) ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    return for_each_optim_batch(p, select, nullptr, false, [&](const AdamRanges& r, unsigned, bool) -> int {
        HIP_TRY(launch_ema_ranges(ema, params, w, vec, r, s));
        return WUN_OK;
    });
}
