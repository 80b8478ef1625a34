/*
 * wun.h -- C ABI of the MI355X-native Wave-U-Net hot path (libwun.so).
 *
 * Drop-in boundary for the reference's separator "plugin" surface
 *   UnetAudioSeparator(model_config)                 /root/reference/Models/UnetAudioSeparator.py:15-32
 *   .get_padding(shape)                              /root/reference/Models/UnetAudioSeparator.py:34-83
 *   .get_output(input, training, ...)                /root/reference/Models/UnetAudioSeparator.py:85-144
 * and for one `sess.run([separator_solver, ...])` of the training loop
 *   loss + tf.gradients + AdamOptimizer.minimize     /root/reference/Training.py:50-63,70-77,103-109
 *
 * Plain C types only.  All device buffers are owned by the CALLER (torch / hipMalloc);
 * the library owns only an opaque, immutable plan (shape tables + a small device-side
 * descriptor table).  Every call is asynchronous with respect to the hipStream_t passed
 * (as void*), re-entrant across plans, and returns 0 or a negative wun_status; the
 * message is available from wun_last_error() (thread-local).  Nothing aborts.
 *
 * Threading: one host thread drives a plan at a time (the reference is a single-threaded
 * sess.run loop); different plans may be driven from different threads.  A plan also owns
 * its side HIP streams / events, its split-reduction bookkeeping and -- after wun_plan_tune --
 * the tuned launch table, so the plan is immutable in its SHAPES, not in that scheduling
 * state.  wun_profile_begin/end and the wun_op_* entry points (single-operator tests and
 * benchmarks) use process-global state and are not meant for concurrent use.
 *
 * Streams: the side streams (weight gradients, deferred skip-window convs: work that fills the gaps of the
 * dependent chain on the caller's stream) are created at NORMAL queue priority, and at the LOWEST priority only
 * when wun_config.exclusive_streams = 1 (nothing else shares the device; see the field's comment for the hazard).
 * The plan's internal cross-stream events carry no system-scope fence: they order kernels of this device only.
 * Everything a call enqueues is complete with respect to the caller's stream when the call's work on that stream
 * is (the last internal operation of every call is the caller's stream waiting for the side streams); host code
 * synchronises through that stream, never through the plan's events.
 *
 * Concurrency caveat (measured on MI355X, tools/probes/pk_fma_probe.hip): a packed fp32 FMA whose low lane
 * reads the high half of a register pair (v_pk_fma_f32 ... op_sel:[0,1,0], which the compiler emits freely) returns wrong
 * results while ANOTHER kernel's v_mfma_f32_16x16x32_bf16 waves share the CU.  Every kernel of the bf16 mode, and every kernel
 * both modes share, is built without packed fp32 instructions; the exact-fp32 MFMA kernels keep them (0.5 % per step) because
 * inside one plan they only ever run beside fp32 MFMA kernels.  Do not RUN an exact-fp32 plan concurrently (other stream /
 * thread, same device) with a bf16-mode plan or with other bf16-MFMA work (e.g. a bf16 GEMM); back to back is fine.
 * `make -C wave-u-net_amd/csrc nopkall` builds a library without any packed fp32 instruction for callers who must.
 *
 * Tensor layouts at the boundary are the reference's: audio is float32 [B, T, C]
 * (channel-last, exactly what get_output receives/returns); kernels are TF layout
 * [K, Cin, Cout]; variables sit in a flat float32 arena in TF creation order
 * (conv1d, conv1d_1, ... and interp_<i>), each tensor at the offset the plan reports.
 */
#ifndef WUN_H
#define WUN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum wun_status {
    WUN_OK = 0,
    WUN_ERR_INVALID = -1,      /* bad argument / impossible shape (reference: assert)        */
    WUN_ERR_UNSUPPORTED = -2,  /* reference: NotImplementedError                             */
    WUN_ERR_HIP = -3,          /* a HIP runtime call failed                                   */
    WUN_ERR_NOMEM = -4
} wun_status;

/* The model_config keys UnetAudioSeparator.__init__ reads (UnetAudioSeparator.py:20-32). */
typedef struct wun_config {
    int32_t num_layers;
    int32_t num_initial_filters;
    int32_t filter_size;        /* 1..15 (the register-staged loaders hold at most 15 taps;       */
    int32_t merge_filter_size;  /*  larger sizes return WUN_ERR_UNSUPPORTED at plan creation)     */
    int32_t input_filter_size;  /* used by get_padding only (UnetAudioSeparator.py:73); the graph */
                                /* convolves layer 0 with filter_size (UnetAudioSeparator.py:98)   */
    int32_t output_filter_size;
    int32_t upsampling;         /* 0 = "linear", 1 = "learned"                                */
    int32_t output_type;        /* 0 = "direct", 1 = "difference"                             */
    int32_t context;            /* 0 = same padding, 1 = valid convolutions with context      */
    int32_t num_sources;        /* len(source_names)                                          */
    int32_t num_channels;       /* 1 if mono_downmix else 2                                   */
    int32_t output_activation;  /* 0 = "tanh", 1 = "linear"                                   */
    int32_t compute_dtype;      /* 0 = exact fp32 (v_mfma_f32_16x16x4_f32; the reference's arithmetic),                   */
                                /* 1 = bf16 mode: every activation and activation-gradient tensor lives in HBM as bf16   */
                                /*     (rounded once, by the epilogue that writes it), convs / input gradients / weight  */
                                /*     gradients on v_mfma_f32_16x16x32_bf16 with fp32 accumulate; parameters, weight    */
                                /*     gradients, Adam state, the audio and the head's d(pre-activation) stay fp32.      */
                                /*     Needs num_initial_filters % 8 == 0 (else the plan is the exact-fp32 plan:        */
                                /*     wun_plan_info.compute_dtype_effective says which one was built).                  */
                                /*     Not recommended with upsampling = 1 (learned): the gradient of an interpolation    */
                                /*     weight is a sum of DIFFERENCES of adjacent activations that are already rounded   */
                                /*     to bf16 (cancellation amplifies the storage rounding: up to 0.5 of max|g| on the  */
                                /*     312-element interp_0 of M5 against the un-rounded oracle, tests/test_gpu_bf16.py). */
    int32_t exclusive_streams;  /* scheduling hint, no effect on results.  1 = nothing else runs on this device  */
                                /* beside the plan's calls: its side streams get the LOWEST queue priority (they  */
                                /* fill the gaps of the dependent chain on the caller's stream, ~1 % per step).   */
                                /* 0 (default) = normal priority -- REQUIRED when collectives (RCCL) or other     */
                                /* streams share the device: low-priority queues beside a communication stream    */
                                /* were measured 40 % slower (and a process that ever created them stays slow).   */
} wun_config;

typedef struct wun_plan wun_plan;

typedef struct wun_plan_info {
    int64_t batch;
    int64_t input_frames;       /* Tin                                                       */
    int64_t output_frames;      /* Tout                                                      */
    int64_t num_params;         /* trainable scalars (sum of tensor sizes, no padding)       */
    int64_t arena_floats;       /* size of the param / grad / m / v arenas (with padding)    */
    int64_t workspace_floats;   /* activation + gradient + scratch workspace                 */
    int64_t num_tensors;        /* number of TF variables                                    */
    int64_t num_outputs;        /* == num_sources                                            */
    double  fwd_flops;          /* algorithmic conv FLOPs / step as executed (dead work skipped) */
    double  bwd_flops;
    double  fwd_flops_dense;    /* the reference graph's FLOPs (no dead-work skipping)       */
    double  fwd_flops_unique;   /* every OBSERVED conv output computed once.  == fwd_flops for same-padding plans and for  */
    double  bwd_flops_unique;   /* context plans of the exact-fp32 mode (round 6); the bf16 mode's context plans still run */
                                /* a full-rate conv over each skip window, i.e. compute its even positions twice           */
    int64_t compute_dtype_effective; /* the arithmetic the plan really runs: 0 = exact fp32, 1 = bf16 mode.  A config that   */
                                /* asks for compute_dtype = 1 but does not qualify (num_initial_filters % 8 != 0, a      */
                                /* tap-less conv phase, rows beyond the bf16 kernels' 32-bit offsets) gets the exact-fp32 */
                                /* plan and reports 0 here -- callers label their results with THIS value.                */
} wun_plan_info;

typedef struct wun_tensor_info {
    char    name[64];           /* TF variable name, e.g. "separator/conv1d_3/kernel"        */
    int64_t offset;             /* float offset into the arenas                              */
    int32_t ndim;
    int64_t shape[4];
} wun_tensor_info;

/* UnetAudioSeparator.get_padding (UnetAudioSeparator.py:34-83): smallest valid
 * (input_frames, output_frames) whose output covers desired_frames.  Pure host integer work. */
int wun_get_padding(const wun_config* cfg, int64_t desired_frames,
                    int64_t* input_frames, int64_t* output_frames);

/* Build the static plan for (config, batch, input_frames): the equivalent of the reference
 * building its TF graph once (Training.py:47).  Fails with WUN_ERR_INVALID where the
 * reference's asserts would (UnetAudioSeparator.py:55,121; Utils.py:117). */
int wun_plan_create(const wun_config* cfg, int64_t batch, int64_t input_frames, wun_plan** out);
void wun_plan_destroy(wun_plan* plan);
int wun_plan_query(const wun_plan* plan, wun_plan_info* info);
int wun_plan_tensor(const wun_plan* plan, int64_t index, wun_tensor_info* info);

/* Where the forward activations of the plan live in the caller's workspace after wun_forward(training = 1) -- what
 * the backward pass reads its LeakyReLU derivatives from (Utils.py:79-80).  Used by the parity tests to pin the float64
 * oracle's LeakyReLU branch decisions to the ones the kernels took (a pre-activation within fp32 rounding of 0 otherwise
 * decides a 1-vs-0.2 factor differently in the two precisions), and by tools/ws_diff.py.  Every tensor is NCW:
 * element (b, c, j) is element b*batch_stride + c*pitch + j of the array that starts `offset` floats into the workspace
 * (float32 or bfloat16 elements: elem_bytes) and holds the POST-activation output of conv
 * position t0 + j*tstep of its layer (UnetAudioSeparator.py:98-100,102,123):
 *   kind 0, index i : decimated stream of down level i  (t0 = 0, tstep = 2: the [:, ::2, :] of :100)
 *   kind 1, index i : skip window of down level i       (context: the centre crop Utils.crop takes, t0 = crop start;
 *                                                         same padding: the whole conv output)
 *   kind 2          : bottleneck conv output (:102)
 *   kind 3, index j : output of up conv j (:123)
 * and, for the layer-by-layer parity tests of the bf16 mode (each launch's output against a float64 computation from the
 * tensors that launch read; tests/test_gpu_bf16.py), the other tensors a training step leaves in the workspace -- valid
 * after wun_loss_backward, same addressing, no activation implied:
 *   kind 4, index j : the 2x-upsampled input of up conv j (:109-118); not written by plans whose split-K epilogue
 *                     fuses the interpolation (compute_dtype = 0)
 *   kind 5, index j : d loss / d pre-activation of up conv j
 *   kind 6, index j : d loss / d (tensor of kind 4); compute_dtype = 0: only where the adjoint is not fused
 *   kind 7, index i : d loss / d pre-activation of down conv i at the positions of kind 1
 *   kind 8, index i : d loss / d pre-activation of down conv i at the positions of kind 0 (context only; with same
 *                     padding kind 7 holds the whole row)
 *   kind 9          : d loss / d pre-activation of the bottleneck conv
 * All fields are int64.  WUN_ERR_INVALID for an unknown kind / index. */
typedef struct wun_activation_info {
    int64_t offset;                         /* of the tensor, in FLOATS from the workspace base */
    int64_t batch_stride, pitch;            /* in ELEMENTS of the tensor */
    int64_t channels, frames;               /* frames = valid positions j per row */
    int64_t t0, tstep;
    int64_t elem_bytes;                     /* 4 = float32; 2 = bfloat16 (compute_dtype = 1: activations live in HBM as bf16) */
} wun_activation_info;
int wun_plan_activation(const wun_plan* plan, int32_t kind, int32_t index, wun_activation_info* info);

/* get_output (UnetAudioSeparator.py:85-144).
 *   params   : device, arena_floats
 *   mix_btc  : device, [B, Tin, C]
 *   workspace: device, workspace_floats (intermediates are kept for wun_loss_backward)
 *   outputs  : device, [S, B, Tout, C] -- source s in source_names order
 *   training : 0 => AudioClip active (Utils.py:82-92) */
int wun_forward(const wun_plan* plan, const float* params, const float* mix_btc,
                float* workspace, float* outputs, int training, void* stream);

/* Loss (Training.py:50-63) + full backward of the graph (the tf.gradients implied by
 * Training.py:77).  Must follow wun_forward(training=1) on the same workspace/outputs.
 *   targets  : device, [S, B, Tout, C]
 *   grads    : device, arena_floats (overwritten)
 *   loss     : device, 1 float */
int wun_loss_backward(const wun_plan* plan, const float* params, const float* mix_btc,
                      float* workspace, const float* outputs, const float* targets,
                      float* grads, float* loss, void* stream);

/* Same as wun_loss_backward, plus data-parallel overlap hooks: bucket k covers arena floats
 * [bucket_starts[k], end) where `end` is the previous bucket's start (buckets are given from the
 * END of the arena towards 0, i.e. in backward completion order).  bucket_events[k] (hipEvent_t,
 * created by the caller) is recorded -- on an internal stream -- as soon as every gradient at an
 * offset >= bucket_starts[k] is final, so the caller can start that bucket's all-reduce on a
 * communication stream (hipStreamWaitEvent) while the rest of the backward pass still runs.
 *
 * A C caller (no torch.distributed) pairs the events with its own RCCL calls -- the library itself links no collective
 * library -- exactly as wave-u-net_amd/parallel.py does:
 *     hipEventCreateWithFlags(&ev[k], hipEventDisableTiming) for every bucket;  comm = a non-blocking stream, highest priority
 *     wun_loss_backward_ex(..., stream, starts, (void* const*)ev, n);
 *     for k in 0..n-1:  hipStreamWaitEvent(comm, ev[k], 0);
 *                       ncclAllReduce(grads + starts[k], grads + starts[k], end[k] - starts[k], ncclFloat, ncclSum, nccl_comm, comm);
 *     hipEventRecord(done, comm); hipStreamWaitEvent(stream, done, 0);
 *     wun_adam_step(..., grad_scale = 1.0f / world_size, stream);
 * with wun_config.exclusive_streams = 0 (low-priority side streams beside a communication stream cost 40 %). */
int wun_loss_backward_ex(const wun_plan* plan, const float* params, const float* mix_btc,
                         float* workspace, const float* outputs, const float* targets,
                         float* grads, float* loss, void* stream,
                         const int64_t* bucket_starts, void* const* bucket_events, int32_t nbuckets);

/* Backward pass of get_output from an arbitrary upstream gradient -- what tf.gradients gives the reference for any loss
 * built on get_output's outputs (Training.py:50-63 picks MSE or a spectral L1; a caller may use any), with respect to the
 * variables and, optionally, the input mix.  Must follow wun_forward(training = 1) on the same workspace / outputs.
 *   outputs   : device, [S, B, Tout, C]  what wun_forward wrote (read for the tanh derivative)
 *   d_outputs : device, [S, B, Tout, C]  dL/d outputs
 *   grads     : device, arena_floats.  Parameter gradients are OVERWRITTEN exactly as wun_loss_backward writes them (same
 *               tensors, same offsets; padding floats are left as they are)
 *   d_mix     : device, [B, Tin, C] or NULL.  dL/d mix_btc, overwritten (0 at samples the network never reads); NULL = not
 *               computed, no extra launch.  One more launch (mix_grad_kernel) on `stream` near the end of the pass.
 * With d_outputs = 2 / (S B Tout C) * (outputs - targets) the parameter gradients are those of wun_loss_backward.
 * WUN_ERR_INVALID for a null plan / params / workspace / outputs / d_outputs / grads or bad buckets, before any GPU work;
 * WUN_ERR_UNSUPPORTED (with a message) for a d_mix the plan's shapes cannot serve.  mix_btc is not read (may be NULL).
 * wun_backward_ex: the data-parallel bucket hooks of wun_loss_backward_ex. */
int wun_backward(const wun_plan* plan, const float* params, const float* mix_btc, float* workspace,
                 const float* outputs, const float* d_outputs, float* grads, float* d_mix, void* stream);
int wun_backward_ex(const wun_plan* plan, const float* params, const float* mix_btc, float* workspace,
                    const float* outputs, const float* d_outputs, float* grads, float* d_mix, void* stream,
                    const int64_t* bucket_starts, void* const* bucket_events, int32_t nbuckets);

/* Backward pass for a subset of the variables (frozen layers, input-only gradients).  The arguments of wun_backward_ex /
 * wun_loss_backward_ex plus:
 *   select   : host, nselect bytes; select[k] != 0 selects tensor k (wun_plan_tensor order).  NULL = every tensor: the call
 *              is then exactly wun_backward_ex / wun_loss_backward_ex (nselect 0 or num_tensors).
 *   nselect  : num_tensors when select is given.
 * The gradient floats of a selected tensor are bit-identical to the full call's on the same inputs; the floats of the other
 * tensors in `grads` are NOT written.  d_mix and loss, when requested, are bit-identical to the full call's.  Layers in forward
 * order -- mix, down 0 .. L-1, bottleneck, then interp_j and up j for each j, the head; e = the earliest selected layer, or the
 * mix when d_mix is requested: no launch before e runs, and a weight-gradient launch runs only for a selected layer
 * (DESIGN.md 5.5).  Tuned launch positions, accumulation orders and the bucket events are those of the full call (every
 * event is recorded exactly once; a bucket without a selected tensor when the call reaches it).
 * A conv's kernel and bias are selected together, and the output layer's convs (every source) together: else
 * WUN_ERR_UNSUPPORTED.  interp_<j> is selected on its own.  wun_backward_select: grads may be NULL only when no tensor is
 * selected (input-only gradient: d_mix required).  No tensor selected and no d_mix, a bad nselect, or a NULL grads with a
 * selection: WUN_ERR_INVALID.  Every argument check runs before any GPU work.  Both compute modes; same workspace. */
int wun_backward_select(const wun_plan* plan, const float* params, const float* mix_btc, float* workspace,
                        const float* outputs, const float* d_outputs, float* grads, float* d_mix, void* stream,
                        const int64_t* bucket_starts, void* const* bucket_events, int32_t nbuckets,
                        const uint8_t* select, int64_t nselect);
int wun_loss_backward_select(const wun_plan* plan, const float* params, const float* mix_btc,
                             float* workspace, const float* outputs, const float* targets,
                             float* grads, float* loss, void* stream,
                             const int64_t* bucket_starts, void* const* bucket_events, int32_t nbuckets,
                             const uint8_t* select, int64_t nselect);

/* Gradient accumulation (k micro-batches per optimizer step): the arguments of wun_backward_select /
 * wun_loss_backward_select, but the parameter gradients are ADDED to `grads` instead of overwriting them.  Let G be what the
 * matching _select call with the same arguments would write to a gradient float: after the call every float of a selected
 * tensor holds old + G -- one IEEE fp32 add, round to nearest even (bit-equal to torch's float32 a + b).  All other floats
 * (unselected tensors, padding floats) are not written.  select = NULL means every tensor.
 *   d_mix, loss : WRITTEN, not accumulated; bit-equal to the _select call's.
 * Selection rules, argument checks (all before any GPU work) and bucket events are those of the _select calls; an event fires
 * once the ACCUMULATED values at offsets >= its start are final.  `grads` is read only after everything the caller queued on
 * `stream` before the call (the side streams wait on `stream` before they touch it).  Same launches, launch positions, tilings
 * and split counts as the _select call -- a pinned tuning table applies unchanged and G is bit-identical; only the kernels'
 * final gradient stores differ.  Both compute modes; same workspace.  Typical use: the first micro-batch calls
 * wun_loss_backward_ex (overwrite), the others wun_loss_backward_accumulate, the last one with the bucket events. */
int wun_backward_accumulate(const wun_plan* plan, const float* params, const float* mix_btc, float* workspace,
                            const float* outputs, const float* d_outputs, float* grads, float* d_mix, void* stream,
                            const int64_t* bucket_starts, void* const* bucket_events, int32_t nbuckets,
                            const uint8_t* select, int64_t nselect);
int wun_loss_backward_accumulate(const wun_plan* plan, const float* params, const float* mix_btc, float* workspace,
                                 const float* outputs, const float* targets, float* grads, float* loss, void* stream,
                                 const int64_t* bucket_starts, void* const* bucket_events, int32_t nbuckets,
                                 const uint8_t* select, int64_t nselect);

/* Optional autotuning pass (no reference counterpart): runs one forward + loss/backward on the
 * given buffers while timing, for every conv / weight-gradient launch of the step, the candidate
 * tile shapes and split factors, and caches the fastest per launch in the plan.  The contents of
 * outputs / loss / grads / workspace after this call are NOT meaningful (accumulating launches are
 * replayed while timing): run the real step afterwards.  Parameters and optimizer state are not
 * touched.  Synchronises the stream. */
int wun_plan_tune(const wun_plan* plan, const float* params, const float* mix_btc, float* workspace,
                  float* outputs, const float* targets, float* grads, float* loss, void* stream);

/* Tuned choices as text (one line per launch position), so a later process can reuse them without
 * re-tuning: export writes a NUL-terminated string into buf (WUN_ERR_INVALID if cap is too small or
 * the plan is untuned); import accepts that string for a plan of the same config / batch / length
 * written by the same library build (WUN_ERR_INVALID otherwise: the header line carries the config,
 * the launch-order version and the entry counts, and the table ends with an "end" line, so stale or
 * truncated tables are refused) and switches the plan to the tuned choices.  An entry that is not a
 * legal choice for the launch at its position is ignored at launch time (heuristic choice instead);
 * a split factor can never exceed the split-K scratch. */
int wun_plan_tune_export(const wun_plan* plan, char* buf, int64_t cap);
int wun_plan_tune_import(const wun_plan* plan, const char* text);

/* tf.train.AdamOptimizer update (Training.py:77), TF rule:
 *   lr_t = lr*sqrt(1-b2^t)/(1-b1^t); m,v; theta -= lr_t*m/(sqrt(v)+eps); g := grad_scale*grad
 * step is 1-based.  grad_scale = 1/world_size after a sum all-reduce. */
int wun_adam_step(const wun_plan* plan, float* params, const float* grads, float* m, float* v,
                  int64_t step, float lr, float beta1, float beta2, float eps, float grad_scale,
                  void* stream);

/* wun_adam_step on the selected tensors only (TF's minimize(loss, var_list=...)): params, m and v of a selected tensor are
 * bit-equal to what wun_adam_step writes; every other float of the three arenas is left as it is.  select / nselect as for
 * wun_backward_select, except that any subset is accepted (kernel and bias need not agree; nothing selected = no launch).
 * NULL select = wun_adam_step.  Same lr_t.  No host synchronisation, no allocation. */
int wun_adam_step_select(const wun_plan* plan, float* params, const float* grads, float* m, float* v,
                         int64_t step, float lr, float beta1, float beta2, float eps, float grad_scale,
                         void* stream, const uint8_t* select, int64_t nselect);

/* ---- global gradient norm, clipping, non-finite step skipping ---------------------------
 * Floats of the norm workspace (device, caller-owned, 8-byte aligned): [0, num_tensors) the per-tensor norms,
 * [num_tensors] the global norm, then float64 partial sums (one per chunk of at most 8192 floats of one tensor).
 * Negative (WUN_ERR_INVALID) for a null plan. */
int64_t wun_grad_norm_workspace_floats(const wun_plan* plan);

/* Global / per-tensor L2 norms of grad_scale * grads over the selected tensors (tf.clip_by_global_norm's global_norm):
 *   norm_ws[k]           = |grad_scale| * sqrt(sum of grads^2 over tensor k)  (0 for an unselected tensor)
 *   norm_ws[num_tensors] = |grad_scale| * sqrt(sum over the selected tensors)
 * Squares and sums in float64, each norm rounded once to fp32.  No atomics: the result is bitwise reproducible and does
 * not depend on the grid; a selected tensor's entry is bit-identical whatever else is selected.  Only the selected
 * tensors' floats are read (padding floats and unselected tensors may hold anything, NaN included).
 * select / nselect as wun_adam_step_select (any subset; NULL = every tensor).  grads is read in stream order on `stream`
 * (after a data-parallel all-reduce: once `stream` has waited for it, as for wun_adam_step).  No host synchronisation.
 * WUN_ERR_INVALID before any GPU work for a null plan / grads / norm_ws, a misaligned norm_ws or a bad nselect. */
int wun_grad_norm(const wun_plan* plan, const float* grads, float grad_scale, float* norm_ws,
                  void* stream, const uint8_t* select, int64_t nselect);

#define WUN_CLIP_SKIP_NONFINITE 1
/* wun_grad_norm into norm_ws, then TF-Adam (wun_adam_step / wun_adam_step_select) on the clipped gradient, the global
 * norm N read on the device (the host never sees it):
 *   g := grad_scale * grad;  if (N > clip_norm) g := g * (clip_norm / N);  then wun_adam_step's m, v, theta.
 * With no clipping (N <= clip_norm, or clip_norm = +INFINITY) params, m and v are BIT-EQUAL to wun_adam_step /
 * wun_adam_step_select.  tf.clip_by_global_norm scales by clip_norm * min(1/N, 1/clip_norm), which is not exactly 1 when
 * inactive; the scale here, clip_norm / N, is rounded once and may differ from TF's by 1 ulp when clipping.
 * flags & WUN_CLIP_SKIP_NONFINITE: when N is not finite (an inf / NaN in a selected gradient), params, m and v are not
 * written and the device int64 *skipped is incremented by one.  Without that flag skipped may be NULL and a non-finite N
 * flows into the update as TF's would.
 * step: the caller's global_step, counted per call as TF counts sess.run -- a skipped step still advances it, so the next
 * applied update uses lr_t of the caller's step, not that of the number of updates applied (no device step counter).
 * WUN_ERR_INVALID before any GPU work for a null plan / params / grads / m / v / norm_ws, a misaligned norm_ws,
 * clip_norm <= 0 or NaN, step < 1, unknown flags, a bad nselect, or a null skipped with WUN_CLIP_SKIP_NONFINITE.
 * Both compute modes (the arenas are fp32 in both).  No host synchronisation, no allocation. */
int wun_adam_step_clip(const wun_plan* plan, float* params, const float* grads, float* m, float* v,
                       int64_t step, float lr, float beta1, float beta2, float eps, float grad_scale,
                       float clip_norm, int32_t flags, float* norm_ws, int64_t* skipped,
                       void* stream, const uint8_t* select, int64_t nselect);

/* ---- the extended optimizer: decoupled weight decay (AdamW) and an EMA of the weights ---------
 * flags: WUN_CLIP_SKIP_NONFINITE as for wun_adam_step_clip, and WUN_OPTIM_EMA_WARMUP. */
#define WUN_OPTIM_EMA_WARMUP 2
typedef struct wun_optim_config {
    float beta1, beta2, eps;       /* TF-Adam's, as wun_adam_step takes them */
    float weight_decay;            /* >= 0; 0 = none */
    float ema_decay;               /* in [0, 1); read only when ema is given */
    float clip_norm;               /* > 0; +INFINITY = no clipping */
    int32_t flags;
} wun_optim_config;
/* sizeof(wun_optim_config) as the library was compiled (wun_abi_sizes keeps its three entries). */
int64_t wun_optim_abi_size(void);

/* wun_adam_step_clip with two more steps fused into the same pass over the arenas.  For every float of a selected tensor, in
 * this order, each product rounded as written (no fused multiply-add where the formula has none):
 *   g, the clip scale, m, v      exactly as wun_adam_step_clip (grad_scale, clip_norm / N, WUN_CLIP_SKIP_NONFINITE, skipped)
 *   theta = theta * (1 - lr * weight_decay)          only for a tensor in decay_select -- torch.optim.AdamW's decoupled decay:
 *                                                    lr, not lr_t; the factor is formed once on the host in float64 and rounded
 *                                                    to fp32, so weight_decay = 0 gives exactly 1 and leaves the bits alone
 *   theta -= lr_t * m / (sqrt(v) + eps)              wun_adam_step's expression
 *   ema -= (1 - d_t) * (ema - theta)                 only when ema is non-NULL, on the NEW theta: the form of
 *                                                    tf.train.ExponentialMovingAverage / assign_moving_average;
 *                                                    d_t = ema_decay, or min(ema_decay, (1 + step) / (10 + step)) with
 *                                                    WUN_OPTIM_EMA_WARMUP (TF's num_updates rule); 1 - d_t is formed once on
 *                                                    the host in float64 from the fp32 ema_decay and rounded once
 * PINNED: with weight_decay = 0 and ema = NULL, params, m and v are BIT-EQUAL to wun_adam_step / _select / _clip for the same
 * arguments; with ema given and no decay they still are, and ema is the formula applied to those bits (wun_ema_update's bits).
 * decay_select / ndecay: a second byte table with select's conventions (NULL = every tensor decays); a tensor decays when it
 * is selected and in decay_select.  ema is an arena like params (the caller initialises it, e.g. as a copy of params: TF's
 * shadow variables start at the variable's value).
 * A skipped step writes none of theta, m, v, ema and increments *skipped once.  Unselected tensors and the padding floats
 * between tensors are not touched in any of the four arenas (NULL select = every tensor, still not the padding).  No atomics;
 * the bits do not depend on the grid, the stream, the arenas' alignment beyond 4 bytes (16-byte accesses run only where all
 * arenas share one alignment, through the same expressions) or on how tensors merge into ranges.
 * clip_norm = +INFINITY without WUN_CLIP_SKIP_NONFINITE: the norm is not launched and norm_ws may be NULL; otherwise norm_ws
 * as for wun_adam_step_clip.  step: as wun_adam_step_clip (1-based, counted per call).
 * WUN_ERR_INVALID before any GPU work for a null plan / params / grads / m / v / cfg, a null or misaligned norm_ws when the
 * norm is needed, step < 1, weight_decay < 0 or NaN, ema_decay outside [0, 1) with a non-null ema, clip_norm <= 0 or NaN,
 * unknown flags, a bad nselect or ndecay, or a null skipped with WUN_CLIP_SKIP_NONFINITE.
 * Both compute modes (the arenas are fp32 in both).  No host synchronisation, no allocation. */
int wun_optim_step(const wun_plan* plan, float* params, const float* grads, float* m, float* v, float* ema,
                   int64_t step, float lr, float grad_scale, const wun_optim_config* cfg, float* norm_ws,
                   int64_t* skipped, void* stream, const uint8_t* select, int64_t nselect,
                   const uint8_t* decay_select, int64_t ndecay);

/* The EMA line of wun_optim_step alone, for callers whose optimizer is not this library's (torch.optim on the autograd
 * module): ema -= (1 - d_t) * (ema - params) on the selected tensors, the same bits as the fused path given the same params,
 * ema_decay, step and flag.  flags: 0 or WUN_OPTIM_EMA_WARMUP.  WUN_ERR_INVALID before any GPU work for a null plan / ema /
 * params, ema_decay outside [0, 1), step < 0, unknown flags or a bad nselect.  No host synchronisation, no allocation. */
int wun_ema_update(const wun_plan* plan, float* ema, const float* params, float ema_decay, int64_t step, int32_t flags,
                   void* stream, const uint8_t* select, int64_t nselect);

/* ---- sample-rate conversion of the audio boundary ---------------------------------------
 * Rational polyphase resampler: what the reference does with librosa on the way into and out of Evaluate.predict
 * (Evaluate.py:59-67,104; Utils.py:94-95), fused with the channel mapping and the context padding around it.
 *   y[n] = sum_m v[m] * h[n*down - m*up + half],  v = the channel-mapped input, zero outside [0, n_in)
 * up / down = sr_out / sr_in reduced by their gcd; the result has ceil(n_in * up / down) frames (librosa's and scipy's
 * rule).  h is the default filter of scipy.signal.resample_poly -- NOT resampy's kaiser_best table that librosa uses:
 * half = 10 * max(up, down), 2*half + 1 taps, windowed sinc with cutoff 1 / max(up, down) of Nyquist, Kaiser window
 * beta = 5.0, unit DC gain, times up.  The table the kernel reads is PHASE-MAJOR fp32: K = ceil((2*half + 1) / up) floats per
 * row, up rows, table[p*K + k] = h[p + k*up] (0 past the last tap); output n uses row (n*down + half) % up.
 * Audio is float32 [T, C] channel-last.  Every device buffer is the caller's; nothing allocates or synchronises. */

/* up / down after the gcd.  WUN_ERR_INVALID for a null pointer or a rate <= 0; WUN_ERR_UNSUPPORTED when max(up, down)
 * exceeds 16384 (44 100 -> 8 192 Hz needs 11 025): the table has about 20 * max(up, down) floats. */
int     wun_resample_ratio(int32_t sr_in, int32_t sr_out, int32_t* up, int32_t* down);
/* ceil(n_in * up / down), and the floats of the phase-major table; negative wun_status for bad arguments (up, down must be
 * positive, coprime and within the ceiling). */
int64_t wun_resample_frames(int64_t n_in, int32_t up, int32_t down);
int64_t wun_resample_table_floats(int32_t up, int32_t down);
/* Host: design the filter in float64 (Bessel I0 by its power series) and write the fp32 phase-major table into
 * table_host[cap].  WUN_ERR_INVALID for a null pointer or cap < wun_resample_table_floats.  up == down == 1 gives the
 * unit impulse (never read by wun_resample). */
int     wun_resample_design(int32_t up, int32_t down, float* table_host, int64_t cap);
/* Device: y[(y_offset + n) * c_out + c] for n < n_out <= wun_resample_frames(n_in, up, down); nothing else of y is
 * written (a caller that zeroes a longer y gets the context padding of Evaluate.py:121-122 for free; a caller that caps
 * n_out gets the [:n] of Evaluate.py:64).
 *   x          : device, [n_in, c_in]
 *   y          : device, at least [y_offset + n_out, c_out]
 *   channels   : c_in == c_out (1 or 2): per channel;  c_out == 1, c_in <= 8: the mean of the input channels (sequential
 *                fp32 sum, one divide: np.mean(axis=1), Evaluate.py:98-99);  c_in == 1, c_out == 2: duplicated
 *                (Evaluate.py:65-67,101-102)
 *   table_dev  : device copy of wun_resample_design's table for the same up / down (may be NULL when up == down)
 * One output frame per lane, taps accumulated by fp32 FMA in one fixed order (k ascending): the result is bitwise
 * reproducible and does not depend on y_offset, the grid or pointer alignment; no atomics.  up == down is the
 * channel-mapped copy, exact.  WUN_ERR_INVALID before any GPU work for null pointers, up / down not positive and coprime,
 * another channel pair, negative lengths or n_out beyond the rule; WUN_ERR_UNSUPPORTED above the ratio ceiling or when
 * the input window of 256 outputs (255 * down / up + K frames) exceeds 64 KB. */
int     wun_resample(const float* x, int64_t n_in, int32_t c_in, float* y, int64_t y_offset, int64_t n_out,
                     int32_t c_out, const float* table_dev, int32_t up, int32_t down, void* stream);

/* ---- BSS Eval v4 scoring: lagged correlations and window energies -----------
 * The two heavy steps of scoring a separation the way museval's `v4` mode does (Evaluate.py:146-158): the correlations
 * the track's 512-tap projection filters are solved from, and, per window and source, the projections on those filters
 * with the eight energies SDR / ISR / SIR / SAR are ratios of.  The solve between the two is the caller's (float64,
 * any LAPACK; wave_u_net_amd.bsseval does it with torch.linalg).
 *   refs, ests : device, float32 [S, n, C] channel-last: references and estimates, one sample rate, same source order
 *   A = S * C reference signals, signal a = j * C + c;  L = filters_len in 1..512;  signals are zero outside [0, n)
 * Everything is accumulated in float64 in ONE order fixed by the sizes: correlations in chunks of 16384 frames, each an
 * FMA chain in ascending time, the chunks then added in ascending order; energies in tiles of 256 output frames, each
 * reduced by one fixed tree, the tiles then added in ascending order (tiles count from the window's start).  No atomics:
 * the bits do not depend on the grid, the stream, pointer alignment or where a track lies in a buffer.
 * Every buffer is the caller's; nothing allocates or synchronises, and every argument check runs before any GPU work.
 * All entries: WUN_ERR_INVALID for a null pointer, S < 1, C not 1 or 2, L outside 1..512 or n < 1. */

/* Host: the window table.  window, hop in frames (museval: int(1.0 * sr) each); nwin = (n - window + hop) / hop windows
 * [k hop, k hop + window), the LAST one extended to end at n; n < window or window == 0 (no windowing): one window
 * [0, n).  Returns the count and writes starts[cap] / lengths[cap] (both NULL: count only).  WUN_ERR_INVALID for
 * n < 1, window < 0, hop < 1 with a window, one table NULL without the other, or a cap below the count. */
int64_t wun_bss_windows(int64_t n, int64_t window, int64_t hop, int64_t* starts, int64_t* lengths, int64_t cap);

/* float64 elements of `scratch` that serve both entries below: the larger of ceil(n / 16384) * A * 2A * L (correlation
 * partials) and min(nwin, 64) * S * ceil((max_len + L - 1) / 256) * 8 (energy partials), max_len = the longest window.
 * Negative wun_status for bad arguments (also nwin < 0 or max_len outside 0..n). */
int64_t wun_bss_scratch_doubles(int32_t S, int64_t n, int32_t C, int32_t L, int64_t nwin, int64_t max_len);

/* R[a][b][l] = sum_t s_a[t] * s_b[t + l] and D[a][q][l] = sum_t s_a[t] * est_q[t + l] for l in [0, L), every ordered
 * pair: device float64 [A][A][L] each (q = j * C + c of the estimates).  Negative lags are not stored:
 * r_ab[-l] = R[b][a][l].  One launch covers R and D (each staged sample feeds up to 4 x 4 pairs) plus one finish launch. */
int wun_bss_correlations(const float* refs, const float* ests, int32_t S, int64_t n, int32_t C, int32_t L,
                         double* R, double* D, double* scratch, void* stream);

/* energies[k][j][0..8) for window k < nwin and source j, device float64 [nwin][S][8], over the w + L - 1 output frames of
 * the window's slices (w = lengths[k]; slices zero-extended):
 *   0 E(s)  1 E(est)  2 E(est - s)  3 E(P_own - s)  4 E(P_own)  5 E(P_all - P_own)  6 E(P_all)  7 E(est - P_all)
 *   P_all[u][c] = sum_a sum_l c_all[j][a][l][c] * s_a[start + u - l],  P_own the same over source j's own C signals with
 *   c_own[j][c'][l][c]; only frames of the WINDOW's slice enter (u - l in [0, w)).  E sums squares over frames and channels.
 *   c_all : device float64 [S][A][L][C];  c_own : device float64 [S][C][L][C];  both NULL: the filter-free form -- only
 *           energies 0..2 are computed (3..7 are written as 0), each audio float is read once, L is not used beyond its check
 *   starts, lengths : HOST, nwin windows in frames (wun_bss_windows; copied into the launches, 64 windows per launch)
 * WUN_ERR_INVALID also for nwin < 1, a window outside [0, n) or one filter pointer NULL without the other;
 * WUN_ERR_UNSUPPORTED with filters when A = S * C > 8 (the projection stages A * (255 + L) float64 in LDS). */
int wun_bss_window_energies(const float* refs, const float* ests, int32_t S, int64_t n, int32_t C, int32_t L,
                            const double* c_all, const double* c_own, const int64_t* starts, const int64_t* lengths,
                            int64_t nwin, double* energies, double* scratch, void* stream);

/* ---- recursive filtering along time and the BS.1770-4 loudness meter -----------
 * Audio is device float32 [n, C] interleaved, C in {1, 2}, any 4-byte alignment; arithmetic is float64.  Every buffer is
 * the caller's; nothing allocates or synchronises, no atomics, every sum has one order fixed by the sizes, and every
 * argument check runs before any GPU work.  All entries: WUN_ERR_INVALID for a null pointer, n < 1, C not 1 or 2, a
 * scratch / float64 pointer off 8 bytes; WUN_ERR_UNSUPPORTED above 2^40 frames.
 *
 * The parallel schedule of a recurrence is part of its definition here (the bits do not depend on the grid, the stream or
 * where buffers lie): time is cut into chunks of wun_sos_chunk() frames.  (1) every chunk runs the cascade with the true
 * input history and ZERO recursive state and keeps its end state; (2) a carry pass turns the end states into every chunk's
 * true start state, v[k+1] = M v[k] + e[k], with M the 2 nsec x 2 nsec zero-input transition of a whole chunk (formed on
 * the host in float64 by repeated squaring) -- in two levels: the wun_sos_tile() chunks of a group are walked from zero, the
 * group ends are walked with M^tile, the groups are walked again from their true starts; a step computes row r as
 * acc = e[r], acc = fma(M[r][q], v[q], acc) for q ascending; (3) every chunk runs again from its true state and writes.  The state of section s is (y_s[t-1], y_s[t-2]).  A short last chunk needs no power of
 * its own: its end state has no reader. */
int32_t wun_sos_chunk(void);                      /* frames per chunk (256) */
int32_t wun_sos_tile(void);                       /* chunks per workgroup and per carry group (64) */

/* float64 elements of `scratch` for wun_sosfilt: 2 nsec C (chunks + groups).  Negative wun_status for bad arguments. */
int64_t wun_sosfilt_scratch_doubles(int64_t n, int32_t C, int32_t nsec);

/* y = sosfilt(sos, x) per channel from zero initial state (scipy.signal.sosfilt): sos is HOST float64 [nsec][6] =
 * b0 b1 b2 a0 a1 a2 with a0 == 1, 1 <= nsec <= 8.  Per section, direct form I,
 *   y[t] = b0 x[t] + b1 x[t-1] + b2 x[t-2] - a1 y[t-1] - a2 y[t-2]
 * in float64 (the five products added in that order by FMA), the last section's output rounded once to float32.
 * WUN_ERR_INVALID also for nsec outside 1..8, a coefficient that is not finite, a0 != 1, or x and y overlapping. */
int wun_sosfilt(const float* x, int64_t n, int32_t C, const double* sos, int32_t nsec, float* y, double* scratch,
                void* stream);

/* Host: the K-weighting of ITU-R BS.1770-4 at sample rate sr as two sections sos[2][6] (the high shelf, then the
 * high-pass with b = 1, -2, 1), from the analogue prototype by the bilinear transform -- at 48000 Hz the standard's
 * table.  WUN_ERR_INVALID for sr outside 4000..384000. */
int wun_kweight_design(int32_t sr, double* sos);

/* Host: complete gating blocks of n frames at sr: Nb = round(0.4 sr) frames at a step of round(0.1 sr) (halves up);
 * (n - Nb) / step + 1 for n >= Nb, else 0.  Negative wun_status for n < 1 or sr outside 4000..384000. */
int64_t wun_loudness_blocks(int64_t n, int32_t sr);

/* float64 elements of `scratch` for wun_loudness.  Negative wun_status for bad arguments. */
int64_t wun_loudness_scratch_doubles(int64_t n, int32_t C, int32_t sr);

/* Integrated loudness of x (BS.1770-4 / EBU R 128, every channel weighted 1), all of it on the device:
 *   the signal is K-weighted by the schedule above; its third pass accumulates squares, the filtered signal is never written
 *   z_j = sum_c (sum_t y_c[t]^2) / Nb over block j (channels ascending; within a channel ascending time, in pieces cut at
 *         chunk and block boundaries);  l_j = -0.691 + 10 log10 z_j
 *   absolute gate l_j > -70;  relative gate l_j > (-0.691 + 10 log10 mean of the absolute-gated z) - 10
 *   L = -0.691 + 10 log10 mean of z over the blocks passing both (means: 256 strided partial sums, then a fixed tree)
 *   meter  : device float64 [4]: L (-inf when no block passes, NaN when a block is NaN), blocks kept, blocks nb, max |x|
 *            (NaN when x holds one)
 *   blocks : device float64 [nb] momentary values l_j, or NULL
 * WUN_ERR_INVALID also for sr outside 4000..384000. */
int wun_loudness(const float* x, int64_t n, int32_t C, int32_t sr, double* meter, double* blocks, double* scratch,
                 void* stream);

/* gain[0] = (float) g and gain[1] = (float)(1.0 / (double) gain[0]), device float32 [2], from a meter of wun_loudness:
 * in float64 g = 10^((target_lufs - L) / 20), capped at 10^(max_gain_db / 20) and, when peak_limit > 0, at
 * peak_limit / peak; a non-finite L gives exactly 1.  WUN_ERR_INVALID for a target that is not finite, max_gain_db < 0
 * or peak_limit < 0 (0: no limit). */
int wun_loudness_gain(const double* meter, double target_lufs, double max_gain_db, double peak_limit, float* gain,
                      void* stream);

/* x[i] *= *gain for i < count, in place, one fp32 rounding; the factor is read on the device.  WUN_ERR_INVALID for
 * count < 1. */
int wun_scale_by(float* x, int64_t count, const float* gain, void* stream);

/* ---- the rest of an EBU R 128 meter: true peak, short-term loudness, loudness range ----
 * The contract of the section above holds: the caller's buffers, scratch sized by a *_scratch_doubles query, no
 * allocation, no host synchronisation, no atomics, every argument check before any GPU work.
 *
 * Oversampling factor: the smallest power of two L in 1..32 with L * sr >= 176400 (192 k: 1, 96 k: 2, 48 k and
 * 44.1 k: 4, 22.05 k: 8, 8 k: 32).  Negative wun_status for sr outside 4000..384000. */
int32_t wun_true_peak_factor(int32_t sr);

/* float64 elements of `scratch` for wun_true_peak: one partial per channel and workgroup of 1024 frames. */
int64_t wun_true_peak_scratch_doubles(int64_t n, int32_t C);

/* True peak: max over t, c of |r_c[t]|, r being BIT FOR BIT what wun_resample writes for up = L, down = 1 per channel
 * (no channel mapping), all n L outputs: with the table of wun_resample_design(L, 1) on the device (K = 21 taps per
 * phase), u = t + 10 L, q = u / L, p = u % L, acc = fmaf(table[p K + k], x[q - k], acc) for k ascending from +0, x = +0
 * outside the input.  r is never written.  L == 1: r = x, the sample peak; table_dev may be NULL then.
 *   out : device float64 [1 + C]: the overall maximum, then one per channel, each holding a float32 value exactly.  A NaN
 *         SAMPLE in a channel makes that channel's and the overall value NaN; the NaNs an infinite sample makes of r are
 *         dropped by the maximum, which is then +inf.
 * The interpolator is this project's resampler -- scipy.signal.resample_poly's default Kaiser design -- NOT the 48-tap
 * table of BS.1770-4 Annex 2; no bound on the under-read is claimed.  WUN_ERR_INVALID also for an L that is not a power
 * of two in 1..32 or a null table with L > 1. */
int wun_true_peak(const float* x, int64_t n, int32_t C, int32_t L, const float* table_dev, double* out, double* scratch,
                  void* stream);

/* Host: complete short-term blocks of n frames at sr: N3 = round(3 sr) frames at the meter's step round(0.1 sr) (halves
 * up, in integers); (n - N3) / step + 1 for n >= N3, else 0.  Negative wun_status for n < 1 or sr out of range. */
int64_t wun_loudness_short_term_blocks(int64_t n, int32_t sr);

/* float64 elements of `scratch` for wun_loudness_r128.  Negative wun_status for bad arguments. */
int64_t wun_loudness_r128_scratch_doubles(int64_t n, int32_t C, int32_t sr);

/* The R 128 readings of x in one call.  The K-weighting schedule runs ONCE; its third pass adds every y[t]^2 into the
 * 0.4 s pieces exactly as wun_loudness does and into a second set of pieces cut at the 3 s blocks' starts and ends.
 *   z3_j = sum_c (sum_t y_c[t]^2) / N3 over short-term block j (the order of z_j above);  s_j = -0.691 + 10 log10 z3_j
 *   range: absolute gate s_j > -70, relative gate s_j > (-0.691 + 10 log10 mean of the absolute-gated z3) - 20; the m
 *          values that pass sorted ascending (ties by block index) as v:
 *          LRA = v[((m - 1) 95 + 50) / 100] - v[((m - 1) 10 + 50) / 100] (integer division), 0 for m == 0, NaN with a
 *          NaN block.  The two ranks are selected on the device by counting, m^2 comparisons, without sorting.
 *   report     : device float64 [8]: integrated loudness, loudness range, largest momentary value l_j, largest short-term
 *                value s_j (both -inf with no complete block), true peak (L = wun_true_peak_factor(sr)), sample peak,
 *                gating blocks kept, short-term blocks kept (m).  Integrated loudness, sample peak and gating blocks
 *                kept are wun_loudness's bits for the same input.
 *   short_term : device float64 [wun_loudness_short_term_blocks] the s_j, or NULL
 *   table_dev  : wun_resample_design(L, 1) on the device; may be NULL when L == 1
 * WUN_ERR_INVALID also for sr outside 4000..384000; WUN_ERR_UNSUPPORTED above 2^20 short-term blocks (29 hours). */
int wun_loudness_r128(const float* x, int64_t n, int32_t C, int32_t sr, const float* table_dev, double* report,
                      double* short_term, double* scratch, void* stream);

/* ---- spectral training loss: STFT-magnitude L1 and its waveform gradient ----
 * The reference's other objective (Training.py:55-60): the L1 distance between STFT magnitudes, frame 1024, hop 768,
 * periodic Hann window, no padding -- here for up to 8 resolutions at once, next to the time-domain MSE.
 *   audio      : device, float32 [S, B, T, C] channel-last, as wun_forward writes its outputs; a ROW is one (s, b, c),
 *                R = S * B * C rows, row r = (s * B + b) * C + c; any 4-byte alignment
 *   resolution : (n_fft, hop), n_fft a power of two in 64..2048, 1 <= hop <= n_fft;  K = n_fft / 2 + 1 bins,
 *                F = 1 + (T - n_fft) / hop frames (integer division: tf's pad_end=False), frame f = samples [f hop, f hop + n_fft)
 *   table      : fp32 [2][n_fft][K]: Cb[n][k] = w[n] cos(2 pi ((n k) mod n_fft) / n_fft), then Sb[n][k] = -w[n] sin(the same),
 *                w[n] = 0.5 - 0.5 cos(2 pi n / n_fft); element (plane, n, k) at (plane * n_fft + n) * K + k
 *   Re[r][f][k] = sum_n x_r[f hop + n] Cb[n][k],  Im with Sb,  M = sqrt(Re^2 + Im^2)
 * No FFT: the transform is a GEMM against the table on the exact-fp32 MFMA, n ascending in one accumulator per output, so
 * the bits of a row do not depend on the batch around it.  Every buffer is the caller's; nothing allocates or
 * synchronises, no atomics, and every argument check runs before any GPU work.
 * All entries: WUN_ERR_UNSUPPORTED for an n_fft outside the list, WUN_ERR_INVALID for a hop outside 1..n_fft or T < n_fft
 * (checked in this order); the device entries also WUN_ERR_INVALID for a null pointer, S < 1, B < 1 or C not 1 or 2. */

/* F of T frames of audio, and the floats of a table; negative wun_status for bad arguments. */
int64_t wun_stft_frames(int64_t frames, int32_t n_fft, int32_t hop);
int64_t wun_stft_table_floats(int32_t n_fft);
/* Host: the table, designed in float64 (the angle reduced in integers first) and rounded once to fp32, into table_host[cap].
 * WUN_ERR_INVALID for a null pointer or cap < wun_stft_table_floats. */
int     wun_stft_design(int32_t n_fft, float* table_host, int64_t cap);
/* mags[r][f][k] = M of x (device float32 [R][F][K]): the magnitude spectrogram.  table_dev: device copy of the table of
 * n_fft.  The same kernel computes the magnitudes inside wun_spectral_loss: its signs are those of the differences of the
 * floats this entry returns for the same inputs. */
int     wun_stft_magnitude(const float* x, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                           const float* table_dev, float* mags, void* stream);
/* floats of `scratch` for wun_spectral_loss with these sizes: per resolution R F (4 K + n_fft) (both magnitudes, Re and Im
 * of the estimates, the gradients of the frames), plus the float64 partial sums (one per 1024 elements) and 2 floats of
 * alignment room.  Negative wun_status as wun_spectral_loss for the same arguments. */
int64_t wun_spectral_scratch_floats(int32_t S, int32_t B, int64_t Tout, int32_t C, int32_t nres, const int32_t* n_fft,
                                    const int32_t* hop);
/* L = mse_weight * MSE + sum_j weights[j] * L_j and dL / d outputs.
 *   MSE  = mean of (outputs - targets)^2 over all S B Tout C floats (wun_loss_backward's loss)
 *   L_j  = mean over rows, frames and bins of |M_est - M_tgt| at resolution j (Training.py:60,63)
 *   d_outputs[r][t] = mse_weight * 2 (out - tgt) / (S B Tout C)
 *                   + sum_j weights[j] / (R F_j K_j) * sum_{f: 0 <= t - f hop < n_fft} sum_k sgn(M_est - M_tgt)[f][k]
 *                     * (Re_est Cb[n][k] + Im_est Sb[n][k]) / M_est,  n = t - f hop
 *     with sgn(0) = 0 and the term of a bin with M_est == 0 equal to 0 (tf's gradient of a complex abs).  Samples behind
 *     the last frame get the MSE term alone; the targets carry no gradient.
 *   outputs, targets : device [S, B, Tout, C]
 *   n_fft, hop, weights : HOST, nres entries (0 <= nres <= 8; nres == 0: the MSE and its gradient alone)
 *   tables_dev       : HOST array of nres device pointers, tables_dev[j] = the table of n_fft[j]
 *   d_outputs        : device [S, B, Tout, C], every float written once; NULL: the losses only
 *   losses           : device float32 [2 + nres]: [0] = L, [1] = MSE, [2 + j] = L_j (unweighted)
 *   scratch          : device, wun_spectral_scratch_floats floats; what it held does not matter
 * The loss sums are float64 in an order fixed by the sizes (1024 elements per partial, one tree per partial, the partials
 * strided over 64 lanes and one tree).  The gradient is destination-driven: one lane per output float adds the MSE term,
 * then resolution after resolution the covering frames in ascending f; two calls give the same bits, whatever the grid,
 * the scratch contents or the pointer alignment.  Both compute modes (the outputs are fp32 in both).
 * WUN_ERR_INVALID also for nres outside 0..8, a null resolution table with nres > 0, or a negative or non-finite weight
 * (mse_weight included). */
int     wun_spectral_loss(const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
                          float mse_weight, int32_t nres, const int32_t* n_fft, const int32_t* hop, const float* weights,
                          const float* const* tables_dev, float* d_outputs, float* losses, float* scratch, void* stream);

/* ---- the multi-resolution STFT loss: four terms per resolution ----
 * wun_spectral_loss with L_j = sum_t termweight_t * term_t(j) in place of its one term.  Per resolution j, with the framing,
 * window, table, row order and [R][F][K] layout above:  E = Re_e + i Im_e the STFT of the estimates, T that of the targets,
 * Me = |E| and Mt = |T| THE FLOATS wun_stft_magnitude RETURNS, d = Me - Mt in fp32, sg = sgn(d) with sgn(0) = 0.
 *   mag_l1     : the mean over all R F K bins of |d| -- wun_spectral_loss's L_j.
 *                coefficient of (Re_e, Im_e) in the gradient: sg * (Re_e, Im_e) / Me, 0 where Me == 0
 *   log_mag_l1 : the mean over all bins of |log(Me + log_eps) - log(Mt + log_eps)| (fp32 logf); its sign is sg, log being monotone.
 *                coefficient: sg / (Me + log_eps) * (Re_e, Im_e) / Me, 0 where Me == 0
 *   sc         : spectral convergence PER SOURCE s, so that a quiet source is not swamped by a loud one:
 *                D_s = sum d^2 and N_s = sum Mt^2 over the source's B C F K bins, each square formed and summed in float64 from
 *                the fp32 d and Mt;  SC_s = sqrt(D_s / (N_s + sc_eps));  the term is the mean of SC_s over s.
 *                coefficient: d / (sqrt(D_s) sqrt(N_s + sc_eps)) / S * (Re_e, Im_e) / Me, 0 where D_s == 0 or Me == 0
 *   complex_l1 : phase-aware, the mean over all bins of |E - T| = sqrt(fmaf(a, a, b * b)), a = Re_e - Re_t, b = Im_e - Im_t.
 *                coefficient: (a, b) / |E - T|, 0 where the modulus is 0
 *   total = mse_weight * MSE + sum_j weights[j] * L_j;  d_outputs is the exact gradient of that total, signs and zero cases
 *   treated as constants (as wun_spectral_loss treats them).
 * The term weights must be finite and >= 0, log_eps and sc_eps finite and > 0; one set serves all resolutions.  A term whose
 * weight is 0 is not computed.  The usual log_eps = 1e-3 and sc_eps = 1.0 are choices, not measurements: log_eps sits above the
 * fp32 transform's own error on unit-scale audio (about 2e-4 at n_fft 64; it grows with n_fft, so long frames want a larger
 * one), so that the log of a silent bin is not the log of rounding noise; sc_eps keeps a source that is silent in the whole
 * batch (N_s == 0) finite: its SC_s is then sqrt(D_s / sc_eps). */
typedef struct { float mag_l1, log_mag_l1, sc, complex_l1, log_eps, sc_eps; } wun_spectral_terms;
/* floats of `scratch` for wun_spectral_loss_terms with these sizes and terms: wun_spectral_scratch_floats' per-resolution slice
 * R F (4 K + n_fft), plus 2 R F K (Re and Im of the targets) when complex_l1 > 0; then as float64 (2 floats each) one partial
 * per 1024 elements for the MSE and per resolution one per 1024 bins for each of mag_l1, log_mag_l1, complex_l1 in use, and
 * when sc > 0 per resolution 2 S ceil(B C F K / 1024) partials and 3 S per-source scalars; 2 floats of alignment room.
 * Negative wun_status as wun_spectral_loss_terms for the same arguments. */
int64_t wun_spectral_terms_scratch_floats(int32_t S, int32_t B, int64_t Tout, int32_t C, int32_t nres, const int32_t* n_fft,
                                          const int32_t* hop, const wun_spectral_terms* terms);
/* wun_spectral_loss's arguments and contract (the caller's buffers, no allocation, no sync, no atomics, every check before any
 * GPU work, d_outputs may be NULL, any 4-byte alignment, both compute modes, bits independent of the grid, the scratch
 * contents, the alignment and repetition), plus `terms` (HOST).  The checks of wun_spectral_loss come first, in its order; then
 * WUN_ERR_INVALID for a null `terms`, a negative or non-finite term weight, or an eps that is not finite and > 0.
 *   losses : device float32 [2 + 5 nres]: [0] = total, [1] = MSE, [2 + j] = L_j, [2 + nres + 4 j + t] = the unweighted term t
 *            of resolution j, t in the order mag_l1, log_mag_l1, sc, complex_l1 (0 for a term whose weight is 0)
 *   scratch: wun_spectral_terms_scratch_floats floats for the same terms
 * The means of mag_l1, log_mag_l1 and complex_l1 are summed as wun_spectral_loss sums (1024 consecutive bins per float64
 * partial, one tree, the partials strided over 64 lanes); the sums of sc run over 1024-bin blocks of each source's own bins, so
 * a source's D_s and N_s do not depend on the other sources.  With terms = {1, 0, 0, 0, ..} the first 2 + nres losses and
 * d_outputs are wun_spectral_loss's, bit for bit. */
int     wun_spectral_loss_terms(const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
                                float mse_weight, int32_t nres, const int32_t* n_fft, const int32_t* hop, const float* weights,
                                const wun_spectral_terms* terms, const float* const* tables_dev, float* d_outputs, float* losses,
                                float* scratch, void* stream);

/* ---- waveform losses: MSE, L1, scale-invariant SDR and SNR ----
 * The time-domain objectives beside the spectral ones: total = sum_t weight_t * term_t over the four terms below, and
 * d total / d outputs.  outputs (the estimates e) and targets (t) are device float32 [S, B, Tout, C] as above.
 *   N = S B Tout C floats.  A ROW is one (s, b): R = S B rows, r = s B + b, the n = Tout C contiguous floats of that excerpt,
 *   all channels together -- one scale per excerpt, as BSS Eval has one per track.
 * Flat terms (d = e - t formed in fp32):
 *   mse    : the mean over all N floats of d^2.   gradient cm * d, cm = (float)(mse * 2.0 / N) -- what wun_spectral_loss forms
 *   l1     : the mean of |d|.                     gradient (float)(l1 / N) * sgn(d), sgn(0) = 0
 * Row quantities, in float64 from the fp32 samples: sum e, sum t, sum e e, sum t t, sum e t, sum d d per row, every product
 * formed in float64 (exact), for sum d d the difference too.  With zero_mean: mu_e = sum e / n, mu_t = sum t / n and
 *   See = max(sum ee - sum e mu_e, 0)   Stt = max(sum tt - sum t mu_t, 0)   Set = sum et - sum e mu_t
 *   Dd  = max(sum dd - (sum e - sum t)^2 / n, 0)
 * without it mu_e = mu_t = 0 and See, Stt, Set, Dd are the raw sums.  e' = e - mu_e, t' = t - mu_t, d' = e' - t'.
 * Row terms, k = 10 / ln 10, w the term's weight:
 *   si_sdr : P = Set^2 / (Stt + eps), Nn = max(See - P, 0), SI_r = 10 log10((P + eps) / (Nn + eps)); the term is -(1 / R) sum_r SI_r.
 *            gradient of the weighted term: A_r e'_i + B_r t'_i,  A_r = 2 k w / (R (Nn + eps)),
 *            B_r = -(w k / R) (2 Set / (Stt + eps)) (1 / (P + eps) + 1 / (Nn + eps))
 *   snr    : SNR_r = 10 log10((Stt + eps) / (Dd + eps)); the term is -(1 / R) sum_r SNR_r.
 *            gradient: G_r d'_i,  G_r = 2 k w / (R (Dd + eps))
 *   The clamps are constants of the gradient: the closed forms are evaluated at the clamped values and max() itself is not
 *   differentiated.  A term whose weight is 0 is not computed, is reported as 0 and adds nothing to the gradient.
 * Consequences: a row of zero estimates gets an si_sdr gradient of exactly 0 (Set = 0 and e' = 0: the term cannot leave silence
 * on its own; combine it with l1 or mse).  A silent target row stays finite: SI_r = 10 log10(eps / (See + eps)).  Estimates
 * bit-equal to the targets give SI_r ~ 10 log10(Stt / (2 eps)), not infinity.  eps = 1e-8 (the Python default) is a choice, not
 * a measurement: it lies 80 dB below a row of unit energy and far above the float64 sums' own error.
 *   losses : device float32 [5 + 2 S]: [0] the total, [1..4] the UNWEIGHTED mse, l1, si_sdr, snr terms, [5 + s] the mean of SI_r
 *            over source s's B rows (dB, higher is better), [5 + S + s] the mean of SNR_r, same convention
 *   d_outputs : device [S, B, Tout, C], every float written once; NULL: the losses only.  The targets carry no gradient.
 *   accumulate: 1: d_outputs += the gradient (one fp32 add of the old value, last) -- how this loss composes with the
 *            spectral one: wun_spectral_loss* writes d_outputs, this entry adds to it
 *   scratch: wun_waveform_scratch_floats floats: as float64 on an 8-byte boundary inside the buffer 2 ceil(N / 1024) flat
 *            partials, 6 R ceil(n / 1024) row partials and 8 R row scalars, plus 2 floats of alignment room
 * Summation: the flat sums keep wun_spectral_loss's partition and trees (1024 consecutive floats per float64 partial, lane tid
 * takes the items tid + 256 it ascending, one tree per block; the partials strided over 64 lanes ascending, one tree), so with
 * terms {mse: w} alone and accumulate = 0, losses[0], losses[1] and d_outputs are those of wun_spectral_loss(mse_weight = w,
 * nres = 0), bit for bit.  The row sums run over 1024-float chunks of each row's own floats (no block crosses a row), the
 * chunk partials strided over 256 lanes ascending and one tree: a row's scalars do not depend on the other rows.  The row
 * scalars stay on the device as float64; no host sync.
 * Gradient, per float: v = (A_r e' + B_r t') + G_r d' in float64 from the fp32 samples, every operation rounded on its own
 * (nothing fused), rounded once to fp32; then in fp32, unfused, in this order: cm * d, plus the l1 part, plus (float)v, and with
 * accumulate one final add of the old d_outputs[i].  Parts whose weights are 0 are left out, not added as zeros.
 * Contract: every buffer is the caller's; no allocation, no synchronisation, no atomics; every argument check runs before any
 * GPU work; any 4-byte alignment; runs beside plans of both compute modes; the bits do not depend on the grid, on what scratch
 * held, on pointer alignment or on repetition.  2 launches with mse / l1 alone, 4 with a row term.
 * WUN_ERR_INVALID for a null pointer (d_outputs excepted), S < 1, B < 1, Tout < 1, C not 1 or 2, a negative or non-finite term
 * weight, an eps that is not finite and > 0, accumulate not 0 or 1, or accumulate == 1 with d_outputs NULL. */
typedef struct { float mse, l1, si_sdr, snr, eps; int32_t zero_mean; } wun_waveform_terms;
/* floats of `scratch` for wun_waveform_loss with these sizes (the same for every set of terms):
 * 2 * (2 ceil(N / 1024) + 6 R ceil(n / 1024) + 8 R) + 2.  Negative wun_status as wun_waveform_loss for the same arguments. */
int64_t wun_waveform_scratch_floats(int32_t S, int32_t B, int64_t Tout, int32_t C, const wun_waveform_terms* terms);
int     wun_waveform_loss(const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
                          const wun_waveform_terms* terms, int32_t accumulate, float* d_outputs, float* losses, float* scratch,
                          void* stream);

/* ---- inverse STFT and soft-mask post-filter ----
 * The synthesis half of the spectral section, on the same table, and the post-filter built on the pair: the estimates of a
 * track are masked against the mixture's own STFT, so they share its phase and sum back to it.
 *   audio, rows, the table [2][n_fft][K] (Cb = w cos, Sb = -w sin), the periodic Hann window w and K = n_fft / 2 + 1 are
 *   those of the spectral section above.
 *   Centred framing : lead = n_fft - hop, F = ceil((T + lead) / hop) (wun_stft_centered_frames); frame f holds
 *                x[f hop - lead + n], 0 <= n < n_fft, and is zero outside [0, T).  When hop divides n_fft every sample of
 *                [0, T) lies in exactly n_fft / hop frames.  A track shorter than n_fft is legal.
 *   Complex STFT : Re[r][f][k] = sum_n frame_f[n] Cb[n][k], Im likewise with Sb.  lead and F are given by the caller;
 *                lead = 0 with F = wun_stft_frames(...) is the framing of the loss.  The accumulation order is the existing
 *                one: n ascending in one accumulator per output.
 *   Inverse STFT : frame_f[n] = (1 / n_fft) sum_k c_k (Re[f][k] Cb[n][k] + Im[f][k] Sb[n][k]), c_0 = c_{n_fft/2} = 1, every
 *                other c_k = 2; k ascending, a bin's real part before its imaginary part.
 *                y[t] = (sum_f frame_f[t + lead - f hop]) / (sum_f w^2[t + lead - f hop]), both sums over the covering frames
 *                (0 <= f < F, 0 <= t + lead - f hop < n_fft) in ascending f.  Where the denominator is below 1e-8, y[t] = 0
 *                (librosa's rule).  The denominator is computed from the window (float64), not from the table.  The
 *                overlap-add is destination-driven: one writer per output float, no atomics.
 *   Soft-mask filter, for one track with mix [n, C] and estimates [S, n, C], per channel:
 *                X = STFT(mix) and E_s = STFT(est_s) in the centred framing;  A_s = |E_s|^p, p in {1, 2} (p = 2 takes no
 *                square root);  mask_s = (A_s + eps / S) / (sum_j A_j + eps), j ascending -- the masks sum to 1 by
 *                construction;  out_s = ISTFT(mask_s X) over [0, n).  Requires hop a power of two and hop <= n_fft / 2, so
 *                every sample's window-square sum is at least 0.5.  Defaults of the callers: p = 2, eps = 1e-10.
 * Every buffer is the caller's; nothing allocates or synchronises; every argument check runs before any GPU work.  Results
 * do not depend on what `scratch` held, on pointer alignment beyond 4 bytes, or on how the frames are blocked internally
 * (blocks of 256 frames bound the scratch).  Both compute modes.
 * All entries, in this order: WUN_ERR_INVALID for a null pointer (device entries), S < 1, B < 1, C not 1 or 2 or T < 1;
 * WUN_ERR_UNSUPPORTED for an n_fft outside the spectral section's list; WUN_ERR_INVALID for a hop outside 1..n_fft, then
 * for lead outside [0, n_fft) or F < 1 (WUN_ERR_UNSUPPORTED for more than 2^30 frames in all). */

/* F of the centred framing: ceil((T + n_fft - hop) / hop).  Host only; negative wun_status for bad arguments. */
int64_t wun_stft_centered_frames(int64_t T, int32_t n_fft, int32_t hop);
/* re, im (device float32 [R][F][K]) = the complex STFT of x [S, B, T, C] with the caller's lead and F.  WUN_ERR_INVALID
 * also when re or im overlap x or each other. */
int     wun_stft_complex(const float* x, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                         int32_t lead, int64_t F, const float* table_dev, float* re, float* im, void* stream);
/* floats of `scratch` for wun_istft: R min(F, 256 + ceil(n_fft / hop) - 1) n_fft (the frames of one block), n_fft float64
 * window squares and 2 floats of alignment room.  Negative wun_status as wun_istft for the same arguments. */
int64_t wun_istft_scratch_floats(int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop, int32_t lead,
                                 int64_t F);
/* y (device [S, B, T, C], every float written once) = the inverse STFT of re, im [R][F][K].  Samples no frame covers are 0.
 * WUN_ERR_INVALID also when y overlaps re or im. */
int     wun_istft(const float* re, const float* im, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                  int32_t lead, int64_t F, const float* table_dev, float* y, float* scratch, void* stream);
/* floats of `scratch` for wun_mask_filter: with nb = min(F, 256 + n_fft / hop - 1) frames per block, 2 (S + 1) C nb K
 * (the spectra) + S C nb n_fft (the frames) + 2 n_fft + 2.  Negative wun_status as wun_mask_filter. */
int64_t wun_mask_filter_scratch_floats(int32_t S, int64_t n, int32_t C, int32_t n_fft, int32_t hop);
/* out (device [S, n, C], every float written once) = the soft-mask filter of ests [S, n, C] against mix_tc [n, C].
 * WUN_ERR_INVALID also for a hop that is no power of two or above n_fft / 2, a power other than 1 or 2, an eps that is not
 * finite and positive, or `out` overlapping an input; WUN_ERR_UNSUPPORTED for S > 8 (after the hop checks). */
int     wun_mask_filter(const float* mix_tc, const float* ests, int32_t S, int64_t n, int32_t C, int32_t n_fft, int32_t hop,
                        int32_t power, float eps, const float* table_dev, float* out, float* scratch, void* stream);

/* ---- multichannel Wiener post-filter: EM iterations of a local Gaussian model ----
 * What the soft mask cannot use is where a source sits between the channels.  For one track with mix [n, C] and estimates
 * [S, n, C], in the centred framing above, with X = STFT(mix), E_s = STFT(est_s) and vectors over the C channels:
 *   y_s(0) = mask_s X, the soft-mask filter exactly as defined above (power p in {1, 2}; mask_eps is its eps).
 *   For it = 1 .. I, every sum in ascending index order:
 *     v_s[f,k]  = (1 / C) sum_c |y_s[f,k,c]|^2
 *     R_s[k]    = (sum_f y_s[f,k] y_s[f,k]^H) / (eps + sum_f v_s[f,k])     C x C Hermitian, over ALL F frames of the track
 *     Cxx[f,k]  = sum_s v_s[f,k] R_s[k] + sqrt(eps) I
 *     y_s[f,k] <- v_s[f,k] R_s[k] Cxx[f,k]^-1 X[f,k]
 *   out_s = ISTFT(y_s(I)) over [0, n), through the inverse above.
 * The statistics (v, both sums, R) and the per-bin algebra (Cxx, its closed-form inverse, the gain, the product with X) are
 * computed in float64; spectra are stored as float32, so each y_s(it) is rounded to float32 once.  There is no global
 * rescaling of the mix (norbert's max_abs): with float64 algebra it is not needed.  Parity with norbert is not claimed.
 * C in {1, 2}, S <= 8, I in 0..4; defaults of the callers: p = 2, mask_eps = 1e-10, I = 1, eps = 1e-10.
 * I = 0 is wun_mask_filter, bit for bit.  The y_s sum to (Cxx - sqrt(eps) I) Cxx^-1 X: the mix up to the regulariser.
 * R_s needs the whole track and scratch must not grow with it, so the call makes I + 1 passes over the blocks of 256 frames:
 * pass i < I recomputes a block's spectra and mask, applies R(1) .. R(i) to reach y(i) (a frame's y(i) depends on that frame
 * and the R's alone) and adds the block's statistics of R(i+1); the last pass applies all I filters and inverts.  The
 * statistics are partial sums over chunks of 16 frames aligned to absolute frame numbers, added in ascending chunk order: no
 * atomics, the same bits from run to run, whatever `scratch` held.  Contract, checks and their order as wun_mask_filter; then
 * WUN_ERR_INVALID for `iterations` outside 0..4 or an `eps` that is not finite and positive.  Both compute modes. */

/* floats of `scratch` for wun_wiener_filter: wun_mask_filter_scratch_floats(S, n, C, n_fft, hop), plus, for iterations > 0,
 * 2 (iterations + 16) S (C^2 + 1) K -- per (source, bin) the C^2 real numbers of the Hermitian R and sum_f v, as float64, for
 * every iteration, and the 16 chunks' partial sums of one block.  Negative wun_status as wun_wiener_filter. */
int64_t wun_wiener_filter_scratch_floats(int32_t S, int64_t n, int32_t C, int32_t n_fft, int32_t hop, int32_t iterations);
/* out (device [S, n, C], every float written once) = the Wiener filter of ests [S, n, C] against mix_tc [n, C]. */
int     wun_wiener_filter(const float* mix_tc, const float* ests, int32_t S, int64_t n, int32_t C, int32_t n_fft, int32_t hop,
                          int32_t power, float mask_eps, int32_t iterations, float eps, const float* table_dev,
                          float* out, float* scratch, void* stream);

/* ---- the FFT path of the complex STFT, its inverse and the post-filters ----
 * The three sections above run every frame transform as a GEMM against a [2][n_fft][K] table: n_fft^2 + n_fft floats and
 * about 2 n_fft^2 flops per frame, which is why they stop at n_fft = 2048.  The entries below compute the SAME definitions --
 * framing, periodic Hann window, Re / Im layout [R][F][K], inverse, overlap-add, mask, EM -- with a fast Fourier transform,
 * for n_fft a power of two in 64..8192.  Only the summation order inside a frame transform differs, so the results agree with
 * the GEMM entries to float32 rounding, not bit for bit.
 *   table      : fp32 [3][n_fft], element (plane, t) at plane * n_fft + t:
 *                plane 0 = cos(2 pi t / n_fft), plane 1 = -sin(2 pi t / n_fft), plane 2 = w[t] = 0.5 - 0.5 cos(2 pi t / n_fft).
 *                Designed on the host in float64 -- t reduced in integers to a quarter turn, the quadrant applied exactly, so
 *                the entries at the multiples of pi / 2 are exactly 0 and +-1 -- and rounded once to fp32.  3 n_fft floats.
 *   forward    : y[n] = w[n] frame_f[n] (one fp32 product);  z[m] = y[2m] + i y[2m+1], Z = DFT of n_fft / 2 points (Stockham
 *                radix 4, one radix-2 stage last for an odd log2), then with M = n_fft / 2, for k = 0..M:
 *                E = (Z[k] + conj Z[M-k]) / 2,  O = (Z[k] - conj Z[M-k]) / 2i,  Re + i Im = E + exp(-2 pi i k / n_fft) O
 *                (Z[M] = Z[0]).  Im of the bins 0 and n_fft / 2 is written as exactly 0.
 *   inverse    : frame_f[n] = w[n] (1 / n_fft) sum_k c_k (Re[f][k] cos(2 pi n k / n_fft) - Im[f][k] sin(2 pi n k / n_fft)), c_k as
 *                above: w times the inverse real transform.  Im of the bins 0 and n_fft / 2 is not read (the GEMM definition
 *                multiplies it by Sb = 0).  The scale 1 / n_fft, a power of two, is applied once, then the window.  The
 *                overlap-add, the window-square sums and the 1e-8 rule are the inverse section's, by the same kernel.
 * A frame's floats depend on that frame's samples (or bins) and the table alone: not on the block, the grid, the frames that
 * share its workgroup, what `scratch` held or pointer alignment beyond 4 bytes.  No atomics; nothing allocates or
 * synchronises; every argument check runs before any GPU work.  Both compute modes.
 * Every entry takes the arguments of the entry it is named after, with table_dev = a device copy of THIS section's table,
 * and has its contract, scratch formula, checks and check order: null pointers, the audio shape, then WUN_ERR_UNSUPPORTED for
 * an n_fft that is no power of two in 64..8192, then the hop, lead and F (the filters: hop a power of two of at most
 * n_fft / 2, S <= 8, C in {1, 2}, power, eps, iterations).
 * The Wiener filter above 2048: see DESIGN.md 5.13 for why the float64 algebra needs no rescaling of the mix up to 8192. */

/* Floats of the table (3 n_fft), and the table itself into table_host[cap] (host).  WUN_ERR_UNSUPPORTED for an n_fft outside
 * the list; WUN_ERR_INVALID for a null pointer or cap < wun_fft_table_floats. */
int64_t wun_fft_table_floats(int32_t n_fft);
int     wun_fft_design(int32_t n_fft, float* table_host, int64_t cap);
/* wun_stft_frames (the framing without padding: 1 + (T - n_fft) / hop, WUN_ERR_INVALID for T < n_fft after the n_fft and hop
 * checks) and wun_stft_centered_frames for this section's n_fft list. */
int64_t wun_fft_frames(int64_t T, int32_t n_fft, int32_t hop);
int64_t wun_fft_centered_frames(int64_t T, int32_t n_fft, int32_t hop);
/* wun_stft_complex: one launch. */
int     wun_stft_complex_fft(const float* x, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                             int32_t lead, int64_t F, const float* table_dev, float* re, float* im, void* stream);
/* wun_istft_scratch_floats / wun_istft. */
int64_t wun_istft_fft_scratch_floats(int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop, int32_t lead,
                                     int64_t F);
int     wun_istft_fft(const float* re, const float* im, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                      int32_t lead, int64_t F, const float* table_dev, float* y, float* scratch, void* stream);
/* wun_mask_filter_scratch_floats / wun_mask_filter. */
int64_t wun_mask_filter_fft_scratch_floats(int32_t S, int64_t n, int32_t C, int32_t n_fft, int32_t hop);
int     wun_mask_filter_fft(const float* mix_tc, const float* ests, int32_t S, int64_t n, int32_t C, int32_t n_fft, int32_t hop,
                            int32_t power, float eps, const float* table_dev, float* out, float* scratch, void* stream);
/* wun_wiener_filter_scratch_floats / wun_wiener_filter.  iterations = 0 is wun_mask_filter_fft, bit for bit. */
int64_t wun_wiener_filter_fft_scratch_floats(int32_t S, int64_t n, int32_t C, int32_t n_fft, int32_t hop, int32_t iterations);
int     wun_wiener_filter_fft(const float* mix_tc, const float* ests, int32_t S, int64_t n, int32_t C, int32_t n_fft,
                              int32_t hop, int32_t power, float mask_eps, int32_t iterations, float eps,
                              const float* table_dev, float* out, float* scratch, void* stream);

/* ---- Griffin-Lim phase reconstruction: magnitudes to audio ----
 * Audio whose STFT magnitude approaches a given `mag`, by alternating projections (Griffin & Lim 1984; the reference's
 * Utils.reconPhase) with the optional acceleration of Perraudin, Balazs & Sondergaard 2013.  Rows are r = (s B + b) C + c of
 * audio [S, B, T, C]; spectra are [R][F][K], K = n_fft / 2 + 1; the caller gives lead and F exactly as for
 * wun_stft_complex_fft / wun_istft_fft.  STFT and ISTFT below are THAT section's, bit for bit: periodic Hann, wun_fft_design's
 * table, the window-square-normalised overlap-add (the least-squares inverse the method's convergence argument needs), the
 * 1e-8 rule, samples outside [0, T) read as 0.
 *   unit(c)   : c / |c|, and unit(0) = 1 (numpy's angle(0) is 0).  In float32, with c = re + i im:
 *                   if (re == 0 && im == 0)  u = 1 + 0 i            (either sign of zero)
 *                   else  s = fmaxf(fabsf(re), fabsf(im));  a = re / s;  b = im / s;        (IEEE divisions: |a|, |b| <= 1, one is 1)
 *                         n = sqrtf(fmaf(a, a, b * b));  u = a / n + i (b / n)               (n in [1, sqrt 2])
 *               so neither re^2 + im^2 nor its reciprocal can overflow or flush to zero.  A NaN in c gives NaN; so does an
 *               infinity.  The projected bin is S = mag * Re u + i (mag * Im u): one float32 product each.
 *   plain     : (momentum = 0) for i = 0 .. iterations - 1:  c_i = STFT(y_{i-1}) -- for i = 0 the caller's initial spectrum
 *               when one is given (its Im at the bins 0 and n_fft / 2 counts as 0), STFT(y_init) otherwise;
 *               S_i = mag * unit(c_i), which at the bins 0 and n_fft / 2 is mag * sign(Re), sign(0) = 1;
 *               y_i = ISTFT(S_i) over [0, T).  The result is y_{iterations - 1}.
 *   fast      : (0 < momentum < 1)  t_i = c_i + momentum (c_i - c_{i-1}) as fmaf(momentum, c_i - c_{i-1}, c_i) on Re and on Im,
 *               t_0 = c_0;  S_i = mag * unit(t_i).  c_{i-1} is one [R][F][K] complex spectrum in `scratch`; the frame kernel's
 *               epilogue reads and rewrites it at the lane's own bin.  momentum = 0 touches no such buffer, needs no scratch
 *               for it and gives the plain path's bits.
 *   inconsistency : optional device float64 [iterations][2] (may be NULL).  For an iteration that runs a forward transform,
 *               slot 0 = sum (|c_i| - mag)^2 and slot 1 = sum mag^2 over all rows, frames and bins, with
 *               |c_i| = sqrt(Re^2 + Im^2) in float64 on the float32 Re, Im.  Per frame: every lane adds its bins
 *               k = lane, lane + L, .. (L = min(256, n_fft / 8) lanes per frame; bin n_fft / 2 is lane 0's last) in ascending k,
 *               the lanes are added in groups of 8 in ascending lane order, the groups in ascending order; a finishing launch adds
 *               the frames in ascending (r, f).  No atomics, no host sync; the bits do not depend on the grid.  sqrt(slot 0 /
 *               slot 1) is the spectral convergence a caller stops on.  An iteration that starts from a given spectrum writes
 *               NaN into both slots.
 * One launch per block of 256 frames takes a frame from samples to FFT, projection, inverse FFT and windowed frame inside one
 * workgroup's LDS -- the spectrum never reaches memory -- followed by wun_istft's overlap-add kernel.  Iteration i + 1 reads the
 * whole of y_i: the iterations alternate between y and an audio buffer in `scratch`, so no launch reads what it writes (an
 * y_init that overlaps y is first copied into that buffer when iteration 0 would write y).  A frame's floats depend on that
 * frame's samples, its `mag` row and the table alone: not on the frames sharing its workgroup, the block, the grid, what
 * `scratch` held or pointer alignment beyond 4 bytes.  Caller-owned buffers; nothing allocates or synchronises; every check
 * runs before any GPU work.  Both compute modes. */

/* floats of `scratch` for wun_griffin_lim, with R = S B C and nb = min(F, 256 + ceil(n_fft / hop) - 1):
 *   R nb n_fft (the frames of one block) + R T (the second audio buffer) + (momentum_nonzero ? 2 R F K : 0) (c_{i-1})
 *   + 2 n_fft (the float64 window squares) + 4 R F (the frames' float64 partial sums) + 2 (alignment room).
 * Negative wun_status as wun_griffin_lim for the same arguments. */
int64_t wun_griffin_lim_scratch_floats(int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop, int32_t lead,
                                       int64_t F, int32_t momentum_nonzero);
/* y (device [S, B, T, C], every float written) = y_{iterations - 1} from mag (device [R][F][K]) and exactly one start: the
 * spectrum init_re, init_im (device [R][F][K]) or the audio y_init (device [S, B, T, C]; may be y itself).  table_dev is
 * wun_fft_design's table.  Checks and their order as wun_istft_fft (null mag, table_dev, y or scratch; the audio shape; n_fft;
 * hop; lead; F); then WUN_ERR_INVALID for iterations < 1, a momentum outside [0, 1) or not finite, both or neither start
 * given (init_re without init_im, or the reverse, is refused too), y overlapping mag or the initial spectrum. */
int     wun_griffin_lim(const float* mag, const float* init_re, const float* init_im, const float* y_init, int32_t S, int32_t B,
                        int64_t T, int32_t C, int32_t n_fft, int32_t hop, int32_t lead, int64_t F, int32_t iterations,
                        float momentum, const float* table_dev, float* y, double* inconsistency, float* scratch, void* stream);

/* ---- the FFT path of the spectral loss and its gradient ----
 * wun_stft_magnitude, wun_spectral_loss and wun_spectral_loss_terms with both frame transforms of a resolution computed by the
 * FFT of the section above instead of a GEMM, for n_fft a power of two in 64..8192: the loss at the resolutions the filters
 * above run at (4096 / 1024), and about 0.1 MFLOP instead of 8.4 per 2048-point frame.  Every entry takes the arguments of the
 * entry it is named after, in its order, with table_dev / tables_dev[j] = a device copy of wun_fft_design's table of n_fft[j]
 * (3 n_fft floats), and has its contract: the framing without padding (F = 1 + (T - n_fft) / hop, wun_fft_frames), the [R][F][K]
 * layout, the definitions of L_j, of the four terms and of d_outputs, the `losses` slots, the float64 partition and summation
 * order, the caller's buffers, no allocation, no sync, no atomics, any 4-byte alignment, both compute modes.  The checks are the
 * sibling's in its order and with its codes, WUN_ERR_UNSUPPORTED now for an n_fft that is no power of two in 64..8192 (nothing
 * is launched); T < n_fft is WUN_ERR_INVALID as there.
 *   forward  : the section above's forward transform (lead 0); M = sqrtf(fmaf(Re, Re, Im * Im)) as in the GEMM entries, Im of the
 *              bins 0 and n_fft / 2 exactly 0.  One kernel serves the magnitude entry and both losses: the loss's signs are those
 *              of the floats wun_stft_magnitude_fft returns.
 *   gradient : dframe[n] = w[n] sum_{k = 0..n_fft/2} (cre[k] cos(2 pi n k / n_fft) - cim[k] sin(2 pi n k / n_fft)), every bin once:
 *              the inverse transform above on the coefficients with the bins 0 and n_fft / 2 doubled and the scale 1 / 2 in place
 *              of 1 / n_fft (powers of two: exact), the window applied once at the store.  The imaginary coefficients of the bins 0
 *              and n_fft / 2 are not read.  The overlap-add over the frames is wun_spectral_loss's kernel, unchanged.
 * Only the summation order inside a frame transform differs from the GEMM entries: losses and gradients agree with them to
 * float32 rounding, not bit for bit.  A frame's magnitudes and its gradient frame depend on that frame and the table alone --
 * not on the frames sharing its workgroup, the grid, the batch around the row, what `scratch` held or pointer alignment.
 * The scratch formulas are IDENTICAL to the siblings' (the same slices hold the same arrays); the entries differ in the n_fft
 * they accept.  With terms = {1, 0, 0, 0, ..} wun_spectral_loss_terms_fft gives wun_spectral_loss_fft's first 2 + nres losses and
 * d_outputs bit for bit. */
int     wun_stft_magnitude_fft(const float* x, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                               const float* table_dev, float* mags, void* stream);
int64_t wun_spectral_fft_scratch_floats(int32_t S, int32_t B, int64_t Tout, int32_t C, int32_t nres, const int32_t* n_fft,
                                        const int32_t* hop);
int     wun_spectral_loss_fft(const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
                              float mse_weight, int32_t nres, const int32_t* n_fft, const int32_t* hop, const float* weights,
                              const float* const* tables_dev, float* d_outputs, float* losses, float* scratch, void* stream);
int64_t wun_spectral_terms_fft_scratch_floats(int32_t S, int32_t B, int64_t Tout, int32_t C, int32_t nres, const int32_t* n_fft,
                                              const int32_t* hop, const wun_spectral_terms* terms);
int     wun_spectral_loss_terms_fft(const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
                                    float mse_weight, int32_t nres, const int32_t* n_fft, const int32_t* hop, const float* weights,
                                    const wun_spectral_terms* terms, const float* const* tables_dev, float* d_outputs,
                                    float* losses, float* scratch, void* stream);

/* ---- mel-scale terms of the spectral loss ----
 * Two more terms per resolution, on mel spectrograms: the magnitudes of a resolution projected onto n_mels triangular bands.
 *
 * Filterbank.  n_fft a power of two in 64..8192, sample_rate > 0 (Hz), n_mels in 1..512, 0 <= fmin < fmax <= sample_rate / 2
 * (fmax == 0 means sample_rate / 2), norm 0 (none) or 1 (area).  The scale is HTK's: mel(f) = 2595 log10(1 + f / 700).
 * c[0 .. n_mels + 1] are the frequencies of n_mels + 2 points equally spaced in mel from mel(fmin) to mel(fmax); bin k lies at
 * f_k = k sample_rate / n_fft;
 *     W[b][k] = max(0, min((f_k - c[b]) / (c[b+1] - c[b]), (c[b+2] - f_k) / (c[b+2] - c[b+1])))
 * times 2 / (c[b+2] - c[b]) with norm == 1.  All of it in float64 on the host, rounded ONCE to float32.  Of those floats every
 * bin has a positive weight in at most two bands, which are adjacent, and the bins a band weights form one contiguous run.
 * A band whose float32 weights are all 0 (it lies between two bins) would train on nothing: wun_mel_design refuses the whole
 * filterbank with WUN_ERR_INVALID and names the band.
 *
 * Table: 3 K + 2 n_mels 4-byte words, K = n_fft / 2 + 1 (wun_mel_table_floats), int32 and float32 words in one array:
 *   b0[K] int32   bin k has weight w0[k] in band b0[k] and w1[k] in band b0[k] + 1.  b0[k] is the lowest band that weights the
 *                 bin (0 for a bin outside every band); a band index outside 0 .. n_mels - 1 has weight 0, and so has band
 *                 b0[k] + 1 wherever one band alone weights the bin
 *   w0[K], w1[K]  float32
 *   lo[n_mels], hi[n_mels] int32: band b weights exactly the bins lo[b] <= k < hi[b]
 * The caller uploads it, as wun_fft_design's.
 *
 * Projection.  P[m][b] = sum_{k = lo[b]}^{hi[b] - 1} W[b][k] M[m][k]: ONE float32 accumulator started at +0 and one fmaf per
 * bin, k ascending; no atomics.  A band's float depends on that frame's magnitudes and the table alone -- not on the grid, the
 * frames sharing its workgroup, or pointer alignment beyond 4 bytes.  A bin outside [lo[b], hi[b]) is not read for band b.
 * Adjoint.    q[m][k] = fmaf(w1[k], g[m][b0[k] + 1], w0[k] * g[m][b0[k]]), where a band whose weight at k is 0 (or whose index
 * is outside 0 .. n_mels - 1) counts as g = 0 and is not read.  One writer per bin.
 *
 * Terms, per resolution j on Pe and Pt [R][F][n_mels_j], the projections of the floats wun_stft_magnitude[_fft] returns for
 * the estimates and the targets; d = Pe - Pt in fp32, sg = sgn(d), sgn(0) = 0:
 *   mel_l1     : the mean over the R F n_mels values of |d|
 *   log_mel_l1 : the mean of |logf(Pe + log_eps) - logf(Pt + log_eps)|
 *   g[m][b] = mel_l1 weight * sg + log_mel_l1 weight * sg / (Pe + log_eps): the gradient with respect to Pe times R F n_mels.
 * The coefficient of (Re_e, Im_e) / Me at bin (m, k) gains (K / n_mels) q[m][k] of that g -- pre-scaled, so that the
 * resolution's one scale stays weights[j] / (R F K) -- added to the four terms' coefficient before the one division by Me; 0
 * where Me == 0.  L_j = the four terms' weighted sum + mel_l1 weight * mel_l1 + log_mel_l1 weight * log_mel_l1; the total and
 * d_outputs as wun_spectral_loss_terms defines them.  The two means are summed as that entry's: 1024 consecutive elements of
 * [R F][n_mels] per float64 partial, the same tree.  log_eps = 1e-3 is the usual value: a choice, not a measurement. */
int64_t wun_mel_table_floats(int32_t n_fft, int32_t n_mels);
/* Host: the table into table_host[cap] (int32 words stored in place).  WUN_ERR_UNSUPPORTED for the n_fft; then WUN_ERR_INVALID for
 * n_mels outside 1..512, a sample_rate that is not finite and > 0, fmin / fmax outside the range above or not finite, norm not
 * 0 or 1, a null pointer, cap < wun_mel_table_floats, or an empty band. */
int     wun_mel_design(int32_t n_fft, double sample_rate, int32_t n_mels, double fmin, double fmax, int32_t norm,
                       float* table_host, int64_t cap);
/* Single operators on device arrays: out[m][b] = P of mags [M][K]; q[m][k] = the unscaled adjoint of g [M][n_mels].
 * 1 <= M <= 2^30, K = n_fft / 2 + 1 of an n_fft above, n_mels in 1..512 (WUN_ERR_INVALID otherwise, or for a null pointer);
 * mel_table_dev: a device copy of wun_mel_design's table for that K and n_mels.  One launch each, no sync. */
int     wun_op_mel_project(const float* mags, int64_t M, int32_t K, int32_t n_mels, const float* mel_table_dev, float* out,
                           void* stream);
int     wun_op_mel_project_transpose(const float* g, int64_t M, int32_t K, int32_t n_mels, const float* mel_table_dev, float* q,
                                     void* stream);
/* the two term weights (finite, >= 0; a term whose weight is 0 is not computed) and log_eps (finite, > 0) */
typedef struct wun_mel_terms { float mel_l1, log_mel_l1, log_eps; } wun_mel_terms;
int64_t wun_mel_abi_size(void);        /* sizeof(wun_mel_terms) */
/* wun_spectral_loss_terms[_fft] with the mel terms: its arguments in its order and its contract (the caller's buffers, no
 * allocation, no sync, no atomics, every check before any GPU work, d_outputs may be NULL, any 4-byte alignment, bits
 * independent of the grid, the scratch contents, the alignment and repetition), then
 *   mel            : HOST, the weights above
 *   n_mels         : HOST, nres band counts
 *   mel_tables_dev : HOST array of nres device pointers, [j] = wun_mel_design's table for n_fft[j] and n_mels[j]
 * All four weights of `terms` may be 0: the mel terms alone.  The checks are the sibling's in its order; then WUN_ERR_INVALID
 * for a null `mel`, a negative or non-finite mel weight, a log_eps that is not finite and > 0, null n_mels / mel_tables_dev with
 * nres > 0, an n_mels[j] outside 1..512 or a null mel table.
 *   losses : device float32 [2 + 7 nres]: the first 2 + 5 nres as wun_spectral_loss_terms has them (L_j and the total include
 *            the mel terms), then [2 + 5 nres + 2 j] = mel_l1 and [2 + 5 nres + 2 j + 1] = log_mel_l1 of resolution j, unweighted
 *            (0 for a term whose weight is 0)
 *   scratch: wun_spectral_mel[_fft]_scratch_floats floats: wun_spectral_terms[_fft]_scratch_floats' and, where a mel weight is
 *            > 0, per resolution 2 R F n_mels floats (Pe, which g replaces in place, and Pt) and one float64 partial (2 floats)
 *            per 1024 mel values for each mel term in use
 * With both mel weights 0 nothing mel is launched: the first 2 + 5 nres losses and d_outputs are wun_spectral_loss_terms[_fft]'s
 * bit for bit, and the mel slots are 0. */
int64_t wun_spectral_mel_scratch_floats(int32_t S, int32_t B, int64_t Tout, int32_t C, int32_t nres, const int32_t* n_fft,
                                        const int32_t* hop, const wun_spectral_terms* terms, const wun_mel_terms* mel,
                                        const int32_t* n_mels);
int     wun_spectral_loss_mel(const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
                              float mse_weight, int32_t nres, const int32_t* n_fft, const int32_t* hop, const float* weights,
                              const wun_spectral_terms* terms, const float* const* tables_dev, float* d_outputs, float* losses,
                              float* scratch, void* stream, const wun_mel_terms* mel, const int32_t* n_mels,
                              const float* const* mel_tables_dev);
int64_t wun_spectral_mel_fft_scratch_floats(int32_t S, int32_t B, int64_t Tout, int32_t C, int32_t nres, const int32_t* n_fft,
                                            const int32_t* hop, const wun_spectral_terms* terms, const wun_mel_terms* mel,
                                            const int32_t* n_mels);
int     wun_spectral_loss_mel_fft(const float* outputs, const float* targets, int32_t S, int32_t B, int64_t Tout, int32_t C,
                                  float mse_weight, int32_t nres, const int32_t* n_fft, const int32_t* hop, const float* weights,
                                  const wun_spectral_terms* terms, const float* const* tables_dev, float* d_outputs,
                                  float* losses, float* scratch, void* stream, const wun_mel_terms* mel, const int32_t* n_mels,
                                  const float* const* mel_tables_dev);

/* ---- whole-track separation (Evaluate.predict_track, Evaluate.py:113-143) ------------------
 * The hop loop of the reference around get_output, on the device: hop windows are read straight from the zero-padded
 * track and the estimates are written straight into the track-long result.  Audio is float32 channel-last: the track is
 * [track_frames, C], the result [S, pred_frames, C], C = num_channels of the plan.  Every buffer is the caller's; nothing
 * allocates device memory or synchronises, and every argument check runs before any GPU work. */

/* The hop table of Evaluate.py:125-128: hops at 0, Tout, 2 Tout, ... with the last one re-aligned to n_frames - Tout.
 * Returns the number of hops, ceil(n_frames / output_frames), and writes them to positions[cap] (NULL: count only).
 * WUN_ERR_INVALID for output_frames < 1, n_frames < output_frames or a cap below the count. */
int64_t wun_separate_positions(int64_t output_frames, int64_t n_frames, int64_t* positions, int64_t cap);

/* wun_forward, with row b of the mix read from a track: row b < npos is track_tc[positions[b] .. positions[b] + Tin)
 * (frames), rows npos .. batch - 1 are zeros (a short last chunk needs no second plan).
 *   track_tc  : device, [track_frames, C]
 *   positions : HOST, npos window starts in frames (copied into the launch; free to reuse after the call returns)
 * Everything else as wun_forward.  One gather kernel replaces wun_forward's layout pass and writes the same floats to
 * the same workspace elements; the rest of the forward is the same launch sequence, so outputs row b is bit-identical to
 * wun_forward on the materialised [batch, Tin, C] batch.  positions[b] * C need not be 16-byte aligned.
 * WUN_ERR_INVALID for a null pointer, npos < 1, npos > batch, a window outside [0, track_frames], a track that is not
 * 4-byte or a workspace that is not 16-byte aligned. */
int wun_forward_windows(const wun_plan* plan, const float* params, const float* track_tc, int64_t track_frames,
                        const int64_t* positions, int64_t npos, float* workspace, float* outputs, int training,
                        void* stream);

/* preds[s][positions[b] + t][c] = outputs[s][b][t][c] for b < npos, hops taken in index order: where windows overlap the
 * HIGHEST-indexed one wins (Evaluate.py:139 with the re-aligned last hop written last).  Destination-driven: the host cuts
 * the windows into disjoint runs of frames, one writer per float -- no race, no atomics, deterministic.  Frames no window
 * covers are not written.
 *   outputs   : device, [S, batch, Tout, C] (what the forward wrote)
 *   positions : HOST, npos window starts in frames of preds
 *   preds     : device, [S, pred_frames, C]
 * WUN_ERR_INVALID for a null pointer, npos < 1, npos > batch, a window outside [0, pred_frames]. */
int wun_scatter_windows(const wun_plan* plan, const float* outputs, const int64_t* positions, int64_t npos,
                        float* preds, int64_t pred_frames, void* stream);

/* The whole loop: hops of wun_separate_positions(Tout, n_frames) in chunks of the plan's batch, each chunk
 * wun_forward_windows(training = 0) then wun_scatter_windows, all on `stream` (chunk k + 1 reuses workspace and outputs
 * behind the scatter of chunk k: stream order is the only ordering needed).
 *   track_tc  : device, [n_frames + 2 pad, C], pad = (Tin - Tout) / 2: the track with `pad` zero frames on both sides
 *               (Evaluate.py:121-122; wun_resample with y_offset = pad into a zeroed buffer produces exactly this)
 *   preds     : device, [S, n_frames, C]; every frame is written
 * WUN_ERR_INVALID for a null pointer, n_frames < Tout (pad short tracks with zeros behind, Evaluate.py:108-113) or an odd
 * Tin - Tout.  A plan with a longer Tin / Tout (wun_get_padding on a multiple of the hop, or on the whole track) pays the
 * context Tin - Tout once per hop instead of once per default hop: see DESIGN.md 5.8 for what that changes. */
int wun_separate_track(const wun_plan* plan, const float* params, const float* track_tc, int64_t n_frames,
                       float* workspace, float* outputs, float* preds, void* stream);

/* ---- blended separation: overlapping hops and shifted passes ---------------
 * Every frame of the result is a weighted mean over every window that covers it, taken in one fixed order.
 * Geometry: Tout = the hop's output frames, V = overlap_frames (0 <= V <= Tout - 1), H = Tout - V the stride.  A pass with
 * shift s >= 0 has windows at p_k = k H - s, k = 0 .. K - 1, K = 1 + ceil(max(0, n_frames + s - Tout) / H): the last window
 * is not re-aligned, it hangs over the end of the track.  The window list of a separation is its passes one behind the other
 * in the order of the shifts, windows inside a pass in order of k; g is the index in that list.
 * Weight of frame t of a window, a float32 trapezoid:  w[t] = (float)min(t + 1, Tout - t, V + 1) / (float)(V + 1), one
 * correctly rounded division, without the t + 1 term for a window flagged WUN_BLEND_NO_RISE (the first of a pass) and without
 * the Tout - t term for one flagged WUN_BLEND_NO_FALL (the last): the weight is 1 there.
 * Result, for every frame f, source s and channel c:  acc = den = +0 (float32);  for g ascending over the windows covering f:
 * acc = fmaf(w_g, x_g, acc), den = den + w_g;  pred = acc / den (correctly rounded), +0 where nothing covers f.
 * acc and den live in `preds` and `den` as float32 between calls, so a frame's chain is the same numbers however the window
 * list is cut into calls, batches or launches: the result's bits do not depend on it.  Averaging over shifts is this mean over
 * the union of the passes' windows, not a mean of per-pass results.  (A frame that a single weight-1 window covers keeps that
 * window's value: fmaf(1, x, +0) / 1 == x, with -0 becoming +0.) */
typedef struct wun_blend_window {     /* 16 bytes */
    int64_t pos;     /* first frame of the window in preds; may be negative or beyond pred_frames (clipped) */
    int32_t row;     /* row of `outputs` that holds the window's Tout frames */
    int32_t flags;   /* WUN_BLEND_NO_RISE | WUN_BLEND_NO_FALL */
} wun_blend_window;
#define WUN_BLEND_NO_RISE 1
#define WUN_BLEND_NO_FALL 2
int32_t wun_blend_abi_size(void);     /* sizeof(wun_blend_window) */

/* One pass's table: windows[k] = {k H - shift, row = k, NO_RISE for k == 0 | NO_FALL for k == K - 1} (the caller renumbers the
 * rows per chunk).  Returns K and writes windows[cap] (NULL: count only).  Host only.  WUN_ERR_INVALID for output_frames < 1,
 * n_frames < 1, overlap_frames outside [0, output_frames - 1], shift < 0 or a cap below K. */
int64_t wun_blend_positions(int64_t output_frames, int64_t n_frames, int64_t overlap_frames, int64_t shift,
                            wun_blend_window* windows, int64_t cap);

/* The accumulation above for the windows of one table, in table order (the caller's ascending g), into preds (acc) and den,
 * which the caller zeroed before the first call of a separation.  Independent of any plan.  Destination-driven: the host cuts
 * the windows, clipped to [0, pred_frames), into runs of frames whose covering set is constant; one lane owns one 16-byte
 * granule of preds and walks the run's covering rows -- one writer per float per launch, no atomics.  A covering set larger
 * than 4 rows continues in the next launch on `stream`.
 *   outputs : device, [S, B, Tout, C];  windows : HOST, nwin entries (copied into the launches);  C is 1 or 2
 *   preds   : device, [S, pred_frames, C];  den : device, [pred_frames]
 * WUN_ERR_INVALID for a null pointer, a size out of range, a row outside [0, B), unknown flag bits, overlap_frames outside
 * [0, Tout - 1] or a pointer that is not 4-byte aligned. */
int wun_blend_windows(const float* outputs, int64_t S, int64_t B, int64_t Tout, int64_t C, const wun_blend_window* windows,
                      int64_t nwin, int64_t overlap_frames, float* preds, float* den, int64_t pred_frames, void* stream);

/* preds[s][f][c] = den[f] != 0 ? preds[s][f][c] / den[f] : +0, in place. */
int wun_blend_finish(float* preds, const float* den, int64_t S, int64_t pred_frames, int64_t C, void* stream);

/* The whole loop: preds and den zeroed (hipMemsetAsync), the window list of `shifts` walked in chunks of the plan's batch
 * (chunks run across pass boundaries, a short last chunk runs as zero rows), per chunk the forward pass on windows read from
 * the track (training = 0) then wun_blend_windows, at the end wun_blend_finish; all on `stream`.
 *   track_tc : device, [track_frames, C]: lead + pad zero frames, the track, zeros; pad = (Tin - Tout) / 2.  The window at
 *              pred position p reads track_tc[lead + p .. lead + p + Tin)
 *   shifts   : HOST, nshifts frame offsets >= 0
 *   preds    : device, [S, n_frames, C]; den : device, [n_frames]; every frame is covered
 * WUN_ERR_INVALID for a null pointer, an odd Tin - Tout, a bad size, a misaligned pointer, or a window of a pass outside
 * [0, track_frames] (lead >= every shift, and enough zeros behind for the overhanging last hop); the message names it. */
int wun_separate_track_blend(const wun_plan* plan, const float* params, const float* track_tc, int64_t track_frames,
                             int64_t lead, int64_t n_frames, int64_t overlap_frames, const int64_t* shifts, int64_t nshifts,
                             float* workspace, float* outputs, float* preds, float* den, void* stream);

/* ---- training batches from resident tracks (Datasets.py:29-34, Utils.py:26-42) --------------
 * One batch of the reference's snippet pipeline, and the source-level augmentations around it, in one kernel: the sources of
 * a data set live on the device as S planes [plane_frames, C] (the zero-padded tracks one behind the other) and, with
 * mix_mode 0, a mix plane of the same shape.  Row b of the batch reads the window of Tin frames at desc[b][s].start of
 * plane s:
 *   a_s[t][c]        = gain_s * x_s[start_s + t][c']     c' = the other channel with flag bit 0, sign flipped with bit 1
 *   targets[s][b]    = a_s[pad .. pad + Tout),           pad = (Tin - Tout) / 2 (Utils.crop_sample)
 *   mix[b]           = ((a_0 + a_1) + a_2) + ...         mix_mode 1 (Utils.random_amplify's re-summed mix)
 *                    = mix_plane[start_0 .. start_0 + Tin)   mix_mode 0 (the targets still get their gains and flags)
 * The product is one float32 multiplication rounded on its own and every addition is rounded (no fused multiply-add), so the
 * batch is bit-identical to the host pipeline's; with gain == 1.0f a source's bits pass through unchanged (negative zero,
 * denormals and NaN payloads included).  Sources of one row may start at different frames (independent remix).
 * Every buffer is the caller's; nothing allocates device memory, copies from the host or synchronises: the descriptor
 * table travels by value in the kernel arguments, WUN_SNIPPET_ROWS rows per launch (a larger batch is several launches on
 * `stream`).  Every argument check runs before any GPU work.  Nothing outside a window is read; a window may start at any
 * frame (no alignment beyond a float's). */
typedef struct wun_snippet_source {   /* one source of one batch row; 16 bytes */
    int64_t  start;   /* first frame of the window inside that source's plane */
    float    gain;    /* multiplies every sample */
    uint32_t flags;   /* bit 0: swap the two channels (C == 2 only); bit 1: negate */
} wun_snippet_source;
#define WUN_SNIPPET_SWAP 1u
#define WUN_SNIPPET_NEGATE 2u
#define WUN_SNIPPET_ROWS 24           /* batch rows per launch: 24 rows x 8 sources x 16 bytes = 3 KB of kernel arguments */
int32_t wun_snippet_abi_size(void);   /* sizeof(wun_snippet_source) */

/*   planes      : HOST array of S device pointers, each [plane_frames, C]
 *   mix_plane   : device [plane_frames, C], or NULL with mix_mode 1
 *   desc        : HOST, [B][S] (copied into the launches; free to reuse after the call returns)
 *   mix_out     : device [B, Tin, C];  targets_out : device [S, B, Tout, C]
 * WUN_ERR_INVALID for a null required pointer (mix_plane with mix_mode 0 included), mix_mode outside {0, 1}, C outside
 * {1, 2}, the swap flag with C == 1, S outside 1..8, B < 1, Tout > Tin, an odd Tin - Tout, Tout < 1, a window outside
 * [0, plane_frames], unknown flag bits, a plane or an output that is not 4-byte aligned. */
int wun_gather_snippets(const float* const* planes, const float* mix_plane, int64_t plane_frames, int32_t C, int32_t S,
                        int32_t B, int64_t Tin, int64_t Tout, const wun_snippet_source* desc, int32_t mix_mode,
                        float* mix_out, float* targets_out, void* stream);

/* Speed perturbation (pitch and tempo together) inside the gather: a source of a row may be played at speed
 * down / up, its window of Tin frames resampled while it is read from n_src = wun_speed_source_frames(Tin, up, down) frames
 * of its plane.  The ratios come from a bank of up to WUN_SPEED_RATES entries, each with a device copy of
 * wun_resample_design(up, down)'s phase-major table (K = ceil((2 half + 1) / up), half = 10 max(up, down)).  rate[b][s] = 0 is
 * the unit rate, exactly wun_gather_snippets' path and bits; i >= 1 selects bank entry i - 1:
 *   v[m][c]   = x_s[start_s + m][c']   for 0 <= m < n_src, +0 outside   (c' = the other channel with flag bit 0)
 *   u = t down + half;  q = u / up;  p = u % up
 *   r_s[t][c] = acc after  acc = fmaf(table[p K + k], v[q - k][c], acc)  for k = 0, 1, .., K - 1;  acc starts at +0
 *   a_s[t][c] = gain_s * r_s[t][c]     (one rounded product, skipped when gain == 1.0f), sign flipped with flag bit 1
 * which is bit for bit wun_resample(plane_s + start_s C, n_src, C, .., y_offset 0, n_out Tin, C, table, up, down) followed by the
 * gain, swap and sign above.  Targets and mix as for wun_gather_snippets; nothing outside [start_s, start_s + n_src) is read.
 * A rated source needs mix_mode 1 (with mix_mode 0 the mix plane would have to be resampled too). */
#define WUN_SPEED_RATES 8             /* entries of a rate bank */
#define WUN_SPEED_MAX_RATIO 64        /* ceiling on max(up, down) of an entry; and 1/2 <= down / up <= 2 */
typedef struct wun_speed_bank {
    int32_t      n;                        /* entries in use, 0..WUN_SPEED_RATES */
    int32_t      up[WUN_SPEED_RATES];      /* positive, coprime with down, not 1/1 */
    int32_t      down[WUN_SPEED_RATES];
    const float* table[WUN_SPEED_RATES];   /* device: wun_resample_design(up, down)'s table, wun_resample_table_floats floats */
} wun_speed_bank;
int32_t wun_speed_abi_size(void);     /* sizeof(wun_speed_bank) */
/* ((Tin - 1) down) / up + 1: the smallest n with wun_resample_frames(n, up, down) >= Tin.  Host only.  WUN_ERR_INVALID for
 * Tin < 1 (or above 2^40) or a ratio that is not positive and coprime or is 1/1; WUN_ERR_UNSUPPORTED above the ceiling or
 * outside [1/2, 2]. */
int64_t wun_speed_source_frames(int64_t Tin, int32_t up, int32_t down);
/*   rate : HOST uint8 [B][S], NULL = all unit;  bank : HOST, may be NULL when rate is NULL or all zero
 * With all rates unit: wun_gather_snippets' bits in both mix modes.  WUN_ERR_INVALID for everything wun_gather_snippets refuses,
 * a rate index above bank->n, a non-zero rate with a null bank or with mix_mode 0, bank->n outside 0..8, a ratio that is not
 * positive and coprime or is 1/1, a table that is null or not 4-byte aligned, a rated window with start < 0 or start + n_src >
 * plane_frames (unit windows keep the rule with Tin); WUN_ERR_UNSUPPORTED for a ratio above the ceiling or outside [1/2, 2].
 * Every check runs before any GPU work.  WUN_SNIPPET_ROWS rows per launch, no intermediate, no atomics, no copy. */
int wun_gather_snippets_speed(const float* const* planes, const float* mix_plane, int64_t plane_frames, int32_t C, int32_t S,
                              int32_t B, int64_t Tin, int64_t Tout, const wun_snippet_source* desc, const uint8_t* rate,
                              const wun_speed_bank* bank, int32_t mix_mode, float* mix_out, float* targets_out, void* stream);

/* ---- phase vocoder: time stretch at constant pitch --------------------------
 * A job stretches one span of interleaved audio x[n_in][C] into y[n_out][C] at the tempo ratio num / den (above 1 plays faster:
 * the output is shorter).  With pitch_shift = a stretch followed by wun_resample at the same ratio, the two augmentations that
 * wun_gather_snippets_speed does not have: tempo without pitch and pitch without tempo.  Jobs are independent and batched: the
 * table travels by value in the kernel arguments, WUN_STRETCH_JOBS jobs per launch set of four launches (a longer table is
 * several sets on `stream`).
 *
 * With N = n_fft, h = hop, K = N / 2 + 1, w the periodic Hann window of wun_fft_design, lead = N - h, every channel on its own and
 * F = wun_fft_centered_frames(n_out, N, h), for f = 0 .. F - 1:
 *   a_f      = (f h num) / den                                   (64-bit integers, floor)
 *   X_f      = the forward FFT of wun_stft_complex_fft, bit for bit, of w[n] x[a_f - lead + n];  P_f the same at a_f - h - lead;
 *              samples outside [0, n_in) read as +0 and nothing outside the span is read
 *   M_f[k]   = sqrtf(fmaf(Re, Re, Im Im)) of X_f[k]
 *   q        = X_f[k] conj(P_f[k]) in float64 (the four products are exact, each sum is rounded once)
 *   ang      = atan2(q_im, q_re) / 2 pi, 0 where q_re == 0 and q_im == 0 (either sign of zero);  adv = ((k h) mod N) / N
 *   D_f[k]   = (float)(d - rint(d)),  d = ang - adv;     D_0[k] = (float)(atan2(Im X_0, Re X_0) / 2 pi), the same zero rule
 *   Phi_0    = D_0;   Phi_f = Phi_{f-1} + (adv + D_f)             (float64, ascending f per channel and bin)
 *   Y_f[k]   = (M_f (float)cos(2 pi Phi_f), M_f (float)sin(2 pi Phi_f)), one float32 product each; Im of the bins 0 and N / 2 is 0
 *   y        = wun_istft_fft's inverse transform of Y_f, windowed, overlap-added at f h - lead and divided by the float64
 *              window squares of the covering frames (0 where those sum to less than 1e-8), over [0, n_out)
 * Every float of y[0 .. n_out C) is written and nothing else.  At 1/1, P_f is X_{f-1} bit for bit and the entry is STFT -> ISTFT up
 * to the float32 rounding of D.  A job's floats depend on its span, its ratio, N, h and the table -- not on the other jobs, its
 * place in the table, the launch set, the grid, what `scratch` held or pointer alignment. */
#define WUN_STRETCH_JOBS 64            /* jobs per launch set; more jobs = more launch sets on the same stream */
typedef struct wun_stretch_job {       /* 32 bytes */
    const float* x;                    /* device, [n_in][C]; any 4-byte alignment */
    float*       y;                    /* device, [n_out][C]; any 4-byte alignment */
    int32_t      n_in, n_out, num, den;
} wun_stretch_job;
int32_t wun_stretch_abi_size(void);    /* sizeof(wun_stretch_job) */
/* ceil(n_in den / num): the longest n_out of a job.  Host only.  WUN_ERR_INVALID for n_in < 1 (or above 2^40) or a ratio that is
 * not positive and coprime; WUN_ERR_UNSUPPORTED for max(num, den) > 64 or a ratio outside [1/2, 2].  1/1 is legal. */
int64_t wun_time_stretch_frames(int64_t n_in, int32_t num, int32_t den);
/* Floats of `scratch` for this table: rows (2 K + N) of the largest launch set, rows = C times the sum of its jobs' F (only n_out
 * of a job is read).  Errors as wun_time_stretch's for jobs, J, C, n_fft, hop and n_out < 1. */
int64_t wun_time_stretch_scratch_floats(const wun_stretch_job* jobs, int32_t J, int32_t C, int32_t n_fft, int32_t hop);
/*   jobs      : HOST, [J] (copied into the launches; free to reuse after the call returns)
 *   table_dev : device, wun_fft_design(n_fft)'s table;  scratch : device, wun_time_stretch_scratch_floats floats
 * WUN_ERR_INVALID for a null pointer, J < 1, C outside {1, 2}, a hop that is not a power of two or is above n_fft / 4, and per job
 * n_in < 1, n_out < 1 or above wun_time_stretch_frames, a ratio that is not positive and coprime, a pointer that is not 4-byte
 * aligned, a y that overlaps the x of any job;  WUN_ERR_UNSUPPORTED for an n_fft that is not a power of two in 64..8192, a ratio
 * above the ceiling of 64 or outside [1/2, 2], more than 2^31 - 1 frame rows in a launch set.  Every check runs before any GPU
 * work.  No allocation, no synchronisation, no atomics; both compute modes. */
int wun_time_stretch(const wun_stretch_job* jobs, int32_t J, int32_t C, int32_t n_fft, int32_t hop, const float* table_dev,
                     float* scratch, void* stream);

/* ---- the spectrogram U-Net baseline, inference only ------------------------
 * The reference's other separator (Models/UnetSpectrogramSeparator.py:40-108, configs unet_spectrogram / unet_spectrogram_l1)
 * at training = False: per source one U-Net of 5 x 5 stride-2 convolutions over log1p of the mixture's STFT magnitude, whose
 * sigmoid mask multiplies the mixture's spectrogram.  Mono, channel-last: activations are [B, F, n_fft / 2, C] (TF's NHWC).
 *   X = STFT(mix[b, :, 0]) in the spectral section's framing without padding (F = 1 + (T - n_fft) / hop frames, K = n_fft / 2 + 1
 *   bins, periodic Hann; computed by the FFT of wun_stft_complex_fft);  M = |X|;  A0[b][f][k] = log1p(M[b][f][k]) for k < K - 1.
 *   down i = 0..L-1 : conv 5 x 5 stride 2, "same" = 1 before and 2 after (out[y][x] = sum A[2y + ky - 1][2x + kx - 1][ci]
 *                     W[ky][kx][ci][co], zeros outside) to nif 2^i channels, + bias, batch norm, LeakyReLU(0.2); levels i < L - 1
 *                     are kept as skips
 *   up i = 0..L-2   : transposed conv 5 x 5 stride 2 "same" (the gradient of the conv above: out[t] = sum over 2 j + k - 1 == t of
 *                     A[j] W[k] per axis, t in [0, 2 N)) to nif 2^(L-i-2) channels, + bias, batch norm, ReLU; then the channel
 *                     concatenation [skip_{L-2-i}, that], skip first
 *   mask            : sigmoid(transposed conv to 1 channel + bias); the dropped bin K - 1 gets 0.5
 *   batch norm      : (z - moving_mean) / sqrt(moving_variance + 1e-3) + beta -- no gamma
 *   mags[s] = M mask_s, [S][B][F][K];  audio[s] = ISTFT_tf(mask_s X), [S][B][T][1] (wun_istft_tf_fft below)
 * Shape conditions (else WUN_ERR_INVALID, before any GPU work): T == (F - 1) hop + n_fft, F and n_fft / 2 multiples of 2^L.
 * The convolutions run on the exact-fp32 MFMA (the first down layer and the mask layer, thin GEMMs, on the VALU with the same
 * bits), the reduction in ascending (ky, kx, ci) order in one accumulator per output, no atomics: an excerpt's bits do not depend
 * on the batch around it, the grid, what the workspace held or pointer alignment beyond 4 bytes.  Every buffer is the caller's;
 * nothing allocates or synchronises; every argument check runs before any GPU work.  Training on the magnitude objective is the
 * next section; the raw-audio objective, stereo and a bf16 mode are not built. */
typedef struct wun_spec_config {
    int32_t num_layers;          /* L in 1..10 */
    int32_t num_initial_filters; /* nif; nif 2^(L-1) <= 65536 */
    int32_t num_sources;         /* 1..8 (the reference asserts 2, UnetSpectrogramSeparator.py:24) */
    int32_t n_fft;               /* a power of two in 64..8192 (the reference: 1024) */
    int32_t hop;                 /* 1..n_fft (the reference: 768) */
} wun_spec_config;
/* sizeof(wun_spec_config) as the library was compiled (wun_abi_sizes keeps its three entries). */
int64_t wun_spec_abi_size(void);
/* The variable table: tf.layers / tf.contrib.layers names in graph-construction order inside scope "separator", an index 0
 * without suffix; for source s: conv2d_{s L + i}/kernel [5, 5, Cin, Cout] and /bias, BatchNorm_{s (2L - 1) + j}/beta,
 * /moving_mean, /moving_variance (j = i on the down path, L + i on the up path), conv2d_transpose_{s L + i}/kernel
 * [5, 5, Cout, Cin] and /bias (i = L - 1: the mask layer).  Offsets are floats into one flat params buffer of
 * wun_spec_param_floats floats, packed in table order.  Negative wun_status for a bad config or index. */
int64_t wun_spec_num_tensors(const wun_spec_config* cfg);
int64_t wun_spec_param_floats(const wun_spec_config* cfg);
int     wun_spec_tensor(const wun_spec_config* cfg, int64_t index, wun_tensor_info* info);
/* F for T samples, or WUN_ERR_INVALID where the shape conditions fail; host only. */
int64_t wun_spec_frames(const wun_spec_config* cfg, int64_t T);
/* floats of `workspace` for wun_spec_forward: X, M, A0, the activations of one source's network, the mask, the masked spectra of
 * all sources and wun_istft_tf_fft's scratch.  Negative wun_status as wun_spec_forward for the same arguments. */
int64_t wun_spec_workspace_floats(const wun_spec_config* cfg, int32_t B, int64_t T);
/*   params    : device, wun_spec_param_floats floats
 *   mix       : device, [B, T, 1]
 *   table_dev : device copy of wun_fft_design's table of n_fft (3 n_fft floats)
 *   audio     : device [S, B, T, 1] or NULL;  mags : device [S, B, F, K] or NULL (return_spectrogram); at least one
 * WUN_ERR_INVALID for a null pointer, both outputs null, the shape conditions, B < 1 or a workspace that overlaps another
 * buffer; WUN_ERR_UNSUPPORTED for an n_fft outside the list, sizes beyond the limits above, or a resolution wun_istft_tf_fft refuses. */
int     wun_spec_forward(const wun_spec_config* cfg, const float* params, const float* mix, int32_t B, int64_t T,
                         const float* table_dev, float* audio, float* mags, float* workspace, void* stream);

/* ---- training the spectrogram U-Net: the magnitude objective ------------------
 * One step of UnetSpectrogramSeparator.py:63-92 at training = True with Jansson's L1 on magnitudes (Training.py:55-63,
 * raw_audio_loss = False) and TF-Adam with the batch-norm UPDATE_OPS (Training.py:74-77).  float32, mono.
 *   forward   every layer with a batch norm: z = conv + bias; per channel over the n = B H W pixels of the layer's output
 *             mu = mean z, var = mean (z - mu)^2 (biased, two passes, float64 sums); zhat = (z - mu) / sqrt(var + 1e-3) + beta,
 *             then the activation.  The mask layer has no batch norm.
 *   dropout   on the concatenation [skip, up] of up levels i < 3 (the input of transposed layer i + 1): element e (the flat
 *             index into [B][H][W][c_skip + c_up]) is multiplied by 1 / (1 - rate) if kept and by 0 otherwise.  The keep bit is
 *             stateless and counter-based.  With uint64 arithmetic modulo 2^64 and
 *               mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) 0x94D049BB133111EB;
 *                       return z ^ z >> 31
 *               key = mix(mix(mix(seed) + step) + (source << 8 | level))
 *               u   = mix(key + e) >> 40                                  (24 bits)
 *             element e is kept iff u 2^-24 >= rate (compared in float32).  rate = 0 disables dropout and its buffers.
 *   loss      R_s = |STFT(target_s)| (wun_stft_magnitude_fft);  losses[1 + s] = mean over all B F K bins of |R_s - M mask_s|,
 *             losses[0] = their mean over the sources.  The padded bin K - 1 (mask 0.5) adds to the loss and to no gradient.
 *             1024 consecutive bins per float64 partial, as wun_spectral_loss sums.
 *   backward  dmask = -sign(R - M mask) M / (S B F K), sign(0) = 0;  ReLU passes where zhat > 0, LeakyReLU has slope 1 where
 *             zhat > 0 and 0.2 elsewhere;  batch norm: dbeta = sum g, dz = rstd (g - mean g - xh mean(g xh));  the conv biases
 *             under a batch norm get sum dz (mathematically zero, computed all the same, as TF does).
 *             Weight gradients: split reductions over chunks of 256 pixels of the small map, the partition a function of the
 *             shapes alone, the chunks added in ascending order (see wun_op_conv2d_s2_wgrad).  No atomics.
 *   Adam      wun_adam_step's rule on kernels, biases and betas; then moving_mean -= (1 - decay) (moving_mean - mu) and
 *             moving_variance -= (1 - decay) (moving_variance - var n / max(n - 1, 1)) from the statistics of the last forward.
 *             grads, m and v of the moving statistics stay 0.
 * Contract as wun_spec_forward: the caller's buffers, no allocation, no sync, every check before any GPU work, a workspace that
 * overlaps another buffer is refused; the bits depend on neither the grid, what the workspace held nor pointer alignment beyond
 * 4 bytes.  The three entries of one step take the same (cfg, tcfg, B, T) and the same workspace, in this order. */
typedef struct wun_spec_train_config {
    float   bn_decay;            /* in [0, 1]; tf.contrib.layers.batch_norm: 0.999 */
    float   dropout_rate;        /* in [0, 1); tf.layers.dropout: 0.5; 0 = none */
    int64_t dropout_seed;
} wun_spec_train_config;
/* sizeof(wun_spec_train_config) as the library was compiled. */
int64_t wun_spec_train_abi_size(void);
/* floats of the training workspace: X, M, A0, R, and per source every layer's z, batch mean, batch variance and activation, the
 * dropout masks and dropped concatenations of up levels i < 3 and the mask; the gradient buffers of the backward pass, the
 * weight-gradient partials and the float64 partial sums.  Negative wun_status as wun_spec_train_forward. */
int64_t wun_spec_train_workspace_floats(const wun_spec_config* cfg, int32_t B, int64_t T);
/* Where a retained tensor of the last wun_spec_train_forward lies in the workspace: *offset floats from its base, *count floats
 * (the role of wun_plan_activation).  layer: 0 .. L-1 the down path, L .. 2L-2 the up path; WUN_SPEC_TT_ACT also takes 2L-1, the
 * sigmoid mask [B][F][K - 1]; WUN_SPEC_TT_DROPOUT takes the up level i in 0 .. L-2 and gives count 0 for i >= 3 (the mask holds
 * the multipliers 0 and 1 / (1 - rate), and is not written when rate = 0).  Host only. */
enum { WUN_SPEC_TT_Z = 0, WUN_SPEC_TT_MEAN = 1, WUN_SPEC_TT_VAR = 2, WUN_SPEC_TT_ACT = 3, WUN_SPEC_TT_DROPOUT = 4 };
int     wun_spec_train_tensor(const wun_spec_config* cfg, int32_t B, int64_t T, int32_t kind, int32_t source, int32_t layer,
                              int64_t* offset, int64_t* count);
/*   step : the counter of the dropout keep bit (>= 0);  mags : device [S, B, F, K], required
 * WUN_ERR_INVALID also for a bn_decay outside [0, 1] or a dropout_rate outside [0, 1) (NaN included). */
int     wun_spec_train_forward(const wun_spec_config* cfg, const wun_spec_train_config* tcfg, const float* params,
                               const float* mix, int32_t B, int64_t T, const float* table_dev, int64_t step, float* mags,
                               float* workspace, void* stream);
/*   targets : device [S, B, T, 1];  grads : device, wun_spec_param_floats floats, every float written;  losses : device [1 + S]
 * Reads what wun_spec_train_forward left in the workspace. */
int     wun_spec_loss_backward(const wun_spec_config* cfg, const wun_spec_train_config* tcfg, const float* params,
                               const float* targets, int32_t B, int64_t T, const float* table_dev, float* grads, float* losses,
                               float* workspace, void* stream);
/* step is 1-based (lr_t = lr sqrt(1 - beta2^step) / (1 - beta1^step)); the workspace is read only (the batch statistics). */
int     wun_spec_adam_step(const wun_spec_config* cfg, const wun_spec_train_config* tcfg, float* params, const float* grads,
                           float* m, float* v, const float* workspace, int32_t B, int64_t T, int64_t step, float lr, float beta1,
                           float beta2, float eps, float grad_scale, void* stream);

/* ---- the spectrogram U-Net: backward from any loss, on magnitudes or audio ------
 * The training forward's two outputs are mags_s = M mask_s [S][B][F][K] and audio_s = ISTFT_tf(mask_s X) [S][B][T][1]; these entries
 * give the second one and the backward pass from an upstream gradient on either or both, in place of the objective compiled into
 * wun_spec_loss_backward.  All of them read what the last wun_spec_train_forward on that workspace retained (X, M, the masks, every
 * z, activation, batch mean and variance, the dropout masks) and leave it unchanged; they take that call's (cfg, tcfg, B, T).
 *   adjoint of ISTFT_tf   u[t] = d_audio[t] / D[t mod hop], D[p] = sum_i w^2[p + i hop] in float64 (i ascending, the squares as
 *                         wun_istft_tf_fft forms them) ROUNDED ONCE to float32: the kernel DIVIDES by the rounded D, as the forward
 *                         does, and does not multiply by a reciprocal.  G = STFT(u) in the forward's framing, window and FFT;
 *                         ga[k] = c_k fmaf(Re X[k], Re G[k], Im X[k] Im G[k]), c_0 = 1 / n_fft, c_k = 2 / n_fft for 0 < k < K - 1.
 *                         G is never stored: the gradient is the FFT kernel's epilogue.
 *   head, k < K - 1       d_mags alone: dmask = d_mags M;  d_audio alone: dmask = ga;  both: dmask = fmaf(d_mags, M, ga);
 *                         dz = dmask * (mask * (1 - mask)).  Bin K - 1 (mask 0.5) receives no gradient from either domain.
 *                         With d_mags = -sign(R - M mask) / (S B F K) in float32 the gradients are wun_spec_loss_backward's bits.
 *   body                  the backward of the previous section from dz on: same launches, order and arithmetic.  grads gets
 *                         every float written; the moving statistics' slots are 0.
 * The gradient with respect to the mix is not built.  Contract as the previous section: the caller's buffers, no allocation, no
 * sync, every check before any GPU work, no atomics; the bits depend on neither the grid, what the scratch held nor pointer
 * alignment beyond 4 bytes.  The backward entries may be called any number of times after one forward, in any order with
 * wun_spec_loss_backward: each call gives the bits of the first.
 * WUN_ERR_INVALID for a null pointer, both gradients null, the shape conditions, a bad tcfg, or a workspace, scratch or gradient
 * buffer that overlaps another buffer; WUN_ERR_UNSUPPORTED for an n_fft outside the list or a resolution wun_istft_tf_fft refuses.
 *
 * scratch of the audio output, floats:  2 ceil4(S B F K) + wun_istft_tf_fft_scratch_floats of (S, B, T, 1, n_fft, hop, F)
 *   (the masked spectra of all sources, Re then Im, then the inverse transform's own scratch; ceil4 rounds up to a multiple of 4)
 *   audio : device [S, B, T, 1], every float written;  workspace : the training workspace, read only */
int64_t wun_spec_train_audio_scratch_floats(const wun_spec_config* cfg, int32_t B, int64_t T);
int     wun_spec_train_audio(const wun_spec_config* cfg, const wun_spec_train_config* tcfg, int32_t B, int64_t T,
                             const float* table_dev, float* audio, const float* workspace, float* scratch, void* stream);
/* scratch of the backward, floats:  ceil4(hop) + B T   (D, then u of one source; the same with d_audio null)
 *   d_mags : device [S, B, F, K] or NULL;  d_audio : device [S, B, T, 1] or NULL;  at least one
 *   grads  : device, wun_spec_param_floats floats; wun_spec_adam_step takes them as it takes wun_spec_loss_backward's */
int64_t wun_spec_backward_scratch_floats(const wun_spec_config* cfg, int32_t B, int64_t T);
int     wun_spec_backward(const wun_spec_config* cfg, const wun_spec_train_config* tcfg, const float* params, const float* d_mags,
                          const float* d_audio, int32_t B, int64_t T, const float* table_dev, float* grads, float* workspace,
                          float* scratch, void* stream);
/* The UPDATE_OPS alone: the moving averages of wun_spec_adam_step from the batch statistics of the last forward, the same launch
 * and bits, for callers whose optimizer is not wun_spec_adam_step.  The workspace is read only. */
int     wun_spec_update_moving_averages(const wun_spec_config* cfg, const wun_spec_train_config* tcfg, float* params,
                                        const float* workspace, int32_t B, int64_t T, void* stream);

/* tf.contrib.signal.inverse_stft with inverse_stft_window_fn(hop): wun_istft in the framing without padding (lead 0), except for
 * the normaliser:  y[t] = (sum_f frame_f[t - f hop]) / D[t mod hop],  D[p] = sum_i w^2[p + i hop] over 0 <= p + i hop < n_fft
 * (i ascending, float64) -- the steady-state window-square sum, at the track's edges too, where wun_istft divides by the sum
 * over the covering frames only.  Frames, table, scratch formula, contract, checks and their order are wun_istft's (lead = 0);
 * then WUN_ERR_UNSUPPORTED for a resolution where some D[p] is below 1e-8 (1024 / 768: min D = 2 sin^4(pi / 8) = 0.0429).  Samples no frame covers
 * are 0.  wun_istft_tf_fft: the same on wun_istft_fft (the table of wun_fft_design, n_fft up to 8192). */
int64_t wun_istft_tf_scratch_floats(int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop, int64_t F);
int     wun_istft_tf(const float* re, const float* im, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                     int64_t F, const float* table_dev, float* y, float* scratch, void* stream);
int64_t wun_istft_tf_fft_scratch_floats(int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop, int64_t F);
int     wun_istft_tf_fft(const float* re, const float* im, int32_t S, int32_t B, int64_t T, int32_t C, int32_t n_fft, int32_t hop,
                         int64_t F, const float* table_dev, float* y, float* scratch, void* stream);

/* ---- single operators (used by the parity tests and for per-kernel profiling) ---------- */

/* One layer of the spectrogram U-Net, channel-last float32.  y = act(bn(conv + bias)):
 *   x [B][H][W][cin], w [5][5][cin][cout] (TF layout), y [B][H / 2][W / 2][cout]; H and W even
 *   bias [cout] or NULL;  bn_mean, bn_var, bn_beta [cout], all three or none: (z - mean) / sqrt(var + 1e-3) + beta
 *   act : 0 none, 1 LeakyReLU(0.2), 2 ReLU, 3 sigmoid
 *         a NaN before the activation comes out as NaN from all four (ReLU is z > 0 ? z : (z != z ? z : 0), as torch.relu and TF's)
 * cin == 1 runs on the VALU, everything else on the exact-fp32 MFMA; same accumulation order, same bits.
 * WUN_ERR_INVALID before any GPU work for a null x / w / y, a size below 1, odd H or W, an unknown act or a partial batch norm. */
int wun_op_conv2d_s2(const float* x, const float* w, const float* bias, const float* bn_mean, const float* bn_var,
                     const float* bn_beta, float* y, int B, int H, int W, int cin, int cout, int act, void* stream);
/* The transposed layer: the input is the virtual channel concatenation of x0 [B][H][W][c0] and (optionally) x1 [B][H][W][c1],
 * w [5][5][cout][c0 + c1] (TF layout), y [B][2 H][2 W][cout], every float written once; epilogue as above.  cout == 1 runs on
 * the VALU.  WUN_ERR_INVALID also for c0 < 1, c1 < 0, or x1 given without c1 (and the reverse). */
int wun_op_conv2d_transpose_s2(const float* x0, int c0, const float* x1, int c1, const float* w, const float* bias,
                               const float* bn_mean, const float* bn_var, const float* bn_beta, float* y, int B, int H, int W,
                               int cout, int act, void* stream);

/* The weight gradients of the two layers above, one form: G[ky][kx][p][q] = sum_{b,y,x} Big[b][2y + ky - 1][2x + kx - 1][p]
 * Small[b][y][x][q], zeros outside the big map.  The reduction over the B Hs Ws pixels of the small map is cut into chunks of 256
 * consecutive pixels; chunk c's partial goes to scratch, a second pass adds the chunks in ascending order.  Exact-fp32 MFMA where
 * both channel counts exceed 1, the VALU otherwise.  db = sum dz over the pixels (float64 partials per 1024 pixels) or NULL.
 *   strided   : x [B][H][W][cin] (Big), dz [B][H / 2][W / 2][cout] (Small), dw [5][5][cin][cout], db [cout]
 *   transposed: dz [B][2 H][2 W][cout] (Big), x0 [B][H][W][c0] and optionally x1 [..][c1] (Small), dw [5][5][cout][c0 + c1]
 * scratch: *_scratch floats (negative wun_status for bad sizes); what it held does not matter; it may not overlap an operand. */
int64_t wun_op_conv2d_s2_wgrad_scratch(int B, int H, int W, int cin, int cout);
int     wun_op_conv2d_s2_wgrad(const float* x, const float* dz, float* dw, float* db, float* scratch, int B, int H, int W,
                               int cin, int cout, void* stream);
int64_t wun_op_conv2d_transpose_s2_wgrad_scratch(int B, int H, int W, int cin, int cout);
int     wun_op_conv2d_transpose_s2_wgrad(const float* x0, int c0, const float* x1, int c1, const float* dz, float* dw, float* db,
                                         float* scratch, int B, int H, int W, int cout, void* stream);
/* mean[c] and the biased variance var[c] of z [B][H][W][C] over its n = B H W pixels: two passes, float64 partials per 1024
 * pixels added in a fixed order, rounded to float32 once each. */
int64_t wun_op_bn2d_stats_scratch(int B, int H, int W, int C);
int     wun_op_bn2d_stats(const float* z, float* mean, float* var, float* scratch, int B, int H, int W, int C, void* stream);

/* The head of wun_spec_backward for one source, without a network: dz [B][F][K - 1] from re, im, mag [B][F][K] (X and M of the
 * mix), mask [B][F][K - 1], d_mags [B][F][K] or NULL and d_audio [B][T] or NULL (at least one), by the formulas of that section.
 * T == (F - 1) hop + n_fft, n_fft a power of two in 64..8192, hop in 1..n_fft; table_dev is wun_fft_design's table.
 * scratch, floats:  ceil4(hop) + B T;  it may overlap neither dz nor an operand, nor dz an operand. */
int64_t wun_op_spec_head_backward_scratch(int32_t B, int64_t T, int32_t n_fft, int32_t hop);
int     wun_op_spec_head_backward(const float* re, const float* im, const float* mag, const float* mask, const float* d_mags,
                                  const float* d_audio, int32_t B, int64_t T, int32_t n_fft, int32_t hop, const float* table_dev,
                                  float* dz, float* scratch, void* stream);

/* The launch ledger of the FFT path (test entries; host only, nothing on a hot path reads it).  The eight kernel bodies of the
 * FFT path are built for each of the eight sizes n_fft = 64 << j, j = 0 .. WUN_FFT_SIZE_COUNT - 1; every launch of one that the
 * runtime accepted adds 1 to the process-wide counter [family][j].  A refused n_fft (WUN_ERR_UNSUPPORTED) adds nothing.
 *   FORWARD            Re / Im of every bin     wun_stft_complex_fft and the *_fft filters' analysis
 *   MAGNITUDE          the loss's forward       wun_stft_magnitude_fft, wun_spectral_loss*_fft
 *   SPEC_HEAD          the mask-gradient head   wun_spec_backward, wun_op_spec_head_backward (with d_audio)
 *   INVERSE            frames of a spectrum     wun_istft_fft, wun_istft_tf_fft, the *_fft filters, wun_time_stretch's synthesis
 *   ADJOINT            the loss's gradient      wun_spectral_loss*_fft with d_outputs
 *   GRIFFIN_LIM        a step from audio        wun_griffin_lim
 *   GRIFFIN_LIM_GIVEN  a step from a spectrum   wun_griffin_lim with re0 / im0, its first step
 *   VOC_ANALYSIS       the vocoder's analysis   wun_time_stretch
 * wun_fft_launch_counts copies the table to counts[family * WUN_FFT_SIZE_COUNT + j]; WUN_ERR_INVALID for a null pointer or
 * cap < WUN_FFT_FAMILY_COUNT * WUN_FFT_SIZE_COUNT.  wun_fft_launch_counts_reset sets every counter to 0. */
enum { WUN_FFT_FAMILY_FORWARD = 0, WUN_FFT_FAMILY_MAGNITUDE = 1, WUN_FFT_FAMILY_SPEC_HEAD = 2, WUN_FFT_FAMILY_INVERSE = 3,
       WUN_FFT_FAMILY_ADJOINT = 4, WUN_FFT_FAMILY_GRIFFIN_LIM = 5, WUN_FFT_FAMILY_GRIFFIN_LIM_GIVEN = 6,
       WUN_FFT_FAMILY_VOC_ANALYSIS = 7, WUN_FFT_FAMILY_COUNT = 8 };
enum { WUN_FFT_SIZE_COUNT = 8 };
int  wun_fft_launch_counts(int64_t* counts, int32_t cap);
void wun_fft_launch_counts_reset(void);

/* y[b][co][q] = act(bias[co] + sum_{k,ci} w[k][ci][co] * x[b][ci][q*stride + k - pad_left]),
 * x zero outside [0, t_in).  NCW float32, w in TF layout [K, Cin, Cout].
 * stride in {1, 2}; t_out is given by the caller.  lrelu: 0/1 (alpha = 0.2). */
int wun_op_conv1d(const float* x, const float* w, const float* bias, float* y,
                  int batch, int cin, int cout, int k, int t_in, int t_out,
                  int stride, int pad_left, int lrelu, void* stream);

/* dw[k][ci][co] = sum_{b,q} x[b][ci][q*stride + k - pad_left] * dz[b][co][q]; db[co] = sum dz.
 * scratch: device floats, at least wun_op_conv1d_wgrad_scratch(...) of them. */
int64_t wun_op_conv1d_wgrad_scratch(int batch, int cin, int cout, int k, int t_out);
int wun_op_conv1d_wgrad(const float* x, const float* dz, float* dw, float* db, float* scratch,
                        int batch, int cin, int cout, int k, int t_in, int t_out,
                        int stride, int pad_left, void* stream);

/* dx[b][ci][t] = sum_{k,co} w[k][ci][co] * dz[b][co][(t + pad_left - k)/stride] (when divisible
 * and in range).  wt_scratch: device floats, >= 2*k*cin*cout. */
int wun_op_conv1d_dgrad(const float* dz, const float* w, float* dx, float* wt_scratch,
                        int batch, int cin, int cout, int k, int t_in, int t_out,
                        int stride, int pad_left, void* stream);

/* The plan's general conv launch as a single operator: the input is the virtual channel-concat of
 * x0 [B][c0][t_in] and (optionally) x1 [B][c1][t_in] (Utils.crop_and_concat, Utils.py:11-24, without
 * the copy); output element q of channel n is stored at y[b][n][ooff + q*ostride] (y is [B][cout][t_y]);
 * mask (same geometry as y, or NULL) multiplies by the LeakyReLU derivative of the value stored
 * there (1 if > 0 else 0.2); accumulate adds to what y already holds.  Semantics otherwise as
 * wun_op_conv1d. */
int wun_op_conv1d_ex(const float* x0, int c0, const float* x1, int c1, const float* w, const float* bias,
                     float* y, const float* mask, int batch, int cout, int k, int t_in, int t_out,
                     int t_y, int stride, int pad_left, int lrelu, int accumulate, int ostride, int ooff,
                     void* stream);

/* Test hook for the secondary outputs of the plan's conv launch (round 6: a context plan computes every conv output once --
 * the decimated stream is a slice of the encoder output, UnetAudioSeparator.py:98-100).  Every following wun_op_conv1d_ex
 * launch also writes
 *   copy0 [B][cout][t0]: expand = 0: the compact copy of its EVEN outputs, copy0[b][n][q / 2] (same-padding down levels);
 *                        expand = 1: output q at copy0[b][n][2q - exp_lo] where 0 <= 2q - exp_lo < exp_len (the stride-2
 *                        launch of a down level writing the even positions of the skip window);
 *   copy1 [B][cout][t1]: the compact copy of its ODD outputs, copy1[b][n][q / 2] (an up level's input gradient splitting
 *                        the skip window's gradient by parity);
 * and, when acc_len > 0, `accumulate` applies only to the row positions ooff + q*ostride inside [acc_lo, acc_lo + acc_len)
 * (stored elsewhere).  NULL pointers / acc_len = 0 switch each part off; wun_op_set_conv_copies(0,0,0,0,0,0,0,0,0) resets. */
int wun_op_set_conv_copies(float* copy0, int t0, int expand, int exp_lo, int exp_len, float* copy1, int t1,
                           int acc_lo, int acc_len);

/* Test hook: force the tile variant (index into the kernel's variant table, -1 = automatic) and
 * split-K factor (0 = automatic) of every following wun_op_conv1d / _ex / _dgrad launch, so the parity
 * tests can reach every tiling.  A choice the dispatcher would never make for that launch (tile
 * mostly padding, split past the scratch buffer, loader not supported by the tile) makes the
 * launch fail with WUN_ERR_HIP -- it is rejected, not miscomputed. */
int wun_op_force_conv_variant(int variant, int ksplit);
int wun_op_num_conv_variants(void);

/* Test hook for wun_op_conv1d_wgrad: force the weight-gradient tile geometry (mtw in {1,2,4,6} row
 * tiles per wave, nw in 1..5 column tiles; 0,0 = automatic) and the number of reduction splits
 * (0 = automatic).  Call wun_op_conv1d_wgrad_scratch AFTER forcing: the scratch size depends on it.
 * A geometry the kernel's staging cannot hold for the shape fails with WUN_ERR_UNSUPPORTED. */
int wun_op_force_wgrad_variant(int mtw, int nw, int nsplit);

/* Test hook: run the following wun_op_conv1d_wgrad calls on the bf16 speed-mode kernel (operands rounded
 * to bf16, v_mfma_f32_16x16x32_bf16, fp32 accumulate; same tiles / splits / reduction). */
int wun_op_set_wgrad_bf16(int on);

/* Test hook: run the following (exact-fp32) wun_op_conv1d_wgrad calls on the register-window form of the weight-gradient
 * kernel (wgrad_win_kernel: aligned 16-byte operand reads, DMA staging issued from inside the MFMA stream, split partials
 * in the final [K][Cin][Cout] layout) -- the form the plan uses for every layer it serves.  wun_op_force_wgrad_variant then
 * means (1, column tiles per wave 1..5|6, splits; a negative split count = target grid size).  Shapes the kernel does not
 * serve (taps other than 15 / 5; 15 taps with Cin not a multiple of 8) fail with WUN_ERR_UNSUPPORTED.  Ignored while the
 * bf16 hook is on. */
int wun_op_set_wgrad_win(int on);

/* Test hook: run the following wun_op_conv1d_wgrad calls on the direct-reduction ("narrow") kernels the plan uses for the
 * layers without a dense channel x channel face -- the 1-/2-channel audio-input conv and the output head (wun_narrow.hip:
 * the LDS-staged form for Cin * Cout <= 256, the streaming form for one input channel and <= 24 output channels).  Other
 * shapes fail with WUN_ERR_UNSUPPORTED. */
int wun_op_set_wgrad_narrow(int on);

/* Test hook: what the plan asks of the last conv of a level (DESIGN.md "fused upsampling").  Every following stride-1
 * wun_op_conv1d_ex launch also produces ups_y[b][c][0 .. ups_tup) = the 2x upsampling of its output y[b][c][0 .. t_out)
 * (rows ups_pitch floats apart, batch stride cout * ups_pitch; ups_tup = 2 t_out - 1 or 2 t_out; ups_w = the learned
 * per-channel weights before the sigmoid, or NULL = linear; ups_y 16-byte aligned).  A launch that ends in the split-K
 * epilogue writes it there; any other launch is followed by the stand-alone kernel, as in the plan.
 * wun_op_last_path(WUN_OP_CONV_EPILOGUE) tells which.  wun_op_set_conv_upsample(NULL, 0, 0, NULL) resets. */
int wun_op_set_conv_upsample(float* ups_y, int ups_pitch, int ups_tup, const float* ups_w);

/* Input gradient of an up conv over concat(skip, 2x LINEAR upsampling of x_prev), as the plan launches it: the bias-free,
 * activation-free stride-1 conv  g[b][m][q] = sum_{j, c} wt[j][c][m] dz[b][c][q + j - pad_left]  (wt [k][cin][n_skip + n_cur],
 * dz [batch][cin][t_in], 0 <= q < tup, zero outside [0, t_in)).  Columns m < n_skip go to d_skip [batch][n_skip][tup]; the
 * others are d(upsampled tensor) and go through the adjoint of the upsampling into
 *   dz_prev[b][c][i] = LeakyReLU'(x_prev[b][c][i]) * (g[2i] + wa g[2i+1] + 1/2 g[2i-1]),  0 <= i < n,  tup in {2n - 1, 2n}
 * (wa = 1 at i = n - 1 with tup = 2n, else 1/2; rows of dz_prev / x_prev prev_pitch floats apart).  A launch that ends in the
 * split-K epilogue (wun_op_force_conv_variant(v, ksplit >= 2)) does this there and leaves d_up [batch][n_cur][tup] untouched;
 * any other launch stores d_up and runs the stand-alone adjoint.  wun_op_last_path(WUN_OP_CONV_EPILOGUE) tells which. */
int wun_op_conv1d_upsample_adjoint(const float* dz, const float* wt, float* d_skip, float* d_up, float* dz_prev,
                                   const float* x_prev, int batch, int cin, int n_skip, int n_cur, int k, int t_in, int tup,
                                   int pad_left, int n, int prev_pitch, void* stream);

/* ---- The elementwise family as single operators (upsampling, head, layout change) ---------------------------------------
 * Thin wrappers over the launchers the plan uses.  Rows may sit anywhere: no alignment is asked of pointers or pitches, a
 * tensor that is not 16-byte aligned with padded pitches is served by the scalar forms.  Pitches are in ELEMENTS, the batch
 * stride of a tensor is channels * pitch.  bf16 != 0: the rows hold bfloat16 elements (arithmetic in fp32, one rounding to
 * nearest even on the store).  FOOTPRINT: exactly the elements [0, length) of every output row are written; row padding
 * between length and pitch and everything before / behind the tensor is never touched.
 * WUN_ERR_INVALID (before any GPU work) for a null required pointer, a shape below 1, a pitch below its row length, tup
 * outside {2n - 1, 2n}, more than 4 head sources or 2 channels. */

/* y[b][c][2i] = x[b][c][i];  y[b][c][2i+1] = s x[i] + (1 - s) x[i+1], s = sigmoid(w[c]), x[n] = 0   (w != NULL, learned)
 *                                           = 0.5 (x[i] + x[i+1]), x[n] = x[n-1]                     (w == NULL, linear)
 * for 0 <= t < tup; tup = 2n - 1 (context) or 2n. */
int wun_op_upsample(const void* x, void* y, const float* w, int B, int C, int n, int tup, int xpitch, int ypitch, int bf16,
                    void* stream);
/* The adjoint, times the LeakyReLU derivative of the level's stored activation x (1 for x > 0, else 0.2):
 *   dz[b][c][i] = LeakyReLU'(x[i]) (dy[2i] + wa dy[2i+1] + wb dy[2i-1])     (terms outside [0, tup) dropped)
 * learned: wa = s, wb = 1 - s; linear: wa = wb = 1/2, wa = 1 at i = n - 1 when tup = 2n.  dz has x's geometry.
 * With w and dw: dw[c] (=, or += with accumulate) s (1 - s) sum_{b, i} dy[2i+1] (x[i] - x[i+1]); dw_partial = B * C floats of
 * scratch selects the two-stage form where the rows allow it, NULL the one-stage form. */
int wun_op_upsample_backward(const void* dy, const void* x, void* dz, const float* w, float* dw, float* dw_partial, int B,
                             int C, int n, int tup, int ypitch, int xpitch, int bf16, int accumulate, void* stream);

/* The output head (OutputLayer.py): S estimates [S][B][Tout][C] from the mix rows [B][C][mix_pitch] and the feature map
 * [B][F][feat_pitch] (Tfeat valid).  Sh = S - difference sources have a conv of Ko taps over concat(mix, features):
 *   pre_s[b][t][c] = bias_s[c] + sum_{k, ci} W_s[k][ci][c] in[b][ci][t + k - padl]     (zero outside [0, Tfeat))
 * with in = mix[mix_off_feat + .] for ci < C and feat for ci >= C; out_s = tanh(pre_s) (tanh != 0), or pre_s clipped to
 * [-1, 1] unless training.  difference: out[S-1] = mix[mix_off_diff + t] - sum_s out_s (clipped unless training).
 * Source s' parameters {W [Ko][C+F][C], bias [C]} start at params + hoff[s]: any order, gaps allowed. */
typedef struct wun_op_head_desc {
    int32_t C, F, S, difference, Ko, padl, Tfeat, Tout, B, tanh, training, feat_bf16;
    int32_t mix_pitch, feat_pitch, dpre_pitch;      /* elements; dpre is [Sh][B][C][dpre_pitch] */
    int32_t mix_off_feat, mix_off_diff;             /* crop offsets into a mix row */
} wun_op_head_desc;
int32_t wun_op_head_abi_size(void);   /* sizeof(wun_op_head_desc) */
int wun_op_head_forward(const wun_op_head_desc* desc, const float* mix, const void* feat, const float* params,
                        const int64_t* hoff, float* out, void* stream);
/* MSE over all S estimates: *loss = mean (out - targets)^2; dpre = dL/d pre_s; dzfeat (feat's geometry and type) =
 * LeakyReLU'(feat) * dL/d feat.  out: what wun_op_head_forward wrote with training != 0 -- the gradient is the training graph's
 * (clipping happens at inference only), the backward entries do not read desc->training. */
int wun_op_head_loss_backward(const wun_op_head_desc* desc, const void* feat, const float* params, const int64_t* hoff,
                              const float* out, const float* targets, float* dpre, void* dzfeat, float* loss, void* stream);
/* The same from an upstream gradient d_outputs [S][B][Tout][C] instead of the MSE. */
int wun_op_head_backward(const wun_op_head_desc* desc, const void* feat, const float* params, const int64_t* hoff,
                         const float* out, const float* d_outputs, float* dpre, void* dzfeat, void* stream);

/* dst[b][c][t] = src[b][t][c]  ([B][T][C] -> [B][C][pitch]), any C >= 1. */
int wun_op_btc_to_ncw(const float* src, float* dst, int B, int T, int C, int pitch, void* stream);

/* Which form the last launch of an operator took on the calling thread (the forms share one profiler name): */
#define WUN_OP_UPSAMPLE          0   /* scalar / vec4 / vec8-bf16 */
#define WUN_OP_UPSAMPLE_BACKWARD 1   /* scalar / vec4 */
#define WUN_OP_INTERP_GRAD       2   /* one-stage / two-stage */
#define WUN_OP_HEAD_FORWARD      3   /* generic / four-position */
#define WUN_OP_HEAD_DFEAT        4   /* generic / four-position (d feature map of both head backward entries) */
#define WUN_OP_CONV_EPILOGUE     5   /* fused / not fused (wun_op_set_conv_upsample, wun_op_conv1d_upsample_adjoint) */
#define WUN_OP_BTC_TO_NCW        6   /* scalar / vec4 */
#define WUN_OP_FIRST_CONV        7   /* WUN_PATH_FIRST_CONV once wun_op_first_conv has launched first_conv_kernel */
#define WUN_PATH_NONE          0     /* no launch yet */
#define WUN_PATH_SCALAR        1
#define WUN_PATH_VEC4          2
#define WUN_PATH_VEC8_BF16     3
#define WUN_PATH_ONE_STAGE     4
#define WUN_PATH_TWO_STAGE     5
#define WUN_PATH_GENERIC       6
#define WUN_PATH_FOUR_POSITION 7
#define WUN_PATH_NOT_FUSED     8
#define WUN_PATH_FUSED         9
#define WUN_PATH_FIRST_CONV    10
#define WUN_OP_WGRAD             8   /* direct epilogue / split reduction (wun_op_wgrad_ex) */
#define WUN_PATH_WGRAD_DIRECT  11
#define WUN_PATH_WGRAD_SPLIT   12
int wun_op_last_path(int op);

/* The bf16 mode's conv as a single operator (wun_op_conv1d semantics, Cin >= 8, K <= 15): x and w
 * are rounded to bf16 (nearest-even; x into a temporary bf16 copy -- the kernel reads bf16 rows), products accumulate
 * in fp32, y is stored as fp32.  scratch: device floats, at least
 * wun_op_conv1d_bf16_scratch(cin, cout, k) (packed bf16 weight image).  Synchronises the stream. */
int64_t wun_op_conv1d_bf16_scratch(int cin, int cout, int k);
int wun_op_conv1d_bf16(const float* x, const float* w, const float* bias, float* y, float* scratch,
                       int batch, int cin, int cout, int k, int t_in, int t_out, int stride, int pad_left,
                       int lrelu, void* stream);

/* Input gradient in the bf16 mode (wun_op_conv1d_dgrad semantics; stride 2 = the fused two-phase transposed
 * conv, pad_left 0 and cin % 4 == 0).  scratch: device floats, >= wun_op_conv1d_dgrad_bf16_scratch(cin, cout, k).
 * Synchronises the stream. */
int64_t wun_op_conv1d_dgrad_bf16_scratch(int cin, int cout, int k);
int wun_op_conv1d_dgrad_bf16(const float* dz, const float* w, float* dx, float* scratch, int batch, int cin,
                             int cout, int k, int t_in, int t_out, int stride, int pad_left, void* stream);

/* Tile codes of the bf16 conv: wun_op_force_conv_variant(WUN_BF16_VARIANT_BASE + code, 0), code = (log2 MT) * 9 + (NW - 2) * 3 +
 * (NCK - 1) in 0..26 (MT in {1, 2, 4} tiles of 16 positions per wave, NW in {2, 3, 4} column tiles, NCK in {1, 2, 3} chunks of
 * 32 channels per stage), forces that tile on every following launch of the bf16 conv entries (wun_op_conv1d_bf16,
 * wun_op_conv1d_dgrad_bf16, wun_op_conv_bf16_ex).  A code the launcher would refuse for the launch returns
 * WUN_ERR_UNSUPPORTED before any GPU work.  The bf16 entries ignore forced variants below the base, the fp32 entries those at
 * or above it. */
#define WUN_BF16_VARIANT_BASE 1000

/* The bf16 conv launch of the plan as a single operator, on bf16 rows THE CALLER made.  mode 0 / 1: the stride-1 / stride-2 conv
 *   v[b][n][q] = bias[n] + sum_{k, c} w[k][c][n] x[b][c][q * stride + k - shift]      (zero outside [0, Tin), 0 <= q < Tout)
 * over the virtual channel-concat of x0 [B][C0][x0_pitch] and x1 [B][C1][x1_pitch] (C1 = 0: x1 unused); w is fp32 [K][C0 + C1][N]
 * (rounded to bf16 when it is packed).  mode 2: the input gradient of a valid stride-2 conv of K taps as the plan's fused
 * two-phase launch (shift 0, C1 = 0, N0 = N, N % 4 == 0, no bias / lrelu / dec):
 *   v[b][n][t] = sum_{k, m} w[k][n][m] x[b][m][(t - k) / 2]   (t - k even and inside [0, 2 Tin)),  w fp32 [K][N][C0], 0 <= t < Tout.
 * The first element of every input row is x_off elements (even or odd) behind the row's start; the rest of the row, to its
 * pitch, is never used (it is READ: dword pairs -- it must be addressable, its content is dropped).  x0 / x1: 16-byte aligned,
 * even pitches.  Then lrelu (max(0.2 v, v)), mask (v *= mask > 0 ? 1 : 0.2; mask0 / mask1 have the geometry and type of y0 / y1,
 * or NULL), accumulate (v += what the destination holds, at the row positions y_off + q inside [acc_lo, acc_lo + acc_len);
 * acc_len = 0: everywhere), store: columns n < N0 to y0 [B][N0][y0_pitch] at y0_off + q, the others to y1 [B][N - N0][y1_pitch]
 * at y1_off + q; dec (or NULL): dec[b][n][q >> 1] = the stored value at even q, n < N0, [B][N0][dec_pitch].  out_bf16: y0, y1,
 * the masks and dec hold bf16 (one rounding to nearest even on the store), else fp32.  scratch: device floats, at least
 * wun_op_conv_bf16_ex_scratch(desc).  Every check runs before any GPU work: WUN_ERR_INVALID for a null required pointer, a bad
 * shape, a row that does not fit its pitch or a misaligned input; WUN_ERR_UNSUPPORTED for what the bf16 kernel does not serve
 * (fewer than 8 channels, K > 15, odd pitches, C0 % 8 != 0 with two sources) and for a forced tile code the launcher refuses.
 * Synchronises the stream. */
typedef struct wun_op_conv_bf16_desc {
    int32_t mode, B, C0, C1, N, N0, K, Tin, Tout, shift;
    int32_t lrelu, out_bf16, accumulate, acc_lo, acc_len;
    int32_t x0_pitch, x1_pitch, x_off;                           /* bf16 elements */
    int32_t y0_pitch, y0_off, y1_pitch, y1_off, dec_pitch;       /* elements of the output type */
} wun_op_conv_bf16_desc;
int32_t wun_op_conv_bf16_abi_size(void);   /* sizeof(wun_op_conv_bf16_desc) */
int64_t wun_op_conv_bf16_ex_scratch(const wun_op_conv_bf16_desc* desc);
int wun_op_conv_bf16_ex(const wun_op_conv_bf16_desc* desc, const void* x0, const void* x1, const float* w, const float* bias,
                        void* y0, void* y1, const void* mask0, const void* mask1, void* dec, float* scratch, void* stream);
/* Host only, no GPU work: 1 when the launcher accepts tile `code` (0..26) for the launch `desc` describes, 0 when it refuses
 * it (or the shape); negative for a null or malformed descriptor.  Pointers play no part (rows are taken as aligned). */
int wun_op_conv_bf16_choice_ok(const wun_op_conv_bf16_desc* desc, int code);

/* The audio-input conv of the bf16 mode (first_conv_kernel) as a single operator: fp32 x [B][cin][x_pitch] (cin 1 or 2), fp32 w
 * [k][cin][cout], wun_op_conv1d semantics with stride 1 / 2, output y [B][cout][y_pitch] and the optional compact copy of the even
 * positions dec [B][cout][dec_pitch] (dec[q >> 1] = y[q], even q < t_out) as bf16 (out_bf16) or fp32.  Refuses what the plan's
 * launcher refuses (WUN_ERR_UNSUPPORTED: cin outside {1, 2}, k outside 1..15, y not 16-byte aligned, y_pitch % 4 != 0);
 * WUN_ERR_INVALID for a null pointer, a shape below 1 or a pitch below its row.  Every check runs before any GPU work.
 * wun_op_last_path(WUN_OP_FIRST_CONV) = WUN_PATH_FIRST_CONV afterwards. */
int wun_op_first_conv(const float* x, const float* w, const float* bias, void* y, void* dec, int batch, int cin, int cout, int k,
                      int t_in, int t_out, int stride, int pad_left, int lrelu, int out_bf16, int x_pitch, int y_pitch,
                      int dec_pitch, void* stream);

/* A layer's weight / bias gradient exactly as the plan launches it (run_wgrad / run_narrow_wgrad), on rows THE CALLER made:
 * nothing is repacked or converted, the entry fills the launchers' argument blocks and calls them.  One or two PARTS (a down
 * level: its decimated and its window positions) over one virtual channel-concat of x0 [B][C0][x0_pitch] and x1 [B][C1][x1_pitch]
 * (C1 = 0: x1 unused); part p reads the window [off, off + Tin[p]) of every row (off = x0_off[p] / x1_off[p]; what lies before
 * and behind it in the row is activations of other launches: loaded perhaps, never summed) against dz_p [B][N][dz_pitch[p]]:
 *   dW[k][c][n] = sum_p sum_{b, q < Tq[p]} win_p[b][c][S q + k - shift[p]] dz_p[b][n][q]   (win_p zero outside [0, Tin[p]))
 *   db[n]       = sum_p sum_{b, q} dz_p[b][n][q],          S = 1 (loader 0, direct) or 2 (loader 1, de-interleaving).
 * family: WUN_WGRAD_LDS = wgrad_mfma_kernel, WUN_WGRAD_WIN = the register-window kernel, WUN_WGRAD_BF16 = the bf16 kernel
 * (rows_bf16 must be 1: x0, x1 and dz hold bfloat16 elements, pitches and offsets in elements), WUN_WGRAD_NARROW = the
 * direct-reduction kernels.  grads + 0: the weights [K][C0 + C1][N] with the bias [N] directly behind them -- the plan's arena
 * layout; `accumulate` adds to what the block holds (grad_acc_add: bit-equal to float32 old + stored).  nsplit[p]: requested
 * reduction splits of part p, 0 = the library's choice, else min(request, the part's work units).  Total split count 1: the
 * direct epilogue writes the block; otherwise the parts' splits lie one after the other in `scratch` (device floats, at least
 * wun_op_wgrad_ex_scratch(desc)) and ONE reduction sums them.  Afterwards wun_op_last_path(WUN_OP_WGRAD) is
 * WUN_PATH_WGRAD_DIRECT or WUN_PATH_WGRAD_SPLIT and wun_op_wgrad_last_splits() the total split count.
 * force_mtw / force_nw: as wun_op_force_wgrad_variant takes them for the family (0, 0 = the plan's default; the bf16 family
 * mtw in {4, 8}; the window family mtw = column groups per workgroup 1 / 2, nw = column tiles per wave); a geometry that does
 * not resolve for every part is WUN_ERR_UNSUPPORTED.  Two parts share one tile geometry (LDS / bf16 family: the default is
 * lowered until they agree, as the plan does).
 * WUN_WGRAD_NARROW: N = planes * Nper dz rows; plane s of part p is dz_p + s * zss elements; its block {weights
 * [K][C0 + C1][Nper], bias [Nper]} starts at grads + plane_off[s] (planes in 1..4).  et: bit 0 (value 1) = x0, bit 1 (value 2) = x1,
 * bit 2 (value 4) = dz hold bf16 (instantiated: 0, 2, 4; the streaming form of the audio-input conv 0, 4); rows_bf16 must
 * be 0.  No direct epilogue: always the split reduction.
 * REFUSED, before any GPU work (nothing is computed by another kernel instead) -- WUN_ERR_INVALID: a null required pointer, a
 * size below 1, nparts outside {1, 2}, a loader outside {0, 1}, a negative offset / shift / split request, shift >= K, a window
 * that does not fit its pitch, Tq above dz_pitch, a pitch or zss that is not a multiple of 4 elements, x0 / x1 / dz off 16
 * bytes, rows_bf16 that contradicts the family, planes outside 1..4 or not dividing N, unknown et bits.  WUN_ERR_UNSUPPORTED:
 * what the family's support predicate or launcher refuses (window: K outside {15, 5}, K = 5 with loader 1, fewer than 8
 * channels or 16 columns, K = 15 with (C0 + C1) % 8 or, with two sources, C0 % 8; bf16: K > 15, fewer than 8 channels, odd C0
 * with two sources; LDS: a row group the staging registers cannot hold; narrow: (C0 + C1) * N > 256, K > 15, an et the
 * kernels are not instantiated for); a forced geometry that does not resolve, or two parts whose splits would not share one
 * partial layout; a forced geometry with the narrow family is WUN_ERR_INVALID; and the combinations the plan never builds:
 * two parts with two sources (C1 > 0), and shift > 0 together with a nonzero window offset.
 * Launches on `stream`, does not synchronise. */
#define WUN_WGRAD_LDS    0
#define WUN_WGRAD_WIN    1
#define WUN_WGRAD_BF16   2
#define WUN_WGRAD_NARROW 3
typedef struct wun_op_wgrad_desc {
    int32_t family, B, C0, C1, N, K, x0_pitch, x1_pitch, rows_bf16, nparts;
    int32_t loader[2], x0_off[2], x1_off[2], Tin[2], shift[2], Tq[2], dz_pitch[2], nsplit[2];   /* per part */
    int32_t accumulate, force_mtw, force_nw;
    int32_t planes, zss, et, plane_off[4];                           /* WUN_WGRAD_NARROW */
} wun_op_wgrad_desc;
int32_t wun_op_wgrad_abi_size(void);   /* sizeof(wun_op_wgrad_desc) */
int64_t wun_op_wgrad_ex_scratch(const wun_op_wgrad_desc* desc);
int wun_op_wgrad_ex(const wun_op_wgrad_desc* desc, const void* x0, const void* x1, const void* dz_part0, const void* dz_part1,
                    float* grads, float* scratch, void* stream);
/* Host only: the work units of part `part` under the descriptor's family and geometry (the most splits it can be granted);
 * negative for a descriptor wun_op_wgrad_ex would refuse on shape grounds (pointers play no part). */
int wun_op_wgrad_max_units(const wun_op_wgrad_desc* desc, int part);
/* Total split count of the calling thread's last wun_op_wgrad_ex launch (0 before the first). */
int wun_op_wgrad_last_splits(void);

/* Lane layout probe of v_mfma_f32_16x16x32_bf16: d[16][16] = bf16(a[16][32]) * bf16(b[32][16]) (row-major). */
int wun_op_mfma_bf16_probe(const float* a, const float* b, float* d, void* stream);

/* Lane layout probe of v_mfma_f32_16x16x4_f32: d[16][16] = a[16][4] * b[4][16] (row-major). */
int wun_op_mfma_probe(const float* a, const float* b, float* d, void* stream);

/* Per-kernel timing with HIP events recorded on the launch stream around every heavy launch
 * between begin and end; end() synchronises and writes a JSON summary
 * {"bracket_overhead_ms", "kernels":[{"name","launches","ms","flops"}]} (used by bench.py for the
 * roofline line).  While active, the library's internal side stream is not used, so launch
 * durations are not distorted by concurrent kernels.  "ms" is the raw sum of the event brackets;
 * "bracket_overhead_ms" is the median duration of an EMPTY bracket recorded after every launch
 * (two event packets cost ~5 us that are not kernel time): subtract it once per launch to compare
 * with a profiler's kernel durations. */
int wun_profile_begin(void);
int wun_profile_end(char* json_out, int64_t capacity);

const char* wun_last_error(void);
const char* wun_version(void);

/* sizeof() of the structs this header declares, as the LIBRARY was compiled: sizes[0] = wun_config,
 * sizes[1] = wun_plan_info, sizes[2] = wun_tensor_info; writes min(n, 3) entries and returns 3.  A binding written
 * in another language (the ctypes stub of INTEGRATION.md, cffi, cgo ...) checks its own struct sizes against these
 * before the first call instead of passing a short struct to a library that reads a longer one. */
int wun_abi_sizes(int64_t* sizes, int n);

#ifdef __cplusplus
}
#endif
#endif /* WUN_H */
