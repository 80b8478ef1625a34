"""ctypes binding of libwun.so (include/wun.h).  Fails loudly when the HIP library is
missing -- there is NO CPU fallback in the product path."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("WUN_LIB", "libwun.so"))


class WunConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "num_layers", "num_initial_filters", "filter_size", "merge_filter_size",
        "input_filter_size", "output_filter_size", "upsampling", "output_type", "context",
        "num_sources", "num_channels", "output_activation", "compute_dtype", "exclusive_streams")]


class WunPlanInfo(C.Structure):
    _fields_ = [("batch", C.c_int64), ("input_frames", C.c_int64), ("output_frames", C.c_int64),
                ("num_params", C.c_int64), ("arena_floats", C.c_int64),
                ("workspace_floats", C.c_int64), ("num_tensors", C.c_int64),
                ("num_outputs", C.c_int64), ("fwd_flops", C.c_double), ("bwd_flops", C.c_double),
                ("fwd_flops_dense", C.c_double), ("fwd_flops_unique", C.c_double),
                ("bwd_flops_unique", C.c_double), ("compute_dtype_effective", C.c_int64)]


class WunActivationInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("offset", "batch_stride", "pitch", "channels", "frames", "t0", "tstep", "elem_bytes")]


class WunTensorInfo(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("offset", C.c_int64), ("ndim", C.c_int32),
                ("shape", C.c_int64 * 4)]


class WunSpectralTerms(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("mag_l1", "log_mag_l1", "sc", "complex_l1", "log_eps", "sc_eps")]


class WunMelTerms(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("mel_l1", "log_mel_l1", "log_eps")]


class WunWaveformTerms(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("mse", "l1", "si_sdr", "snr", "eps")] + [("zero_mean", C.c_int32)]


class WunSpecConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_layers", "num_initial_filters", "num_sources", "n_fft", "hop")]


class WunSpecTrainConfig(C.Structure):
    _fields_ = [("bn_decay", C.c_float), ("dropout_rate", C.c_float), ("dropout_seed", C.c_int64)]


class WunOptimConfig(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("beta1", "beta2", "eps", "weight_decay", "ema_decay", "clip_norm")] + [("flags", C.c_int32)]


class WunSnippetSource(C.Structure):
    _fields_ = [("start", C.c_int64), ("gain", C.c_float), ("flags", C.c_uint32)]


class WunSpeedBank(C.Structure):
    _fields_ = [("n", C.c_int32), ("up", C.c_int32 * 8), ("down", C.c_int32 * 8), ("table", C.c_void_p * 8)]


class WunStretchJob(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("n_in", C.c_int32), ("n_out", C.c_int32), ("num", C.c_int32),
                ("den", C.c_int32)]


class WunBlendWindow(C.Structure):
    _fields_ = [("pos", C.c_int64), ("row", C.c_int32), ("flags", C.c_int32)]


class WunOpHeadDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "C", "F", "S", "difference", "Ko", "padl", "Tfeat", "Tout", "B", "tanh", "training", "feat_bf16",
        "mix_pitch", "feat_pitch", "dpre_pitch", "mix_off_feat", "mix_off_diff")]


class WunOpConvBf16Desc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "mode", "B", "C0", "C1", "N", "N0", "K", "Tin", "Tout", "shift", "lrelu", "out_bf16", "accumulate", "acc_lo", "acc_len",
        "x0_pitch", "x1_pitch", "x_off", "y0_pitch", "y0_off", "y1_pitch", "y1_off", "dec_pitch")]


class WunOpWgradDesc(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("family", "B", "C0", "C1", "N", "K", "x0_pitch", "x1_pitch", "rows_bf16", "nparts")] +
                [(n, C.c_int32 * 2) for n in ("loader", "x0_off", "x1_off", "Tin", "shift", "Tq", "dz_pitch", "nsplit")] +
                [(n, C.c_int32) for n in ("accumulate", "force_mtw", "force_nw", "planes", "zss", "et")] +
                [("plane_off", C.c_int32 * 4)])


WGRAD_LDS, WGRAD_WIN, WGRAD_BF16, WGRAD_NARROW = range(4)     # wun_op_wgrad_desc.family
BF16_VARIANT_BASE = 1000                           # WUN_BF16_VARIANT_BASE: wun_op_force_conv_variant(base + tile code, 0)

# wun_op_last_path: operators and forms (WUN_OP_*, WUN_PATH_* of include/wun.h)
(OP_UPSAMPLE, OP_UPSAMPLE_BACKWARD, OP_INTERP_GRAD, OP_HEAD_FORWARD, OP_HEAD_DFEAT, OP_CONV_EPILOGUE, OP_BTC_TO_NCW) = range(7)
OP_FIRST_CONV = 7
OP_WGRAD = 8
(PATH_NONE, PATH_SCALAR, PATH_VEC4, PATH_VEC8_BF16, PATH_ONE_STAGE, PATH_TWO_STAGE, PATH_GENERIC, PATH_FOUR_POSITION,
 PATH_NOT_FUSED, PATH_FUSED, PATH_FIRST_CONV, PATH_WGRAD_DIRECT, PATH_WGRAD_SPLIT) = range(13)

BLEND_NO_RISE, BLEND_NO_FALL = 1, 2                 # wun_blend_window.flags
SNIPPET_SWAP, SNIPPET_NEGATE = 1, 2                 # wun_snippet_source.flags
SPEED_RATES, SPEED_MAX_RATIO = 8, 64                # WUN_SPEED_RATES, WUN_SPEED_MAX_RATIO: the rate bank of wun_gather_snippets_speed
STRETCH_JOBS = 64                                   # WUN_STRETCH_JOBS: jobs per launch set of wun_time_stretch
SNIPPET_ROWS = 24                                   # WUN_SNIPPET_ROWS: batch rows per launch of wun_gather_snippets

SPEC_TT_Z, SPEC_TT_MEAN, SPEC_TT_VAR, SPEC_TT_ACT, SPEC_TT_DROPOUT = range(5)     # wun_spec_train_tensor kinds

# wun_fft_launch_counts: the kernel bodies of the FFT path (WUN_FFT_FAMILY_*) and its sizes n_fft = 64 << j, j < FFT_SIZE_COUNT
(FFT_FAMILY_FORWARD, FFT_FAMILY_MAGNITUDE, FFT_FAMILY_SPEC_HEAD, FFT_FAMILY_INVERSE, FFT_FAMILY_ADJOINT, FFT_FAMILY_GRIFFIN_LIM,
 FFT_FAMILY_GRIFFIN_LIM_GIVEN, FFT_FAMILY_VOC_ANALYSIS, FFT_FAMILY_COUNT) = range(9)
FFT_SIZE_COUNT = 8

_P = C.c_void_p
_SIGS = {
    "wun_get_padding": (C.c_int, [C.POINTER(WunConfig), C.c_int64, C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int64)]),
    "wun_plan_create": (C.c_int, [C.POINTER(WunConfig), C.c_int64, C.c_int64, C.POINTER(_P)]),
    "wun_plan_destroy": (None, [_P]),
    "wun_plan_query": (C.c_int, [_P, C.POINTER(WunPlanInfo)]),
    "wun_plan_tensor": (C.c_int, [_P, C.c_int64, C.POINTER(WunTensorInfo)]),
    "wun_plan_activation": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(WunActivationInfo)]),
    "wun_forward": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _P]),
    "wun_loss_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "wun_loss_backward_ex": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.c_int32]),
    "wun_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "wun_backward_ex": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.c_int32]),
    "wun_backward_select": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.c_int32,
                                      C.POINTER(C.c_uint8), C.c_int64]),
    "wun_loss_backward_select": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_void_p),
                                           C.c_int32, C.POINTER(C.c_uint8), C.c_int64]),
    "wun_backward_accumulate": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_void_p),
                                          C.c_int32, C.POINTER(C.c_uint8), C.c_int64]),
    "wun_loss_backward_accumulate": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_void_p),
                                               C.c_int32, C.POINTER(C.c_uint8), C.c_int64]),
    "wun_plan_tune": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "wun_plan_tune_export": (C.c_int, [_P, C.c_char_p, C.c_int64]),
    "wun_plan_tune_import": (C.c_int, [_P, C.c_char_p]),
    "wun_adam_step": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float,
                                C.c_float, C.c_float, _P]),
    "wun_adam_step_select": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float,
                                       C.c_float, C.c_float, _P, C.POINTER(C.c_uint8), C.c_int64]),
    "wun_grad_norm_workspace_floats": (C.c_int64, [_P]),
    "wun_grad_norm": (C.c_int, [_P, _P, C.c_float, _P, _P, C.POINTER(C.c_uint8), C.c_int64]),
    "wun_adam_step_clip": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                     C.c_float, C.c_int32, _P, _P, _P, C.POINTER(C.c_uint8), C.c_int64]),
    "wun_optim_abi_size": (C.c_int64, []),
    "wun_optim_step": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.POINTER(WunOptimConfig), _P, _P, _P,
                                 C.POINTER(C.c_uint8), C.c_int64, C.POINTER(C.c_uint8), C.c_int64]),
    "wun_ema_update": (C.c_int, [_P, _P, _P, C.c_float, C.c_int64, C.c_int32, _P, C.POINTER(C.c_uint8), C.c_int64]),
    "wun_resample_ratio": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "wun_resample_frames": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "wun_resample_table_floats": (C.c_int64, [C.c_int32, C.c_int32]),
    "wun_resample_design": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int64]),
    "wun_resample": (C.c_int, [_P, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int64, C.c_int32, _P, C.c_int32, C.c_int32, _P]),
    "wun_bss_windows": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int64]),
    "wun_bss_scratch_doubles": (C.c_int64, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int64]),
    "wun_bss_correlations": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "wun_bss_window_energies": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, _P, C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int64), C.c_int64, _P, _P, _P]),
    "wun_sos_chunk": (C.c_int32, []),
    "wun_sos_tile": (C.c_int32, []),
    "wun_sosfilt_scratch_doubles": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "wun_sosfilt": (C.c_int, [_P, C.c_int64, C.c_int32, C.POINTER(C.c_double), C.c_int32, _P, _P, _P]),
    "wun_kweight_design": (C.c_int, [C.c_int32, C.POINTER(C.c_double)]),
    "wun_loudness_blocks": (C.c_int64, [C.c_int64, C.c_int32]),
    "wun_loudness_scratch_doubles": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "wun_loudness": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "wun_loudness_gain": (C.c_int, [_P, C.c_double, C.c_double, C.c_double, _P, _P]),
    "wun_scale_by": (C.c_int, [_P, C.c_int64, _P, _P]),
    "wun_true_peak_factor": (C.c_int32, [C.c_int32]),
    "wun_true_peak_scratch_doubles": (C.c_int64, [C.c_int64, C.c_int32]),
    "wun_true_peak": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "wun_loudness_short_term_blocks": (C.c_int64, [C.c_int64, C.c_int32]),
    "wun_loudness_r128_scratch_doubles": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "wun_loudness_r128": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    "wun_stft_frames": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "wun_stft_table_floats": (C.c_int64, [C.c_int32]),
    "wun_stft_design": (C.c_int, [C.c_int32, C.POINTER(C.c_float), C.c_int64]),
    "wun_stft_magnitude": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "wun_spectral_scratch_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                                C.POINTER(C.c_int32)]),
    "wun_spectral_loss": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_float, C.c_int32, C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_void_p), _P, _P, _P, _P]),
    "wun_spectral_terms_scratch_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                                      C.POINTER(C.c_int32), C.POINTER(WunSpectralTerms)]),
    "wun_spectral_loss_terms": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_float, C.c_int32,
                                          C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                          C.POINTER(WunSpectralTerms), C.POINTER(C.c_void_p), _P, _P, _P, _P]),
    "wun_waveform_scratch_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(WunWaveformTerms)]),
    "wun_waveform_loss": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(WunWaveformTerms), C.c_int32,
                                    _P, _P, _P, _P]),
    "wun_stft_centered_frames": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "wun_stft_complex": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                   _P, _P, _P, _P]),
    "wun_istft_scratch_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int64]),
    "wun_istft": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                            _P, _P, _P, _P]),
    "wun_mask_filter_scratch_floats": (C.c_int64, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "wun_mask_filter": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                  _P, _P, _P, _P]),
    "wun_wiener_filter_scratch_floats": (C.c_int64, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "wun_wiener_filter": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                    C.c_int32, C.c_float, _P, _P, _P, _P]),
    "wun_fft_table_floats": (C.c_int64, [C.c_int32]),
    "wun_fft_design": (C.c_int, [C.c_int32, C.POINTER(C.c_float), C.c_int64]),
    "wun_fft_frames": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "wun_fft_centered_frames": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "wun_stft_complex_fft": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                       _P, _P, _P, _P]),
    "wun_istft_fft_scratch_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                 C.c_int64]),
    "wun_istft_fft": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                _P, _P, _P, _P]),
    "wun_mask_filter_fft_scratch_floats": (C.c_int64, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "wun_mask_filter_fft": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                      _P, _P, _P, _P]),
    "wun_wiener_filter_fft_scratch_floats": (C.c_int64, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "wun_wiener_filter_fft": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                        C.c_int32, C.c_float, _P, _P, _P, _P]),
    "wun_griffin_lim_scratch_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                   C.c_int64, C.c_int32]),
    "wun_griffin_lim": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int64, C.c_int32, C.c_float, _P, _P, _P, _P, _P]),
    "wun_stft_magnitude_fft": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "wun_spectral_fft_scratch_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                                    C.POINTER(C.c_int32)]),
    "wun_spectral_loss_fft": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_float, C.c_int32,
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_void_p),
                                        _P, _P, _P, _P]),
    "wun_spectral_terms_fft_scratch_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                                          C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(WunSpectralTerms)]),
    "wun_spectral_loss_terms_fft": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_float, C.c_int32,
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                              C.POINTER(WunSpectralTerms), C.POINTER(C.c_void_p), _P, _P, _P, _P]),
    "wun_mel_table_floats": (C.c_int64, [C.c_int32, C.c_int32]),
    "wun_mel_design": (C.c_int, [C.c_int32, C.c_double, C.c_int32, C.c_double, C.c_double, C.c_int32, C.POINTER(C.c_float),
                                 C.c_int64]),
    "wun_op_mel_project": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P]),
    "wun_op_mel_project_transpose": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P]),
    "wun_mel_abi_size": (C.c_int64, []),
    "wun_spectral_mel_scratch_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                                    C.POINTER(C.c_int32), C.POINTER(WunSpectralTerms), C.POINTER(WunMelTerms),
                                                    C.POINTER(C.c_int32)]),
    "wun_spectral_loss_mel": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_float, C.c_int32,
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                        C.POINTER(WunSpectralTerms), C.POINTER(C.c_void_p), _P, _P, _P, _P,
                                        C.POINTER(WunMelTerms), C.POINTER(C.c_int32), C.POINTER(C.c_void_p)]),
    "wun_spectral_mel_fft_scratch_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                                        C.POINTER(C.c_int32), C.POINTER(WunSpectralTerms), C.POINTER(WunMelTerms),
                                                        C.POINTER(C.c_int32)]),
    "wun_spectral_loss_mel_fft": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_float, C.c_int32,
                                            C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                            C.POINTER(WunSpectralTerms), C.POINTER(C.c_void_p), _P, _P, _P, _P,
                                            C.POINTER(WunMelTerms), C.POINTER(C.c_int32), C.POINTER(C.c_void_p)]),
    "wun_spec_abi_size": (C.c_int64, []),
    "wun_spec_num_tensors": (C.c_int64, [C.POINTER(WunSpecConfig)]),
    "wun_spec_param_floats": (C.c_int64, [C.POINTER(WunSpecConfig)]),
    "wun_spec_tensor": (C.c_int, [C.POINTER(WunSpecConfig), C.c_int64, C.POINTER(WunTensorInfo)]),
    "wun_spec_frames": (C.c_int64, [C.POINTER(WunSpecConfig), C.c_int64]),
    "wun_spec_workspace_floats": (C.c_int64, [C.POINTER(WunSpecConfig), C.c_int32, C.c_int64]),
    "wun_spec_forward": (C.c_int, [C.POINTER(WunSpecConfig), _P, _P, C.c_int32, C.c_int64, _P, _P, _P, _P, _P]),
    "wun_spec_train_abi_size": (C.c_int64, []),
    "wun_spec_train_workspace_floats": (C.c_int64, [C.POINTER(WunSpecConfig), C.c_int32, C.c_int64]),
    "wun_spec_train_tensor": (C.c_int, [C.POINTER(WunSpecConfig), C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                        C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "wun_spec_train_forward": (C.c_int, [C.POINTER(WunSpecConfig), C.POINTER(WunSpecTrainConfig), _P, _P, C.c_int32, C.c_int64, _P,
                                         C.c_int64, _P, _P, _P]),
    "wun_spec_loss_backward": (C.c_int, [C.POINTER(WunSpecConfig), C.POINTER(WunSpecTrainConfig), _P, _P, C.c_int32, C.c_int64, _P,
                                         _P, _P, _P, _P]),
    "wun_spec_adam_step": (C.c_int, [C.POINTER(WunSpecConfig), C.POINTER(WunSpecTrainConfig), _P, _P, _P, _P, _P, C.c_int32,
                                     C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    "wun_spec_train_audio_scratch_floats": (C.c_int64, [C.POINTER(WunSpecConfig), C.c_int32, C.c_int64]),
    "wun_spec_train_audio": (C.c_int, [C.POINTER(WunSpecConfig), C.POINTER(WunSpecTrainConfig), C.c_int32, C.c_int64, _P, _P, _P, _P,
                                       _P]),
    "wun_spec_backward_scratch_floats": (C.c_int64, [C.POINTER(WunSpecConfig), C.c_int32, C.c_int64]),
    "wun_spec_backward": (C.c_int, [C.POINTER(WunSpecConfig), C.POINTER(WunSpecTrainConfig), _P, _P, _P, C.c_int32, C.c_int64, _P,
                                    _P, _P, _P, _P]),
    "wun_spec_update_moving_averages": (C.c_int, [C.POINTER(WunSpecConfig), C.POINTER(WunSpecTrainConfig), _P, _P, C.c_int32,
                                                  C.c_int64, _P]),
    "wun_op_spec_head_backward_scratch": (C.c_int64, [C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "wun_op_spec_head_backward": (C.c_int, [_P] * 6 + [C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "wun_fft_launch_counts": (C.c_int, [C.POINTER(C.c_int64), C.c_int32]),
    "wun_fft_launch_counts_reset": (None, []),
    "wun_op_conv2d_s2_wgrad_scratch": (C.c_int64, [C.c_int] * 5),
    "wun_op_conv2d_s2_wgrad": (C.c_int, [_P] * 5 + [C.c_int] * 5 + [_P]),
    "wun_op_conv2d_transpose_s2_wgrad_scratch": (C.c_int64, [C.c_int] * 5),
    "wun_op_conv2d_transpose_s2_wgrad": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P, _P] + [C.c_int] * 4 + [_P]),
    "wun_op_bn2d_stats_scratch": (C.c_int64, [C.c_int] * 4),
    "wun_op_bn2d_stats": (C.c_int, [_P] * 4 + [C.c_int] * 4 + [_P]),
    "wun_istft_tf_scratch_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "wun_istft_tf": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                               _P, _P, _P, _P]),
    "wun_istft_tf_fft_scratch_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "wun_istft_tf_fft": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                   _P, _P, _P, _P]),
    "wun_op_conv2d_s2": (C.c_int, [_P] * 7 + [C.c_int] * 6 + [_P]),
    "wun_op_conv2d_transpose_s2": (C.c_int, [_P, C.c_int, _P, C.c_int] + [_P] * 6 + [C.c_int] * 5 + [_P]),
    "wun_separate_positions": (C.c_int64, [C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.c_int64]),
    "wun_forward_windows": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_int64), C.c_int64, _P, _P, C.c_int, _P]),
    "wun_scatter_windows": (C.c_int, [_P, _P, C.POINTER(C.c_int64), C.c_int64, _P, C.c_int64, _P]),
    "wun_separate_track": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P]),
    "wun_blend_abi_size": (C.c_int32, []),
    "wun_blend_positions": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(WunBlendWindow), C.c_int64]),
    "wun_blend_windows": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(WunBlendWindow), C.c_int64,
                                    C.c_int64, _P, _P, C.c_int64, _P]),
    "wun_blend_finish": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int64, _P]),
    "wun_separate_track_blend": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64),
                                           C.c_int64, _P, _P, _P, _P, _P]),
    "wun_snippet_abi_size": (C.c_int32, []),
    "wun_gather_snippets": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, _P, C.c_int32,
                                      _P, _P, _P]),
    "wun_speed_abi_size": (C.c_int32, []),
    "wun_speed_source_frames": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "wun_gather_snippets_speed": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, _P, _P,
                                            _P, C.c_int32, _P, _P, _P]),
    "wun_stretch_abi_size": (C.c_int32, []),
    "wun_time_stretch_frames": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "wun_time_stretch_scratch_floats": (C.c_int64, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "wun_time_stretch": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "wun_op_conv1d": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 9 + [_P]),
    "wun_op_conv1d_wgrad_scratch": (C.c_int64, [C.c_int] * 5),
    "wun_op_conv1d_wgrad": (C.c_int, [_P, _P, _P, _P, _P] + [C.c_int] * 8 + [_P]),
    "wun_op_conv1d_dgrad": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 8 + [_P]),
    "wun_op_mfma_probe": (C.c_int, [_P, _P, _P, _P]),
    "wun_op_mfma_bf16_probe": (C.c_int, [_P, _P, _P, _P]),
    "wun_op_conv1d_bf16_scratch": (C.c_int64, [C.c_int] * 3),
    "wun_op_conv1d_bf16": (C.c_int, [_P, _P, _P, _P, _P] + [C.c_int] * 9 + [_P]),
    "wun_op_conv1d_dgrad_bf16_scratch": (C.c_int64, [C.c_int] * 3),
    "wun_op_conv1d_dgrad_bf16": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 8 + [_P]),
    "wun_op_force_conv_variant": (C.c_int, [C.c_int, C.c_int]),
    "wun_op_num_conv_variants": (C.c_int, []),
    "wun_op_force_wgrad_variant": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "wun_op_set_wgrad_bf16": (C.c_int, [C.c_int]),
    "wun_op_set_wgrad_win": (C.c_int, [C.c_int]),
    "wun_op_set_wgrad_narrow": (C.c_int, [C.c_int]),
    "wun_op_conv1d_ex": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P, _P] + [C.c_int] * 12 + [_P]),
    "wun_op_set_conv_copies": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int]),
    "wun_op_set_conv_upsample": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "wun_op_conv1d_upsample_adjoint": (C.c_int, [_P] * 6 + [C.c_int] * 10 + [_P]),
    "wun_op_upsample": (C.c_int, [_P, _P, _P] + [C.c_int] * 7 + [_P]),
    "wun_op_upsample_backward": (C.c_int, [_P] * 6 + [C.c_int] * 8 + [_P]),
    "wun_op_head_abi_size": (C.c_int32, []),
    "wun_op_head_forward": (C.c_int, [C.POINTER(WunOpHeadDesc), _P, _P, _P, C.POINTER(C.c_int64), _P, _P]),
    "wun_op_head_loss_backward": (C.c_int, [C.POINTER(WunOpHeadDesc), _P, _P, C.POINTER(C.c_int64), _P, _P, _P, _P, _P, _P]),
    "wun_op_head_backward": (C.c_int, [C.POINTER(WunOpHeadDesc), _P, _P, C.POINTER(C.c_int64), _P, _P, _P, _P, _P]),
    "wun_op_btc_to_ncw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "wun_op_last_path": (C.c_int, [C.c_int]),
    "wun_op_conv_bf16_abi_size": (C.c_int32, []),
    "wun_op_conv_bf16_ex_scratch": (C.c_int64, [C.POINTER(WunOpConvBf16Desc)]),
    "wun_op_conv_bf16_ex": (C.c_int, [C.POINTER(WunOpConvBf16Desc)] + [_P] * 11),
    "wun_op_conv_bf16_choice_ok": (C.c_int, [C.POINTER(WunOpConvBf16Desc), C.c_int]),
    "wun_op_first_conv": (C.c_int, [_P] * 5 + [C.c_int] * 13 + [_P]),
    "wun_op_wgrad_abi_size": (C.c_int32, []),
    "wun_op_wgrad_ex_scratch": (C.c_int64, [C.POINTER(WunOpWgradDesc)]),
    "wun_op_wgrad_ex": (C.c_int, [C.POINTER(WunOpWgradDesc)] + [_P] * 7),
    "wun_op_wgrad_max_units": (C.c_int, [C.POINTER(WunOpWgradDesc), C.c_int]),
    "wun_op_wgrad_last_splits": (C.c_int, []),
    "wun_profile_begin": (C.c_int, []),
    "wun_profile_end": (C.c_int, [C.c_char_p, C.c_int64]),
    "wun_abi_sizes": (C.c_int, [C.POINTER(C.c_int64), C.c_int]),
    "wun_last_error": (C.c_char_p, []),
    "wun_version": (C.c_char_p, []),
}

EXPORTED_SYMBOLS = tuple(sorted(_SIGS))
WUN_CLIP_SKIP_NONFINITE = 1      # wun_adam_step_clip flags
WUN_OPTIM_EMA_WARMUP = 2         # wun_optim_step / wun_ema_update flags
_lib = None

# (size entry, struct): the structs of this binding against the sizes the library was compiled with, checked by load().
# wun_abi_sizes reports its three in this order; every later struct has an entry of its own.
_ABI_SIZES = (
    ("wun_abi_sizes", WunConfig), ("wun_abi_sizes", WunPlanInfo), ("wun_abi_sizes", WunTensorInfo),
    ("wun_spec_abi_size", WunSpecConfig), ("wun_spec_train_abi_size", WunSpecTrainConfig), ("wun_mel_abi_size", WunMelTerms),
    ("wun_snippet_abi_size", WunSnippetSource), ("wun_op_head_abi_size", WunOpHeadDesc),
    ("wun_op_conv_bf16_abi_size", WunOpConvBf16Desc), ("wun_op_wgrad_abi_size", WunOpWgradDesc), ("wun_speed_abi_size", WunSpeedBank),
    ("wun_stretch_abi_size", WunStretchJob), ("wun_optim_abi_size", WunOptimConfig), ("wun_blend_abi_size", WunBlendWindow))
_DEVICE_TABLES = {}    # device_table's cache


def c_name(cls):
    """The header's name of a struct of this binding: WunOpConvBf16Desc -> wun_op_conv_bf16_desc."""
    return "".join("_" + ch.lower() if ch.isupper() else ch for ch in cls.__name__)[1:]


# Process-wide record of the scheduling hint wun_config.exclusive_streams (include/wun.h): plans created with it run
# their side streams on LOWEST-priority hardware queues, and a process that has ever created those queues is ~40 %
# slower once a communication stream (RCCL) shares the device.  parallel.init_distributed() refuses to start a
# process group after such a plan exists (the hazard cannot be undone inside the process).
LOW_PRIORITY_PLANS = {"created": 0}


def load():
    """Load libwun.so.  torch must already be imported on a GPU box so that the library
    binds to the same HIP runtime instance torch uses (shared SONAME libamdhip64.so.7)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libwun.so not found at %s -- build it with `python __graft_entry__.py` or "
            "`make -C wave-u-net_amd/csrc`; there is no CPU fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)      # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    sizes = (C.c_int64 * 3)()
    lib.wun_abi_sizes(sizes, 3)
    triple = iter(sizes)
    for entry, cls in _ABI_SIZES:
        size = next(triple) if entry == "wun_abi_sizes" else getattr(lib, entry)()
        if size != C.sizeof(cls):
            raise RuntimeError("libwun.so %s size %d != this binding's %d (stale library or binding)" % (
                c_name(cls), size, C.sizeof(cls)))
    _lib = lib
    return lib


class WunError(RuntimeError):
    pass


def check(rc):
    """Map wun_status to the exception the reference would raise in the same situation."""
    if rc == 0:
        return
    msg = load().wun_last_error().decode("utf-8", "replace")
    if rc == -2:
        raise NotImplementedError(msg)            # Training.py:33, UnetAudioSeparator.py:136,144
    if rc == -1:
        raise ValueError(msg)                     # the reference's shape asserts
    raise WunError("wun status %d: %s" % (rc, msg))


def count(v):
    """A frame, float or window count of the library as an int; its negative values are error codes and raise as check does."""
    v = int(v)
    check(min(v, 0))
    return v


def stream(device):
    """torch's current stream on `device` as the void* every entry takes."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def device_table(key, device, make):
    """The device copy of a table designed on the host, uploaded once per process: `key` is (kind, the design's arguments...),
    make() returns the numpy array.  Cached under key + (str(device),), so "cuda" and "cuda:0" hold separate copies."""
    key = tuple(key) + (str(device),)
    if key not in _DEVICE_TABLES:
        import torch
        _DEVICE_TABLES[key] = torch.from_numpy(make()).to(device)
    return _DEVICE_TABLES[key]
