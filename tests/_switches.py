"""The table of the library's environment switches: one row per WUN_* name wun_switches_from_env (wun_plan.hip) reads, the
values the suite runs it at, the class that says what the switch may change, the plans it applies to and what shows that it
took effect.  Data only (no torch, no GPU): tests/test_switches_host.py checks it against the source,
tests/test_gpu_switches.py runs it.

Classes
  schedule          nothing but streams, priorities, fences and placement may change: outputs, every gradient float and d_mix
                    equal the default plan's bit for bit
  wgrad-only        the forward pass and the input-gradient chain are untouched (outputs and d_mix bit-equal); parameter
                    gradients agree with the default's to fp32 summation order and, on fp32 plans, with the float64 oracle
  forward-touching  the switch may select other forward kernels: checked against the float64 oracle under the default plan's
                    tolerance (`equal` rows: the other kernel runs the same arithmetic, bit-equality is asserted)
  owned             tested by the file named in `where`, not repeated
  not-a-launch      changes no launch of a step (tuner, diagnostics): one line saying why

Evidence kinds (what shows the switch took effect; the profiled step's launches come from wun_profile_end's JSON with
WUN_PROFILE_DETAIL=1)
  spelling          a schedule switch leaves no trace in results by design: the name is spelled as the library reads it
                    (test_switches_host.py)
  no_window         the default step has a wgrad_win_kernel launch, the switched one none
  no_narrow         the switched fp32 step has no narrow_wgrad_kernel launch
  fewer_narrow      fewer narrow_wgrad_kernel launches than the default, more than none
  lds_form          no narrow launch carries the streaming form's tag, and a launch whose default counterpart was streaming is
                    now the LDS form (both forms are named narrow_wgrad_kernel; the streaming one's tag ends in "stream")
  nsplit_tag        the nsplit= field of every narrow launch's tag is within the cap and some launch's differs from the default's
  tk_tag            the tk= field of the window launches' tags
  no_dma_name       the default step has a conv_mfma_kernel<..., dma> launch, the switched one none
  launch_list       the step's list of (kernel, tag) differs from the default's
  operator          the plans of the suite are too small for the switch to change a launch (see the row's note): the evidence
                    is in the operator tier of test_gpu_switches.py
  default_bits      a parse edge: the value must be read as "unset", the launches and every bit equal the default plan's"""
from collections import namedtuple

Row = namedtuple("Row", "name values cls plans evidence where note")

# The plans of the plan tier.  golden: the GOLDEN_CASES name (fp32) or BF16_CASES key (bf16) the plan is built from; frames:
# None = that case's own length; rows: None = every row that applies to the mode, else the switches the case was added for.
Case = namedtuple("Case", "key golden mode padding batch frames rows")
CASES = [
    Case("baseline_context_small", "baseline_context_small", "fp32", "context", 3, None, None),
    Case("full_small", "full_small", "fp32", "context", 3, None, None),
    Case("full_multi_small", "full_multi_small", "fp32", "context", 3, None, None),
    Case("learned_same_small", "learned_same_small", "fp32", "same", 3, None, None),
    Case("m4_shaped", "m4_shaped", "bf16", "context", 2, None, None),
    Case("deep_l16_f48_shaped", "deep_l16_f48_shaped", "bf16", "same", 2, None, None),
    # The cases above are too short for three switches to change a launch: every conv has <= 96 outputs per row (batch-folded
    # tiles, which have no DMA instantiation), every window launch already runs units of <= 32 positions (rows of <= 32, or the
    # staging budget of the K = 5 / de-interleaved forms), and every narrow launch has <= 3 work units (B x 1).  The smallest
    # plan that shows all three: learned_same_small at 256 frames (level 1: 128 positions at stride 1, 15 taps), 5 excerpts.
    Case("learned_same_long", "learned_same_small", "fp32", "same", 5, 256,
         ("WUN_NO_DMA", "WUN_WIN_TK", "WUN_NARROW_SPLITS", "WUN_SINGLE_STREAM")),      # (and the serial reference on more tiles)
]

SCHEDULE, WGRAD, FORWARD, OWNED, NOT_LAUNCH = "schedule", "wgrad-only", "forward-touching", "owned", "not-a-launch"
TESTED = (SCHEDULE, WGRAD, FORWARD)
ALL, F32, BF16 = ("fp32", "bf16"), ("fp32",), ("bf16",)
HERE = "tests/test_gpu_switches.py"

ROWS = [
    # ---- schedule ----
    Row("WUN_SINGLE_STREAM", ("1",), SCHEDULE, ALL, "spelling", HERE,
        "everything on the caller's stream, in issue order: THE reference of the three-stream schedule; also run with an "
        "accumulating and a frozen-subset backward, which change what the side streams carry"),
    Row("WUN_SIDE_PRIO", ("low", "normal", "high"), SCHEDULE, ALL, "spelling", HERE, "queue priority of the two side streams"),
    Row("WUN_EVENT_SCOPE", ("system", "device"), SCHEDULE, ALL, "spelling", HERE,
        "fence scope of the stream_dep events (tests/test_event_scope_gpu.py checks the flags themselves)"),
    Row("WUN_BF16_HEAD_SERIAL", ("1",), SCHEDULE, BF16, "spelling", HERE,
        "bf16 plans: the LDS-staged narrow launch joins both side streams and runs on the caller's stream"),
    # ---- wgrad-only ----
    Row("WUN_NO_WIN", ("1",), WGRAD, F32, "no_window", HERE, "bf16 plans never take the window kernel (run_wgrad: !parts[0].bf16)"),
    Row("WUN_NO_NARROW", ("1",), WGRAD, F32, "no_narrow", HERE,
        "MFMA weight gradients for the head and the audio-input conv; bf16 plans ignore it (p->bf16 || ...)"),
    Row("WUN_NO_NARROW_DOWN0", ("1",), WGRAD, F32, "fewer_narrow", HERE, "... for the audio-input conv only: the head stays narrow"),
    Row("WUN_NO_NARROW_STREAM", ("1",), WGRAD, ALL, "lds_form", HERE,
        "the audio-input conv (1 or 2 channels, 15 taps) is the one shape narrow_stream_ok() serves in every case"),
    Row("WUN_NARROW_SPLITS", ("1", "3"), WGRAD, ALL, "nsplit_tag", HERE, "the narrow tag carries nsplit=; operator tier: wun_op_wgrad_last_splits"),
    Row("WUN_WIN_TK", ("16", "32", "128"), WGRAD, F32, "tk_tag", HERE,
        "wgrad_win_geom halves TK while TK / 2 >= Tq, so a request of 128 shows as tk=128 only on rows longer than 64 positions"),
    # ---- forward-touching ----
    Row("WUN_NO_DMA", ("1",), FORWARD, ALL, "no_dma_name", HERE,
        "equal: the register-staged instantiation of the same tile runs the same MFMA stream (per launch: test_gpu_variants.py); "
        "bf16 plans: only their fp32 launches could change, the evidence is asserted on fp32 plans"),
    Row("WUN_NO_FUSE_UPS", ("1",), FORWARD, F32, "launch_list", HERE, "fuse_ups = !bf16 && !no_fuse_ups; per launch: test_gpu_fused_upsample.py"),
    Row("WUN_BF16_LDS_CAP", ("32", "160"), FORWARD, BF16, "operator", HERE,
        "launch_conv_bf16 settles on 64-position tiles (MT = 1) before the cap is read unless a launch has >= 512 tiles of 128 "
        "positions -- 2^16 positions per column group, whose float64 oracle is no few-second test; the plan tier holds the two "
        "bf16 cases to their bounds under both caps, the operator tier shows the tile height moving, at shapes chosen with "
        "bf16_lds() on paper"),
    Row("WUN_NO_K3", ("1",), FORWARD, ALL, "operator", HERE,
        "conv_pick_variant never returns an in-workgroup split-K tile: only a forced, tuned or imported choice reaches "
        "conv_choice_ok's `sw.no_k3` branch, so an untuned plan launches none; the refusal is asserted at the operator tier"),
    # ---- owned elsewhere ----
    Row("WUN_NO_DEDUP", (), OWNED, ALL, None, "tests/test_gpu_dedup.py", "the two-launch plan of rounds 1 - 5"),
    Row("WUN_EARLY_WINDOW", (), OWNED, ALL, None, "tests/test_gpu_dedup.py", "schedule of the odd-window input gradients"),
    Row("WUN_ODD_FUSE_MIN", (), OWNED, ALL, None, "tests/test_gpu_dedup.py", "fuse floor of the odd-window input gradients"),
    Row("WUN_NO_ODD_ALIGN", (), OWNED, ALL, None, "tests/test_gpu_dedup.py", "odd start of the fused odd-window launch"),
    # ---- not a launch switch ----
    Row("WUN_TUNE_ROUNDS", (), NOT_LAUNCH, ALL, None, None, "timing rounds of wun_plan_tune: read by the tuner only, an untuned step never sees it"),
    Row("WUN_TUNE_LOG", (), NOT_LAUNCH, ALL, None, None, "one stderr line per tuned launch position"),
    Row("WUN_TUNE_ALTS", (), NOT_LAUNCH, ALL, None, None, "file the tuner appends near-best candidates to"),
    Row("WUN_TUNE_ALTS_MAX", (), NOT_LAUNCH, ALL, None, None, "how many of them per position"),
    Row("WUN_TUNE_ALTS_TOL", (), NOT_LAUNCH, ALL, None, None, "what counts as near-best"),
    Row("WUN_DUMP_LAYOUT", (), NOT_LAUNCH, ALL, None, None, "workspace map on stderr at plan creation"),
    Row("WUN_PROFILE_DETAIL", (), NOT_LAUNCH, ALL, None, None,
        "per-launch list in the profile JSON, read at wun_profile_begin: the instrument of the evidence above"),
    Row("WUN_WIN_OCC", (), NOT_LAUNCH, ALL, None, None, "occupancy query and a stderr line per window launch; the launch is the same"),
]

# A step between wun_profile_begin and wun_profile_end runs on one stream as well (s2 = ... !g_profiling ... ? p->side : s):
# a schedule-class row without a name in the environment.
PROFILED_STEP = "profiled"

# Values the parser must read as "unset": (name, value, why)
PARSE_EDGES = [
    ("WUN_NO_NARROW_STREAM", "0", "atoi != 0 decides, not presence"),
    ("WUN_NO_K3", "0", "atoi != 0 decides, not presence"),
    ("WUN_WIN_TK", "48", "not one of 16 / 32 / 64 / 128: ignored"),
]
PARSE_EDGE_CASES = ("full_small", "m4_shaped")          # one fp32 and one bf16 plan

# The equal rows of the forward-touching class
FORWARD_EQUAL = ("WUN_NO_DMA",)
# Rows that also run an accumulating and a decoder-only backward against the default schedule's, on these cases
SCHEDULE_EXTRA = {"WUN_SINGLE_STREAM": ("full_small", "m4_shaped")}


def row(name):
    return next(r for r in ROWS if r.name == name)


def names():
    return [r.name for r in ROWS]


def applies(r, case):
    return case.mode in r.plans and (case.rows is None or r.name in case.rows)


def plan_matrix(cls):
    """[(row, value, case)] of one tested class."""
    return [(r, v, c) for r in ROWS if r.cls == cls for v in r.values for c in CASES if applies(r, c)]
