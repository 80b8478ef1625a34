"""CPU-only checks of the C ABI: the library loads, exports every symbol include/wun.h
declares, and its host-side integer logic (get_padding, variable arena, plan shapes)
agrees with the reference-pinned oracle.  No compute calls (no GPU here)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from oracle import shapes
from oracle.golden_params import GOLDEN_CASES

import wave_u_net_amd as wun
from wave_u_net_amd import _lib
from wave_u_net_amd.separator import UnetAudioSeparator, _wun_config

import _abi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_exports_every_declared_symbol(lib):
    hdr = open(os.path.join(ROOT, "include", "wun.h")).read()
    declared = set(re.findall(r"\b(wun_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations found"
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.wun_version().decode().startswith("wun")


# ---- the whole binding against the whole header (tests/_abi.py) ----
@pytest.fixture(scope="module")
def header():
    return _abi.parse(os.path.join(ROOT, "include", "wun.h"))


_BOUND_STRUCTS = [v for v in vars(_lib).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure]


def test_every_prototype_matches_its_binding(header):
    """Arity, return type, and per argument scalar-or-pointer, width, kind and pointee of all of _lib._SIGS; the names agree in
    both directions."""
    assert len(header["functions"]) == len(_lib._SIGS) > 100
    assert _abi.compare_functions(header["functions"], _lib._SIGS) == []


def test_every_struct_matches_its_binding(header):
    """Field names, order, types and array lengths of every ctypes Structure; every header struct but the opaque plan is bound."""
    assert header["opaque"] == {"wun_plan"}
    assert _abi.compare_structs(header["structs"], _BOUND_STRUCTS) == []
    for entry, cls in _lib._ABI_SIZES:                       # load()'s size table names entries and structs of the header
        assert entry in header["functions"] and _lib.c_name(cls) in header["structs"]
    assert len(set(cls for _, cls in _lib._ABI_SIZES)) == len(_lib._ABI_SIZES)


def test_load_refuses_a_struct_of_another_size(lib, monkeypatch):
    class WunBlendWindow(C.Structure):
        _fields_ = _lib.WunBlendWindow._fields_ + [("more", C.c_int64)]
    monkeypatch.setattr(_lib, "_ABI_SIZES", _lib._ABI_SIZES[:-1] + (("wun_blend_abi_size", WunBlendWindow),))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(RuntimeError, match=r"libwun.so wun_blend_window size 16 != this binding's 24 \(stale library or binding\)"):
        _lib.load()


def test_every_constant_of_the_header_is_the_bindings(header):
    """A #define or enumerator the binding repeats (as NAME or WUN_NAME) has the header's value, and every #define is repeated."""
    for name, value in list(header["defines"].items()) + list(header["enums"].items()):
        mine = [getattr(_lib, n) for n in (name, name[4:]) if hasattr(_lib, n)]
        assert mine == [value] or (not mine and name in header["enums"]), name


def test_abi_surface_is_the_pinned_list(lib, header):
    """tests/golden/abi_symbols.txt: the sorted names of the ABI.  Header, binding, library and list agree."""
    pinned = open(os.path.join(ROOT, "tests", "golden", "abi_symbols.txt")).read().split()
    assert pinned == sorted(set(pinned)) == sorted(header["functions"]) == list(_lib.EXPORTED_SYMBOLS)
    assert all(hasattr(lib, name) for name in pinned)


def _edit_function(header, name, edit):
    functions = dict(header["functions"])
    ret, args = functions[name]
    functions[name] = (ret, edit(list(args)))
    return _abi.compare_functions(functions, _lib._SIGS)


def _set(i, value):
    return lambda args: args[:i] + [value] + args[i + 1:]


@pytest.mark.parametrize("name, edit, reason", [
    ("wun_resample", lambda args: args[:-1], "wun_resample: arity 10 != 11"),                       # a dropped argument
    ("wun_resample", _set(2, ("int", 8)), "wun_resample: argument 2: width 8 != 4"),                # int32_t -> int64_t
    ("wun_adam_step", _set(6, ("float", 8)), "wun_adam_step: argument 6: width 8 != 4"),            # float -> double
    ("wun_adam_step", _set(5, ("float", 8)), "wun_adam_step: argument 5: kind float != int"),       # int64_t -> double
    ("wun_resample", _set(1, ("ptr", ("int", 8))),
     "wun_resample: argument 1: pointer in the header, scalar in the binding"),                     # a scalar turned into a pointer
    ("wun_resample", _set(0, ("float", 4)),
     "wun_resample: argument 0: scalar in the header, pointer in the binding"),                     # and the reverse
    ("wun_get_padding", _set(2, ("ptr", ("int", 4))), "wun_get_padding: argument 2: pointee: width 4 != 8"),
])
def test_the_comparison_refuses_an_edited_prototype(header, name, edit, reason):
    """The check can fail: each edit of the PARSED table (never of the library) is reported, for the stated reason only."""
    assert _edit_function(header, name, edit) == [reason]


def test_the_comparison_refuses_edited_structs(header):
    structs = dict(header["structs"])
    f = structs["wun_blend_window"]
    structs["wun_blend_window"] = [f[0], f[2], f[1]]                                               # a swapped struct field
    assert _abi.compare_structs(structs, _BOUND_STRUCTS) == [
        "wun_blend_window: fields ['pos', 'flags', 'row'] != ['pos', 'row', 'flags']"]
    bank = [(n, t, 4 if n == "up" else k) for n, t, k in header["structs"]["wun_speed_bank"]]
    structs = dict(header["structs"], wun_speed_bank=bank)
    assert _abi.compare_structs(structs, _BOUND_STRUCTS) == ["wun_speed_bank.up: array length 4 != 8"]
    structs = dict(header["structs"])
    del structs["wun_mel_terms"]
    assert _abi.compare_structs(structs, _BOUND_STRUCTS) == ["wun_mel_terms: bound, not declared"]
    functions = dict(header["functions"], wun_new_entry=(("int", 4), []))
    assert _abi.compare_functions(functions, _lib._SIGS) == ["wun_new_entry: declared, not bound"]


def test_the_parser_refuses_what_it_does_not_understand(tmp_path):
    for text in ("typedef union u { int a; } u;", "int wun_f(int (*cb)(int));", "int wun_f(wun_unknown* p);",
                 "typedef struct s { int a : 3; } s;", "#define WUN_X (1 << 2)\n", "int wun_f(int a)"):
        path = tmp_path / "h.h"
        path.write_text(text)
        with pytest.raises((ValueError, KeyError)):
            _abi.parse(str(path))


def _oracle_cfg(**kw):
    return shapes.finalize_config(dict(shapes.BASE_MODEL_CONFIG, **kw))


def test_get_padding_through_abi_matches_reference(golden_dir):
    cases = json.load(open(os.path.join(golden_dir, "get_padding.json")))
    for c in cases:
        cfg = wun.get_config("baseline", num_layers=c["num_layers"], filter_size=c["filter_size"],
                             merge_filter_size=c["merge_filter_size"],
                             input_filter_size=c["input_filter_size"],
                             output_filter_size=c["output_filter_size"], context=c["context"],
                             mono_downmix=c["mono_downmix"])
        sep = UnetAudioSeparator(cfg)
        i, o = sep.get_padding(np.array([16, c["desired"], 0]))
        assert list(i) == c["input_shape"] and list(o) == c["output_shape"], c


@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_plan_tables_match_oracle(name, lib):
    case = GOLDEN_CASES[name]
    ocfg = _oracle_cfg(**case["cfg"])
    cfg = wun.get_config("baseline", **case["cfg"])
    sep = UnetAudioSeparator(cfg)
    i, o = shapes.get_padding(ocfg, [case["batch"], case["frames"], 0])
    plan = sep._plan(case["batch"], i[1])
    assert plan.info.input_frames == i[1]
    lt = shapes.layer_table(ocfg, i[1])
    assert plan.info.output_frames == lt["t_out"]
    if ocfg["context"]:
        assert plan.info.output_frames == o[1]
        # (input_filter_size != filter_size -- UnetAudioSeparator.py:73 vs :98: the graph ignores
        # input_filter_size, the surplus input is absorbed by uneven skip crops, Utils.py:120-121;
        # the golden of that case pins the resulting numbers)
        g = np.load(os.path.join(ROOT, "tests", "golden", "fwd_%s.npz" % name))
        assert plan.info.output_frames == g["out_" + ocfg["source_names"][0]].shape[1]
    want = shapes.variable_table(ocfg)
    got = [(n, list(s)) for n, _, s in plan.tensors]
    assert got == [(n, list(s)) for n, s in want]
    # arena is the TF-order concatenation with no padding
    off = 0
    for (n, o_, s) in plan.tensors:
        assert o_ == off, n
        off += int(np.prod(s))
    assert plan.info.arena_floats == off == plan.info.num_params == shapes.num_params(ocfg)
    assert plan.info.workspace_floats > 0
    # dead-work skipping never executes more than the dense graph (except for 1-tap filters, where
    # the stride-2 + crop-window split has no halo to save and the two parts overlap)
    assert plan.info.fwd_flops <= plan.info.fwd_flops_dense + 1e-6 * plan.info.fwd_flops_dense \
        or not ocfg["context"] or ocfg["filter_size"] < 3


def test_m1_sizes_and_flops():
    sep = UnetAudioSeparator(wun.get_config("m1_context"))
    plan = sep._plan(16, 147443)
    assert plan.info.output_frames == 16389
    assert plan.info.num_params == 10263028
    per_ex = plan.info.fwd_flops_dense / 16
    assert abs(per_ex - 22.79e9) / 22.79e9 < 0.01          # 22.79 GFLOP / example
    # dead-work skipping removes ~39 % of the forward FLOPs
    assert 0.55 < plan.info.fwd_flops / plan.info.fwd_flops_dense < 0.68
    sep1 = UnetAudioSeparator(wun.get_config("baseline"))
    plan1 = sep1._plan(16, 16384)
    assert abs(plan1.info.fwd_flops_dense / 16 - 4.887e9) / 4.887e9 < 0.01
    assert plan1.info.fwd_flops == plan1.info.fwd_flops_dense


def test_error_behaviour_matches_reference():
    # same-padding input not divisible by 2^L trips the reference assert (UnetAudioSeparator.py:121)
    sep = UnetAudioSeparator(wun.get_config("baseline", num_layers=3))
    with pytest.raises(ValueError):
        sep._plan(1, 100)
    # get_padding assert x >= 2 (UnetAudioSeparator.py:55) can not trip for desired >= 1; but an
    # input that is too short for the valid convs must fail
    sepc = UnetAudioSeparator(wun.get_config("m1_context"))
    with pytest.raises(ValueError):
        sepc._plan(1, 1000)
    with pytest.raises(NotImplementedError):                 # UnetAudioSeparator.py:136
        UnetAudioSeparator(wun.get_config("baseline", output_activation="relu"))
    with pytest.raises(NotImplementedError):                 # UnetAudioSeparator.py:144
        UnetAudioSeparator(wun.get_config("baseline", output_type="sum"))


def test_named_configs_present():
    for n in ["baseline", "baseline_diff", "baseline_context", "baseline_stereo", "full", "full_44KHz",
              "baseline_context_smallfilter_deep", "full_multi_instrument", "baseline_comparison"]:
        cfg = wun.get_config(n)
        assert cfg["num_sources"] == len(cfg["source_names"])
    assert wun.get_config("full_multi_instrument")["source_names"] == ["bass", "drums", "other", "vocals"]


# Literal transcription of the reference's sacred named configs (/root/reference/Config.py:52-134; the spectrogram
# U-Net ones, :136-161, are out of scope) and of its base dict (:9-39, minus the site paths of :9-11).
_REF_BASE = {
    "model_base_dir": "checkpoints", "log_dir": "logs", "batch_size": 16, "init_sup_sep_lr": 1e-4,
    "epoch_it": 2000, "cache_size": 4000, "num_workers": 4, "num_snippets_per_track": 100,
    "num_layers": 12, "filter_size": 15, "merge_filter_size": 5, "input_filter_size": 15,
    "output_filter_size": 1, "num_initial_filters": 24, "num_frames": 16384, "expected_sr": 22050,
    "mono_downmix": True, "output_type": "direct", "output_activation": "tanh", "context": False,
    "network": "unet", "upsampling": "linear", "task": "voice", "augmentation": True,
    "raw_audio_loss": True, "worse_epochs": 20,
}
_REF_NAMED = {
    "baseline": {},                                                                              # :52-54
    "baseline_diff": {"output_type": "difference"},                                              # :56-61
    "baseline_context": {"output_type": "difference", "context": True},                          # :63-69
    "baseline_stereo": {"output_type": "difference", "context": True, "mono_downmix": False},    # :71-78
    "full": {"output_type": "difference", "context": True, "upsampling": "learned",
             "mono_downmix": False},                                                             # :80-88
    "full_44KHz": {"output_type": "difference", "context": True, "upsampling": "learned",
                   "mono_downmix": False, "expected_sr": 44100},                                 # :90-99
    "baseline_context_smallfilter_deep": {"output_type": "difference", "context": True, "num_layers": 14,
                                          "duration": 7, "filter_size": 5, "merge_filter_size": 1},   # :101-110
    "full_multi_instrument": {"output_type": "difference", "context": True, "upsampling": "linear",
                              "mono_downmix": False, "task": "multi_instrument"},                # :112-121
    "baseline_comparison": {"batch_size": 4, "output_type": "difference", "context": True,
                            "num_frames": 768 * 127 + 1024, "duration": 13, "expected_sr": 8192,
                            "num_initial_filters": 34},                                          # :123-134
}


def test_named_configs_equal_the_reference_dicts():
    """Every reference named config resolves to the reference's model_config, key by key (a dropped override trains
    a different network without any error: round 4's `baseline_comparison` lacked expected_sr / num_initial_filters)."""
    from wave_u_net_amd import config as C
    assert C.BASE_MODEL_CONFIG == _REF_BASE
    for name, over in _REF_NAMED.items():
        assert C.NAMED_CONFIGS[name] == over, name
        want = dict(_REF_BASE)
        want.update(over)
        multi = want["task"] == "multi_instrument"                                               # Config.py:43-50
        want["source_names"] = ["bass", "drums", "other", "vocals"] if multi else ["accompaniment", "vocals"]
        want["num_sources"] = len(want["source_names"])
        want["num_channels"] = 1 if want["mono_downmix"] else 2
        assert wun.get_config(name) == want, name
    cmp_ = wun.get_config("baseline_comparison")
    assert cmp_["num_initial_filters"] == 34 and cmp_["expected_sr"] == 8192 and cmp_["num_frames"] == 98560
    # its plan is the 34-filter network (13.7 M parameters at 12 levels), not the 24-filter one
    sep = UnetAudioSeparator(cmp_)
    (tin, _), (tout, _) = [(s[1], s[2]) for s in sep.get_padding(np.array([4, cmp_["num_frames"], 0]))]
    plan = sep._plan(1, int(tin))
    assert plan.info.num_params == sum(
        15 * ci * co + co for ci, co in zip([1] + [34 * i for i in range(1, 13)], [34 * i for i in range(1, 14)])
    ) + sum(5 * (34 * (12 - j) + 34 * (13 - j)) * 34 * (12 - j) + 34 * (12 - j) for j in range(12)) + 1 * (1 + 34) * 1 + 1


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "wave-u-net_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "oracle" not in src, fn


def test_scheduling_hint_defaults_to_shared_device():
    """wun_config.exclusive_streams (low-priority side streams) is opt-in: a plan created without the key must assume
    that collectives may share the device; the key maps to the last field of the config struct and nothing else."""
    cfg = wun.get_config("baseline")
    c0 = _wun_config(cfg)
    assert c0.exclusive_streams == 0
    c1 = _wun_config(dict(cfg, exclusive_streams=True))
    assert c1.exclusive_streams == 1
    for name, _ in c0._fields_:
        if name != "exclusive_streams":
            assert getattr(c0, name) == getattr(c1, name)
    # the header declares the field last, after compute_dtype (the struct is passed by pointer to wun_plan_create)
    hdr = open(os.path.join(ROOT, "include", "wun.h")).read()
    body = hdr[hdr.index("typedef struct wun_config"):hdr.index("} wun_config;")]
    names = [ln.split(";")[0].split()[-1] for ln in body.splitlines() if ln.strip().startswith("int32_t")]
    assert names == [n for n, _ in c0._fields_]


def test_integration_doc_stub_matches_the_binding(lib):
    """INTEGRATION.md's ctypes stub is what a maintainer pastes: its field list must be the binding's, and the struct it
    builds must have the size the library was compiled with (round 2: the stub had 13 of 14 fields)."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blk = doc[doc.index("class WunConfig(C.Structure):"):]
    blk = blk[:blk.index(")]") + 2]
    fields = re.findall(r'"([a-z_]+)"', blk)
    assert fields == [n for n, _ in _lib.WunConfig._fields_]
    sizes = (C.c_int64 * 3)()
    assert lib.wun_abi_sizes(sizes, 3) == 3
    assert sizes[0] == 4 * len(fields) == C.sizeof(_lib.WunConfig)
    assert sizes[1] == C.sizeof(_lib.WunPlanInfo) and sizes[2] == C.sizeof(_lib.WunTensorInfo)
    init = re.search(r"cfg = WunConfig\(([^)]*)\)", doc).group(1)
    assert len(init.split(",")) == len(fields)


def test_op_descriptors_match_the_header(lib):
    """The single-operator descriptors are passed by pointer: the binding's field lists are the header's, in its order, and
    their sizes the ones the library was compiled with (wun_op_head_abi_size, wun_op_conv_bf16_abi_size)."""
    hdr = open(os.path.join(ROOT, "include", "wun.h")).read()
    for cname, cls, size in (("wun_op_head_desc", _lib.WunOpHeadDesc, lib.wun_op_head_abi_size()),
                             ("wun_op_conv_bf16_desc", _lib.WunOpConvBf16Desc, lib.wun_op_conv_bf16_abi_size())):
        body = hdr[hdr.index("typedef struct %s {" % cname):hdr.index("} %s;" % cname)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in re.findall(r"int32_t\s+([^;]+);", body):
            names += [n.strip() for n in decl.split(",")]
        assert names == [n for n, _ in cls._fields_], cname
        assert all(t is C.c_int32 for _, t in cls._fields_)
        assert size == 4 * len(names) == C.sizeof(cls), cname


def test_c_caller_links_and_runs(tmp_path):
    """tests/abi_smoke.c: a plain C program against include/wun.h + libwun.so (no ctypes, no torch)."""
    import shutil
    import subprocess
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = os.path.join(str(tmp_path), "abi_smoke")
    cmd = [cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "abi_smoke.c"),
           "-L", libdir, "-lwun", "-L", "/opt/rocm/lib", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "abi_smoke: ok" in r.stdout


def test_bf16_mode_units_carry_no_packed_fp32_instructions():
    """tools/pk_check.sh on the objects libwun.so was linked from: the translation units whose kernels can run beside a bf16
    MFMA kernel hold no v_pk_{fma,mul,add}_f32 / v_pk_mov_b32 (the compiler's packed instruction mix returns
    different results from run to run beside v_mfma_f32_16x16x32_bf16 waves -- tools/probes/pk_fma_probe.hip,
    profiles/round6_pk_fma_probe.txt; a Makefile edit that drops the flag from one unit must fail here, not on the GPU)."""
    import subprocess
    objs = os.path.join(ROOT, "wave-u-net_amd", "csrc", "wun_narrow.o")
    if not os.path.exists(objs):
        pytest.skip("objects not built in-tree (library built elsewhere)")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "pk_check.sh")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wun_narrow.o" in r.stdout and " 0 packed fp32 VALU instructions" in r.stdout


# ---- tuning-table headers: the plan's switch snapshot decides which header it accepts ----
def _import_rc(lib, plan, text):
    return lib.wun_plan_tune_import(plan.handle, text.encode())


@pytest.mark.parametrize("name, batch, frames, table", [
    ("m1_context", 16, 147443, "round6_tune_table.txt"),
    ("baseline", 16, 16384, "round6_tune_table_baseline.txt"),
])
def test_pinned_tuning_tables_import(name, batch, frames, table, lib, monkeypatch):
    for k in ("WUN_NO_DEDUP", "WUN_EARLY_WINDOW", "WUN_ODD_FUSE_MIN", "WUN_NO_ODD_ALIGN"):
        monkeypatch.delenv(k, raising=False)
    plan = UnetAudioSeparator(wun.get_config(name))._plan(batch, frames)
    text = open(os.path.join(ROOT, "profiles", table)).read()
    assert _import_rc(lib, plan, text) == 0, lib.wun_last_error().decode()


# the small context config of tests/test_gpu_dedup.py, B = 2 (a dedup plan), under each environment that test uses
_SMALL_CTX = dict(num_layers=5, num_initial_filters=8, num_frames=301, merge_filter_size=3, filter_size=5, input_filter_size=5)
_SMALL_HEAD = ("wun-tune 2 order=r6a variants=67 B=2 Tin=637 L=5 F=8 K=5,3,1 ups=0 out=0 ctx=1 S=2 C=1 act=0 dt=0 "
               "arena=46748 cf=0 cb=0 wg=0")     # + the switch tokens, then a zero-entry table: "\nend\n"
_SWITCHES = ("WUN_NO_DEDUP", "WUN_EARLY_WINDOW", "WUN_ODD_FUSE_MIN", "WUN_NO_ODD_ALIGN")


@pytest.mark.parametrize("env, tokens", [
    ({}, ""),
    ({"WUN_NO_DEDUP": "1"}, " dedup=0"),
    ({"WUN_EARLY_WINDOW": "deep"}, " ew=deep"),
    ({"WUN_EARLY_WINDOW": "0"}, " ew=0"),
    ({"WUN_ODD_FUSE_MIN": "256"}, " oddfuse=256"),
    ({"WUN_ODD_FUSE_MIN": "1"}, " oddfuse=1"),
    ({"WUN_EARLY_WINDOW": "0", "WUN_ODD_FUSE_MIN": "1"}, " ew=0 oddfuse=1"),
    ({"WUN_NO_ODD_ALIGN": "1"}, " oddalign=0"),
    ({"WUN_NO_ODD_ALIGN": "1", "WUN_ODD_FUSE_MIN": "1", "WUN_EARLY_WINDOW": "0"}, " ew=0 oddfuse=1 oddalign=0"),
    # any other value runs the deep-levels order in the backward pass: the header must say so
    ({"WUN_EARLY_WINDOW": "1"}, " ew=deep"),
])
def test_tuning_header_follows_the_switches(env, tokens, lib, monkeypatch):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = wun.get_config("m1_context", **_SMALL_CTX)
    sep = UnetAudioSeparator(cfg)
    i, _ = sep.get_padding(np.array([2, cfg["num_frames"], 0]))
    plan = sep._plan(2, int(i[1]))
    assert _import_rc(lib, plan, _SMALL_HEAD + tokens + "\nend\n") == 0, lib.wun_last_error().decode()
    if tokens:
        assert _import_rc(lib, plan, _SMALL_HEAD + "\nend\n") == -1


def test_tuning_header_is_fixed_at_plan_creation(lib, monkeypatch):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    cfg = wun.get_config("m1_context", **_SMALL_CTX)
    sep = UnetAudioSeparator(cfg)
    i, _ = sep.get_padding(np.array([2, cfg["num_frames"], 0]))
    plan = sep._plan(2, int(i[1]))
    monkeypatch.setenv("WUN_EARLY_WINDOW", "0")
    monkeypatch.setenv("WUN_NO_ODD_ALIGN", "1")
    assert _import_rc(lib, plan, _SMALL_HEAD + "\nend\n") == 0, lib.wun_last_error().decode()
    assert _import_rc(lib, plan, _SMALL_HEAD + " ew=0 oddalign=0\nend\n") == -1
