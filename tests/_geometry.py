"""Crop and window geometry of context plans: the integers that drive a plan's launch sequence, as a signature computed from
oracle/shapes.py, a grid of small plans that moves them, and a greedy cover of everything the grid reaches.

A context plan's host code branches on a handful of integers per down level (DownShape, csrc/wun_plan_impl.h): the crop start
`cs` of the skip window and its parity, t_ev0 / n_even / t_odd0 / n_odd, whether the crop is symmetric, and whether the even
half E of level i - 1's window gradient lies inside the range W that level i's odd window positions read
(BackwardPass::level_early, wun_backward.hip).  The level signature is

    (cs & 1, crop asymmetric, min(n_odd, 2), min(n_even, 2), ((t_odd0 - 1) & 3) != 0, t_in & 1, t_conv & 1, E inside W)

with E inside W = -1 for level 0, and the head's is

    (in_crop_start & 1, input crop asymmetric, Tout & 1, output-filter crop asymmetric).

The named cases of the suite (GOLDEN_CASES with context, test_gpu_dedup.CASES) take their lengths from get_padding with
filter_size 15 / merge_filter_size 5 or a near relative and reach 6 level and 2 head signatures; CANDIDATES reaches every
value of every field.  tests/test_geometry_host.py pins both counts, tests/test_gpu_geometry.py runs SWEEP against the oracles."""
import numpy as np

from oracle import shapes

TRIPLES = [(15, 5, 1), (8, 4, 2), (3, 2, 3), (2, 1, 1)]      # (filter_size, merge_filter_size, output_filter_size)
LAYERS = [1, 2, 3, 4]
FILTERS = 8
DRESSINGS = {
    # both head kernels and both upsamplers meet every geometry
    "mono": dict(mono_downmix=True, upsampling="linear", output_type="difference"),
    "stereo": dict(mono_downmix=False, upsampling="learned", output_type="direct", task="multi_instrument"),
}
MAX_SWEEP = 40


def overrides(triple, num_layers, dressing="mono"):
    """The model_config overrides (on BASE_MODEL_CONFIG / get_config("baseline")) of one grid point."""
    kd, ku, ko = triple
    return dict(DRESSINGS[dressing], context=True, num_layers=num_layers, num_initial_filters=FILTERS, filter_size=kd,
                input_filter_size=kd, merge_filter_size=ku, output_filter_size=ko)


def oracle_config(triple, num_layers, dressing="mono"):
    return shapes.finalize_config(dict(shapes.BASE_MODEL_CONFIG, **overrides(triple, num_layers, dressing)))


def valid(ocfg, t_in):
    """layer_table passes (every conv has an output, no crop is negative) and there is at least one output frame -- the plan
    refuses t_out < 1 ("input too short for the output layer"), which layer_table does not catch."""
    try:
        lt = shapes.layer_table(ocfg, t_in)
    except AssertionError:
        return False
    return lt["t_out"] >= 1


def _levels(ocfg, t_in):
    """Per down level: the DownShape integers of wun_plan.hip, restated on layer_table."""
    lt = shapes.layer_table(ocfg, t_in)
    L = ocfg["num_layers"]
    out = []
    for i, d in enumerate(lt["down"]):
        u = lt["up"][L - 1 - i]
        tc, cs = u["t_up"], u["crop_start"]
        t_ev0, t_odd0 = cs + (cs & 1), cs + 1 - (cs & 1)
        n_even = len(range(t_ev0, cs + tc, 2))
        out.append(dict(cs=cs, tc=tc, asym=u["crop_end"] != cs, t_ev0=t_ev0, t_odd0=t_odd0, n_even=n_even, n_odd=tc - n_even,
                        t_in=d["t_in"], t_conv=d["t_conv"]))
    return lt, out


def nested(ocfg, t_in):
    """Per level: 1 / 0 = E of level i - 1 lies / does not lie inside W of level i (level_early's condition on a plan that
    computes every output once), -1 for level 0.  E = (t_ev0 / 2, n_even) of level i - 1; W = (t_odd0, 2 (n_odd - 1) + Kd) of
    level i, or (t_odd0, 0) when it has no odd position."""
    kd = ocfg["filter_size"]
    _, lv = _levels(ocfg, t_in)
    out = [-1]
    for i in range(1, len(lv)):
        e_lo, e_len = lv[i - 1]["t_ev0"] // 2, lv[i - 1]["n_even"]
        w_lo, w_len = lv[i]["t_odd0"], (2 * (lv[i]["n_odd"] - 1) + kd if lv[i]["n_odd"] > 0 else 0)
        out.append(int(w_len > 0 and (e_len == 0 or (w_lo <= e_lo and e_lo + e_len <= w_lo + w_len))))
    return out


def signature(ocfg, t_in):
    """(set of level signatures, head signature) of the context plan of `ocfg` on t_in input frames."""
    lt, lv = _levels(ocfg, t_in)
    inside = nested(ocfg, t_in)
    levels = set()
    for d, ew in zip(lv, inside):
        levels.add((d["cs"] & 1, int(d["asym"]), min(d["n_odd"], 2), min(d["n_even"], 2), int(((d["t_odd0"] - 1) & 3) != 0),
                    d["t_in"] & 1, d["t_conv"] & 1, ew))
    h = lt["head"]
    head = (h["in_crop_start"] & 1, int(h["in_crop_end"] != h["in_crop_start"]), h["t_out"] & 1,
            int((h["t_feat"] - h["t_out"]) & 1))
    return levels, head


def shortest_valid(ocfg, count=1, start=1):
    """The first `count` valid input lengths >= start."""
    out, t = [], start
    while len(out) < count:
        if valid(ocfg, t):
            out.append(t)
        t += 1
        assert t < start + 100000
    return out


def _candidates():
    out = []
    for triple in TRIPLES:
        for L in LAYERS:
            ocfg = oracle_config(triple, L)
            lengths = shortest_valid(ocfg, 8)
            lengths += shortest_valid(ocfg, 8, start=shapes.get_padding(ocfg, [1, 40, 0])[0][1])
            out += [(triple, L, t) for t in sorted(set(lengths))]
    return out


def _tokens(cand):
    triple, L, t_in = cand
    levels, head = signature(oracle_config(triple, L), t_in)
    return {("level", s) for s in levels} | {("head", head)}


def _greedy_cover(cands):
    """Fewest-first greedy cover of every signature the candidates reach; ties go to the earlier candidate."""
    tok = [_tokens(c) for c in cands]
    todo = set().union(*tok)
    chosen = []
    while todo:
        gain = [len(t & todo) for t in tok]
        k = int(np.argmax(gain))                     # (first maximum)
        chosen.append(k)
        todo -= tok[k]
    return [cands[k] for k in sorted(chosen)]


def reached(cands):
    """(level signatures, head signatures) a list of (triple, num_layers, t_in) reaches."""
    tok = set().union(*[_tokens(c) for c in cands]) if cands else set()
    return {s for k, s in tok if k == "level"}, {s for k, s in tok if k == "head"}


CANDIDATES = _candidates()                 # [(triple, num_layers, t_in)]: the grid
SWEEP_PLANS = _greedy_cover(CANDIDATES)    # the cover, in grid order
NON_NESTED = [c for c in CANDIDATES if 0 in nested(oracle_config(c[0], c[1]), c[2])]      # E outside W at some level


def _grouped(plans):
    out = {}
    for triple, L, t in plans:
        out.setdefault((triple, L), []).append(t)
    return out


SWEEP = _grouped(SWEEP_PLANS)              # (triple, num_layers) -> [t_in]
NON_NESTED_GROUPS = _grouped(NON_NESTED)
GROUPS = sorted(set(SWEEP) | set(NON_NESTED_GROUPS))


def group_id(group):
    (kd, ku, ko), L = group
    return "k%d-%d-%d_L%d" % (kd, ku, ko, L)


def batch(ocfg, B, t_in, t_out, seed):
    """(mix [B, t_in, C], {source: [B, t_out, C]}): uniform sources scaled 0.9 / S, mix = their sum, targets = the reference's
    crop of the sources (start (t_in - t_out) // 2, the odd remainder dropped at the end: Utils.py:104-123).
    waveunet_torch.synthetic_batch asserts an even t_in - t_out; these plans have both."""
    ocfg = shapes.finalize_config(ocfg)
    S, C = ocfg["num_sources"], ocfg["num_channels"]
    rng = np.random.default_rng(seed)
    srcs = [(rng.uniform(-1.0, 1.0, size=(B, t_in, C)) * (0.9 / S)).astype(np.float32) for _ in range(S)]
    mix = np.sum(np.stack(srcs, 0), axis=0).astype(np.float32)
    start, _ = shapes.crop_offsets(t_in, t_out)
    targets = {n: s[:, start:start + t_out, :].copy() for n, s in zip(ocfg["source_names"], srcs)}
    return mix, targets
