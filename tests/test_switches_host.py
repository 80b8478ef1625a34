"""The switch table (tests/_switches.py) against the one function that reads the environment, wun_switches_from_env in
wun_plan.hip: every name the function reads has a row and every row names a switch the function reads, so a new switch cannot
land without saying which class it belongs to and what tests it.  CPU only."""
import os
import re

import _switches as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wave-u-net_amd", "csrc")


def names_read_by_the_library(text):
    """Every "WUN_..." literal in the body of wun_switches_from_env."""
    m = re.search(r"^WunSwitches\s+wun::wun_switches_from_env\(\)\s*\{\n(.*?)^\}", text, re.S | re.M)
    assert m, "wun_switches_from_env not found in wun_plan.hip"
    return set(re.findall(r'"(WUN_[A-Z0-9_]+)"', m.group(1)))


def _source():
    return open(os.path.join(CSRC, "wun_plan.hip")).read()


def test_every_switch_the_library_reads_has_a_row():
    read, rows = names_read_by_the_library(_source()), S.names()
    assert len(rows) == len(set(rows)), sorted(n for n in rows if rows.count(n) > 1)
    assert read == set(rows), {"read but no row": sorted(read - set(rows)), "row but never read": sorted(set(rows) - read)}


def test_a_new_getenv_line_is_noticed():
    """The extraction sees a name added anywhere in the function's body, whichever helper reads it."""
    text = _source()
    head = "WunSwitches w;\n"
    assert head in text
    for line in ('    w.no_dma = getenv("WUN_X") != nullptr;\n', '    if (set("WUN_X2")) w.win_tk = 32;\n'):
        added = names_read_by_the_library(text.replace(head, head + line, 1)) - set(S.names())
        assert len(added) == 1 and added.pop().startswith("WUN_X")


def test_the_struct_documents_every_switch():
    """struct WunSwitches (wun_internal.h) names each switch next to the field it sets."""
    text = open(os.path.join(CSRC, "wun_internal.h")).read()
    m = re.search(r"struct WunSwitches \{(.*?)^\};", text, re.S | re.M)
    assert m
    assert set(re.findall(r"\b(WUN_[A-Z0-9_]+)\b", m.group(1))) == set(S.names())


def test_tested_rows_name_cases_and_evidence():
    doc = S.__doc__
    for r in S.ROWS:
        assert r.cls in S.TESTED + (S.OWNED, S.NOT_LAUNCH), r
        assert r.note, r.name
        if r.cls in S.TESTED:
            assert r.values and all(isinstance(v, str) and v for v in r.values), r.name
            assert [c for c in S.CASES if S.applies(r, c)], (r.name, "applies to no case")
            assert r.evidence and re.search(r"^  %s\s" % re.escape(r.evidence), doc, re.M), (r.name, "evidence kind not described")
            assert r.where and os.path.exists(os.path.join(ROOT, r.where)), r
        elif r.cls == S.OWNED:
            assert not r.values and os.path.exists(os.path.join(ROOT, r.where)), r
            assert r.name in open(os.path.join(ROOT, r.where)).read(), (r.name, "not named by the file that owns it")
        else:
            assert not r.values and r.where is None, r


def test_every_tested_value_is_named_by_the_gpu_file_or_the_table():
    """The plan tier is generated from the table; the operator tier names its switches itself."""
    text = open(os.path.join(ROOT, S.HERE)).read()
    for name in ("WUN_WIN_TK", "WUN_NO_NARROW_STREAM", "WUN_NARROW_SPLITS", "WUN_NO_K3", "WUN_BF16_LDS_CAP"):
        assert '"%s"' % name in text, name
    for r in S.ROWS:
        if r.evidence == "operator":
            assert '"%s"' % r.name in text, r.name


def test_parse_edges_and_extras_refer_to_rows_and_cases():
    keys = {c.key for c in S.CASES}
    for name, value, why in S.PARSE_EDGES:
        assert S.row(name).cls in S.TESTED and value not in S.row(name).values and why
    assert set(S.PARSE_EDGE_CASES) <= keys
    assert {c.mode for c in S.CASES if c.key in S.PARSE_EDGE_CASES} == {"fp32", "bf16"}
    for name, cases in S.SCHEDULE_EXTRA.items():
        assert S.row(name).cls == S.SCHEDULE and set(cases) <= keys
        assert {c.mode for c in S.CASES if c.key in cases} == {"fp32", "bf16"}
    assert all(S.row(n).cls == S.FORWARD for n in S.FORWARD_EQUAL)
    for cls in S.TESTED:
        assert S.plan_matrix(cls)
