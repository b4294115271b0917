"""--completeness without a GPU: the estimator, the table's text, the stats struct, the refusals (before any device
call and before any file is written), the usage text."""
import ctypes
import math
import os
import re
import subprocess
import sys

import pytest

import helpers as H
from ntedit_amd import _lib

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
E_ARG, E_OVERFLOW = -1, -4


def card(set_bits, slots, h):
    """the issue's formula, in Python floats (IEEE double)"""
    return -(slots / h) * math.log1p(-set_bits / slots)


@pytest.mark.parametrize("set_bits,slots,h", [(0, 1000, 1), (1, 1 << 35, 1), (123456, 1 << 20, 1), (225000, 1 << 20, 3)])
def test_bloom_cardinality(set_bits, slots, h):
    lib = _lib.load()
    got = lib.ntedit_hip_bloom_cardinality(set_bits, slots, h)
    if set_bits == 0:
        assert got == 0.0
    else:
        assert got == pytest.approx(card(set_bits, slots, h), rel=1e-12)
        assert got >= set_bits / h  # (collisions only hide keys)


@pytest.mark.parametrize("h", [1, 3, 8])
def test_bloom_cardinality_over_h_and_its_special_values(h):
    lib = _lib.load()
    for set_bits, slots in ((0, 1000), (1, 1 << 35), (123456, 1 << 20), (225000, 1 << 20), (999, 1000)):
        got = lib.ntedit_hip_bloom_cardinality(set_bits, slots, h)
        assert got == pytest.approx(card(set_bits, slots, h), rel=1e-12) if set_bits else got == 0.0
    assert lib.ntedit_hip_bloom_cardinality(1000, 1000, h) == float("inf")  # set == slots
    assert lib.ntedit_hip_bloom_cardinality(1001, 1000, h) == float("inf")
    assert math.isnan(lib.ntedit_hip_bloom_cardinality(0, 0, h))            # slots == 0
    assert math.isnan(lib.ntedit_hip_bloom_cardinality(5, 0, h))
    assert math.isnan(lib.ntedit_hip_bloom_cardinality(5, 1000, 0))         # h == 0


def _stats(bits, h, k, filter_set, before, after):
    st = _lib.SharedStats()
    st.bits, st.hash_num, st.k, st.filter_set = bits, h, k, filter_set
    st.shared_set[0], st.shared_set[1] = before, after
    return st


def test_rows_as_text():
    lib = _lib.load()
    assert lib.ntedit_hip_completeness_header().decode() == \
        "stage\tfilter_bits\tfilter_set\tfilter_kmers\tshared_set\tshared_kmers\tcompleteness\n"
    buf = ctypes.create_string_buffer(512)
    bits = 1 << 20
    st = _stats(bits, 3, 25, 225000, 70000, 80000)
    fk = card(225000, bits, 3)
    for which, stage, marked in ((0, b"before", 70000), (1, b"after", 80000)):
        assert lib.ntedit_hip_completeness_format_row(stage, ctypes.byref(st), which, buf, len(buf)) == 0
        sk = card(marked, bits, 1)
        assert buf.value.decode() == "%s\t%d\t225000\t%d\t%d\t%d\t%.6f\n" % (
            stage.decode(), bits, int(math.floor(fk + 0.5)), marked, int(math.floor(sk + 0.5)), sk / fk)
    # not clipped at 1: more distinct draft k-mers than the filter's estimate
    st = _stats(bits, 3, 25, 3000, 2000, 0)
    assert lib.ntedit_hip_completeness_format_row(b"before", ctypes.byref(st), 0, buf, len(buf)) == 0
    assert float(buf.value.decode().rstrip("\n").split("\t")[6]) > 1.0
    # an empty mark array: 0 k-mers, completeness 0
    assert lib.ntedit_hip_completeness_format_row(b"after", ctypes.byref(st), 1, buf, len(buf)) == 0
    assert buf.value.decode().rstrip("\n").split("\t")[4:] == ["0", "0", "0.000000"]


def test_rows_of_saturated_and_empty_arrays_say_NA():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(512)
    bits = 1 << 10
    st = _stats(bits, 3, 25, 500, bits, 17)  # M[0] saturated
    assert lib.ntedit_hip_completeness_format_row(b"before", ctypes.byref(st), 0, buf, len(buf)) == 0
    assert buf.value.decode() == "before\t1024\t500\t%d\t1024\tNA\tNA\n" % int(math.floor(card(500, bits, 3) + 0.5))
    st = _stats(bits, 3, 25, bits, 17, 17)   # the filter saturated
    assert lib.ntedit_hip_completeness_format_row(b"after", ctypes.byref(st), 1, buf, len(buf)) == 0
    assert buf.value.decode() == "after\t1024\t1024\tNA\t17\t%d\tNA\n" % int(math.floor(card(17, bits, 1) + 0.5))
    st = _stats(bits, 3, 25, 0, 0, 0)        # an empty filter: 0 / 0
    assert lib.ntedit_hip_completeness_format_row(b"after", ctypes.byref(st), 1, buf, len(buf)) == 0
    assert buf.value.decode() == "after\t1024\t0\t0\t0\t0\tNA\n"
    st = _stats(0, 3, 25, 0, 0, 0)           # no slots at all
    assert lib.ntedit_hip_completeness_format_row(b"after", ctypes.byref(st), 1, buf, len(buf)) == 0
    assert buf.value.decode() == "after\t0\t0\tNA\t0\tNA\tNA\n"


def test_row_overflow_and_bad_arguments():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(512)
    st = _stats(1 << 20, 3, 25, 225000, 70000, 80000)
    assert lib.ntedit_hip_completeness_format_row(b"before", ctypes.byref(st), 0, buf, 4) == E_OVERFLOW
    assert lib.ntedit_hip_completeness_format_row(b"before", ctypes.byref(st), 2, buf, len(buf)) == E_ARG
    assert lib.ntedit_hip_completeness_format_row(None, ctypes.byref(st), 0, buf, len(buf)) == E_ARG


def test_stats_struct_matches_the_header():
    """ntedit_hip_shared_stats in include/ntedit_hip.h: the fields of the ctypes mirror, in order, at the C offsets"""
    text = open(os.path.join(H.ROOT, "include", "ntedit_hip.h")).read()
    body = re.search(r"typedef struct ntedit_hip_shared_stats\s*\{(.*?)\}\s*ntedit_hip_shared_stats;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, rest = decl.split(None, 1)
            for f in rest.split(","):
                m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", f.strip())
                fields.append((m.group(1), ctype[typ] * int(m.group(2)) if m.group(2) else ctype[typ]))
    assert [f for f, _ in fields] == [f for f, _ in _lib.SharedStats._fields_]
    assert [t for _, t in fields] == [t for _, t in _lib.SharedStats._fields_]
    assert ctypes.sizeof(_lib.SharedStats) == 56
    assert [getattr(_lib.SharedStats, f).offset for f, _ in fields] == [0, 8, 12, 16, 24, 40, 48]
    assert re.search(r"#define NTEDIT_HIP_APPLY_SHARED (\d+)u", text).group(1) == str(_lib.APPLY_SHARED)
    import ntedit_amd
    assert ntedit_amd.APPLY_SHARED == 4 and not (ntedit_amd.APPLY_SHARED & (ntedit_amd.APPLY_QV | ntedit_amd.APPLY_EDITED))


def _refused(tmp_path, extra, needle):
    draft = tmp_path / "d.fa"
    draft.write_text(">a\nACGT\n")
    r = subprocess.run([NTEDIT, "-f", str(draft), "-r", str(tmp_path / "missing.bf"), "-b", str(tmp_path / "o"), "--completeness"] + extra,
                       capture_output=True, text=True)
    assert r.returncode != 0
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(lines) == 1 and "--completeness" in lines[0] and needle in lines[0], r.stderr
    assert not list(tmp_path.glob("o*"))  # (nothing was written; the filter file was never looked at)
    assert "missing.bf" not in r.stderr


def test_completeness_without_qv_is_refused(tmp_path):
    _refused(tmp_path, [], "--qv")


def test_completeness_with_shard_is_refused(tmp_path):
    _refused(tmp_path, ["--qv", "--shard", "0/2"], "--shard")


def test_run_completeness_is_refused(tmp_path):
    draft = tmp_path / "d.fa"
    draft.write_text(">a\nACGT\n")
    r = subprocess.run([sys.executable, "-m", "ntedit_amd.run", "-f", str(draft), "-r", str(tmp_path / "missing.bf"), "--completeness"],
                       capture_output=True, text=True, cwd=H.ROOT)
    assert r.returncode == 1
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(lines) == 1 and "--completeness" in lines[0] and "out of scope" in lines[0], r.stderr
    assert not [p for p in tmp_path.iterdir() if p.name != "d.fa"]


def test_usage_names_completeness():
    r = subprocess.run([NTEDIT, "--help"], capture_output=True, text=True)
    assert "--completeness" in r.stderr + r.stdout
    assert "_completeness.tsv" in r.stderr + r.stdout
