"""--spectrum without a GPU: the two table formatters (host only), the refusals (one line, before the device is opened and
before a file is written), the pinned --help and the option's own paragraph, the new structs, and the numpy model against
the definition taken one k-mer at a time."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np

import helpers as H
import spectrum_model as SM

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import record_cli_transcripts as R  # noqa: E402

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
HEADER = os.path.join(H.ROOT, "include", "ntedit_hip.h")
E_ARG, E_OVERFLOW = -1, -4


def _inputs(tmp_path):
    draft, bf = tmp_path / "d.fa", tmp_path / "f.bf"
    draft.write_text(">a\nACGT\n")
    bf.write_text("not a filter: only its being readable is looked at before the refusal\n")
    return str(draft), str(bf)


def test_spectrum_rows_as_text():
    from ntedit_amd import _lib
    lib = _lib.load()
    assert lib.ntedit_hip_spectrum_header() == b"multiplicity\tbefore\tafter\n"
    buf = ctypes.create_string_buffer(128)
    assert lib.ntedit_hip_spectrum_format_row(0, 17, 3, buf, len(buf)) == 0 and buf.value == b"0\t17\t3\n"
    assert lib.ntedit_hip_spectrum_format_row(255, 2 ** 64 - 1, 0, buf, len(buf)) == 0
    assert buf.value == b"255\t18446744073709551615\t0\n"
    assert lib.ntedit_hip_spectrum_format_row(256, 1, 1, buf, len(buf)) == E_ARG
    # a buffer that is too small is refused, not overrun
    small = ctypes.create_string_buffer(b"\x7f" * 16, 16)
    assert lib.ntedit_hip_spectrum_format_row(255, 2 ** 64 - 1, 2 ** 64 - 1, small, 8) == E_OVERFLOW
    assert small.raw == b"\x7f" * 16
    assert lib.ntedit_hip_spectrum_format_row(7, 1, 2, small, 6) == E_OVERFLOW  # (6 characters and the terminator)
    assert lib.ntedit_hip_spectrum_format_row(7, 1, 2, small, 7) == 0 and small.value == b"7\t1\t2\n"


def _depth(name, fields, cap=512):
    from ntedit_amd import _lib
    lib = _lib.load()
    row = _lib.DepthRow(*fields)
    buf = ctypes.create_string_buffer(cap)
    return lib.ntedit_hip_depth_format_row(name, ctypes.byref(row), buf, cap), buf.value


def test_depth_rows_as_text():
    from ntedit_amd import _lib
    lib = _lib.load()
    assert lib.ntedit_hip_depth_header() == \
        b"name\tkmers_before\tmean_before\tsaturated_before\tkmers_after\tmean_after\tsaturated_after\n"
    # the name is cut at its first space or tab; mean = sum / kmers, two decimals
    assert _depth(b"chr1 some description", (100, 3050, 2, 101, 3131, 0)) == (0, b"chr1\t100\t30.50\t2\t101\t31.00\t0\n")
    assert _depth(b"ctg7\tlen=100 x", (3, 1, 0, 3, 2, 0)) == (0, b"ctg7\t3\t0.33\t0\t3\t0.67\t0\n")
    # no k-mers: NA, on either side alone
    assert _depth(b"short", (0, 0, 0, 0, 0, 0)) == (0, b"short\t0\tNA\t0\t0\tNA\t0\n")
    assert _depth(b"grown", (0, 0, 0, 4, 1020, 4)) == (0, b"grown\t0\tNA\t0\t4\t255.00\t4\n")
    # the last row of the table
    assert _depth(b"#total", (10 ** 12, 31 * 10 ** 12, 5, 10 ** 12, 32 * 10 ** 12, 6)) == \
        (0, b"#total\t1000000000000\t31.00\t5\t1000000000000\t32.00\t6\n")
    # a buffer that is too small is refused, not overrun
    rc, text = _depth(b"a_long_sequence_name", (1, 2, 3, 4, 5, 6), cap=16)
    assert rc == E_OVERFLOW and text == b""
    assert lib.ntedit_hip_depth_format_row(None, None, None, 0) == E_ARG


def test_structs_match_the_header():
    from ntedit_amd import _lib
    text = open(HEADER).read()
    ctype = {"uint64_t": ctypes.c_uint64, "float": ctypes.c_float}
    for name, mirror, size in (("ntedit_hip_depth_row", _lib.DepthRow, 48), ("ntedit_hip_spectrum_stats", _lib.SpectrumStats, 24)):
        body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), text, re.S).group(1)
        fields = []
        for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
            if decl.strip():
                typ, rest = decl.strip().split(None, 1)
                for f in rest.split(","):
                    m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", f.strip())
                    fields.append((m.group(1), ctype[typ] * int(m.group(2)) if m.group(2) else ctype[typ]))
        assert fields == list(mirror._fields_), name
        assert ctypes.sizeof(mirror) == size, name
    assert np.dtype(_lib.DEPTH_DTYPE).itemsize == 48 and np.dtype(_lib.SPECTRUM_ROW_DTYPE).itemsize == 24 == SM.ROW_DTYPE.itemsize


def test_the_switch_is_no_sixth_apply_flag():
    flags = re.findall(r"#define NTEDIT_HIP_APPLY_[A-Z]+ \d+u", open(HEADER).read())
    assert len(flags) == 5, flags
    assert "ntedit_hip_set_spectrum" in open(HEADER).read()


def _refused(args, tmp_path):
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode != 0
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(lines) == 1, r.stderr
    assert "no usable HIP device" not in r.stderr
    assert not list(tmp_path.glob("o*"))
    return lines[0]


def test_spectrum_with_shard_is_refused(tmp_path):
    draft, bf = _inputs(tmp_path)
    line = _refused([NTEDIT, "-f", draft, "-r", bf, "-b", str(tmp_path / "o"), "--spectrum", "--shard", "0/2"], tmp_path)
    assert "--spectrum" in line and "--shard" in line
    # behind the older refusal of --qv --shard
    line = _refused([NTEDIT, "-f", draft, "-r", bf, "-b", str(tmp_path / "o"), "--spectrum", "--qv", "--shard", "0/2"], tmp_path)
    assert "--qv and --shard" in line and "--spectrum" not in line


def test_spectrum_with_genome_is_refused(tmp_path):
    draft, bf = _inputs(tmp_path)
    line = _refused([NTEDIT, "-f", draft, "--genome", draft, "-b", str(tmp_path / "o"), "--spectrum"], tmp_path)
    assert "--spectrum" in line and "--genome" in line and "counting" in line


def test_spectrum_with_reads_without_counts_is_refused(tmp_path):
    draft, bf = _inputs(tmp_path)
    line = _refused([NTEDIT, "-f", draft, "--reads", draft, "-k", "25", "-b", str(tmp_path / "o"), "--spectrum"], tmp_path)
    assert "--spectrum" in line and "--counts" in line
    # with --counts the option passes its own rules: whatever ends the run without a device, it is not this refusal
    r = subprocess.run([NTEDIT, "-f", draft, "--reads", draft, "-k", "25", "--counts", "-b", str(tmp_path / "o"), "--spectrum"],
                       capture_output=True, text=True)
    assert "--spectrum" not in r.stderr


def test_run_spectrum_is_refused(tmp_path):
    draft, bf = _inputs(tmp_path)
    r = subprocess.run([sys.executable, "-m", "ntedit_amd.run", "-f", draft, "-r", bf, "--spectrum"], capture_output=True, text=True,
                       cwd=H.ROOT)
    assert r.returncode == 1
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(lines) == 1 and "--spectrum" in lines[0] and "one GPU" in lines[0], r.stderr
    # ... behind the older ones
    for older in ("--qv", "--bgzip", "--bed"):
        r = subprocess.run([sys.executable, "-m", "ntedit_amd.run", "-f", draft, "-r", bf, "--spectrum", older], capture_output=True,
                           text=True, cwd=H.ROOT)
        assert r.returncode == 1 and older + ":" in r.stderr and "--spectrum:" not in r.stderr, older


def test_help_is_the_recorded_one_and_the_option_has_its_own_paragraph():
    gold = {c["name"]: c for c in json.load(open(R.GOLDEN))["cases"]}["help"]
    r = subprocess.run([NTEDIT, "--help"], capture_output=True, text=True)
    assert (r.returncode, r.stdout, r.stderr) == (gold["status"], gold["stdout"], gold["stderr"])
    assert "--spectrum" not in r.stderr
    r = subprocess.run([NTEDIT, "--help-spectrum"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == ""
    for word in ("--spectrum", "_spectrum.tsv", "_depth.tsv", "--counts", "--shard", "--report", "--help-spectrum"):
        assert word in r.stderr, word


def test_model_against_the_definition():
    """300 bases with an N, an R, lower case and a repeat; h = 3, 4099 counters (no power of two)"""
    rng = np.random.default_rng(913)
    k, h, counters = 25, 3, 4099
    seq = bytearray(H.random_genome(rng, 300))
    seq[40] = ord("N")
    seq[97] = ord("R")
    seq[120:160] = bytes(seq[120:160]).lower()
    seq[230:270] = seq[180:220]
    seq = bytes(seq)
    data = SM.counting_filter([seq[:200].upper().replace(b"N", b"A").replace(b"R", b"C")], k, h, counters, lambda i: 1 + (i * 37) % 255)
    bins, rows = SM.spectrum([seq, seq[:k - 1], b""], data, k, h)
    want_bins, n, total, sat = SM.brute_force(seq, data, k, h)
    assert bins.tolist() == want_bins and n == 300 - k + 1 - 2 * k  # (two bad bytes, k windows each)
    assert tuple(rows[0]) == (n, total, sat) and tuple(rows[1]) == (0, 0, 0) and tuple(rows[2]) == (0, 0, 0)
    assert bins[0] > 0 and int((bins[1:] > 0).sum()) >= 5
    assert int(bins.sum()) == int(rows["kmers"].sum()) and int((np.arange(256) * bins).sum()) == int(rows["sum"].sum())
    assert int(rows["saturated"].sum()) == int(bins[255])
