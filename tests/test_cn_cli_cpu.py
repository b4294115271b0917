"""--spectrum --cn without a GPU: the refusals (one line, before the device is opened and before a file is written), the
option's own paragraph and the pinned --help, the host-only formatters and ntedit_hip_cn_distinct, the new structs, and
the numpy model against the definition taken one k-mer at a time with a dictionary of canonical k-mers."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np

import cn_model as CM
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


def _refused(args, tmp_path):
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode != 0
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(lines) == 1, r.stderr
    assert "no usable HIP device" not in r.stderr
    assert not list(tmp_path.glob("o*"))
    return lines[0]


def test_cn_without_spectrum_is_refused(tmp_path):
    draft, bf = _inputs(tmp_path)
    line = _refused([NTEDIT, "-f", draft, "-r", bf, "-b", str(tmp_path / "o"), "--cn"], tmp_path)
    assert "--cn" in line and "--spectrum" in line


def test_cn_settings_without_cn_are_refused(tmp_path):
    draft, bf = _inputs(tmp_path)
    base = [NTEDIT, "-f", draft, "-r", bf, "-b", str(tmp_path / "o"), "--spectrum"]
    line = _refused(base + ["--cn_store", "1000000"], tmp_path)
    assert "--cn_store" in line and "--cn" in line
    line = _refused(base + ["--cn_sketch", str(1 << 22)], tmp_path)
    assert "--cn_sketch" in line and "--cn" in line


def test_cn_sketch_must_be_a_power_of_two_in_range(tmp_path):
    draft, bf = _inputs(tmp_path)
    base = [NTEDIT, "-f", draft, "-r", bf, "-b", str(tmp_path / "o"), "--spectrum", "--cn", "--cn_sketch"]
    for bad in (str(3 << 20), str((1 << 22) + 1), str(1 << 19), str(1 << 37), "0", "-4", "many", ""):
        line = _refused(base + [bad], tmp_path)
        assert "--cn_sketch" in line and "power of two" in line, bad
    # a size in range passes the option's own rules: whatever ends the run without a device, it is not this refusal
    for good in (str(1 << 20), str(1 << 36)):
        r = subprocess.run(base + [good], capture_output=True, text=True)
        assert "--cn_sketch" not in r.stderr, good
    line = _refused(base[:-1] + ["--cn_store", "lots"], tmp_path)
    assert "--cn_store" in line


def test_everything_spectrum_refuses_is_refused_first(tmp_path):
    draft, bf = _inputs(tmp_path)
    out = ["-b", str(tmp_path / "o")]
    line = _refused([NTEDIT, "-f", draft, "-r", bf, *out, "--spectrum", "--cn", "--shard", "0/2"], tmp_path)
    assert "--spectrum" in line and "--shard" in line and "--cn" not in line.replace("--cn_", "")
    line = _refused([NTEDIT, "-f", draft, "--genome", draft, *out, "--spectrum", "--cn"], tmp_path)
    assert "--spectrum" in line and "--genome" in line
    line = _refused([NTEDIT, "-f", draft, "--reads", draft, "-k", "25", *out, "--spectrum", "--cn"], tmp_path)
    assert "--spectrum" in line and "--counts" in line
    # ... and behind those, --cn's own rule still holds where --spectrum is missing
    line = _refused([NTEDIT, "-f", draft, "-r", bf, *out, "--cn", "--shard", "0/2"], tmp_path)
    assert "--cn" in line and "--spectrum" in line


def test_run_cn_is_refused(tmp_path):
    draft, bf = _inputs(tmp_path)
    r = subprocess.run([sys.executable, "-m", "ntedit_amd.run", "-f", draft, "-r", bf, "--cn"], capture_output=True, text=True, cwd=H.ROOT)
    assert r.returncode == 1
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(lines) == 1 and "--cn" in lines[0] and "one GPU" in lines[0], r.stderr
    # ... behind the older ones
    for older in ("--qv", "--bgzip", "--bed", "--spectrum"):
        r = subprocess.run([sys.executable, "-m", "ntedit_amd.run", "-f", draft, "-r", bf, "--cn", older], capture_output=True, text=True,
                           cwd=H.ROOT)
        assert r.returncode == 1 and older + ":" in r.stderr and "--cn:" not in r.stderr, older


def test_help_is_the_recorded_one_and_the_option_has_its_own_paragraph():
    gold = {c["name"]: c for c in json.load(open(R.GOLDEN))["cases"]}["help"]
    r = subprocess.run([NTEDIT, "--help"], capture_output=True, text=True)
    assert (r.returncode, r.stdout, r.stderr) == (gold["status"], gold["stdout"], gold["stderr"])
    assert "--cn" not in r.stderr
    r = subprocess.run([NTEDIT, "--help-cn"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == ""
    for word in ("--cn", "--spectrum", "--cn_store", "--cn_sketch", "_spectrum_cn.tsv", "_cn_contigs.tsv", "5plus", "h = 1", "--report",
                 "--completeness", "--help-cn"):
        assert word in r.stderr, word


def test_tables_as_text():
    from ntedit_amd import _lib
    lib = _lib.load()
    assert lib.ntedit_hip_cn_header() == ("multiplicity\t" + "\t".join("%s_cn%s" % (s, c) for s in ("before", "after")
                                                                    for c in ("1", "2", "3", "4", "5plus")) + "\n").encode()
    d0 = np.arange(5 * 256, dtype=np.uint64).reshape(5, 256)
    d1 = d0 * np.uint64(3)
    d1[4][255] = 2 ** 64 - 1
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    buf = ctypes.create_string_buffer(512)
    assert lib.ntedit_hip_cn_format_row(7, ptr(d0), ptr(d1), buf, len(buf)) == 0
    assert buf.value == b"7\t7\t263\t519\t775\t1031\t21\t789\t1557\t2325\t3093\n"
    assert lib.ntedit_hip_cn_format_row(255, ptr(d0), ptr(d1), buf, len(buf)) == 0
    assert buf.value.endswith(b"\t18446744073709551615\n") and buf.value.startswith(b"255\t255\t511\t")
    assert lib.ntedit_hip_cn_format_row(256, ptr(d0), ptr(d1), buf, len(buf)) == E_ARG
    assert lib.ntedit_hip_cn_format_row(1, None, ptr(d1), buf, len(buf)) == E_ARG
    small = ctypes.create_string_buffer(b"\x7f" * 16, 16)
    assert lib.ntedit_hip_cn_format_row(255, ptr(d0), ptr(d1), small, 8) == E_OVERFLOW and small.raw == b"\x7f" * 16
    # the contig rows: the name cut at its first space or tab, kmers and five classes of either side
    assert lib.ntedit_hip_cn_contig_header() == ("name\t" + "\t".join("%s_%s" % ((f, s) if f == "kmers" else (s, f)) for s in ("before", "after")
                                                                      for f in ("kmers", "cn1", "cn2", "cn3", "cn4", "cn5plus")) + "\n").encode()
    a, b = _lib.CnRow(100, 90, 4, 3, 0, 3), _lib.CnRow(101, 101, 0, 0, 0, 0)
    assert lib.ntedit_hip_cn_contig_format_row(b"chr1 some description", ctypes.byref(a), ctypes.byref(b), buf, len(buf)) == 0
    assert buf.value == b"chr1\t100\t90\t4\t3\t0\t3\t101\t101\t0\t0\t0\t0\n"
    assert lib.ntedit_hip_cn_contig_format_row(b"#total", ctypes.byref(a), ctypes.byref(a), buf, len(buf)) == 0
    assert buf.value == b"#total\t100\t90\t4\t3\t0\t3\t100\t90\t4\t3\t0\t3\n"
    assert lib.ntedit_hip_cn_contig_format_row(b"a_long_sequence_name", ctypes.byref(a), ctypes.byref(b), small, 16) == E_OVERFLOW
    assert lib.ntedit_hip_cn_contig_format_row(None, None, None, None, 0) == E_ARG


def test_distinct_from_occurrences():
    """(occ + c / 2) / c for the classes 1 .. 4, (w5 + 2^31) >> 32 for 5plus, in 64-bit integers"""
    from ntedit_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(914)
    occ = rng.integers(0, 1 << 40, size=(5, 256), dtype=np.uint64)
    occ[:, 0] = [0, 1, 1, 2, 9]
    occ[:, 1] = [2 ** 63, 2 ** 63 + 1, 2 ** 63 + 2, 2 ** 63 + 2, 1]
    w5 = rng.integers(0, 1 << 62, size=256, dtype=np.uint64)
    w5[:4] = [0, (1 << 31) - 1, 1 << 31, 376 * int(CM.RECIP[255])]
    out = np.zeros((5, 256), dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.ntedit_hip_cn_distinct(ptr(occ), ptr(w5), ptr(out)) == 0
    assert (out == CM.distinct(occ, w5)).all()
    for c in range(1, 5):
        assert out[c - 1].tolist() == [(int(x) + c // 2) // c for x in occ[c - 1]]
    assert out[4].tolist() == [(int(x) + (1 << 31)) >> 32 for x in w5]
    assert out[4][:4].tolist() == [0, 0, 1, 1]  # (376 occurrences at "255 or more": 1.47 k-mers, one)
    assert lib.ntedit_hip_cn_distinct(None, ptr(w5), ptr(out)) == E_ARG


def test_structs_match_the_header():
    from ntedit_amd import _lib
    text = open(HEADER).read()
    ctype = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float}
    for name, mirror, size in (("ntedit_hip_cn_row", _lib.CnRow, 48), ("ntedit_hip_cn_stats", _lib.CnStats, 104)):
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
    assert np.dtype(_lib.CN_ROW_DTYPE).itemsize == 48 == CM.ROW_DTYPE.itemsize
    for name, value in (("OFF", 0), ("ON", 1), ("OVER_CAP", 2), ("NO_MEMORY", 3)):
        assert re.search(r"#define NTEDIT_CN_%s %d\b" % (name, value), text) and getattr(_lib, "CN_" + name) == value
    assert "#define NTEDIT_CN_STORE_DEFAULT (32ull << 30)" in text and _lib.CN_STORE_DEFAULT == 32 << 30
    # a switch of its own: no sixth apply flag, no existing struct grew
    assert len(re.findall(r"#define NTEDIT_HIP_APPLY_[A-Z]+ \d+u", text)) == 5
    assert ctypes.sizeof(_lib.DepthRow) == 48 and ctypes.sizeof(_lib.SpectrumStats) == 24


def test_model_against_the_definition():
    """two batches of a small draft with a repeat on both strands, an N, lower case, a run of 300 A and a short entry: the
    numpy model with a sketch without collisions equals the dictionary of canonical k-mers, whatever the batching"""
    rng = np.random.default_rng(915)
    k, h, counters, sketch = 25, 3, 4099, 1 << 22
    g = bytearray(H.random_genome(rng, 3000))
    g[40] = ord("N")
    g[1200:1300] = bytes(g[1200:1300]).lower()
    g[2000:2200] = CM.revcomp(bytes(g[300:500]))
    g[2500:2600] = g[300:400]
    a, b, c = bytes(g[:1700]), bytes(g[1700:]), b"A" * 300
    data = SM.counting_filter([a, b], k, h, counters, lambda i: (i * 37) % 256)
    one, two = CM.side([[a, b, c, a[:k - 1]]], data, k, h, sketch), CM.side([[a], [b, c], [a[:k - 1]]], data, k, h, sketch)
    for x, y in zip(one, two):
        assert (np.asarray(x) == np.asarray(y)).all()
    occ, w5, rows = CM.brute_force([[a, b, c, a[:k - 1]]], data, k, h)
    assert one[0].tolist() == occ and one[1].tolist() == w5 and [tuple(int(v) for v in r) for r in one[2]] == rows
    classes = one[0].sum(axis=1).tolist()
    # (a flank base that happens to match extends a copy by one k-mer: class 2 holds the 100 k-mers made here, or a few more)
    assert classes[0] > 0 and 2 * 100 <= classes[1] <= 2 * 110 and classes[1] % 2 == 0 and classes[2] == 3 * 76 and classes[3] == 0, classes
    assert classes[4] == 276
    assert one[1].astype(object).sum() == 276 * int(CM.RECIP[255])
    assert tuple(one[2][3]) == (0, 0, 0, 0, 0, 0)
    # the identities: the classes sum to the plain spectrum, the rows to the table
    bins, depth = SM.spectrum([a, b, c, a[:k - 1]], data, k, h)
    assert (one[0].sum(axis=0) == bins).all() and (one[2]["kmers"] == depth["kmers"]).all()
    for ci, f in enumerate(("cn1", "cn2", "cn3", "cn4", "cn5plus")):
        assert int(one[0][ci].sum()) == int(one[2][f].sum())
    for ci in range(1, 5):
        assert not (one[0][ci - 1] % np.uint64(ci)).any()
    # a sketch of 64 counters is all collisions: never below the truth
    tiny = CM.side_sketch([[a, b, c]], k, h, 1 << 6)
    counts, per_entry = CM.exact_counts([[a, b, c]], k)
    for e, words in zip((a, b, c), per_entry):
        assert (CM.copy_numbers(e, tiny, k, h) >= np.array([min(counts[w], 255) for w in words])).all()
