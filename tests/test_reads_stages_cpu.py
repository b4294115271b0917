"""The two host-only seams of the reads filter build, without a GPU: the decide stage (ntedit_hip_reads_stage_decide: from
the histogram bins to the cutoff, the size, the --hist file and the refusals) against the three calls it is made of,
composed by hand; and the reads-option rules (ntedit_hip_reads_options_check) in both dialects, against the messages and
the order the four front ends had when each carried its own copy (the strings below are copied from those sources)."""
import ctypes
import os
import re

import numpy as np
import pytest

import helpers as H


@pytest.fixture(scope="module")
def lib():
    from ntedit_amd import _lib
    return _lib.load()


def u64(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def occ_of(f):
    """bins whose summary is f: occ[c] = c * f[c]"""
    occ = np.zeros(256, dtype=np.uint64)
    for c, n in f.items():
        occ[c] = c * n
    return occ


def by_hand(lib, occ, hashes, fpr, cmin=None):
    """(f, F0, F1, cutoff or None, bytes sized from the histogram) through hist_summary, solid_cutoff and bf_size"""
    f = np.zeros(256, dtype=np.uint64)
    F0, F1, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
    assert lib.ntedit_hip_reads_hist_summary(u64(occ), u64(f), ctypes.byref(F0), ctypes.byref(F1)) == 0
    cut = c.value if lib.ntedit_hip_reads_solid_cutoff(u64(f), ctypes.byref(c)) == 0 else None
    at = cmin if cmin is not None else cut
    size = None if at is None else lib.ntedit_hip_reads_bf_size(int(f[at:].sum()), hashes, fpr)
    return f, F0.value, F1.value, cut, size


def decide(lib, occ, rank=0, **kw):
    """-> (status, result, message, [(to_stdout, line)])"""
    from ntedit_amd import _lib
    lines = []
    log = _lib.READS_LOG_FN(lambda user, to_stdout, line: lines.append((to_stdout, line.decode())))
    files = (ctypes.c_char_p * 1)(b"reads.fa")
    a = dict(files=files, n_files=1, k=25, hash_num=3, cmin=2, fpr=0.01, batch_bytes=1 << 20, log=log, rank=rank, world=2)
    a.update(kw)
    res = _lib.ReadsBuildResult()
    rc = lib.ntedit_hip_reads_stage_decide(_lib.ReadsBuildArgs(**a), None if occ is None else u64(occ), res)
    return rc, res, lib.ntedit_hip_reads_last_error(None).decode() if rc else "", lines


VALLEY = {1: 100000, 2: 20000, 3: 5000, 4: 8000, 5: 30000, 6: 50000, 7: 30000, 8: 9000, 255: 12}
NO_VALLEY = {c: 4000 // c for c in range(1, 256)}
NO_VALLEY_TEXT = "--solid: the k-mer histogram has no valley after the error peak (no c with f[c+1] > f[c]); pass -c"


def test_a_clear_valley_gives_the_cutoff_and_the_size(lib):
    occ = occ_of(VALLEY)
    f, F0, F1, cut, size = by_hand(lib, occ, 3, 0.01)
    assert cut == 3 and size > 0
    rc, res, _, lines = decide(lib, occ, solid=1, cmin=0, bf_bytes=0)
    assert (rc, res.cmin, res.bf_bytes) == (0, cut, size)
    text = [line for _, line in lines]
    assert "k-mer histogram: F1 = %d (k-mers), F0 = %d (distinct k-mers)" % (F1, F0) in text
    assert "--solid: minimum k-mer count 3" in text
    assert ("Sized from the k-mer histogram: --num_elements %d (k-mers at 3 or above), %d bytes"
            % (int(f[3:].sum()), size)) in text
    assert (1, "BF size (bytes): %d" % size) in lines
    # a rank other than 0 decides the same and says nothing
    rc, res, _, lines = decide(lib, occ, rank=1, solid=1, cmin=0, bf_bytes=0)
    assert (rc, res.cmin, res.bf_bytes, lines) == (0, cut, size, [])


def test_a_given_cutoff_sizes_from_its_own_bin_on(lib):
    occ = occ_of(VALLEY)
    _, _, _, _, size = by_hand(lib, occ, 4, 0.02, cmin=5)
    rc, res, _, _ = decide(lib, occ, cmin=5, hash_num=4, fpr=0.02, bf_bytes=0, hist_path=os.devnull.encode())
    assert (rc, res.cmin, res.bf_bytes) == (0, 5, size)


def test_no_valley_refuses_solid_after_the_hist_file_is_written(lib, tmp_path):
    from ntedit_amd import _lib
    occ = occ_of(NO_VALLEY)
    f, F0, F1, cut, _ = by_hand(lib, occ, 3, 0.01)
    assert cut is None
    want, got = tmp_path / "want.hist", tmp_path / "got.hist"
    assert lib.ntedit_hip_reads_write_hist(str(want).encode(), u64(f), F0, F1) == 0
    for rank in (0, 1):
        rc, _, why, _ = decide(lib, occ, rank=rank, solid=1, cmin=0, bf_bytes=4096, hist_path=str(got).encode())
        assert (rc, why) == (_lib.E_ARG, NO_VALLEY_TEXT)
        if rank == 0:
            assert got.read_bytes() == want.read_bytes()
            got.unlink()
        else:
            assert not got.exists()  # (only rank 0 writes it)
    rc, _, why, _ = decide(lib, occ, solid=1, cmin=0, bf_bytes=0)
    assert (rc, why) == (_lib.E_ARG, NO_VALLEY_TEXT)


def test_nothing_at_the_cutoff_or_above_would_be_empty(lib):
    from ntedit_amd import _lib
    occ = occ_of({1: 1000, 2: 300, 3: 20})
    assert by_hand(lib, occ, 3, 0.01, cmin=4)[4] == 0
    for rank in (0, 1):
        rc, _, why, _ = decide(lib, occ, rank=rank, cmin=4, bf_bytes=0, hist_path=os.devnull.encode())
        assert (rc, why) == (_lib.E_ARG, "The output filter would be empty (no k-mer at the minimum count or above).")


def test_a_given_size_is_not_touched_by_the_histogram(lib, tmp_path):
    from ntedit_amd import _lib
    occ = occ_of(VALLEY)
    f, F0, F1, cut, _ = by_hand(lib, occ, 3, 0.01)
    want, got = tmp_path / "want.hist", tmp_path / "got.hist"
    assert lib.ntedit_hip_reads_write_hist(str(want).encode(), u64(f), F0, F1) == 0
    # --hist without --solid: the cutoff as given; with --solid: the valley's; the same file either way
    for solid, cmin in ((0, 7), (1, cut)):
        rc, res, _, lines = decide(lib, occ, solid=solid, cmin=0 if solid else 7, bf_bytes=4096, hist_path=str(got).encode())
        assert (rc, res.cmin, res.bf_bytes) == (0, cmin, 4096)
        assert got.read_bytes() == want.read_bytes()
        assert (0, "Histogram written to %s" % got) in lines and not any("Sized from" in line for _, line in lines)
        got.unlink()
    # no histogram at all: the arguments pass through, and an empty size is refused in the words of the sizing
    rc, res, _, lines = decide(lib, None, cmin=9, bf_bytes=12345)
    assert (rc, res.cmin, res.bf_bytes, lines) == (0, 9, 12345, [])
    assert decide(lib, None, cmin=9, bf_bytes=0)[0] == _lib.E_ARG  # (no histogram to size from)
    assert decide(lib, None, solid=1, cmin=0, bf_bytes=4096)[0] == _lib.E_ARG


# ------------------------------------------------------------------ the option rules
def check(lib, dialect, final=1, files=(), solid=False, hist=False, **texts):
    from ntedit_amd import _lib
    arr = (ctypes.c_char_p * max(1, len(files)))(*[os.fsencode(str(f)) for f in files])
    o = _lib.ReadsOptions(solid=solid, hist=hist, files=arr, n_files=len(files),
                          **{k: v.encode() for k, v in texts.items()})
    r = _lib.ReadsRules()
    rc = lib.ntedit_hip_reads_options_check(o, dialect, final, r)
    return rc, lib.ntedit_hip_reads_last_error(None).decode() if rc else "", r


GOOD = dict(k="25", cutoff="2", bf="4096")
SIZE = ("--bf or --num_elements: one of them is required (or --solid / --hist, which size the filter from the k-mer "
        "histogram)")
ONE_OF = ": give one of them (--solid takes the minimum count from the k-mer histogram)"
REFUSED, NOT_A_NUMBER, EMPTY = 1, 2, 3

# (options, solid, the tool's status and message, the polisher's)
RULES = [
    (dict(cutoff="2", bf="4096"), False, REFUSED, "-k: required.", REFUSED, "-k: required with --reads"),
    (dict(GOOD, k="11"), False, REFUSED, "-k 11: k must be between 12 and 200.", REFUSED, "-k 11: k must be between 12 and 200"),
    (dict(GOOD, k="201"), False, REFUSED, "-k 201: k must be between 12 and 200.", REFUSED, "-k 201: k must be between 12 and 200"),
    (dict(GOOD, k="x25"), False, NOT_A_NUMBER, "-k: not a number: 'x25'", REFUSED, "-k x25: k must be between 12 and 200"),
    (GOOD, True, REFUSED, "--solid and -c" + ONE_OF + ".", REFUSED, "--cutoff and --solid" + ONE_OF),
    (dict(k="25", bf="4096"), False, REFUSED, "-c: required (or --solid).", REFUSED,
     "--cutoff or --solid: one of them is required with --reads"),
    (dict(GOOD, cutoff="0"), False, REFUSED, "-c 0: the minimum count must be between 1 and 255.", REFUSED,
     "--cutoff 0: the minimum count must be between 1 and 255"),
    (dict(GOOD, cutoff="256"), False, REFUSED, "-c 256: the minimum count must be between 1 and 255.", REFUSED,
     "--cutoff 256: the minimum count must be between 1 and 255"),
    (dict(GOOD, cutoff="x"), False, NOT_A_NUMBER, "-c: not a number: 'x'", NOT_A_NUMBER, "invalid option: `--cutoff x'"),
    (dict(GOOD, hashes="0"), False, REFUSED, "--hashes 0: the number of hash functions must be between 1 and 8.", REFUSED,
     "--hashes 0: the number of hash functions must be between 1 and 8"),
    (dict(GOOD, hashes="9"), False, REFUSED, "--hashes 9: the number of hash functions must be between 1 and 8.", REFUSED,
     "--hashes 9: the number of hash functions must be between 1 and 8"),
    (dict(GOOD, fpr="1.5"), False, REFUSED, "--fpr: needs a number between 0 and 1: '1.5'", REFUSED,
     "--fpr 1.5: needs a number between 0 and 1"),
    (dict(GOOD, fpr="0.1x"), False, REFUSED, "--fpr: needs a number between 0 and 1: '0.1x'", REFUSED,
     "--fpr 0.1x: needs a number between 0 and 1"),
    (dict(k="25", cutoff="2"), False, REFUSED, SIZE + ".", REFUSED, SIZE),
    (dict(GOOD, bf="0"), False, EMPTY, "The output filter would be empty (--bf 0 or --num_elements too small).", REFUSED,
     "--bf / --num_elements: the filter would be empty"),
    (dict(k="25", cutoff="2", num_elements="0"), False, EMPTY,
     "The output filter would be empty (--bf 0 or --num_elements too small).", REFUSED,
     "--bf / --num_elements: the filter would be empty"),
    (dict(GOOD, batch_bytes="100"), False, REFUSED, "--batch_bytes: at least 4096.", REFUSED, "--batch_bytes: at least 4096"),
    (dict(GOOD, sketch_bytes="-1"), False, NOT_A_NUMBER, "--sketch_bytes: not a number: '-1'", NOT_A_NUMBER,
     "invalid option: `--sketch_bytes -1'"),
    (dict(GOOD, num_elements="+5"), False, NOT_A_NUMBER, "--num_elements: not a number: '+5'", NOT_A_NUMBER,
     "invalid option: `--num_elements +5'"),
    (dict(GOOD, bf=""), False, NOT_A_NUMBER, "--bf: not a number: ''", NOT_A_NUMBER, "invalid option: `--bf '"),
    # two rules broken at once: the first in the front ends' order
    (dict(GOOD, k="11", cutoff="0"), False, REFUSED, "-k 11: k must be between 12 and 200.", REFUSED,
     "-k 11: k must be between 12 and 200"),
    (dict(k="25", cutoff="2"), True, REFUSED, "--solid and -c" + ONE_OF + ".", REFUSED, "--cutoff and --solid" + ONE_OF),
    (dict(GOOD, cutoff="0", hashes="9"), False, REFUSED, "-c 0: the minimum count must be between 1 and 255.", REFUSED,
     "--cutoff 0: the minimum count must be between 1 and 255"),
    # (the tool says "would be empty" last, after it has printed its parameters; the polisher before --batch_bytes)
    (dict(GOOD, bf="0", batch_bytes="100"), False, REFUSED, "--batch_bytes: at least 4096.", REFUSED,
     "--bf / --num_elements: the filter would be empty"),
]


@pytest.mark.parametrize("texts,solid,tool_rc,tool,polisher_rc,polisher", RULES, ids=[r[3] for r in RULES])
def test_each_rule_refuses_in_both_dialects(lib, texts, solid, tool_rc, tool, polisher_rc, polisher):
    from ntedit_amd import _lib
    assert check(lib, _lib.READS_DIALECT_TOOL, solid=solid, **texts)[:2] == (tool_rc, tool)
    assert check(lib, _lib.READS_DIALECT_POLISHER, solid=solid, **texts)[:2] == (polisher_rc, polisher)


def test_at_the_option_only_the_option_itself_is_refused(lib):
    from ntedit_amd import _lib
    T, P = _lib.READS_DIALECT_TOOL, _lib.READS_DIALECT_POLISHER
    # nothing that needs the whole argument list: no -k, no cutoff, no size, values out of range
    for d in (T, P):
        assert check(lib, d, final=0)[0] == 0
        assert check(lib, d, final=0, k="11", cutoff="0", hashes="9", batch_bytes="1")[0] == 0
    assert check(lib, T, final=0, k="x25")[:2] == (NOT_A_NUMBER, "-k: not a number: 'x25'")
    assert check(lib, P, final=0, k="x25")[0] == 0  # (ntedit takes any -k without --reads)
    assert check(lib, T, final=0, fpr="1.5")[:2] == (REFUSED, "--fpr: needs a number between 0 and 1: '1.5'")
    assert check(lib, P, final=0, store_cap="x")[:2] == (NOT_A_NUMBER, "invalid option: `--resident_cap x'")
    assert check(lib, T, final=0, threads="x")[:2] == (NOT_A_NUMBER, "-t: not a number: 'x'")


def test_the_normalised_arguments_and_the_defaults(lib, tmp_path):
    from ntedit_amd import _lib
    reads = tmp_path / "r.fa"
    reads.write_bytes(b">r\nACGT\n" * 1000)
    files = (ctypes.c_char_p * 1)(str(reads).encode())
    for d in (_lib.READS_DIALECT_TOOL, _lib.READS_DIALECT_POLISHER):
        rc, _, r = check(lib, d, files=[reads], k="31", cutoff="3", num_elements="1000000", fpr="0.02", hashes="4")
        want = lib.ntedit_hip_reads_bf_size(1000000, 4, 0.02)
        assert rc == 0 and (r.k, r.cmin, r.hash_num, r.fpr, r.num_elements, r.bf_bytes) == (31, 3, 4, 0.02, 1000000, want)
        assert (r.gather_hist, r.size_from_hist, r.sketch_bytes, r.threads) == (0, 0, 0, 12)
        assert r.sketch_counters == lib.ntedit_hip_reads_default_sketch(files, 1, want)
        assert (r.batch_bytes, r.store_cap) == (_lib.READS_BATCH_DEFAULT, _lib.READS_RESIDENT_CAP_DEFAULT)
        rc, _, r = check(lib, d, files=[reads], solid=True, hist=True, k="25", sketch_bytes="1000003", store_cap="0",
                         batch_bytes="65536")
        assert rc == 0 and (r.cmin, r.bf_bytes, r.gather_hist, r.size_from_hist) == (0, 0, 1, 1)
        assert (r.sketch_bytes, r.sketch_counters, r.store_cap, r.batch_bytes) == (1000003, 1000003, 0, 65536)
        rc, _, r = check(lib, d, files=[reads], hist=True, k="25", cutoff="2")
        assert rc == 0 and r.sketch_counters == lib.ntedit_hip_reads_default_sketch(files, 1, 0)
    # the values _lib mirrors are the header's
    header = open(os.path.join(H.ROOT, "include", "ntedit_hip.h")).read()
    for name, value in (("BATCH_DEFAULT", _lib.READS_BATCH_DEFAULT), ("RESIDENT_CAP_DEFAULT", _lib.READS_RESIDENT_CAP_DEFAULT),
                        ("GZIP_WEIGHT", _lib.READS_GZIP_WEIGHT), ("DIALECT_TOOL", _lib.READS_DIALECT_TOOL),
                        ("DIALECT_POLISHER", _lib.READS_DIALECT_POLISHER), ("REFUSED", _lib.READS_REFUSED),
                        ("NOT_A_NUMBER", _lib.READS_NOT_A_NUMBER), ("EMPTY", _lib.READS_EMPTY)):
        m = re.search(r"#define NTEDIT_READS_%s \(?(\d+)(?:ull << (\d+)\))?" % name, header)
        assert m and int(m.group(1)) << int(m.group(2) or 0) == value, name
