"""The reject filter (ntedit -e) of the reads filter build, without a GPU: the rules of --reject_cutoff, --reject_bf and
--reject_num_elements in ntedit_hip_reads_options_check (both dialects), the decide stage's reject size and its
"R <= cmin" refusal under --solid, and the four front ends' help texts and refusals, all of which come before any
device is opened."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from test_reads_hist_cpu import FIXTURE, read_hist
from test_reads_stages_cpu import GOOD, NOT_A_NUMBER, REFUSED, VALLEY, decide, occ_of, u64

NTEDIT = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
TOOL = os.path.join(H.ROOT, "ntedit_amd", "ntedit-make-reads-bf")


@pytest.fixture(scope="module")
def lib():
    from ntedit_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def binaries():
    if not (os.path.exists(TOOL) and os.path.exists(NTEDIT)):
        subprocess.run(["make", "-s", "-j4", "-C", os.path.join(H.ROOT, "ntedit_amd", "csrc")], check=True)


def check(lib, dialect, final=1, solid=False, hist=False, counts=False, reject_out=False, **texts):
    from ntedit_amd import _lib
    files = (ctypes.c_char_p * 1)(b"reads.fa")
    o = _lib.ReadsOptions(solid=solid, hist=hist, files=files, n_files=1, counts=counts, reject_out=reject_out,
                          **{k: v.encode() for k, v in texts.items()})
    r = _lib.ReadsRules()
    rc = lib.ntedit_hip_reads_options_check(o, dialect, final, r)
    return rc, lib.ntedit_hip_reads_last_error(None).decode() if rc else "", r


REJECT = dict(GOOD, reject_cutoff="40", reject_bf="2048")
REJECT_SIZE = ("--reject_bf or --reject_num_elements: one of them is required with --reject_cutoff (or --solid / --hist, "
               "which size the reject filter from the k-mer histogram)")
COUNTS = "--reject_cutoff and --counts: a counting filter needs no reject filter (ntedit -q sets the maximum count)"

# (options, flags, status, the message without the tool's final period, the polisher's name where the two differ)
RULES = [
    (dict(REJECT, reject_cutoff="x"), {}, NOT_A_NUMBER, None, None),
    (dict(REJECT, reject_bf="-1"), {}, NOT_A_NUMBER, None, None),
    (dict(REJECT, reject_num_elements="1e6"), {}, NOT_A_NUMBER, None, None),
    (dict(REJECT, reject_cutoff="1"), {}, REFUSED, "--reject_cutoff 1: the reject count must be between 2 and 255", None),
    (dict(REJECT, reject_cutoff="0"), {}, REFUSED, "--reject_cutoff 0: the reject count must be between 2 and 255", None),
    (dict(REJECT, reject_cutoff="256"), {}, REFUSED, "--reject_cutoff 256: the reject count must be between 2 and 255", None),
    (dict(REJECT, reject_cutoff="2"), {}, REFUSED, "--reject_cutoff 2: the reject count must be above {cut} 2", None),
    (dict(REJECT, cutoff="50"), {}, REFUSED, "--reject_cutoff 40: the reject count must be above {cut} 50", None),
    (dict(GOOD, reject_bf="2048"), {}, REFUSED, "--reject_bf: only with --reject_cutoff", None),
    (dict(GOOD, reject_num_elements="1000"), {}, REFUSED, "--reject_num_elements: only with --reject_cutoff", None),
    (GOOD, dict(reject_out=True), REFUSED, "--reject_out: only with --reject_cutoff", "--save_reject_bf: only with --reject_cutoff"),
    (dict(GOOD, reject_cutoff="40"), {}, REFUSED, REJECT_SIZE, None),
    (dict(REJECT, reject_bf="0"), {}, REFUSED, "--reject_bf / --reject_num_elements: the reject filter would be empty", None),
    (dict(GOOD, reject_cutoff="40", reject_num_elements="0"), {}, REFUSED,
     "--reject_bf / --reject_num_elements: the reject filter would be empty", None),
    (REJECT, dict(counts=True), REFUSED, COUNTS, None),
    (dict(REJECT, reject_num_elements="1000"), {}, REFUSED, "--reject_bf and --reject_num_elements: give one of them", None),
]


@pytest.mark.parametrize("texts,flags,rc,why,polisher", RULES, ids=[str(i) for i in range(len(RULES))])
def test_each_reject_rule_refuses_in_both_dialects(lib, texts, flags, rc, why, polisher):
    from ntedit_amd import _lib
    got_t = check(lib, _lib.READS_DIALECT_TOOL, **flags, **texts)
    got_p = check(lib, _lib.READS_DIALECT_POLISHER, **flags, **texts)
    assert got_t[0] == got_p[0] == rc
    if rc == NOT_A_NUMBER:
        name = [n for n in ("reject_cutoff", "reject_bf", "reject_num_elements") if texts.get(n) in ("x", "-1", "1e6")][0]
        assert got_t[1] == "--%s: not a number: '%s'" % (name, texts[name])
        assert got_p[1] == "invalid option: `--%s %s'" % (name, texts[name])
        # a malformed number is refused at the option itself, as the other numbers are
        assert check(lib, _lib.READS_DIALECT_TOOL, final=0, **{name: texts[name]})[0] == NOT_A_NUMBER
        assert check(lib, _lib.READS_DIALECT_POLISHER, final=0, **{name: texts[name]})[0] == NOT_A_NUMBER
    else:
        assert got_t[1] == why.format(cut="-c") + "."
        assert got_p[1] == (polisher or why).format(cut="--cutoff")


def test_the_existing_rules_come_first(lib):
    from ntedit_amd import _lib
    for d, dot in ((_lib.READS_DIALECT_TOOL, "."), (_lib.READS_DIALECT_POLISHER, "")):
        rc, why, _ = check(lib, d, **dict(REJECT, k="11", reject_cutoff="1"))
        assert (rc, why) == (REFUSED, "-k 11: k must be between 12 and 200" + dot)
        rc, why, _ = check(lib, d, **dict(REJECT, batch_bytes="100", reject_cutoff="1"))
        assert (rc, why) == (REFUSED, "--batch_bytes: at least 4096" + dot)
        # what needs the whole argument list is not refused at the option
        assert check(lib, d, final=0, reject_cutoff="1", reject_bf="0")[0] == 0


def test_the_normalised_reject_fields_and_the_untouched_defaults(lib):
    from ntedit_amd import _lib
    files = (ctypes.c_char_p * 1)(b"reads.fa")
    for d in (_lib.READS_DIALECT_TOOL, _lib.READS_DIALECT_POLISHER):
        rc, _, plain = check(lib, d, **GOOD)
        assert rc == 0
        assert (plain.reject_cmin, plain.reject_bf_bytes, plain.reject_num_elements, plain.reject_size_from_hist) == (0, 0, 0, 0)
        rc, _, r = check(lib, d, reject_out=True, **REJECT)
        assert rc == 0 and (r.reject_cmin, r.reject_bf_bytes, r.reject_size_from_hist) == (40, 2048, 0)
        # the sketch is sized from the primary output alone, and nothing else moves
        for name, _ in _lib.ReadsRules._fields_:
            if not name.startswith("reject_"):
                assert getattr(r, name) == getattr(plain, name), name
        assert r.sketch_counters == lib.ntedit_hip_reads_default_sketch(files, 1, 4096)
        rc, _, r = check(lib, d, **dict(GOOD, reject_cutoff="255", reject_num_elements="1000000", fpr="0.02", hashes="4"))
        want = lib.ntedit_hip_reads_bf_size(1000000, 4, 0.02)
        assert rc == 0 and (r.reject_cmin, r.reject_num_elements, r.reject_bf_bytes) == (255, 1000000, want) and want > 0
        # sized from the histogram: with --hist or --solid; under --solid "above the cutoff" waits for the decide stage
        rc, _, r = check(lib, d, hist=True, **dict(GOOD, reject_cutoff="3"))
        assert rc == 0 and (r.reject_cmin, r.reject_bf_bytes, r.reject_size_from_hist) == (3, 0, 1)
        rc, _, r = check(lib, d, solid=True, k="25", reject_cutoff="2")
        assert rc == 0 and (r.cmin, r.reject_cmin, r.reject_size_from_hist, r.size_from_hist) == (0, 2, 1, 1)


def test_the_new_calls_are_exported_and_declared(lib):
    from ntedit_amd import _lib
    header = open(os.path.join(H.ROOT, "include", "ntedit_hip.h")).read()
    for name in _lib.EXPORTS_NUMBERED + ["ntedit_hip_reads_set_reject_cutoff"]:
        assert hasattr(lib, name) and ("int %s(ntedit_hip_ctx* ctx, " % name) in header, name
    assert "ntedit_hip_reads_set_reject_cutoff" in _lib.EXPORTS
    # without a context they are argument errors, not crashes
    assert lib.ntedit_hip_filter_insert_solid2(None, b"ACGT", 4, 0, 2, 3) == _lib.E_ARG
    assert lib.ntedit_hip_resident_insert_solid2(None, 2, 3) == _lib.E_ARG
    assert lib.ntedit_hip_reads_set_reject_cutoff(None, 3) == _lib.E_ARG


# ------------------------------------------------------------------ the decide stage
def test_decide_sizes_the_reject_filter_from_the_histogram(lib):
    occ = occ_of(VALLEY)
    f = np.zeros(256, dtype=np.uint64)
    F0, F1 = ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.ntedit_hip_reads_hist_summary(u64(occ), u64(f), ctypes.byref(F0), ctypes.byref(F1)) == 0
    n7 = int(f[7:].sum())
    want = lib.ntedit_hip_reads_bf_size(n7, 3, 0.01)
    assert n7 == 30000 + 9000 + 12 and want > 0
    # --solid finds 3; the primary is sized from 3 on, the reject filter from 7 on
    rc, res, _, lines = decide(lib, occ, solid=1, cmin=0, bf_bytes=0, reject_cmin=7)
    assert (rc, res.cmin, res.reject_bf_bytes) == (0, 3, want)
    assert res.bf_bytes == lib.ntedit_hip_reads_bf_size(int(f[3:].sum()), 3, 0.01)
    text = [line for _, line in lines]
    assert ("Reject filter sized from the k-mer histogram: --reject_num_elements %d (k-mers at 7 or above), %d bytes"
            % (n7, want)) in text
    assert (1, "Reject BF size (bytes): %d" % want) in lines
    # the primary's result is the one of the run without the reject filter
    rc0, res0, _, lines0 = decide(lib, occ, solid=1, cmin=0, bf_bytes=0)
    assert (rc0, res0.cmin, res0.bf_bytes, res0.reject_bf_bytes) == (0, 3, res.bf_bytes, 0)
    assert [l for l in lines if "eject" not in l[1]] == lines0
    # a given size passes through, with or without a histogram; another rank decides the same and says nothing
    rc, res, _, _ = decide(lib, occ, solid=1, cmin=0, bf_bytes=0, reject_cmin=7, reject_bf_bytes=12344)
    assert (rc, res.reject_bf_bytes) == (0, 12344)
    rc, res, _, lines = decide(lib, None, cmin=2, bf_bytes=4096, reject_cmin=7, reject_bf_bytes=999)
    assert (rc, res.cmin, res.bf_bytes, res.reject_bf_bytes, lines) == (0, 2, 4096, 999, [])
    rc, res, _, lines = decide(lib, occ, rank=1, solid=1, cmin=0, bf_bytes=0, reject_cmin=7)
    assert (rc, res.reject_bf_bytes, lines) == (0, want, [])


def test_decide_refuses_a_reject_count_at_or_below_the_cutoff(lib, tmp_path):
    from ntedit_amd import _lib
    # the reference demo's ntCard histogram: --solid finds 5, so 5 is refused and 6 accepted
    _, f = read_hist(FIXTURE)
    occ = np.array([c * int(f[c]) for c in range(256)], dtype=np.uint64)
    hist = tmp_path / "demo.hist"
    for rank in (0, 1):
        rc, res, why, _ = decide(lib, occ, rank=rank, solid=1, cmin=0, bf_bytes=0, reject_cmin=5, hist_path=str(hist).encode())
        assert rc == _lib.E_ARG and res.cmin == 5
        assert why == "--reject_cutoff 5: the reject count must be above the minimum count, and --solid found 5"
    assert hist.exists()  # (rank 0 wrote it before the refusal: it is left to look at)
    rc, res, _, _ = decide(lib, occ, solid=1, cmin=0, bf_bytes=0, reject_cmin=6)
    assert (rc, res.cmin) == (0, 5) and 0 < res.reject_bf_bytes < res.bf_bytes
    assert res.reject_bf_bytes == lib.ntedit_hip_reads_bf_size(int(f[6:].sum()), 3, 0.01)
    # without --solid the same rule, in the stage's own words; and an empty reject filter
    rc, _, why, _ = decide(lib, None, cmin=9, bf_bytes=4096, reject_cmin=9, reject_bf_bytes=4096)
    assert (rc, why) == (_lib.E_ARG, "--reject_cutoff 9: the reject count must be above the minimum count 9")
    rc, _, why, _ = decide(lib, occ_of({1: 1000, 2: 300, 3: 20}), cmin=2, bf_bytes=4096, reject_cmin=4,
                           hist_path=os.devnull.encode())
    assert (rc, why) == (_lib.E_ARG, "The reject filter would be empty (no k-mer at --reject_cutoff 4 or above).")
    # arguments the stages refuse outright: no histogram to size from, a counting filter, a count past 255
    assert decide(lib, None, cmin=2, bf_bytes=4096, reject_cmin=7)[0] == _lib.E_ARG
    assert decide(lib, None, cmin=2, bf_bytes=4096, reject_cmin=7, reject_bf_bytes=64, counts=1)[0] == _lib.E_ARG
    assert decide(lib, None, cmin=2, bf_bytes=4096, reject_cmin=256, reject_bf_bytes=64)[0] == _lib.E_ARG


# ------------------------------------------------------------------ the four front ends
FLAGS = ("--reject_cutoff", "--reject_bf", "--reject_num_elements")


def _make_reads(argv, capsys):
    from ntedit_amd import make_reads
    rc = make_reads.main(argv)
    return rc, capsys.readouterr().err


def _run(argv, capsys):
    from ntedit_amd import run
    rc = run.main(argv)
    return rc, capsys.readouterr().err


def test_help_lists_the_options(binaries, capsys):
    r = subprocess.run([TOOL, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(f in r.stderr for f in FLAGS + ("--reject_out", "reads_k<K>_reject.bf"))
    r = subprocess.run([NTEDIT, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(f in r.stderr for f in FLAGS + ("--save_reject_bf", "reads_k<K>_reject.bf"))
    rc, err = _make_reads(["--help"], capsys)
    assert rc == 0 and all(f in err for f in FLAGS + ("--reject_out",))
    from ntedit_amd import run
    with pytest.raises(SystemExit) as e:
        run.parse(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert all(f in out for f in FLAGS + ("--save_reject_bf",))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("reject_cpu")
    (d / "reads.fa").write_bytes(b">r\n" + b"ACGT" * 20 + b"\n")
    (d / "draft.fa").write_bytes(b">c\n" + b"ACGT" * 50 + b"\n")
    (d / "e.bf").write_bytes(b"x")
    return d


# (the reject options, the tool dialect's message, the polisher dialect's)
REFUSALS = [
    (["--reject_cutoff", "x", "--reject_bf", "64"], "--reject_cutoff: not a number: 'x'", "invalid option: `--reject_cutoff x'"),
    (["--reject_cutoff", "1", "--reject_bf", "64"], "--reject_cutoff 1: the reject count must be between 2 and 255.",
     "--reject_cutoff 1: the reject count must be between 2 and 255"),
    (["--reject_cutoff", "2", "--reject_bf", "64"], "--reject_cutoff 2: the reject count must be above -c 2.",
     "--reject_cutoff 2: the reject count must be above --cutoff 2"),
    (["--reject_bf", "64"], "--reject_bf: only with --reject_cutoff.", "--reject_bf: only with --reject_cutoff"),
    (["--reject_cutoff", "9"], REJECT_SIZE + ".", REJECT_SIZE),
    (["--reject_cutoff", "9", "--reject_bf", "0"], "--reject_bf / --reject_num_elements: the reject filter would be empty.",
     "--reject_bf / --reject_num_elements: the reject filter would be empty"),
    (["--reject_cutoff", "9", "--reject_bf", "64", "--counts"], COUNTS + ".", COUNTS),
]


@pytest.mark.parametrize("extra,tool_why,polisher_why", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_the_front_ends_refuse_before_any_device(binaries, inputs, capsys, extra, tool_why, polisher_why):
    reads, draft = str(inputs / "reads.fa"), str(inputs / "draft.fa")
    out = inputs / "never"
    tool_args = ["--reads", reads, "-k", "25", "-c", "2", "--bf", "4096", "-o", str(out) + ".bf"] + extra
    r = subprocess.run([TOOL] + tool_args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and tool_why in r.stderr and "Sketch size" not in r.stdout, r.stderr
    rc, err = _make_reads(tool_args, capsys)
    assert rc == 1 and tool_why in err, err
    pol_args = ["-f", draft, "--reads", reads, "-k", "25", "--cutoff", "2", "--bf", "4096", "-b", str(out)] + extra
    r = subprocess.run([NTEDIT] + pol_args, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and polisher_why in r.stderr and "building Bloom filter" not in r.stdout, r.stderr
    rc, err = _run(pol_args, capsys)
    assert rc == 1 and polisher_why in err, err
    assert not [p for p in os.listdir(inputs) if p.startswith("never")]


def test_the_output_options_need_the_cutoff(binaries, inputs, capsys):
    reads, draft = str(inputs / "reads.fa"), str(inputs / "draft.fa")
    tool_args = ["--reads", reads, "-k", "25", "-c", "2", "--bf", "4096", "--reject_out", str(inputs / "never.bf")]
    r = subprocess.run([TOOL] + tool_args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--reject_out: only with --reject_cutoff." in r.stderr
    rc, err = _make_reads(tool_args, capsys)
    assert rc == 1 and "--reject_out: only with --reject_cutoff." in err
    pol_args = ["-f", draft, "--reads", reads, "-k", "25", "--cutoff", "2", "--bf", "4096", "--save_reject_bf",
                str(inputs / "never.bf")]
    r = subprocess.run([NTEDIT] + pol_args, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--save_reject_bf: only with --reject_cutoff" in r.stderr
    rc, err = _run(pol_args, capsys)
    assert rc == 1 and "--save_reject_bf: only with --reject_cutoff" in err


def test_the_polishers_refuse_it_without_reads_and_with_e(binaries, inputs, capsys):
    draft, reads, e = str(inputs / "draft.fa"), str(inputs / "reads.fa"), str(inputs / "e.bf")
    without = ["-f", draft, "-r", e, "--reject_cutoff", "9", "--reject_bf", "64"]
    r = subprocess.run([NTEDIT] + without, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--reject_cutoff: only with --reads" in r.stderr
    rc, err = _run(without, capsys)
    assert rc == 1 and "--reject_cutoff: only with --reads" in err
    with_e = ["-f", draft, "--reads", reads, "-k", "25", "--cutoff", "2", "--bf", "4096", "-e", e, "--reject_cutoff", "9",
              "--reject_bf", "64"]
    why = "--reject_cutoff and -e: give one of them (--reject_cutoff builds the filter that -e would load)"
    r = subprocess.run([NTEDIT] + with_e, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and why in r.stderr and "building Bloom filter" not in r.stdout
    rc, err = _run(with_e, capsys)
    assert rc == 1 and why in err
