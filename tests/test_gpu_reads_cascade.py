"""`ntedit --reads -k K1,K2,...,Kn` on the GPU: polishing in a cascade of k from one pass over the read files.

1. k_count<H, POW2, true> (pass 1 staged from the resident store) against the byte kernel and the model through the C
   ABI, for every H and both POW2, at a smaller and a larger k than the store was filled at, on the tile and halo edge
   blobs, and across saturation;
2. the store survives ntedit_hip_sketch_reset and not ntedit_hip_sketch_free; ntedit_hip_resident_count needs it ON;
3. the store is filled with the reads the smallest k needs: every round's filter equals ntedit-make-reads-bf's, with the
   host parser, --gpu_parse on plain files and --gpu_parse on BGZF files;
4. one cascade run equals the stand-alone runs, each fed the previous _edited.fa; rounds 2.. open no read file;
5. without the store (cap 0, or a cap smaller than the reads) every round reads the files, with the same outputs;
6. a single -k is unchanged: its standard output, line by line, and its file names."""
import ctypes
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import bgzf_corpus as BC
import helpers as H
from reads_model import blob_of, kmer_hashes, model_sketch, rounded, simulate_reads
from test_gpu_reads_bf import NTEDIT, TOOL, write_fasta, write_fastq
from test_gpu_reads_matrix import EDGES, Reads, device_batches, edge_blobs, host_batches, matrix_data

from ntedit_amd import _lib

pytestmark = pytest.mark.gpu

SKETCH = 1 << 24
OUTPUTS = ("_edited.fa", "_changes.tsv", "_variants.vcf")


def run(cmd, cwd=None):
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=600, cwd=cwd)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def read(path):
    with open(path, "rb") as f:
        return f.read()


# ------------------------------------------------------------------ 1. pass 1 from the store, through the C ABI
def byte_sketch(blobs, counters, h, k):
    """a fresh context counts the batches as bytes at k"""
    with Reads() as r:
        r.alloc(counters, h, k)
        r.count(host_batches(blobs))
        return r.sketch(rounded(counters))


def store_sketches(blobs, counters, h, k_fill, ks, on_device):
    """the batches counted as bytes at k_fill with the store on, then for each k of ks the sketch reset to k and counted
    from the store: [(k, sketch)], and the sketch at k_fill"""
    keep, out = [], []
    with Reads() as r:
        batches = device_batches(blobs, keep) if on_device else host_batches(blobs)
        r.alloc(counters, h, k_fill)
        r.ok(r.lib.ntedit_hip_reads_set_min_read(r.h, min(ks + [k_fill])), "reads_set_min_read")
        r.ok(r.lib.ntedit_hip_resident_begin(r.h, 1 << 40), "resident_begin")
        r.count(batches)
        first = r.sketch(rounded(counters))
        for k in ks:
            r.ok(r.lib.ntedit_hip_sketch_reset(r.h, counters, h, k), "sketch_reset")
            assert not r.sketch(rounded(counters)).any()  # (a fresh sketch: zeroed)
            r.ok(r.lib.ntedit_hip_resident_count(r.h), "resident_count")
            out.append((k, r.sketch(rounded(counters))))
    return out, first


def _count_cases():
    return [pytest.param(h, pow2, id="k_count<%d,%d,1>" % (h, int(pow2))) for h in range(1, 9) for pow2 in (True, False)]


@pytest.mark.parametrize("h,pow2", _count_cases())
def test_packed_pass_1_equals_the_byte_pass_and_the_model(h, pow2):
    blobs, hv31, counters, _, _ = matrix_data(2 * h + int(pow2), h, pow2, 31)
    got, first = store_sketches(blobs, counters, h, 31, [15, 40], on_device=h % 2 == 1)
    assert np.array_equal(first, model_sketch(hv31, rounded(counters)))
    joined = b"".join(blobs)
    for k, sk in got:
        want = model_sketch(kmer_hashes(joined, k, h), rounded(counters))
        assert (want == 255).any() and (want == 1).any()  # (a read 300 times: saturation is crossed from the store)
        assert np.array_equal(sk, want), "k = %d: the model" % k
        assert np.array_equal(sk, byte_sketch(blobs, counters, h, k)), "k = %d: the byte pass" % k


@pytest.mark.parametrize("k,h,counters", EDGES, ids=["k%d-h%d" % (k, h) for k, h, _ in EDGES])
def test_packed_pass_1_on_tile_and_halo_edges(k, h, counters):
    """a read that ends on a tile edge, reads that span it by k - 1, batches whose n is no multiple of 16: stored at
    another k, counted from the store at the k the blobs were made for"""
    blobs = edge_blobs(k, seed=k)
    assert {len(b) % 16 for b in blobs} - {0}
    joined = b"\n".join(blobs)
    want = model_sketch(kmer_hashes(joined, k, h), rounded(counters))
    fill = 31 if k != 31 else 25
    for tag, bl, dev in (("host", blobs, False), ("device", blobs, True), ("one batch", [joined], False)):
        got, _ = store_sketches(bl, counters, h, fill, [k], on_device=dev)
        assert np.array_equal(got[0][1], want), "%s batches: the model" % tag
    assert np.array_equal(want, byte_sketch(blobs, counters, h, k)), "the byte pass"


# ------------------------------------------------------------------ 2. the store and the sketch's life
def _info(r):
    st = _lib.ResidentStats()
    r.ok(r.lib.ntedit_hip_resident_info(r.h, ctypes.byref(st)), "resident_info")
    return st.state, st.batches, st.bases, st.bytes, st.cap


def test_the_store_survives_a_sketch_reset_and_not_a_sketch_free():
    blobs, _, counters, _, _ = matrix_data(0, 3, True, 31)
    with Reads() as r:
        r.alloc(counters, 3, 31)
        assert r.lib.ntedit_hip_resident_count(r.h) == _lib.E_ARG  # the store is OFF
        assert "no complete resident store" in r.lib.ntedit_hip_reads_last_error(r.h).decode()
        r.ok(r.lib.ntedit_hip_resident_begin(r.h, 1 << 40), "resident_begin")
        r.count(host_batches(blobs))
        before = _info(r)
        assert before[:3] == (_lib.RESIDENT_ON, len(blobs), sum(len(b) for b in blobs)) and before[3] > 0
        r.ok(r.lib.ntedit_hip_sketch_reset(r.h, counters + 8, 5, 17), "sketch_reset")
        assert _info(r) == before
        n, hn, k = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        r.ok(r.lib.ntedit_hip_sketch_info(r.h, ctypes.byref(n), ctypes.byref(hn), ctypes.byref(k)), "sketch_info")
        assert (n.value, hn.value, k.value) == (rounded(counters + 8), 5, 17)
        # the counters alone released: no sketch, the store still there
        r.ok(r.lib.ntedit_hip_sketch_reset(r.h, 0, 0, 0), "sketch_reset(0)")
        assert _info(r) == before
        assert r.lib.ntedit_hip_sketch_info(r.h, None, None, None) != 0
        assert r.lib.ntedit_hip_resident_count(r.h) == _lib.E_ARG
        r.ok(r.lib.ntedit_hip_sketch_reset(r.h, counters, 3, 20), "sketch_reset")
        r.ok(r.lib.ntedit_hip_resident_count(r.h), "resident_count")
        assert _info(r) == before
        # a bad reset touches nothing
        assert r.lib.ntedit_hip_sketch_reset(r.h, counters, 3, 11) == _lib.E_ARG
        assert _info(r) == before
        # sketch_alloc and sketch_free release the store, as always
        r.alloc(counters, 3, 31)
        assert _info(r)[:2] == (_lib.RESIDENT_OFF, 0)
        assert r.lib.ntedit_hip_resident_count(r.h) == _lib.E_ARG
        r.lib.ntedit_hip_sketch_free(r.h)
        st = _lib.ResidentStats()
        assert r.lib.ntedit_hip_resident_info(r.h, ctypes.byref(st)) != 0


# ------------------------------------------------------------------ the read set of 3. to 6.
K_LIST = (40, 30, 25)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """a 200 kbp genome, a draft of it with 2e-3 substitutions (and indels), 30 x of 150-base reads, and reads of 26 to
    39 bases from a region that no 150-base read covers, 3 x: k-mers that only the short reads carry"""
    d = tmp_path_factory.mktemp("cascade")
    rng = np.random.default_rng(41)
    truth = H.random_genome(rng, 200000)
    draft = H.mutate(rng, truth, p_sub=2e-3, p_ins=3e-4, p_del=3e-4)
    H.write_fasta(str(d / "draft.fa"), [(b"ctg1", draft[:120000]), (b"ctg2", draft[120000:])], width=80)
    long_reads = [bytes(r) for r in simulate_reads(rng, truth, 30)]
    island = H.random_genome(rng, 3000)
    short_reads = []
    for _ in range(3):
        at = int(rng.integers(0, 13))
        while at + 39 <= len(island):
            n = int(rng.integers(26, 40))
            short_reads.append(island[at:at + n])
            at += n - 24  # (consecutive reads share 24 bases: no 25-mer spans two of them)
    assert {len(r) for r in short_reads} == set(range(26, 40))
    # on the CPU: at k = 30 and k = 25 the island's k-mers reach the cutoff 2 through the short reads alone, and at
    # k = 40 those reads hold no k-mer
    long_blob, short_blob = blob_of(long_reads), blob_of(short_reads)
    for k in (30, 25):
        ls = np.unique(kmer_hashes(long_blob, k, 1)[:, 0])
        u, c = np.unique(kmer_hashes(short_blob, k, 1)[:, 0], return_counts=True)
        assert (c >= 2).sum() > 500 and not np.isin(u, ls).any(), k
    assert len(kmer_hashes(short_blob, 40, 1)) == 0
    reads = long_reads + short_reads
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    half = len(reads) // 2
    write_fastq(d / "a.fq", reads[:half])
    write_fasta(d / "b.fa", reads[half:])
    write_fastq(d / "a.fq.gz", reads[:half], opener=gzip.open)
    for name in ("a.fq", "b.fa"):
        with open(d / (name + ".bgz"), "wb") as f:
            f.write(BC.bgzf(read(d / name)))
    files = dict(host=[d / "a.fq.gz", d / "b.fa"], plain=[d / "a.fq", d / "b.fa"], bgzf=[d / "a.fq.bgz", d / "b.fa.bgz"])
    # (the reads reach the device as one batch: each read of at least min_read bases and its '\n')
    return dict(dir=d, draft=d / "draft.fa", files=files, reads_bytes=sum(len(r) + 1 for r in reads),
                batch_bytes=lambda min_read: sum(len(r) + 1 for r in reads if len(r) >= min_read))


# ------------------------------------------------------------------ 3. min_read: the store holds what the smallest k needs
@pytest.fixture(scope="module")
def tool_filters(case):
    """ntedit-make-reads-bf -k K -c 2 over the files, for each K"""
    out = {}
    for k in K_LIST:
        path = case["dir"] / ("tool_%d.bf" % k)
        run([TOOL, "--reads"] + case["files"]["host"] + ["-k", k, "-c", 2, "--bf", 1 << 20, "--sketch_bytes", SKETCH,
                                                         "-o", path])
        out[k] = read(path)
    return out


@pytest.mark.parametrize("form", ["host", "plain", "bgzf"])
def test_every_rounds_filter_equals_the_tools(case, tool_filters, form):
    d = case["dir"]
    extra = [] if form == "host" else ["--gpu_parse"]
    r = run([NTEDIT, "-f", case["draft"], "--reads"] + case["files"][form] +
            ["-k", "40,30,25", "--cutoff", 2, "--bf", 1 << 20, "--sketch_bytes", SKETCH, "--save_bf",
             d / (form + "_f_{k}.bf"), "-b", d / (form + "_p")] + extra)
    assert rounds_from_store(r) == [False, True, True], r.stdout
    if form != "host":
        assert "chunks parsed on the device" in r.stderr
        assert ("BGZF: " in r.stderr) == (form == "bgzf")
    for k in K_LIST:
        assert read(d / ("%s_f_%d.bf" % (form, k))) == tool_filters[k], k


# ------------------------------------------------------------------ 4. cascade equals sequence
ROUND_RE = r"^Round (\d) of (\d): k = (\d+), minimum count (\d+), (.*)$"
CONFIGS = {
    "solid": ((40, 30, 25), ["--solid"]),
    "reject": ((30, 40, 25), ["--cutoff", 2, "--bf", 1 << 20, "--reject_cutoff", 40, "--reject_bf", 100000]),
    "snv": ((40, 30, 25), ["--cutoff", 2, "--bf", 1 << 20, "-s", 1]),
}


def rounds_from_store(r):
    """per round, from the standard output: did every pass read the store"""
    rounds = re.findall(ROUND_RE, r.stdout, flags=re.M)
    assert [int(x[0]) for x in rounds] == list(range(1, len(rounds) + 1)) and rounds
    return ["every pass read the resident store, no read file was opened" in x[4] for x in rounds]


def saved(name, args, k):
    """the options that save this configuration's filters and histogram, k in the names"""
    out = ["--save_bf", "%s_%s.bf" % (name, k)]
    if "--solid" in args:
        out += ["--hist", "%s_%s.hist" % (name, k)]
    if "--reject_cutoff" in args:
        out += ["--save_reject_bf", "%s_%s_reject.bf" % (name, k)]
    return out


@pytest.fixture(scope="module")
def sequences(case):
    """per configuration, computed once: the stand-alone runs, each fed the previous _edited.fa -> the directory"""
    done = {}

    def get(name):
        if name not in done:
            ks, args = CONFIGS[name]
            d = case["dir"] / ("seq_" + name)
            d.mkdir()
            draft = case["draft"]
            for k in ks:
                r = run([NTEDIT, "-f", draft, "--reads"] + case["files"]["host"] + ["-k", k, "--sketch_bytes", SKETCH] +
                        args + saved(name, args, k) + ["-b", "p_%d" % k], cwd=d)
                assert "Round" not in r.stdout
                draft = d / ("p_%d_edited.fa" % k)
            done[name] = d
        return done[name]
    return get


def same_as_sequence(name, d, seq):
    """every round's outputs, saved filters and histograms of the cascade in d equal the stand-alone runs' in seq"""
    ks, args = CONFIGS[name]
    for i, k in enumerate(ks):
        mine = "p" if i + 1 == len(ks) else "p_k%d" % k
        for suffix in ("_edited.fa", "_changes.tsv"):
            assert read(d / (mine + suffix)) == read(seq / ("p_%d%s" % (k, suffix))), (k, suffix)
        assert H.vcf_body(str(d / (mine + "_variants.vcf"))) == H.vcf_body(str(seq / ("p_%d_variants.vcf" % k))), k
        for opt in saved(name, args, k)[1::2]:
            assert read(d / opt) == read(seq / opt), opt
    first = "p_k%d_edited.fa" % ks[0]
    assert read(d / "p_edited.fa") != read(d / first)  # (the later rounds edited: the comparison shows something)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_one_cascade_equals_the_stand_alone_runs(case, sequences, name):
    ks, args = CONFIGS[name]
    seq = sequences(name)
    d = case["dir"] / ("cas_" + name)
    d.mkdir()
    r = run([NTEDIT, "-f", case["draft"], "--reads"] + case["files"]["host"] +
            ["-k", ",".join(str(k) for k in ks), "--sketch_bytes", SKETCH] + args + saved(name, args, "{k}") + ["-b", "p"],
            cwd=d)
    same_as_sequence(name, d, seq)
    rounds = re.findall(ROUND_RE, r.stdout, flags=re.M)
    assert [int(x[2]) for x in rounds] == list(ks)
    assert rounds_from_store(r) == [False] + [True] * (len(ks) - 1)
    # rounds 2.. logged the store for each of their passes, pass 1 included, and no pass over the files
    passes = 3 if "--solid" in args else 2
    builds = r.stderr.split("Pass 1: counting k-mers")
    assert len(builds) == len(ks) + 1
    later = "".join(builds[2:])
    assert len(re.findall(r"Pass 1 \(count\): .* batches of the resident store", later)) == len(ks) - 1
    assert len(re.findall(r"Pass [1H2] \([^)]*\): .* batches of the resident store", later)) == passes * (len(ks) - 1)
    assert len(re.findall(r"Pass [1H2] \([^)]*\): ", later)) == passes * (len(ks) - 1)
    assert r.stderr.count("Resident store: kept from the build before") == len(ks) - 1
    if name == "solid":
        cuts = [int(x[3]) for x in rounds]
        assert all(2 <= c <= 10 for c in cuts), cuts


# ------------------------------------------------------------------ 5. without the store every round reads the files
@pytest.mark.parametrize("cap", ["off", "small"])
def test_without_the_store_every_round_reads_the_files(case, sequences, cap):
    ks, args = CONFIGS["solid"]
    seq = sequences("solid")
    d = case["dir"] / ("cap_" + cap)
    d.mkdir()
    cap_bytes = 0 if cap == "off" else case["reads_bytes"] // 8
    r = run([NTEDIT, "-f", case["draft"], "--reads"] + case["files"]["host"] +
            ["-k", "40,30,25", "--sketch_bytes", SKETCH, "--resident_cap", cap_bytes] + args + saved("solid", args, "{k}") +
            ["-b", "p"], cwd=d)
    same_as_sequence("solid", d, seq)
    rounds = re.findall(ROUND_RE, r.stdout, flags=re.M)
    assert len(rounds) == 3 and all("every pass read the files" in x[4] for x in rounds), r.stdout
    # released once, in round 1, and not tried again
    assert r.stderr.count("Resident store: released") == 1 and "batches of the resident store" not in r.stderr
    assert "would pass its cap of %d bytes" % cap_bytes in r.stderr


def stored_bytes(n):
    """the device bytes of a stored batch of n bytes (nte_reads.hip: per 16 bases a u32 of codes, padded to 16 bytes, and
    a u16 of validity bits)"""
    groups = (n + 15) // 16
    return (groups * 4 + 15) // 16 * 16 + groups * 2


def test_a_store_that_was_released_is_not_filled_again_without_the_short_reads(case, tool_filters):
    """a cap between what the store takes with the reads of 25 bases or more and with those of 30 or more: round 1
    (k = 40, keeping reads from 25 bases) passes it.  A round 2 that filled the store again, keeping only its own reads
    of 30 bases or more, would fit, and round 3 at k = 25 would count from a store without the reads of 25 to 29 bases.
    Every round's filter must still be the tool's."""
    d = case["dir"]
    n25, n30 = case["batch_bytes"](25), case["batch_bytes"](30)
    assert stored_bytes(n30) + 64 < stored_bytes(n25)
    cap = (stored_bytes(n25) + stored_bytes(n30)) // 2
    r = run([NTEDIT, "-f", case["draft"], "--reads"] + case["files"]["host"] +
            ["-k", "40,30,25", "--cutoff", 2, "--bf", 1 << 20, "--sketch_bytes", SKETCH, "--resident_cap", cap, "--save_bf",
             d / "between_f_{k}.bf", "-b", d / "between_p"])
    assert "would pass its cap of %d bytes" % cap in r.stderr
    assert rounds_from_store(r) == [False, False, False], r.stdout
    assert "batches of the resident store" not in r.stderr
    for k in K_LIST:
        assert read(d / ("between_f_%d.bf" % k)) == tool_filters[k], k
    # (the cap is what it is meant to be: with it, a stand-alone run at k = 30 keeps its store and one at k = 25 does not)
    for k, kept in ((30, True), (25, False)):
        one = run([NTEDIT, "-f", case["draft"], "--reads"] + case["files"]["host"] +
                  ["-k", k, "--cutoff", 2, "--bf", 1 << 20, "--sketch_bytes", SKETCH, "--resident_cap", cap, "-b",
                   d / ("between_one_%d" % k)])
        assert ("read the resident store" in one.stdout) == kept, (k, one.stdout)


# ------------------------------------------------------------------ 6. a single k is unchanged
# The transcript below is the parent commit's own: written from the printf sequence of its main.cpp, then compared once,
# masked as the test masks, with the standard output that a build of the parent commit printed for this command on
# this read set (it was equal).  `-t 4` is the default number of render threads; the blank lines are ctime's '\n'
# followed by the format's own.
DATE = r"[A-Z][a-z]{2} [A-Z][a-z]{2} [ \d]\d \d\d:\d\d:\d\d \d{4}"
SINGLE_K_STDOUT = """---------- initializing                             : <date>
---------- building Bloom filter from reads         : <date>

BF size (bytes): 1048576
Sketch size (counters): 16777216
Sketch occupancy: <n> / 16777216 counters (<x>)
Reads filter built in <x> ms (minimum count 2; the histogram pass and pass 2 read the resident store)
Bloom filter saved to f.bf
BLOOM::\tcounting: NO\tsize: 1048576\tnumber hash functions: 3\tkmer size: 25

---------- verifying parameters                     : <date>

running : ntEdit v2.1.1 (MI355X HIP hot path)
 -f draft.fa
 -k 25
 -z 100
 -b P
 -r f.bf
 -e <empty>
 -i 5
 -d 5
 -x 5
 -y 9
 -j 3
 -m 0
 -s 0
 -l <empty>
 -a 0
 -t 4
 -v 0

---------- reading/processing input sequence        : <date>
---------- process complete                         : <date>
"""


def test_a_single_k_is_unchanged(case, tmp_path):
    """the standard output of a run with one k, line by line as the program printed it before -k took a list (dates,
    times and the occupancy masked), and the names of its files"""
    r = run([NTEDIT, "-f", case["draft"], "--reads"] + case["files"]["host"] +
            ["-k", 25, "--cutoff", 2, "--bf", 1 << 20, "--sketch_bytes", SKETCH, "--save_bf", "f.bf", "-b", "P"],
            cwd=tmp_path)
    out = re.sub(DATE, "<date>", r.stdout)
    out = re.sub(r"occupancy: \d+ / (\d+) counters \([\d.e-]+\)", r"occupancy: <n> / \1 counters (<x>)", out)
    out = re.sub(r"built in [\d.]+ ms", "built in <x> ms", out)
    assert out == SINGLE_K_STDOUT.replace("<empty>", "")
    assert sorted(os.listdir(tmp_path)) == ["P_changes.tsv", "P_edited.fa", "P_variants.vcf", "f.bf"]
    assert "kept from the build before" not in r.stderr and "Round" not in r.stdout
