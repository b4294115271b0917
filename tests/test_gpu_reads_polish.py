"""`ntedit --reads` on the GPU: polishing straight from reads, with the filter built into the context that polishes.

1. one step equals two steps (ntedit-make-reads-bf, then ntedit -r): outputs, --save_bf against -o, --hist, and the
   oracle given the saved filter, for --cutoff, --solid, --counts -p 2 and -s 1;
2. with no -b, the one-step run writes the files the two-step run writes under default names;
3. the resident store against the files (store forced off, cap 0, and a cap smaller than the reads) for plain and gzip,
   FASTA and FASTQ, reads with N, lower case and reads shorter than k, and many small batches;
4. every packed instantiation k_hist<H, POW2, true>, k_solid<H, POW2, COUNTS, true> against the model through the C ABI,
   and the tile and halo edges of the packed staging;
5. the full-size run (3 Gbases of FASTA): one step equals two steps, and the timing of the passes."""
import ctypes
import gzip
import json
import os
import re
import subprocess
import time

import numpy as np
import pytest

import helpers as H
from reads_model import awkward_reads, blob_of, kmer_hashes, simulate_reads
from test_gpu_reads_bf import NTEDIT, TOOL, write_fasta, write_fastq, write_large_reads
from test_gpu_reads_matrix import EDGES, MATRIX, Reads, check_passes, device_batches, edge_blobs, host_batches, matrix_data

from ntedit_amd import _lib

pytestmark = pytest.mark.gpu

K = 25
SKETCH = 1 << 24
OUTPUTS = ("_edited.fa", "_changes.tsv", "_variants.vcf")


def run(cmd, cwd=None, timeout=900):
    t0 = time.monotonic()
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=timeout, cwd=cwd)
    r.wall = time.monotonic() - t0
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def read(path):
    with open(path, "rb") as f:
        return f.read()


def logged_cutoff(r):
    m = re.search(r"minimum count (\d+);", r.stdout)
    assert m, r.stdout
    return int(m.group(1))


def store_used(r):
    if "read the resident store" in r.stdout:
        assert re.search(r"Resident store: \d+ batches", r.stderr), r.stderr
        return True
    assert "read the files" in r.stdout and "Resident store: released" in r.stderr, r.stdout + r.stderr
    return False


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """a 200 kbp genome, a draft of it with errors, and 30 x of reads split over a gzip FASTQ and a plain FASTA file"""
    d = tmp_path_factory.mktemp("polish")
    rng = np.random.default_rng(29)
    truth = H.random_genome(rng, 200000)
    draft = H.mutate(rng, truth, p_sub=2e-3, p_ins=3e-4, p_del=3e-4)
    H.write_fasta(str(d / "draft.fa"), [(b"ctg1", draft[:120000]), (b"ctg2", draft[120000:])], width=80)
    reads = [bytes(r) for r in simulate_reads(rng, truth, 30)]
    half = len(reads) // 2
    write_fastq(d / "r1.fq.gz", reads[:half], opener=gzip.open)
    write_fasta(d / "r2.fa", reads[half:])
    return dict(dir=d, draft=d / "draft.fa", reads=[d / "r1.fq.gz", d / "r2.fa"])


# ------------------------------------------------------------------ 1. one step equals two steps
CONFIGS = {
    "cutoff": (["--bf", 1 << 20], ["--cutoff", 2], ["-c", 2], [], {}),
    "solid": ([], ["--solid"], ["--solid"], [], {}),
    "counts": (["--bf", 1 << 20, "--counts"], ["--cutoff", 2], ["-c", 2], ["-p", 2], dict(min_threshold=2)),
    "snv": (["--bf", 1 << 20], ["--cutoff", 2], ["-c", 2], ["-s", 1], dict(snv=1)),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_one_step_equals_two_steps(case, name):
    d, draft = case["dir"], case["draft"]
    filt, one_cut, two_cut, polish, params = CONFIGS[name]
    common = ["-k", K, "--sketch_bytes", SKETCH] + filt
    run([TOOL, "--reads"] + case["reads"] + common + two_cut + ["--hist", d / (name + "_two.hist"),
                                                                "-o", d / (name + "_two.bf")])
    run([NTEDIT, "-f", draft, "-r", d / (name + "_two.bf"), "-b", d / (name + "_two")] + polish)
    r = run([NTEDIT, "-f", draft, "--reads"] + case["reads"] + common + one_cut +
            ["--hist", d / (name + "_one.hist"), "--save_bf", d / (name + "_one.bf"), "-b", d / (name + "_one")] + polish)
    assert store_used(r)
    assert read(d / (name + "_one.bf")) == read(d / (name + "_two.bf"))
    assert read(d / (name + "_one.hist")) == read(d / (name + "_two.hist"))
    for suffix in OUTPUTS:
        assert read(d / (name + "_one" + suffix)) == read(d / (name + "_two" + suffix)), suffix
    bf = H.load_bf(str(d / (name + "_one.bf")))
    assert bf["counting"] == (name == "counts")
    if name == "solid":
        assert 2 <= logged_cutoff(r) <= 10
    H.run_oracle(str(draft), str(d / (name + "_one.bf")), H.default_params(**params), str(d / (name + "_o")))
    for suffix in ("_edited.fa", "_changes.tsv"):
        assert read(d / (name + "_one" + suffix)) == read(d / (name + "_o" + suffix)), suffix
    if name == "snv":
        assert H.vcf_body(str(d / "snv_one_variants.vcf")) == H.vcf_body(str(d / "snv_o_variants.vcf"))
        assert len(H.vcf_body(str(d / "snv_one_variants.vcf"))) > 20


# ------------------------------------------------------------------ 2. default output names
def test_default_output_names_match_the_two_step_run(case, tmp_path):
    one, two = tmp_path / "one", tmp_path / "two"
    one.mkdir()
    two.mkdir()
    args = ["-k", K, "--bf", 1 << 20, "--sketch_bytes", SKETCH]
    run([TOOL, "--reads"] + case["reads"] + args + ["-c", 2], cwd=two)
    assert os.listdir(two) == ["reads_k25.bf"]
    run([NTEDIT, "-f", case["draft"], "-r", "reads_k25.bf"], cwd=two)
    run([NTEDIT, "-f", case["draft"], "--reads"] + case["reads"] + args + ["--cutoff", 2], cwd=one)
    names = sorted(os.listdir(one))
    assert names == sorted(set(os.listdir(two)) - {"reads_k25.bf"})
    assert "draft.fa_k25_z100_rreads_k25.bf_i5_d5_m0_edited.fa" in names
    for n in names:
        if not n.endswith(".vcf"):
            assert read(one / n) == read(two / n), n
    # --save_bf names the _r part
    run([NTEDIT, "-f", case["draft"], "--reads"] + case["reads"] + args + ["--cutoff", 2, "--save_bf", "mine.bf"],
        cwd=one)
    assert read(one / "mine.bf") == read(two / "reads_k25.bf")
    assert (one / "draft.fa_k25_z100_rmine.bf_i5_d5_m0_edited.fa").exists()


# ------------------------------------------------------------------ 3. the resident store against the files
@pytest.fixture(scope="module")
def awkward(tmp_path_factory):
    """reads with errors, N runs, reads shorter than k and a read 300 times; some in lower case"""
    d = tmp_path_factory.mktemp("store")
    rng = np.random.default_rng(31)
    reads = []
    for r in awkward_reads(K, seed=19, genome_len=40000):
        r = bytearray(r)
        if rng.random() < 0.2:
            at = int(rng.integers(0, len(r)))
            r[at:at + 30] = bytes(r[at:at + 30]).lower()
        reads.append(bytes(r))
    assert any(len(r) < K for r in reads) and any(b"N" in r for r in reads)
    files = {"fa": d / "r.fa", "fq": d / "r.fq", "fa.gz": d / "r.fa.gz", "fq.gz": d / "r.fq.gz"}
    write_fasta(files["fa"], reads)
    write_fastq(files["fq"], reads)
    with gzip.open(files["fa.gz"], "wb") as f:
        f.write(read(files["fa"]))
    write_fastq(files["fq.gz"], reads, opener=gzip.open)
    H.write_fasta(str(d / "draft.fa"), [(b"c", H.random_genome(rng, 5000))])
    return dict(dir=d, files=files, draft=d / "draft.fa", bases=sum(len(r) for r in reads))


@pytest.mark.parametrize("form,batch", [("fa", None), ("fq", None), ("fa.gz", None), ("fq.gz", None),
                                        ("fa", 4096), ("fq.gz", 100000)])
def test_store_and_files_give_identical_filters(awkward, form, batch):
    d = awkward["dir"]
    extra = ["--batch_bytes", batch] if batch else []
    got = {}
    for tag, cap in (("store", None), ("off", 0), ("small", awkward["bases"] // 8)):
        p = d / ("%s_%s_%s" % (form, batch, tag))
        caps = ["--resident_cap", cap] if cap is not None else []
        r = run([NTEDIT, "-f", awkward["draft"], "--reads", awkward["files"][form], "-k", K, "--solid",
                 "--sketch_bytes", 1000003, "--hist", str(p) + ".hist", "--save_bf", str(p) + ".bf", "-b", p] +
                extra + caps)
        assert store_used(r) == (tag == "store"), tag
        if tag == "small":
            assert "would pass its cap of %d bytes" % cap in r.stderr
        got[tag] = (read(str(p) + ".bf"), read(str(p) + ".hist"), logged_cutoff(r))
    assert got["store"] == got["off"] == got["small"]
    # and the same as the tool, which reads the files
    out = d / ("%s_%s_tool.bf" % (form, batch))
    run([TOOL, "--reads", awkward["files"][form], "-k", K, "--solid", "--sketch_bytes", 1000003, "-o", out] + extra)
    assert read(out) == got["store"][0]


# ------------------------------------------------------------------ 4. the packed instantiations through the C ABI
def store_passes(blobs, counters, h, k, cmin, plain_bytes, count_bytes, on_device):
    """run_passes of test_gpu_reads_matrix with the histogram pass and pass 2 reading the resident store"""
    keep = []
    with Reads() as r:
        batches = device_batches(blobs, keep) if on_device else host_batches(blobs)
        r.alloc(counters, h, k)
        r.ok(r.lib.ntedit_hip_resident_begin(r.h, 1 << 40), "resident_begin")
        r.count(batches)
        st = _lib.ResidentStats()
        r.ok(r.lib.ntedit_hip_resident_info(r.h, ctypes.byref(st)), "resident_info")
        assert st.state == _lib.RESIDENT_ON and st.batches == sum(1 for b in blobs if len(b))
        assert st.bases == sum(len(b) for b in blobs)
        sk = r.sketch(_rounded(counters))
        sk_occ = r.sketch_occupancy()
        r.ok(r.lib.ntedit_hip_resident_histogram(r.h), "resident_histogram")
        occ = np.zeros(256, dtype=np.uint64)
        r.ok(r.lib.ntedit_hip_sketch_histogram_download(r.h, occ.ctypes.data_as(ctypes.c_void_p)), "histogram_download")
        r.plain(plain_bytes, h, k)
        r.ok(r.lib.ntedit_hip_resident_insert_solid(r.h, 0, cmin), "resident_insert_solid")
        plain = r.pol.filter_download(0)
        r.counting(count_bytes, h, k)
        r.ok(r.lib.ntedit_hip_resident_insert_solid(r.h, 0, cmin), "resident_insert_solid")
        counts = r.pol.filter_download(0)
        c_occ = r.pol.filter_occupancy(0)
    return sk, occ, plain, counts, sk_occ, c_occ


def _rounded(n):
    return (n + 7) // 8 * 8


@pytest.mark.parametrize("i,h,pow2,k", MATRIX)
def test_every_packed_instantiation_equals_the_model(i, h, pow2, k):
    blobs, hv, counters, plain_bytes, count_bytes = matrix_data(i, h, pow2, k)
    got = store_passes(blobs, counters, h, k, 4, plain_bytes, count_bytes, on_device=h % 2 == 1)
    check_passes(got, hv, counters, 4, plain_bytes, count_bytes)


@pytest.mark.parametrize("k,h,counters", EDGES, ids=["k%d-h%d" % (k, h) for k, h, _ in EDGES])
def test_packed_tile_and_halo_edges(k, h, counters):
    blobs = edge_blobs(k, seed=k)
    joined = b"\n".join(blobs)
    hv = kmer_hashes(joined, k, h)
    for tag, bl, dev in (("host", blobs, False), ("device", blobs, True), ("one batch", [joined], False)):
        got = store_passes(bl, counters, h, k, 2, 1 << 17, 100003, on_device=dev)
        try:
            check_passes(got, hv, counters, 2, 1 << 17, 100003)
        except AssertionError as e:
            raise AssertionError("%s batches: %s" % (tag, e)) from None


def test_store_past_its_cap_is_released():
    blob = blob_of(awkward_reads(K, seed=7, genome_len=8000))
    with Reads() as r:
        r.alloc(1 << 20, 3, K)
        # the first quarter fits (6 bytes per 16 bases), the rest would pass the cap
        r.ok(r.lib.ntedit_hip_resident_begin(r.h, len(blob) // 8), "resident_begin")
        half = len(blob) // 4
        r.count([(blob[:half], half, 0)])
        st = _lib.ResidentStats()
        r.ok(r.lib.ntedit_hip_resident_info(r.h, ctypes.byref(st)), "resident_info")
        assert st.state == _lib.RESIDENT_ON and st.batches == 1 and 0 < st.bytes <= len(blob) // 8
        r.count([(blob[half:], len(blob) - half, 0)])
        r.ok(r.lib.ntedit_hip_resident_info(r.h, ctypes.byref(st)), "resident_info")
        assert st.state == _lib.RESIDENT_OVER_CAP and st.batches == 0 and st.bytes == 0
        assert r.lib.ntedit_hip_resident_histogram(r.h) != 0
        assert "no complete resident store" in r.lib.ntedit_hip_reads_last_error(r.h).decode()


# ------------------------------------------------------------------ 5. full size: 100 Mbp x 30, 3 Gbases of FASTA
PASS_RE = r"Pass (\d|H) \([^)]*\): (\d+) bases, ([\d.]+) ms"


def test_full_size_one_step_equals_two_steps(tmp_path):
    fa = tmp_path / "large.fa"
    genome, n_reads = write_large_reads(fa)
    rng = np.random.default_rng(11)
    draft = H.mutate(rng, genome[:2_000_000], p_sub=2e-3, p_ins=3e-4, p_del=3e-4)
    H.write_fasta(str(tmp_path / "draft.fa"), [(b"ctg1", draft)], width=80)
    del genome
    common = ["-k", K, "--bf", 200_000_000, "--sketch_bytes", 1 << 32]
    two = run([TOOL, "--reads", fa] + common + ["-c", 3, "--hist", tmp_path / "two.hist", "-o", tmp_path / "two.bf"],
              timeout=1800)
    r2 = run([NTEDIT, "-f", tmp_path / "draft.fa", "-r", tmp_path / "two.bf", "-b", tmp_path / "two"], timeout=1800)
    one = run([NTEDIT, "-f", tmp_path / "draft.fa", "--reads", fa] + common +
              ["--cutoff", 3, "--hist", tmp_path / "one.hist", "--save_bf", tmp_path / "one.bf", "-b", tmp_path / "one"],
              timeout=1800)
    assert store_used(one)
    assert read(tmp_path / "one.hist") == read(tmp_path / "two.hist")
    assert read(tmp_path / "one.bf") == read(tmp_path / "two.bf")
    for suffix in ("_edited.fa", "_changes.tsv"):
        assert read(str(tmp_path / "one") + suffix) == read(str(tmp_path / "two") + suffix), suffix
    files = {p: float(ms) for p, b, ms in re.findall(PASS_RE, two.stderr)}
    store = {p: float(ms) for p, b, ms in re.findall(PASS_RE, one.stderr)}
    assert set(files) == set(store) == {"1", "H", "2"}
    assert all(int(b) == n_reads * 150 for _, b, _ in re.findall(PASS_RE, one.stderr))
    print(json.dumps(dict(reads_bases=n_reads * 150, files_ms=files, store_ms=store, two_step_s=two.wall + r2.wall,
                          tool_s=two.wall, one_step_s=one.wall)))
    # the store's reason to exist: the two later passes at less than half their cost from the files
    assert store["H"] + store["2"] < 0.5 * (files["H"] + files["2"]), (files, store)
