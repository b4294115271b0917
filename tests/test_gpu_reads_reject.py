"""The reject filter (ntedit -e) built by the same pass 2 as the primary filter, on the GPU:

1. every instantiation k_solid2<H, POW2, PACKED> against the count-min model through the C ABI, two outputs of different
   sizes, from byte batches (ntedit_hip_filter_insert_solid2) and from the resident store (_resident_insert_solid2);
2. the tile and halo edges of both stagings;
3. the thresholds at 254 / 255 / 256 and the refusals of the two calls;
4. the tool: the primary file is the run's without the options, the reject file a second run's with -c R;
5. a polish that the reject filter changes: `ntedit --reads --reject_cutoff` against `ntedit -r -e`, the oracle, and
   the same run without the reject filter;
6. the resident store off, past its cap, and --gpu_parse: the same two filters;
7. the sharded drivers: make_reads at world 2, run --reads at worlds 1 and 2, the --report fields."""
import ctypes
import gzip
import re
import subprocess

import numpy as np
import pytest

import helpers as H
from reads_model import blob_of, kmer_hashes, model_bf, model_estimates, model_sketch, rounded, simulate_reads
from test_gpu_reads_bf import NTEDIT, TOOL, write_fasta, write_fastq
from test_gpu_reads_matrix import (EDGES, MATRIX, Reads, _three_kmers, device_batches, edge_blobs, host_batches,
                                   matrix_data)
from test_gpu_reads_multi import _binary, _driver
from test_gpu_reads_polish import case  # noqa: F401 (the fixture: a gzip FASTQ and a plain FASTA of 30x reads)
from test_gpu_reads_run import driver, reports

pytestmark = pytest.mark.gpu

K = 25


def read(path):
    with open(path, "rb") as f:
        return f.read()


def run(cmd, timeout=600):
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


# ------------------------------------------------------------------ the C ABI
def two_slots(r, b1, b2, h, k):
    """zeroed plain filters of b1 bytes in the PRIMARY and b2 bytes in the SECONDARY slot"""
    r.pol.filter_alloc(b1, h, k, slot=0)
    r.pol.filter_alloc(b2, h, k, slot=1)


def dual_passes(blobs, counters, h, k, cmin, rmin, b1, b2, on_device):
    """pass 1 (the reads kept resident), then the dual pass 2 twice into fresh filters: over the byte batches and over
    the store.  -> ((primary, reject) from the batches, (primary, reject) from the store)"""
    keep = []
    with Reads() as r:
        batches = device_batches(blobs, keep) if on_device else host_batches(blobs)
        r.alloc(counters, h, k)
        r.ok(r.lib.ntedit_hip_resident_begin(r.h, 1 << 40), "resident_begin")
        r.count(batches)
        two_slots(r, b1, b2, h, k)
        for ptr, n, dev in batches:
            r.ok(r.lib.ntedit_hip_filter_insert_solid2(r.h, ptr, n, dev, cmin, rmin), "filter_insert_solid2")
        byte = (r.pol.filter_download(0), r.pol.filter_download(1))
        two_slots(r, b1, b2, h, k)
        r.ok(r.lib.ntedit_hip_resident_insert_solid2(r.h, cmin, rmin), "resident_insert_solid2")
        packed = (r.pol.filter_download(0), r.pol.filter_download(1))
    return byte, packed


def check_dual(got, hv, est, cmin, rmin, b1, b2):
    want = (model_bf(hv, est, cmin, rounded(b1)), model_bf(hv, est, rmin, rounded(b2)))
    for tag, (primary, reject) in zip(("byte batches", "resident store"), got):
        assert np.array_equal(primary, want[0]), tag + ": primary"
        assert np.array_equal(reject, want[1]), tag + ": reject"
    return want


# ------------------------------------------------------------------ 1. every instantiation, byte and packed
DUAL = [pytest.param(*p.values, id="k_solid2<%d,%d,0>+k_solid2<%d,%d,1>-k%d" % (p.values[1], p.values[2], p.values[1],
                                                                                   p.values[2], p.values[3])) for p in MATRIX]


@pytest.mark.parametrize("i,h,pow2,k", DUAL)
def test_every_dual_instantiation_equals_the_model(i, h, pow2, k):
    blobs, hv, counters, plain_bytes, count_bytes = matrix_data(i, h, pow2, k)
    cmin, rmin = 4, 40
    # the reject filter takes the other size, so that a mixed-up geometry cannot pass
    b1, b2 = plain_bytes, rounded(count_bytes)
    assert rounded(b1) != b2
    est = model_estimates(hv, model_sketch(hv, rounded(counters)))
    distinct = len(np.unique(hv[:, 0]))
    at_cmin, at_rmin = len(np.unique(hv[est >= cmin, 0])), len(np.unique(hv[est >= rmin, 0]))
    # both thresholds keep some distinct k-mers and drop others
    assert 0 < at_rmin < at_cmin < distinct, (at_rmin, at_cmin, distinct)
    got = dual_passes(blobs, counters, h, k, cmin, rmin, b1, b2, on_device=h % 2 == 1)
    want = check_dual(got, hv, est, cmin, rmin, b1, b2)
    # and the two bitmaps differ, also at one size: no case is vacuous
    assert not np.array_equal(model_bf(hv, est, cmin, b2), want[1])


def test_the_matrix_covers_every_dual_instantiation():
    assert {(p.values[1], p.values[2]) for p in MATRIX} == {(h, pow2) for h in range(1, 9) for pow2 in (True, False)}


# ------------------------------------------------------------------ 2. tile and halo edges
@pytest.mark.parametrize("k,h,counters", EDGES, ids=["k%d-h%d" % (k, h) for k, h, _ in EDGES])
def test_dual_tile_and_halo_edges_for_every_batching(k, h, counters):
    blobs = edge_blobs(k, seed=k)
    joined = b"\n".join(blobs)
    hv = kmer_hashes(joined, k, h)
    cmin, rmin, b1, b2 = 2, 3, 1 << 17, 100003
    est = model_estimates(hv, model_sketch(hv, rounded(counters)))
    assert (est < cmin).any() and ((est >= cmin) & (est < rmin)).any() and (est >= rmin).any()
    for tag, bl, dev in (("host", blobs, False), ("device", blobs, True), ("one batch", [joined], False)):
        got = dual_passes(bl, counters, h, k, cmin, rmin, b1, b2, on_device=dev)
        try:
            check_dual(got, hv, est, cmin, rmin, b1, b2)
        except AssertionError as e:
            raise AssertionError("%s batches: %s" % (tag, e)) from None


# ------------------------------------------------------------------ 3. threshold edges and refusals
@pytest.mark.parametrize("k,h", [(33, 3), (128, 8)])
def test_cmin_254_and_reject_255(k, h):
    """three k-mers that occur 254, 255 and 256 times in a collision-free sketch: all three are solid at 254, and the
    reject filter at 255 holds exactly the two whose counters saturate"""
    a, b, c = _three_kmers(k, seed=k)
    blob = blob_of([a] * 254 + [b] * 255 + [c] * 256)
    hv = kmer_hashes(blob, k, h)
    counters = 1 << 20
    u = np.unique(hv, axis=0)
    assert len(u) == 3 and len(np.unique(u % np.uint64(counters))) == 3 * h  # collision-free
    est = model_estimates(hv, model_sketch(hv, counters))
    assert sorted(set(est.tolist())) == [254, 255]
    assert len(np.unique(hv[est >= 254], axis=0)) == 3 and len(np.unique(hv[est >= 255], axis=0)) == 2
    got = dual_passes([blob], counters, h, k, 254, 255, 1 << 12, 4104, on_device=False)
    want = check_dual(got, hv, est, 254, 255, 1 << 12, 4104)
    two = kmer_hashes(blob_of([b, c]), k, h)
    assert np.array_equal(want[1], model_bf(two, np.full(len(two), 255, dtype=np.uint8), 255, 4104))
    assert 0 < int(np.unpackbits(got[0][1]).sum()) <= 2 * h and 0 < int(np.unpackbits(got[0][0]).sum()) <= 3 * h


def test_the_dual_calls_refuse_bad_thresholds_and_filters():
    k, h = 25, 3
    blob = blob_of([H.random_genome(np.random.default_rng(3), 200)])
    with Reads() as r:
        def both(cmin, rmin):
            """(status, message) of the two calls, which must refuse alike"""
            out = []
            for call in (lambda: r.lib.ntedit_hip_filter_insert_solid2(r.h, blob, len(blob), 0, cmin, rmin),
                         lambda: r.lib.ntedit_hip_resident_insert_solid2(r.h, cmin, rmin)):
                rc = call()
                out.append((rc, r.lib.ntedit_hip_reads_last_error(r.h).decode()))
            assert out[0][0] == out[1][0]
            return out

        r.alloc(1 << 16, h, k)
        r.ok(r.lib.ntedit_hip_resident_begin(r.h, 1 << 30), "resident_begin")
        r.count(host_batches([blob]))
        two_slots(r, 4096, 2048, h, k)
        for cmin, rmin in ((4, 4), (4, 3), (4, 0), (4, 256), (0, 5)):
            for rc, why in both(cmin, rmin):
                assert rc != 0 and ("needs cmin < rmin <= 255" in why or "needs 1 <= cmin <= 255" in why), (cmin, rmin, why)
        assert not r.pol.filter_download(0).any() and not r.pol.filter_download(1).any()
        # the SECONDARY slot: not set, a counting filter, another hash_num, another k
        r.pol.filter_alloc(4096, h, k, slot=0)
        r.ok(r.lib.ntedit_hip_filter_alloc_counting(r.h, 1, 2048, h, k), "filter_alloc_counting")
        for rc, why in both(2, 3):
            assert rc != 0 and "SECONDARY filter is a counting filter" in why, why
        r.pol.filter_alloc(2048, h + 1, k, slot=1)
        for rc, why in both(2, 3):
            assert rc != 0 and "hash_num = %d, the sketch k = %d, hash_num = %d" % (h + 1, k, h) in why, why
        r.pol.filter_alloc(2048, h, k + 1, slot=1)
        for rc, why in both(2, 3):
            assert rc != 0 and "the filter has k = %d" % (k + 1) in why, why
        # a counting PRIMARY filter is refused too; and the context setting follows the same bound
        r.pol.filter_alloc(2048, h, k, slot=1)
        r.ok(r.lib.ntedit_hip_filter_alloc_counting(r.h, 0, 4096, h, k), "filter_alloc_counting")
        for rc, why in both(2, 3):
            assert rc != 0 and "PRIMARY filter is a counting filter" in why, why
        assert r.lib.ntedit_hip_reads_set_reject_cutoff(r.h, 256) != 0
        assert r.lib.ntedit_hip_reads_set_reject_cutoff(r.h, 255) == 0
        assert r.lib.ntedit_hip_reads_set_reject_cutoff(r.h, 0) == 0
        # after all the refusals the pair still works
        two_slots(r, 4096, 2048, h, k)
        for rc, why in both(1, 2):
            assert rc == 0, why
        assert r.pol.filter_download(0).any()
    with Reads() as r:  # (without a sketch)
        assert r.lib.ntedit_hip_filter_insert_solid2(r.h, blob, len(blob), 0, 2, 3) != 0
        assert r.lib.ntedit_hip_resident_insert_solid2(r.h, 2, 3) != 0
        assert r.lib.ntedit_hip_reads_set_reject_cutoff(r.h, 3) != 0


# ------------------------------------------------------------------ 4. the tool
@pytest.mark.parametrize("mode", ["c", "solid"])
def test_tool_writes_the_files_of_two_separate_runs(case, mode):  # noqa: F811
    d = case["dir"]
    R, B2 = 25, 1 << 18  # (30x reads: k-mer counts around 20, so 25 keeps some k-mers and drops most)
    base = [TOOL, "--reads"] + case["reads"] + ["-k", K]
    cut = ["-c", 2, "--bf", 1 << 20] if mode == "c" else ["--solid"]
    size = ["--reject_bf", B2] if mode == "c" else []
    f1, f2, p0, e0 = (d / ("rj_%s_%s.bf" % (mode, n)) for n in ("primary", "reject", "alone", "second"))
    r = run(base + cut + ["--reject_cutoff", R] + size + ["--reject_out", f2, "-o", f1])
    r0 = run(base + cut + ["-o", p0])
    assert read(f1) == read(p0)
    sketch = int(re.search(r"Sketch size \(counters\): (\d+)", r.stdout).group(1))
    assert sketch == int(re.search(r"Sketch size \(counters\): (\d+)", r0.stdout).group(1))
    if mode == "solid":  # (both sized from the histogram)
        B2 = int(re.search(r"Reject BF size \(bytes\): (\d+)", r.stdout).group(1))
        assert "Reject BF size (bytes): from the k-mer histogram" in r.stdout
        assert int(re.search(r"--solid: minimum k-mer count (\d+)", r.stderr).group(1)) < R
    run(base + ["-c", R, "--bf", B2, "--sketch_bytes", sketch, "-o", e0])
    assert read(f2) == read(e0)
    m1, m2 = H.load_bf(str(f1)), H.load_bf(str(f2))
    assert (m2["k"], m2["hash_num"], m2["counting"], m2["bytes"]) == (m1["k"], m1["hash_num"], False, rounded(B2))
    assert m2["data"].any() and np.unpackbits(m2["data"]).sum() < np.unpackbits(m1["data"]).sum()
    # without the options the console lines stay as they were
    assert "eject" not in r0.stdout + r0.stderr and "the reject filter those seen at least %d times" % R in r.stderr


# ------------------------------------------------------------------ 5. a polish that the reject filter changes
R_REPEAT = 96


@pytest.fixture(scope="module")
def repeats(tmp_path_factory):
    """A 130 kbp genome that holds a 3 kbp unit eight times, a draft of it mutated as in `case`, and 30x reads with 1 %
    errors in a gzip FASTQ and a plain FASTA.  At k = 25 in a 2^24-counter sketch the count-min model (reads_model) gives
    the genome's k-mers outside the unit estimates of 0 to 64 (about 20 expected, one k-mer at 64) and the unit's 2,976
    k-mers 127 to 200 (about 150 expected); the reject count 96 lies between the two ranges, and exactly the unit's
    2,976 distinct k-mers pass it.  (On the CPU oracle with the model's filters _changes.tsv has 320 lines without -e and 279
    with it, and so it has on the GPU.)"""
    d = tmp_path_factory.mktemp("repeats")
    rng = np.random.default_rng(53)
    unit = H.random_genome(rng, 3000)
    truth = b"".join(H.random_genome(rng, 13250) + unit for _ in range(8))
    draft = H.mutate(rng, truth, p_sub=2e-3, p_ins=3e-4, p_del=3e-4)
    H.write_fasta(str(d / "draft.fa"), [(b"ctg1", draft)], width=80)
    reads = [bytes(r) for r in simulate_reads(rng, truth, 30)]
    half = len(reads) // 2
    write_fastq(d / "r1.fq.gz", reads[:half], opener=gzip.open)
    write_fasta(d / "r2.fa", reads[half:])
    return dict(dir=d, draft=d / "draft.fa", reads=[d / "r1.fq.gz", d / "r2.fa"], plain=d / "r2.fa", done={})


FILTER = ["-k", K, "--cutoff", 2, "--bf", 1 << 20, "--sketch_bytes", 1 << 24]
REJECT = ["--reject_cutoff", R_REPEAT, "--reject_bf", 1 << 15]


def one_step(repeats, tag, extra=(), reject=REJECT, reads=None):
    """`ntedit --reads` over the fixture, once per tag: -> the prefix of its outputs and of <prefix>.a.bf / .b.bf"""
    if tag not in repeats["done"]:
        p = repeats["dir"] / tag
        save = ["--save_bf", str(p) + ".a.bf"] + (["--save_reject_bf", str(p) + ".b.bf"] if reject else [])
        r = run([NTEDIT, "-f", repeats["draft"], "--reads"] + (reads or repeats["reads"]) + FILTER + list(reject) + save +
                ["-b", p] + list(extra))
        repeats["done"][tag] = (p, r)
    return repeats["done"][tag]


def rows(path):
    return len(read(path).splitlines())


def test_polish_with_the_reject_filter_built_from_the_reads(repeats, oracle_build):
    d, draft = repeats["dir"], repeats["draft"]
    p, r = one_step(repeats, "one")
    a, b = str(p) + ".a.bf", str(p) + ".b.bf"
    assert "secondary Bloom filter built from reads" in r.stdout and "loading secondary Bloom filter" not in r.stdout
    assert re.search(r"\n -e one\.b\.bf\n", r.stdout), r.stdout
    # the two-step route with the saved files, and the oracle
    run([NTEDIT, "-f", draft, "-r", a, "-e", b, "-b", d / "two"])
    H.run_oracle(str(draft), a, H.default_params(), str(d / "oracle"), rep_path=b)
    for suffix in ("_edited.fa", "_changes.tsv"):
        assert read(str(p) + suffix) == read(str(d / "two") + suffix), suffix
        assert read(str(p) + suffix) == read(str(d / "oracle") + suffix), suffix
    # the reject filter holds the unit's k-mers, and it changes the polish: strictly fewer rows than without it
    q, _ = one_step(repeats, "none", reject=())
    assert read(str(q) + ".a.bf") == read(a)
    assert rows(str(p) + "_changes.tsv") < rows(str(q) + "_changes.tsv")
    assert read(str(p) + "_edited.fa") != read(str(q) + "_edited.fa")
    print("rows of _changes.tsv: %d with the reject filter, %d without" % (rows(str(p) + "_changes.tsv"),
                                                                          rows(str(q) + "_changes.tsv")))


def test_snv_polish_with_the_reject_filter_built_from_the_reads(repeats, oracle_build):
    d, draft = repeats["dir"], repeats["draft"]
    p, _ = one_step(repeats, "snv", ["-s", 1])
    a, b = str(p) + ".a.bf", str(p) + ".b.bf"
    run([NTEDIT, "-f", draft, "-r", a, "-e", b, "-s", 1, "-b", d / "snv_two"])
    H.run_oracle(str(draft), a, H.default_params(snv=1), str(d / "snv_oracle"), rep_path=b)
    body = H.vcf_body(str(p) + "_variants.vcf")
    assert len(body) > 20
    assert body == H.vcf_body(str(d / "snv_two_variants.vcf")) == H.vcf_body(str(d / "snv_oracle_variants.vcf"))
    for suffix in ("_edited.fa", "_changes.tsv"):
        assert read(str(p) + suffix) == read(str(d / "snv_two") + suffix) == read(str(d / "snv_oracle") + suffix), suffix


def test_default_reject_name_in_the_echo_and_no_file(repeats, tmp_path):
    r = subprocess.run([str(c) for c in [NTEDIT, "-f", repeats["draft"], "--reads", repeats["plain"]] + FILTER + REJECT],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    assert re.search(r"\n -e reads_k25_reject\.bf\n", r.stdout), r.stdout
    names = sorted(p.name for p in tmp_path.iterdir())
    # (the reference's prefix has no -e part, and neither filter is written)
    assert names == ["draft.fa_k25_z100_rreads_k25.bf_i5_d5_m0" + s for s in ("_changes.tsv", "_edited.fa", "_variants.vcf")]


# ------------------------------------------------------------------ 6. store, files and parser
def test_store_files_and_parser_give_the_same_two_filters(repeats):
    p, r = one_step(repeats, "one")
    assert "read the resident store" in r.stdout
    want = (read(str(p) + ".a.bf"), read(str(p) + ".b.bf"))
    bases = int(re.search(r"Pass 1 \(count\): (\d+) bases", r.stderr).group(1))
    for tag, extra in (("cap0", ["--resident_cap", 0]), ("small", ["--resident_cap", bases // 8, "--batch_bytes", 1 << 18])):
        q, r = one_step(repeats, tag, extra)
        assert "read the files" in r.stdout and "Resident store: released" in r.stderr, tag
        assert (read(str(q) + ".a.bf"), read(str(q) + ".b.bf")) == want, tag
        for suffix in ("_edited.fa", "_changes.tsv"):
            assert read(str(q) + suffix) == read(str(p) + suffix), (tag, suffix)
    # --gpu_parse on the plain file, from the store and from the files, against the host parser on the same file (half
    # the reads, 15x: the unit's k-mers are seen about 75 times, the others about 10 times)
    got, half = {}, ["--reject_cutoff", R_REPEAT // 2, "--reject_bf", 1 << 15]
    for tag, extra in (("host", []), ("gpu", ["--gpu_parse"]), ("gpu_cap0", ["--gpu_parse", "--resident_cap", 0])):
        q, r = one_step(repeats, "plain_" + tag, extra, reject=half, reads=[repeats["plain"]])
        if "gpu" in tag:
            m = re.search(r"--gpu_parse: (\d+) chunks parsed on the device", r.stderr)
            assert m and int(m.group(1)) > 0 and "unclean" not in r.stderr, r.stderr[-2000:]
        got[tag] = (read(str(q) + ".a.bf"), read(str(q) + ".b.bf"), read(str(q) + "_changes.tsv"))
    assert got["host"] == got["gpu"] == got["gpu_cap0"]
    assert H.load_bf(str(q) + ".b.bf")["data"].any()


# ------------------------------------------------------------------ 7. sharded
def test_make_reads_at_world_2_writes_the_tools_two_files(repeats):
    d = repeats["dir"]
    args = ["--reads"] + [str(f) for f in repeats["reads"]] + ["-k", str(K), "-c", "2", "--bf", str(1 << 20), "--sketch_bytes",
                                                              str(1 << 24), "--reject_cutoff", str(R_REPEAT), "--reject_bf",
                                                              str(1 << 15)]
    r = _binary(args + ["-o", str(d / "tool.a.bf"), "--reject_out", str(d / "tool.b.bf")])
    assert r.returncode == 0, r.stderr[-3000:]
    r = _driver(2, args + ["-o", str(d / "drv.a.bf"), "--reject_out", str(d / "drv.b.bf")], "gloo")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    assert r.stderr.count("Pass 1 (count)") == 2 and "ranges" in r.stderr  # (the plain file is cut into ranges)
    assert re.findall(r"exchange (\S+) of", r.stderr).count("or") == 4  # (two filters, two ranks)
    assert read(d / "drv.a.bf") == read(d / "tool.a.bf")
    assert read(d / "drv.b.bf") == read(d / "tool.b.bf")
    # and they are the files of the one-binary polish
    p, _ = one_step(repeats, "one")
    assert read(d / "tool.a.bf") == read(str(p) + ".a.bf") and read(d / "tool.b.bf") == read(str(p) + ".b.bf")


@pytest.mark.parametrize("world,backend", [(1, "nccl"), (2, "gloo")])
def test_run_reads_with_a_reject_cutoff_equals_the_one_binary_run(repeats, world, backend):
    ref, _ = one_step(repeats, "one")
    p = repeats["dir"] / ("run_w%d" % world)
    r = driver(world, ["-f", repeats["draft"], "--reads"] + repeats["reads"] + FILTER + REJECT +
               ["--save_bf", str(p) + ".a.bf", "--save_reject_bf", str(p) + ".b.bf", "-b", p, "--report"], backend)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    for suffix in ("_edited.fa", "_changes.tsv", ".a.bf", ".b.bf"):
        assert read(str(p) + suffix) == read(str(ref) + suffix), suffix
    assert H.vcf_body(str(p) + "_variants.vcf") == H.vcf_body(str(ref) + "_variants.vcf")
    reps = reports(r)
    assert [x["rank"] for x in reps] == list(range(world))
    for x in reps:
        rj = x["reads"]["reject"]
        assert rj["cutoff"] == R_REPEAT and rj["filter_bytes"] == 1 << 15 and rj["merge_ms"] >= 0
        assert [e["op"] for e in x["reads"]["exchanges"]] == ["sat-add", "or", "or"]
        assert x["reads"]["filter_bytes"] == 1 << 20 and x["reads"]["store"]["used"]
    assert "Reject Bloom filter saved to" in r.stderr
