"""`python -m ntedit_amd.run --reads` on the GPU: reads and a draft in, polished files out, the filter built by every rank
in HBM and never written or broadcast.  Every run is compared byte for byte with `ntedit --reads` with the same flags on
one GPU: _edited.fa, _changes.tsv, the VCF body, --save_bf and --hist.

1. where it runs: world 1 without a launcher, world 1 over RCCL, worlds 2 and 3 over gloo sharing one GPU;
2. modes: --cutoff, --solid, --counts -p 2 and -s 1, one case with contigs cut into segments;
3. the resident store forced off (--resident_cap 0) and a cap smaller than one rank's share: the same bytes;
4. the oracle, given the saved filter, agrees; the default output names are those of `ntedit --reads`;
5. a multi-line FASTQ cut into ranges is refused, naming --no-split, and leaves no output;
6. the resident store beside an adopted sketch (ntedit_hip_sketch_set_device) through the C ABI.

The reads: 30x of the draft's genome in a gzip FASTQ (one unit, whole), a plain FASTQ with awkward reads (N runs, lower
case, reads shorter than k) and a plain FASTA, both cut into ranges at world > 1.  Every subprocess runs under a timeout,
and a test starts at most 3 processes that hold the GPU at a time."""
import gzip
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from reads_model import awkward_reads, simulate_reads
from test_gpu_reads_bf import NTEDIT, write_fasta, write_fastq
from test_gpu_reads_multi import _multiline_fastq

pytestmark = pytest.mark.gpu

K = 25
SKETCH = 1 << 22
OUTPUTS = ("_edited.fa", "_changes.tsv")

# name: (filter flags, polish flags, oracle params)
CONFIGS = {
    "cutoff": (["--bf", 1 << 20, "--cutoff", 2], [], {}),
    "solid": (["--solid"], [], {}),
    "counts": (["--bf", 1 << 20, "--counts", "--cutoff", 2], ["-p", 2], dict(min_threshold=2)),
    "snv": (["--bf", 1 << 20, "--cutoff", 2], ["-s", 1], dict(snv=1)),
}


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("reads_run")
    rng = np.random.default_rng(41)
    truth = H.random_genome(rng, 150000)
    draft = H.mutate(rng, truth, p_sub=2e-3, p_ins=3e-4, p_del=3e-4)
    H.write_fasta(str(d / "draft.fa"), [(b"ctg1", draft[:100000]), (b"ctg2", draft[100000:])], width=80)
    reads = [bytes(r) for r in simulate_reads(rng, truth, 30)]
    third = len(reads) // 3
    awkward = []
    for i, r in enumerate(awkward_reads(K, seed=23, genome_len=20000)):
        awkward.append(r[:40].lower() + r[40:] if i % 5 == 0 else r)
    assert any(len(r) < K for r in awkward) and any(b"N" in r for r in awkward)
    files = [d / "r1.fq.gz", d / "r2.fq", d / "r3.fa"]
    write_fastq(files[0], reads[:third], opener=gzip.open)
    write_fastq(files[1], reads[third:2 * third] + awkward)
    write_fasta(files[2], reads[2 * third:])
    return dict(dir=d, draft=d / "draft.fa", reads=[str(f) for f in files], refs={})


def run_ntedit(args, cwd=None, timeout=600):
    r = subprocess.run([NTEDIT] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, cwd=cwd)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def driver(world, args, backend=None, cwd=None, timeout=600):
    """world 0: plain, without a launcher; else under torch.distributed.run with `world` ranks"""
    if world == 0:
        cmd = [sys.executable, "-m", "ntedit_amd.run"]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", str(world),
               "--master-port", str(29561 + world), "-m", "ntedit_amd.run", "--backend", backend]
    env = dict(os.environ, PYTHONPATH=H.ROOT, OMP_NUM_THREADS="4")
    return subprocess.run(cmd + [str(a) for a in args], capture_output=True, text=True, timeout=timeout,
                          cwd=str(cwd or H.ROOT), env=env)


def reports(r):
    return sorted((json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")), key=lambda x: x["rank"])


def reference(case, name):
    """`ntedit --reads` with the config's flags on one GPU (once per config)"""
    if name not in case["refs"]:
        filt, polish, _ = CONFIGS[name]
        p = case["dir"] / ("ref_" + name)
        r = run_ntedit(["-f", case["draft"], "--reads"] + case["reads"] + ["-k", K, "--sketch_bytes", SKETCH] + filt +
                       polish + ["--hist", str(p) + ".hist", "--save_bf", str(p) + ".bf", "-b", p])
        m = re.search(r"Pass 1 \(count\): (\d+) bases", r.stderr)
        assert m, r.stderr
        case["refs"][name] = (p, int(m.group(1)))
    return case["refs"][name]


def compare(case, name, world, backend=None, extra=()):
    ref, ref_bases = reference(case, name)
    filt, polish, _ = CONFIGS[name]
    tag = "%s_w%d_%s_%d" % (name, world, backend, len(extra))
    p = case["dir"] / tag
    r = driver(world, ["-f", case["draft"], "--reads"] + case["reads"] + ["-k", K, "--sketch_bytes", SKETCH] + filt +
               polish + ["--hist", str(p) + ".hist", "--save_bf", str(p) + ".bf", "-b", p, "--report"] + list(extra),
               backend)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert read(str(p) + ".bf") == read(str(ref) + ".bf"), tag
    assert read(str(p) + ".hist") == read(str(ref) + ".hist"), tag
    for suffix in OUTPUTS:
        assert read(str(p) + suffix) == read(str(ref) + suffix), (tag, suffix)
    assert H.vcf_body(str(p) + "_variants.vcf") == H.vcf_body(str(ref) + "_variants.vcf"), tag
    reps = reports(r)
    assert [x["rank"] for x in reps] == list(range(max(1, world))), r.stdout
    # every rank counted its own share in pass 1, and the shares add up to the reads
    assert r.stderr.count("Pass 1 (count)") == max(1, world)
    assert sum(x["reads"]["passes"]["1"]["bases"] for x in reps) == ref_bases
    for x in reps:
        assert {"1", "2"} <= set(x["reads"]["passes"]) and x["reads"]["filter_bytes"] > 0
    if world > 1:
        assert all(0 < x["reads"]["passes"]["1"]["bases"] < ref_bases for x in reps)
        assert all(x["reads"]["exchange_bytes"] > 0 for x in reps)
    return r, reps, p


# ------------------------------------------------------------------ 1. + 2. where it runs, modes
def test_world_1_plain_without_a_launcher(case):
    r, reps, _ = compare(case, "cutoff", 0)
    assert reps[0]["world"] == 1 and reps[0]["reads"]["exchanges"] == []
    assert reps[0]["reads"]["store"]["used"] and not reps[0]["reads"]["store"]["fallback"]
    assert re.search(r"Resident store: \d+ batches", r.stderr), r.stderr[-3000:]


def test_world_1_rccl_solid(case):
    r, reps, _ = compare(case, "solid", 1, "nccl")
    assert "rccl" in r.stderr and {"1", "H", "2"} == set(reps[0]["reads"]["passes"])
    assert [e["op"] for e in reps[0]["reads"]["exchanges"]] == ["sat-add", "sum", "or"]


@pytest.mark.parametrize("world,name", [(2, "cutoff"), (3, "solid"), (3, "snv")])  # (--counts: the oracle test)
def test_gloo_worlds(case, world, name):
    extra = ["--seg-bases", 20000] if name == "cutoff" else []
    r, reps, _ = compare(case, name, world, "gloo", extra)
    assert all(x["reads"]["store"]["used"] for x in reps)
    assert r.stderr.count("Resident store: ") == world
    if extra:  # contigs of 100 and 50 kbp cut into segments of about 20 kbp
        assert sum(x["segments"] for x in reps) >= 2, reps
    # the histogram pass and pass 2 read the store: their bases are pass 1's
    for x in reps:
        passes = x["reads"]["passes"]
        assert all(v["bases"] == passes["1"]["bases"] for v in passes.values())


# ------------------------------------------------------------------ 3. the resident store off and past its cap
def test_store_forced_off(case):
    r, reps, _ = compare(case, "solid", 2, "gloo", ["--resident_cap", 0])
    assert r.stderr.count("would pass its cap of 0 bytes") == 2
    assert all(x["reads"]["store"]["fallback"] and not x["reads"]["store"]["used"] for x in reps)
    assert r.stderr.count("Pass H (histogram)") == 2 and "batches of the resident store" not in r.stderr


def test_store_cap_smaller_than_a_rank_share(case):
    # small batches, so that a few are stored before the cap is passed
    r, reps, _ = compare(case, "cutoff", 3, "gloo", ["--resident_cap", 100000, "--batch_bytes", 65536])
    assert r.stderr.count("would pass its cap of 100000 bytes") >= 1
    assert any(x["reads"]["store"]["fallback"] for x in reps)


# ------------------------------------------------------------------ 4. the oracle, default names
def test_oracle_agrees_given_the_saved_filter(case, oracle_build):
    _, reps, p = compare(case, "counts", 2, "gloo")
    assert all(x["reads"]["store"]["used"] for x in reps)
    o = case["dir"] / "oracle_counts"
    H.run_oracle(str(case["draft"]), str(p) + ".bf", H.default_params(**CONFIGS["counts"][2]), str(o))
    for suffix in OUTPUTS:
        assert read(str(p) + suffix) == read(str(o) + suffix), suffix


def test_default_output_names_are_those_of_ntedit_reads(case, tmp_path):
    args = ["-f", case["draft"], "--reads"] + case["reads"] + ["-k", K, "--bf", 1 << 20, "--cutoff", 2,
                                                               "--sketch_bytes", SKETCH]
    for tag, extra in (("default", []), ("saved", ["--save_bf", "mine.bf"])):
        one, drv = tmp_path / ("one_" + tag), tmp_path / ("run_" + tag)
        one.mkdir()
        drv.mkdir()
        run_ntedit(args + extra, cwd=one)
        r = driver(0, args + extra, cwd=drv)
        assert r.returncode == 0, r.stderr[-3000:]
        names = sorted(os.listdir(drv))
        assert names == sorted(os.listdir(one)), (names, os.listdir(one))
        stem = "draft.fa_k25_z100_r%s_i5_d5_m0" % ("mine.bf" if extra else "reads_k25.bf")
        assert stem + "_edited.fa" in names
        for n in names:
            if not n.endswith(".vcf"):
                assert read(drv / n) == read(one / n), n


# ------------------------------------------------------------------ 5. a file that cannot be cut
def test_multiline_fastq_cut_into_ranges_is_refused(case, tmp_path):
    from ntedit_amd.make_reads import check_cuts, file_facts, plan
    from ntedit_amd import _lib
    import ctypes
    rng = np.random.default_rng(5)
    genome = H.random_genome(rng, 30000)
    ml = tmp_path / "multi.fq"
    _multiline_fastq(ml, [bytes(r) for r in simulate_reads(rng, genome, 20, length=151)])
    # the ranges of world 2 do not meet (host-only reader): the run has to refuse
    lib = _lib.load()
    units, _ = plan([str(ml)], file_facts(lib, [str(ml)]), 2)
    cuts = []
    for u in units:
        n, c, s, nx = (ctypes.c_uint64() for _ in range(4))
        lib.ntedit_hip_reads_range_text(str(ml).encode(), u.begin, u.end, None, 0, ctypes.byref(n), ctypes.byref(c),
                                        ctypes.byref(s), ctypes.byref(nx))
        cuts.append((u.file, u.begin, s.value, nx.value))
    assert check_cuts(cuts) is not None
    out = tmp_path / "out"
    out.mkdir()
    r = driver(2, ["-f", case["draft"], "--reads", ml, "-k", K, "--cutoff", 2, "--bf", 1 << 16, "--hist", "h.hist",
                   "--save_bf", "s.bf", "-b", "p"], "gloo", cwd=out)
    assert r.returncode != 0
    assert "--no-split" in r.stderr, r.stderr[-3000:]
    assert os.listdir(out) == []
    # and with --no-split the same file is read whole, as `ntedit --reads` reads it
    ref = tmp_path / "ref"
    run_ntedit(["-f", case["draft"], "--reads", ml, "-k", K, "--cutoff", 2, "--bf", 1 << 16, "--save_bf",
                str(ref) + ".bf", "-b", ref])
    r = driver(2, ["-f", case["draft"], "--reads", ml, "-k", K, "--cutoff", 2, "--bf", 1 << 16, "--no-split",
                   "--save_bf", "s.bf", "-b", "p"], "gloo", cwd=out)
    assert r.returncode == 0, r.stderr[-3000:]
    assert read(out / "s.bf") == read(str(ref) + ".bf")
    for suffix in OUTPUTS:
        assert read(str(out / "p") + suffix) == read(str(ref) + suffix), suffix


# ------------------------------------------------------------------ 6. the store beside an adopted sketch, through the C ABI
def test_store_over_an_adopted_sketch_equals_an_allocated_one():
    """ntedit_hip_resident_begin over a sketch adopted with ntedit_hip_sketch_set_device, as every rank of `run --reads`
    uses it: the same histogram and filter as beside ntedit_hip_sketch_alloc's sketch; ntedit_hip_sketch_free releases
    the store and leaves the adopted memory to its owner"""
    import ctypes
    import torch
    import ntedit_amd
    from ntedit_amd import _lib
    from reads_model import blob_of
    lib = _lib.load()
    blob = blob_of(awkward_reads(K, seed=7, genome_len=8000))
    half = blob.index(b"\n", len(blob) // 2) + 1
    counters, bf = 1 << 20, 1 << 15
    got = []
    for adopt in (False, True):
        pol = ntedit_amd.Polisher(0)
        try:
            h = pol._h
            if adopt:
                t = torch.zeros(counters, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                assert lib.ntedit_hip_sketch_set_device(h, t.data_ptr(), counters, 3, K) == 0
            else:
                assert lib.ntedit_hip_sketch_alloc(h, counters, 3, K) == 0
            assert lib.ntedit_hip_resident_begin(h, 1 << 30) == 0, lib.ntedit_hip_reads_last_error(h)
            for part in (blob[:half], blob[half:]):
                assert lib.ntedit_hip_sketch_count(h, part, len(part), 0) == 0, lib.ntedit_hip_reads_last_error(h)
            st = _lib.ResidentStats()
            assert lib.ntedit_hip_resident_info(h, ctypes.byref(st)) == 0
            assert st.state == _lib.RESIDENT_ON and st.batches == 2 and st.bases == len(blob)
            assert lib.ntedit_hip_resident_histogram(h) == 0, lib.ntedit_hip_reads_last_error(h)
            occ = np.zeros(256, dtype=np.uint64)
            assert lib.ntedit_hip_sketch_histogram_download(h, occ.ctypes.data_as(ctypes.c_void_p)) == 0
            pol.filter_alloc(bf, 3, K)
            assert lib.ntedit_hip_resident_insert_solid(h, 0, 2) == 0, lib.ntedit_hip_reads_last_error(h)
            got.append((occ, pol.filter_download(0)))
            lib.ntedit_hip_sketch_free(h)
            assert lib.ntedit_hip_resident_info(h, ctypes.byref(st)) != 0  # (gone with the sketch)
            if adopt:
                t.fill_(1)
                torch.cuda.synchronize()
                assert int(t.sum()) == counters
        finally:
            pol.close()
    assert got[0][0].sum() > 0 and got[0][1].any()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
