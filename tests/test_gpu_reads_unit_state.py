"""The per-context state of the three device units of the reads front end (nte_reads_unit.h: Keep and Scratch) on the GPU:
ntedit_hip_sketch_free takes the scratch and leaves the settings and the last pass's counts; two live contexts share no
setting; and the raw buffer and the line table grow, stay and are re-made for the quality sums under each caller's own
rule (reads, genome, the chunk cut) with every text the serial model's.  (The text buffer of the *_device calls is the caller's;
the unit's own is used by the one small pass of the first test and grows, by the same function, under the passes of the
other suites.)  Inputs are generated here."""
import ctypes
import random

import numpy as np
import pytest

import bam_corpus as BAM
import bgzf_corpus as BC
import genome_corpus as GC
import min_qual_twin as MQ
import parse_corpus as PC
import read_filter_twin as RF
from ntedit_amd import _lib

pytestmark = pytest.mark.gpu

K = RF.K
GUARD = 256
MIN_QUAL, MIN_LEN, MIN_MEAN_QUAL, MIN_RQ = 20, 40, 15, 0.9
SEGMENT, WIDTH = 256, 8
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def new_context():
    import torch  # noqa: F401  (torch's HIP runtime first, as the drivers load it)
    import ntedit_amd
    p = ntedit_amd.Polisher(0)
    # the reads settings hang off the context's address and ntedit_hip_destroy leaves them: a context made
    # where an earlier test's was inherits that test's, so each begins with every setting off
    lib, h = p._lib, p._h
    assert lib.ntedit_hip_reads_set_device_parse(h, 0) == 0 and lib.ntedit_hip_reads_set_min_qual(h, 0) == 0
    assert lib.ntedit_hip_reads_set_read_filter(h, 0, 0, 0.0) == 0
    assert lib.ntedit_hip_reads_bam_set_segment(h, 0) == 0 and lib.ntedit_hip_reads_bam_set_group_width(h, 0) == 0
    return p


def close(p):
    p._lib.ntedit_hip_sketch_free(p._h)  # (the units' scratch)
    p.close()


@pytest.fixture()
def pol():
    p = new_context()
    yield p
    close(p)


# ---------------------------------------------------------------------------------- the *_device entry points
def ok(pol, rc):
    assert rc == 0, pol._lib.ntedit_hip_reads_last_error(pol._h)


def parse_device(pol, raw, k=K):
    """ntedit_hip_reads_parse_device, host input -> (the result's fields, the text); the guard behind the cap is checked"""
    import torch
    cap = (len(raw) + 15) // 16 * 16
    text = torch.full((cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    res = _lib.ReadsParseResult()
    torch.cuda.synchronize()
    ok(pol, pol._lib.ntedit_hip_reads_parse_device(pol._h, raw, len(raw), 0, k, text.data_ptr(), cap, res))
    torch.cuda.synchronize()
    host = bytes(text.cpu().numpy())
    assert host[cap:] == b"\xEE" * GUARD
    return parse_fields(res), host[:res.text_len]


def parse_fields(res):
    return (res.clean, res.broken, res.kind, res.text_len, res.reads, res.bases)


def bam_device(pol, raw, min_len=K):
    import torch
    cap = len(raw)
    out = torch.full((GUARD + cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    res = _lib.ReadsBamResult()
    torch.cuda.synchronize()
    ok(pol, pol._lib.ntedit_hip_reads_bam_device(pol._h, raw, len(raw), 0, 1, min_len, out.data_ptr() + GUARD, cap, res))
    torch.cuda.synchronize()
    host = bytes(out.cpu().numpy())
    assert host[:GUARD] == b"\xEE" * GUARD and host[GUARD + cap:] == b"\xEE" * GUARD
    return BAM.result_dict(res), host[GUARD:GUARD + res.text_len]


def inflate_device(pol, blob, members, n_out):
    import torch
    out = torch.full((n_out + BC.GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    status = (ctypes.c_uint32 * max(len(members), 1))()
    torch.cuda.synchronize()
    ok(pol, pol._lib.ntedit_hip_reads_inflate_device(pol._h, blob, len(blob), 0, BC.table(members), len(members), out.data_ptr(), n_out,
                                                     status))
    torch.cuda.synchronize()
    host = bytes(out.cpu().numpy())
    assert host[n_out:] == b"\xEE" * BC.GUARD
    return list(status)[:len(members)], host[:n_out]


def genome_device(pol, raw):
    import torch
    cap = (len(raw) + 15) // 16 * 16
    text = torch.full((cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    res = _lib.GenomeParseResult()
    torch.cuda.synchronize()
    ok(pol, pol._lib.ntedit_hip_genome_parse_device(pol._h, raw, len(raw), 0, GC.LINE_START, 1, text.data_ptr(), cap, res))
    torch.cuda.synchronize()
    host = bytes(text.cpu().numpy())
    assert host[cap:] == b"\xEE" * GUARD
    return GC.fields(res), host[:res.text_len]


def last_start_device(pol, raw):
    got = ctypes.c_uint64()
    ok(pol, pol._lib.ntedit_hip_reads_last_start_device(pol._h, raw, len(raw), 0, got))
    return got.value


# ---------------------------------------------------------------------------------- what a context reports
INFOS = (("parse", _lib.ReadsParseStats, "ntedit_hip_reads_parse_info"), ("inflate", _lib.ReadsInflateStats, "ntedit_hip_reads_inflate_info"),
         ("bam", _lib.ReadsBamStats, "ntedit_hip_reads_bam_info"), ("genome", _lib.GenomePassInfo, "ntedit_hip_genome_pass_get_info"),
         ("filter", _lib.ReadsReadFilterStats, "ntedit_hip_reads_read_filter_info"))


def infos(pol):
    """every *_info struct, field by field, and the --min_qual counts"""
    out = {}
    for name, cls, call in INFOS:
        st = cls()
        ok(pol, getattr(pol._lib, call)(pol._h, st))
        out[name] = {f[0]: getattr(st, f[0]) for f in st._fields_ if isinstance(getattr(st, f[0]), (int, float))}
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    ok(pol, pol._lib.ntedit_hip_reads_min_qual_info(pol._h, a, b))
    out["min_qual"] = dict(qual_bases=a.value, masked_bases=b.value)
    return out


def counts_of(info):
    """the whole-number fields (a time grows by what the clock says: it is compared for not having gone back)"""
    return {(unit, f): v for unit, st in info.items() for f, v in st.items() if isinstance(v, int)}


def times_of(info):
    return {(unit, f): v for unit, st in info.items() for f, v in st.items() if isinstance(v, float)}


def read_filter(pol):
    a, b, r = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_float()
    ok(pol, pol._lib.ntedit_hip_reads_get_read_filter(pol._h, a, b, r))
    return a.value, b.value, r.value


# ---------------------------------------------------------------------------------- 1. scratch goes, settings and counts stay
def six_fastq_records():
    """reads on both sides of each rule at k 25, --min_read_len 40, --min_mean_qual 15, --min_qual 20"""
    rng = random.Random(1)
    seq = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    q = lambda level, n: bytes([33 + level]) * n
    some_low = bytearray(q(30, 60))
    for i in (0, 7, 16, 31, 59):  # five bases below --min_qual: masked, and the mean stays above 15
        some_low[i] = 33 + 10
    return [(b"short_of_min_len", seq(30), q(30, 30), None),          # 25 <= 30 < 40: dropped by length
            (b"good", seq(60), q(30, 60), None),                      # kept as it is
            (b"kept_and_masked", seq(60), bytes(some_low), None),     # kept, five bases to N
            (b"low_mean", seq(60), q(12, 60), None),                  # mean quality 12 < 15: dropped
            (b"at_both_thresholds", seq(40), q(15, 40), None),        # 40 bases of quality 15: kept, and every base masked
            (b"one_short", seq(39), q(40, 39), None)]                 # 39 < 40: dropped by length


def six_bam_records():
    """... and of --min_rq 0.9, with and without the tag; an odd length among them"""
    rng = random.Random(2)
    seq = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    q = lambda level, n: bytes([33 + level]) * n
    some_low = bytearray(q(30, 61))
    for i in (1, 2, 33, 60):
        some_low[i] = 33 + 19
    return [(b"good", seq(60), q(30, 60), 0.95),
            (b"low_rq", seq(60), q(30, 60), 0.85),                    # dropped by rq
            (b"short", seq(30), q(30, 30), 0.99),                     # dropped by length
            (b"low_mean", seq(60), q(12, 60), 0.99),                  # dropped by mean quality
            (b"rq_at_the_threshold", seq(61), bytes(some_low), RF.f32(MIN_RQ)),  # kept (>=), four bases masked
            (b"untagged", seq(60), q(30, 60), RF.NO_RQ)]              # no rq field: the rule does not apply


def test_sketch_free_takes_the_scratch_and_leaves_settings_and_counts(pol, tmp_path):
    lib, h = pol._lib, pol._h
    f = dict(L=MIN_LEN, Q=MIN_MEAN_QUAL)
    fq_recs, bam_recs = six_fastq_records(), six_bam_records()
    fq = RF.fastq_of(fq_recs)
    bam = RF.bam_of(bam_recs)[1]
    blob, members, n_out = BC.table_of([BC.member(fq)])
    # the models, and the twin's word on what they should be
    mres, mtext, mst = RF.parse_model_f(lib, fq, K, MIN_QUAL, MIN_LEN, MIN_MEAN_QUAL)
    assert mres.clean == 1 and mtext == RF.text_of(fq_recs, K, q=MIN_QUAL, **f) and mtext.count(b"\n") == 3 and b"N" * 40 + b"\n" in mtext
    assert RF.same_counts(mst, RF.counts(fq_recs, K, **f)) and mst[RF.LENGTH] == 2 and mst[RF.MEAN_QUAL] == 1
    bres, btext, bst = RF.bam_model_f(lib, bam, K, MIN_QUAL, MIN_LEN, MIN_MEAN_QUAL, MIN_RQ)
    assert bres.clean == 1 and btext == RF.text_of(bam_recs, K, q=MIN_QUAL, R=MIN_RQ, **f) and btext.count(b"\n") == 3 and b"N" in btext
    assert RF.same_counts(bst, RF.counts(bam_recs, K, R=MIN_RQ, **f)) and bst[RF.LENGTH] == bst[RF.RQ] == bst[RF.MEAN_QUAL] == 1
    assert BC.model(lib, blob, members, n_out) == ([0], fq)
    segments = (len(bam) + SEGMENT - 1) // SEGMENT
    assert segments > 1  # (one segment is what the default setting would make of so small a chunk)

    ok(pol, lib.ntedit_hip_reads_set_device_parse(h, 1))
    ok(pol, lib.ntedit_hip_reads_set_min_qual(h, MIN_QUAL))
    ok(pol, lib.ntedit_hip_reads_set_read_filter(h, MIN_LEN, MIN_MEAN_QUAL, MIN_RQ))
    ok(pol, lib.ntedit_hip_reads_bam_set_segment(h, SEGMENT))
    ok(pol, lib.ntedit_hip_reads_bam_set_group_width(h, WIDTH))

    def run():
        return parse_device(pol, fq), inflate_device(pol, blob, members, n_out), bam_device(pol, bam)

    zero = infos(pol)
    first = run()
    assert first == ((parse_fields(mres), mtext), ([0], fq), (BAM.result_dict(bres), btext))
    before = infos(pol)
    added = {key: v - counts_of(zero)[key] for key, v in counts_of(before).items()}
    assert added[("bam", "chunks")] == 1 and added[("bam", "segments")] == segments and added[("bam", "records")] == 6
    assert added[("min_qual", "masked_bases")] == 5 + 40 + 4 and added[("filter", "records")] == 12
    assert {key[1]: v for key, v in added.items() if key[0] == "filter"} == {name: mst[name] + bst[name] for name in mst}
    assert lib.ntedit_hip_reads_bam_group_width(h) == WIDTH and read_filter(pol) == (MIN_LEN, MIN_MEAN_QUAL, RF.f32(MIN_RQ))

    lib.ntedit_hip_sketch_free(h)
    assert read_filter(pol) == (MIN_LEN, MIN_MEAN_QUAL, RF.f32(MIN_RQ))
    assert lib.ntedit_hip_reads_bam_group_width(h) == 0  # (the width the last chunk ran at is scratch)
    assert infos(pol) == before

    # the same inputs again, on scratch made anew: masked, filtered, cut into segments of 256 bytes as before
    assert run() == first
    after = infos(pol)
    assert {key: v - counts_of(before)[key] for key, v in counts_of(after).items()} == added
    assert all(after_t >= times_of(before)[key] for key, after_t in times_of(after).items())
    assert lib.ntedit_hip_reads_bam_group_width(h) == WIDTH

    # device_parse is read by the pass alone: after another free a pass over the chunk as a file still parses it on the device
    lib.ntedit_hip_sketch_free(h)
    (tmp_path / "six.fq").write_bytes(fq)
    ok(pol, lib.ntedit_hip_sketch_alloc(h, 1 << 20, 3, K))
    files = (ctypes.c_char_p * 1)(str(tmp_path / "six.fq").encode())
    st = _lib.ReadsPassStats()
    ok(pol, lib.ntedit_hip_reads_pass(h, _lib.READS_PASS_COUNT, files, (ctypes.c_uint64 * 1)(0), (ctypes.c_uint64 * 1)((1 << 64) - 1), 1, 1 << 18,
                                      0, st, None, None))
    passed = infos(pol)
    assert passed["parse"]["device_chunks"] == 1 and passed["parse"]["fallback_chunks"] == 0
    assert st.bases == len(mtext) - mtext.count(b"\n")  # (masked and filtered by the settings that stayed)
    assert {name: passed["filter"][name] for name in mst} == mst and passed["min_qual"]["masked_bases"] == 5 + 40


# ---------------------------------------------------------------------------------- 2. two live contexts
@pytest.mark.parametrize("order", ["a_first", "b_first"])
def test_two_live_contexts_do_not_share_settings(order):
    recs = MQ.draw_records(random.Random(3), 40, lengths=(20, 120), q=30)
    raw = MQ.fastq(recs)
    a, b = new_context(), new_context()
    try:
        ok(a, a._lib.ntedit_hip_reads_set_min_qual(a._h, 30))
        ok(b, b._lib.ntedit_hip_reads_set_min_qual(b._h, 0))
        masked = MQ.parse_model_q(a._lib, raw, K, 30)[1]
        plain = PC.model(a._lib, raw, K)[1]
        assert masked == MQ.text_of(MQ.mask_records(recs, 30), K) and plain == MQ.text_of(recs, K) and b"N" in masked and b"N" not in plain
        got = {}
        for name in (("a", "b") if order == "a_first" else ("b", "a")) * 2:  # (each a second time, after the other has run)
            got[name] = parse_device(a if name == "a" else b, raw)[1]
            assert got[name] == (masked if name == "a" else plain), name
    finally:
        close(a)
        close(b)


# ---------------------------------------------------------------------------------- 3. growth and shrink on one context
SMALL, LARGE = 4 << 10, 5 << 19  # 4 KiB; 2.5 MiB: past the MiB of slack behind a 4 KiB chunk, so the raw buffer and the table are re-made


def fastq_of_size(seed, size):
    """4-line FASTQ records of 150 bases, quality levels around 20, at least `size` bytes"""
    rng = np.random.default_rng(seed)
    n = size // (10 + 151 + 2 + 151) + 1
    seqs = rng.choice(ACGT, (n, 150))
    level = 20 + rng.choice(np.array([-12, -3, -1, 0, 0, 1, 3, 15]), n)
    quals = (33 + np.clip(level[:, None] + rng.choice(np.array([-4, -1, 0, 0, 1, 6]), (n, 150)), 0, 60)).astype(np.uint8)
    return b"".join(b"@r%07d\n%s\n+\n%s\n" % (i, seqs[i].tobytes(), quals[i].tobytes()) for i in range(n))


def fasta_of_size(seed, size):
    """genome FASTA, lines of 60, a header every 50 lines, at least `size` bytes"""
    rng = np.random.default_rng(seed)
    n = size // 61 + 1
    lines = rng.choice(ACGT, (n, 60))
    return b"".join((b">contig%d\n" % i if i % 50 == 0 else b"") + lines[i].tobytes() + b"\n" for i in range(n))


@pytest.fixture(scope="module")
def chunks():
    return {"fq_small": fastq_of_size(1, SMALL), "fq_large": fastq_of_size(2, LARGE), "fa_small": fasta_of_size(3, SMALL),
            "fa_large": fasta_of_size(4, LARGE + (64 << 10))}  # (the genome's table rule: a MiB of slack counted in)


def check_reads(pol, raw, q=0, L=0, Q=0):
    lib = pol._lib
    ok(pol, lib.ntedit_hip_reads_set_min_qual(pol._h, q))
    ok(pol, lib.ntedit_hip_reads_set_read_filter(pol._h, L, Q, 0.0))
    mres, mtext, _ = RF.parse_model_f(lib, raw, K, q, L, Q)
    assert mres.clean == 1 and mres.reads > 0
    assert parse_device(pol, raw) == (parse_fields(mres), mtext)
    return mres.reads


def check_genome(pol, raw):
    mres, mtext = GC.model(pol._lib, raw)
    assert mres.clean == 1 and mres.text_len > 0
    assert genome_device(pol, raw) == (GC.fields(mres), mtext)


def check_cut(pol, raw):
    """a buffer that ends inside a record: the device's cut is the host rule's, and the parser's time does not move (the
    line table's kernels are inside the inflate unit's own event pair)"""
    raw = raw[:len(raw) - 57]
    want = pol._lib.ntedit_hip_reads_last_record_start(raw, len(raw), ord("@"))
    assert want not in (0, _lib.READS_NO_START) and raw[want:want + 2] == b"@r"
    before = infos(pol)
    assert last_start_device(pol, raw) == want
    after = infos(pol)
    assert after["parse"] == before["parse"] and after["genome"] == before["genome"]
    assert after["inflate"]["ms_kernels"] > before["inflate"]["ms_kernels"]


def test_reads_chunks_grow_shrink_and_gain_the_quality_sums(pol, chunks):
    small, large = chunks["fq_small"], chunks["fq_large"]
    for raw in (small, large, small):
        check_reads(pol, raw)
    # --min_mean_qual comes on: the table is made again for the sums, at the size it has
    all_reads = check_reads(pol, small)
    assert 0 < check_reads(pol, small, Q=20) < all_reads
    assert 0 < check_reads(pol, large, q=22, L=150, Q=21)
    check_reads(pol, small)


def test_genome_chunks_on_the_reads_table_and_on_their_own(pol, chunks):
    check_reads(pol, chunks["fq_small"], Q=20)  # (a table of the reads parser's, with sums)
    for name in ("fa_small", "fa_large", "fa_small"):
        check_genome(pol, chunks[name])
    check_reads(pol, chunks["fq_small"], Q=20)  # ... which gets its sums back
    pol._lib.ntedit_hip_sketch_free(pol._h)
    for name in ("fa_small", "fa_large", "fa_small"):  # from no table at all
        check_genome(pol, chunks[name])


def test_the_chunk_cut_on_the_same_table_adds_nothing_to_the_parsers_time(pol, chunks):
    check_genome(pol, chunks["fa_small"])
    for name in ("fq_small", "fq_large", "fq_small"):
        check_cut(pol, chunks[name])
    check_reads(pol, chunks["fq_small"], Q=20)
    check_cut(pol, chunks["fq_small"])
    pol._lib.ntedit_hip_sketch_free(pol._h)
    for name in ("fq_small", "fq_large", "fq_small"):  # from no table at all
        check_cut(pol, chunks[name])
