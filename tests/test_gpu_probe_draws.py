"""GPU tests of the partitioned screening: the partition kernel's tile of 1,024 threads x 32 starts from packed 4-bit codes
(nte_tile.h, nte_bin_wc.inc) and the probe stage's step-major draws (nte_probe_draw.h): the partition
kernels' drain records every slice's longest run, k_bin_probe's counter enumerates 512-record steps with the run index
fastest and ends behind the longest run's last step.  Every bitmap is compared with the CPU oracle's, bit for bit, with
screen_mode=2; small filters are cut with the test-only tuning key "bin_slice_log2" into as many slices as a 4 GiB filter
has, and every case checks from the library's "bin_timing" line that the binned path ran with the geometry it asked for.

  runs        one and three slices (every round overruns the ring: groups leave behind direct stores), h = 1, 2, 5, runs
              that end at `cap` and feed the overflow list, the narrow 1,024-slice layout
  draws       a short draft that leaves slices without a record, 11 runs per slice (no multiple of a draw's 8 steps), one
              XCD, slices probed in 2 and 4 parts, several record chunks (the longest-run words are zeroed per chunk), a
              counting filter with -p 2, the candidate map of -s 1, a whole polish
  tiles, k    (the packed tile: 32,768 starts, words of eight codes, the entering code funnelled by k mod 8 nibbles)
              batch lengths around multiples of the partition tile, batches of k - 1, k and 32,767 bytes, an N-run and an
              IUPAC code across byte 32,768, contigs shorter than k between long ones; k = 24, 25, 31, 32, 33 and 200"""
import filecmp
import os
import re

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

_GEOMETRY = re.compile(r"binned chunk \d+ k-mers, (\d+) slices of 2\^(\d+) bits \(rings of (\d+)\)")


def _case(tmp, seed, **kw):
    kw.setdefault("n", 60000)  # x 3 contigs: 180,000 bases, 11 partition workgroups
    kw.setdefault("flavor", "N rep")
    case = H.make_case(str(tmp), seed, **kw)
    bf = H.load_bf(case["bf"])
    recs = H.read_fasta(case["draft"])
    return dict(case=case, bf=bf, recs=recs, blob=H.pack_batch(recs)[0])


def _polisher(bf, tune, **params):
    import ntedit_amd
    pol = ntedit_amd.Polisher(0)
    try:
        pol.set_filter(bf["data"], bf["hash_num"], bf["k"], counting=bool(bf.get("counting")))
        pol.set_params(ntedit_amd.default_params(screen_mode=2, **params))
        pol.set_tuning("bin_timing", 1)
        for key, value in tune.items():
            pol.set_tuning(key, value)
    except Exception:
        pol.close()
        raise
    return pol


def _geometry(capfd):
    return {tuple(int(x) for x in m) for m in _GEOMETRY.findall(capfd.readouterr().err)}


def _screen(c, tune, capfd, **params):
    pol = _polisher(c["bf"], tune, **params)
    try:
        capfd.readouterr()
        got = pol.screen(c["blob"])
    finally:
        pol.close()
    return got, _geometry(capfd)


@pytest.fixture(scope="module")
def plain16(tmp_path_factory, oracle_build):
    """a plain 16 MiB filter (k = 25, h = 3): 2,048 slices of 2^16 slots; the oracle's bitmap of its draft"""
    c = _case(tmp_path_factory.mktemp("draws16"), 9110, bfbytes=1 << 24)
    c["want"] = H.oracle_screen(c["blob"], c["bf"])
    c["want"].setflags(write=False)
    return c


# ---------------------------------------------------------------- runs
@pytest.mark.parametrize("ring", [8, 16])
@pytest.mark.parametrize("slices", [1, 3])
def test_few_slices_with_very_long_runs(tmp_path, slices, ring, capfd, oracle_build):
    """3,072 records a round for one slice or three: a ring-full stays, the rest is stored directly (tokens whose `first`
    field is not zero); the slice's runs are as long as `cap` lets them be"""
    c = _case(tmp_path, 9710 + slices, bfbytes=slices << 21)
    got, geo = _screen(c, dict(bin_ring=ring), capfd)
    assert geo == {(slices, 24, ring)}
    assert np.array_equal(got, H.oracle_screen(c["blob"], c["bf"]))


@pytest.mark.parametrize("hashes", [1, 2, 5])
def test_other_hash_counts(tmp_path, hashes, capfd, oracle_build):
    """h <= 2: two k-mer starts per thread and round; h = 5: the most tokens per round"""
    c = _case(tmp_path, 9310 + hashes, bfbytes=1 << 24, hashes=hashes)
    got, geo = _screen(c, dict(bin_slice_log2=16), capfd)
    assert geo == {(2048, 16, 8)}
    assert np.array_equal(got, H.oracle_screen(c["blob"], c["bf"]))


@pytest.mark.parametrize("percent", [50, 5])
def test_runs_that_end_at_cap(plain16, percent, capfd):
    """runs that fill up -- the longest run of every slice is `cap` -- and an overflow list beside them"""
    got, geo = _screen(plain16, dict(bin_slice_log2=16, bin_cap_percent=percent), capfd)
    assert geo == {(2048, 16, 8)}
    assert np.array_equal(got, plain16["want"])


def test_1024_slices_with_rings_of_16(plain16, capfd):
    """the narrow layout: 64-bit state words in the drain that records the longest run"""
    got, geo = _screen(plain16, dict(bin_slice_log2=17), capfd)
    assert geo == {(1024, 17, 16)}
    assert np.array_equal(got, plain16["want"])


# ---------------------------------------------------------------- draws
def test_short_draft_leaves_slices_without_a_record(tmp_path, capfd, oracle_build):
    """20,000 bases at 2,048 slices: short runs, slices with none -- each still hands out its one draw"""
    c = _case(tmp_path, 9410, n=6667, bfbytes=1 << 24)
    got, geo = _screen(c, dict(bin_slice_log2=16), capfd)
    assert geo == {(2048, 16, 8)}
    assert np.array_equal(got, H.oracle_screen(c["blob"], c["bf"]))


@pytest.mark.parametrize("tune", [dict(), dict(force_xcc=1), dict(probe_parts_log2=1), dict(probe_parts_log2=2),
                                  dict(bin_chunk=3 * 16384)], ids=lambda t: "-".join("%s%d" % kv for kv in t.items()) or "plain")
def test_draws_in_step_major_order(plain16, tune, capfd):
    """11 runs per slice (no multiple of a draw's 8 steps): as it comes, on one XCD, slices probed in parts, several record
    chunks (the longest-run words are zeroed per chunk)"""
    got, geo = _screen(plain16, dict(bin_slice_log2=16, **tune), capfd)
    assert geo == {(2048, 16, 8)}
    assert np.array_equal(got, plain16["want"])


def test_counting_filter_with_p_2(tmp_path, capfd, oracle_build):
    """2^21 8-bit counters in 2,048 slices of 2^10, -p 2: a slot is a byte, "absent" = counter < 2"""
    c = _case(tmp_path, 9610, bfbytes=1 << 18, flavor="cbf N rep")
    assert c["bf"]["counting"] and c["bf"]["bytes"] == 1 << 21
    got, geo = _screen(c, dict(bin_slice_log2=10), capfd, min_threshold=2)
    assert geo == {(2048, 10, 8)}
    assert np.array_equal(got, H.oracle_screen(c["blob"], c["bf"], min_threshold=2))


def _polish_equals_oracle(c, tmp_path, tune, capfd, **params):
    """a whole polish: _edited.fa and _changes.tsv identical to the oracle's; returns the geometries that ran"""
    import ntedit_amd
    H.run_oracle(c["case"]["draft"], c["case"]["bf"], H.default_params(**params), str(tmp_path / "o"), c["case"]["rep"])
    pol = ntedit_amd.Polisher(0)
    try:
        pol.load_filter_file(c["case"]["bf"], 0)
        pol.set_params(ntedit_amd.default_params(screen_mode=2, **params))
        pol.set_tuning("bin_timing", 1)
        for key, value in tune.items():
            pol.set_tuning(key, value)
        capfd.readouterr()
        st = pol.polish_records(c["recs"], str(tmp_path / "g"))
    finally:
        pol.close()
    geo = _geometry(capfd)
    for suffix in ("_edited.fa", "_changes.tsv"):
        assert filecmp.cmp(str(tmp_path / ("o" + suffix)), str(tmp_path / ("g" + suffix)), shallow=False), suffix
    return st, geo


def test_candidate_map_of_snv_mode(tmp_path, capfd, oracle_build):
    """-s 1 with "candmap" 1: the partition kernel's MODE 1 records, the probe stage ORs the bits that ARE set"""
    c = _case(tmp_path, 9810, n=50000, bfbytes=1 << 22, flavor="N lower iupac")
    st, geo = _polish_equals_oracle(c, tmp_path, dict(candmap=1), capfd, snv=1)
    assert geo, "no record chunk was reported: the candidate map did not go through the binned pipeline"
    assert H.vcf_body(str(tmp_path / "o_variants.vcf")) == H.vcf_body(str(tmp_path / "g_variants.vcf"))


def test_whole_polish_at_2048_slices(plain16, tmp_path, capfd):
    st, geo = _polish_equals_oracle(plain16, tmp_path, dict(bin_slice_log2=16), capfd)
    assert geo == {(2048, 16, 8)}
    assert st.screen_binned and st.screen_chunks_direct == 0


# ---------------------------------------------------------------- tiles, k
def _planted(tmp, seed, contigs, k=25, plant=()):
    """a draft of contigs of the given lengths (substitutions only: the lengths hold) over a 16 MiB filter of its truth;
    plant: (contig, position, bytes) written over the draft"""
    os.makedirs(str(tmp), exist_ok=True)
    rng = np.random.default_rng(seed)
    truth = [H.random_genome(rng, n) for n in contigs]
    H.write_fasta(os.path.join(str(tmp), "truth.fa"), [(b"t%d" % i, s) for i, s in enumerate(truth)] + [(b"more", H.random_genome(rng, 1000))])
    H.mkbf([os.path.join(str(tmp), "truth.fa")], os.path.join(str(tmp), "t.bf"), k=k, hashes=3, nbytes=1 << 24)
    draft = [bytearray(H.mutate(rng, s, 2e-3, 0.0, 0.0)) for s in truth]
    for ci, pos, what in plant:
        draft[ci][pos:pos + len(what)] = what
    recs = [(b"c%d" % i, bytes(d)) for i, d in enumerate(draft)]
    blob = H.pack_batch(recs)[0]
    assert len(blob) == sum(contigs) + len(contigs)
    return dict(bf=H.load_bf(os.path.join(str(tmp), "t.bf")), blob=blob)


def _check_2048(c, capfd):
    got, geo = _screen(c, dict(bin_slice_log2=16), capfd)
    assert geo == {(2048, 16, 8)}
    assert np.array_equal(got, H.oracle_screen(c["blob"], c["bf"]))


@pytest.mark.parametrize("d", [-17, -16, -1, 0, 1, 15, 16, 17])
def test_batch_lengths_around_whole_tiles(tmp_path, d, capfd, oracle_build):
    """one contig, a batch of 65,536 + d bytes (the separator included)"""
    _check_2048(_planted(tmp_path, 9500 + d, [65536 + d - 1]), capfd)


@pytest.mark.parametrize("length", [24, 25, 32767])
def test_short_batches(tmp_path, length, capfd, oracle_build):
    """batches of k - 1 (no k-mer at all), k (one) and 32,767 bytes"""
    c = _planted(tmp_path, 9520 + length % 97, [length - 1] if length > 25 else [length])
    if length <= 25:
        c["blob"] = c["blob"][:length]  # (without the separator: the batch ends with its last base)
    _check_2048(c, capfd)


@pytest.mark.parametrize("what", [b"N" * 15, b"R"], ids=["n_run", "iupac"])
def test_codes_across_byte_32768(tmp_path, what, capfd, oracle_build):
    _check_2048(_planted(tmp_path, 9540 + len(what), [70000], plant=[(0, 32768 - len(what) // 2, what)]), capfd)


def test_contigs_shorter_than_k_between_long_ones(tmp_path, capfd, oracle_build):
    _check_2048(_planted(tmp_path, 9550, [40000, 24, 1, 10, 40000]), capfd)


@pytest.mark.parametrize("k", [24, 25, 31, 32, 33, 200])
def test_other_k(tmp_path, k, capfd, oracle_build):
    """all residues of k mod 8 next to 32, and a k whose halo is most of a row"""
    c = _case(tmp_path, 9900 + k, bfbytes=1 << 24, k=k)
    _check_2048(c, capfd)
