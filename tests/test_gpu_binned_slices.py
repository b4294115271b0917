"""GPU tests of the partitioned screening's geometry beyond 1,024 slices: the partition kernel's wide layout (2,048 slices,
rings of 8 slots, 32-bit state words) against the CPU oracle's bitmap, bit for bit.

The test-only tuning key "bin_slice_log2" cuts a small filter into as many slices as a 4 GiB filter has, so every case
runs in milliseconds; "bin_ring" forces the ring size.  Every case checks that the geometry it asked for is the one
that ran, from the library's "bin_timing" line."""
import filecmp
import re

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

_GEOMETRY = re.compile(r"binned chunk \d+ k-mers, (\d+) slices of 2\^(\d+) bits \(rings of (\d+)\)")


def _ran(capfd):
    """the {(slices, slice_log2, ring slots)} of the record chunks since the last call, and their number"""
    found = [tuple(int(x) for x in m) for m in _GEOMETRY.findall(capfd.readouterr().err)]
    return set(found), len(found)


def _case(tmp, seed, **kw):
    kw.setdefault("n", 60000)  # x 3 contigs: 180,000 bases, 11 partition workgroups
    kw.setdefault("flavor", "N rep")
    case = H.make_case(str(tmp), seed, **kw)
    bf = H.load_bf(case["bf"])
    recs = H.read_fasta(case["draft"])
    blob = H.pack_batch(recs)[0]
    return dict(case=case, bf=bf, recs=recs, blob=blob)


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


def _screen(c, tune, capfd, **params):
    pol = _polisher(c["bf"], tune, **params)
    try:
        capfd.readouterr()
        got = pol.screen(c["blob"])
    finally:
        pol.close()
    geo, chunks = _ran(capfd)
    return got, geo, chunks


@pytest.fixture(scope="module")
def plain16(tmp_path_factory, oracle_build):
    """a plain 16 MiB filter (k = 25, h = 3): 2,048 slices of 2^16 slots; the oracle's bitmap of its draft"""
    c = _case(tmp_path_factory.mktemp("plain16"), 9100, bfbytes=1 << 24)
    c["want"] = H.oracle_screen(c["blob"], c["bf"])
    c["want"].setflags(write=False)
    return c


@pytest.fixture(scope="module")
def plain16_oracle_files(plain16, tmp_path_factory, oracle_build):
    out = tmp_path_factory.mktemp("plain16_oracle")
    H.run_oracle(plain16["case"]["draft"], plain16["case"]["bf"], H.default_params(), str(out / "o"), plain16["case"]["rep"])
    return out


@pytest.mark.parametrize("bin_chunk", [0, 3 * 16384])
def test_2048_slices(plain16, bin_chunk, capfd):
    got, geo, chunks = _screen(plain16, dict(bin_slice_log2=16, bin_chunk=bin_chunk), capfd)
    assert geo == {(2048, 16, 8)}
    assert chunks == 1 if bin_chunk == 0 else chunks >= 4
    assert np.array_equal(got, plain16["want"])


def test_1526_slices_of_a_filter_that_is_no_power_of_two(tmp_path, capfd, oracle_build):
    c = _case(tmp_path, 9200, bfbytes=100000007)
    got, geo, _ = _screen(c, dict(bin_slice_log2=19), capfd)
    assert geo == {(1526, 19, 8)}
    assert np.array_equal(got, H.oracle_screen(c["blob"], c["bf"]))


@pytest.mark.parametrize("hashes", [1, 2, 4, 5])
def test_2048_slices_other_hash_counts(tmp_path, hashes, capfd, oracle_build):
    """h <= 2 runs two k-mers per thread and round, h = 5 has the most tokens per round"""
    c = _case(tmp_path, 9300 + hashes, bfbytes=1 << 24, hashes=hashes)
    got, geo, _ = _screen(c, dict(bin_slice_log2=16), capfd)
    assert geo == {(2048, 16, 8)}
    assert np.array_equal(got, H.oracle_screen(c["blob"], c["bf"]))


@pytest.mark.parametrize("percent", [50, 5])
def test_2048_slices_overflow_list(plain16, percent, capfd):
    got, geo, _ = _screen(plain16, dict(bin_slice_log2=16, bin_cap_percent=percent), capfd)
    assert geo == {(2048, 16, 8)}
    assert np.array_equal(got, plain16["want"])


def test_2048_slices_lost_chunks_are_screened_again(plain16, plain16_oracle_files, tmp_path, capfd):
    """an overflow list that runs out in every forced chunk: the direct kernel screens those chunks again"""
    tune = dict(bin_slice_log2=16, bin_cap_percent=5, bin_chunk=3 * 16384, bin_ovf_cap=4096)
    pol = _polisher(plain16["bf"], tune)
    try:
        capfd.readouterr()
        got = pol.screen(plain16["blob"])
        geo, chunks = _ran(capfd)
        st = pol.polish_records(plain16["recs"], str(tmp_path / "g"))
    finally:
        pol.close()
    assert geo == {(2048, 16, 8)} and chunks >= 4
    assert np.array_equal(got, plain16["want"])
    assert st.screen_binned and st.screen_chunks_direct > 0
    for suffix in ("_edited.fa", "_changes.tsv"):
        assert filecmp.cmp(str(plain16_oracle_files / ("o" + suffix)), str(tmp_path / ("g" + suffix)), shallow=False)


@pytest.mark.parametrize("xcc", [1, 13])
def test_2048_slices_on_one_xcd(plain16, xcc, capfd):
    got, geo, _ = _screen(plain16, dict(bin_slice_log2=16, force_xcc=xcc), capfd)
    assert geo == {(2048, 16, 8)}
    assert np.array_equal(got, plain16["want"])


def test_2048_slices_of_a_counting_filter(tmp_path, capfd, oracle_build):
    """2^21 8-bit counters in 2,048 slices of 2^10, -p 2"""
    c = _case(tmp_path, 9600, bfbytes=1 << 18, flavor="cbf N rep")
    assert c["bf"]["counting"] and c["bf"]["bytes"] == 1 << 21
    got, geo, _ = _screen(c, dict(bin_slice_log2=10), capfd, min_threshold=2)
    assert geo == {(2048, 10, 8)}
    assert np.array_equal(got, H.oracle_screen(c["blob"], c["bf"], min_threshold=2))


@pytest.mark.parametrize("ring", [8, 16])
@pytest.mark.parametrize("slices", [1, 3])
def test_few_slices_overrun_the_ring_every_round(tmp_path, slices, ring, capfd, oracle_build):
    """1,024 threads x 3 records a round for one slice or three: the ring takes a group, the rest is stored directly and
    the group's token says from which lane on the ring still holds it"""
    c = _case(tmp_path, 9700 + slices, bfbytes=slices << 21)
    got, geo, _ = _screen(c, dict(bin_ring=ring), capfd)
    assert geo == {(slices, 24, ring)}
    assert np.array_equal(got, H.oracle_screen(c["blob"], c["bf"]))


def test_barrier_free_kernel_keeps_1024_slices(plain16, tmp_path, capfd):
    """"bin_scatter" 1 has rings for 1,024 slices: the geometry follows the kernel that runs, and stays binned"""
    pol = _polisher(plain16["bf"], dict(bin_slice_log2=16, bin_scatter=1))
    try:
        capfd.readouterr()
        got = pol.screen(plain16["blob"])
        geo, _ = _ran(capfd)
        st = pol.polish_records(plain16["recs"], str(tmp_path / "g"))
    finally:
        pol.close()
    assert geo == {(1024, 17, 16)}
    assert np.array_equal(got, plain16["want"])
    assert st.screen_binned and st.screen_chunks_direct == 0


def test_2048_slices_at_k_200(tmp_path, capfd, oracle_build):
    """the LDS guard: the partition kernel's LDS does not grow with k, 2,048 slices stay on the binned pipeline"""
    c = _case(tmp_path, 9900, bfbytes=1 << 24, k=200)
    pol = _polisher(c["bf"], dict(bin_slice_log2=16))
    try:
        capfd.readouterr()
        got = pol.screen(c["blob"])
        geo, _ = _ran(capfd)
        st = pol.polish_records(c["recs"], str(tmp_path / "g"))
        geo_polish, _ = _ran(capfd)
    finally:
        pol.close()
    assert geo == {(2048, 16, 8)} and geo_polish == {(2048, 16, 8)}
    assert st.screen_binned
    assert np.array_equal(got, H.oracle_screen(c["blob"], c["bf"]))


def test_polish_at_2048_slices(plain16, plain16_oracle_files, tmp_path, capfd):
    pol = _polisher(plain16["bf"], dict(bin_slice_log2=16))
    try:
        capfd.readouterr()
        st = pol.polish_records(plain16["recs"], str(tmp_path / "g"))
    finally:
        pol.close()
    geo, _ = _ran(capfd)
    assert geo == {(2048, 16, 8)}
    assert st.screen_binned and st.screen_chunks_direct == 0
    for suffix in ("_edited.fa", "_changes.tsv"):
        assert filecmp.cmp(str(plain16_oracle_files / ("o" + suffix)), str(tmp_path / ("g" + suffix)), shallow=False)


def test_automatic_geometry_asks_for_long_runs(plain16, capfd):
    """a 4 GiB filter without "bin_slice_log2": 1,024 slices of 4 MiB while a (slice, workgroup) pair expects fewer records
    than the rule asks for (this draft: one), 2,048 slices of 2 MiB from there on; an empty filter: every k-mer is absent,
    and the direct kernel says the same"""
    import ntedit_amd
    import torch
    bits = torch.zeros(1 << 32, dtype=torch.uint8, device="cuda")
    pol = ntedit_amd.Polisher(0)
    try:
        pol.set_filter_device(bits.data_ptr(), 1 << 32, 3, 25)
        pol.set_params(ntedit_amd.default_params(screen_mode=2))
        pol.set_tuning("bin_timing", 1)
        capfd.readouterr()
        short_runs = pol.screen(plain16["blob"])
        geo_short, _ = _ran(capfd)
        pol.set_tuning("bin_wide_min_run", 1)
        long_runs = pol.screen(plain16["blob"])
        geo_long, _ = _ran(capfd)
        pol.set_params(ntedit_amd.default_params(screen_mode=1))
        direct = pol.screen(plain16["blob"])
    finally:
        pol.close()
    assert geo_short == {(1024, 25, 16)}
    assert geo_long == {(2048, 24, 8)}
    assert np.array_equal(short_runs, direct) and np.array_equal(long_runs, direct)
    assert int(np.unpackbits(direct.view(np.uint8)).sum()) > 100000
