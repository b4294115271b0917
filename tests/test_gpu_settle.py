"""k_settle (ntedit_amd/csrc/nte_settle.hip) on the GPU: the plain substitution events of a batch settled in front of the
event machine's thread-per-event launch.  Results with and without it are identical and equal the oracle's; it settles
exactly the events the CPU program (tests/settle/settle_host.cpp) says settle_event() accepts; it stays off where the
machine is not restated."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import settle_case as S

pytestmark = pytest.mark.gpu

K, HASHES = 25, 3


@pytest.fixture(scope="module")
def case(tmp_path_factory, oracle_build):
    """the 2 Mbp i.i.d. case and the planted contigs in one batch, a 16 MiB filter, and the oracle's files for it"""
    tmp = str(tmp_path_factory.mktemp("settle_gpu"))
    c = S.make_settle_case(tmp, k=K, hashes=HASHES)
    c["tmp"] = tmp
    c["hp"] = dict(min_contig_len=0)
    H.run_oracle(c["draft"], c["bf"], H.default_params(**c["hp"]), os.path.join(tmp, "o"))
    c["recs"] = H.read_fasta(c["draft"])
    return c


def _polisher(case, **tuning):
    import ntedit_amd
    pol = ntedit_amd.Polisher(0)
    for key, v in tuning.items():
        pol.set_tuning(key, v)
    pol.load_filter_file(case["bf"])
    pol.set_params(ntedit_amd.default_params(**case["hp"]))
    return pol


def _counts(st):
    return tuple(getattr(st, f) for f in ("bases", "absent_kmers", "events", "events_applied", "substitutions", "insertions", "deletions"))


def _run(case, tag, **tuning):
    """one polish of the case: (edit records, pool, result counts, settle info); the files go to <tmp>/<tag>_*"""
    import ntedit_amd
    pol = _polisher(case, **tuning)
    try:
        blob, offs, lens, names = ntedit_amd.pack_batch(case["recs"], 0)
        res = pol.polish_batch(blob, offs, lens)
        info = pol.settle_info()
        recs, pool = res.edits(blob, offs, lens)
        prefix = os.path.join(case["tmp"], tag)
        pol.write_tsv_header(prefix + "_changes.tsv")
        open(prefix + "_edited.fa", "wb").close()
        res.write(blob, offs, lens, names, prefix + "_edited.fa", prefix + "_changes.tsv", append=True)
        st = _counts(res.stats())
        res.free()
    finally:
        pol.close()
    return recs, pool, st, info


def _same_as_oracle(case, tag):
    for suffix in ("_changes.tsv", "_edited.fa"):
        assert filecmp.cmp(os.path.join(case["tmp"], "o" + suffix), os.path.join(case["tmp"], tag + suffix), shallow=False), (tag, suffix)


@pytest.fixture(scope="module")
def cpu_settled(case):
    """events settle_event() accepts in the batch, by the CPU program (which also checks each against the machine)"""
    import ntedit_amd
    exe = S.build_settle_host(case["tmp"])
    blob, _, _, _ = ntedit_amd.pack_batch(case["recs"], 0)
    open(os.path.join(case["tmp"], "blob.bin"), "wb").write(blob)
    H.load_bf(case["bf"])["data"].tofile(os.path.join(case["tmp"], "bits.bin"))
    r = subprocess.run([exe, "count", os.path.join(case["tmp"], "blob.bin"), os.path.join(case["tmp"], "bits.bin"), str(K), str(HASHES)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-2000:]
    events, settled, mismatches = S.tally(r.stdout)
    assert mismatches == 0
    return events, settled


@pytest.mark.parametrize("rounds", ["no_rounds", "force_rounds"])
def test_results_identical_and_the_oracles(case, cpu_settled, rounds):
    off = _run(case, rounds + "_0", settle=0, **{rounds: 1})
    on = _run(case, rounds + "_1", settle=1, **{rounds: 1})
    assert off[3][:2] == (0, 0)
    assert np.array_equal(off[0], on[0]) and off[1] == on[1]
    assert off[2] == on[2]
    _same_as_oracle(case, rounds + "_0")
    _same_as_oracle(case, rounds + "_1")
    # it ran: without rounds every event is handed to it once, and it settles the events the CPU program counts
    seen, settled, ms = on[3]
    if rounds == "no_rounds":
        assert (seen, settled) == cpu_settled
    else:
        # in rounds an event that an earlier event's run overtakes is never handed to a launch, k_settle's included:
        # the kernel sees a subset of the events, which subset depends on the rounds, so only the bounds are fixed
        assert 0 < settled <= cpu_settled[1] and settled <= seen <= cpu_settled[0]
    assert settled * 2 >= seen and ms > 0


def test_auto_mode_small_batch_is_the_parents(case):
    """auto: a list of few events goes to the thread-per-event launch as it is"""
    recs, pool, st, info = _run(case, "auto")
    assert info[:2] == (0, 0)
    _same_as_oracle(case, "auto")


@pytest.mark.parametrize("what", ["secondary", "snv", "counting", "k65"])
def test_off_where_the_machine_is_not_restated(tmp_path, oracle_build, what):
    import ntedit_amd
    kw = dict(n=20000, contigs=2)
    par = {}
    if what == "secondary":
        kw["flavor"] = "sec"
    elif what == "snv":
        kw.update(n=6000)
        par["snv"] = 1
    elif what == "counting":
        kw["flavor"] = "cbf"
    else:
        kw["k"] = 65
    c = H.make_case(str(tmp_path), 77, **kw)
    H.run_oracle(c["draft"], c["bf"], H.default_params(**par), str(tmp_path / "o"), c["rep"])
    pol = ntedit_amd.Polisher(0)
    try:
        pol.set_tuning("settle", 1)
        pol.load_filter_file(c["bf"])
        if c["rep"]:
            pol.load_filter_file(c["rep"], 1)
        pol.set_params(ntedit_amd.default_params(**par))
        st = pol.polish_records(H.read_fasta(c["draft"]), str(tmp_path / "g"))
        info = pol.settle_info()
    finally:
        pol.close()
    assert st.events > 0 and info[:2] == (0, 0)
    assert filecmp.cmp(str(tmp_path / "o_changes.tsv"), str(tmp_path / "g_changes.tsv"), shallow=False)
    assert filecmp.cmp(str(tmp_path / "o_edited.fa"), str(tmp_path / "g_edited.fa"), shallow=False)


def test_arena_full_retry(case):
    """an arena k_settle's chunks do not fit in: EV_ARENA_FULL, the batch runs again with four times as much"""
    roomy = _run(case, "roomy", settle=1, no_rounds=1)
    small = _run(case, "small", settle=1, no_rounds=1, arena_chunks=3000)
    assert small[3][1] == roomy[3][1] > 3000  # (the last attempt's figures)
    assert np.array_equal(roomy[0], small[0]) and roomy[1] == small[1] and roomy[2] == small[2]
    _same_as_oracle(case, "small")
