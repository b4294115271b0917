"""The rules of ntedit_amd/host/batch_rules.h, compiled on their own, without a GPU: the --shard partition equals
ntedit_amd.dist.shard_contigs, and the admission rule of the two draft readers (skip, take, close the batch then take)
gives what the two loops it replaced gave -- both applied `total + len + 1 > budget`, `total` counting len + 1 per kept
contig, to a batch that holds a contig already.  The expected values below are worked out by hand from those loops."""
import os
import subprocess

import pytest

import helpers as H

HOST = os.path.join(H.ROOT, "ntedit_amd", "host")

DRIVER = r"""#include "batch_rules.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace nte_cli;
// shard N len...                         -> a line per share: the ordinals it holds
// admit MIN BUDGET CAP MINE|- len...     -> a line per contig offered, then "seen bases"
int main(int argc, char** argv) {
    if (strcmp(argv[1], "shard") == 0) {
        const unsigned n = (unsigned)strtoul(argv[2], nullptr, 10);
        std::vector<uint64_t> lens;
        for (int i = 3; i < argc; i++) lens.push_back(strtoull(argv[i], nullptr, 10));
        for (unsigned s = 0; s < n; s++) {
            const std::vector<uint8_t> mine = shard_partition(lens, n, s);
            if (mine.size() != lens.size()) return 1;
            for (size_t i = 0; i < mine.size(); i++) if (mine[i]) printf("%zu ", i);
            printf("\n");
        }
        return 0;
    }
    std::vector<uint8_t> mine;
    for (const char* m = argv[5]; *m && *m != '-'; m++) mine.push_back(*m == '1');
    Admission adm(strtoull(argv[2], nullptr, 10), argv[5][0] == '-' ? nullptr : &mine, strtoull(argv[3], nullptr, 10),
                  strtoull(argv[4], nullptr, 10));
    for (int i = 6; i < argc; i++) {
        const Admission::Verdict v = adm.offer(strtoull(argv[i], nullptr, 10));
        if (v == Admission::SKIP) printf("skip\n");
        else if (v == Admission::TOO_LONG) printf("too long\n");
        else printf("%s %llu %llu %llu\n", v == Admission::TAKE ? "take" : "close", (unsigned long long)adm.ordinal(),
                    (unsigned long long)adm.offset(), (unsigned long long)adm.budget());
    }
    printf("%llu %llu\n", (unsigned long long)adm.seen(), (unsigned long long)adm.bases());
}
"""


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_rules")
    src, exe = d / "t.cpp", d / "t"
    src.write_text(DRIVER)
    subprocess.run(["c++", "-std=c++17", "-Wall", "-I", HOST, "-o", str(exe), str(src)], check=True)

    def run(*args):
        return subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout.splitlines()
    return run


LENGTHS = {
    "ties": [500, 300, 500, 300, 300, 500, 100, 100],
    "all equal": [250] * 7,
    "fewer contigs than shards": [900, 100],
    "one contig": [12345],
    "mixed": [10, 4000, 35, 35, 2200, 1, 999, 1000, 1001, 4000, 7, 512],
    "a large one and many small": [10 ** 9] + [1000] * 11,
}


@pytest.mark.parametrize("name", list(LENGTHS))
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_the_shard_partition_is_the_python_partition(rules, name, n):
    from ntedit_amd.dist import shard_contigs
    lens = LENGTHS[name]
    got = [[int(x) for x in line.split()] for line in rules("shard", n, *lens)]
    assert got == [[int(i) for i in part] for part in shard_contigs(lens, n)]
    assert sorted(i for part in got for i in part) == list(range(len(lens)))


def _admit(rules, min_len, budget, cap, mine, lens):
    out = rules("admit", min_len, budget, cap, mine, *lens)
    return out[:-1], [int(x) for x in out[-1].split()]


def test_a_batch_is_cut_where_the_next_contig_would_pass_the_budget(rules):
    """--batch-bases 1000 (budget = cap: it does not move), -z 100"""
    got, (seen, bases) = _admit(rules, 100, 1000, 1000, "-", [2000, 499, 499, 1, 500, 498, 100])
    assert got == [
        "take 0 0 1000",     # larger than the budget, but the first of its batch: taken alone, no batch is ever empty
        "close 1 0 1000",    # 2001 + 499 + 1 > 1000
        "take 2 500 1000",   # 500 + 499 + 1 = 1000: an exact fit stays in the batch
        "skip",              # below -z: neither the ordinal nor the batch moves
        "close 3 0 1000",    # 1000 + 500 + 1: one byte over closes the batch
        "take 4 501 1000",   # 501 + 498 + 1 = 1000
        "close 5 0 1000",
    ]
    assert (seen, bases) == (7, 2000 + 499 + 499 + 500 + 498 + 100)


def test_a_contig_of_another_shard_advances_the_ordinal_only(rules):
    got, (seen, bases) = _admit(rules, 100, 1000, 1000, "0101", [200, 300, 50, 400, 500, 100])
    assert got == [
        "skip",              # ordinal 0: another shard's
        "take 1 0 1000",
        "skip",              # below -z: no ordinal
        "skip",              # ordinal 2: another shard's
        "take 3 301 1000",   # the batch held 300 + 1 bytes: the contigs skipped took no room
        "skip",              # ordinal 4: past the partition, nobody's
    ]
    assert (seen, bases) == (6, 800)


def test_a_contig_above_the_2_32_limit_is_an_error_where_the_run_would_take_it(rules):
    got, _ = _admit(rules, 100, 1 << 30, 1 << 30, "-", [0xFFFFFFF0, 0xFFFFFFF1])
    assert got == ["take 0 0 %d" % (1 << 30), "too long"]
    got, _ = _admit(rules, 100, 1 << 30, 1 << 30, "01", [0xFFFFFFF1, 0xFFFFFFF1])
    assert got == ["skip", "too long"]  # (another shard's: skipped, as the readers did)


def test_the_budget_doubles_from_2_27_and_stops_at_the_cap(rules):
    """contigs of 2^27 bases (2^27 + 1 bytes each): batches of 1, 1, 3, 7, 7, ... contigs"""
    M = 1 << 27
    got, (seen, bases) = _admit(rules, 100, M, 1 << 30, "-", [M] * 21)
    step = M + 1
    want = ["take 0 0 %d" % M, "close 1 0 %d" % (2 * M), "close 2 0 %d" % (4 * M), "take 3 %d %d" % (step, 4 * M),
            "take 4 %d %d" % (2 * step, 4 * M), "close 5 0 %d" % (8 * M)]
    want += ["take %d %d %d" % (5 + i, i * step, 8 * M) for i in range(1, 7)]
    want += ["close 12 0 %d" % (8 * M)] + ["take %d %d %d" % (12 + i, i * step, 8 * M) for i in range(1, 7)]
    want += ["close 19 0 %d" % (8 * M), "take 20 %d %d" % (step, 8 * M)]
    assert got == want
    assert (seen, bases) == (21, 21 * M)
