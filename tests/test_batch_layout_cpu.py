"""The layout rule of ntedit_amd/host/batch_layout.h, compiled on its own with the sanitizers, without a GPU: the index of the
first entry that breaks the layout of a batch of n bytes, with the separator rule (the polish) and without it (the interval
extractor, the spectrum, the draft store).  The driver also evaluates the expression that stood in front of the polish
before the rule was shared, `offs + len > n || (.. && offs + len >= next)`: an offset near 2^64 wraps in it and passes."""
import os
import subprocess

import pytest

import helpers as H

HOST = os.path.join(H.ROOT, "ntedit_amd", "host")
OK = "ok"

DRIVER = r"""#include "batch_layout.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
// SEPARATED N off:len...  ->  "ok" or the first breaking index, then the same from the polish's earlier expression
static unsigned long old_polish_rule(uint64_t n, const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& lens) {
    const uint32_t n_contigs = (uint32_t)offsets.size();
    for (uint32_t i = 0; i < n_contigs; i++) {
        if (offsets[i] + lens[i] > n || (i + 1 < n_contigs && offsets[i] + lens[i] >= offsets[i + 1])) return i;
    }
    return nte_host::LAYOUT_OK;
}
static void show(unsigned long v) {
    if (v == nte_host::LAYOUT_OK) printf("ok\n");
    else printf("%lu\n", v);
}
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const bool separated = atoi(argv[1]) != 0;
    const uint64_t n = strtoull(argv[2], nullptr, 10);
    std::vector<uint64_t> offs;
    std::vector<uint32_t> lens;
    for (int i = 3; i < argc; i++) {
        char* colon = nullptr;
        offs.push_back(strtoull(argv[i], &colon, 10));
        lens.push_back((uint32_t)strtoull(colon + 1, nullptr, 10));
    }
    show(nte_host::first_layout_break(n, offs.data(), lens.data(), (uint32_t)offs.size(), separated));
    show(old_polish_rule(n, offs, lens));
}
"""


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_layout")
    src, exe = d / "t.cpp", d / "t"
    src.write_text(DRIVER)
    subprocess.run(["c++", "-std=c++17", "-Wall", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-I", HOST, "-o", str(exe), str(src)],
                   check=True)

    def run(separated, n, *entries):
        """(the rule's answer, the earlier polish expression's): "ok" or an index"""
        args = [str(exe), str(int(separated)), str(n)] + ["%d:%d" % e for e in entries]
        out = subprocess.run(args, capture_output=True, text=True, check=True).stdout.split()
        return [OK if x == OK else int(x) for x in out]
    return run


BOTH = pytest.mark.parametrize("separated", [False, True], ids=["abutting", "separated"])


@BOTH
def test_an_empty_batch(layout, separated):
    assert layout(separated, 0)[0] == OK
    assert layout(separated, 1000)[0] == OK


@BOTH
def test_one_entry_filling_the_batch(layout, separated):
    assert layout(separated, 1000, (0, 1000))[0] == OK


def test_abutting_entries_need_the_separator_rule_off(layout):
    entries = [(0, 100), (101, 200), (301, 50), (352, 10)]  # entry 1 ends where entry 2 begins
    assert layout(False, 400, *entries)[0] == OK
    assert layout(True, 400, *entries) == [1, 1]  # (the polish refused it before, at the same index)
    apart = [(0, 100), (101, 199), (301, 50), (352, 10)]
    assert layout(True, 400, *apart) == [OK, OK]


@BOTH
def test_an_entry_ending_one_byte_past_n(layout, separated):
    assert layout(separated, 400, (0, 100), (101, 300))[0] == 1
    assert layout(separated, 400, (0, 100), (101, 299))[0] == OK


@BOTH
def test_entries_out_of_order(layout, separated):
    assert layout(separated, 400, (200, 100), (0, 100))[0] == 0
    assert layout(separated, 400, (0, 100), (150, 100), (120, 10))[0] == 1  # (entry 2 lies inside entry 1)


@BOTH
def test_an_offset_that_wraps_is_refused(layout, separated):
    """offs = 2^64 - 1, len = 2: offs + len is 1.  The rule refuses the entry; the polish's earlier expression let it pass."""
    got, old = layout(separated, 1000, ((1 << 64) - 1, 2))
    assert got == 0 and old == OK
    got, old = layout(separated, 1000, (0, 100), ((1 << 64) - 1, 2))
    assert got == 1 and old == OK
    # ... and as an entry in front of another one: the wrapped end, 1, lies below the next offset
    got, old = layout(separated, 1000, ((1 << 64) - 1, 2), (500, 100))
    assert got == 0 and old == OK


@BOTH
def test_an_empty_entry_at_the_end(layout, separated):
    """offs = n, len = 0: inside the batch"""
    assert layout(separated, 400, (400, 0))[0] == OK
    assert layout(separated, 400, (0, 399), (400, 0))[0] == OK
    assert layout(separated, 400, (401, 0))[0] == 0


@BOTH
def test_the_longest_length_in_a_small_batch(layout, separated):
    assert layout(separated, 1000, (0, (1 << 32) - 1))[0] == 0
    assert layout(separated, 1000, (0, 10), (11, (1 << 32) - 1))[0] == 1
    assert layout(separated, (1 << 32) - 1, (0, (1 << 32) - 1))[0] == OK
