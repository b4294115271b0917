"""The stages of the `ntedit` binary fit together: a small draft cut into several batches passes the reader, the GPU and
the writer, once on the mapped reader and once on the streaming one, with --qv, --completeness and --report on."""
import filecmp
import json
import os
import re
import subprocess

import pytest

import helpers as H

DATE = r"[A-Z][a-z]{2} [A-Z][a-z]{2} [ \d]\d \d\d:\d\d:\d\d \d{4}"
# the keys of the three --report lines, in the order the program prints them
COMPLETENESS_KEYS = ["filter_bits", "filter_set", "filter_kmers", "shared_set_before", "shared_kmers_before", "shared_set_after",
                     "shared_kmers_after", "completeness_before", "completeness_after", "ms_mark"]
QV_KEYS = ["kmers_before", "absent_before", "kmers_after", "absent_after", "apply_ms", "screen_ms", "count_ms"]
ROUND_KEYS = ["bases", "seconds", "open_outputs_s", "index_s", "read_s", "polish_call_s", "write_s", "gpu_ms", "screen_ms",
              "machine_ms", "screening", "events", "events_applied", "absent_kmers", "substitutions", "insertions", "deletions"]
SCREENING_KEYS = ["batches_partitioned", "batches_direct_kernel", "record_chunks_rescreened_direct", "overflow_records"]
TIMES = re.compile(r"(_s|_ms|^seconds|^ms_mark)$")


def _without_times(d):
    return {k: (_without_times(v) if isinstance(v, dict) else v) for k, v in d.items() if not TIMES.search(k)}


@pytest.mark.gpu
def test_several_batches_pass_all_three_stages_on_both_readers(tmp_path, oracle_build):
    cli = os.path.join(H.ROOT, "ntedit_amd", "ntedit")
    case = H.make_case(str(tmp_path), 424242, n=40000, contigs=3, flavor="N lower")
    H.run_oracle(case["draft"], case["bf"], H.default_params(), str(tmp_path / "o"))
    runs = {}
    for tag, extra in (("m", []), ("s", ["--no-map"])):
        os.makedirs(str(tmp_path / tag))
        r = subprocess.run([cli, "-f", case["draft"], "-r", case["bf"], "-b", "p", "--qv", "--completeness", "--report",
                            "--batch-bases", "15000"] + extra, capture_output=True, text=True, cwd=str(tmp_path / tag))
        assert r.returncode == 0, r.stderr
        for suf in ("_edited.fa", "_changes.tsv"):
            assert filecmp.cmp(str(tmp_path / ("o" + suf)), str(tmp_path / tag / ("p" + suf)), shallow=False), (tag, suf)
        lines = r.stdout.splitlines()
        reports = [json.loads(l) for l in lines if l.startswith("{")]
        assert len(reports) == 3 and [l.startswith("{") for l in lines[-3:]] == [True] * 3
        assert list(reports[0]) == ["completeness"] and list(reports[0]["completeness"]) == COMPLETENESS_KEYS
        assert list(reports[1]) == ["qv"] and list(reports[1]["qv"]) == QV_KEYS
        assert list(reports[2]) == ROUND_KEYS and list(reports[2]["screening"]) == SCREENING_KEYS
        kept = [len(s) for _, s in H.read_fasta(case["draft"]) if len(s) >= 100]
        assert len(kept) == 3 and reports[2]["bases"] == sum(kept)
        # (a batch holds 15000 bytes or one contig: every contig of 40,000 bases went through the stages in a batch of its own)
        assert reports[2]["screening"]["batches_partitioned"] + reports[2]["screening"]["batches_direct_kernel"] == 3
        text = re.sub(DATE, "<date>", "\n".join(l for l in lines if not l.startswith("{")))
        runs[tag] = (text, [_without_times(x) for x in reports], r.stderr)
    assert runs["m"] == runs["s"]
    names = sorted(os.listdir(str(tmp_path / "m")))
    assert names == sorted(os.listdir(str(tmp_path / "s"))) and len(names) == 5
    for name in names:
        a, b = (open(str(tmp_path / t / name), "rb").read() for t in ("m", "s"))
        if name.endswith(".vcf"):
            a, b = (re.sub(rb"##fileDate=\d{8}", b"", x) for x in (a, b))
        assert a == b, name
