"""Records what `ntedit` answers to command lines that end before the device is opened: exit status, stdout and stderr of
each case of CASES, into tests/golden/cli_transcripts.json.  tests/test_cli_transcripts_cpu.py replays the list against the
built binary and compares all three, whole.  The expected values are a known-good build's (the commit before the command
line was split into units): record from such a build only, never to make a failing case pass.

    python tests/tools/record_cli_transcripts.py <path to ntedit> [--check]

Runs nothing on a GPU: a case that got as far as `no usable HIP device' is refused by the recorder."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cli_transcripts.json")
DATE = r"[A-Z][a-z]{2} [A-Z][a-z]{2} [ \d]\d \d\d:\d\d:\d\d \d{4}"  # (ctime; tests/test_gpu_reads_cascade.py)

F = ["-f", "d.fa"]
FR = F + ["-r", "f.bf"]
READS = F + ["--reads", "r.fq", "--cutoff", "2", "--bf", "4096"]
RK = READS + ["-k", "25"]
LIST = READS + ["-b", "p"]
GENOME = F + ["--genome", "g.fa"]
GK = GENOME + ["-k", "25"]

CASES = {
    # usage and version
    "help": ["--help"],
    "version": ["--version"],
    "help after good options": FR + ["--help"],
    "help before a malformed option": ["--help", "-t", "x"],
    "a malformed option before help": ["-t", "x", "--help"],
    # getopt's own refusals, and what is missing
    "no arguments": [],
    "an unknown option": FR + ["--nonsense"],
    "an option without its argument": FR + ["-z"],
    "no -f": ["-r", "f.bf"],
    "no -r": F,
    "an unreadable -f": ["-f", "missing.fa", "-r", "f.bf"],
    "an unreadable -r": ["-f", "d.fa", "-r", "missing.bf"],
    "an unreadable -e": FR + ["-e", "missing_e.bf"],
    "an unreadable -f and an unreadable -r": ["-f", "missing.fa", "-r", "missing.bf"],
    "an unreadable -r and an unreadable -f": ["-r", "missing.bf", "-f", "missing.fa"],
    "no -f and an unreadable -r": ["-r", "missing.bf"],
    "an unknown option and an unreadable -r": ["--nonsense", "-f", "d.fa", "-r", "missing.bf"],
    # a malformed value at each short option
    **{"malformed -%s" % c: FR + ["-" + c, "1x"] for c in "tzdixyXYcjmsavpq"},
    **{"malformed -%s" % c: ["-" + c, "two words"] for c in "fbrel"},
    "malformed --gpu": FR + ["--gpu", "x"],
    "malformed --batch-bases": FR + ["--batch-bases", "1e6"],
    "malformed --start-grid": FR + ["--start-grid", "x"],
    "malformed --event-budget": FR + ["--event-budget", "x"],
    "two malformed options": FR + ["-t", "x", "-z", "y"],
    "two malformed options, the other way round": FR + ["-z", "y", "-t", "x"],
    # --shard and --tune forms
    "--shard without a slash": FR + ["--shard", "1"],
    "--shard 2/2": FR + ["--shard", "2/2"],
    "--shard 0/0": FR + ["--shard", "0/0"],
    "--shard x/2": FR + ["--shard", "x/2"],
    "--tune without =": FR + ["--tune", "knob"],
    "--tune without a key": FR + ["--tune", "=3"],
    "--tune without a value": FR + ["--tune", "knob="],
    "--tune with a trailing letter": FR + ["--tune", "knob=3x"],
    "--tune with a negative value": FR + ["--tune", "knob=-1"],
    "a malformed --tune before a malformed --shard": FR + ["--tune", "knob", "--shard", "2/2"],
    "a malformed --shard before a malformed --tune": FR + ["--shard", "2/2", "--tune", "knob"],
    # --completeness, --qv, --shard
    "--completeness without --qv": FR + ["--completeness"],
    "--completeness and --shard": FR + ["--qv", "--completeness", "--shard", "0/2"],
    "--shard and --completeness": FR + ["--shard", "0/2", "--completeness", "--qv"],
    "--completeness and --counts": RK + ["--qv", "--completeness", "--counts"],
    "--completeness without --qv, with --shard and --counts": FR + ["--completeness", "--shard", "0/2", "--counts"],
    "--qv and --shard": FR + ["--qv", "--shard", "0/2"],
    "--completeness and an unreadable -f": ["-f", "missing.fa", "-r", "f.bf", "--completeness"],
    "--completeness and no -f": ["-r", "f.bf", "--completeness"],
    "--qv, --shard and a list of k": LIST + ["-k", "40,30", "--qv", "--shard", "0/2"],
    # a reads option without --reads, in both wordings; the first one given is named
    "--cutoff without --reads": FR + ["--cutoff", "2"],
    "--hashes without --reads": FR + ["--hashes", "3"],
    "--gpu_parse without --reads": FR + ["--gpu_parse"],
    "--solid then --bf without --reads": F + ["--solid", "--bf", "4096"],
    "--bf then --solid without --reads": F + ["--bf", "4096", "--solid"],
    "--save_reject_bf without --reads and without -r": F + ["--save_reject_bf", "x.bf"],
    # the reads options that are refused at the option
    "malformed --cutoff": RK + ["--cutoff", "x"],
    "malformed --hashes without --reads": FR + ["--hashes", "x"],
    "malformed --bf": F + ["--reads", "r.fq", "--cutoff", "2", "--bf", "4k", "-k", "25"],
    "malformed --num_elements": RK + ["--num_elements", "-5"],
    "malformed --sketch_bytes": RK + ["--sketch_bytes", "+5"],
    "malformed --batch_bytes": RK + ["--batch_bytes", ""],
    "malformed --resident_cap": RK + ["--resident_cap", "1.5"],
    "malformed --reject_cutoff": RK + ["--reject_cutoff", "x"],
    "malformed --reject_bf": RK + ["--reject_bf", "x"],
    "malformed --reject_num_elements": RK + ["--reject_num_elements", "x"],
    "--fpr out of range": RK + ["--fpr", "2"],
    "--fpr not a number, without --reads": FR + ["--fpr", "x"],
    "a malformed --cutoff before a malformed -t": RK + ["--cutoff", "x", "-t", "y"],
    "a malformed -t before a malformed --cutoff": RK + ["-t", "y", "--cutoff", "x"],
    "a malformed --cutoff before help": ["--cutoff", "x", "--help"],
    "--fpr out of range and an unreadable -f": ["-f", "missing.fa", "--fpr", "2"],
    # every other refusal of --reads
    "--reads and -r": RK + ["-r", "f.bf"],
    "--reads without files": F + ["--reads", "--cutoff", "2", "--bf", "4096", "-k", "25"],
    "--reads and --shard": RK + ["--shard", "0/2"],
    "--reads, -r and --shard": RK + ["--shard", "0/2", "-r", "f.bf"],
    "--reject_cutoff and -e": RK + ["--reject_cutoff", "9", "--reject_bf", "4096", "-e", "f.bf"],
    "--reads without -k": READS,
    "--reads -k 11": READS + ["-k", "11"],
    "--reads -k x": READS + ["-k", "x"],
    "--cutoff and --solid": RK + ["--solid"],
    "neither --cutoff nor --solid": F + ["--reads", "r.fq", "--bf", "4096", "-k", "25"],
    "--cutoff 0": F + ["--reads", "r.fq", "--cutoff", "0", "--bf", "4096", "-k", "25"],
    "--cutoff 256": F + ["--reads", "r.fq", "--cutoff", "256", "--bf", "4096", "-k", "25"],
    "--hashes 9 with --reads": RK + ["--hashes", "9"],
    "no size for the filter": F + ["--reads", "r.fq", "--cutoff", "2", "-k", "25"],
    "--bf 0": F + ["--reads", "r.fq", "--cutoff", "2", "--bf", "0", "-k", "25"],
    "--num_elements 0": F + ["--reads", "r.fq", "--cutoff", "2", "--num_elements", "0", "-k", "25"],
    "--batch_bytes 100": RK + ["--batch_bytes", "100"],
    "--reject_bf without --reject_cutoff": RK + ["--reject_bf", "4096"],
    "--reject_num_elements without --reject_cutoff": RK + ["--reject_num_elements", "100"],
    "--save_reject_bf without --reject_cutoff": RK + ["--save_reject_bf", "x.bf"],
    "--reject_cutoff 1": RK + ["--reject_cutoff", "1", "--reject_bf", "4096"],
    "--reject_cutoff and --counts": RK + ["--reject_cutoff", "9", "--reject_bf", "4096", "--counts"],
    "--reject_cutoff not above --cutoff": RK + ["--reject_cutoff", "2", "--reject_bf", "4096"],
    "--reject_bf and --reject_num_elements": RK + ["--reject_cutoff", "9", "--reject_bf", "4096", "--reject_num_elements", "100"],
    "no size for the reject filter": RK + ["--reject_cutoff", "9"],
    "--reject_bf 0": RK + ["--reject_cutoff", "9", "--reject_bf", "0"],
    "an unreadable reads file": F + ["--reads", "r.fq", "missing.fq", "--cutoff", "2", "--bf", "4096", "-k", "25"],
    "an unreadable reads file and an unreadable -f": ["-f", "missing.fa", "--reads", "missing.fq", "--cutoff", "2", "--bf", "4096",
                                                      "-k", "25"],
    "an unreadable reads file and a bad -k": F + ["--reads", "missing.fq", "--cutoff", "2", "--bf", "4096", "-k", "11"],
    "an unreadable -e with --reads": RK + ["-e", "missing_e.bf"],
    # every branch of the rules of a list of k
    "a list of k with -r": FR + ["-k", "40,30", "-b", "p"],
    "a list of k with --genome": GENOME + ["-k", "40,30", "-b", "p"],
    "a list of k with --shard": LIST + ["-k", "40,30", "--shard", "0/2"],
    "a list of k without -b": READS + ["-k", "40,30"],
    "a list of k: not a number": LIST + ["-k", "40,x"],
    "a list of k: an empty k": LIST + ["-k", "40,,30"],
    "a list of k: a trailing comma": LIST + ["-k", "40,"],
    "a list of k: k below 12": LIST + ["-k", "40,11"],
    "a list of k: k above 200": LIST + ["-k", "201,40"],
    "a list of k: nine k": LIST + ["-k", "12,13,14,15,16,17,18,19,20"],
    "a list of k: a k twice": LIST + ["-k", "40,30,40"],
    "a list of k: --save_bf without {k}": LIST + ["-k", "40,30", "--save_bf", "f_k.bf"],
    "a list of k: --save_reject_bf without {k}": LIST + ["-k", "40,30", "--reject_cutoff", "9", "--reject_bf", "4096", "--save_bf",
                                                         "f_{k}.bf", "--save_reject_bf", "rej.bf"],
    "a list of k: --hist without {k}": LIST + ["-k", "40,30", "--hist", "h.hist"],
    "a list of k: a rule of one round": F + ["--reads", "r.fq", "--cutoff", "2", "-k", "40,30", "-b", "p"],
    "a list of k without -b and with -r": READS + ["-k", "40,30", "-r", "f.bf"],
    # every branch of the rules of --genome
    "--genome and -r": GK + ["-r", "f.bf"],
    "--genome and --reads": GK + ["--reads", "r.fq"],
    "--reads and --genome": F + ["--reads", "r.fq", "--genome", "g.fa", "-k", "25"],
    "--genome and --shard": GK + ["--shard", "0/2"],
    "--genome without files": F + ["--genome", "-k", "25"],
    "--genome and --cutoff": GK + ["--cutoff", "2"],
    "--genome and --solid after --bf": GK + ["--bf", "4096", "--solid"],
    "--genome and --resident_cap": GK + ["--resident_cap", "0"],
    "--genome without -k": GENOME,
    "--genome -k x": GENOME + ["-k", "x"],
    "--genome -k 11": GENOME + ["-k", "11"],
    "--genome -k 201": GENOME + ["-k", "201"],
    "--genome -k -25": GENOME + ["-k", "-25"],
    "--genome with an empty -k": GENOME + ["-k", ""],
    "--genome --hashes 0": GK + ["--hashes", "0"],
    "--genome --hashes 9": GK + ["--hashes", "9"],
    "--genome --bf 0": GK + ["--bf", "0"],
    "--genome --num_elements 0": GK + ["--num_elements", "0"],
    "--genome --batch_bytes 0": GK + ["--batch_bytes", "0"],
    "--genome with an unreadable file": F + ["--genome", "g.fa", "missing_g.fa", "-k", "25"],
    "--genome without -k and with an unreadable file": F + ["--genome", "missing_g.fa"],
    "--genome, -r, --shard and no -k": GENOME + ["-r", "f.bf", "--shard", "0/2"],
    "--genome and an unreadable -e": GK + ["-e", "missing_e.bf"],
}


def make_inputs(where):
    """the files the cases name, in the directory they run in (the names are relative: the texts hold no path)"""
    with open(os.path.join(where, "d.fa"), "w") as f:
        f.write(">c\n" + "ACGTTGCAAC" * 20 + "\n")
    with open(os.path.join(where, "g.fa"), "w") as f:
        f.write(">g\n" + "ACGTTGCAAC" * 20 + "\n")
    with open(os.path.join(where, "r.fq"), "w") as f:
        f.write("@r1\n" + "ACGTACGTAC" * 5 + "\n+\n" + "I" * 50 + "\n")
    with open(os.path.join(where, "f.bf"), "w") as f:
        f.write("not a filter\n")


def transcript(binary, args, where):
    """exit status, stdout and stderr of one case, the date masked (argv[0] is fixed: getopt's own lines name it)"""
    before = sorted(os.listdir(where))
    r = subprocess.run(["ntedit"] + args, executable=binary, capture_output=True, timeout=60, cwd=where)
    assert sorted(os.listdir(where)) == before, "the case wrote a file"
    text = [re.sub(DATE, "<date>", t.decode("latin-1")) for t in (r.stdout, r.stderr)]
    return {"status": r.returncode, "stdout": text[0], "stderr": text[1]}


def record(binary):
    out = []
    with tempfile.TemporaryDirectory() as where:
        make_inputs(where)
        for name, args in CASES.items():
            t = transcript(os.path.abspath(binary), args, where)
            if "no usable HIP device" in t["stderr"] or t["status"] < 0:
                sys.exit("case `%s' does not end before the device is opened: %r" % (name, t))
            out.append(dict(name=name, args=args, **t))
    return out


if __name__ == "__main__":
    got = record(sys.argv[1])
    if "--check" in sys.argv[2:]:
        want = json.load(open(GOLDEN))["cases"]
        bad = [g["name"] for g, w in zip(got, want) if g != w]
        sys.exit("differs: %s" % bad if bad or len(got) != len(want) else 0)
    with open(GOLDEN, "w") as f:
        json.dump({"about": "exit status, stdout and stderr of ntedit for command lines that end before the device is opened; "
                            "written by tests/tools/record_cli_transcripts.py", "cases": got}, f, indent=1)
        f.write("\n")
    print("%d cases -> %s" % (len(got), GOLDEN))
