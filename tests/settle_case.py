"""Shared by test_settle_cpu.py and test_gpu_settle.py: the stand-alone host program tests/settle/settle_host.cpp
(settle_event() against the event machine) and the batch both tiers look at.  Test infrastructure only."""
import os
import re
import subprocess

import numpy as np

import helpers as H

SETTLE_DIR = os.path.join(H.ROOT, "tests", "settle")
_SRC = [os.path.join(SETTLE_DIR, "settle_host.cpp"), os.path.join(H.ROOT, "ntedit_amd", "host", "params.cpp")]


def build_settle_host(out_dir, sanitize=False):
    """g++ build of the host program; returns its path"""
    exe = os.path.join(out_dir, "settle_host_san" if sanitize else "settle_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", exe] + _SRC, check=True)
    return exe


def tally(text):
    """(events, settled, mismatches) of the program's last line"""
    m = re.search(r"^events (\d+) settled (\d+) mismatches (\d+)\s*$", text.strip().splitlines()[-1])
    assert m, text[-400:]
    return int(m.group(1)), int(m.group(2)), int(m.group(3))


def make_settle_case(tmp, seed=20261, n=2_000_000, k=25, hashes=3, bfbytes=16 << 20):
    """The i.i.d. case (n bases, 0.5 % substitutions, 0.05 % indels) and planted contigs -- two substitutions at every
    distance, one at every distance from a contig's end and start, a lower-case error base, N / IUPAC codes at every
    window offset, decoy candidates, one missing k-mer -- in one draft, with one filter of bfbytes bytes.
    Returns dict(draft, bf)."""
    os.makedirs(tmp, exist_ok=True)
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    truth = H.random_genome(rng, n)
    # the filter's text: the truth, and what the planted cases add to it or leave out of it
    texts = [(b"truth", truth)]
    # i.i.d. draft, vectorised (helpers.mutate walks base by base): substitutions in place, then indels from the back
    d = np.frombuffer(truth, dtype=np.uint8).copy()
    sub = np.flatnonzero(rng.random(n) < 5e-3)
    d[sub] = acgt[(np.searchsorted(acgt, d[sub]) + rng.integers(1, 4, size=sub.size)) % 4]
    d = bytearray(d.tobytes())
    for q in sorted((int(x) for x in np.flatnonzero(rng.random(n) < 5e-4)), reverse=True):
        L = int(rng.integers(1, 4))
        if rng.random() < 0.5:
            del d[q:q + L]
        else:
            d[q:q] = H.random_genome(rng, L)
    draft = [(b"iid", bytes(d))]

    def piece(L):
        st = int(rng.integers(0, n - L))
        return bytearray(truth[st:st + L])

    def sub_at(c, q):
        c[q] = b"ACGT"[(b"ACGT".index(bytes([c[q] & 0xDF])) + 1 + int(rng.integers(0, 3))) % 4]

    planted = []
    for dist in range(1, 2 * k + 3):  # two substitutions
        c = piece(8 * k)
        sub_at(c, 3 * k)
        sub_at(c, 3 * k + dist)
        planted.append(c)
    for dist in range(0, 2 * k + 5 + 11):  # contig ends and starts, contigs of 2k .. 4k bases
        for L in range(2 * k, 4 * k + 1, k // 2):
            if dist >= L:
                continue
            a, b = piece(L), piece(L)
            sub_at(a, L - 1 - dist)
            sub_at(b, dist)
            planted += [a, b]
    c = piece(8 * k)  # a lower-case error base
    sub_at(c, 4 * k)
    c[4 * k] |= 0x20
    planted.append(c)
    for o in range(0, 2 * k + 4):  # N and IUPAC codes at every window offset
        for odd in (b"N", b"RYSWKMBDHV"):
            c = piece(8 * k)
            s = 4 * k
            sub_at(c, s)
            c[s - (k - 1) + o] = odd[int(rng.integers(0, len(odd)))]
            planted.append(c)
    # decoys: their own k-mer only / fully supported; every draft base, every true base and each of the two bases left
    # as the decoy, a contig each: in candidate order the decoy stands in front of the true base in half of them and
    # behind it in the other half
    for variant in (0, 1):
        for draft_base in b"ACGT":
            for good in b"ACGT":
                if good == draft_base:
                    continue
                for decoy in b"ACGT":
                    if decoy in (good, draft_base):
                        continue
                    s = 4 * k
                    c = piece(8 * k)
                    while c[s] != good:
                        c = piece(8 * k)
                    c[s] = draft_base
                    dk = bytearray(c[s - (k - 1):s + (k if variant else 1)])
                    dk[k - 1] = decoy
                    texts.append((b"decoy%d" % len(texts), bytes(dk)))
                    planted.append(c)
    # one missing k-mer: a truth of its own, in the filter as two pieces that leave the k-mer at start + i out
    for i in range(1, k + 1):
        tr = bytearray(H.random_genome(rng, 8 * k))
        c = bytearray(tr)
        s = 4 * k
        start = s - (k - 1)
        sub_at(c, s)
        texts.append((b"m%da" % i, bytes(tr[:start + i + k - 1])))
        texts.append((b"m%db" % i, bytes(tr[start + i + 1:])))
        planted.append(c)
    draft += [(b"p%d" % i, bytes(c)) for i, c in enumerate(planted)]
    H.write_fasta(os.path.join(tmp, "truth.fa"), texts)
    H.mkbf([os.path.join(tmp, "truth.fa")], os.path.join(tmp, "t.bf"), k=k, hashes=hashes, nbytes=bfbytes)
    H.write_fasta(os.path.join(tmp, "draft.fa"), draft, width=0)
    return {"draft": os.path.join(tmp, "draft.fa"), "bf": os.path.join(tmp, "t.bf")}
